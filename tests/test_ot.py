"""Optimal-transport alignment without a device: the numpy yardstick of tests/ot_util.py tied to exact results, the C
declarations, the refusals that need no device, the exports and the dispatcher ops' fake functions.

Anchors of the yardstick (what tests/test_ot_gpu.py then holds the kernels to):
(a) pure expression cost (alpha = 0, n = m = 60, uniform marginals, P = 8, Poisson(3) counts): the exact transport cost is
    the assignment optimum / n (tests/golden/reference_ot.npz, scipy's linear_sum_assignment).  The yardstick's <M, T> lies
    in [exact - s, exact + e log n + s] with s = 2 |M|_inf marginal_error: e log n is the entropic bound
    (KL(T* || a x b) <= log min(n, m) for a vertex T*), s what a plan whose marginals are off by marginal_error can gain or
    lose.  Measured with 40 x 50 sweeps, seed 0: relative epsilon 0.1 / 0.01 / 0.001 -> gap 4.3e-2 / 1.5e-3 / 2.0e-6 under
    bounds 0.204 / 0.0204 / 0.00204, row-marginal L1 4e-16 / 3.5e-5 / 1.0e-3.
(b) permutation recovery: slice B is slice A rotated by 0.7 rad, shifted and row-permuted with identical expression, so
    the exact optimum is the permutation with objective 0.  Seeds 0-4, (n, P) in {(40, 10), (150, 20)}, alpha in {0.1, 0.5},
    relative epsilon in {0.05, 0.01, 0.002}, max_iter = 40, sinkhorn_iters = 50: every row's argmax of T is its true
    partner in all 60 cases; the stacked B lands on centred A within 7.8e-3 / 7.9e-4 / 5.2e-4 (max abs, field 10 wide) at
    epsilon 0.05 / 0.01 / 0.002 - asserted: <= 1e-2 at epsilon 0.01, more than ten times the yardstick's own error.  At
    epsilon 0.002 the sweeps have not all converged; marginal_error up to 3e-4 says so.
(c) bookkeeping on the same cases: objective = (1 - alpha) expression_cost + alpha gw_cost, gw_cost equals the four-index
    sum written out, stack_slices' outputs equal (X_k - t_k) R_k^T with orthogonal R_k.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import ot_util as U
import spatial_alignment_amd as pkg
from spatial_alignment_amd import _lib, ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_ot.npz")
PERM_CASES = [(seed, n, P, alpha, eps) for seed in range(5) for (n, P) in ((40, 10), (150, 20)) for alpha in (0.1, 0.5)
              for eps in (0.05, 0.01, 0.002)]
NAMES = ("gpsa_ot_dist_f64", "gpsa_ot_sqmatvec_f64", "gpsa_ot_expr_rows_workspace", "gpsa_ot_expr_rows_f32",
         "gpsa_ot_expr_cost_f64", "gpsa_ot_cost_workspace", "gpsa_ot_cost_f64", "gpsa_ot_sinkhorn_workspace",
         "gpsa_ot_sinkhorn_f64", "gpsa_ot_plan_workspace", "gpsa_ot_plan_f64")


# ------------------------------------------------------------------------------------------------------------------------
# (a) the pure expression cost against the assignment optimum
# ------------------------------------------------------------------------------------------------------------------------
def test_golden_holds_seeds_and_scalars_only():
    g = np.load(GOLDEN)
    assert sorted(g.files) == ["P", "exact", "m_inf", "n", "seeds"]
    assert int(g["n"]) == 60 and int(g["P"]) == 8 and list(g["seeds"]) == [0, 1, 2]
    assert os.path.getsize(GOLDEN) < 4096


@pytest.mark.parametrize("epsilon", [0.1, 0.01, 0.001])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_expression_cost_stays_inside_the_entropic_bound(k, epsilon):
    g = np.load(GOLDEN)
    seed, n, exact = int(g["seeds"][k]), int(g["n"]), float(g["exact"][k])
    XA, YA, XB, YB = U.assignment_case(seed, n, int(g["P"]))
    M = U.expr_cost(YA, YB, "kl")
    assert abs(np.abs(M).max() - float(g["m_inf"][k])) < 1e-12
    r = U.solve(U.dist(XA), U.dist(XB), M, alpha=0.0, epsilon=epsilon, max_iter=40, sinkhorn_iters=50)
    s = 2.0 * np.abs(M).max() * r["marginal_error"]
    bound = r["epsilon_used"] * np.log(n)
    gap = r["expression_cost"] - exact
    print(f"seed {seed} epsilon {epsilon}: gap {gap:.3e}, bound {bound:.3e}, marginal error {r['marginal_error']:.1e}")
    assert abs(r["epsilon_used"] - epsilon * np.mean(np.abs(M))) <= 1e-15 * np.mean(np.abs(M))  # alpha = 0: cost_0 = M
    assert -s <= gap <= bound + s
    assert abs(r["objective"] - r["expression_cost"]) == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# (b) permutation recovery, (c) bookkeeping on the same cases
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _perm_result(seed, n, P, alpha, eps):
    XA, YA, XB, YB, perm = U.permutation_case(seed, n, P)
    C1, C2 = U.dist(XA), U.dist(XB)
    r = U.solve(C1, C2, U.expr_cost(YA, YB, "kl"), alpha=alpha, epsilon=eps, max_iter=40, sinkhorn_iters=50)
    return XA, XB, C1, C2, perm, r


@pytest.mark.parametrize("case", PERM_CASES, ids=lambda c: "s%d-n%d-P%d-a%g-e%g" % c)
def test_planted_permutation_is_recovered_and_stacked(case):
    XA, XB, C1, C2, perm, r = _perm_result(*case)
    alpha, eps = case[3], case[4]
    T = r["T"]
    assert np.array_equal(np.argmax(T, axis=1), U.partner(perm))
    (A, B), rots, trans = U.stack_slices([XA, XB], [T])
    err = np.max(np.abs(B - A[perm]))
    print(f"{case}: stacking error {err:.2e}, marginal error {r['marginal_error']:.1e}, objective {r['objective']:.3e}")
    if eps == 0.01:
        assert err <= 1e-2
    # (c) the objective's bookkeeping and the stacking arithmetic
    assert abs(r["objective"] - ((1 - alpha) * r["expression_cost"] + alpha * r["gw_cost"])) <= 1e-15 * abs(r["objective"])
    direct = U.gw_objective_direct(C1, C2, T)
    scale = float(T.sum(1) @ (C1 * C1) @ T.sum(1))
    assert abs(r["gw_cost"] - direct) <= 1e-12 * scale
    assert np.allclose(A, (XA - trans[0]) @ rots[0].T, rtol=0, atol=1e-12)
    assert np.allclose(B, (XB - trans[1]) @ rots[1].T, rtol=0, atol=1e-12)
    assert np.allclose(rots[1] @ rots[1].T, np.eye(2), rtol=0, atol=1e-12)
    assert np.allclose(T.sum(1) @ A, 0.0, atol=1e-12) and np.allclose(T.sum(0) @ B, 0.0, atol=1e-10)


def test_stack_slices_chain_and_reflection_guard():
    """three slices; the third is a MIRROR image, so the unguarded rotation is a reflection (det R = -1) and lands exactly,
    while the guarded one is a proper rotation"""
    rs = np.random.RandomState(5)
    X0 = rs.uniform(0, 10, (30, 2))
    X1 = X0 @ U.rotation(0.4).T + 2.0
    X2 = X0 * np.array([1.0, -1.0]) + 1.0
    T = np.eye(30) / 30
    (A, B, Cc), rots, _ = U.stack_slices([X0, X1, X2], [T, T], reflection=True)
    assert np.allclose(A, B, atol=1e-12) and np.allclose(B, Cc, atol=1e-12)
    assert np.linalg.det(rots[1]) > 0 and np.linalg.det(rots[2]) < 0
    (_, _, Cg), rots_g, _ = U.stack_slices([X0, X1, X2], [T, T], reflection=False)
    assert np.linalg.det(rots_g[2]) > 0 and not np.allclose(Cg, Cc, atol=1e-3)
    # the library's own stack_slices is plain torch off the device: the same numbers
    for refl in (True, False):
        want = U.stack_slices([X0, X1, X2], [T, T], reflection=refl)
        got = pkg.stack_slices([torch.tensor(X0), torch.tensor(X1), torch.tensor(X2)], [torch.tensor(T)] * 2, reflection=refl)
        for k in range(3):
            assert np.allclose(got[0][k].numpy(), want[0][k], atol=1e-12)
            assert np.allclose(got[1][k].numpy(), want[1][k], atol=1e-12)
            assert np.allclose(got[2][k].numpy(), want[2][k], atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI, the refusals, the exports, the fake functions
# ------------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"([a-z ]+?)\b" + name + r"\s*\(([^;]*?)\)\s*;", src)
    assert m, name
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def test_c_declarations_equal_signatures():
    import ctypes as C

    def ctype(arg):
        if "*" in arg:
            return C.c_void_p
        base = arg.rsplit(" ", 1)[0].replace("const ", "").strip() if " " in arg else arg
        return {"int": C.c_int, "long long": C.c_longlong, "double": C.c_double}[base]

    for name in NAMES:
        ret, args = _declaration(name)
        res, argtypes = _lib.SIGNATURES[name]
        assert res is {"int": C.c_int, "long long": C.c_longlong}[ret], name
        assert [ctype(a) for a in args] == list(argtypes), name
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)


def test_workspace_queries_are_pure():
    lib = _lib.load()
    groups = lambda n: -(-n // max(64, -(-n // 128)))
    for n, m in ((1, 1), (64, 65), (65, 64), (130, 257), (10000, 9000), (8193, 3)):
        tc = -(-m // 64)
        assert lib.gpsa_ot_sinkhorn_workspace(n, m) == 16 * groups(n) * m
        assert lib.gpsa_ot_plan_workspace(n, m) == 8 * (n * tc + groups(n) * m + groups(n) * tc)
        assert lib.gpsa_ot_cost_workspace(n, m) == 24 * min(n, 1024)
        assert lib.gpsa_ot_expr_rows_workspace(n) == 8 * n
    assert lib.gpsa_ot_sinkhorn_workspace(0, 5) == 0 and lib.gpsa_ot_plan_workspace(5, 0) == 0
    assert groups(64) == 1 and groups(65) == 2 and groups(8192) == 128 and groups(8193) == 127


def test_entries_refuse_bad_arguments_before_any_launch():
    import ctypes as C

    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    E, Un, W = _lib.GPSA_EINVAL, _lib.GPSA_EUNSUPPORTED, _lib.GPSA_EWORKSPACE
    big = 1 << 31
    assert lib.gpsa_ot_dist_f64(None, 4, 2, p, None) == E
    assert lib.gpsa_ot_dist_f64(p, 0, 2, p, None) == E
    assert lib.gpsa_ot_dist_f64(p, 4, 5, p, None) == Un
    assert lib.gpsa_ot_dist_f64(p, 65535 * 64 + 1, 2, p, None) == Un
    assert lib.gpsa_ot_sqmatvec_f64(p, 4, 0, p, p, None) == E
    assert lib.gpsa_ot_sqmatvec_f64(p, 4, big, p, p, None) == Un
    assert lib.gpsa_ot_expr_rows_f32(2, p, 4, 3, p, p, p, p, p, 1 << 20, None) == E       # unknown mode
    assert lib.gpsa_ot_expr_rows_f32(0, p, 4, 3, p, None, p, p, p, 1 << 20, None) == E    # "kl" needs Lg
    assert lib.gpsa_ot_expr_rows_f32(0, p, 4, 3, p, p, p, p, p, 31, None) == W
    assert lib.gpsa_ot_expr_rows_f32(1, p, 4, 3, p, None, p, p, None, 1 << 20, None) == W
    assert lib.gpsa_ot_expr_cost_f64(1, p, 4, 3, p, None, None) == E                      # "euclidean" needs rb
    assert lib.gpsa_ot_expr_cost_f64(0, p, 0, 3, p, None, None) == E
    a = (p, p, p, p, p, p, p)
    assert lib.gpsa_ot_cost_f64(*a, 1.5, 4, 3, p, p, 1 << 20, None) == E
    assert lib.gpsa_ot_cost_f64(*a, float("nan"), 4, 3, p, p, 1 << 20, None) == E
    assert lib.gpsa_ot_cost_f64(*a, 0.5, 4, 3, None, p, 1 << 20, None) == E
    assert lib.gpsa_ot_cost_f64(*a, 0.5, 4, 3, p, p, 95, None) == W
    assert lib.gpsa_ot_cost_f64(*a, 0.5, big, 3, p, p, 1 << 20, None) == Un
    assert lib.gpsa_ot_sinkhorn_f64(p, 4, 3, p, p, None, p, p, 1, p, 1 << 20, None) == E  # eps is a device pointer
    assert lib.gpsa_ot_sinkhorn_f64(p, 4, 3, p, p, p, p, p, -1, p, 1 << 20, None) == E
    assert lib.gpsa_ot_sinkhorn_f64(p, 4, 3, p, p, p, p, p, 1, p, 47, None) == W
    assert lib.gpsa_ot_sinkhorn_f64(p, 4, 3, p, p, p, p, p, 1, None, 1 << 20, None) == W
    assert lib.gpsa_ot_plan_f64(p, 4, 3, p, p, p, p, p, None, p, p, p, p, 1 << 20, None) == E
    assert lib.gpsa_ot_plan_f64(p, 4, 3, p, p, p, p, p, p, p, p, p, p, 8 * (4 + 3 + 1) - 1, None) == W
    assert lib.gpsa_ot_plan_f64(p, 4, big, p, p, p, p, p, p, p, p, p, p, 1 << 20, None) == Un


def test_refusals_that_need_no_device():
    XA, XB = torch.rand(6, 2, dtype=torch.float64), torch.rand(5, 2, dtype=torch.float64)
    YA, YB = torch.rand(6, 3), torch.rand(5, 3)
    with pytest.raises(ValueError, match="device 'cpu'"):
        pkg.ot_align(XA, YA, XB, YB)
    with pytest.raises(ValueError, match="share their genes; YA has 3 columns and YB has 2"):
        pkg.ot_align(XA, YA, XB, YB[:, :2])
    with pytest.raises(ValueError, match="D = 5"):
        pkg.ot_align(torch.rand(6, 5), YA, torch.rand(5, 5), YB)
    with pytest.raises(ValueError, match="XB has D = 3"):
        pkg.ot_align(XA, YA, torch.rand(5, 3), YB)
    with pytest.raises(ValueError, match="YA has 5 rows for 6 spots"):
        pkg.ot_align(XA, YA[:5], XB, YB)
    for bad in (XA.long(), XA[:, 0], XA[:0], XA.numpy()):
        with pytest.raises(ValueError, match="has shape"):
            pkg.ot_align(bad, YA, XB, YB)
    with pytest.raises(ValueError, match="has shape"):
        pkg.ot_align(XA, YA.long(), XB, YB)
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="outside \\[0, 1\\]"):
            pkg.ot_align(XA, YA, XB, YB, alpha=alpha)
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            pkg.ot_align(XA, YA, XB, YB, epsilon=eps)
    with pytest.raises(ValueError, match="dissimilarity must be one of"):
        pkg.ot_align(XA, YA, XB, YB, dissimilarity="cosine")
    for kw in (dict(max_iter=0), dict(sinkhorn_iters=0), dict(sync_every=0), dict(max_iter=2.5), dict(tol=-1.0),
               dict(T_init=torch.rand(5, 6, dtype=torch.float64))):
        with pytest.raises(ValueError):
            pkg.ot_align(XA, YA, XB, YB, **kw)
    # the marginals' rules, checked on whatever device the marginal is on
    with pytest.raises(ValueError, match="strictly positive; 2 of its 6"):
        ot._marginal(torch.tensor([0.5, 0.0, 0.25, 0.25, -0.1, 0.1]), "a", "ot_align", 6)
    with pytest.raises(ValueError, match="must sum to 1"):
        ot._marginal(torch.full((6,), 0.2), "a", "ot_align", 6)
    with pytest.raises(ValueError, match="strictly positive; 1 of"):
        ot._marginal(torch.tensor([0.5, float("nan")]), "b", "ot_align", 2)
    with pytest.raises(ValueError, match="has shape"):
        ot._marginal(torch.full((5,), 0.2), "a", "ot_align", 6)
    with pytest.raises(ValueError, match="does not partition"):
        pkg.paste_baseline(torch.rand(11, 2), torch.rand(11, 3), [6, 6])
    with pytest.raises(ValueError, match="2 slices need 1 couplings"):
        pkg.stack_slices([XA, XB], [])
    with pytest.raises(ValueError, match=r"T_list\[0\] has shape"):
        pkg.stack_slices([XA, XB], [torch.rand(5, 6, dtype=torch.float64)])


def test_exports_and_alias():
    import gpsa

    for name in ("ot_align", "OTAlignment", "stack_slices", "paste_baseline"):
        assert name in pkg.__all__ and name in gpsa.__all__
        assert getattr(gpsa, name) is getattr(pkg, name)
    doc = ot.__doc__ + pkg.ot_align.__doc__
    assert "NOT PASTE'S" in doc and "smoothed" in doc and "POT" in doc


def test_dispatcher_ops_propagate_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from spatial_alignment_amd import torch_ops  # noqa: F401

    f64 = torch.float64
    o = torch.ops.gpsa
    with FakeTensorMode():
        X, Y = torch.empty(70, 2, dtype=f64), torch.empty(70, 5)
        C1 = o.ot_dist(X)
        assert C1.shape == (70, 70) and C1.dtype == f64
        v = torch.empty(70, dtype=f64)
        assert o.ot_sqmatvec(C1, v).shape == (70,)
        Pm, Lg, term, bad = o.ot_expr_rows(Y, "kl")
        assert Pm.shape == Lg.shape == (70, 5) and Pm.dtype == Lg.dtype == term.dtype == f64 and term.shape == (70,)
        assert bad.shape == (1,) and bad.dtype == torch.int64
        assert o.ot_expr_rows(Y, "euclidean")[1].shape == (0, 5)
        G, w = torch.empty(70, 33, dtype=f64), torch.empty(33, dtype=f64)
        assert o.ot_expr_cost(G, v, None, "kl") is None
        s = o.ot_cost(G, G, G, v, w, v, w, 0.1)
        assert s.shape == (3,) and s.dtype == f64
        eps = torch.empty(1, dtype=f64)
        assert o.ot_sinkhorn(G, v, w, eps, v, w, 5) is None
        r, c, ps = o.ot_plan(G, v, w, v, w, eps, G)
        assert r.shape == (70,) and c.shape == (33,) and ps.shape == (3,) and r.dtype == c.dtype == ps.dtype == f64


def test_kernel_resources():
    """the kernels of csrc/ot.hip in the built library: launch bounds of 256 threads, nothing in scratch, no spills"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    ks = library_kernels(_lib.LIB_PATH)
    by = dict(zip(demangle([k["name"] for k in ks]), ks))
    families = ("ot_dist_kernel(", "ot_sqmatvec_kernel(", "ot_expr_rows_kernel<", "ot_expr_cost_kernel<", "ot_cost_kernel(",
                "ot_close3_kernel(", "ot_sink_row_kernel(", "ot_sink_col_kernel(", "ot_sink_merge_kernel(",
                "ot_plan_kernel(", "ot_fold_kernel(", "ot_plan_close_kernel(", "ot_count_kernel(")
    seen = {f: 0 for f in families}
    for nm, k in by.items():
        for f in families:
            if f in nm:
                seen[f] += 1
                assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0, (nm, k)
                assert k["lds"] <= 64 * 1024, (nm, k)
    assert all(seen.values()), seen
