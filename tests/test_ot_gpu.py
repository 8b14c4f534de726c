"""Optimal-transport alignment on the device: the entries of csrc/ot.hip through ops.py, and ``ot_align`` / ``stack_slices`` /
``paste_baseline`` of spatial_alignment_amd/ot.py, against the numpy fp64 yardstick of tests/ot_util.py (itself tied to exact
results in tests/test_ot.py).  Reads numpy and tests/golden only.

Shapes: the base set {(1, 1), (1, 7), (5, 3), (63, 65), (64, 64), (130, 257), (257, 130), (300, 513)} and shapes on both
sides of every constant of csrc/ot.hip: 4 rows per workgroup of the row pass (3, 4, 5), a row group of 64 rows (63 .. 65,
128, 129), the 128 groups beyond which a group grows (8193), a column tile of 64 (63 .. 65), the row pass' four loads of 64
columns (255 .. 257, 513), the 1024 workgroups of the cost pass (1025), the 4096 row slots of the expression cost (4097).

Bars: every comparison is the largest |device - yardstick| divided by the magnitude of the terms that were summed (named
at each test), printed before it is asserted.
* Per kernel: the largest discrepancy measured on the MI355X is 6.7e-16 (the plan; distance 1.9e-16, expression rows
  6.0e-16, expression cost 6.1e-16 / 0 ("euclidean": sums of small integers), cost pass 2.1e-16, Sinkhorn sweeps 2.5e-16,
  sqmatvec 4.4e-16); ``KERNEL_BAR`` = 7e-14 is 100 times that.  Above 1e-10 would be a defect to find.
* Whole call: every field of the 30 permutation cases and of seven of the eight unequal-size cases is within 1.1e-13 (the
  marginals / T_init case: 1.0e-12); (130, 257) "kl" with ``norm`` reaches 4.7e-10 of max T, its f and g 3.6e-11, its cost
  fields <= 3.3e-12.  Every kernel on the way agrees to 1e-15; the case itself is that sensitive: the yardstick against
  itself with T_0 moved by 2 ulp per entry ends 2.4e-11 of max T away here, and 9.0e-14 away without ``norm`` (ten outer
  steps of 20 sweeps, marginal error still 4e-2).  100 times 4.7e-10 would
  pass the line of 1e-8 of max T beyond which a difference is a defect, so ``WHOLE_BAR`` is that line.
"""
import functools

import numpy as np
import pytest
import torch

import ot_util as U
import spatial_alignment_amd as pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = torch.float64
KERNEL_BAR = 7e-14  # 100 x 6.7e-16, the largest per-kernel discrepancy measured
WHOLE_BAR = 1e-8     # the defect line; measured: 4.7e-10 at most
BASE = [(1, 1), (1, 7), (5, 3), (63, 65), (64, 64), (130, 257), (257, 130), (300, 513)]
EDGES = [(3, 255), (4, 256), (65, 63), (128, 64), (129, 1), (1025, 2), (4097, 1), (8193, 3)]
SHAPES = BASE + EDGES
SIZES = sorted({n for n, _ in SHAPES} | {m for _, m in SHAPES})


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _dev(a, dtype=f64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def _np(t):
    return t.detach().cpu().numpy()


def _check(name, err, bar):
    print(f"{name}: discrepancy {err:.3e} (bar {bar:.1e})")
    assert np.isfinite(err) and err <= bar, (name, err, bar)


@functools.lru_cache(maxsize=None)
def _problem(n, m, ratio=3.0):
    """a random outer step at (n, m): cost-like G, M, a plan T with non-uniform marginals, potentials; eps so that
    max |cost| / eps is about ``ratio``"""
    rs = np.random.RandomState(7 * n + m)
    a, b = rs.uniform(0.5, 1.5, n), rs.uniform(0.5, 1.5, m)
    a, b = a / a.sum(), b / b.sum()
    T = np.outer(a, b) * rs.uniform(0.5, 1.5, (n, m))
    G, M = rs.uniform(0.0, 4.0, (n, m)), rs.uniform(0.0, 3.0, (n, m))
    cA, cB, cAt, cBt = (rs.uniform(0.0, 5.0, k) for k in (n, m, n, m))
    cost, sums = U.cost_pass(G, M, T, cA, cB, cAt, cBt, 0.3)
    eps = float(np.abs(cost).max() / ratio)
    f, g = rs.normal(size=n) * eps, rs.normal(size=m) * eps
    out = dict(a=a, b=b, T=T, G=G, M=M, cA=cA, cB=cB, cAt=cAt, cBt=cBt, cost=cost, sums=sums, eps=eps, f=f, g=g)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# kernel contracts
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3])
def test_distance_matrix(D):
    """scale: the largest distance.  Symmetric to the bit, the diagonal exactly 0, a repeated call the same bits."""
    o, worst = _ops(), 0.0
    for n in (1, 5, 63, 64, 65, 130, 257):
        X = np.random.RandomState(n + D).uniform(0.0, 10.0, (n, D))
        if n >= 2:
            X[1] = X[0]
        C = o.ot_dist(_dev(X))
        assert torch.equal(C, C.T) and bool((torch.diagonal(C) == 0).all())
        assert torch.equal(C, o.ot_dist(_dev(X)))
        ref = U.dist(X)
        worst = max(worst, np.max(np.abs(_np(C) - ref)) / max(ref.max(), 1.0))
    _check(f"distance D={D}", worst, KERNEL_BAR)


@pytest.mark.parametrize("P", [1, 3, 50, 130])
def test_expression_rows(P):
    """scale: 1 for Pm (entries of a simplex row), the largest |log| for Lg, sum |Pm Lg| (<= log P + ...) for the term.  A row
    of zeros is valid after the 0.01 shift (uniform); negative, NaN and inf entries are counted."""
    o, worst = _ops(), 0.0
    for n in (1, 5, 63, 130):
        Y = np.random.RandomState(n * 31 + P).poisson(3.0, (n, P)).astype(np.float32)
        Y[n // 2] = 0.0
        for mode in ("kl", "euclidean"):
            Pm, Lg, term, bad = o.ot_expr_rows(_dev(Y, torch.float32), mode)
            rP, rL, rt, rbad = U.expr_rows(Y, mode)
            assert int(bad) == rbad == 0
            e = [np.max(np.abs(_np(Pm) - rP)) / max(np.abs(rP).max(), 1.0), np.max(np.abs(_np(Lg) - rL)) / max(np.abs(rL).max(), 1.0),
                 np.max(np.abs(_np(term) - rt) / np.maximum(np.sum(np.abs(rP * rL), axis=1), 1.0))]
            worst = max(worst, *e)
            again = o.ot_expr_rows(_dev(Y, torch.float32), mode)
            assert torch.equal(Pm, again[0]) and torch.equal(term, again[2]) and torch.equal(Lg, again[1])
            if mode == "kl":
                assert np.allclose(_np(Pm)[n // 2], 1.0 / P, rtol=1e-15)
    _check(f"expression rows P={P}", worst, KERNEL_BAR)
    Y = np.random.RandomState(3).poisson(3.0, (70, P)).astype(np.float32)
    Y[0, 0], Y[69, P - 1], Y[33, P // 2] = -1.0, np.nan, np.inf
    want_kl = len({(0, 0), (69, P - 1), (33, P // 2)})
    assert int(o.ot_expr_rows(_dev(Y, torch.float32), "kl")[3]) == want_kl == U.expr_rows(Y, "kl")[3]
    assert int(o.ot_expr_rows(_dev(Y, torch.float32), "euclidean")[3]) == U.expr_rows(Y, "euclidean")[3]


@pytest.mark.parametrize("mode", ["kl", "euclidean"])
def test_expression_cost(mode):
    """the whole M through ot.expression_cost (the rows kernel, gpsa_gemm, the in-place close); scale: sum_p |P_ip log Q_jp| +
    |term_i| ("kl"), |a_i|^2 + |b_j|^2 + 2 sum |a_ip b_jp| ("euclidean"), the largest over the matrix"""
    worst = 0.0
    for n, m in BASE + [(4097, 1), (129, 1)]:
        for P in (1, 3, 50):
            rs = np.random.RandomState(n + 3 * m + P)
            YA, YB = rs.poisson(3.0, (n, P)).astype(np.float32), rs.poisson(3.0, (m, P)).astype(np.float32)
            M = pkg.ot.expression_cost(_dev(YA, torch.float32), _dev(YB, torch.float32), mode)
            ref = U.expr_cost(YA, YB, mode)
            Pa, La, ta, _ = U.expr_rows(YA, mode)
            Pb, Lb, tb, _ = U.expr_rows(YB, mode)
            scale = np.abs(Pa) @ np.abs(Lb).T + np.abs(ta)[:, None] if mode == "kl" else \
                ta[:, None] + tb[None, :] + 2.0 * np.abs(Pa) @ np.abs(Pb).T
            worst = max(worst, np.max(np.abs(_np(M) - ref)) / max(scale.max(), 1.0))
            assert torch.equal(M, pkg.ot.expression_cost(_dev(YA, torch.float32), _dev(YB, torch.float32), mode))
    _check(f"expression cost {mode}", worst, KERNEL_BAR)


@pytest.mark.parametrize("n,m", SHAPES)
def test_cost_pass(n, m):
    """scale: the largest sum of the terms' magnitudes for the cost, sum |terms| for each of the three reductions"""
    o, p = _ops(), _problem(n, m)
    run = lambda: o.ot_cost(_dev(p["G"]), _dev(p["M"]), _dev(p["T"]), _dev(p["cA"]), _dev(p["cB"]), _dev(p["cAt"]),
                            _dev(p["cBt"]), 0.3)
    cost, sums = run()
    mag = 0.7 * p["M"] + 0.6 * (p["cA"][:, None] + p["cB"][None, :] + 2.0 * p["G"])
    e_c = np.max(np.abs(_np(cost) - p["cost"])) / mag.max()
    mags = np.array([np.sum(np.abs(p["cost"])), np.sum(p["M"] * p["T"]),
                     np.sum((p["cAt"][:, None] + p["cBt"][None, :] + 2.0 * p["G"]) * p["T"])])
    e_s = np.max(np.abs(_np(sums) - p["sums"]) / mags)
    again = run()
    assert torch.equal(cost, again[0]) and torch.equal(sums, again[1])
    _check(f"cost pass ({n}, {m})", max(e_c, e_s), KERNEL_BAR)


@pytest.mark.parametrize("ratio", [3.0, 5000.0])
@pytest.mark.parametrize("n,m", SHAPES)
def test_sinkhorn_sweeps(n, m, ratio):
    """three sweeps from given potentials.  scale: max |cost| + max |potential| + eps max |log marginal| - the terms of one
    exponent times eps; at ratio 5000 (|cost| / eps up to 5000) everything stays finite."""
    o, p = _ops(), _problem(n, m, ratio)
    eps, loga, logb = p["eps"], np.log(p["a"]), np.log(p["b"])

    def run():
        f, g = _dev(p["f"]), _dev(p["g"])
        o.ot_sinkhorn(_dev(p["cost"]), _dev(loga), _dev(logb), _dev([eps]), f, g, 3)
        return f, g

    f, g = run()
    rf, rg = U.sinkhorn(p["cost"], loga, logb, eps, p["f"], p["g"], 3)
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(g).all())
    scale = np.abs(p["cost"]).max() + max(np.abs(rf).max(), np.abs(rg).max()) + eps * max(np.abs(loga).max(), np.abs(logb).max())
    err = max(np.max(np.abs(_np(f) - rf)), np.max(np.abs(_np(g) - rg))) / scale
    f2, g2 = run()
    assert torch.equal(f, f2) and torch.equal(g, g2)
    _check(f"sinkhorn ({n}, {m}) ratio {ratio:g}", err, KERNEL_BAR)


@pytest.mark.parametrize("ratio", [3.0, 5000.0])
@pytest.mark.parametrize("n,m", SHAPES)
def test_plan(n, m, ratio):
    """the plan from potentials after three yardstick sweeps, over a T_old.  scale: max T times the size of the exponent's
    terms (an error of u in an exponent of size E changes T by T E u) for T; the sums of |terms| for the marginals and the
    three reductions."""
    o, p = _ops(), _problem(n, m, ratio)
    eps, a, b = p["eps"], p["a"], p["b"]
    f, g = U.sinkhorn(p["cost"], np.log(a), np.log(b), eps, p["f"], p["g"], 3)
    rT, rr, rc, rs = U.plan(p["cost"], f, g, a, b, eps, p["T"])

    def run():
        T = _dev(p["T"])
        return o.ot_plan(_dev(p["cost"]), _dev(f), _dev(g), _dev(a), _dev(b), _dev([eps]), T)

    T, r, c, s = run()
    assert bool(torch.isfinite(T).all())
    E = max(1.0, (np.abs(p["cost"]).max() + np.abs(f).max() + np.abs(g).max()) / eps)
    errs = [np.max(np.abs(_np(T) - rT)) / (rT.max() * E), np.max(np.abs(_np(r) - rr) / ((rr + a) * E)),
            np.max(np.abs(_np(c) - rc) / ((rc + b) * E)),
            np.max(np.abs(_np(s) - rs) / (np.array([rr.sum() + 1.0, rc.sum() + 1.0, rT.sum() + 1.0]) * E))]
    again = run()
    assert all(torch.equal(x, y) for x, y in zip((T, r, c, s), again))
    _check(f"plan ({n}, {m}) ratio {ratio:g}", max(errs), KERNEL_BAR)


def test_sqmatvec():
    """scale: sum_k C_ik^2 |v_k|"""
    o, worst = _ops(), 0.0
    for n, k in ((1, 1), (5, 3), (63, 65), (130, 257), (257, 64)):
        rs = np.random.RandomState(n + k)
        Cm, v = rs.uniform(0.0, 10.0, (n, k)), rs.uniform(0.0, 1.0, k)
        out = o.ot_sqmatvec(_dev(Cm), _dev(v))
        ref = U.sqmatvec(Cm, v)
        worst = max(worst, np.max(np.abs(_np(out) - ref) / ref))
        assert torch.equal(out, o.ot_sqmatvec(_dev(Cm), _dev(v)))
    _check("sqmatvec", worst, KERNEL_BAR)


# ------------------------------------------------------------------------------------------------------------------------
# the whole call
# ------------------------------------------------------------------------------------------------------------------------
FIELDS = ("objective", "expression_cost", "gw_cost", "marginal_error", "plan_change")


def _compare_whole(name, got, ref, bar=WHOLE_BAR):
    """T, f, g and the scalar fields against the yardstick; scale: max T for T, the total mass 1 for the L1 diagnostics (sums
    over all of T's entries), the magnitudes of the terms the cost fields sum (_with_mags), max |potential| + epsilon for f
    and g"""
    T, rT = _np(got.T), ref["T"]
    errs = {"T": np.max(np.abs(T - rT)) / rT.max()}
    pot = max(np.abs(ref["f"]).max(), np.abs(ref["g"]).max()) + ref["epsilon_used"]
    # the potentials are fixed up to a constant shift (f + c, g - c); the sweeps fix it, rounding moves it with the rest
    errs["f"] = np.max(np.abs(_np(got.f) - ref["f"])) / pot
    errs["g"] = np.max(np.abs(_np(got.g) - ref["g"])) / pot
    errs["epsilon"] = abs(got.epsilon_used - ref["epsilon_used"]) / ref["epsilon_used"]
    gw_mag = ref["gw_pos"]
    mags = dict(objective=max(ref["expr_pos"], gw_mag), expression_cost=ref["expr_pos"],
                gw_cost=gw_mag, marginal_error=1.0, plan_change=1.0)
    for k in FIELDS:
        errs[k] = abs(getattr(got, k) - ref[k]) / mags[k]
    assert got.n_iter == ref["n_iter"]
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    _check(name, max(errs.values()), bar)


def _with_mags(ref, C1, C2, YA, YB, mode="kl"):
    """the magnitudes of the terms that the two cost fields sum: the GW sum's positive part, and sum_ij T_ij (the terms
    of M_ij taken by magnitude) - with identical expression <M, T> itself cancels to nothing and is no scale"""
    T = ref["T"]
    p, q = T.sum(1), T.sum(0)
    ref["gw_pos"] = float(p @ (C1 * C1) @ p + q @ (C2 * C2) @ q) + 1e-300
    Pa, _, ta, _ = U.expr_rows(YA, mode)
    Pb, Lb, tb, _ = U.expr_rows(YB, mode)
    mag = np.abs(ta)[:, None] + np.abs(Pa) @ np.abs(Lb).T if mode == "kl" else \
        ta[:, None] + tb[None, :] + 2.0 * np.abs(Pa) @ np.abs(Pb).T
    ref["expr_pos"] = float(np.sum(mag * T)) + 1e-300
    return ref


@functools.lru_cache(maxsize=None)
def _perm_ref(seed, alpha, eps):
    XA, YA, XB, YB, perm = U.permutation_case(seed, 40, 10)
    ref = U.ot_align(XA, YA, XB, YB, alpha=alpha, epsilon=eps)
    return XA, YA, XB, YB, perm, _with_mags(ref, U.dist(XA), U.dist(XB), YA, YB)


@pytest.mark.parametrize("eps", [0.05, 0.01, 0.002])
@pytest.mark.parametrize("alpha", [0.1, 0.5])
@pytest.mark.parametrize("seed", range(5))
def test_ot_align_recovers_the_planted_permutation(seed, alpha, eps):
    XA, YA, XB, YB, perm, ref = _perm_ref(seed, alpha, eps)
    got = pkg.ot_align(_dev(XA), _dev(YA, torch.float32), _dev(XB), _dev(YB, torch.float32), alpha=alpha, epsilon=eps)
    _compare_whole(f"ot_align perm seed {seed} alpha {alpha} eps {eps}", got, ref)
    assert np.array_equal(_np(got.T.argmax(1)), U.partner(perm))
    (A, B), _, _ = pkg.stack_slices([_dev(XA), _dev(XB)], [got.T])
    err = float((B - A[_dev(perm, torch.int64)]).abs().max())
    print(f"stacking error {err:.2e}, marginal error {got.marginal_error:.1e}")
    if eps == 0.01:
        assert err <= 1e-2
    if seed == 0 and alpha == 0.1:
        again = pkg.ot_align(_dev(XA), _dev(YA, torch.float32), _dev(XB), _dev(YB, torch.float32), alpha=alpha, epsilon=eps)
        assert torch.equal(got.T, again.T) and got.objective == again.objective and torch.equal(got.f, again.f)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("mode", ["kl", "euclidean"])
@pytest.mark.parametrize("n,m", [(63, 65), (130, 257)])
def test_ot_align_unequal_sizes(n, m, mode, norm):
    rs = np.random.RandomState(n + m)
    XA, XB = rs.uniform(0.0, 10.0, (n, 2)), rs.uniform(0.0, 10.0, (m, 2))
    YA, YB = rs.poisson(rs.gamma(2.0, 2.0, (n, 12))).astype(np.float32), rs.poisson(rs.gamma(2.0, 2.0, (m, 12))).astype(np.float32)
    kw = dict(alpha=0.1, dissimilarity=mode, epsilon=0.01, norm=norm, max_iter=10, sinkhorn_iters=20)
    ref = _with_mags(U.ot_align(XA, YA, XB, YB, **kw), U.dist(XA, norm), U.dist(XB, norm), YA, YB, mode)
    got = pkg.ot_align(_dev(XA), _dev(YA, torch.float32), _dev(XB), _dev(YB, torch.float32), **kw)
    _compare_whole(f"ot_align ({n}, {m}) {mode} norm={norm}", got, ref)
    assert abs(got.objective - (0.9 * got.expression_cost + 0.1 * got.gw_cost)) <= 1e-15 * abs(got.objective)


def test_ot_align_marginals_t_init_and_tol():
    rs = np.random.RandomState(11)
    n, m = 63, 65
    XA, XB = rs.uniform(0.0, 10.0, (n, 3)), rs.uniform(0.0, 10.0, (m, 3))
    YA, YB = rs.poisson(3.0, (n, 50)).astype(np.float32), rs.poisson(3.0, (m, 50)).astype(np.float32)
    a, b = rs.uniform(0.5, 1.5, n), rs.uniform(0.5, 1.5, m)
    a, b = a / a.sum(), b / b.sum()
    T0 = np.outer(a, b) * rs.uniform(0.8, 1.2, (n, m))
    kw = dict(alpha=0.3, epsilon=0.05, relative_epsilon=False, max_iter=6, sinkhorn_iters=10)
    ref = _with_mags(U.ot_align(XA, YA, XB, YB, a=a, b=b, T_init=T0, **kw), U.dist(XA), U.dist(XB), YA, YB)
    args = (_dev(XA), _dev(YA, torch.float32), _dev(XB), _dev(YB, torch.float32))
    got = pkg.ot_align(*args, a=_dev(a), b=_dev(b), T_init=_dev(T0), **kw)
    assert got.epsilon_used == 0.05
    _compare_whole("ot_align marginals + T_init", got, ref)
    # tol: the loop ends at the first check (every 2 steps) where the plan moved less than tol
    loose = pkg.ot_align(*args, a=_dev(a), b=_dev(b), T_init=_dev(T0), tol=10.0, sync_every=2, **kw)
    assert loose.n_iter == 2 and loose.plan_change < 10.0
    tight = pkg.ot_align(*args, a=_dev(a), b=_dev(b), T_init=_dev(T0), tol=0.0, sync_every=2, **kw)
    assert tight.n_iter == 6 and torch.equal(tight.T, got.T)


def test_stack_slices_and_paste_baseline():
    """a chain of three slices against the yardstick, both reflection settings, the third slice a mirror image (det R < 0
    without the guard); paste_baseline returns the rows in data_dict order"""
    XA, YA, XB, YB, perm = U.permutation_case(3, 40, 10)
    XC = (XA * np.array([1.0, -1.0]) + 1.0)[perm]
    T1 = pkg.ot_align(_dev(XA), _dev(YA, torch.float32), _dev(XB), _dev(YB, torch.float32)).T
    T2 = _dev(np.eye(40) / 40.0)
    for refl in (True, False):
        got = pkg.stack_slices([_dev(XA), _dev(XB), _dev(XC)], [T1, T2], reflection=refl)
        want = U.stack_slices([XA, XB, XC], [_np(T1), _np(T2)], reflection=refl)
        for k in range(3):
            for q in range(3):
                assert np.allclose(_np(got[q][k]), want[q][k], rtol=0, atol=1e-11), (refl, k, q)
        assert (np.linalg.det(_np(got[1][2])) < 0) == refl
    X, Y = np.concatenate([XA, XB]), np.concatenate([YA, YB])
    coords = pkg.paste_baseline(_dev(X), _dev(Y, torch.float32), [40, 40])
    (A, B), _, _ = pkg.stack_slices([_dev(XA), _dev(XB)], [T1])
    assert coords.shape == (80, 2) and torch.equal(coords[:40], A) and torch.equal(coords[40:], B)
    assert float((coords[40:] - coords[:40][_dev(perm, torch.int64)]).abs().max()) <= 1e-2


class _Spy:
    """every op the solve would launch, recorded by name"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.real, name)


def test_value_errors_are_raised_before_any_launch():
    from spatial_alignment_amd import ops

    XA, XB = torch.rand(6, 2, dtype=f64, device=DEV), torch.rand(5, 2, dtype=f64, device=DEV)
    YA, YB = torch.rand(6, 3, device=DEV), torch.rand(5, 3, device=DEV)
    real = ops.get_ops()
    spy = _Spy(real)
    ops.set_ops(spy)
    try:
        cases = [
            (dict(alpha=1.5), "outside"), (dict(epsilon=0.0), "epsilon"), (dict(dissimilarity="cosine"), "dissimilarity"),
            (dict(a=torch.tensor([0.5, 0.5, 0.0, 0.0, 0.0, 0.0], device=DEV)), "strictly positive; 4 of its 6"),
            (dict(b=torch.full((5,), 0.25, device=DEV)), "must sum to 1"),
            (dict(a=torch.full((6,), 1 / 6)), "a is on device 'cpu'"),
        ]
        for kw, match in cases:
            with pytest.raises(ValueError, match=match):
                pkg.ot_align(XA, YA, XB, YB, **kw)
        with pytest.raises(ValueError, match="YB has 2"):
            pkg.ot_align(XA, YA, XB, YB[:, :2].contiguous())
        with pytest.raises(ValueError, match="D = 5"):
            pkg.ot_align(torch.rand(6, 5, device=DEV), YA, torch.rand(5, 5, device=DEV), YB)
        with pytest.raises(ValueError, match="device 'cpu'"):
            pkg.ot_align(XA.cpu(), YA, XB, YB)
        assert spy.calls == []
        # what "kl" cannot take is counted by the kernel that reads the expression; nothing of the solve runs
        bad = YA.clone()
        bad[0, 0], bad[3, 2] = -1.0, float("nan")
        with pytest.raises(ValueError, match="2 entries of YA and 0 of YB"):
            pkg.ot_align(XA, bad, XB, YB)
        assert set(spy.calls) == {"ot_expr_rows"}
        spy.calls.clear()
        with pytest.raises(ValueError, match="1 entries of YA and 0 of YB"):
            pkg.ot_align(XA, bad, XB, YB, dissimilarity="euclidean")  # the negative entry is fine here, the NaN is not
        assert set(spy.calls) == {"ot_expr_rows"}
    finally:
        ops.set_ops(real)


def test_dispatcher_ops_reach_the_same_entries():
    from spatial_alignment_amd import torch_ops  # noqa: F401

    o, t, p = _ops(), torch.ops.gpsa, _problem(63, 65)
    X = _dev(np.random.RandomState(0).uniform(0, 10, (63, 2)))
    assert torch.equal(t.ot_dist(X), o.ot_dist(X))
    C = o.ot_dist(X)
    assert torch.equal(t.ot_sqmatvec(C, _dev(p["a"])), o.ot_sqmatvec(C, _dev(p["a"])))
    Y = _dev(np.random.RandomState(1).poisson(3.0, (63, 7)), torch.float32)
    for x, y in zip(t.ot_expr_rows(Y, "kl"), o.ot_expr_rows(Y, "kl")):
        assert torch.equal(x, y)
    G1, G2 = _dev(p["G"]), _dev(p["G"])
    s1 = t.ot_cost(G1, _dev(p["M"]), _dev(p["T"]), _dev(p["cA"]), _dev(p["cB"]), _dev(p["cAt"]), _dev(p["cBt"]), 0.3)
    _, s2 = o.ot_cost(G2, _dev(p["M"]), _dev(p["T"]), _dev(p["cA"]), _dev(p["cB"]), _dev(p["cAt"]), _dev(p["cBt"]), 0.3)
    assert torch.equal(G1, G2) and torch.equal(s1, s2)
    la, lb, eps = _dev(np.log(p["a"])), _dev(np.log(p["b"])), _dev([p["eps"]])
    f1, g1, f2, g2 = _dev(p["f"]), _dev(p["g"]), _dev(p["f"]), _dev(p["g"])
    t.ot_sinkhorn(G1, la, lb, eps, f1, g1, 2)
    o.ot_sinkhorn(G2, la, lb, eps, f2, g2, 2)
    assert torch.equal(f1, f2) and torch.equal(g1, g2)
    T1, T2 = _dev(p["T"]), _dev(p["T"])
    r1 = t.ot_plan(G1, f1, g1, _dev(p["a"]), _dev(p["b"]), eps, T1)
    r2 = o.ot_plan(G2, f2, g2, _dev(p["a"]), _dev(p["b"]), eps, T2)[1:]
    assert torch.equal(T1, T2) and all(torch.equal(x, y) for x, y in zip(r1, r2))
    M1, M2 = _dev(p["M"]), _dev(p["M"])
    t.ot_expr_cost(M1, _dev(p["cA"]), _dev(p["cB"]), "euclidean")
    o.ot_expr_cost(M2, _dev(p["cA"]), _dev(p["cB"]), "euclidean")
    assert torch.equal(M1, M2)
