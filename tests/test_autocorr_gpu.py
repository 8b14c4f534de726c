"""Spatial autocorrelation on the device: the graph entries and the permuted statistic of csrc/autocorr.hip, then the calls
of spatial_alignment_amd/autocorr.py, against the numpy fp64 yardstick of tests/autocorr_util.py (itself held to exact
facts in tests/test_autocorr.py).

Bars (every comparison prints what it measures next to its bar):
* the graph: crow / col EQUAL, w equal to the bit (1 or 1 / deg), n_isolated equal, a second build the same bits;
* S0 / S1 / S2 and the permuted numerators: 1e-11 of the sum of the terms' magnitudes - the project's bar for fixed-order
  fp64 sums (n eps with n <= 1e5);
* I / C, var_norm, sims: 1e-9 absolute, the bar tests/test_neighbors_gpu.py holds Moran's I to;
* the derived columns (pval_sim, var_sim, pval_z_sim, the three _fdr_bh): 1e-12 against the yardstick's rules applied to
  the device's own sims - that separates the kernel from the formulas;
* the >= counts against the yardstick's own sims: equal wherever the yardstick's |sim - stat| exceeds 1e-9; with the
  seeded continuous data none is set aside (asserted; the smallest gap measured in numpy is 4.9e-6).
"""
import functools
import itertools
import re

import numpy as np
import pytest
import torch

import autocorr_util as au
import neighbors_util as nu
import spatial_alignment_amd as gp
from spatial_alignment_amd import autocorr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64, f32, i32, i64 = torch.float64, torch.float32, torch.int32, torch.int64
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
KINDS = ("none", "union", "mutual")
# (n, D, k): the sizes cross the 256-row workgroup of the graph kernels; "lattice": every row ties
GRAPHS = [(63, 2, 1), (64, 2, 6), (65, 2, 6), (257, 2, 32), (300, 3, 10), (1301, 2, 6), "lattice"]
# (n, k, P, R): the wave width in genes, the workgroup (16 permutations) and the row groups (32 rows at least, 32 groups
# at most) in rows, one against many permutations
PERM_CASES = [(64, 6, 64, 7), (65, 6, 65, 1), (63, 1, 1, 2), (300, 6, 130, 99), (257, 32, 5, 3), (1000, 10, 63, 20),
              (1301, 6, 200, 10)]


def _lib():
    from spatial_alignment_amd import _lib as L

    return L.load()


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _dev(a, dt=f64):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _points(n, D):
    return au.points(n, D, 1000 * n + D)


@functools.lru_cache(maxsize=None)
def _yard_graph(n, D, k, kind, std):
    """(A, W) of the yardstick, computed once, shared, never changed"""
    X = nu.lattice() if n == "lattice" else _points(n, D)
    return au.adjacency(X, k, kind), au.dense_weights(X, k, kind, std)


def _graph_case(case):
    return ("lattice", 2, 6) if case == "lattice" else case


def _rel(got, want, mag):
    return float(np.max(np.abs(got - want) / np.maximum(mag, 1e-300)))


# ------------------------------------------------------------------------------------------------------------------------
# the graph
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(GRAPHS)))
def test_graph_equals_the_yardstick(case):
    n, D, k = _graph_case(GRAPHS[case])
    X = nu.lattice() if n == "lattice" else _points(n, D)
    Xd = _dev(X)
    for kind in KINDS:
        for std in (True, False):
            A, W = _yard_graph(n, D, k, kind, std)
            crow, col, w = au.csr(W, A)
            g = gp.spatial_graph(Xd, k=k, symmetric=kind, row_standardize=std)
            assert g.n == len(X) and g.crow.dtype == i64 and g.col.dtype == i32 and g.w.dtype == f64
            assert np.array_equal(g.crow.cpu().numpy(), crow) and np.array_equal(g.col.cpu().numpy(), col)
            assert np.array_equal(g.w.cpu().numpy(), w)  # to the bit
            iso = int((A.sum(1) == 0).sum())
            assert int(g.n_isolated) == iso
            S = np.array(au.graph_sums(W))
            got = g.sums.cpu().numpy()
            err = _rel(got, S, S)  # every term is >= 0: the sums are their own magnitudes
            print(f"[autocorr graph] {GRAPHS[case]} {kind} std={std}: nnz {len(col)}, isolated {iso}, S0/S1/S2 off by "
                  f"{err:.2e} relative (bar 1e-11)")
            assert err <= 1e-11
            g2 = gp.spatial_graph(Xd, k=k, symmetric=kind, row_standardize=std, rows_per_chunk=100)
            for a, b in ((g.crow, g2.crow), (g.col, g2.col), (g.w, g2.w), (g.sums, g2.sums)):
                assert torch.equal(a, b)


def test_mutual_graph_with_isolated_rows_exists_among_the_cases():
    """the "mutual" cases above do exercise a row of degree 0"""
    assert any((_yard_graph(*_graph_case(c), "mutual", True)[0].sum(1) == 0).any() for c in GRAPHS)


def _star_graph():
    crow, col, w, n = au.star(500)
    return gp.SpatialGraph.from_csr(_dev(crow, i64), _dev(col, i32), _dev(w), n), au.dense_from_csr(crow, col, w, n)


def test_callers_star_graph():
    g, W = _star_graph()
    crow, col, w, n = au.star(500)
    assert g.n == n and np.array_equal(g.col.cpu().numpy(), col) and np.array_equal(g.w.cpu().numpy(), w)
    S = np.array(au.graph_sums(W))
    err = _rel(g.sums.cpu().numpy(), S, S)
    print(f"[autocorr graph] star: S0/S1/S2 {g.sums.tolist()} off by {err:.2e} relative (bar 1e-11)")
    assert err <= 1e-11 and int(g.n_isolated) == 0
    # other integer / float dtypes are converted
    g2 = gp.SpatialGraph.from_csr(_dev(crow, i32), _dev(col, i64), _dev(w, f32), n)
    assert g2.crow.dtype == i64 and g2.col.dtype == i32 and g2.w.dtype == f64


@pytest.mark.parametrize("rule", range(5))
def test_malformed_csr_is_refused_by_name(rule):
    crow, col, w, n = au.star(5)  # row 0: 1 2 3 4 5; rows 1..5: 0
    count = 1
    if rule == 0:
        crow = crow.copy()
        crow[3] = crow[2] - 1  # a decrease (and the next step up is none)
    elif rule == 1:
        col = col.copy()
        col[4], count = n, 1
    elif rule == 2:
        col = col.copy()
        col[1], col[2] = col[2], col[1]
    elif rule == 3:
        col = col.copy()
        col[0] = 0
    else:
        w = w.copy()
        w[2], w[7], count = -0.5, float("nan"), 2
    with pytest.raises(ValueError, match=re.escape(f"{autocorr._RULES[rule]}: {count}")):
        gp.SpatialGraph.from_csr(_dev(crow, i64), _dev(col, i32), _dev(w), n)


# ------------------------------------------------------------------------------------------------------------------------
# the permuted statistic through the C ABI alone
# ------------------------------------------------------------------------------------------------------------------------
def _perm_abi(Zt, crowt, colt, wt, permst, mode, nbytes=None, num_t=None, n_bad_t=None, **over):
    """one call of gpsa_autocorr_perm_f64 on device tensors -> (rc, num, n_bad)"""
    lib = _lib()
    n, P = Zt.shape
    R = permst.shape[0]
    need = int(lib.gpsa_autocorr_perm_workspace(n, P, R))
    nbytes = need if nbytes is None else nbytes
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=DEV)
    num = torch.empty(R, P, dtype=f64, device=DEV) if num_t is None else num_t
    n_bad = torch.empty(1, dtype=i64, device=DEV) if n_bad_t is None else n_bad_t
    a = dict(Z=Zt.data_ptr(), n=n, P=P, crow=crowt.data_ptr(), col=colt.data_ptr(), w=wt.data_ptr(), nnz=colt.numel(),
             perms=permst.data_ptr(), R=R, mode=mode, num=num.data_ptr(), n_bad=n_bad.data_ptr(), ws=ws.data_ptr(),
             nbytes=nbytes)
    a.update(over)
    rc = lib.gpsa_autocorr_perm_f64(*a.values(), _stream())
    torch.cuda.synchronize()
    return rc, num, n_bad


@functools.lru_cache(maxsize=None)
def _perm_inputs(case):
    """(X, Z, perms) of a case: row 0 the identity, and again the last row where R >= 3"""
    n, k, P, R = PERM_CASES[case]
    X = _points(n, 2)
    Z = au.centre(au.expression(X, P, case))
    rng = np.random.default_rng(100 + case)
    perms = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(R - 1)])
    if R >= 3:
        perms[-1] = np.arange(n)
    return X, Z, perms


def _check_num(tag, Zh, W, perms, mode, Zd, g):
    """the entry against the yardstick, twice, and cut into chunks of 1, 3 and R permutations"""
    want, mag = au.numerators(W, Zh, perms, "geary" if mode else "moran")
    pd = _dev(perms, i32)
    rc, num, bad = _perm_abi(Zd, g.crow, g.col, g.w, pd, mode)
    assert rc == 0 and int(bad) == 0
    got = num.cpu().numpy()
    err = _rel(got, want, mag)
    print(f"[autocorr perm] {tag} mode {mode}: numerators off by {err:.2e} of the sum of |terms| (bar 1e-11)")
    assert err <= 1e-11
    rc, again, _ = _perm_abi(Zd, g.crow, g.col, g.w, pd, mode)
    assert rc == 0 and torch.equal(num, again)
    R = len(perms)
    for c in sorted({1, 3, R}):
        if c > R:
            continue
        parts = [_perm_abi(Zd, g.crow, g.col, g.w, pd[a: a + c].contiguous(), mode)[1] for a in range(0, R, c)]
        assert torch.equal(torch.cat(parts), num), (tag, c)
    if R >= 3:
        assert torch.equal(num[0], num[-1])  # the identity ties with itself exactly, wherever it stands
    return num


@pytest.mark.parametrize("kind", ("none", "union"))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("case", range(len(PERM_CASES)))
def test_permuted_numerators_equal_the_yardstick(case, mode, kind):
    n, k, P, R = PERM_CASES[case]
    X, Zh, perms = _perm_inputs(case)
    _, W = _yard_graph(n, 2, k, kind, True)
    g = gp.spatial_graph(_dev(X), k=k, symmetric=kind)
    _check_num(f"{PERM_CASES[case]} {kind}", Zh, W, perms, mode, _dev(Zh), g)


@pytest.mark.parametrize("mode", (0, 1))
def test_permuted_numerators_on_a_hub_and_on_isolated_rows(mode):
    rng = np.random.default_rng(7)
    g, W = _star_graph()  # row 0 is longer than a wave and than a workgroup
    Zh = au.centre(rng.normal(size=(501, 70)).astype(np.float32))
    perms = np.stack([np.arange(501)] + [rng.permutation(501) for _ in range(4)] + [np.arange(501)])
    _check_num("star", Zh, W, perms, mode, _dev(Zh), g)
    n, D, k = 63, 2, 1  # k = 1: a row whose nearest point has another nearest point is left without an edge
    A, W = _yard_graph(n, D, k, "mutual", True)
    assert (A.sum(1) == 0).any() and (A.sum(1) > 0).any()
    g = gp.spatial_graph(_dev(_points(n, D)), k=k, symmetric="mutual")
    Zh = au.centre(rng.normal(size=(n, 33)).astype(np.float32))
    perms = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(5)] + [np.arange(n)])
    _check_num("mutual with isolated rows", Zh, W, perms, mode, _dev(Zh), g)


def test_exact_means_over_all_permutations_on_the_device():
    SIX = np.array([[0.0, 0.0], [1.0, 0.1], [0.4, 0.9], [5.0, 5.0], [5.6, 5.2], [2.6, 2.4]])
    n = 6
    perms = _dev(np.array(list(itertools.permutations(range(n)))), i32)
    Zh = au.centre(np.random.default_rng(0).normal(size=(n, 3)))
    Zd, den = _dev(Zh), (Zh * Zh).sum(0)
    worst = 0.0
    for kind in KINDS:
        for std in (True, False):
            g = gp.spatial_graph(_dev(SIX), k=2, symmetric=kind, row_standardize=std)
            S0 = float(g.S0)
            for mode, want, scale in ((0, -1.0 / (n - 1), n / S0), (1, 1.0, (n - 1) / (2.0 * S0))):
                rc, num, bad = _perm_abi(Zd, g.crow, g.col, g.w, perms, mode)
                assert rc == 0 and int(bad) == 0
                worst = max(worst, float(np.abs((scale * num.cpu().numpy() / den).mean(0) - want).max()))
    print(f"[autocorr perm] mean over all 720 permutations off by {worst:.2e} (bar 1e-12)")
    assert worst <= 1e-12


def test_out_of_range_entries_are_counted_and_never_followed():
    n, k, P, R = PERM_CASES[0]
    X, Zh, perms = _perm_inputs(0)
    g = gp.spatial_graph(_dev(X), k=k)
    Zd = _dev(Zh)
    good = _perm_abi(Zd, g.crow, g.col, g.w, _dev(perms, i32), 0)[1]
    bad_perms = perms.copy()
    bad_perms[2, 5] = n
    bad_col = g.col.clone()
    bad_col[17] = -1
    for pm, col, want in ((bad_perms, g.col, 1), (perms, bad_col, 1), (bad_perms, bad_col, 2)):
        for mode in (0, 1):
            rc, num, bad = _perm_abi(Zd, g.crow, col, g.w, _dev(pm, i32), mode)
            assert rc == 0 and int(bad) == want and bool(torch.isfinite(num).all())
    # a permutation row without a bad entry is untouched by another row's
    rc, num, _ = _perm_abi(Zd, g.crow, g.col, g.w, _dev(bad_perms, i32), 0)
    keep = [r for r in range(R) if r != 2]
    assert torch.equal(num[keep], good[keep])
    # the whole call raises on the count (a graph tampered with after its check)
    bad_graph = gp.SpatialGraph.from_csr(g.crow, g.col, g.w, n)
    bad_graph.col = bad_col
    with pytest.raises(ValueError, match="outside"):
        gp.spatial_autocorr(bad_graph, _dev(Zh, f32), n_perms=2)


def test_refusals_come_before_any_launch():
    n, k, P, R = PERM_CASES[0]
    X, Zh, perms = _perm_inputs(0)
    g = gp.spatial_graph(_dev(X), k=k)
    Zd, pd = _dev(Zh), _dev(perms, i32)
    need = int(_lib().gpsa_autocorr_perm_workspace(n, P, R))
    num = torch.full((R, P), 7.0, dtype=f64, device=DEV)
    n_bad = torch.full((1,), -5, dtype=i64, device=DEV)
    call = lambda **kw: _perm_abi(Zd, g.crow, g.col, g.w, pd, kw.pop("mode", 0), num_t=num, n_bad_t=n_bad, **kw)[0]
    assert call(nbytes=need - 1) == EWORKSPACE and call(ws=None) == EWORKSPACE
    for over in (dict(mode=2), dict(mode=-1), dict(n=0), dict(P=0), dict(R=0), dict(nnz=-1), dict(Z=None), dict(crow=None),
                 dict(col=None), dict(w=None), dict(perms=None), dict(num=None), dict(n_bad=None)):
        assert call(**over) == EINVAL, over
    assert call(n=1 << 31) == EUNSUPPORTED
    assert bool((num == 7.0).all()) and int(n_bad) == -5
    assert call() == 0 and bool((num != 7.0).any()) and int(n_bad) == 0


# ------------------------------------------------------------------------------------------------------------------------
# the whole call
# ------------------------------------------------------------------------------------------------------------------------
WHOLE = (300, 6, 130, 99)  # (n, k, P, R)


@functools.lru_cache(maxsize=None)
def _whole_inputs():
    n, k, P, R = WHOLE
    X = _points(n, 2)
    Y = au.expression(X, P, 42)
    rng = np.random.default_rng(43)
    perms = np.stack([rng.permutation(n) for _ in range(R)])
    return X, Y, perms


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ("moran", "geary"))
def test_whole_call_equals_the_yardstick(mode, kind):
    n, k, P, R = WHOLE
    X, Y, perms = _whole_inputs()
    _, W = _yard_graph(n, 2, k, kind, True)
    want = au.table(W, Y, perms, mode)
    res = gp.spatial_autocorr(_dev(X), _dev(Y, f32), mode=mode, perms=_dev(perms, i64), k=k, symmetric=kind)
    stat = res["I" if mode == "moran" else "C"].cpu().numpy()
    sims = res.sims.cpu().numpy()
    assert sims.shape == (R, P) and ("C" if mode == "moran" else "I") not in res
    e_stat, e_sims = np.abs(stat - want["stat"]).max(), np.abs(sims - want["sims"]).max()
    e_var = abs(float(res.var_norm[0]) - want["var_norm"])
    print(f"[autocorr] {mode} {kind}: statistic {e_stat:.2e}, sims {e_sims:.2e}, var_norm {e_var:.2e} absolute (bar 1e-9)")
    assert e_stat <= 1e-9 and e_sims <= 1e-9 and e_var <= 1e-9
    assert bool((res.var_norm == res.var_norm[0]).all()) and float(res.expected[0]) == want["expected"]
    e_p = np.abs(res.pval_norm.cpu().numpy() - au.folded_p((stat - want["expected"]) / np.sqrt(float(res.var_norm[0])))).max()
    e_bh = np.abs(res.pval_norm_fdr_bh.cpu().numpy() - au.bh(res.pval_norm.cpu().numpy())).max()
    own = au.derived(stat, sims)
    errs = {name: float(np.abs(res[name].cpu().numpy() - own[name]).max()) for name in own}
    print(f"[autocorr] {mode} {kind}: pval_norm {e_p:.2e}, its BH {e_bh:.2e}, derived from the device's sims "
          + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()) + " (bar 1e-12)")
    assert e_p <= 1e-12 and e_bh <= 1e-12 and max(errs.values()) <= 1e-12
    # the >= counts against the yardstick's own sims, where its gap is clear
    gap = np.abs(want["sims"] - want["stat"][None])
    clear = gap > 1e-9
    print(f"[autocorr] {mode} {kind}: smallest |sim - stat| of the yardstick {gap.min():.2e}; set aside {(~clear).sum()}")
    assert clear.all()
    assert np.array_equal(sims >= stat[None], want["sims"] >= want["stat"][None])
    assert np.array_equal(au.larger_counts(stat, sims), au.larger_counts(want["stat"], want["sims"]))
    for name in ("S0", "S1", "S2"):
        assert res[name].device.type == "cuda"
    two = gp.spatial_autocorr(_dev(X), _dev(Y, f32), mode=mode, perms=_dev(perms, i64), k=k, symmetric=kind, two_tailed=True,
                              perms_per_chunk=7)
    assert torch.equal(two.sims, res.sims) and torch.equal(two.pval_norm, 2.0 * res.pval_norm)
    assert torch.equal(two.pval_z_sim, 2.0 * res.pval_z_sim) and torch.equal(two.pval_sim, res.pval_sim)


def test_without_permutations_it_is_moran_i():
    n, k, P, R = WHOLE
    X, Y, _ = _whole_inputs()
    Xd, Yd = _dev(X), _dev(Y, f32)
    for std in (True, False):
        ref = gp.moran_i(Xd, Yd, k=k, row_standardize=std)
        res = gp.spatial_autocorr(Xd, Yd, mode="moran", n_perms=0, k=k, symmetric="none", row_standardize=std)
        z = (res.I - res.expected) / res.var_norm.sqrt()
        errs = [float((res.I - ref.I).abs().max()), float((res.var_norm - ref.variance).abs().max()),
                float((z - ref.z).abs().max())]
        print(f"[autocorr] n_perms=0 against moran_i (std={std}): I {errs[0]:.2e}, variance {errs[1]:.2e}, z {errs[2]:.2e} "
              "(bar 1e-9)")
        assert max(errs) <= 1e-9
        for name in ("sims", "pval_sim", "var_sim", "pval_z_sim", "pval_sim_fdr_bh", "pval_z_sim_fdr_bh"):
            assert res[name] is None
        # a graph passed in is the same call
        g = gp.spatial_graph(Xd, k=k, row_standardize=std)
        assert torch.equal(gp.spatial_autocorr(g, Yd, n_perms=0).I, res.I)


def test_constant_column_nan_in_y_generator_and_bad_perms():
    n, k, P, R = WHOLE
    X, Y, perms = _whole_inputs()
    Yc = Y[:, :12].copy()
    Yc[:, 5] = 3.25
    Xd = _dev(X)
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)
    for mode in ("moran", "geary"):
        res = gp.spatial_autocorr(Xd, _dev(Yc, f32), mode=mode, n_perms=19, generator=gen(), symmetric="union")
        stat = res["I" if mode == "moran" else "C"]
        for name in ("pval_norm", "pval_sim", "var_sim", "pval_z_sim", "pval_norm_fdr_bh", "pval_sim_fdr_bh",
                     "pval_z_sim_fdr_bh"):
            v = res[name]
            assert bool(torch.isnan(v[5])) and not bool(torch.isnan(v[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]]).any()), name
        assert bool(torch.isnan(stat[5])) and bool(torch.isnan(res.sims[:, 5]).all())
        others = [c for c in range(12) if c != 5]
        bh = au.bh(res.pval_norm.cpu().numpy()[others])  # BH over the 11 finite entries: the NaN does not count
        assert np.abs(res.pval_norm_fdr_bh.cpu().numpy()[others] - bh).max() <= 1e-12
        again = gp.spatial_autocorr(Xd, _dev(Yc, f32), mode=mode, n_perms=19, generator=gen(), symmetric="union",
                                    perms_per_chunk=4)
        for name in res:  # the same generator state: the same bits (NaN where NaN)
            if torch.is_tensor(res[name]) and res[name].is_floating_point():
                assert torch.equal(torch.nan_to_num(res[name], nan=-9.0), torch.nan_to_num(again[name], nan=-9.0)), name
    Yn = Y[:, :3].copy()
    Yn[4, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        gp.spatial_autocorr(Xd, _dev(Yn, f32))
    twice = perms[:3].copy()
    twice[1, 0] = twice[1, 1]
    with pytest.raises(ValueError, match="not a permutation"):
        gp.spatial_autocorr(Xd, _dev(Y[:, :3], f32), perms=_dev(twice, i64))
    with pytest.raises(ValueError, match="device 'cpu'"):
        gp.spatial_autocorr(Xd, torch.tensor(Y[:, :3]))


def test_memory_stays_within_z_sims_workspace_and_graph():
    n, P, R, k = 4000, 2000, 100, 6
    gen = torch.Generator(device=DEV).manual_seed(5)
    X = torch.rand(n, 2, dtype=f64, device=DEV, generator=gen) * 60.0
    Y = torch.randn(n, P, dtype=f32, device=DEV, generator=gen)
    ws_bytes = int(_lib().gpsa_autocorr_perm_workspace(n, P, R))
    held = _ops()._ws(ws_bytes, X)  # the workspace already held: it is the ops object's, kept between calls
    assert held.numel() >= ws_bytes
    graph_bytes = 8 * (n + 1) + (4 + 8) * 2 * n * k + 8 * 3  # crow, col and w of a union graph at most, the sums
    bound = 8 * n * P + 8 * R * P + ws_bytes + graph_bytes
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = gp.spatial_autocorr(X, Y, mode="moran", n_perms=R, generator=gen, k=k, symmetric="union")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[autocorr] {n} x {P}, {R} permutations: peak {peak / 2**20:.1f} MiB above the inputs and the held workspace; "
          f"bound {bound / 2**20:.1f} MiB = Z {8 * n * P / 2**20:.1f} + sims {8 * R * P / 2**20:.1f} + workspace "
          f"{ws_bytes / 2**20:.1f} + graph {graph_bytes / 2**20:.2f}; a permuted copy per permutation would be "
          f"{8 * n * P * R / 2**20:.0f} MiB")
    assert tuple(res.sims.shape) == (R, P) and bool(torch.isfinite(res.I).all())
    assert peak <= bound, (peak, bound)
