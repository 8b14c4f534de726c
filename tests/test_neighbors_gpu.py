"""Neighbour statistics on the device: the entries of csrc/neighbors.hip through the C ABI alone, then the calls of
spatial_alignment_amd/neighbors.py, against the numpy fp64 yardstick of tests/neighbors_util.py (itself held against
sklearn in tests/test_neighbors.py).

Bars (every comparison prints what it measures next to its bar):
* neighbour indices: EQUAL, position for position, on every row whose consecutive yardstick distances among the first
  k + 1 differ by more than 1e-12 relative (the kernel's fp64 differs from numpy's by fused multiply-adds only); with the
  seeds used the smallest such gap is 8e-7, so no row is set aside - asserted before comparing;
* d2: 1e-13 relative (D <= 4 fused multiply-adds at 1.1e-16 each);
* averages, regression: 1e-6 relative to max(1, |value|), the fp32 output's rounding (6e-8) with room;
* R^2 from those predictions: 1e-6 relative to max(1, |value|) (a ratio of sums of squares of values carrying 6e-8);
* Moran's I, its variance and z: 1e-9 absolute against the dense fp64 yardstick (the lag is accumulated and stored in fp64).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import neighbors_util as nu
import spatial_alignment_amd as gp
from golden_io import Golden
from model_util import build_model
from spatial_alignment_amd import neighbors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64, f32 = torch.float64, torch.float32
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
# (nq, nr, D, k, self-excluded): the sizes cross the 256-thread block and the 512-row LDS tile
SHAPES = [(1000, 1000, 2, 10, True), (777, 1301, 2, 32, False), (300, 515, 3, 10, False), (257, 600, 4, 1, False),
          (500, 500, 1, 6, True), (1, 40, 2, 3, False), (40, 11, 2, 10, True)]


def _lib():
    from spatial_alignment_amd import _lib as L

    return L.load()


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _dev(a, dt=f64):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _points(case):
    """the case's seeded uniform points in [0, 10]^D with the yardstick's k + 1 neighbours (computed once, shared, never
    changed).  Self-excluded: the queries are the references (and further points where nq > nr)"""
    nq, nr, D, k, excl = SHAPES[case]
    rng = np.random.default_rng(case)
    R = rng.uniform(0, 10, (nr, D))
    Q = rng.uniform(0, 10, (nq, D))
    if excl:
        Q[: min(nq, nr)] = R[: min(nq, nr)]
    idx, d2 = nu.knn(Q, R, k, exclude_self=excl, extra=1)
    return Q, R, idx, d2


def _knn_raw(Q, R, k, excl=False, parts=0, short=0, D=None, same=False):
    """gpsa_knn_f64 through ctypes -> (rc, idx, d2) on the host; outputs pre-filled with -7 / NaN.  ``same``: Q and R are
    one device array (the leave-one-out contract); ``short``: bytes withheld from the workspace size passed"""
    lib = _lib()
    Rd = _dev(R)
    Qd = Rd if same else _dev(Q)
    nq, nr = int(Qd.shape[0]), int(Rd.shape[0])
    D = int(Rd.shape[1]) if D is None else D
    idx = torch.full((nq, max(k, 1)), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((nq, max(k, 1)), float("nan"), dtype=f64, device=DEV)
    nbytes = int(lib.gpsa_knn_workspace(nq, nr, k, parts))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=DEV)
    rc = lib.gpsa_knn_f64(Qd.data_ptr(), nq, Rd.data_ptr(), nr, D, k, int(excl), parts, idx.data_ptr(), d2.data_ptr(),
                          ws.data_ptr(), nbytes - short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), d2.cpu().numpy(), nbytes


# ------------------------------------------------------------------------------------------------------------------------
# 1. gpsa_knn_f64
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_knn_equals_the_yardstick(case):
    nq, nr, D, k, excl = SHAPES[case]
    Q, R, want_i, want_d = _points(case)
    clear = nu.rows_with_clear_order(want_d, k)
    gap = np.diff(want_d[:, : k + 1], axis=1) / np.maximum(want_d[:, 1: k + 1], 1e-300)
    print(f"[neighbors] case {case} {SHAPES[case]}: smallest relative gap among the first k + 1 "
          f"{gap.min() if gap.size else float('inf'):.1e}; rows set aside {int((~clear).sum())} of {nq}")
    assert int((~clear).sum()) == 0
    rc, idx, d2, _ = _knn_raw(Q, R, k, excl, same=excl and nq == nr)
    assert rc == 0
    assert np.array_equal(idx[clear], want_i[clear, :k])
    err = (np.abs(d2 - want_d[:, :k]) / np.maximum(want_d[:, :k], 1e-300)).max()
    print(f"[neighbors] case {case}: d2 {err:.2e} (bar 1e-13)")
    assert err <= 1e-13
    assert np.all(np.diff(d2, axis=1) >= 0)


@functools.lru_cache(maxsize=None)
def _lattice():
    X = nu.lattice()
    idx, d2 = nu.knn(X, X, 6, exclude_self=True, extra=1)
    return X, idx, d2


def test_ties_go_to_the_lower_index():
    X, want_i, want_d = _lattice()
    tied = int((want_d[:, 5] == want_d[:, 6]).sum())
    print(f"[neighbors] lattice 13 x 11: rows with a tie across the 6th place {tied} of {len(X)}")
    assert tied == len(X) == 143
    rc, idx, d2, _ = _knn_raw(X, X, 6, True, same=True)
    assert rc == 0 and np.array_equal(idx, want_i[:, :6]) and np.array_equal(d2, want_d[:, :6])


def test_the_result_does_not_depend_on_the_split():
    Q, R, _, _ = _points(1)
    X, _, _ = _lattice()
    for what, (q, r, k, excl) in (("(777, 1301, 2, 32)", (Q, R, 32, False)), ("lattice", (X, X, 6, True))):
        rc, i1, d1, nb1 = _knn_raw(q, r, k, excl, parts=1, same=excl)
        assert rc == 0 and nb1 == 0
        for parts in (2, 3, 7, 0, 1):
            rc, i, d, nb = _knn_raw(q, r, k, excl, parts=parts, same=excl)
            assert rc == 0 and (nb > 0 if parts > 1 else nb == 0 if parts == 1 else True)
            assert np.array_equal(i, i1) and np.array_equal(d.view(np.int64), d1.view(np.int64)), (what, parts)
    print("[neighbors] parts in {1, 2, 3, 7, 0} and a second run: the same bits")


def test_error_codes_come_back_without_a_launch():
    Q, R, _, _ = _points(2)
    untouched = lambda idx: bool((idx == -7).all())
    rc, idx, _, _ = _knn_raw(Q, R, 33)
    assert rc == EUNSUPPORTED and untouched(idx)
    rc, idx, _, _ = _knn_raw(Q, R, 3, D=5)
    assert rc == EUNSUPPORTED and untouched(idx)
    rc, idx, _, _ = _knn_raw(Q, R[:7], 8)
    assert rc == EINVAL and untouched(idx)
    rc, idx, _, _ = _knn_raw(R[:8], R[:8], 8, True, same=True)  # 7 other points
    assert rc == EINVAL and untouched(idx)
    for k, D in ((0, None), (3, 0)):
        rc, idx, _, _ = _knn_raw(Q, R, k, D=D)
        assert rc == EINVAL and untouched(idx)
    rc, idx, _, nbytes = _knn_raw(Q, R, 10, parts=2, short=8)
    assert nbytes >= 8 and rc == EWORKSPACE and untouched(idx)
    rc, idx, _, _ = _knn_raw(Q, R, 10, parts=2)
    assert rc == 0 and not untouched(idx)
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    z = torch.zeros(64, dtype=f64, device=DEV)
    p = z.data_ptr()
    assert lib.gpsa_knn_f64(0, 4, p, 4, 2, 1, 0, 0, p, p, 0, 0, st) == EINVAL
    assert lib.gpsa_knn_average_f32(p, 0, 4, 1, p, 4, 2, 1, p, st) == EINVAL  # inverse distance without d2
    assert lib.gpsa_knn_average_f32(p, p, 4, 1, p, 4, 2, 2, p, st) == EINVAL  # an unknown weighting
    assert lib.gpsa_knn_average_f32(p, p, 4, 0, p, 4, 2, 0, p, st) == EINVAL
    assert lib.gpsa_knn_average_f32(p, 0, 4, 1, 0, 4, 2, 0, p, st) == EINVAL
    torch.cuda.synchronize()


def test_new_kernels_have_no_scratch_and_no_spills():
    """register allocation of every kernel of csrc/neighbors.hip, read from the code objects inside the built library: a
    top-k list indexed at run time would show here as scratch"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from kernel_meta import demangle, library_kernels

    from spatial_alignment_amd import _lib as L

    ks = library_kernels(L.LIB_PATH)
    mine = [(n, k) for n, k in zip(demangle([k["name"] for k in ks]), ks)
            if "knn_scan_kernel<" in n or "knn_merge_kernel<" in n or "knn_average_kernel<" in n]
    assert len(mine) == 6 * 4 * 2 + 6 + 2 * 3 * 2, [n for n, _ in mine]  # K x D x direct + K + type x width x weights
    for n, k in mine:
        assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
        assert k["lds"] <= 16 * 1024, (n, k)


# ------------------------------------------------------------------------------------------------------------------------
# 2. gpsa_knn_average_f32
# ------------------------------------------------------------------------------------------------------------------------
def _avg_err(got, want):
    got = got.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float((np.abs(got - want)[ok] / np.maximum(1.0, np.abs(want[ok]))).max()) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def _avg_points():
    rng = np.random.default_rng(100)
    R, Q = rng.uniform(0, 10, (400, 2)), rng.uniform(0, 10, (257, 2))
    idx, d2 = nu.knn(Q, R, 10)
    Y = rng.normal(size=(400, 130)).astype(np.float32)
    return idx, d2, Y


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_knn_average_equals_the_yardstick(weights):
    idx, d2, Y = _avg_points()
    o, worst = _ops(), 0.0
    for P in (1, 3, 50, 130):
        for nq in (1, 257):
            for k in (1, 10):
                i, d, y = idx[:nq, :k], d2[:nq, :k], np.ascontiguousarray(Y[:, :P])
                got = o.knn_average(_dev(i, torch.int32), _dev(d) if weights == "distance" else None, _dev(y, f32), weights)
                assert got.dtype == f32 and tuple(got.shape) == (nq, P)
                worst = max(worst, _avg_err(got, nu.average(i, d, y, weights)))
    print(f"[neighbors] knn_average {weights}: largest error {worst:.2e} (bar 1e-06)")
    assert worst <= 1e-6


def test_knn_average_with_zero_distances_and_missing_entries():
    rng = np.random.default_rng(101)
    R = rng.uniform(0, 10, (200, 2))
    R[100:110] = R[:10]  # ten duplicated points ...
    Q = R[:10]  # ... queried at their own location: two zero distances per row
    idx, d2 = nu.knn(Q, R, 10)
    assert ((d2 == 0).sum(1) == 2).all()
    Y = rng.normal(size=(200, 50)).astype(np.float32)
    o = _ops()
    for w in ("uniform", "distance"):
        got = o.knn_average(_dev(idx, torch.int32), _dev(d2), _dev(Y, f32), w)
        e = _avg_err(got, nu.average(idx, d2, Y, w))
        print(f"[neighbors] knn_average {w}, duplicated points: {e:.2e} (bar 1e-06)")
        assert e <= 1e-6
    want = 0.5 * (Y[:10].astype(np.float64) + Y[100:110])  # exactly the two zero-distance neighbours
    assert np.abs(o.knn_average(_dev(idx, torch.int32), _dev(d2), _dev(Y, f32), "distance").cpu().numpy() - want).max() <= 1e-6
    # 10 % NaN, and one row whose neighbours are all NaN
    Yn = Y.copy()
    Yn[rng.random(Yn.shape) < 0.1] = np.nan
    Yn[idx[0]] = np.nan
    for w in ("uniform", "distance"):
        got = o.knn_average(_dev(idx, torch.int32), _dev(d2), _dev(Yn, f32), w)
        want = nu.average(idx, d2, Yn, w)
        assert np.isnan(want[0]).all() and bool(torch.isnan(got[0]).all()) and not np.isnan(want[1:]).all()
        e = _avg_err(got, want)
        print(f"[neighbors] knn_average {w}, 10 % NaN: {e:.2e} (bar 1e-06); NaN results {int(np.isnan(want).sum())}")
        assert e <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------
# 3. the calls
# ------------------------------------------------------------------------------------------------------------------------
def test_knn_does_not_depend_on_rows_per_chunk():
    Q, R, want_i, _ = _points(0)
    X = _dev(R, f32).double()  # any float dtype is taken to fp64
    whole = neighbors.knn(X)
    assert whole.idx.dtype == torch.int32 and whole.dist.dtype == f64 and tuple(whole.idx.shape) == (1000, 10)
    assert torch.equal(whole.dist, whole.d2.sqrt())
    part = neighbors.knn(X, rows_per_chunk=100)
    assert torch.equal(whole.idx, part.idx) and torch.equal(whole.d2, part.d2)
    r = neighbors.knn(_dev(R), rows_per_chunk=333)
    assert np.array_equal(r.idx.cpu().numpy(), want_i[:, :10])  # each chunk leaves out its own rows
    Qd, Rd = _dev(_points(1)[0]), _dev(_points(1)[1])
    a, b = neighbors.knn(Qd, Rd, k=32), neighbors.knn(Qd, Rd, k=32, rows_per_chunk=100)
    assert torch.equal(a.idx, b.idx) and torch.equal(a.d2, b.d2)
    assert np.array_equal(a.idx.cpu().numpy(), _points(1)[2][:, :32])
    i2, d2 = torch.ops.gpsa.knn(Qd, Rd, 32)
    assert torch.equal(i2, a.idx) and torch.equal(d2, a.d2)


@functools.lru_cache(maxsize=None)
def _field():
    """300 points with three outputs, fp32-representable: a smooth field plus noise, pure noise, a constant column"""
    rng = np.random.default_rng(200)
    X = rng.uniform(0, 10, (300, 2))
    smooth = np.sin(X[:, 0] / 2.0) + np.cos(X[:, 1] / 3.0) + 0.1 * rng.normal(size=300)
    Y = np.stack([smooth, rng.normal(size=300), np.full(300, 1.75)], 1).astype(np.float32).astype(np.float64)
    return X, Y


def _same(a, b):
    """the same bits, NaN in the same places"""
    return torch.equal(torch.nan_to_num(a, nan=-77.0), torch.nan_to_num(b, nan=-77.0))


def _rel1(got, want):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    return float((np.abs(got - want)[ok] / np.maximum(1.0, np.abs(want[ok]))).max())


def test_regression_scores_equal_the_yardstick():
    X, Y = _field()
    rng = np.random.default_rng(201)
    T = rng.uniform(0, 10, (77, 2))
    Xd, Yd, Td = _dev(X), _dev(Y, f32), _dev(T)
    for w in ("uniform", "distance"):
        got = neighbors.knn_regress(Xd, Yd, Td, k=10, weights=w)
        assert got.dtype == f32 and tuple(got.shape) == (77, 3)
        e = _rel1(got, nu.regress(X, Y, T, 10, w))
        assert torch.equal(got, neighbors.knn_regress(Xd, Yd, Td, k=10, weights=w, rows_per_chunk=20))
        loo = neighbors.knn_regress(Xd, Yd, k=10, weights=w, exclude_self=True, rows_per_chunk=128)
        e2 = _rel1(loo, nu.regress(X, Y, X, 10, w, exclude_self=True))
        r2 = neighbors.spatial_r2(Xd, Yd, k=10, weights=w)
        want = nu.r2(Y, nu.regress(X, Y, X, 10, w, exclude_self=True))
        assert r2.dtype == f64 and np.isnan(want[2]) and want[0] > 0.8 and want[1] < 0.2
        e3 = _rel1(r2, want)
        print(f"[neighbors] {w}: knn_regress {e:.2e}, leave-one-out {e2:.2e}, spatial_r2 {e3:.2e} (bars 1e-06); "
              f"R2 of the smooth / noise columns {want[0]:.3f} / {want[1]:.3f}")
        assert e <= 1e-6 and e2 <= 1e-6 and e3 <= 1e-6
    d = neighbors.kth_neighbor_distance(Xd, k=10)
    want = np.sqrt(nu.knn(X, X, 10, exclude_self=True)[1][:, 9])
    e = float((np.abs(d.cpu().numpy() - want) / want).max())
    print(f"[neighbors] kth_neighbor_distance {e:.2e} (bar 1e-13)")
    assert d.dtype == f64 and tuple(d.shape) == (300,) and e <= 1e-13


@pytest.mark.parametrize("standardize", [True, False])
def test_morans_i_equals_the_dense_yardstick(standardize):
    X, Y = _field()
    want = nu.moran(X, Y, 6, standardize)
    got = neighbors.moran_i(_dev(X), _dev(Y, f32), k=6, row_standardize=standardize)
    chunked = neighbors.moran_i(_dev(X), _dev(Y), k=6, row_standardize=standardize, rows_per_chunk=64)
    assert all(_same(got[name], chunked[name]) for name in ("I", "variance", "z"))
    errs = {}
    for name in ("I", "expected", "variance", "z", "p_norm"):
        g = got[name].cpu().numpy()
        assert got[name].dtype == f64 and g.shape == (3,)
        assert np.array_equal(np.isnan(g), np.isnan(want[name])), name
        ok = ~np.isnan(want[name])
        errs[name] = float(np.abs(g - want[name])[ok].max())
    print(f"[neighbors] moran_i row_standardize={standardize}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f" (bar 1e-09); I = {want['I'][0]:.4f} / {want['I'][1]:.4f}, z = {want['z'][0]:.2f} / {want['z'][1]:.2f}")
    assert all(v <= 1e-9 for v in errs.values()), errs
    assert np.isnan(want["I"][2]) and np.isnan(want["z"][2])  # the constant column
    assert want["I"][0] > 0.5 and abs(want["z"][1]) < 4


# ------------------------------------------------------------------------------------------------------------------------
# 4. the alignment score
# ------------------------------------------------------------------------------------------------------------------------
def _rows(model, m, v):
    r = model.view_idx[m][v]
    return np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.int64)


def _want_scores(coords, Ys, k, V, P):
    r2, pr = np.full((V, V, P), np.nan), np.full((V, V, P), np.nan)
    for a in range(V):
        for b in range(V):
            if a != b and coords[a] is not None and coords[b] is not None:
                pred = nu.regress(coords[a], Ys[a], coords[b], k)
                r2[a, b], pr[a, b] = nu.r2(Ys[b], pred), nu.pearson(Ys[b], pred)
    return r2, pr


@pytest.mark.parametrize("name", ["c1_example_fixed0", "c2_three_free_views", "c10_unequal_two_fixed"])
def test_alignment_score_equals_the_yardstick_on_the_warp_field(name):
    g = Golden(name)
    model, dd = build_model(g, device=DEV)
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    Y = {m: dd[m]["outputs"] for m in g.mods}
    V = int(model.n_views)
    k = min(5, min(len(_rows(model, m, v)) for m in g.mods for v in range(V) if len(_rows(model, m, v))))
    res = model.alignment_score(X, Y, k=k)
    Gfull = {}
    for m in g.mods:
        Xm, Ym = X[m].double().cpu().numpy(), Y[m].float().cpu().numpy().astype(np.float64)
        P = Ym.shape[1]
        Gm = torch.empty_like(X[m], dtype=f64)
        native, aligned, Ys = [], [], []
        for v in range(V):
            rows = _rows(model, m, v)
            if not len(rows):
                native.append(None), aligned.append(None), Ys.append(None)
                continue
            Gv = model.warp_field(X[m][rows], v, jacobian=False).G_mean
            if model._is_fixed(v):
                assert torch.equal(Gv, X[m][rows].double())
            Gm[rows] = Gv
            native.append(Xm[rows]), aligned.append(Gv.cpu().numpy()), Ys.append(Ym[rows])
        Gfull[m] = Gm
        r = res[m]
        assert tuple(r.r2.shape) == (V, V, P) and tuple(r.r2_mean.shape) == (V, V) and r.r2.dtype == f64
        want_r2, want_pr = _want_scores(aligned, Ys, k, V, P)
        raw_r2, raw_pr = _want_scores(native, Ys, k, V, P)
        errs = [_rel1(r.r2, want_r2), _rel1(r.pearson, want_pr), _rel1(r.r2_raw, raw_r2), _rel1(r.pearson_raw, raw_pr)]
        with np.errstate(invalid="ignore"):
            mean = np.array([[np.nanmean(want_r2[a, b]) if (~np.isnan(want_r2[a, b])).any() else np.nan
                              for b in range(V)] for a in range(V)])
        errs.append(_rel1(r.r2_mean, mean))
        print(f"[neighbors] alignment_score {name} {m} (k = {k}): r2 {errs[0]:.2e}, pearson {errs[1]:.2e}, raw "
              f"{errs[2]:.2e} / {errs[3]:.2e}, r2_mean {errs[4]:.2e} (bar 1e-06)")
        assert max(errs) <= 1e-6
        assert bool(torch.isnan(torch.diagonal(r.r2, dim1=0, dim2=1)).all())
    given = gp.alignment_score(model, X, Y, k=k, G=Gfull, raw=False)
    for m in g.mods:
        assert _same(given[m].r2, res[m].r2) and _same(given[m].pearson, res[m].pearson)
        assert _same(given[m].r2_mean, res[m].r2_mean)
        assert "r2_raw" not in given[m] and "r2_mean_raw" not in given[m] and "pearson_raw" not in given[m]


def test_a_fit_raises_the_alignment_score_of_the_simulated_lattice():
    """the wiring end to end, a sign and nothing more: two views of one lattice, view 1 warped, 300 steps"""
    from spatial_alignment_amd import simulate
    from spatial_alignment_amd.synthetic import make_model
    from spatial_alignment_amd.train import fit

    torch.manual_seed(0)
    X, Y, nsl, _ = simulate.generate_twod_data(2, 10, 20, noise_variance=0.01, fixed_view_idx=0, seed=0)
    dd = simulate.as_data_dict(X, Y, nsl)
    model = make_model(dd, m=25, fixed_view_idx=0, device=torch.device(DEV))
    dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(DEV), outputs=d["outputs"].to(DEV)) for m, d in dd.items()}
    fit(model, dd, 300, lr=1e-2, S=3, sync_every=100)
    m = model.modality_names[0]
    s = model.alignment_score({m: dd[m]["spatial_coords"]}, {m: dd[m]["outputs"]})[m]
    print(f"[neighbors] simulated lattice after 300 steps: r2_mean[0, 1] {float(s.r2_mean_raw[0, 1]):.4f} -> "
          f"{float(s.r2_mean[0, 1]):.4f}; [1, 0] {float(s.r2_mean_raw[1, 0]):.4f} -> {float(s.r2_mean[1, 0]):.4f}")
    assert float(s.r2_mean[0, 1]) > float(s.r2_mean_raw[0, 1])
