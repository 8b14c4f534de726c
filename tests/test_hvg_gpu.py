"""Highly variable genes on the device: the two entries of csrc/moments.hip through ``ops`` / ``torch.ops.gpsa.*`` and the
calls of spatial_alignment_amd/counts.py on them (``column_moments``, ``highly_variable_genes``, ``prepare_counts(selection=
"seurat")``), dense and CSR, against the fp64 numpy yardstick of tests/hvg_util.py (itself held against pandas in
tests/test_hvg.py).

The kernels' constants (csrc/moments.hip; tests/test_hvg.py holds the Python copies to the source): a row group has at
least MOM_ROWS_MIN = 16 rows; a view is cut into at most MOM_MAX_GROUPS = 512 groups by the dense walk (the groups grow
beyond N = 8192) and MOM_CSR_MAX_GROUPS = 16 by the CSR walk (beyond N = 256); a column tile is MOM_COL_TILE = 512 columns;
a wave is 64 lanes (the CSR walk's chunk of a row, the fold's columns per workgroup), a workgroup 4 waves; the dense walk
loads 16 bytes per lane where P % 4 == 0.  SHAPES puts N and P on both sides of each, with V = 1, 2, 3, view boundaries
that are no multiple of 16, a view of exactly 2 rows, P = 1 and N = 2; the largest is 1100 x 1100.  The CSR matrices
have their first and last row empty, a row that stores all P columns with its zeros, rows of exactly 1, 63, 64, 65,
255, 256 and 257 entries (P >= 300), a column no row stores, and (``keep``) a mask that empties whole row groups.

Bars:
* s1, s2, abs1: |err| <= 1e-11 x the yardstick's sum of the magnitudes of the terms (sum |t| for s1 and abs1, sum t^2 for
  s2) - the counts suites' bar for their fp64 sums; the same bits on a repeated call; integer counts in mode 0: s1
  ``torch.equal`` between the dense and the CSR entry; n_nonfinite EQUAL;
* means, dispersions, dispersions_norm (highly_variable_genes on every case below, prepare_counts' dispersions_norm):
  |err| <= DERIVED_BAR max(1, |value|).  Measured on the MI355X over this suite: at most 3.35e-14 (1100 x 1100, three
  views, "normalize"); the bar is 100 x that, 3.4e-12 - far inside 1e-8, the whole-call bar of the GPR and warp suites;
* highly_variable, genes, and prepare_counts' rows / genes: EQUAL to the yardstick's, on inputs where the yardstick is
  decisive (asserted on the CPU first: no ``means`` within 1e-9 of the range of an interior bin edge, the normalised
  dispersions on both sides of the cutoff more than 1e-6 apart, exact ties excepted); prepare_counts' outputs
  ``torch.equal`` between the dense and the sparse route, and within 1e-6 max(1, |value|) of the yardstick's (fp32).
"""
import functools

import numpy as np
import pytest
import torch

import counts_util as cu
import hvg_util as hu
import spatial_alignment_amd as gp
from spatial_alignment_amd import counts
from test_counts_sparse import memory_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64, f32, i64, i32 = torch.float64, torch.float32, torch.int64, torch.int32
RM, MG, CG, CT = counts.MOM_ROWS_MIN, counts.MOM_MAX_GROUPS, counts.MOM_CSR_MAX_GROUPS, counts.MOM_COL_TILE
SUM_BAR, DERIVED_BAR = 1e-11, 3.4e-12
SHAPES = [(2, 1, [2]), (3, 4, [3]), (33, 65, [33]), (33, 65, [2, 31]), (97, 45, [40, 2, 55]),
          (RM - 1, CT - 1, [RM - 1]), (RM, CT, [RM]), (RM + 1, CT + 1, [7, RM - 6]),       # one group / a second; one tile / two
          (RM * CG - 1, 2 * CT - 1, [100, 155]), (RM * CG, 2 * CT, [RM * CG]),             # the CSR walk's 16 groups ...
          (RM * CG + 1, 2 * CT + 1, [17, 100, 140]),                                       # ... and groups of 17 rows
          (5, 4 * CT + 1, [2, 3]), (9, CT + 4, [4, 5]),                                    # many tiles; the 16-byte loads
          (RM * MG + 5, 3, [RM * MG + 5]), (RM * MG - 1, 2, [5000, RM * MG - 5001]),       # the dense walk's 512 groups
          (1100, 1100, [500, 333, 267])]
IDS = [f"{n}x{p} V={len(ns)}" for n, p, ns in SHAPES]
ROW_LENGTHS = (1, 63, 64, 65, 255, 256, 257)
HVG_CASES = [((257, 130), [257], 25), ((257, 130), [120, 137], 25), ((300, 200), [80, 90, 130], None),
             ((1100, 1100), [500, 333, 267], 150)]


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _lib():
    from spatial_alignment_amd import _lib as L

    return L.load()


def _dev(a, dt=f32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _csr_parts(Yh, stored=None):
    mask = Yh != 0
    if stored is not None:
        mask = mask | stored
    crow = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
    return _dev(crow, i64), _dev(np.nonzero(mask)[1], i32), _dev(Yh[mask]), mask


@functools.lru_cache(maxsize=None)
def _counts(N, P):
    """the recipe's counts at a negative depth (sparse); first and last row empty, one row that will store its zeros, one
    column nobody stores (P >= 8) -> (Y, stored); computed once, shared, never changed"""
    Y = cu.recipe(N, P, seed=N * 31 + P, depth=-1.0, zero_column=False)
    stored = np.zeros((N, P), bool)
    if N >= 8:
        Y[0] = 0.0
        Y[N - 1] = 0.0
        stored[3] = True  # a row that stores all P columns, its zeros included
    if N >= 16 and P >= 300:  # rows of exactly these many entries: the wave (64) is the chunk a row is read in and the
        rng = np.random.default_rng(N * 7 + P)  # size below which a row's tile start is not searched for; 256 = 4 chunks
        for r, n in enumerate(ROW_LENGTHS, start=4):
            Y[r] = 0.0
            Y[r, rng.choice(np.setdiff1d(np.arange(P), [5]), n, replace=False)] = rng.integers(1, 300, n)
    if P >= 8:
        Y[:, 5] = 0.0
        stored[:, 5] = False
    assert Y.max() < 2**24
    Y.setflags(write=False)
    stored.setflags(write=False)
    return Y, stored


def _input(N, P, ns, mode):
    """what each mode reads, as fp32 holds it -> (X fp64, scale or None)"""
    Y, _ = _counts(N, P)
    if mode == "normalize":
        return Y, hu.scale_of(Y.sum(1)) if Y.sum() > 0 else np.zeros(N)
    X = cu.normalize_log1p(Y) if Y.sum() > 0 else Y
    if mode == "identity":  # transformed data of both signs
        X = X - X.mean(0, keepdims=True) * (np.arange(P) % 2)[None, :]
    return X.astype(np.float32).astype(np.float64), None


def _check_sums(got, want, X, ns, mode, scale, keep=None, stored=None, what=""):
    s1, s2, ab, bad = (t.cpu().numpy() for t in got)
    assert s1.shape == s2.shape == ab.shape == (len(ns), X.shape[1]) and s1.dtype == np.float64
    worst = 0.0
    for g, key, scale_key in ((s1, "s1", "abs1"), (s2, "s2", "s2"), (ab, "abs1", "abs1")):
        err = np.abs(g - want[key])
        bar = SUM_BAR * want[scale_key]
        assert (err <= bar).all(), (what, key, float((err - bar).max()))
        worst = max(worst, float((err / np.maximum(want[scale_key], 1e-300)).max()))
    assert int(bad[0]) == want["n_nonfinite"] == 0, what
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# the kernels' sums
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,ns", SHAPES, ids=IDS)
def test_sums_equal_the_yardstick_dense_and_csr(N, P, ns):
    o, off = _ops(), [int(v) for v in hu.offsets(ns)]
    _, stored = _counts(N, P)
    worst = 0.0
    for mode in hu.MODES:
        X, scale = _input(N, P, ns, mode)
        want = hu.sums(X, ns, mode, scale)
        sc = None if scale is None else _dev(scale, f64)
        D = _dev(X)
        got = o.column_moments(D, mode, off, sc)
        worst = max(worst, _check_sums(got, want, X, ns, mode, scale, what=f"dense {mode}"))
        again = torch.ops.gpsa.column_moments(D, mode, off, sc)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), mode  # the same bits on a repeated call
        crow, col, val, _ = _csr_parts(X, stored)
        got_c = o.column_moments_csr(crow, col, val, N, P, mode, off, sc)
        worst = max(worst, _check_sums(got_c, want, X, ns, mode, scale, what=f"csr {mode}"))
        again = torch.ops.gpsa.column_moments_csr(crow, col, val, N, P, mode, off, sc)
        assert all(torch.equal(a, b) for a, b in zip(got_c, again)), mode
    # integer counts in mode 0: exact sums, the same bits from both entries
    Y, _ = _counts(N, P)
    crow, col, val, _ = _csr_parts(Y, stored)
    d, c = o.column_moments(_dev(Y), "identity", off), o.column_moments_csr(crow, col, val, N, P, "identity", off)
    assert torch.equal(d[0], c[0]) and torch.equal(d[1], c[1]) and torch.equal(d[2], c[2])
    assert np.array_equal(d[0].cpu().numpy(), hu.sums(Y, ns, "identity")["s1"])
    print(f"[hvg] {N} x {P}, V = {len(ns)}: sums vs the yardstick {worst:.2e} of the terms' magnitudes (bar {SUM_BAR:g})")


@pytest.mark.parametrize("N,P,ns", [(RM * CG + 1, 2 * CT + 1, [17, 100, 140]), (97, 45, [40, 2, 55])], ids=["257x1025", "97x45"])
def test_a_keep_mask_that_empties_whole_row_groups(N, P, ns):
    o, off = _ops(), [int(v) for v in hu.offsets(ns)]
    _, stored = _counts(N, P)
    keep = np.random.default_rng(N).random(N) < 0.7
    keep[: 2 * RM + 3] = False  # the first groups of the first views: nothing left in them
    keep[-1] = True
    for mode in hu.MODES:
        X, scale = _input(N, P, ns, mode)
        want = hu.sums(X, ns, mode, scale, keep=keep)
        crow, col, val, _ = _csr_parts(X, stored)
        got = o.column_moments_csr(crow, col, val, N, P, mode, off, None if scale is None else _dev(scale, f64),
                                   _dev(keep, torch.bool))
        _check_sums(got, want, X, ns, mode, scale, what=f"keep {mode}")
        assert np.array_equal(got[0].cpu().numpy()[0] == 0, want["s1"][0] == 0)


def test_non_finite_values_are_counted():
    """one NaN and one value whose expm1 overflows (fp32 800: e^800 is beyond fp64); an infinite scale on a row of a
    matrix whose width is no multiple of the column tile counts that row's P entries, not the tile's padding"""
    o = _ops()
    N, P = 40, 70
    Y = np.array(_counts(N, P)[0]) + 1.0
    Y[7, 3], Y[20, 69] = np.nan, 800.0
    scale = hu.scale_of(np.nansum(Y, 1))
    want = {"identity": 1, "expm1": 2, "normalize": 1}
    for ns in ([N], [13, 27]):
        off = [int(v) for v in hu.offsets(ns)]
        for mode, n_bad in want.items():
            sc = _dev(scale, f64) if mode == "normalize" else None
            crow, col, val, _ = _csr_parts(Y)
            for got in (o.column_moments(_dev(Y), mode, off, sc), o.column_moments_csr(crow, col, val, N, P, mode, off, sc)):
                assert int(got[3].item()) == n_bad == hu.sums(Y, ns, mode, scale)["n_nonfinite"], (mode, ns)
                s1 = got[0].cpu().numpy()
                ok = np.ones(P, bool)
                ok[3] = False
                ok[69] = mode != "expm1"
                assert np.isfinite(s1[:, ok]).all() and not np.isfinite(s1[:, ~ok]).all(0).any()
    scale[11] = np.inf
    Yz = np.array(Y)
    Yz[7, 3], Yz[20, 69] = 1.0, 1.0
    Yz[11, ::2] = 0.0  # 0 x inf: NaN, also non-finite; the CSR entry does not see the unstored zeros
    crow, col, val, mask = _csr_parts(Yz)
    assert int(o.column_moments(_dev(Yz), "normalize", [0, N], _dev(scale, f64))[3].item()) == P
    assert int(o.column_moments_csr(crow, col, val, N, P, "normalize", [0, N], _dev(scale, f64))[3].item()) == int(mask[11].sum())
    res = gp.column_moments(_dev(Y), transform="expm1")
    assert res.n_nonfinite == 2 and bool(torch.isnan(res.mean[0, 3])) and bool(torch.isinf(res.mean[0, 69]))


def test_the_ops_refuse_what_the_entries_would():
    o = _ops()
    Y = _dev(np.ones((6, 5)))
    for off in ([0, 6, 6], [1, 6], [0, 5], [0, 4, 3, 6], [0]):
        with pytest.raises(ValueError, match="view_off"):
            o.column_moments(Y, "identity", off)
    with pytest.raises(ValueError, match="mode must be one of"):
        o.column_moments(Y, "log", [0, 6])
    with pytest.raises(ValueError, match="needs scale"):
        o.column_moments(Y, "normalize", [0, 6])
    with pytest.raises(ValueError, match="needs scale"):
        o.column_moments(Y, "normalize", [0, 6], torch.ones(5, dtype=f64, device=DEV))


# ------------------------------------------------------------------------------------------------------------------------
# the public calls: moments, ranking, selection
# ------------------------------------------------------------------------------------------------------------------------
def _hvg_inputs(shape, ns, transform):
    N, P = shape
    Y = cu.recipe(N, P, seed=N + 3 * P, depth=-0.5)
    Y[:, 0] += 1.0  # no row without counts
    if transform == "normalize":
        return Y, Y, hu.scale_of(Y.sum(1))
    return Y, cu.normalize_log1p(Y).astype(np.float32).astype(np.float64), None


def _assert_decisive(want, mask, n_top, n_bins=20):
    for r in want["views"]:
        near, gap = hu.decisive(r, mask, n_top, n_bins)
        assert near > 1e-9 and gap > 1e-6, (near, gap)


def _derived_error(got, want):
    worst = 0.0
    for key in ("means", "dispersions", "dispersions_norm"):
        g, w = got[key].cpu().numpy(), want[key]
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), key
        fin = ~np.isnan(w)
        worst = max(worst, float((np.abs(g[fin] - w[fin]) / np.maximum(1.0, np.abs(w[fin]))).max()))
    return worst


@pytest.mark.parametrize("transform", ["expm1", "normalize"])
@pytest.mark.parametrize("shape,ns,n_top", HVG_CASES, ids=[f"{s[0]}x{s[1]} V={len(ns)} top={t}" for s, ns, t in HVG_CASES])
def test_highly_variable_genes_equal_the_yardstick(shape, ns, n_top, transform):
    Y, X, scale = _hvg_inputs(shape, ns, transform)
    mask = (Y > 0).sum(0) >= 10
    assert 0.3 * shape[1] < mask.sum() < shape[1]
    crow, col, val, _ = _csr_parts(X)
    A = gp.csr_counts((crow, col, val, X.shape))
    worst = 0.0
    for gene_mask, combine in ((None, "intersection"), (mask, "union")):
        want = hu.hvg(X, ns, transform, scale, mask=gene_mask, combine=combine, n_top_genes=n_top)
        _assert_decisive(want, gene_mask, n_top)
        assert 0 < len(want["genes"]) < shape[1]
        kw = dict(transform=transform, n_top_genes=n_top, combine=combine,
                  gene_mask=None if gene_mask is None else _dev(gene_mask, torch.bool))
        for arg in (_dev(X), A):
            got = gp.highly_variable_genes(arg, ns, **kw)
            worst = max(worst, _derived_error(got, want))
            assert got.n_nonfinite == 0 and got.highly_variable.dtype == torch.bool and got.genes.dtype == i64
            assert np.array_equal(got.highly_variable.cpu().numpy(), want["highly_variable"])
            assert np.array_equal(got.genes.cpu().numpy(), want["genes"])
        mom = gp.column_moments(A, ns, transform=transform)
        assert float((np.abs(mom.mean.cpu().numpy() - want["mean"]) / np.maximum(1.0, np.abs(want["mean"]))).max()) <= 1e-12
        assert float((np.abs(mom.var.cpu().numpy() - want["var"]) / np.maximum(1.0, np.abs(want["var"]))).max()) <= 1e-10
    print(f"[hvg] {shape} V = {len(ns)} {transform}: means / dispersions / dispersions_norm vs the yardstick {worst:.2e} "
          f"(bar {DERIVED_BAR:g})")
    assert worst <= DERIVED_BAR


def test_the_variance_filter_on_transformed_data_and_scipy_input():
    """mode "identity" on z-scored log-counts (both signs): the experiments' ``X.var(0) > 0.1`` per slice"""
    sp = pytest.importorskip("scipy.sparse")
    Y, X, _ = _hvg_inputs((300, 200), [130, 170], "expm1")
    ns = [130, 170]
    Z = (X - X.mean(0)).astype(np.float32).astype(np.float64)
    got = gp.column_moments(_dev(Z), ns)
    want = np.stack([Z[:130].var(0, ddof=1), Z[130:].var(0, ddof=1)])
    assert float((np.abs(got.var.cpu().numpy() - want) / np.maximum(1.0, want)).max()) <= 1e-10
    assert np.array_equal((got.var > 0.1).cpu().numpy(), want > 0.1) and 0 < (want > 0.1).all(0).sum() < 200
    assert abs(want - 0.1).min() > 1e-6
    res = gp.column_moments(sp.csr_matrix(X), ns, transform="expm1")
    ref = gp.column_moments(_dev(X), ns, transform="expm1")
    assert float((res.mean - ref.mean).abs().max()) <= 1e-12 * float(ref.mean.abs().max())
    assert res.mean.device.type == "cuda" and res.n_nonfinite == 0


# ------------------------------------------------------------------------------------------------------------------------
# the one call
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [[120, 137], [80, 90, 87]], ids=["two views", "three views"])
@pytest.mark.parametrize("transform,n_top", [("log1p", 40), ("pearson", None), ("counts", 40), ("deviance", 40)])
def test_prepare_counts_seurat_dense_sparse_and_yardstick_agree(transform, n_top, ns):
    Yh = cu.recipe(257, 130, seed=77, depth=-0.5)
    Yh[:, 0] += 1.0
    kw = dict(min_counts=float(np.sort(Yh.sum(1))[5]), max_counts=float(np.sort(Yh.sum(1))[-4]), min_cells=30,
              n_top_genes=n_top, transform=transform, theta=50.0)
    want = hu.prepare_seurat(Yh, ns, **kw)
    near, gap = hu.decisive(want["seurat"], want["passed"], n_top, 20)
    assert near > 1e-9 and gap > 1e-6
    assert 200 < len(want["rows"]) < 257 and 10 < want["passed"].sum() < 130 and 5 < len(want["genes"]) < want["passed"].sum()
    crow, col, val, _ = _csr_parts(Yh)
    A, D = gp.csr_counts((crow, col, val, Yh.shape)), _dev(Yh)
    dense = gp.prepare_counts(D, ns, selection="seurat", **kw)
    for Y in (A, torch.sparse_csr_tensor(crow, col.to(i64), val, size=Yh.shape)):
        res = gp.prepare_counts(Y, ns, selection="seurat", **kw)
        assert torch.equal(res.rows, dense.rows) and torch.equal(res.genes, dense.genes)
        assert torch.equal(res.outputs, dense.outputs) and res.outputs.dtype == f32 and res.outputs.is_contiguous()
        assert res.n_samples_list == dense.n_samples_list == want["n_samples_list"] and res.deviance is None
        assert np.array_equal(res.rows.cpu().numpy(), want["rows"]) and np.array_equal(res.genes.cpu().numpy(), want["genes"])
        dn, wn = res.dispersions_norm.cpu().numpy(), want["dispersions_norm"]
        assert np.array_equal(np.isnan(dn), np.isnan(wn))
        worst = float((np.abs(dn - wn)[~np.isnan(wn)] / np.maximum(1.0, np.abs(wn[~np.isnan(wn)]))).max())
        print(f"[hvg] prepare_counts {transform} V = {len(ns)}: dispersions_norm vs the yardstick {worst:.2e} (bar {DERIVED_BAR:g})")
        assert worst <= DERIVED_BAR
        got = res.outputs.cpu().numpy().astype(np.float64)
        assert float((np.abs(got - want["outputs"]) / np.maximum(1.0, np.abs(want["outputs"]))).max()) <= 1e-6
        if transform == "counts":
            assert torch.equal(res.log_offset, dense.log_offset) and res.n_constant is None
            assert np.array_equal(got, Yh[want["rows"]][:, want["genes"]])
        else:
            assert torch.equal(res.n_constant, dense.n_constant)


def test_prepare_counts_deviance_route_is_unchanged():
    """the default selection returns what the existing yardstick's pipeline returns, on both routes"""
    Yh = cu.recipe(257, 130, seed=257 * 31 + 130, depth=-2.0)
    empty = np.nonzero(Yh.sum(1) == 0)[0]
    Yh[empty, 0] = 1.0
    ns = [120, 137]
    kw = dict(min_counts=float(np.sort(Yh.sum(1))[5]), max_counts=float(np.sort(Yh.sum(1))[-4]), min_cells=8,
              n_top_genes=40, transform="pearson", theta=50.0)
    want = cu.prepare(Yh, ns, **kw)
    assert cu.smallest_relative_gap(want["deviance"]) >= 1e-9
    crow, col, val, _ = _csr_parts(Yh)
    for Y in (_dev(Yh), gp.csr_counts((crow, col, val, Yh.shape))):
        for sel in ({}, dict(selection="deviance")):
            res = gp.prepare_counts(Y, ns, **kw, **sel)
            assert "dispersions_norm" not in res
            assert np.array_equal(res.rows.cpu().numpy(), want["rows"]) and np.array_equal(res.genes.cpu().numpy(), want["genes"])
            parts = cu.poisson_deviance(Yh[want["rows"]])
            bar = 1e-11 * (parts["abs_sat"] + np.abs(parts["ll_null"]))
            assert (np.abs(res.deviance.cpu().numpy() - want["deviance"]) <= bar).all()
            got = res.outputs.cpu().numpy().astype(np.float64)
            assert float((np.abs(got - want["outputs"]) / np.maximum(1.0, np.abs(want["outputs"]))).max()) <= 1e-6


def test_prepare_counts_seurat_stays_far_below_the_dense_matrix():
    """N = 4000, P = 20 000 at about 2 % density, generated on the device in row chunks: the peak allocation of
    prepare_counts(selection="seurat") above its inputs, the workspace held, stays below the bound the deviance route
    is held to (tests/test_counts_sparse.py: memory_bound)"""
    N, P, G = 4000, 20000, 200
    gen = torch.Generator(device=DEV).manual_seed(0)
    crow, cols, vals = [torch.zeros(1, dtype=i64, device=DEV)], [], []
    for a in range(0, N, 500):
        blk = (torch.rand(500, P, device=DEV, generator=gen) < 0.02).float()
        blk *= torch.randint(1, 9, (500, P), device=DEV, generator=gen)
        blk[:, 0] = 1.0  # no row without counts
        nz = blk.nonzero()  # row-major: sorted by row, then by column
        crow.append(torch.cumsum(torch.bincount(nz[:, 0], minlength=500), 0) + crow[-1][-1])
        cols.append(nz[:, 1].to(i32))
        vals.append(blk[nz[:, 0], nz[:, 1]])
        del blk, nz
    A = gp.csr_counts((torch.cat(crow), torch.cat(cols), torch.cat(vals), (N, P)))
    del crow, cols, vals
    assert 0.015 < A.nnz / (N * P) < 0.025
    bound = memory_bound(_lib(), N, P, N, G)
    assert 4 * N * P == 320_000_000 >= 10 * bound and bound <= 26.5 * 2**20
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = gp.prepare_counts(A, [2000, 2000], n_top_genes=G, transform="log1p", selection="seurat")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[hvg] prepare_counts(selection='seurat') {N} x {P}, nnz {A.nnz}: peak {peak / 2**20:.1f} MiB above the inputs, "
          f"bound {bound / 2**20:.1f} MiB, the dense matrix {4 * N * P / 2**20:.1f} MiB")
    assert tuple(res.outputs.shape) == (N, G) and bool(torch.isfinite(res.outputs).all())
    assert peak <= bound, (peak, bound)
