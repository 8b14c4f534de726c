"""Sparse count preprocessing on the device: the entries of csrc/counts_sparse.hip through the C ABI, through
``torch.ops.gpsa.*`` and through the calls of spatial_alignment_amd/counts.py on ``CSRCounts`` / ``torch.sparse_csr`` input,
against the fp64 numpy yardstick of tests/counts_util.py on the densified matrix and against the dense entries.

Bars (derived, none fitted; the counts are integers from ``counts_util.recipe`` with a negative depth):
* row / column sums, the counts of entries > 0, n_invalid, ``densify``: EQUAL, to the yardstick and to the dense entries
  (sums of integers are exact in fp64 in any order); ``prepare_counts``' outputs and log_offset EQUAL to the dense path's;
* ll_sat, abs_sat and the deviance: |err| <= 1e-11 (abs_sat_g + |ll_null_g|), the dense suite's bar;
* gene ORDER only where the yardstick's smallest relative gap between neighbouring deviances is >= 1e-9 (asserted).

Shapes: the dense suite's ``SHAPES`` at two densities, then EDGES: one matrix per (N, P) with
* N = 15, 16, 17: at, below and above CSR_ROWS_MIN (one group / a second group of one row); N = 511, 512, 513: the
  groups reach CSR_MAX_GROUPS = 32 at N = 512 and grow to 17 rows at 513;
* P = 511, 512, 513 and 1023, 1024, 1025: one and two column tiles of CSR_COL_TILE = 512 and one column more;
* first and last row empty; rows of exactly 1, 63, 64, 65, 255, 256, 257 entries: the wave (64) is the chunk a row is
  read in and the size below which the row's tile start is not searched for, 256 = 4 chunks;
* variant "full": a row that stores all P columns, explicit zeros among them; variant "hole": a column no row stores;
and for the gather, G = 8191, 8192, 8193 output columns around CSR_GATHER_TILE = 8192.
"""
import functools

import numpy as np
import pytest
import torch

import counts_util as cu
import spatial_alignment_amd as gp
from spatial_alignment_amd import counts
from test_counts_gpu import ORDERED, SHAPES
from test_counts_sparse import memory_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64, f32, i64, i32 = torch.float64, torch.float32, torch.int64, torch.int32
EINVAL, EWORKSPACE = -1, -2
RM, MG, CT, GT = counts.CSR_ROWS_MIN, counts.CSR_MAX_GROUPS, counts.CSR_COL_TILE, counts.CSR_GATHER_TILE
DEPTHS = (-2.0, -4.0)
CASES = [(s, d) for s in SHAPES for d in DEPTHS]
IDS = [f"{n}x{p} depth {d:g}" for (n, p), d in CASES]
EDGES = [(RM - 1, CT - 1), (RM, CT), (RM + 1, CT + 1), (RM * MG - 1, 2 * CT - 1), (RM * MG, 2 * CT), (RM * MG + 1, 2 * CT + 1)]
ROW_LENGTHS = (1, 63, 64, 65, 255, 256, 257)
# gene order is compared on the dense suite's ORDERED shapes at the first depth: no near-ties (asserted).  At the second
# depth (some 5 % density) genes with a single count in the same spot tie exactly, and the order is not compared.
ORDERED_CASES = [(s, DEPTHS[0]) for s in ORDERED]


def _lib():
    from spatial_alignment_amd import _lib as L

    return L.load()


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _dev(a, dt=f32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _csr_host(Yh, stored=None):
    """dense numpy -> (crow, col, val) numpy, rows sorted by column; ``stored``: a mask of further positions to store"""
    mask = Yh != 0
    if stored is not None:
        mask = mask | stored
    crow = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
    return crow, np.nonzero(mask)[1].astype(np.int64), Yh[mask]


def _csr(Yh, index=i64, stored=None):
    crow, col, val = _csr_host(Yh, stored)
    return gp.csr_counts((_dev(crow, index), _dev(col, index), _dev(val), Yh.shape))


@functools.lru_cache(maxsize=None)
def _data(shape, depth):
    """the recipe's counts at a negative depth, every empty row given one count (so that size factors exist); the
    yardstick's values, computed once, shared, never changed"""
    N, P = shape
    Y = cu.recipe(N, P, seed=N * 31 + P, depth=depth)
    empty = np.nonzero(Y.sum(1) == 0)[0]
    j = empty % P
    if P >= 3:
        j[j == P // 2] = 0  # the recipe's gene without counts stays without
    Y[empty, j] = 1.0
    assert (Y.sum(1) > 0).all() and Y.max() < 2**24
    m, d = cu.margins(Y), cu.poisson_deviance(Y)
    Y.setflags(write=False)
    return Y, m, d


@functools.lru_cache(maxsize=None)
def _edge(shape, variant):
    """-> (Y, stored): see the head of the file"""
    N, P = shape
    rng = np.random.default_rng(N * 7 + P)
    Y = cu.recipe(N, P, seed=N + P, depth=-3.0, zero_column=False)
    stored = np.zeros((N, P), bool)
    hole = 5
    for r, n in enumerate(ROW_LENGTHS, start=1):
        Y[r] = 0.0
        cols = rng.choice(np.setdiff1d(np.arange(P), [hole]), n, replace=False)
        Y[r, cols] = rng.integers(1, 300, n)
    Y[0] = 0.0
    Y[N - 1] = 0.0
    if variant == "full":
        full = len(ROW_LENGTHS) + 1
        Y[full] = rng.integers(0, 4, P)  # the zeros among them are stored explicitly
        Y[full, 0], Y[full, P - 1] = 7.0, 9.0
        stored[full] = True
    else:
        Y[:, hole] = 0.0
    assert (Y != 0).sum(1)[1:8].tolist() == list(ROW_LENGTHS)
    Y.setflags(write=False)
    stored.setflags(write=False)
    return Y, stored


def _margins_raw(A, keep=None, short=0):
    lib = _lib()
    N, P = A.shape
    rs, cs = torch.full((N,), -7.0, dtype=f64, device=DEV), torch.full((P,), -7.0, dtype=f64, device=DEV)
    rn, cn = torch.full((N,), -7, dtype=i64, device=DEV), torch.full((P,), -7, dtype=i64, device=DEV)
    bad = torch.full((1,), -7, dtype=i64, device=DEV)
    nbytes = lib.gpsa_count_csr_workspace(N, P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = lib.gpsa_count_margins_csr_f32(A.crow.data_ptr(), A.col.data_ptr(), A.values.data_ptr(),
                                        None if keep is None else keep.data_ptr(), N, P, A.nnz, rs.data_ptr(), cs.data_ptr(),
                                        rn.data_ptr(), cn.data_ptr(), bad.data_ptr(), ws.data_ptr(), nbytes - short, _stream())
    torch.cuda.synchronize()
    return rc, rs.cpu().numpy(), cs.cpu().numpy(), rn.cpu().numpy(), cn.cpu().numpy(), int(bad.item())


def _assert_margins(got, m):
    for g, key in zip(got, ("row_sum", "col_sum", "row_nnz", "col_nnz")):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert np.array_equal(g, m[key]), key


def test_the_constants_python_exports_are_the_kernels():
    import os
    import re

    src = open(os.path.join(os.path.dirname(counts.__file__), "csrc", "counts_sparse.hip")).read()
    for py, c in ((RM, "CSR_ROWS_MIN"), (MG, "CSR_MAX_GROUPS"), (CT, "CSR_COL_TILE"), (GT, "CSR_GATHER_TILE")):
        assert int(re.search(r"constexpr int " + c + r" = (\d+);", src).group(1)) == py, c


# ------------------------------------------------------------------------------------------------------------------------
# the margins
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,depth", CASES, ids=IDS)
def test_margins_equal_the_yardstick_and_the_dense_entry_bit_for_bit(shape, depth):
    Yh, m, _ = _data(shape, depth)
    A = _csr(Yh)
    assert A.shape == shape and A.nnz == int((Yh != 0).sum()) and A.n_stored_zeros == 0
    rc, *got, bad = _margins_raw(A)
    assert rc == 0 and bad == 0
    _assert_margins(got, m)
    out = torch.ops.gpsa.count_margins_csr(A.crow, A.col, A.values, *shape)
    again = torch.ops.gpsa.count_margins_csr(A.crow, A.col, A.values, *shape)
    dense = torch.ops.gpsa.count_margins(_dev(Yh))
    for a, b, c in zip(out, again, dense):
        assert torch.equal(a, b) and torch.equal(a, c) and a.dtype == c.dtype
    st = gp.count_stats(A)
    assert st.n_invalid == 0 and st.total == m["total"] and st.row_sum.dtype == f64 and st.row_nnz.dtype == i64
    _assert_margins((st.row_sum, st.col_sum, st.row_nnz, st.col_nnz), m)


@pytest.mark.parametrize("index", [i32, i64], ids=["int32", "int64"])
@pytest.mark.parametrize("variant", ["full", "hole"])
@pytest.mark.parametrize("shape", EDGES, ids=[f"{n}x{p}" for n, p in EDGES])
def test_margins_and_deviance_at_the_edges(shape, variant, index):
    Yh, stored = _edge(shape, variant)
    N, P = shape
    A = _csr(Yh, index, stored)
    assert A.col.dtype == i32 and A.crow.dtype == i64
    assert A.n_stored_zeros == int((stored & (Yh == 0)).sum()) and (variant == "hole" or A.n_stored_zeros > 0)
    m = cu.margins(Yh)
    assert m["row_sum"][0] == 0 and m["row_sum"][-1] == 0 and (variant == "full" or m["col_nnz"][5] == 0)
    rc, *got, bad = _margins_raw(A)
    assert rc == 0 and bad == 0
    _assert_margins(got, m)  # an explicitly stored 0 is not an entry > 0
    dense = torch.ops.gpsa.count_margins(_dev(Yh))
    for a, c in zip(torch.ops.gpsa.count_margins_csr(A.crow, A.col, A.values, N, P), dense):
        assert torch.equal(a, c)
    # a mask that drops the first row, the last row and a whole group of the kernel's
    R = max(RM, -(-N // MG))
    keep = np.ones(N, bool)
    keep[0] = keep[N - 1] = False
    if N >= 2 * R:
        keep[R: 2 * R] = False
    Yk = np.where(keep[:, None], Yh, 0.0)
    mk = cu.margins(Yk)
    kd = _dev(keep, torch.bool)
    _assert_margins(torch.ops.gpsa.count_margins_csr(A.crow, A.col, A.values, N, P, kd)[:4], mk)
    rc, *got, bad = _margins_raw(A, kd.view(torch.uint8))
    assert rc == 0 and bad == 0
    _assert_margins(got, mk)
    # the deviance with size factors of the caller's, unmasked and masked, twice
    lsz = _dev(np.linspace(-0.3, 0.4, N), f64)
    for kp, Yw in ((None, Yh), (kd, Yk)):
        w = cu.poisson_deviance(Yw, lsz.cpu().numpy())
        a = torch.ops.gpsa.count_deviance_csr(A.crow, A.col, A.values, N, P, lsz, kp)
        b = torch.ops.gpsa.count_deviance_csr(A.crow, A.col, A.values, N, P, lsz, kp)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert (np.abs(a[0].cpu().numpy() - w["ll_sat"]) <= 1e-11 * w["abs_sat"]).all()
        assert (np.abs(a[1].cpu().numpy() - w["abs_sat"]) <= 1e-11 * w["abs_sat"]).all()
        assert (a[0].cpu().numpy()[w["abs_sat"] == 0] == 0).all()


def test_a_matrix_without_entries():
    A = gp.csr_counts((torch.zeros(41, dtype=i64, device=DEV), torch.zeros(0, dtype=i32, device=DEV),
                       torch.zeros(0, dtype=f32, device=DEV), (40, 700)))
    assert A.nnz == 0 and A.n_stored_zeros == 0
    st = gp.count_stats(A)
    assert st.total == 0 and st.n_invalid == 0 and not st.row_sum.any() and not st.col_sum.any()
    assert not st.row_nnz.any() and not st.col_nnz.any()
    ll, ab = torch.ops.gpsa.count_deviance_csr(A.crow, A.col, A.values, 40, 700, torch.zeros(40, dtype=f64, device=DEV))
    assert not ll.any() and not ab.any()
    assert torch.equal(gp.densify(A, rows=[0, 39]), torch.zeros(2, 700, device=DEV))
    with pytest.raises(ValueError, match="40 of 40 rows have no counts"):
        gp.size_factors(A)


@pytest.mark.parametrize("value", [float("nan"), -1.0, float("inf"), float("-inf")], ids=["NaN", "negative", "inf", "-inf"])
def test_an_invalid_stored_value_is_counted_and_refused(value):
    Yh = np.array(_data((97, 45), DEPTHS[0])[0])
    Yh[40, 17] = value
    Yh[96, 44] = value
    A = _csr(Yh)
    assert cu.margins(Yh)["n_invalid"] == 2
    assert _margins_raw(A)[5] == 2 and gp.count_stats(A).n_invalid == 2
    assert int(torch.ops.gpsa.count_margins(_dev(Yh))[4]) == 2
    S = torch.sparse_csr_tensor(A.crow, A.col, A.values, size=A.shape)
    for Y in (A, S):
        for call in (lambda: gp.size_factors(Y), lambda: gp.poisson_deviance(Y), lambda: gp.deviance_feature_selection(Y),
                     lambda: gp.prepare_counts(Y, [50, 47])):
            with pytest.raises(ValueError, match="2 entries that are NaN, infinite or negative"):
                call()


# ------------------------------------------------------------------------------------------------------------------------
# size factors and the deviance
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,depth", CASES, ids=IDS)
def test_size_factors_and_deviance(shape, depth):
    Yh, m, d = _data(shape, depth)
    A = _csr(Yh)
    sz = gp.size_factors(A)
    e_sz = float(np.abs(sz.cpu().numpy() / cu.size_factors(Yh) - 1).max())
    assert sz.dtype == f64 and e_sz <= 1e-13
    assert torch.allclose(torch.exp(gp.size_factors(A, log=True)), sz, rtol=1e-14, atol=0)
    res = gp.poisson_deviance(A, return_parts=True)
    scale = d["abs_sat"] + np.abs(d["ll_null"])
    e_sat = float((np.abs(res.ll_sat.cpu().numpy() - d["ll_sat"]) / np.maximum(scale, 1e-300)).max())
    e_dev = float((np.abs(res.deviance.cpu().numpy() - d["deviance"]) / np.maximum(scale, 1e-300)).max())
    e_abs = float(np.abs(res.abs_sat.cpu().numpy() / np.maximum(d["abs_sat"], 1e-300) - 1)[d["abs_sat"] > 0].max(initial=0))
    print(f"[counts sparse] {shape} depth {depth:g}: density {(Yh != 0).mean():.3f}, size factors {e_sz:.1e}, ll_sat "
          f"{e_sat:.1e}, deviance {e_dev:.1e} of abs_sat + |ll_null| (bar 1e-11), abs_sat {e_abs:.1e}")
    assert e_sat <= 1e-11 and e_dev <= 1e-11 and e_abs <= 1e-11
    assert (res.deviance.cpu().numpy()[m["col_sum"] == 0] == 0).all()  # a gene without counts: exactly 0
    mine = _dev(np.linspace(-0.3, 0.4, shape[0]), f64)
    a = torch.ops.gpsa.count_deviance_csr(A.crow, A.col, A.values, *shape, mine)
    b = torch.ops.gpsa.count_deviance_csr(A.crow, A.col, A.values, *shape, mine)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # two calls: the same bits
    w = cu.poisson_deviance(Yh, mine.cpu().numpy())
    assert (np.abs(a[0].cpu().numpy() - w["ll_sat"]) <= 1e-11 * w["abs_sat"]).all()
    assert (np.abs(gp.poisson_deviance(A, mine).cpu().numpy() - w["deviance"]) <= 1e-11 * (w["abs_sat"] + np.abs(w["ll_null"]))).all()
    sel = gp.deviance_feature_selection(A)
    assert torch.equal(sel.deviance, res.deviance) and sel.order.dtype == i64
    assert sorted(sel.order.tolist()) == list(range(shape[1]))
    if (shape, depth) in ORDERED_CASES:
        gap = cu.smallest_relative_gap(d["deviance"])
        assert gap >= 1e-9, gap
        assert np.array_equal(sel.order.cpu().numpy(), cu.order(d["deviance"]))
        top = gp.deviance_feature_selection(A, n_top=10)
        assert np.array_equal(top.order.cpu().numpy(), cu.order(d["deviance"])[:10])


# ------------------------------------------------------------------------------------------------------------------------
# densify
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(97, 45), (257, 130), (5, 2049)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_densify_equals_the_dense_block(shape):
    Yh, _, _ = _data(shape, DEPTHS[0])
    N, P = shape
    A, D = _csr(Yh), _dev(Yh)
    rng = np.random.default_rng(0)
    rows = np.sort(rng.choice(N, max(1, N // 3), replace=False))
    genes = np.sort(rng.choice(P, max(1, P // 4), replace=False))
    for r, g in ((None, genes), (rows, None), (rows, genes), ([N // 2], None), (None, [P - 1]), (None, None)):
        got = gp.densify(A, rows=r, genes=g)
        want = D[slice(None) if r is None else _dev(r, i64)][:, slice(None) if g is None else _dev(g, i64)]
        assert got.dtype == f32 and got.is_contiguous() and torch.equal(got, want), (r, g)
    S = torch.sparse_csr_tensor(A.crow, A.col, A.values, size=A.shape)
    assert torch.equal(gp.densify(S, rows=torch.tensor(rows), genes=torch.tensor(genes, device=DEV)),
                       D[_dev(rows, i64)][:, _dev(genes, i64)])
    perm = rng.permutation(P)[:7]  # genes in an order of the caller's, rows repeated
    assert torch.equal(gp.densify(A, rows=[3, 3, 0], genes=perm), D[_dev([3, 3, 0], i64)][:, _dev(perm, i64)])
    for kw, match in ((dict(rows=[N]), "rows holds indices outside"), (dict(genes=[-1]), "genes holds indices outside"),
                      (dict(genes=[1, 1]), "genes holds an index twice"), (dict(rows=[]), "rows must be None or"),
                      (dict(genes=[0.5]), "genes must be None or")):
        with pytest.raises(ValueError, match="densify: " + match):
            gp.densify(A, **kw)


@pytest.mark.parametrize("G", [GT - 1, GT, GT + 1])
def test_densify_around_the_gather_tile(G):
    Yh = cu.recipe(6, G + 2, seed=G, depth=-2.0)
    A, D = _csr(Yh), _dev(Yh)
    assert torch.equal(gp.densify(A, genes=np.arange(1, G + 1)), D[:, 1: G + 1])
    assert torch.equal(gp.densify(A), D)


# ------------------------------------------------------------------------------------------------------------------------
# the one call
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [[120, 137], [80, 90, 87]], ids=["two views", "three views"])
@pytest.mark.parametrize("transform", counts.TRANSFORMS)
def test_prepare_counts_equals_the_dense_path(transform, ns):
    Yh = np.array(_data((257, 130), DEPTHS[0])[0])
    kw = dict(min_counts=float(np.sort(Yh.sum(1))[5]), max_counts=float(np.sort(Yh.sum(1))[-4]), min_cells=8,
              n_top_genes=40, transform=transform, theta=50.0)
    want = cu.prepare(Yh, ns, **kw)
    assert cu.smallest_relative_gap(want["deviance"]) >= 1e-9  # the selection is then decided by the values alone
    assert 200 < len(want["rows"]) < 257 and len(want["genes"]) == 40
    assert (((Yh[want["rows"]] > 0).sum(0) >= 8).sum()) < 130  # min_cells bites
    A, D = _csr(Yh), _dev(Yh)
    before = [t.clone() for t in (A.crow, A.col, A.values)]
    for Y in (A, torch.sparse_csr_tensor(A.crow, A.col, A.values, size=A.shape)):
        res, dense = gp.prepare_counts(Y, ns, **kw), gp.prepare_counts(D, ns, **kw)
        assert torch.equal(res.rows, dense.rows) and torch.equal(res.genes, dense.genes)
        assert res.n_samples_list == dense.n_samples_list == want["n_samples_list"]
        assert torch.equal(res.outputs, dense.outputs) and res.outputs.dtype == f32 and res.outputs.is_contiguous()
        parts = cu.poisson_deviance(Yh[want["rows"]])
        bar = 1e-11 * (parts["abs_sat"] + np.abs(parts["ll_null"]))
        assert (np.abs(res.deviance.cpu().numpy() - dense.deviance.cpu().numpy()) <= 2 * bar).all()
        assert (np.abs(res.deviance.cpu().numpy() - want["deviance"]) <= bar).all()
        if transform == "counts":
            assert res.n_constant is None and torch.equal(res.log_offset, dense.log_offset)
            assert np.array_equal(res.outputs.cpu().numpy(), Yh[want["rows"]][:, want["genes"]])
            assert np.abs(res.log_offset.cpu().numpy() - want["log_offset"]).max() <= 1e-6
        else:
            assert res.log_offset is None and torch.equal(res.n_constant, dense.n_constant)
        # ... and the yardstick's pipeline at the dense suite's tolerances
        assert np.array_equal(res.rows.cpu().numpy(), want["rows"]) and np.array_equal(res.genes.cpu().numpy(), want["genes"])
        got = res.outputs.cpu().numpy().astype(np.float64)
        assert float((np.abs(got - want["outputs"]) / np.maximum(1.0, np.abs(want["outputs"]))).max()) <= 1e-6
    assert all(torch.equal(a, b) for a, b in zip(before, (A.crow, A.col, A.values)))  # the input is untouched
    if transform != "counts":
        res2 = gp.prepare_counts(A, ns, standardize=False, **kw)
        assert res2.n_constant is None and torch.equal(res2.outputs, gp.prepare_counts(D, ns, standardize=False, **kw).outputs)


def test_prepare_counts_without_filters_and_rows_without_counts():
    Yh = np.array(_data((97, 45), DEPTHS[1])[0])
    A, D = _csr(Yh), _dev(Yh)
    for transform in counts.TRANSFORMS:
        res, dense = gp.prepare_counts(A, [50, 47], transform=transform), gp.prepare_counts(D, [50, 47], transform=transform)
        assert res.rows.numel() == 97 and res.genes.numel() == 45 and torch.equal(res.outputs, dense.outputs), transform
    Yh[3] = 0.0
    A = _csr(Yh)
    with pytest.raises(ValueError, match=r"^prepare_counts: 1 of 97 rows have no counts.*min_counts"):
        gp.prepare_counts(A, [50, 47])
    with pytest.raises(ValueError, match=r"^deviance_feature_selection: 1 of 97 rows have no counts"):
        gp.deviance_feature_selection(A)
    res = gp.prepare_counts(A, [50, 47], min_counts=1, transform="counts")
    want = cu.prepare(Yh, [50, 47], min_counts=1, transform="counts")
    assert res.n_samples_list == [49, 47] and np.array_equal(res.rows.cpu().numpy(), want["rows"])
    assert np.array_equal(res.outputs.cpu().numpy(), want["outputs"])


def test_prepare_counts_stays_far_below_the_dense_matrix():
    """N = 4000, P = 20 000 at about 2 % density, generated on the device in row chunks: the peak allocation of
    prepare_counts above its inputs stays below memory_bound (tests/test_counts_sparse.py: workspace + result + 64 (N + P)
    doubles), and the dense matrix alone is at least ten times that bound"""
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
    assert 4 * N * P == 320_000_000 >= 10 * bound
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = gp.prepare_counts(A, [2000, 2000], n_top_genes=G, transform="pearson")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[counts sparse] prepare_counts {N} x {P}, nnz {A.nnz}: peak {peak / 2**20:.1f} MiB above the inputs, bound "
          f"{bound / 2**20:.1f} MiB, the dense matrix {4 * N * P / 2**20:.1f} MiB")
    assert tuple(res.outputs.shape) == (N, G) and bool(torch.isfinite(res.outputs).all())
    assert peak <= bound, (peak, bound)


# ------------------------------------------------------------------------------------------------------------------------
# malformed input: reported by the check entry, which alone runs on it
# ------------------------------------------------------------------------------------------------------------------------
def _malformed(kind):
    Yh = np.array(_data((33, 65), DEPTHS[0])[0])
    crow, col, val = _csr_host(Yh)
    a = int(crow[10])
    assert crow[11] - a >= 2 and crow[20] > crow[19]
    if kind == "crow[0] = 1":
        crow[0] = 1
        return crow, col, val, r"crow is not a row pointer: 1 violations"
    if kind == "a decreasing crow":
        crow[20] = crow[19] - 1
        return crow, col, val, r"crow is not a row pointer: 1 violations"
    if kind == "crow[N] != nnz":
        crow[-1] -= 1
        return crow, col, val, r"crow is not a row pointer: 1 violations.*nnz = %d" % len(col)
    if kind == "an index equal to P":
        col[a + 1] = 65
        col[-1] = 65
        return crow, col, val, r"2 column indices are outside \[0, 65\)"
    if kind == "a negative index":
        col[a] = -1
        return crow, col, val, r"1 column indices are outside \[0, 65\)"
    if kind == "a swapped pair":
        col[a], col[a + 1] = col[a + 1], col[a]
        return crow, col, val, r"rows are not sorted / hold duplicates: at 1 places.*sum_duplicates / sort_indices.*coalesce"
    col[a + 1] = col[a]
    return crow, col, val, r"rows are not sorted / hold duplicates: at 1 places"


@pytest.mark.parametrize("index", [i32, i64], ids=["int32", "int64"])
@pytest.mark.parametrize("kind", ["crow[0] = 1", "a decreasing crow", "crow[N] != nnz", "an index equal to P",
                                  "a negative index", "a swapped pair", "a duplicate"])
def test_a_malformed_matrix_is_refused_by_rule_and_count(kind, index, monkeypatch):
    from spatial_alignment_amd import ops

    def never(*a, **k):
        raise AssertionError("a compute entry ran on a malformed matrix")

    for name in ("count_margins_csr", "count_deviance_csr", "csr_gather_dense"):
        monkeypatch.setattr(ops.HipOps, name, never)
    crow, col, val, match = _malformed(kind)
    parts = (_dev(crow, index), _dev(col, index), _dev(val), (33, 65))
    with pytest.raises(ValueError, match=r"^csr_counts: " + match):
        gp.csr_counts(parts)
    S = torch.sparse_csr_tensor(*parts[:3], size=(33, 65), check_invariants=False)
    for name, call in (("count_stats", lambda: gp.count_stats(S)), ("prepare_counts", lambda: gp.prepare_counts(S, [33])),
                       ("densify", lambda: gp.densify(S))):
        with pytest.raises(ValueError, match=rf"^{name}: " + match):
            call()


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI's refusals, on device memory: the documented code, and nothing written
# ------------------------------------------------------------------------------------------------------------------------
def test_the_entries_refuse_with_the_documented_codes_and_write_nothing():
    lib = _lib()
    A = _csr(_data((33, 65), DEPTHS[0])[0])
    N, P = A.shape
    rc, rs, cs, rn, cn, bad = _margins_raw(A, short=8)
    assert rc == EWORKSPACE and (rs == -7).all() and (cs == -7).all() and (rn == -7).all() and (cn == -7).all() and bad == -7
    need = lib.gpsa_count_csr_workspace(N, P)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out4 = torch.full((4,), -7, dtype=i64, device=DEV)
    a, b = (torch.full((P,), -7.0, dtype=f64, device=DEV) for _ in range(2))
    lsz = torch.zeros(N, dtype=f64, device=DEV)
    rows, slot = torch.arange(3, device=DEV), torch.full((P,), -1, dtype=i32, device=DEV)
    blk = torch.full((3, 4), -7.0, dtype=f32, device=DEV)
    s = _stream()
    base = dict(crow=A.crow.data_ptr(), col=A.col.data_ptr(), val=A.values.data_ptr(), N=N, P=P, nnz=A.nnz)
    shape_kw = (dict(crow=None), dict(col=None), dict(val=None), dict(N=0), dict(P=0), dict(P=2**31), dict(nnz=-1),
                dict(nnz=N * P + 1))

    def check(out=out4.data_ptr(), w=ws.data_ptr(), nb=need, **kw):
        k = dict(base, **kw)
        return lib.gpsa_csr_check(k["crow"], k["col"], k["val"], k["N"], k["P"], k["nnz"], out, w, nb, s)

    def dev(l=lsz.data_ptr(), w=ws.data_ptr(), nb=need, **kw):
        k = dict(base, **kw)
        return lib.gpsa_count_deviance_csr_f32(k["crow"], k["col"], k["val"], None, k["N"], k["P"], k["nnz"], l, a.data_ptr(),
                                               b.data_ptr(), w, nb, s)

    def gather(r=rows.data_ptr(), n_rows=3, sl=slot.data_ptr(), G=4, o=blk.data_ptr(), **kw):
        k = dict(base, **kw)
        return lib.gpsa_csr_gather_dense_f32(k["crow"], k["col"], k["val"], k["N"], k["P"], k["nnz"], r, n_rows, sl, G, o, s)

    for kw in shape_kw:
        assert check(**kw) == EINVAL and dev(**kw) == EINVAL and gather(**kw) == EINVAL, kw
    assert check(out=None) == EINVAL and check(nb=need - 8) == EWORKSPACE and check(w=None) == EWORKSPACE
    assert dev(l=None) == EINVAL and dev(nb=need - 8) == EWORKSPACE and dev(w=None) == EWORKSPACE
    for kw in (dict(r=None), dict(sl=None), dict(o=None), dict(n_rows=0), dict(G=0), dict(G=P + 1)):
        assert gather(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((out4 == -7).all()) and bool((a == -7).all()) and bool((b == -7).all()) and bool((blk == -7).all())
    o = _ops()
    with pytest.raises(ValueError, match="needs contiguous crow int64"):
        o.count_margins_csr(A.crow.to(i32), A.col, A.values, N, P)
    with pytest.raises(ValueError, match="needs contiguous crow int64"):
        o.csr_check(A.crow, A.col.to(i64), A.values, N, P)
    with pytest.raises(ValueError, match="keep must be"):
        o.count_margins_csr(A.crow, A.col, A.values, N, P, torch.ones(N + 1, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="log_sz has shape"):
        o.count_deviance_csr(A.crow, A.col, A.values, N, P, lsz[:-1])
    with pytest.raises(ValueError, match="slot must be"):
        o.csr_gather_dense(A.crow, A.col, A.values, N, P, rows, slot.to(i64), 4)
