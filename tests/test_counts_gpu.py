"""Count preprocessing on the device: the entries of csrc/counts.hip through the C ABI alone, through ``torch.ops.gpsa.*``
and through the calls of spatial_alignment_amd/counts.py, against the fp64 numpy yardstick of tests/counts_util.py (itself
held against the reference's functions in tests/test_counts.py).

Bars (derived, none fitted; every comparison prints what it measures next to its bar):
* row / column sums, the two counts of entries > 0 and n_invalid: EQUAL (sums of integers are exact in fp64 in any order);
* ll_sat and the deviance: |err| <= 1e-11 (abs_sat_g + |ll_null_g|) - some 1e4 fp64 roundings at the largest N here;
* the transforms and the z-score (fp32 results of fp64 arithmetic): |err| <= 1e-6 max(1, |value|); one fp32 rounding is 6e-8;
* gene ORDER only where the yardstick's smallest relative gap between neighbouring deviances is >= 1e-9 (asserted for the
  shapes it is compared on); the tie rule on a matrix with duplicated columns.

Shapes: the seven of the issue, then one at, below and above the kernels' row group (ROWS_MIN), column tile (COL_TILE) and
vector width on both axes, one with more row blocks than the cap on the groups (groups of 17 rows), and two where the
groups have reached ROWS_MAX and their number grows past the cap.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import counts_util as cu
import spatial_alignment_amd as gp
from spatial_alignment_amd import counts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64, f32 = torch.float64, torch.float32
EINVAL, EWORKSPACE = -1, -2
RM, RX, MG, CT = counts.ROWS_MIN, counts.ROWS_MAX, counts.MAX_GROUPS, counts.COL_TILE
SHAPES = [(1, 1), (33, 65), (97, 45), (257, 130), (1000, 7), (5, 2049), (4099, 3),
          (RM - 1, 12), (RM, 13), (RM + 1, 12), (2 * RM + 3, 8),          # the row group; P % 4 == 0 and != 0
          (9, CT - 1), (9, CT), (9, CT + 1), (7, 2 * CT + 4), (6, CT - 4),  # the column tile, both load paths
          (3, 4), (3, 3), (2, 5),                                         # the vector width
          (RM * MG + 37, 5),                                              # more row blocks than the cap: groups of 17 rows
          (RX * MG, 1), (RX * MG + 5, 2)]                                 # groups at ROWS_MAX; more groups than the cap
ORDERED = [(33, 65), (97, 45), (257, 130)]  # gene order is compared here: no near-ties (asserted)
IDS = [f"{n}x{p}" for n, p in SHAPES]


def _lib():
    from spatial_alignment_amd import _lib as L

    return L.load()


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _dev(a, dt=f32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _data(shape):
    """the recipe's counts at this shape with the depth raised until no row is empty (asserted), the yardstick's values
    (computed once, shared, never changed)"""
    N, P = shape
    for depth in (0.5, 1.5, 2.5, 3.5, 4.5):
        Y = cu.recipe(N, P, seed=N * 31 + P, depth=depth)
        if (Y.sum(1) > 0).all():
            break
    else:  # half a million rows of one or two genes: some row is empty at any depth, so every row gets one count more
        Y[:, 0] += 1.0
    assert (Y.sum(1) > 0).all() and Y.max() < 2**24
    m = cu.margins(Y)
    d = cu.poisson_deviance(Y)
    Y.setflags(write=False)
    return Y, m, d


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _margins_raw(Y, short=0):
    lib = _lib()
    N, P = Y.shape
    rs, cs = torch.full((N,), -7.0, dtype=f64, device=DEV), torch.full((P,), -7.0, dtype=f64, device=DEV)
    rn, cn = torch.full((N,), -7, dtype=torch.int64, device=DEV), torch.full((P,), -7, dtype=torch.int64, device=DEV)
    bad = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    nbytes = lib.gpsa_count_workspace(N, P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = lib.gpsa_count_margins_f32(Y.data_ptr(), N, P, rs.data_ptr(), cs.data_ptr(), rn.data_ptr(), cn.data_ptr(),
                                    bad.data_ptr(), ws.data_ptr(), nbytes - short, _stream())
    torch.cuda.synchronize()
    return rc, rs.cpu().numpy(), cs.cpu().numpy(), rn.cpu().numpy(), cn.cpu().numpy(), int(bad.item())


# ------------------------------------------------------------------------------------------------------------------------
# the margins
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_margins_are_equal_bit_for_bit(shape):
    Yh, m, _ = _data(shape)
    Y = _dev(Yh)
    rc, rs, cs, rn, cn, bad = _margins_raw(Y)
    assert rc == 0
    for got, key in ((rs, "row_sum"), (cs, "col_sum"), (rn, "row_nnz"), (cn, "col_nnz")):
        assert np.array_equal(got, m[key]), key
    assert bad == 0
    out = torch.ops.gpsa.count_margins(Y)
    again = torch.ops.gpsa.count_margins(Y)
    for a, b, got in zip(out, again, (rs, cs, rn, cn, np.array([bad]))):
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), got)
    st = gp.count_stats(Y.to(torch.int32))  # any real dtype is taken to fp32
    assert st.n_invalid == 0 and st.total == m["total"] and np.array_equal(st.col_nnz.cpu().numpy(), m["col_nnz"])
    assert st.row_sum.dtype == f64 and st.row_nnz.dtype == torch.int64


def test_a_row_slice_that_is_not_16_byte_aligned_takes_the_scalar_path():
    Yh = cu.recipe(40, 12, seed=3, depth=1.0)
    buf = torch.zeros(40 * 12 + 1, dtype=f32, device=DEV)
    Y = buf[1:].view(40, 12)  # P % 4 == 0 but the base is 4 bytes off
    Y.copy_(_dev(Yh))
    assert Y.data_ptr() % 16 == 4
    m = cu.margins(Yh)
    rs, cs, rn, cn, bad = torch.ops.gpsa.count_margins(Y)
    assert np.array_equal(rs.cpu().numpy(), m["row_sum"]) and np.array_equal(cs.cpu().numpy(), m["col_sum"])
    want = cu.pearson_residuals(Yh, 100.0)
    got = torch.ops.gpsa.count_transform(Y, "pearson", rs, cs, m["total"], 100.0, float(np.sqrt(40)))
    assert _rel(got.cpu().numpy(), want) <= 1e-6


@pytest.mark.parametrize("value,what", [(float("nan"), "NaN"), (-1.0, "negative"), (float("inf"), "inf"),
                                        (float("-inf"), "-inf")])
def test_an_invalid_entry_is_counted_and_refused(value, what):
    Yh = np.array(_data((97, 45))[0])
    Yh[40, 17] = value
    Yh[96, 44] = value
    Y = _dev(Yh)
    assert cu.margins(Yh)["n_invalid"] == 2
    assert _margins_raw(Y)[5] == 2 and gp.count_stats(Y).n_invalid == 2
    for call in (lambda: gp.size_factors(Y), lambda: gp.poisson_deviance(Y), lambda: gp.deviance_feature_selection(Y),
                 lambda: gp.pearson_residuals(Y), lambda: gp.deviance_residuals(Y, 10.0), lambda: gp.normalize_log1p(Y),
                 lambda: gp.prepare_counts(Y, [50, 47])):
        with pytest.raises(ValueError, match="2 entries that are NaN, infinite or negative"):
            call()


# ------------------------------------------------------------------------------------------------------------------------
# size factors and the deviance
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_size_factors_and_deviance(shape):
    Yh, m, d = _data(shape)
    Y = _dev(Yh)
    sz = gp.size_factors(Y)
    lsz = gp.size_factors(Y, log=True)
    want = cu.size_factors(Yh)
    e_sz = float(np.abs(sz.cpu().numpy() / want - 1).max())
    assert sz.dtype == f64 and e_sz <= 1e-13 and torch.allclose(torch.exp(lsz), sz, rtol=1e-14, atol=0)
    res = gp.poisson_deviance(Y, return_parts=True)
    scale = d["abs_sat"] + np.abs(d["ll_null"])
    e_sat = float((np.abs(res.ll_sat.cpu().numpy() - d["ll_sat"]) / np.maximum(scale, 1e-300)).max())
    e_dev = float((np.abs(res.deviance.cpu().numpy() - d["deviance"]) / np.maximum(scale, 1e-300)).max())
    e_abs = float(np.abs(res.abs_sat.cpu().numpy() / np.maximum(d["abs_sat"], 1e-300) - 1)[d["abs_sat"] > 0].max(initial=0))
    print(f"[counts] {shape}: size factors {e_sz:.1e}, ll_sat {e_sat:.1e}, deviance {e_dev:.1e} of abs_sat + |ll_null| "
          f"(bar 1e-11), abs_sat {e_abs:.1e}")
    assert e_sat <= 1e-11 and e_dev <= 1e-11 and e_abs <= 1e-11
    zero = m["col_sum"] == 0
    assert (res.deviance.cpu().numpy()[zero] == 0).all()  # a gene without counts: exactly 0
    # the entry alone, with size factors of the caller's, twice: the same bits
    mine = _dev(np.linspace(-0.3, 0.4, shape[0]), f64)
    a = torch.ops.gpsa.count_deviance(Y, mine)
    b = torch.ops.gpsa.count_deviance(Y, mine)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    w = cu.poisson_deviance(Yh, mine.cpu().numpy())
    assert (np.abs(a[0].cpu().numpy() - w["ll_sat"]) <= 1e-11 * w["abs_sat"]).all()
    assert (np.abs(gp.poisson_deviance(Y, mine).cpu().numpy() - w["deviance"]) <= 1e-11 * (w["abs_sat"] + np.abs(w["ll_null"]))).all()
    sel = gp.deviance_feature_selection(Y)
    assert torch.equal(sel.deviance, res.deviance) and sel.order.dtype == torch.int64
    assert sorted(sel.order.tolist()) == list(range(shape[1]))
    dv = sel.deviance[sel.order]
    assert bool((dv[:-1] >= dv[1:]).all())
    if shape in ORDERED:
        gap = cu.smallest_relative_gap(d["deviance"])
        assert gap >= 1e-9, gap
        assert np.array_equal(sel.order.cpu().numpy(), cu.order(d["deviance"]))
        top = gp.deviance_feature_selection(Y, n_top=10)
        assert np.array_equal(top.order.cpu().numpy(), cu.order(d["deviance"])[:10])


def test_equal_deviances_rank_by_the_lower_index():
    Yh = np.array(_data((5, 2049))[0])
    assert cu.smallest_relative_gap(cu.poisson_deviance(Yh)["deviance"]) == 0  # this shape ties on its own
    Yh = np.array(_data((97, 45))[0])
    Yh[:, 30] = Yh[:, 4]
    Yh[:, 12] = Yh[:, 4]
    sel = gp.deviance_feature_selection(_dev(Yh))
    dev = sel.deviance.cpu().numpy()
    assert dev[4] == dev[12] == dev[30]
    o = sel.order.tolist()
    assert o.index(4) + 2 == o.index(12) + 1 == o.index(30)
    assert np.array_equal(sel.order.cpu().numpy(), np.argsort(-dev, kind="stable"))


def test_rows_without_counts_are_refused_by_name_and_filtered_by_min_counts():
    Yh = cu.recipe(1000, 7, seed=2, depth=0.0)
    empty = int((Yh.sum(1) == 0).sum())
    assert empty > 0  # a narrow shape at the recipe's own depth
    Y = _dev(Yh)
    for call in (lambda: gp.size_factors(Y), lambda: gp.poisson_deviance(Y), lambda: gp.prepare_counts(Y, [500, 500])):
        with pytest.raises(ValueError, match=f"{empty} of 1000 rows have no counts.*min_counts"):
            call()
    res = gp.prepare_counts(Y, [500, 500], min_counts=1, transform="counts")
    want = cu.prepare(Yh, [500, 500], min_counts=1, transform="counts")
    assert np.array_equal(res.rows.cpu().numpy(), want["rows"]) and len(want["rows"]) == 1000 - empty
    assert res.n_samples_list == want["n_samples_list"] and sum(res.n_samples_list) == 1000 - empty
    assert np.abs(res.log_offset.cpu().numpy() - want["log_offset"]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------
# the transforms
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_transforms(shape):
    Yh, m, _ = _data(shape)
    Y = _dev(Yh)
    N = shape[0]
    cases = [("pearson 100", lambda y, **kw: gp.pearson_residuals(y, 100.0, **kw), cu.pearson_residuals(Yh, 100.0)),
             ("pearson 1 unclipped", lambda y, **kw: gp.pearson_residuals(y, 1.0, clipping=False, **kw),
              cu.pearson_residuals(Yh, 1.0, clipping=False)),
             ("deviance 100", lambda y, **kw: gp.deviance_residuals(y, 100.0, **kw), cu.deviance_residuals(Yh, 100.0)[0]),
             ("deviance inf", lambda y, **kw: gp.deviance_residuals(y, float("inf"), **kw),
              cu.deviance_residuals(Yh, np.inf)[0]),
             ("log1p median", lambda y, **kw: gp.normalize_log1p(y, **kw), cu.normalize_log1p(Yh)),
             ("log1p 1e4", lambda y, **kw: gp.normalize_log1p(y, 1e4, **kw), cu.normalize_log1p(Yh, 1e4))]
    worst, outs = {}, {}
    for name, call, want in cases:
        got = outs[name] = call(Y)
        assert got.dtype == f32 and tuple(got.shape) == shape and got.data_ptr() != Y.data_ptr()
        worst[name] = _rel(got.cpu().numpy().astype(np.float64), want)
        assert torch.equal(got, call(Y)), name  # two calls: the same bits
    print(f"[counts] {shape}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + " (bar 1e-6 of max(1, |value|))")
    assert max(worst.values()) <= 1e-6, worst
    assert torch.equal(Y, _dev(Yh))  # the matrix passed is untouched
    # in place equals out of place, through the public call and through the entry
    for name, call, _ in cases[:1] + cases[3:5]:
        Y2 = Y.clone()
        got = call(Y2, inplace=True)
        assert got.data_ptr() == Y2.data_ptr() and torch.equal(got, outs[name]), name
    rs, cs = _dev(m["row_sum"], f64), _dev(m["col_sum"], f64)
    out = torch.ops.gpsa.count_transform(Y, "nb_deviance", rs, cs, m["total"], 7.0)
    Y3 = Y.clone()
    assert _ops().count_transform(Y3, "nb_deviance", rs, cs, total=m["total"], theta=7.0, out=Y3) is Y3
    assert torch.equal(Y3, out)
    assert _rel(out.cpu().numpy().astype(np.float64), cu.deviance_residuals(Yh, 7.0)[0]) <= 1e-6
    if N > 1:  # the clip is sqrt(N): it bites on the unclipped theta = 1 residuals or not at all - either way the same
        got = gp.pearson_residuals(Y, 1.0)
        assert float(got.abs().max()) <= np.float32(np.sqrt(N))


def test_the_transform_takes_the_margins_it_is_given():
    """the entry does not care which matrix the margins came from: those of another matrix, and a zero row and column"""
    Yh, _, _ = _data((33, 65))
    rs = np.linspace(5.0, 90.0, 33)
    cs = np.linspace(0.0, 40.0, 65)  # cs[0] = 0: mu = 0 in that column
    rs[7] = 0.0
    Y = _dev(Yh)
    got = torch.ops.gpsa.count_transform(Y, "pearson", _dev(rs, f64), _dev(cs, f64), 1234.5, 3.0, 2.5).cpu().numpy()
    mu = rs[:, None] * cs[None, :] / 1234.5
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(mu > 0, np.clip((Yh - mu) / np.sqrt(mu + mu**2 / 3.0), -2.5, 2.5), 0.0)
    assert _rel(got.astype(np.float64), want) <= 1e-6 and (got[7] == 0).all() and (got[:, 0] == 0).all()
    got = torch.ops.gpsa.count_transform(Y, "log1p", _dev(rs, f64), None, target=50.0).cpu().numpy()
    assert _rel(got.astype(np.float64), cu.normalize_log1p(Yh, 50.0, row_sum=rs)) <= 1e-6 and (got[7] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------
# the z-score per view
# ------------------------------------------------------------------------------------------------------------------------
def _splits(N):
    out = [[N]]
    if N >= 2:
        out.append([N // 2, N - N // 2])
    if N >= 3:
        out.append([N // 3, (N - N // 3) // 2, N - N // 3 - (N - N // 3) // 2])
    if N > RM + 2:
        out.append([RM, 1, N - RM - 1])  # a view of exactly one group, a view of one row
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_standardize_views(shape):
    Yh, m, _ = _data(shape)
    N, P = shape
    # the Pearson residuals as the fp32 matrix to standardise, shifted far from 0 in one column: a large mean with a
    # small spread is where E[y^2] - E[y]^2 would lose everything
    Zh = cu.pearson_residuals(Yh, 100.0).astype(np.float32)
    Zh[:, P - 1] = (4096.0 + Zh[:, P - 1] / 64.0).astype(np.float32)
    Z = _dev(Zh)
    worst = 0.0
    for ns in _splits(N):
        want, nconst = cu.standardize_views(Zh.astype(np.float64), ns)
        res = gp.standardize_views(Z, ns)
        assert res.outputs.dtype == f32 and res.n_constant.dtype == torch.int64
        assert np.array_equal(res.n_constant.cpu().numpy(), nconst), (ns, nconst)
        worst = max(worst, _rel(res.outputs.cpu().numpy().astype(np.float64), want))
        off = [0] + list(np.cumsum(ns))
        out, nc = torch.ops.gpsa.standardize_views(Z, [int(v) for v in off])
        assert torch.equal(out, res.outputs) and torch.equal(nc, res.n_constant)
        Z2 = Z.clone()
        inp = gp.standardize_views(Z2, ns, inplace=True)
        assert inp.outputs.data_ptr() == Z2.data_ptr() and torch.equal(inp.outputs, res.outputs)
    print(f"[counts] {shape}: z-score {worst:.1e} (bar 1e-6 of max(1, |value|))")
    assert worst <= 1e-6
    assert torch.equal(Z, _dev(Zh))
    if m["col_sum"].min() == 0 and N > 1:  # the recipe's empty gene: constant in every view, written as 0 and counted
        g = int(np.argmin(m["col_sum"]))
        res = gp.standardize_views(Z, _splits(N)[1])
        if g != P - 1:
            assert (res.outputs[:, g] == 0).all() and int(res.n_constant.min()) >= 1


def test_a_column_constant_in_one_view_only_is_zero_there_and_counted_there():
    Zh = np.random.default_rng(0).normal(3.0, 2.0, (300, 9)).astype(np.float32)
    Zh[:100, 2] = 7.25   # constant in view 0 only
    Zh[100:, 5] = -1e-3  # constant in view 1 only
    Zh[:, 8] = 0.1       # constant everywhere (0.1 is not exact in fp32: still exactly constant)
    res = gp.standardize_views(_dev(Zh), [100, 200])
    out = res.outputs.cpu().numpy()
    assert res.n_constant.tolist() == [2, 2]
    assert (out[:100, 2] == 0).all() and (out[100:, 5] == 0).all() and (out[:, 8] == 0).all()
    assert np.isfinite(out).all() and abs(out[100:, 2].std() - 1) < 1e-5
    want, nconst = cu.standardize_views(Zh.astype(np.float64), [100, 200])
    assert nconst.tolist() == [2, 2] and _rel(out.astype(np.float64), want) <= 1e-6


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_standardize_views_refuses_a_matrix_that_is_not_finite(value):
    Zh = np.random.default_rng(1).normal(0.0, 1.0, (60, 7)).astype(np.float32)
    Zh[31, 4] = value
    Z = _dev(Zh)
    with pytest.raises(ValueError, match="standardize_views: Y holds NaN or infinite"):
        gp.standardize_views(Z, [30, 30])
    with pytest.raises(ValueError, match="standardize_views: Y holds NaN or infinite"):
        gp.standardize_views(Z, [60], inplace=True)
    assert torch.equal(Z[:31], _dev(Zh[:31]))  # refused before anything was written
    assert gp.standardize_views(_dev(-np.abs(Zh[:31])), [31]).n_constant.tolist() == [0]  # negative values are fine here


# ------------------------------------------------------------------------------------------------------------------------
# the one call
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [[120, 137], [80, 90, 87]], ids=["two views", "three views"])
@pytest.mark.parametrize("transform", counts.TRANSFORMS)
def test_prepare_counts_against_the_yardsticks_pipeline(transform, ns):
    Yh = np.array(_data((257, 130))[0])
    kw = dict(min_counts=float(np.sort(Yh.sum(1))[5]), max_counts=float(np.sort(Yh.sum(1))[-4]), min_cells=20,
              n_top_genes=40, transform=transform, theta=50.0)
    want = cu.prepare(Yh, ns, **kw)
    gaps = cu.smallest_relative_gap(want["deviance"])
    assert gaps >= 1e-9, gaps  # the selection is then decided by the values alone
    Y = _dev(Yh)
    res = gp.prepare_counts(Y, ns, **kw)
    assert torch.equal(Y, _dev(Yh))
    assert np.array_equal(res.rows.cpu().numpy(), want["rows"]) and 200 < len(want["rows"]) < 257
    assert np.array_equal(res.genes.cpu().numpy(), want["genes"]) and len(want["genes"]) == 40
    assert res.rows.dtype == torch.int64 and res.genes.dtype == torch.int64
    assert res.n_samples_list == want["n_samples_list"]
    parts = cu.poisson_deviance(Yh[want["rows"]])
    assert (np.abs(res.deviance.cpu().numpy() - want["deviance"]) <= 1e-11 * (parts["abs_sat"] + np.abs(parts["ll_null"]))).all()
    err = _rel(res.outputs.cpu().numpy().astype(np.float64), want["outputs"])
    print(f"[counts] prepare_counts {transform} {ns}: outputs {err:.1e} (bar 1e-6 of max(1, |value|))")
    assert res.outputs.dtype == f32 and err <= 1e-6
    if transform == "counts":
        assert res.n_constant is None and res.log_offset.dtype == f32
        assert np.abs(res.log_offset.cpu().numpy() - want["log_offset"]).max() <= 1e-6
        assert np.array_equal(res.outputs.cpu().numpy(), Yh[want["rows"]][:, want["genes"]])
    else:
        assert res.log_offset is None and np.array_equal(res.n_constant.cpu().numpy(), want["n_constant"])
        a = 0
        for n in res.n_samples_list if int(res.n_constant.sum()) == 0 else []:  # every view: mean 0 and unit population std per gene
            blk = res.outputs[a: a + n].double()
            assert float(blk.mean(0).abs().max()) <= 1e-5 and float((blk.std(0, unbiased=False) - 1).abs().max()) <= 1e-5
            a += n
    # without standardisation: the transform's own values
    if transform in ("pearson", "deviance", "log1p"):
        res2 = gp.prepare_counts(Y, ns, standardize=False, **kw)
        want2 = cu.prepare(Yh, ns, standardize=False, **kw)
        assert res2.n_constant is None and _rel(res2.outputs.cpu().numpy().astype(np.float64), want2["outputs"]) <= 1e-6


def test_prepare_counts_never_hands_back_the_callers_own_tensor():
    Yh = np.array(_data((97, 45))[0])
    Y = _dev(Yh)
    for transform in counts.TRANSFORMS:
        res = gp.prepare_counts(Y, [50, 47], transform=transform, standardize=False)
        assert res.rows.numel() == 97 and res.genes.numel() == 45  # nothing dropped: the case where it could
        assert res.outputs.data_ptr() != Y.data_ptr() and torch.equal(Y, _dev(Yh)), transform
    res = gp.prepare_counts(Y, [50, 47], transform="counts")
    assert torch.equal(res.outputs, Y)
    res.outputs.zero_()
    assert torch.equal(Y, _dev(Yh))


def test_refusals_carry_the_name_of_the_call_that_was_made():
    Yh = np.array(_data((97, 45))[0])
    Yh[3] = 0.0
    with pytest.raises(ValueError, match=r"^deviance_feature_selection: 1 of 97 rows have no counts"):
        gp.deviance_feature_selection(_dev(Yh))
    with pytest.raises(ValueError, match=r"^poisson_deviance: 1 of 97 rows have no counts"):
        gp.poisson_deviance(_dev(Yh))
    Yh[5, 5] = -2.0
    with pytest.raises(ValueError, match=r"^deviance_feature_selection: Y holds 1 entries"):
        gp.deviance_feature_selection(_dev(Yh))


def test_the_drop_in_names_end_to_end():
    """gpsa.util's five names on the device, in the reference's orientations (genes x cells for the first three), against
    the yardstick: size factors 1e-13 relative, deviance 1e-11 (abs_sat + |ll_null|), residuals 1e-6 max(1, |value|)"""
    import gpsa.util

    Yh, m, d = _data((97, 45))
    some = m["col_sum"] > 0
    sz = gpsa.util.compute_size_factors(Yh.T)
    assert isinstance(sz, np.ndarray) and sz.dtype == np.float64 and sz.shape == (97,)
    assert np.abs(sz / cu.size_factors(Yh) - 1).max() <= 1e-13
    mine = np.exp(np.linspace(-0.3, 0.4, 97))  # size factors of the caller's: the wrapper takes their log on the device
    w = cu.poisson_deviance(Yh, np.log(mine))
    dev = gpsa.util.poisson_deviance(Yh.T, mine)
    assert list(dev.index) == list(range(45))
    assert (np.abs(dev.values - w["deviance"]) <= 1e-11 * (w["abs_sat"] + np.abs(w["ll_null"]))).all()
    devs, names = gpsa.util.deviance_feature_selection(Yh.T)
    assert np.array_equal(names, np.nonzero(some)[0]) and devs.shape == (int(some.sum()),)  # the gene without counts is dropped
    assert (np.abs(devs - d["deviance"][some]) <= 1e-11 * (d["abs_sat"] + np.abs(d["ll_null"]))[some]).all()
    z = gpsa.util.pearson_residuals(Yh, 100.0)
    assert z.dtype == np.float64 and _rel(z, cu.pearson_residuals(Yh, 100.0)) <= 1e-6
    assert _rel(gpsa.util.pearson_residuals(Yh, 1.0, clipping=False), cu.pearson_residuals(Yh, 1.0, clipping=False)) <= 1e-6
    for theta in (100.0, np.inf):
        assert _rel(gpsa.util.deviance_residuals(Yh, theta), cu.deviance_residuals(Yh, theta)[0]) <= 1e-6


def test_the_drop_in_names_keep_a_data_frames_labels_end_to_end():
    import gpsa.util

    pd = pytest.importorskip("pandas")
    Yh, m, _ = _data((97, 45))
    some = m["col_sum"] > 0
    mine = np.exp(np.linspace(-0.3, 0.4, 97))
    frame = pd.DataFrame(Yh.T, index=[f"g{g}" for g in range(45)])
    s = gpsa.util.poisson_deviance(frame, mine)
    assert isinstance(s, pd.Series) and list(s.index) == list(frame.index)
    assert np.array_equal(s.values, gpsa.util.poisson_deviance(Yh.T, mine).values)
    devs, names = gpsa.util.deviance_feature_selection(frame)
    assert list(names) == [f"g{g}" for g in np.nonzero(some)[0]]
    assert np.array_equal(devs, gpsa.util.deviance_feature_selection(Yh.T)[0])
    assert np.array_equal(gpsa.util.compute_size_factors(frame), gpsa.util.compute_size_factors(Yh.T))


def test_log_offset_goes_straight_into_a_negative_binomial_loss():
    from spatial_alignment_amd import simulate
    from spatial_alignment_amd.synthetic import make_model

    X, Fl, nsl, _ = simulate.generate_twod_data(2, 6, 8, noise_variance=0.0, seed=0)
    n = int(nsl[0])
    gen = torch.Generator().manual_seed(1)
    depth = 0.5 * torch.randn(2 * n, generator=gen) + 1.5
    Y = torch.poisson(torch.exp(Fl + depth[:, None]), generator=gen)
    res = gp.prepare_counts(Y.to(DEV), [n, n], min_counts=1, n_top_genes=4, transform="counts")
    assert tuple(res.outputs.shape) == (sum(res.n_samples_list), 4) and res.log_offset.dtype == f32
    assert abs(float(res.log_offset.double().mean())) <= 1e-6  # geometric mean 1
    rows = res.rows.cpu()
    dd = simulate.as_data_dict(X[rows], res.outputs, res.n_samples_list)
    dd["expression"]["log_offset"] = res.log_offset
    dd = {m: {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()} for m, d in dd.items()}
    model = make_model(dd, m=9, device=torch.device(DEV))
    model.likelihood = "negative_binomial"
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    out = model.forward({"expression": dd["expression"]["spatial_coords"]}, view_idx=view_idx, Ns=Ns, S=2)
    loss = model.loss_fn(dd, out[3])
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(model.log_dispersion["expression"].grad).all())


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI's refusals, on device memory: the documented code, and nothing written
# ------------------------------------------------------------------------------------------------------------------------
def test_the_entries_refuse_with_the_documented_codes_and_write_nothing():
    lib = _lib()
    Yh, m, _ = _data((33, 65))
    Y = _dev(Yh)
    N, P = Y.shape
    assert _margins_raw(Y, short=8)[0] == EWORKSPACE
    rc, rs, cs, rn, cn, bad = _margins_raw(Y, short=8)
    assert (rs == -7).all() and (cs == -7).all() and (rn == -7).all() and (cn == -7).all() and bad == -7
    need = lib.gpsa_count_workspace(N, P)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    a, b = (torch.full((P,), -7.0, dtype=f64, device=DEV) for _ in range(2))
    lsz = torch.zeros(N, dtype=f64, device=DEV)
    s = _stream()
    dev = lambda Yp=Y.data_ptr(), n=N, p=P, l=lsz.data_ptr(), w=ws.data_ptr(), nb=need: \
        lib.gpsa_count_deviance_f32(Yp, n, p, l, a.data_ptr(), b.data_ptr(), w, nb, s)
    assert dev(Yp=None) == EINVAL and dev(l=None) == EINVAL and dev(n=0) == EINVAL and dev(p=0) == EINVAL
    assert dev(nb=need - 8) == EWORKSPACE and dev(w=None) == EWORKSPACE
    rsd, csd = _dev(m["row_sum"], f64), _dev(m["col_sum"], f64)
    out = torch.full((N, P), -7.0, dtype=f32, device=DEV)

    def tr(mode=0, Yp=Y.data_ptr(), n=N, p=P, r=rsd.data_ptr(), c=csd.data_ptr(), total=m["total"], theta=100.0, clip=0.0,
           target=1.0, o=out.data_ptr()):
        return lib.gpsa_count_transform_f32(mode, Yp, n, p, r, c, total, theta, clip, target, o, s)

    for kw in (dict(mode=4), dict(mode=-1), dict(Yp=None), dict(r=None), dict(c=None), dict(o=None), dict(n=0), dict(p=0),
               dict(theta=0.0), dict(theta=-2.0), dict(mode=1, theta=0.0), dict(mode=1, theta=float("inf")),
               dict(total=0.0), dict(mode=3, target=0.0)):
        assert tr(**kw) == EINVAL, kw
    nc = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    std = lambda vo=(0, 20, 33), V=2, w=ws.data_ptr(), nb=need, Yp=Y.data_ptr(): lib.gpsa_standardize_views_f32(
        Yp, N, P, None if vo is None else (C.c_longlong * len(vo))(*vo), V, out.data_ptr(), nc.data_ptr(), w, nb, s)
    for kw in (dict(vo=None), dict(V=0), dict(vo=(1, 20, 33)), dict(vo=(0, 20, 34)), dict(vo=(0, 0, 33)), dict(Yp=None)):
        assert std(**kw) == EINVAL, kw
    assert std(nb=need - 8) == EWORKSPACE and std(w=None) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((a == -7).all()) and bool((b == -7).all()) and bool((out == -7).all()) and bool((nc == -7).all())
    with pytest.raises(ValueError, match="contiguous fp32"):
        _ops().count_margins(Y.double())
    with pytest.raises(ValueError, match="mode must be"):
        _ops().count_transform(Y, "sqrt", rsd, csd)
    with pytest.raises(ValueError, match="view_off"):
        _ops().standardize_views(Y, [0, 40, 33])
    for bad_out in (torch.empty(N, P + 1, device=DEV), torch.empty(N, P, dtype=f64, device=DEV),
                    torch.empty(N, 2 * P, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="out must be a contiguous fp32"):
            _ops().count_transform(Y, "pearson", rsd, csd, total=m["total"], theta=100.0, out=bad_out)
        with pytest.raises(ValueError, match="out must be a contiguous fp32"):
            _ops().standardize_views(Y, [0, 20, 33], out=bad_out)
