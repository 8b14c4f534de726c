"""The register-resident fp32 contraction kernels through the C ABI alone, element by element against the same operation in
fp64, at the edges of their row-tile classes, column tiles, item splits and Gram splits:

  gpsa_quadform_fwd                                   quad_sym_mfma_kernel                                M <= 384
  gpsa_quadform_fwd_keep_f32 -> _bwd_alpha_kept_f32   panel_mfma_kernel<QUAD> with keep, kept_wsum_kernel M <= 256
  gpsa_quadform_bwd_alpha                             panel_mfma_kernel<ACCUM> + panel_slab_reduce_kernel M <= 512
  gpsa_panel_mm                                       panel_mfma_kernel<STORE>                            M <= 256
  gpsa_quadform_bwd_omega, _bwd_omega_delta_f32       gram_mfma_kernel + gram_reduce_kernel               M <= 256

References: fp64 from the fp32 inputs widened, on the CPU (on the device with torch above 1e10 flop).  Bounds: derived in
tests/contraction_util.py, never measured; every test asserts error <= bound element by element and the module prints the
largest ratio per entry and input family when it finishes.

Guards on every call: every output is a view inside a NaN-filled frame, intact afterwards and NaN-free itself; every input
(alpha, Omega, g, dmeanT, dcT, P, X, the kept products) sits in a NaN-filled frame too, so a load past row M or column C
that reaches an MFMA poisons the result; every workspace is a fresh buffer of exactly the queried size, every byte 0xFF;
every call runs twice and repeats bit for bit; nothing skips.  The edge-weighted family's visibility condition (a lost
named row or column moves half of what it feeds by more than 4 x the bound) is asserted again here, from the reference.

Which kernel ran cannot be observed from here: the shapes are chosen by reading the launchers, and
tests/test_contraction_shapes.py holds every such claim to the library's pure queries without a GPU.
"""
import time

import pytest
import torch

import contraction_util as cu
from contraction_util import EUNSUPPORTED, EWORKSPACE, Frame, f32, f64, poisoned, ratio, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODE = {f32: 0, f64: 1, "Om32": 0, "Om64": 1, "P32": 0, "P64": 1}
RATIOS = {}
T0 = time.time()
CLASSES_256 = (2, 4, 7, 13, 16)


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    assert torch.cuda.get_device_properties(0).multi_processor_count == cu.CUS, "the shape lists are written for 256 CUs"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"[contraction] largest error / bound  {k[0]:34s} {k[1]:7s} {RATIOS[k]:.3f}")
    print(f"[contraction] module wall time {time.time() - T0:.1f} s")


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def p(t):
    return 0 if t is None else t.data_ptr()


def frames(inp, off=None):
    """every input tensor inside its own NaN frame on the device"""
    return {k: Frame(t.shape, t.dtype, DEV, src=t.to(DEV), off=(off or {}).get(k, 0)) for k, t in inp.items()}


def rdev(flops):
    return DEV if flops > 1e10 else "cpu"


def on(dev, *ts):
    return [t.to(dev) for t in ts]


def check(entry, family, got, want, bound, what):
    r = ratio(got, want.reshape(got.shape), bound.reshape(got.shape))
    RATIOS[(entry, family)] = max(RATIOS.get((entry, family), 0.0), r)
    assert r <= 1, f"{entry} {what}: error / bound {r:.3f}"
    return r


def twice(once):
    a, b = once(), once()
    assert len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b)), "not repeatable bit for bit"
    return a


# ---- one call of each entry, with the guards ---------------------------------------------------------------------------
def run_fwd(lib, F, om, M, C, L):
    def once():
        v = Frame((L, C), f32, DEV)
        wsb = int(lib.gpsa_quadform_workspace(0, M, C, L))
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_quadform_fwd(0, CODE[om], F["al"].ptr(), F[om].ptr(), M, C, L, v.ptr(), p(ws), wsb, stream())
        torch.cuda.synchronize()
        assert rc == 0 and v.intact() and v.written(), (rc, M, C, L)
        return (v.view,)
    return twice(once)[0]


def run_bwd_alpha(lib, F, om, M, C, L):
    def once():
        out = Frame((M, C), f32, DEV)
        wsb = int(lib.gpsa_quadform_workspace(0, M, C, L))
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_quadform_bwd_alpha(0, CODE[om], F["al"].ptr(), F[om].ptr(), F["g"].ptr(), M, C, L, out.ptr(), p(ws),
                                         wsb, stream())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() and out.written(), (rc, M, C, L)
        return (out.view,)
    return twice(once)[0]


def run_keep(lib, F, om, M, C, L):
    """-> (v, dalpha without the mean term, dalpha with it): the forward that keeps its products in a buffer of exactly
    gpsa_quadform_keep_f32_bytes inside a NaN frame, and the streaming backward over that buffer"""
    def once():
        wsb, nb = int(lib.gpsa_quadform_keep_f32_workspace(M, L)), int(lib.gpsa_quadform_keep_f32_bytes(M, C, L))
        assert wsb == cu.keep_workspace(M, L) and nb == cu.keep_bytes(M, C, L)
        ws, v, W = poisoned(wsb, DEV), Frame((L, C), f32, DEV), Frame(nb // 4, f32, DEV)
        rc = lib.gpsa_quadform_fwd_keep_f32(CODE[om], F["al"].ptr(), F[om].ptr(), M, C, L, v.ptr(), W.ptr(), p(ws), wsb,
                                            stream())
        torch.cuda.synchronize()
        assert rc == 0 and v.intact() and v.written() and W.intact() and W.written(), (rc, M, C, L)
        d0, d1 = Frame((M, C), f32, DEV), Frame((M, C), f32, DEV)
        rc0 = lib.gpsa_quadform_bwd_alpha_kept_f32(W.ptr(), F["g"].ptr(), M, C, L, None, None, d0.ptr(), stream())
        rc1 = lib.gpsa_quadform_bwd_alpha_kept_f32(W.ptr(), F["g"].ptr(), M, C, L, F["dc"].ptr(), F["dm"].ptr(), d1.ptr(),
                                                   stream())
        torch.cuda.synchronize()
        assert rc0 == 0 and rc1 == 0 and all(d.intact() and d.written() for d in (d0, d1)) and W.intact(), (M, C, L)
        return (v.view, d0.view, d1.view, W.view)
    return twice(once)[:3]


def run_mm(lib, F, pk, tp, M, C, colsq=True):
    def once():
        Y, q = Frame((M, C), f32, DEV), (Frame((C,), f32, DEV) if colsq else None)
        wsb = cu.panel_mm_workspace(M)  # (no query: include/gpsa_hip.h states the size)
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_panel_mm(0, CODE[pk], tp, F[pk].ptr(), F["X"].ptr(), M, C, Y.ptr(), q.ptr() if q else 0, p(ws), wsb,
                               stream())
        torch.cuda.synchronize()
        assert rc == 0 and Y.intact() and Y.written() and (q is None or (q.intact() and q.written())), (rc, M, C)
        return (Y.view,) + ((q.view,) if q else ())
    return twice(once)


def run_gram(lib, F, M, C, L, out_dt, delta=None):
    """delta: None (gpsa_quadform_bwd_omega) or (ddelta0 on the CPU or None, dbeta): gpsa_quadform_bwd_omega_delta_f32"""
    def once():
        dOm = Frame((L, M, M), out_dt, DEV)
        wsb = int(lib.gpsa_quadform_workspace(0, M, C, L))
        ws = poisoned(wsb, DEV)
        if delta is None:
            rc = lib.gpsa_quadform_bwd_omega(0, CODE[out_dt], F["al"].ptr(), F["g"].ptr(), M, C, L, dOm.ptr(), p(ws), wsb,
                                             stream())
            dd = None
        else:
            dd0, dbeta = delta
            dd = Frame((M, L), f32, DEV, src=None if dd0 is None else dd0.to(DEV))  # dbeta = 0: NaN, never read
            rc = lib.gpsa_quadform_bwd_omega_delta_f32(CODE[out_dt], F["al"].ptr(), F["g"].ptr(), F["dm"].ptr(), M, C, L,
                                                       dOm.ptr(), dd.ptr(), float(dbeta), p(ws), wsb, stream())
        torch.cuda.synchronize()
        assert rc == 0 and dOm.intact() and dOm.written() and (dd is None or (dd.intact() and dd.written())), (rc, M, C, L)
        assert torch.equal(dOm.view, dOm.view.transpose(1, 2)), "dOmega is not exactly symmetric"
        return (dOm.view,) + ((dd.view,) if dd is not None else ())
    return twice(once)


# ---- checks shared by the lists ----------------------------------------------------------------------------------------
def rows_visible(kind, family, al, Om, g, bound, M, extra=None):
    """the visibility condition for every named row (edge-weighted family only), from the reference alone"""
    if family != "edge":
        return
    for r in cu.named_rows(M):
        if kind == "v":
            d = cu.drop_row_v(al, Om, r)
        elif kind == "dalpha":
            d = cu.drop_row_dalpha(al, Om, g, r)
        else:
            d = cu.drop_row_mm(al, Om, extra, r)  # (P, X, transP)
        assert cu.visible(d, bound), (kind, M, r)


def check_fwd(lib, entry, family, inp, F, om, M, C, L):
    dev = rdev(4.0 * L * M * M * C)
    al, Om = on(dev, inp["al"], inp[om])
    want, bound = cu.ref_v(al, Om)
    check(entry, family, run_fwd(lib, F, om, M, C, L), want, bound, (M, C, L, om))
    rows_visible("v", family, al, Om, None, bound, M)


def check_bwd_alpha(lib, entry, family, inp, F, om, M, C, L):
    dev = rdev(4.0 * L * M * M * C)
    al, Om, g = on(dev, inp["al"], inp[om], inp["g"])
    want, bound = cu.ref_dalpha(al, Om, g)
    check(entry, family, run_bwd_alpha(lib, F, om, M, C, L), want, bound, (M, C, L, om))
    rows_visible("dalpha", family, al, Om, g, bound, M)


def check_keep(lib, entry, family, inp, F, om, M, C, L):
    dev = rdev(6.0 * L * M * M * C)
    al, Om, g, dc, dm = on(dev, inp["al"], inp[om], inp["g"], inp["dc"], inp["dm"])
    v, d0, d1 = run_keep(lib, F, om, M, C, L)
    want, bound = cu.ref_v(al, Om)
    check(entry + " v", family, v, want, bound, (M, C, L, om))
    rows_visible("v", family, al, Om, None, bound, M)
    want, bound = cu.ref_dalpha(al, Om, g, kept=True)
    check(entry + " dalpha", family, d0, want, bound, (M, C, L, om))
    rows_visible("dalpha", family, al, Om, g, bound, M)
    want, bound = cu.ref_dalpha(al, Om, g, kept=True, dc=dc, dm=dm)
    check(entry + " dalpha+mean", family, d1, want, bound, (M, C, L, om))


def check_mm(lib, entry, family, pan, F, pk, tp, M, C, colsq=True):
    Y, E, q, bq = cu.ref_mm(pan[pk], pan["X"], tp)
    got = run_mm(lib, F, pk, tp, M, C, colsq)
    check(entry + " Y", family, got[0], Y, E, (M, C, pk, tp))
    if colsq:
        check(entry + " colsq", family, got[1], q, bq, (M, C, pk, tp))
    rows_visible("Y", family, pan[pk], pan["X"], None, E, M, extra=tp)


def check_gram(lib, entry, family, inp, F, M, C, L, cols=(), delta=True, out_dts=(f32, f64)):
    """the plain entry in both output types; the delta entry, where the shape and the alignment allow it, with dbeta 0 and
    1 - its dOmega equal to the plain entry's bit for bit"""
    dev = rdev(8.0 * L * M * M * C)
    al, g, dm = on(dev, inp["al"], inp["g"], inp["dm"])
    plain = {}
    for dt in out_dts:
        want, bound = cu.ref_gram(al, g, stored32=dt == f32)
        plain[dt] = run_gram(lib, F, M, C, L, dt)[0]
        check(entry + (" fp32" if dt == f32 else " fp64"), family, plain[dt], want, bound, (M, C, L))
        if family == "edge" and dt == f32:
            for c in cols:
                assert cu.visible(cu.drop_col_gram(al, g, c), bound), ("dOmega", M, C, c)
    takes = bool(lib.gpsa_quadform_bwd_omega_takes_delta(M, C))
    assert takes == cu.takes_delta(M, C)
    if not (delta and takes):
        return
    base = torch.randn(M, L, generator=torch.Generator().manual_seed(M + L), dtype=f64).float()
    for i, (dd0, dbeta) in enumerate([(None, 0.0), (base, 1.0)]):
        dt = out_dts[i % len(out_dts)]
        dOm, dd = run_gram(lib, F, M, C, L, dt, delta=(dd0, dbeta))
        assert same_bits(dOm, plain[dt]), "the delta entry's dOmega differs from the plain entry's"
        want, bound = cu.ref_ddelta(al, dm, None if dd0 is None else dd0.to(dev), dbeta)
        check(entry + " ddelta", family, dd, want, bound, (M, C, L, dbeta))
        if family == "edge" and i == 0:
            for c in cols:
                assert cu.visible(cu.drop_col_ddelta(al, dm, c), bound), ("ddelta", M, C, c)


# ---- row classes: M = 1 and the edges of every row-tile class, one full column tile and a tail of 5 / 4 columns ---------
def _row_cases(M):
    return [(C, fam, k) for C in cu.row_class_columns(cu.mb_for(M)) for fam in ("edge", "graded") for k in (32, 64)]


@pytest.mark.parametrize("M", cu.ROWS_384)
def test_rows_quadform_fwd(lib, M):
    for C, fam, k in _row_cases(M):
        inp = cu.make_inputs(M, C, cu.ROW_L, fam, out="cols")
        check_fwd(lib, "quadform_fwd", fam, inp, frames(inp), f"Om{k}", M, C, cu.ROW_L)


@pytest.mark.parametrize("M", cu.ROWS_256)
def test_rows_quadform_keep(lib, M):
    for C, fam, k in _row_cases(M):
        inp = cu.make_inputs(M, C, cu.ROW_L, fam, out="rows")
        check_keep(lib, "fwd_keep_f32", fam, inp, frames(inp), f"Om{k}", M, C, cu.ROW_L)


@pytest.mark.parametrize("M", cu.ROWS_512)
def test_rows_quadform_bwd_alpha(lib, M):
    for C, fam, k in _row_cases(M):
        inp = cu.make_inputs(M, C, cu.ROW_L, fam, out="rows")
        check_bwd_alpha(lib, "quadform_bwd_alpha", fam, inp, frames(inp), f"Om{k}", M, C, cu.ROW_L)


@pytest.mark.parametrize("M", cu.ROWS_256)
def test_rows_panel_mm(lib, M):
    for C, fam, k in _row_cases(M):
        pan = cu.make_panel(M, C, fam)
        F = frames(pan)
        for tp in (0, 1):
            check_mm(lib, "panel_mm", fam, pan, F, f"P{k}", tp, M, C, colsq=(tp == 0) == (k == 32))


@pytest.mark.parametrize("M", cu.ROWS_256)
def test_rows_quadform_bwd_omega(lib, M):
    """both entries: the delta form is taken at every M of the list with a padding row behind it, on the 4-column tail"""
    for C in cu.row_class_columns(cu.mb_for(M)):
        for fam in ("edge", "graded"):
            cols = cu.named_cols_gram(M, C, cu.ROW_L)
            inp = cu.make_inputs(M, C, cu.ROW_L, fam, out="gram", gram_cols=cols)
            check_gram(lib, "bwd_omega", fam, inp, frames(inp), M, C, cu.ROW_L, cols)


# ---- item split of the persistent kernels ------------------------------------------------------------------------------
def _split_params(limit):
    return [pytest.param(MB, i, id=f"MB{MB}-{cu.split_cases(MB)[i][3]}-{i}") for MB in cu.MB_CLASSES if MB <= limit
            for i in range(len(cu.split_cases(MB)))]


def _split_inputs(MB, i, out):
    M, C, L, what = cu.split_cases(MB)[i]
    fam = "graded" if what == "T=G" and i >= 2 else "edge"
    return M, C, L, fam, cu.make_inputs(M, C, L, fam, out=out), ("Om64" if i % 2 else "Om32")


@pytest.mark.parametrize("MB,i", _split_params(24))
def test_split_quadform_fwd(lib, MB, i):
    M, C, L, fam, inp, om = _split_inputs(MB, i, "cols")
    check_fwd(lib, "quadform_fwd", fam, inp, frames(inp), om, M, C, L)


@pytest.mark.parametrize("MB,i", _split_params(16))
def test_split_quadform_keep(lib, MB, i):
    M, C, L, fam, inp, om = _split_inputs(MB, i, "rows")
    check_keep(lib, "fwd_keep_f32", fam, inp, frames(inp), om, M, C, L)


@pytest.mark.parametrize("MB,i", _split_params(32))
def test_split_quadform_bwd_alpha(lib, MB, i):
    M, C, L, fam, inp, om = _split_inputs(MB, i, "rows")
    check_bwd_alpha(lib, "quadform_bwd_alpha", fam, inp, frames(inp), om, M, C, L)


@pytest.mark.parametrize("M,C,L", cu.SOFF_SHAPES)
def test_slab_reduce_with_512_contributors(lib, M, C, L):
    """one column tile shared by all 512 workgroups: panel_slab_reduce_kernel's offset table exactly full"""
    for fam in ("plain", "edge"):
        inp = cu.make_inputs(M, C, L, fam, outputs=cu.named_outputs(L))
        check_bwd_alpha(lib, "quadform_bwd_alpha", fam, inp, frames(inp), "Om32", M, C, L)
    # (edge family, still in ``inp``) a lost contributor is visible as a lost row is
    _, bound = cu.ref_dalpha(inp["al"], inp["Om32"], inp["g"])
    for l in cu.named_outputs(L):
        assert cu.visible(cu.drop_output_dalpha(inp["al"], inp["Om32"], inp["g"], l), bound), (M, C, L, l)


@pytest.mark.parametrize("MB", CLASSES_256)
def test_store_column_tiles(lib, MB):
    """gpsa_panel_mm runs one workgroup per tile: a single column, one column short of a tile, a full tile, one over"""
    for i, C in enumerate(cu.STORE_C(MB)):
        M = (cu.M_SMALL if i % 2 else cu.M_LARGE)[MB]
        for fam in ("edge", "graded"):
            pan = cu.make_panel(M, C, fam)
            F = frames(pan)
            for tp in (0, 1):
                check_mm(lib, "panel_mm", fam, pan, F, "P64" if (i + tp) % 2 else "P32", tp, M, C, colsq=bool((i + tp) % 2) or C == 1)


# ---- kept_wsum_kernel: the pair loop's tail and the mean term's l guard --------------------------------------------------
@pytest.mark.parametrize("L", cu.KEPT_L)
@pytest.mark.parametrize("MB", CLASSES_256)
def test_kept_products_consumer(lib, MB, L):
    M = (cu.M_SMALL if L % 2 else cu.M_LARGE)[MB]
    C = cu.width(MB) + 5
    for fam in ("plain", "edge", "graded"):
        inp = cu.make_inputs(M, C, L, fam, out="rows")
        check_keep(lib, "fwd_keep_f32", fam, inp, frames(inp), "Om32", M, C, L)


def test_keep_refuses_a_short_workspace(lib):
    M, C, L = 57, 300, 3
    inp = cu.make_inputs(M, C, L, "plain")
    F = frames(inp)
    wsb, nb = int(lib.gpsa_quadform_keep_f32_workspace(M, L)), int(lib.gpsa_quadform_keep_f32_bytes(M, C, L))
    ws, v, W = poisoned(wsb - 1, DEV), Frame((L, C), f32, DEV), Frame(nb // 4, f32, DEV)
    rc = lib.gpsa_quadform_fwd_keep_f32(0, F["al"].ptr(), F["Om32"].ptr(), M, C, L, v.ptr(), W.ptr(), p(ws), wsb - 1, stream())
    torch.cuda.synchronize()
    assert rc == EWORKSPACE and v.untouched() and W.untouched() and bool((ws == 0xFF).all())


# ---- Gram ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", cu.GRAM_CHUNKS_C)
@pytest.mark.parametrize("MB", CLASSES_256)
def test_gram_more_than_one_chunk_per_workgroup(lib, MB, C):
    """9 chunks in 3 splits of 3, 10 chunks in splits of 2, 3, 2, 3: the stage-ahead path and the buffer flip"""
    M, L = cu.M_LARGE[MB], cu.GRAM_CHUNKS_L
    cols = cu.named_cols_gram(M, C, L)
    for fam in ("edge", "graded"):
        inp = cu.make_inputs(M, C, L, fam, out="gram", gram_cols=cols)
        check_gram(lib, "bwd_omega", fam, inp, frames(inp), M, C, L, cols, out_dts=(f32, f64) if fam == "edge" else (f64,))


@pytest.mark.parametrize("L", cu.GRAM_NL_L)
@pytest.mark.parametrize("MB", CLASSES_256)
def test_gram_two_outputs_per_workgroup(lib, MB, L):
    """129 chunks in 26 splits, two outputs per workgroup for MB <= 13 (L = 15: the last workgroup's second output is the
    clamped surplus that must not be stored); MB = 16 is the one-output contrast.  The delta form rides along"""
    M, C = cu.M_SMALL[MB] if L % 2 else cu.M_LARGE[MB], cu.GRAM_NL_C
    cols = cu.named_cols_gram(M, C, L)
    for fam in ("edge", "graded"):  # (the named columns carry the edge family's sums: the unnamed splits show in the other)
        inp = cu.make_inputs(M, C, L, fam, out="gram", gram_cols=cols)
        check_gram(lib, "bwd_omega", fam, inp, frames(inp), M, C, L, cols, out_dts=(f32, f64) if fam == "edge" else (f64,))


@pytest.mark.parametrize("C", cu.GRAM_NL_EDGE)
@pytest.mark.parametrize("M", [cu.M_SMALL[2], cu.M_LARGE[13]])
def test_gram_both_sides_of_two_outputs(lib, M, C):
    cols = cu.named_cols_gram(M, C, 3)
    for fam in ("edge", "graded"):
        inp = cu.make_inputs(M, C, 3, fam, out="gram", gram_cols=cols)
        check_gram(lib, "bwd_omega", fam, inp, frames(inp), M, C, 3, cols, out_dts=(f32,) if fam == "edge" else (f64,))


@pytest.mark.parametrize("M,C,L", cu.GRAM_SPLITS)
def test_gram_splits(lib, M, C, L):
    """256 splits of one chunk, 129 splits, and more outputs than CUs with one split of 5 chunks"""
    cols = cu.named_cols_gram(M, C, L)
    for fam in ("edge", "plain"):
        inp = cu.make_inputs(M, C, L, fam, out="gram", gram_cols=cols)
        check_gram(lib, "bwd_omega", fam, inp, frames(inp), M, C, L, cols)


@pytest.mark.parametrize("C", cu.GRAM_TAIL_C)
@pytest.mark.parametrize("M", [cu.M_SMALL[2], cu.M_LARGE[13]])
def test_gram_alignment_and_tails(lib, M, C):
    """C < 8 or C % 4 != 0 is meant for the ALIGNED = false kernel; the aligned ones have a last chunk of 8 .. 64 columns
    and one of 4 behind a full chunk"""
    cols = cu.named_cols_gram(M, C, 3)
    for fam in ("edge", "graded"):
        inp = cu.make_inputs(M, C, 3, fam, out="gram", gram_cols=cols)
        check_gram(lib, "bwd_omega", fam, inp, frames(inp), M, C, 3, cols)


@pytest.mark.parametrize("which", ["al", "g"])
@pytest.mark.parametrize("M,C", [(cu.M_SMALL[2], 68), (cu.M_LARGE[13], 580), (cu.M_LARGE[7], 8252)])
def test_gram_misaligned_operands(lib, M, C, which):
    """alpha one element off 16 bytes: the ALIGNED = false kernel at an aligned C; g alone off: the aligned kernel on the
    padded copy of g.  The delta entry refuses either (and a misaligned dmeanT) with nothing written"""
    L = 3
    cols = cu.named_cols_gram(M, C, L)
    inp = cu.make_inputs(M, C, L, "edge", out="gram", gram_cols=cols)
    F = frames(inp, off={which: 1})
    assert F[which].ptr() % 16 == 4 and all(F[k].ptr() % 16 == 0 for k in F if k != which)
    check_gram(lib, "bwd_omega", "edge", inp, F, M, C, L, cols, delta=False)
    assert lib.gpsa_quadform_bwd_omega_takes_delta(M, C) == 1
    for bad in (which, "dm"):
        Fb = frames(inp, off={bad: 1})
        dOm, dd = Frame((L, M, M), f64, DEV), Frame((M, L), f32, DEV)
        wsb = int(lib.gpsa_quadform_workspace(0, M, C, L))
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_quadform_bwd_omega_delta_f32(1, Fb["al"].ptr(), Fb["g"].ptr(), Fb["dm"].ptr(), M, C, L, dOm.ptr(),
                                                   dd.ptr(), 0.0, p(ws), wsb, stream())
        torch.cuda.synchronize()
        assert rc == EUNSUPPORTED and dOm.untouched() and dd.untouched() and bool((ws == 0xFF).all()), (bad, rc)
