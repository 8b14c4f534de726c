"""gram_x3_kernel, split_image_kernel and gram_reduce_kernel behind them (csrc/qf_x3.hip, csrc/qf_gram.hip) through the C ABI
alone - gpsa_quadform_bwd_omega_x3 with out_dtype fp32 and fp64, gpsa_quadform_bwd_omega_delta_x3 - element by element
against the same sums in fp64: at every row-tile class edge, 32-column chunks with 8-column lane
groups partly past C, several chunks per workgroup, up to 256 splits, more outputs than CUs, the delta entry at the column
counts and operand alignments the fp32 delta entry refuses, and the three-piece case at C = 1.

References: fp64 from the fp32 inputs widened, on the CPU (on the device with torch above 1e10 flop, as section 2e).  Bounds:
tests/x3_util.py gram_bars, derived, never measured.  Guards on every call: dOmega and ddelta are views inside NaN-filled
frames, intact afterwards and NaN-free themselves; alpha, g and dmeanT sit in NaN frames of their own, so a load past row M
or column C that reaches an MFMA poisons the result; the workspace is exactly the queried size, every byte 0xFF; every call
runs twice and repeats bit for bit; dOmega is exactly symmetric; the delta entry's dOmega is bit-equal to the plain
entry's; nothing skips.
"""
import time

import pytest
import torch

import contraction_util as cu
import x3_util as xu
from contraction_util import EUNSUPPORTED, EWORKSPACE, Frame, f32, f64, poisoned, ratio, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODE = {f32: 0, f64: 1}
RATIOS = {}
T0 = time.time()


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    assert torch.cuda.get_device_properties(0).multi_processor_count == xu.CUS, "the shape lists are written for 256 CUs"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"[x3 gram] largest error / bound  {k[0]:24s} {k[1]:7s} {RATIOS[k]:.3f}")
    print(f"[x3 gram] module wall time {time.time() - T0:.1f} s")


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def frames(inp, off=None):
    return {k: Frame(inp[k].shape, inp[k].dtype, DEV, src=inp[k].to(DEV), off=(off or {}).get(k, 0)) for k in ("al", "g", "dm")}


def check(what, family, got, want, bound, where):
    r = ratio(got, want.reshape(got.shape), bound.reshape(got.shape))
    RATIOS[(what, family)] = max(RATIOS.get((what, family), 0.0), r)
    print(f"  {what} {family} {where}: error / bound {r:.3f}")
    assert r <= 1, f"{what} {where}: error / bound {r:.3f}"
    return r


def call(lib, F, M, C, L, out_dt, delta=None, short=0, dtype=0):
    """one call -> (rc, dOmega frame, ddelta frame or None, workspace).  delta: None (gpsa_quadform_bwd_omega_x3) or
    (ddelta0 on the CPU or None, dbeta): gpsa_quadform_bwd_omega_delta_x3"""
    dOm = Frame((L, M, M), out_dt, DEV)
    wsb = int(lib.gpsa_quadform_bwd_omega_x3_workspace(M, C, L)) - short
    assert wsb + short == xu.x3_gram_workspace(M, C, L)
    ws = poisoned(max(wsb, 1), DEV)
    if delta is None:
        dd = None
        rc = lib.gpsa_quadform_bwd_omega_x3(dtype, CODE[out_dt], F["al"].ptr(), F["g"].ptr(), M, C, L, dOm.ptr(), ws.data_ptr(),
                                            wsb, stream())
    else:
        dd0, dbeta = delta
        dd = Frame((M, L), f32, DEV, src=None if dd0 is None else dd0.to(DEV))  # dbeta = 0: NaN, never read
        rc = lib.gpsa_quadform_bwd_omega_delta_x3(CODE[out_dt], F["al"].ptr(), F["g"].ptr(), F["dm"].ptr(), M, C, L, dOm.ptr(),
                                                  dd.ptr(), float(dbeta), ws.data_ptr(), wsb, stream())
    torch.cuda.synchronize()
    return rc, dOm, dd, ws


def run_gram(lib, F, M, C, L, out_dt, delta=None):
    def once():
        rc, dOm, dd, _ = call(lib, F, M, C, L, out_dt, delta)
        assert rc == 0 and dOm.intact() and dOm.written() and (dd is None or (dd.intact() and dd.written())), (rc, M, C, L)
        assert torch.equal(dOm.view, dOm.view.transpose(1, 2)), "dOmega is not exactly symmetric"
        return (dOm.view,) + ((dd.view,) if dd is not None else ())
    a, b = once(), once()
    assert len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b)), "not repeatable bit for bit"
    return a


def refused(lib, F, M, C, L, want_rc, delta=None, short=0, dtype=0):
    rc, dOm, dd, ws = call(lib, F, M, C, L, f32, delta, short, dtype)
    assert rc == want_rc and dOm.untouched() and (dd is None or dd.untouched()) and bool((ws == 0xFF).all()), (rc, M, C, L)


def check_gram(lib, family, inp, F, M, C, L, cols=(), out_dts=(f32, f64), delta=True):
    """the plain entry in both output types; the delta entry wherever row M has a padding row behind it, with dbeta 0 (NaN in
    ddelta beforehand) and 1 - its dOmega equal to the plain entry's bit for bit; elsewhere it refuses, nothing written"""
    dev = DEV if 8.0 * L * M * M * C > 1e10 else "cpu"
    al, g, dm = (inp[k].to(dev) for k in ("al", "g", "dm"))
    bo, bd = xu.gram_bars(C, L)
    plain = {}
    for dt in out_dts:
        want, bound = cu.ref_gram(al, g, stored32=dt == f32, prod_bar=bo)
        plain[dt] = run_gram(lib, F, M, C, L, dt)[0]
        check("bwd_omega_x3 " + ("fp32" if dt == f32 else "fp64"), family, plain[dt], want, bound, (M, C, L))
        if family == "edge" and dt == out_dts[0]:
            for c in cols:
                assert cu.visible(cu.drop_col_gram(al, g, c), bound), ("dOmega", M, C, c)
    if not delta:
        return
    if not xu.x3_takes_delta(M):
        refused(lib, F, M, C, L, EUNSUPPORTED, delta=(None, 0.0))
        return
    base = torch.randn(M, L, generator=torch.Generator().manual_seed(M + L), dtype=f64).float()
    for i, (dd0, dbeta) in enumerate([(None, 0.0), (base, 1.0)]):
        dt = out_dts[i % len(out_dts)]
        dOm, dd = run_gram(lib, F, M, C, L, dt, delta=(dd0, dbeta))
        assert same_bits(dOm, plain[dt]), "the delta entry's dOmega differs from the plain entry's"
        want, bound = cu.ref_ddelta(al, dm, None if dd0 is None else dd0.to(dev), dbeta, prod_bar=bd)
        check("bwd_omega_delta_x3 ddelta", family, dd, want, bound, (M, C, L, dbeta))
        if family == "edge" and i == 0:
            for c in cols:
                assert cu.visible(cu.drop_col_ddelta(al, dm, c), bound), ("ddelta", M, C, c)


def case(lib, M, C, L, families=("edge", "graded"), out_dts=None, off=None, delta=True):
    cols = xu.gram_named_cols(M, C, L)
    for fam in families:
        inp = xu.gram_inputs(M, C, L, fam, cols)
        check_gram(lib, fam, inp, frames(inp, off), M, C, L, cols, out_dts=out_dts or ((f32, f64) if fam == "edge" else (f64, f32)),
                   delta=delta)


# ---- row classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", xu.ELBO_ROWS)
def test_row_classes(lib, M):
    """M = 1 and the edges of every row-tile class (65 / 113 / 192: whole padding tiles, their partials never read), nine
    chunks in nine splits with a last chunk of 9 or 8 columns; the delta entry at every M with a padding row - C = 265 is
    C % 4 != 0, which the fp32 delta entry refuses"""
    for C in xu.GRAM_ROW_C:
        case(lib, M, C, xu.ROW_L)


# ---- chunks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", xu.GRAM_C)
@pytest.mark.parametrize("M", [cu.M_SMALL[2], cu.M_LARGE[13]])
def test_chunks_and_lane_groups(lib, M, C):
    """one, two and three chunks of one workgroup each; C = 1, 7, 31, 33, 63, 65 end inside an 8-column lane group, 8, 32, 64
    on its edge; the delta entry at each (C in {1, 7, 31, 33, 63, 65} is C % 4 != 0, C = 1, 7 is C < 8)"""
    case(lib, M, C, 3)


@pytest.mark.parametrize("C", xu.GRAM_CHUNKS)
@pytest.mark.parametrize("MB", xu.X3_CLASSES)
def test_more_than_one_chunk_per_workgroup(lib, MB, C):
    """L = 64: 17 chunks in splits of 4, 4, 4, 5 and 19 in splits of 4, 5, 5, 5 - the stage-ahead path, both ring slots reused"""
    M, L = cu.M_LARGE[MB], xu.GRAM_CHUNKS_L
    cols = xu.gram_named_cols(M, C, L)
    for fam in ("edge", "graded"):
        inp = xu.gram_inputs(M, C, L, fam, cols)
        check_gram(lib, fam, inp, frames(inp), M, C, L, cols, out_dts=(f32, f64) if fam == "edge" else (f64,))


@pytest.mark.parametrize("M,C,L", xu.GRAM_SPLITS)
def test_splits(lib, M, C, L):
    """256 splits of one chunk, 129 splits of one and two, and more outputs than CUs with one split of nine chunks"""
    case(lib, M, C, L, families=("edge", "plain"))


# ---- what the fp32 delta entry refuses ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["al", "g", "dm"])
@pytest.mark.parametrize("M,C", [(cu.M_SMALL[2], 68), (cu.M_LARGE[13], 580), (cu.M_SMALL[7], 265)])
def test_delta_entry_with_misaligned_operands(lib, M, C, which):
    """alpha, g or dmeanT one element off 16 bytes (no vector load may assume more than 4)"""
    L = 3
    cols = xu.gram_named_cols(M, C, L)
    inp = xu.gram_inputs(M, C, L, "edge", cols)
    F = frames(inp, off={which: 1})
    assert F[which].ptr() % 16 == 4 and all(F[k].ptr() % 16 == 0 for k in F if k != which)
    check_gram(lib, "edge", inp, F, M, C, L, cols)


@pytest.mark.parametrize("C", xu.GRAM_DELTA_C)
@pytest.mark.parametrize("MB", xu.X3_CLASSES)
def test_delta_entry_at_short_column_counts(lib, MB, C):
    """C = 1, 4, 7 in every class, RL either side (M_SMALL on odd classes)"""
    M = cu.M_SMALL[MB] if MB % 2 else cu.M_LARGE[MB]
    assert lib.gpsa_quadform_bwd_omega_takes_delta(M, C) == 0
    case(lib, M, C, 3, families=("edge",))


# ---- the three-piece case ---------------------------------------------------------------------------------------------------
def test_three_pieces(lib):
    """C = 1, L = 1, g = 1, every operand 2^e (1 + c 2^-8 + c 2^-17): each of the six products, lost, moves every element of
    dOmega and ddelta by more than 4 bounds (asserted from the reference here and in tests/test_x3_shapes.py)"""
    M = 21
    inp = xu.three_piece_gram(M)
    for p, (dOm, ddd) in xu.three_piece_gram_moves(inp).items():
        assert float(dOm.min()) > 4 and float(ddd.min()) > 4, p
    check_gram(lib, "three", inp, frames(inp), M, 1, 1)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    M, C, L = 57, 300, 3
    inp = cu.make_inputs(M, C, L, "plain", out="gram")
    F = frames(inp)
    refused(lib, F, M, C, L, EUNSUPPORTED, dtype=1)  # fp64 operands
    refused(lib, F, M, C, L, EWORKSPACE, short=1)
    refused(lib, F, M, C, L, EWORKSPACE, delta=(None, 0.0), short=1)
    refused(lib, F, 64, C, L, EUNSUPPORTED, delta=(None, 0.0))  # no padding row
