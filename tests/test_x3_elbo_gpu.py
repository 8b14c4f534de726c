"""panel_elbo_x3_kernel and pack_x3_kernel (csrc/qf_x3.hip) through the C ABI alone - gpsa_quadform_elbo_x3_f32 and
gpsa_quadform_elbo_delta_x3_f32, both omega_dtype values, always asking for FT - stage against stage, element by element
against the same operation in fp64: at every row-tile class edge of the five shapes of
GPSA_ELBO_X3_SHAPES, wholly empty K blocks, a column tail of 5 and of 4 behind one full tile of 128 or 64 columns, every
position of the mean's padding row, item ranges that leave through slabs, and the three-piece case at M = 1.

FT is held to the fp64 draw from the inputs (for an fp64 Omega: from its fp32 rounding, which is what pack_x3_kernel
splits), dmeanT to the Gaussian closing applied in fp64 to the FT the device returned, g to dmeanT, abar to g, part to the
terms of FT - section 2g's stages with bar_x3 (tests/x3_util.py, derived, never measured) for the matrix-core part.  Guards
on every call: every output is a view inside a NaN-filled frame that is intact afterwards and NaN-free itself; every input
(alpha, Omega, delta or meanT, q, var_u, eps, Y, noise_u) sits in a NaN frame of its own; the workspace is exactly the queried
size, every byte 0xFF; part is NaN beforehand and part[grid ..) comes back exactly 0; every call runs twice and repeats bit
for bit; a second call with FT = NULL returns every other output bit-equal; nothing skips.  The module prints the largest
error / bound per (entry, output, family) when it ends.
"""
import time

import pytest
import torch

import x3_util as xu
from fused_lik_util import EUNSUPPORTED, EWORKSPACE, Frame, f32, f64, poisoned, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
RATIOS = {}
T0 = time.time()
INPUTS = ("al", "Om32", "Om64", "q", "var_u", "eps", "Y", "noise_u", "meanT", "delta")


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    assert torch.cuda.get_device_properties(0).multi_processor_count == xu.CUS, "the shape lists are written for 256 CUs"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"[x3 elbo] largest error / bound  {k[0]:20s} {k[1]:8s} {k[2]:7s} {RATIOS[k]:.3f}")
    print(f"[x3 elbo] module wall time {time.time() - T0:.1f} s")


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def entry_name(delta):
    return "gpsa_quadform_elbo_delta_x3_f32" if delta else "gpsa_quadform_elbo_x3_f32"


def frames(inp):
    return {k: Frame(inp[k].shape, inp[k].dtype, DEV, src=inp[k].to(DEV)) for k in INPUTS if k in inp}


def run(lib, inp, Fr, M, C, L, om, delta, with_FT=True, short=0, om_code=None):
    """one call with the guards -> dict of output views (or, refused: the return code with nothing written asserted)"""
    nparts = lib.gpsa_quadform_elbo_parts()
    o = {"g": Frame((L, C), f32, DEV), "dm": Frame((L, C), f32, DEV), "abar": Frame((M, C), f32, DEV),
         "part": Frame((nparts,), f64, DEV)}
    if with_FT:
        o["FT"] = Frame((L, C), f32, DEV)
    wsb = int(lib.gpsa_quadform_elbo_x3_f32_workspace(M, C, L)) - short
    ws = poisoned(max(wsb, 1), DEV)
    rc = getattr(lib, entry_name(delta))(
        {"Om32": 0, "Om64": 1}[om] if om_code is None else om_code, Fr["al"].ptr(), Fr[om].ptr(), M, C, L,
        Fr["delta" if delta else "meanT"].ptr(), Fr["q"].ptr(), Fr["var_u"].ptr(), Fr["eps"].ptr(), Fr["Y"].ptr(), inp["N"],
        inp["S"], Fr["noise_u"].ptr(), o["g"].ptr(), o["dm"].ptr(), o["abar"].ptr(), o["part"].ptr(),
        o["FT"].ptr() if with_FT else None, ws.data_ptr(), wsb, stream())
    torch.cuda.synchronize()
    if short or rc:
        assert all(f.untouched() for f in o.values()) and bool((ws == 0xFF).all()), (delta, rc, "something was written")
        return rc
    assert all(f.intact() and f.written() for f in o.values()), (delta, M, C, L, {k: (f.intact(), f.written()) for k, f in o.items()})
    return {k: f.view for k, f in o.items()}


def twice(once):
    a, b = once(), once()
    assert a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a), "not repeatable bit for bit"
    return a


def note(delta, what, fam, r, where):
    key = (entry_name(delta)[len("gpsa_quadform_"):], what, fam)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"  {key[0]} {what} {fam} {where}: error / bound {r:.3f}")
    return r


def check(lib, fam, M, C, L, om="Om32", delta=False, inp=None):
    inp = inp or xu.elbo_inputs(M, C, L, fam, delta=delta)
    Fr = frames(inp)
    got = twice(lambda: run(lib, inp, Fr, M, C, L, om, delta))
    cpu = {k: v.cpu() for k, v in got.items()}
    ref = xu.elbo_reference(inp, M, C, L, om, delta)
    assert float(ref["var"].min()) >= 0.25 and bool((ref["E_var"] < 0.1 * ref["var"]).all()), "the variance is too small"
    ratios, cl = xu.elbo_ratios(inp, ref, M, C, L, cpu)
    where = (M, C, L, om, "delta" if delta else "mean")
    bad = {k: r for k, r in ratios.items() if not note(delta, k, fam, r, where) <= 1}
    G = xu.x3_plan(M, C, L)[2]
    assert bool((cpu["part"][G:] == 0).all()), "part's tail is not zeroed"
    assert not bad, f"{entry_name(delta)} {where}: {bad}"
    noft = run(lib, inp, Fr, M, C, L, om, delta, with_FT=False)
    assert all(same_bits(noft[k], got[k]) for k in noft), "FT = NULL changes an output"
    if fam == "edge":
        xu.elbo_visibility(inp, ref, cl, cpu, M, C, L, om)
    return ratios


# ---- row classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", xu.ELBO_ROWS)
def test_row_classes(lib, M):
    """M = 1 and the edges of every row-tile class; 65 / 113 / 192: whole padding tiles, so wholly empty K blocks at MB 7 and
    13; one full column tile and a tail of 5 (S = 7 or 3 samples of N % 16 != 0 rows) or 4 (S = 2); both families meet both
    omega_dtype values"""
    for i, C in enumerate(xu.elbo_columns(xu.mb_for(M))):
        for k, fam in enumerate(("edge", "graded")):
            check(lib, fam, M, C, xu.ROW_L, om="Om64" if (i + k) % 2 else "Om32")


# ---- the mean in the product's padding row ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", xu.DELTA_M)
def test_delta_forms(lib, M):
    """every position lr = M - 16 (MB - 1) of the padding row at MB 2 (all (lr & 3, lr >> 2) pairs of the closing's shuffle
    but (0, 0)), 1, 8, 9, 15 in the other classes; row M of the packed image carries delta through the same six products"""
    assert lib.gpsa_quadform_elbo_takes_delta(M) == 1
    C = xu.elbo_columns(xu.mb_for(M))[0]
    for fam in ("edge", "plain"):
        check(lib, fam, M, C, xu.ROW_L, om="Om64" if fam == "plain" else "Om32", delta=True)


@pytest.mark.parametrize("M", xu.DELTA_REFUSED)
def test_delta_refused_without_a_padding_row(lib, M):
    assert lib.gpsa_quadform_elbo_takes_delta(M) == 0
    C, L = 70, 2
    inp = xu.elbo_inputs(M, C, L, "plain", delta=True)
    assert run(lib, inp, frames(inp), M, C, L, "Om32", True) == EUNSUPPORTED


# ---- item ranges ------------------------------------------------------------------------------------------------------------
def _split_params():
    return [pytest.param(MB, i, id=f"MB{MB}-{c[3]}") for MB in xu.X3_CLASSES for i, c in enumerate(xu.elbo_split_cases(MB))]


@pytest.mark.parametrize("MB,i", _split_params())
def test_item_split(lib, MB, i):
    """G = 256 for every class: T = G (every tile shared by four one-item workgroups), T = G + 1 / + 2, T = G + 5 with both
    slab halves of one workgroup in use, L = 1, T = 2G at L = 2, and T = 5G + 1 (all four range kinds) for MB 7 at 54 653
    columns and MB 13 at 27 325; the delta form and fp64 Omega on every second case"""
    M, C, L, what = xu.elbo_split_cases(MB)[i]
    check(lib, "edge" if i % 2 == 0 else "plain", M, C, L, om="Om64" if i % 2 else "Om32", delta=i % 2 == 1)


# ---- the three-piece case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("om", ["Om32", "Om64"])
def test_three_pieces(lib, om):
    """M = 1, every operand 2^e (1 + c 2^-8 + c 2^-17): the only shape at which the element bound sees a third-order product
    (tests/test_x3_shapes.py: which of the six, and by how much)"""
    C, L = 133, 1
    inp = xu.three_piece_elbo(C, L)
    ratios = check(lib, "three", 1, C, L, om=om, inp=inp)
    ref = xu.elbo_reference(inp, 1, C, L, om, False)
    moves = xu.three_piece_elbo_moves(inp, ref, L)
    assert {p for p, (dF, dab) in moves.items() if bool(((dF > 4) | (dab > 4)).all())} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(float(torch.maximum(dF, dab).min()) > 2.9 for (dF, dab) in moves.values()), "a lost product stays inside the bound"
    assert max(ratios.values()) <= 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [False, True])
def test_refuses_a_short_workspace(lib, delta):
    M, C, L = 57, 300, 3
    inp = xu.elbo_inputs(M, C, L, "plain", delta=delta)
    assert int(lib.gpsa_quadform_elbo_x3_f32_workspace(M, C, L)) == xu.x3_elbo_workspace(M, C, L)
    assert run(lib, inp, frames(inp), M, C, L, "Om32", delta, short=1) == EWORKSPACE


@pytest.mark.parametrize("delta", [False, True])
def test_refuses_another_omega_dtype(lib, delta):
    M, C, L = 57, 300, 3
    inp = xu.elbo_inputs(M, C, L, "plain", delta=delta)
    for code in (2, -1):
        assert run(lib, inp, frames(inp), M, C, L, "Om32", delta, om_code=code) == EINVAL
