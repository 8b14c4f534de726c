"""The fused ELBO kernels through the C ABI alone, stage against stage, element by element against the same operation in fp64
(DESIGN.md section 2g): panel_elbo_kernel, panel_elbo_skip_kernel, panel_elbo_pois_kernel and panel_elbo_nb_kernel
(csrc/qf_elbo_body.hpp) behind gpsa_quadform_elbo_f32, _skip_f32, _pois_f32, _nb_f32 and their four _delta_ forms, at every
row-tile class edge (five shapes of GPSA_ELBO_SHAPES, RL = 2 and 4, the headline FULLT / PAIRB instantiation and the MB 13
kernel without it), a column tail of 5 and of 4 behind one full tile, a sample boundary inside a 16-column tile, every
position of the mean's padding row, and item ranges that leave through slabs.

Every call is made with FT: FT is held to the fp64 draw from the inputs, dmeanT to the closing applied in fp64 to the FT
the device returned, g to dmeanT, abar to g, part to the terms of FT (bounds: tests/fused_lik_util.py, derived, never
measured; a bound carried through the whole chain would be too loose to see a closing error).  Guards on every call:
every output is a view inside a NaN-filled frame that is intact afterwards and NaN-free itself; every input sits in a frame
of its own (NaN; 1e30 around Y where NaN means "missing"); the workspace is exactly the queried size, every byte 0xFF; part
is NaN beforehand; every call runs twice and repeats bit for bit; nothing skips.  The module prints the largest error /
bound per (entry, output, family) when it ends.
"""
import time

import pytest
import torch

import fused_lik_util as fu
from fused_lik_util import EUNSUPPORTED, EWORKSPACE, GAUSS, LIKS, NB, POIS, SKIP, Frame, f32, f64, poisoned, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}
T0 = time.time()
SUFFIX = {GAUSS: "f32", SKIP: "skip_f32", POIS: "pois_f32", NB: "nb_f32"}


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    assert torch.cuda.get_device_properties(0).multi_processor_count == fu.CUS, "the shape lists are written for 256 CUs"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"[fused elbo] largest error / bound  {k[0]:28s} {k[1]:8s} {k[2]:6s} {RATIOS[k]:.3f}")
    print(f"[fused elbo] module wall time {time.time() - T0:.1f} s")


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def entry_name(lik, delta):
    return "gpsa_quadform_elbo_" + ("delta_" if delta else "") + SUFFIX[lik]


def frames(inp, skip):
    fr = {}
    for k, t in inp.items():
        if not torch.is_tensor(t):
            continue
        fr[k] = fu.sentinel_frame(t, DEV) if (k == "Y" and skip) else Frame(t.shape, t.dtype, DEV, src=t.to(DEV))
    return fr


def run(lib, lik, inp, Fr, M, C, L, om, delta, skip, with_FT=True, short=0):
    """one call with the guards -> dict of output views (or, short > 0: the return code with nothing written asserted)"""
    nparts = lib.gpsa_quadform_elbo_parts()
    o = {"g": Frame((L, C), f32, DEV), "dm": Frame((L, C), f32, DEV), "abar": Frame((M, C), f32, DEV),
         "part": Frame((nparts,), f64, DEV)}
    if with_FT:
        o["FT"] = Frame((L, C), f32, DEV)
    if lik == NB:
        o["u"], o["usum"] = Frame((L, C), f32, DEV), Frame((L,), f64, DEV)
    wsb = int(lib.gpsa_quadform_elbo_f32_workspace(M, C, L)) - short
    ws = poisoned(max(wsb, 1), DEV)
    ptr = lambda k: Fr[k].ptr() if k in Fr else None  # noqa: E731
    args = [{"Om32": 0, "Om64": 1}[om], ptr("al"), ptr(om), M, C, L, ptr("delta" if delta else "meanT"), ptr("q"),
            ptr("var_u"), ptr("eps"), ptr("Y"), inp["N"], inp["S"], ptr("noise_u"), o["g"].ptr(), o["dm"].ptr(),
            o["abar"].ptr(), o["part"].ptr(), o["FT"].ptr() if with_FT else None]
    if lik in (POIS, NB):
        args.append(ptr("off"))
    if lik == NB:
        args += [ptr("rho"), o["u"].ptr(), o["usum"].ptr()]
    if lik in (POIS, NB):
        args.append(int(skip))
    rc = getattr(lib, entry_name(lik, delta))(*args, ws.data_ptr(), wsb, stream())
    torch.cuda.synchronize()
    if short or rc:
        assert all(f.untouched() for f in o.values()) and bool((ws == 0xFF).all()), (lik, delta, rc, "something was written")
        return rc
    assert all(f.intact() and f.written() for f in o.values()), (lik, delta, M, C, L, {k: (f.intact(), f.written()) for k, f in o.items()})
    return {k: f.view for k, f in o.items()}


def twice(once):
    a, b = once(), once()
    assert a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a), "not repeatable bit for bit"
    return a


def note(lik, delta, what, fam, r, where):
    key = (entry_name(lik, delta)[len("gpsa_quadform_"):], what, fam)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"  {key[0]} {what} {fam} {where}: error / bound {r:.3f}")
    return r


def check(lib, lik, fam, M, C, L, om="Om32", delta=False, offs=True, miss=None, seed=0):
    skip = lik == SKIP or (lik in (POIS, NB) and bool(miss))
    inp = fu.elbo_inputs(M, C, L, lik, fam, delta=delta, offs=offs, miss=miss if lik != GAUSS else None, seed=seed)
    Fr = frames(inp, skip)
    got = twice(lambda: run(lib, lik, inp, Fr, M, C, L, om, delta, skip))
    cpu = {k: v.cpu() for k, v in got.items()}
    ref = fu.elbo_reference(inp, M, C, L, lik, om=om, delta=delta, skip=skip)
    assert float(ref["var"].min()) >= 0.25 and bool((ref["E_var"] < 0.1 * ref["var"]).all()), "the variance is too small"
    ratios, cl = fu.elbo_stage_ratios(inp, ref, M, C, L, lik, cpu)
    where = (M, C, L, om, "delta" if delta else "mean", "skip" if skip else "all")
    bad = {k: r for k, r in ratios.items() if not note(lik, delta, k, fam, r, where) <= 1}
    # the unused tail of part, and every workgroup's own entry (grid <= items: none is idle)
    G = fu.elbo_plan(M, C, L)[2]
    assert bool((cpu["part"][G:] == 0).all()), "part's tail is not zeroed"
    # missing entries: exact zeros
    if skip:
        gone = ~ref["obs"]
        assert bool(gone.any()) == bool(miss)
        for k in ("g", "dm") + (("u",) if lik == NB else ()):
            assert bool((cpu[k][gone] == 0).all()), f"{k} is not exactly 0 at a missing entry"
    assert not bad, f"{entry_name(lik, delta)} {where}: {bad}"
    # FT = NULL changes nothing
    noft = run(lib, lik, inp, Fr, M, C, L, om, delta, skip, with_FT=False)
    assert all(same_bits(noft[k], got[k]) for k in noft), "FT = NULL changes an output"
    # one kernel, a run-time flag: skip = 1 on a Y without NaN
    if lik in (POIS, NB) and not skip:
        Fr2 = dict(Fr, Y=fu.sentinel_frame(inp["Y"], DEV))
        flag = run(lib, lik, inp, Fr2, M, C, L, om, delta, True)
        assert all(same_bits(flag[k], got[k]) for k in flag), "skip = 1 without a NaN differs from skip = 0"
    # a missing entry replaced by a finite value and counted (skip = 0; the Gaussian skip kernel: its own entry, since
    # panel_elbo_kernel is another kernel) changes that element, its column of abar, and the sums - nothing else
    if skip and miss:
        Y2 = torch.where(torch.isnan(inp["Y"]), torch.full_like(inp["Y"], 3.0), inp["Y"])
        Fr2 = dict(Fr, Y=fu.sentinel_frame(Y2, DEV))
        full = run(lib, lik, dict(inp, Y=Y2), Fr2, M, C, L, om, delta, lik == SKIP)
        gone = (~ref["obs"]).to(DEV)
        assert same_bits(full["FT"], got["FT"])
        for k in ("g", "dm") + (("u",) if lik == NB else ()):
            assert torch.equal(full[k][~gone], got[k][~gone]), f"a counted entry changed {k} elsewhere"
        keep = ~gone.any(0)
        assert torch.equal(full["abar"][:, keep], got["abar"][:, keep]), "a counted entry changed another column of abar"
        assert bool((full["dm"][gone] != 0).all())
    if fam == "edge":
        fu.elbo_visibility(inp, ref, cl, cpu, M, C, L, lik, om)
    return ratios


# ---- row classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("M", fu.ELBO_ROWS)
def test_row_classes(lib, M, lik):
    """M = 1 and the edges of every row-tile class (RL = 2 up to 8 rows in the last tile, 4 above; above 192 the headline
    kernel; 65: two padding tiles; 113 / 192: MB 13 without FULLT), one full column tile and a tail of 5 or 4; C = width +
    5 is S >= 2 samples of N % 16 != 0 rows with a part of Y missing, C = width + 4 has no offsets and no NaN (the skip flag
    alone); fp64 Omega on the plain family"""
    for i, C in enumerate(fu.elbo_columns(fu.mb_for(M))):
        S, N = fu.sample_split(C)
        assert S >= 2 and N % 16 != 0
        for fam in ("edge", "plain"):
            check(lib, lik, fam, M, C, fu.ELBO_ROW_L, om="Om64" if fam == "plain" and i == 1 else "Om32", offs=i == 0,
                  miss=0.3 if i == 0 or lik == SKIP else None)


# ---- the mean in the product's padding row ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", fu.DELTA_M)
def test_delta_forms(lib, M):
    """every position lr = M - 16 (MB - 1) of the padding row at MB 2 (all (lr & 3, lr >> 2) pairs of the closing's shuffle
    but (0, 0)), 1, 8, 9, 15 in the other classes; two of the four closings per M, rotating"""
    assert lib.gpsa_quadform_elbo_takes_delta(M) == 1
    i = fu.DELTA_M.index(M)
    C = fu.elbo_columns(fu.mb_for(M))[0]
    for k, lik in enumerate((LIKS[i % 4], LIKS[(i + 2) % 4])):
        for fam in ("edge", "plain"):
            check(lib, lik, fam, M, C, fu.ELBO_ROW_L, om="Om64" if fam == "plain" else "Om32", delta=True, offs=bool(k),
                  miss=0.3 if k == 0 else None)


@pytest.mark.parametrize("M", fu.DELTA_REFUSED)
def test_delta_refused_without_a_padding_row(lib, M):
    assert lib.gpsa_quadform_elbo_takes_delta(M) == 0
    C, L = 70, 2
    for lik in LIKS:
        inp = fu.elbo_inputs(M, C, L, lik, "plain", delta=True)
        assert run(lib, lik, inp, frames(inp, False), M, C, L, "Om32", True, False) == EUNSUPPORTED


# ---- item ranges ------------------------------------------------------------------------------------------------------------
def _split_params():
    return [pytest.param(MB, i, id=f"MB{MB}-{c[3]}") for MB in fu.ELBO_CLASSES for i, c in enumerate(fu.elbo_split_cases(MB))]


@pytest.mark.parametrize("MB,i", _split_params())
def test_item_split(lib, MB, i):
    """T = G (every tile shared by four one-item workgroups), T = G + 1 / + 2 and the first T above it with both slab halves
    of one workgroup in use, L = 1, T = 2G at L = 2 (one whole tile of two outputs per workgroup; the NB closing: its
    rho is per output) and T = 5G + 1 at the headline class; otherwise the closings rotate, the delta form on every
    second case"""
    M, C, L, what = fu.elbo_split_cases(MB)[i]
    lik = GAUSS if what == "T=5G+" else NB if what == "T=2G" else LIKS[(i + fu.ELBO_CLASSES.index(MB)) % 4]
    check(lib, lik, "edge" if i % 2 == 0 else "plain", M, C, L, om="Om64" if i % 2 else "Om32", delta=i % 2 == 1,
          miss=0.3 if lik != GAUSS and i % 2 == 0 else None)


# ---- the workspace ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("lik", LIKS)
def test_refuses_a_short_workspace(lib, lik, delta):
    M, C, L = 57, 300, 3
    inp = fu.elbo_inputs(M, C, L, lik, "plain", delta=delta)
    assert int(lib.gpsa_quadform_elbo_f32_workspace(M, C, L)) == fu.elbo_workspace(M, C, L)
    assert run(lib, lik, inp, frames(inp, False), M, C, L, "Om32", delta, False, short=1) == EWORKSPACE
