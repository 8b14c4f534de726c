"""The fused LMC likelihood kernels through the C ABI alone, element by element against the same operation in fp64 (DESIGN.md
section 2g): lmc_mfma_kernel, lmc_mfma_skip_kernel, lmc_mfma_pois_kernel and lmc_mfma_nb_kernel (csrc/lmc_body.hpp) behind
gpsa_lmc_loglik_fused_f32, _skip_f32, _pois_f32 and _nb_f32 - all three instantiations of each (L <= 16, 32, 64) on both
sides of their edges, one to three chunks of outputs with the entry's own chunk length (a second chunk of one output, a
third: dF[o] + sum, the reset of the per-chunk sums of u, the per-chunk stores of the partials), spot tiles of 1 to 16 rows,
a workgroup that takes more than one tile, a single workgroup, and a zeroed tail of zpart.

No intermediate is returned, so the bounds carry the chain (tests/fused_lik_util.py: derived, never measured).  Guards on
every call: every output is a view inside a NaN-filled frame, intact afterwards and NaN-free itself; every input sits in a
frame of its own (NaN; 1e30 around Y where NaN means "missing"); the workspace is exactly the queried size, every byte 0xFF;
zpart is NaN beforehand; every call runs twice and repeats bit for bit; nothing skips.  The module prints the largest error
/ bound per (entry, output, family) when it ends.
"""
import os
import time

import pytest
import torch

import fused_lik_util as fu
from fused_lik_util import EUNSUPPORTED, GAUSS, LIKS, NB, POIS, SKIP, Frame, f32, f64, poisoned, ratio, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}
T0 = time.time()
ENTRY = {GAUSS: "gpsa_lmc_loglik_fused_f32", SKIP: "gpsa_lmc_loglik_fused_skip_f32", POIS: "gpsa_lmc_loglik_fused_pois_f32",
         NB: "gpsa_lmc_loglik_fused_nb_f32"}


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    assert torch.cuda.get_device_properties(0).multi_processor_count == fu.CUS, "the shape lists are written for 256 CUs"
    assert os.environ.get("GPSA_LMC_MFMA", "1")[:1] != "0", "these tests are about the matrix-core kernels"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"[fused lmc] largest error / bound  {k[0]:32s} {k[1]:6s} {k[2]:6s} {RATIOS[k]:.3f}")
    print(f"[fused lmc] module wall time {time.time() - T0:.1f} s")


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def frames(inp, skip):
    fr = {}
    for k, t in inp.items():
        if torch.is_tensor(t):
            fr[k] = fu.sentinel_frame(t, DEV) if (k == "Y" and skip) else Frame(t.shape, t.dtype, DEV, src=t.to(DEV))
    return fr


def run(lib, lik, inp, Fr, L, P, nparts, skip):
    """one call with the guards -> dict of output views, or the return code of a refusal (nothing written)"""
    S, N = inp["S"], inp["N"]
    o = {"dF": Frame((S, N, L), f32, DEV), "dW": Frame((L, P), f32, DEV), "zpart": Frame((nparts,), f64, DEV)}
    if lik == NB:
        o["usum"] = Frame((P,), f64, DEV)
    query = lib.gpsa_lmc_loglik_nb_workspace if lik == NB else lib.gpsa_lmc_loglik_workspace
    wsb = int(query(S * N, L, P, nparts))
    assert wsb == (fu.lmc_nb_workspace if lik == NB else fu.lmc_workspace)(S * N, L, P, nparts)
    ws = poisoned(wsb, DEV)
    ptr = lambda k: Fr[k].ptr() if k in Fr else None  # noqa: E731
    head = [ptr("F"), ptr("W"), ptr("Y")]
    dims = [S, N, L, P, o["zpart"].ptr(), nparts, o["dF"].ptr(), o["dW"].ptr()]
    if lik in (GAUSS, SKIP):
        args = head + [ptr("noise_u")] + dims
    elif lik == POIS:
        args = head + [ptr("off"), int(skip)] + dims
    else:
        args = head + [ptr("off"), ptr("rho"), int(skip)] + dims + [o["usum"].ptr()]
    rc = getattr(lib, ENTRY[lik])(*args, ws.data_ptr(), wsb, stream())
    torch.cuda.synchronize()
    if rc:
        assert all(f.untouched() for f in o.values()) and bool((ws == 0xFF).all()), (lik, rc, "something was written")
        return rc
    assert all(f.intact() and f.written() for f in o.values()), (lik, S, N, L, P, {k: (f.intact(), f.written()) for k, f in o.items()})
    return {k: f.view for k, f in o.items()}


def twice(once):
    a, b = once(), once()
    assert a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a), "not repeatable bit for bit"
    return a


def note(lik, what, fam, r, where):
    key = (ENTRY[lik][len("gpsa_"):], what, fam)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"  {key[0]} {what} {fam} {where}: error / bound {r:.3f}")
    return r


def check(lib, lik, fam, S, N, L, P, nparts, mask=None, offs=True):
    skip = lik == SKIP or (lik in (POIS, NB) and mask is not None)
    inp = fu.lmc_inputs(S, N, L, P, lik, fam, mask=mask if lik != GAUSS else None, offs=offs)
    Fr = frames(inp, skip)
    got = twice(lambda: run(lib, lik, inp, Fr, L, P, nparts, skip))
    cpu = {k: v.cpu() for k, v in got.items()}
    G = fu.lmc_grid(S, N, nparts)
    ref = fu.lmc_reference(inp, L, P, lik, skip, G)
    if ref["cl"]["eta"] is not None:
        assert float(ref["cl"]["eta"].abs().max()) <= fu.ETA_MAX, float(ref["cl"]["eta"].abs().max())
    where = (S, N, L, P, nparts, mask)
    rs = {"dF": ratio(cpu["dF"], ref["dF"], ref["b_dF"]), "dW": ratio(cpu["dW"], ref["dW"], ref["b_dW"])}
    err = abs(float(cpu["zpart"].sum()) - ref["z"])
    rs["zpart"] = err / ref["b_z"] if ref["b_z"] > 0 else (0.0 if err == 0 else float("inf"))
    if lik == NB:
        rs["usum"] = ratio(cpu["usum"], ref["usum"], ref["b_usum"])
    bad = {k: r for k, r in rs.items() if not note(lik, k, fam, r, where) <= 1}
    assert bool((cpu["zpart"][G:] == 0).all()), "zpart's tail is not zeroed"
    if skip:
        gone = ~ref["obs"][0]  # [N, P]
        assert bool(gone.any()) or (mask == "random" and gone.numel() < 8)  # (a 30 % draw over a few entries may miss)
        full_p, full_n = gone.all(0), gone.all(1)
        assert bool((cpu["dW"][:, full_p] == 0).all()), "a fully missing output has a gradient"
        assert bool((cpu["dF"][:, full_n, :] == 0).all()), "a fully missing spot has a gradient"
        if lik == NB:
            assert bool((cpu["usum"][full_p] == 0).all())
        if mask == "output":
            assert bool(full_p.any())
        if mask == "spot":
            assert bool(full_n.any())
    assert not bad, f"{ENTRY[lik]} {where}: {bad}"
    if lik in (POIS, NB) and not skip:  # one kernel, a run-time flag
        flag = run(lib, lik, inp, dict(Fr, Y=fu.sentinel_frame(inp["Y"], DEV)), L, P, nparts, True)
        assert all(same_bits(flag[k], got[k]) for k in flag), "skip = 1 without a NaN differs from skip = 0"
    if fam == "edge" and mask is None:
        fu.lmc_visibility(inp, ref, L, P, lik, skip, G)


@pytest.mark.parametrize("L", fu.LMC_L)
@pytest.mark.parametrize("lik", LIKS)
def test_instantiations_chunks_tiles(lib, lik, L):
    """per instantiation edge L: P in {1, 5, PC - 1, PC, PC + 1, 2 PC + 17} with the entry's own chunk length, the spot
    tiles and grids of fu.LMC_GRIDS and the five masks rotating over the list (Latin squares: every L meets every grid),
    the two families alternating; the count entries run every second case without a NaN (skip = 0, and skip = 1 bit-equal)"""
    iL = fu.LMC_L.index(L)
    for iP, P in enumerate(fu.lmc_outputs(L, lik == NB)):
        N, S, nparts = fu.LMC_GRIDS[(iL + iP) % len(fu.LMC_GRIDS)]
        assert S * N * P < 2e5
        masked = lik == SKIP or (lik in (POIS, NB) and (iL + iP) % 2 == 0)
        mask = fu.LMC_MASKS[(iL + 2 * iP) % len(fu.LMC_MASKS)] if masked else None
        check(lib, lik, "edge" if (iL + iP) % 2 else "plain", S, N, L, P, nparts, mask=mask, offs=iP % 3 != 2)
        check(lib, lik, "plain" if (iL + iP) % 2 else "edge", S, N, L, P, nparts, mask=None if lik != SKIP else "random",
              offs=iP % 3 != 0)


@pytest.mark.parametrize("lik", LIKS)
def test_more_tiles_than_workgroups(lib, lik):
    """nparts = 3 at N = 49: workgroup 0 takes tiles 0 and 3 (t += gridDim.x), the last tile holds one row; three chunks of
    outputs on top, so every dF[o] + sum of the second tile follows the first tile's"""
    for L in (3, 20, 40):
        P = 2 * fu.lmc_pc(L, lik == NB) + 17
        assert fu.lmc_grid(3, 49, 3) == 3 and fu.cdiv(49, 16) == 4
        for mask in ((None,) if lik == GAUSS else ("random", "corners")):
            check(lib, lik, "edge", 3, 49, L, P, 3, mask=mask if lik != GAUSS else None)


@pytest.mark.parametrize("lik", LIKS)
def test_refuses_more_than_64_latents(lib, lik):
    inp = fu.lmc_inputs(2, 20, 64, 7, lik, "plain")
    inp["F"] = torch.cat([inp["F"], inp["F"][:, :, :1]], 2).contiguous()
    inp["W"] = torch.cat([inp["W"], inp["W"][:1]], 0).contiguous()
    assert run(lib, lik, inp, frames(inp, False), 65, 7, 8, False) == EUNSUPPORTED
