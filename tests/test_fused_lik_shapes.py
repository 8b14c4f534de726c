"""The arithmetic behind tests/test_fused_elbo_gpu.py and tests/test_lmc_lik_gpu.py, without a GPU.

1. tests/fused_lik_util.py restates the launch arithmetic of the fused ELBO kernels (row-tile class, NCT, tile width,
   workgroups per CU, persistent grid, item ranges, the workspace) and of the fused LMC kernels (instantiation, outputs
   per chunk, lmc_blocks, the min(tiles, G) of the entries, both workspaces) for 256 compute units.  The restatement is
   held to what the library's pure queries reveal, and every claim the GPU tests make about a shape is asserted here.
2. The bounds are honest: a plain fp32 NumPy evaluation of each pass - the kernels' formulation in the natural order,
   and a different one (sigma(a) = 1 / (1 + exp(-a)) directly, softplus through logaddexp, reversed summation order) -
   stays inside every bound on both input families.
3. The edge-weighted family does what it is for: the visibility condition, from the reference alone.
"""
import pytest
import torch

import fused_lik_util as fu
from fused_lik_util import CUS, GAUSS, LIKS, NB, POIS, SKIP, cdiv, mb_for

WORST = {}


@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, "these sums are written for 256 CUs"
    from spatial_alignment_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[fused lik shapes] fp32 NumPy restatement, largest error / bound  {k:28s} {WORST[k]:.3f}")


def worst(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1, (key, r)


# ---- 1. the restatement against the library's pure queries ----------------------------------------------------------------
def test_elbo_restatement_matches_the_library(lib):
    """NCT (hence the tile width) from the slab term of gpsa_quadform_elbo_f32_workspace, which is laid out for 2 CUS
    workgroups whatever the shape's own grid; the whole restated query at every shape of the GPU file; takes_delta at
    every M.  Workgroups per CU do not show in a query: the table is csrc/qf_common.hpp's elbo_wgs_per_cu, stated"""
    assert lib.gpsa_quadform_elbo_parts() == 2 * CUS == fu.elbo_parts()
    for MB, (nct, w, wgs) in {2: (4, 256, 2), 4: (4, 256, 1), 7: (4, 256, 1), 13: (2, 128, 1), 16: (2, 128, 1)}.items():
        M, MP = 16 * MB - 3, 16 * MB
        assert mb_for(M) == MB and fu.elbo_nct_for(MB) == nct and fu.elbo_width(MB) == w and fu.elbo_wgs_per_cu(MB) == wgs
        slab = int(lib.gpsa_quadform_elbo_f32_workspace(M, 1, 1)) - MP * MP * 4
        assert slab == 2 * CUS * 2 * MP * 64 * nct * 4, (MB, slab)
    shapes = {(M, C, fu.ELBO_ROW_L) for M in fu.ELBO_ROWS + fu.DELTA_M for C in fu.elbo_columns(mb_for(M))}
    shapes |= {c[:3] for MB in fu.ELBO_CLASSES for c in fu.elbo_split_cases(MB)} | {(57, 300, 3)}
    for (M, C, L) in sorted(shapes):
        assert int(lib.gpsa_quadform_elbo_f32_workspace(M, C, L)) == fu.elbo_workspace(M, C, L) > 0, (M, C, L)
    assert int(lib.gpsa_quadform_elbo_f32_workspace(257, 100, 3)) == fu.elbo_workspace(257, 100, 3) == 0
    for M in range(1, 300):
        assert lib.gpsa_quadform_elbo_takes_delta(M) == int(fu.elbo_takes_delta(M)), M


def test_lmc_restatement_matches_the_library(lib):
    """both workspace queries at every shape of the GPU file; they give G = lmc_blocks"""
    n = 0
    for lik in LIKS:
        for iL, L in enumerate(fu.LMC_L + [3, 20, 40]):
            for P in fu.lmc_outputs(L, lik == NB):
                for (N, S, nparts) in fu.LMC_GRIDS:
                    C = S * N
                    old = int(lib.gpsa_lmc_loglik_workspace(C, L, P, nparts))
                    assert old == fu.lmc_workspace(C, L, P, nparts) and (old - 256) // (L * P * 4) == fu.lmc_blocks(C, nparts)
                    assert int(lib.gpsa_lmc_loglik_nb_workspace(C, L, P, nparts)) == fu.lmc_nb_workspace(C, L, P, nparts)
                    n += 1
    assert n and int(lib.gpsa_lmc_loglik_workspace(0, 3, 3, 3)) == 0 == fu.lmc_workspace(0, 3, 3, 3)
    assert [fu.lmc_pc(L) for L in (16, 32, 64)] == [512, 256, 128] and [fu.lmc_pc(L, True) for L in (16, 32, 64)] == [256, 128, 64]
    assert fu.lmc_inst(65) is None and fu.lmc_inst(17) == (2, 4) and fu.lmc_inst(33, True) == (4, 1)


# ---- the shapes' claims --------------------------------------------------------------------------------------------------
def test_row_list_reaches_every_elbo_kernel():
    """five shapes x RL 2 / 4, the two headline instantiations on top; 65 is MB 7 with two padding tiles; 113 and 192 are MB
    13 without FULLT, with five whole padding tiles and with one (192 fills twelve tiles exactly).  Below 16 (MB - 1) + 1
    rows the last tile holds none, which last_tile_rl counts as "at most 8": MB 13 without FULLT is always RL = 2, and
    panel_elbo_*_kernel<13, 2, 4> (plain) is an instantiation no M reaches"""
    seen = {fu.elbo_kernel(M) for M in fu.ELBO_ROWS}
    assert seen == {fu.elbo_kernel(M) for M in range(1, 257)}  # every kernel that any M launches
    want = {(MB, fu.ELBO_NCT[MB], RL, False) for MB in (2, 4, 7, 16) for RL in (2, 4)}
    want |= {(13, 2, 2, False), (13, 2, 2, True), (13, 2, 4, True)}
    assert seen == want, seen ^ want
    assert fu.elbo_kernel(65) == (7, 4, 2, False) and 7 - cdiv(65, 16) == 2
    assert fu.elbo_kernel(113) == (13, 2, 2, False) and 13 - cdiv(113, 16) == 5
    assert fu.elbo_kernel(192) == (13, 2, 2, False) and 13 - cdiv(192, 16) == 1
    assert fu.elbo_kernel(193) == (13, 2, 2, True) and fu.elbo_kernel(201) == (13, 2, 4, True)
    # the gather table: NCT = 2 is two operations with 32 surplus lanes, NCT = 4 three full ones - both in the class list
    assert {fu.elbo_ngather(MB) for MB in fu.ELBO_CLASSES} == {(2, 32), (3, 0)}
    assert fu.elbo_ngather(13) == (2, 32) and fu.elbo_ngather(2) == (3, 0)
    for M in fu.ELBO_ROWS:
        for C in fu.elbo_columns(mb_for(M)):
            S, N = fu.sample_split(C)
            assert S >= 2 and N % 16 != 0 and C == S * N  # a sample boundary inside a 16-column tile
            assert fu.elbo_plan(M, C, fu.ELBO_ROW_L)[:3] == (2, 6, 6)
    assert [C % 4 for C in fu.elbo_columns(2)] == [1, 0]


def test_delta_list_covers_the_row_shuffle():
    """row M = 16 (MB - 1) + lr of the product sits in lane j + 16 (lr >> 2), component lr & 3: all pairs but (0, 0) at MB 2"""
    pairs = {((M - 16) & 3, (M - 16) >> 2) for M in fu.DELTA_M if mb_for(M) == 2}
    assert pairs == {(a, b) for a in range(4) for b in range(4)} - {(0, 0)}
    for MB in (4, 7, 13, 16):
        assert {M - 16 * (MB - 1) for M in fu.DELTA_M if mb_for(M) == MB} == {1, 8, 9, 15}
    assert all(fu.elbo_takes_delta(M) for M in fu.DELTA_M) and not any(fu.elbo_takes_delta(M) for M in fu.DELTA_REFUSED)
    assert not fu.elbo_takes_delta(65) and not fu.elbo_takes_delta(113)  # row M lies before the last row tile


def test_split_cases_are_what_they_are_called():
    for MB in fu.ELBO_CLASSES:
        G = fu.elbo_full_grid(MB)
        cases = {c[3]: c for c in fu.elbo_split_cases(MB)}
        assert fu.last_tile_rl(cases["T=G"][0], MB) == 2 and fu.last_tile_rl(cases["T=G+"][0], MB) == 4
        assert all(fu.elbo_takes_delta(c[0]) for c in cases.values())
        nt, T, g, kinds, both = fu.elbo_plan(*cases["T=G"][:3])
        assert T == g == G and cases["T=G"][2] == 4 and kinds == {(True, 0, False), (False, 0, True)}  # one item each
        nt, T, g, kinds, both = fu.elbo_plan(*cases["T=G+"][:3])
        assert g == G and T - G in (1, 2) and cases["T=G+"][2] == 3 and both == 0  # no two-item range crosses a tile edge
        assert not any(k[1] for k in kinds)  # no workgroup covers a tile: every tile leaves through slabs
        nt, T, g, kinds, both = fu.elbo_plan(*cases["T=G++"][:3])
        assert g == G and T - G <= 7 and both >= 1 and (True, 0, True) in kinds  # ``which`` 0 and 1 in one workgroup
        nt, T, g, kinds, both = fu.elbo_plan(*cases["T=2G"][:3])
        assert g == G and T == 2 * G and cases["T=2G"][2] == 2 and kinds == {(False, 1, False)}  # one whole tile each
        nt, T, g, kinds, both = fu.elbo_plan(*cases["L=1"][:3])
        assert (nt, T, g) == (2, 2, 2) and kinds == {(False, 1, False)}
    M, C, L, _ = fu.elbo_split_cases(13)[-1]
    nt, T, g, kinds, both = fu.elbo_plan(M, C, L)
    assert fu.elbo_kernel(M)[3] and T == 5 * g + 1 and both >= 1
    assert kinds == {(False, 2, False), (True, 1, False), (True, 1, True), (False, 1, True)}  # all four range kinds


def test_lmc_lists_reach_chunks_tiles_and_grids():
    for nb in (False, True):
        for L in fu.LMC_L:
            pc = fu.lmc_pc(L, nb)
            assert [cdiv(P, pc) for P in fu.lmc_outputs(L, nb)] == [1, 1, 1, 1, 2, 3]
            assert all(S * N * P < 2e5 for P in fu.lmc_outputs(L, nb) for (N, S, _) in fu.LMC_GRIDS)
        assert {fu.lmc_inst(L, nb) for L in fu.LMC_L} == {fu.lmc_inst(L, nb) for L in (16, 32, 64)}
        for L in (3, 20, 40):  # test_more_tiles_than_workgroups
            assert cdiv(2 * fu.lmc_pc(L, nb) + 17, fu.lmc_pc(L, nb)) == 3
    assert [fu.lmc_inst(L) for L in fu.LMC_L] == [(1, 8), (1, 8), (2, 4), (2, 4), (4, 2), (4, 2)]
    grids = {(N, S, nparts): fu.lmc_grid(S, N, nparts) for (N, S, nparts) in fu.LMC_GRIDS}
    assert grids[(49, 3, 3)] == 3 and cdiv(49, 16) == 4 and 49 - 48 == 1  # workgroup 0: tiles 0 and 3; the last holds one row
    assert grids[(49, 1, 1)] == 1 and grids[(1, 1, 1)] == 1 and grids[(15, 3, 1)] == 1  # one workgroup, zpart of one element
    assert grids[(17, 3, 2 * CUS)] == 2 and grids[(16, 1, 2 * CUS)] == 1  # zpart's tail is zeroed
    assert {N for (N, _, _) in fu.LMC_GRIDS} == {1, 15, 16, 17, 49} and {S for (_, S, _) in fu.LMC_GRIDS} == {1, 3}
    n = len(fu.LMC_GRIDS)
    assert all({(iL + iP) % n for iP in range(6)} == set(range(n)) for iL in range(6))  # every L meets every grid
    # the (0, PC) corner exists only with a second chunk: the rotation puts "corners" on P = PC + 1 or 2 PC + 17
    hits = {(iL, iP) for iL in range(6) for iP in (4, 5) if fu.LMC_MASKS[(iL + 2 * iP) % 5] == "corners"}
    assert hits


# ---- 2. the bounds against an honest fp32 evaluation -------------------------------------------------------------------------
ELBO_SMALL = [(1, 37), (21, 70), (29, 69), (57, 70), (109, 69), (200, 70), (253, 69)]


def _t(x):
    return torch.from_numpy(x.copy()) if not torch.is_tensor(x) else x


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("M,C", ELBO_SMALL)
def test_elbo_bounds_hold_for_plain_fp32(M, C, lik):
    """every stage of the pass in fp32 NumPy, held to the stage before it exactly as the GPU test holds the device"""
    L = 3
    for fam in ("plain", "edge"):
        for delta in ((False, True) if fu.elbo_takes_delta(M) else (False,)):
            for om in ("Om32", "Om64"):
                skip = lik == SKIP or (lik in (POIS, NB) and om == "Om32")
                inp = fu.elbo_inputs(M, C, L, lik, fam, delta=delta, offs=om == "Om32", miss=0.3 if skip else None)
                ref = fu.elbo_reference(inp, M, C, L, lik, om=om, delta=delta, skip=skip)
                assert float(ref["var"].min()) >= 0.25 and bool((ref["E_var"] < 0.1 * ref["var"]).all())
                for other in (False, True):
                    out = fu.elbo_np(inp, M, C, L, lik, om=om, delta=delta, skip=skip, other=other)
                    got = {k: _t(v) for k, v in out.items() if k not in ("part", "u")}
                    got["part"] = torch.tensor([out["part"]])
                    if lik == NB:
                        got["u"] = _t(out["u"])
                        got["usum"] = got["u"].double().sum(1)
                    ratios, cl = fu.elbo_stage_ratios(inp, ref, M, C, L, lik, got)
                    for k, r in ratios.items():
                        worst(f"elbo {lik} {k}", r)
                if fam == "edge":
                    fu.elbo_visibility(inp, ref, cl, got, M, C, L, lik, om)


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("L", fu.LMC_L)
def test_lmc_bounds_hold_for_plain_fp32(L, lik):
    iL = fu.LMC_L.index(L)
    pc = fu.lmc_pc(L, lik == NB)
    for iP, P in enumerate((5, pc + 1)):
        N, S, nparts = fu.LMC_GRIDS[(iL + 4 * iP) % len(fu.LMC_GRIDS)]
        for fam in ("plain", "edge"):
            for mask in ((None,) if lik == GAUSS else (None, "random")):
                skip = lik == SKIP or mask is not None
                inp = fu.lmc_inputs(S, N, L, P, lik, fam, mask="random" if lik == SKIP else mask, offs=iP == 0)
                G = fu.lmc_grid(S, N, nparts)
                ref = fu.lmc_reference(inp, L, P, lik, skip, G)
                if ref["cl"]["eta"] is not None:
                    assert float(ref["cl"]["eta"].abs().max()) <= fu.ETA_MAX
                for other in (False, True):
                    out = fu.lmc_np(inp, L, P, lik, skip, other=other)
                    worst(f"lmc {lik} dF", fu.ratio(_t(out["dF"]), ref["dF"], ref["b_dF"]))
                    worst(f"lmc {lik} dW", fu.ratio(_t(out["dW"]), ref["dW"], ref["b_dW"]))
                    worst(f"lmc {lik} zpart", abs(out["z"] - ref["z"]) / ref["b_z"] if ref["b_z"] else 0.0)
                    if lik == NB:
                        worst(f"lmc {lik} usum", fu.ratio(_t(out["usum"]), ref["usum"], ref["b_usum"]))
                if fam == "edge" and mask is None and lik != SKIP:
                    fu.lmc_visibility(inp, ref, L, P, lik, skip, G)


def test_edge_family_eta_stays_in_range_at_the_gpu_shapes():
    """|eta|, |a| <= 20 (asserted again on the device's FT): the largest class and the longest panel, from the reference"""
    for (M, C, L, lik) in [(253, 133, 3, POIS), (205, 11005, 3, NB), (31, 261, 3, NB)]:
        for delta in (False, True):
            inp = fu.elbo_inputs(M, C, L, lik, "edge", delta=delta)
            ref = fu.elbo_reference(inp, M, C, L, lik, delta=delta)
            cl = fu.elbo_closing(inp, ref, lik, ref["F"])
            assert float(cl["eta"].abs().max()) + float(ref["E_F"].max()) <= fu.ETA_MAX, (M, C, lik)


@pytest.mark.parametrize("lik", LIKS)
def test_lmc_edge_family_is_visible_and_in_range_at_every_gpu_shape(lik):
    """the LMC shapes are all small: the visibility condition and |eta| <= 20 at every unmasked edge-weighted case of the
    GPU file (P = 1 with one spot is the shape at which a named entry near zero hid a latent row before the floor)"""
    skip = lik == SKIP
    cases = [(fu.LMC_GRIDS[(iL + iP) % len(fu.LMC_GRIDS)], L, P) for iL, L in enumerate(fu.LMC_L)
             for iP, P in enumerate(fu.lmc_outputs(L, lik == NB))]
    cases += [((49, 3, 3), L, 2 * fu.lmc_pc(L, lik == NB) + 17) for L in (3, 20, 40)]
    for (N, S, nparts), L, P in cases:
        for offs in (True, False):
            inp = fu.lmc_inputs(S, N, L, P, lik, "edge", offs=offs)
            G = fu.lmc_grid(S, N, nparts)
            ref = fu.lmc_reference(inp, L, P, lik, skip, G)
            if ref["cl"]["eta"] is not None:
                assert float(ref["cl"]["eta"].abs().max()) <= fu.ETA_MAX, (L, P, N, S)
            fu.lmc_visibility(inp, ref, L, P, lik, skip, G)
