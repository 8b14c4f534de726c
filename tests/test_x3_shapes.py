"""The arithmetic behind tests/test_x3_elbo_gpu.py and tests/test_x3_gram_gpu.py, without a GPU.

1. tests/x3_util.py restates the launch arithmetic of the bf16x3 pair (GPSA_ELBO_X3_SHAPES, tile width, K blocks, the
   one-workgroup-per-CU grid, item ranges, elbo_ws(true, ..), gram_nsplit(C, L, 32), gram_x3_ws) for 256 compute units.  The
   restatement is held to the library's pure queries, and every claim the GPU tests make about a shape is asserted here.
2. The split is what the derivation says it is, and the bounds are honest: the contraction emulated on the CPU - torch's
   bfloat16 split, the six products per 32-deep block in the kernels' order, fp32 accumulation - and emulated again in
   another order (blocks backwards, products largest first, rows reversed) stays inside every stage bound on both
   kernels, both operand precisions, mean and delta form.
3. The edge-weighted family's visibility condition and the three-piece case, from the reference alone.
"""
import numpy as np
import pytest
import torch

import contraction_util as cu
import fused_lik_util as fu
import x3_util as xu
from x3_util import CUS, cdiv, mb_for

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
        print(f"[x3 shapes] CPU emulation, largest error / bound  {k:24s} {WORST[k]:.3f}")


def worst(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1, (key, r)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)) if not torch.is_tensor(x) else x


def gram_shapes():
    """every (M, C, L) of tests/test_x3_gram_gpu.py"""
    s = {(M, C, 3) for M in xu.ELBO_ROWS for C in xu.GRAM_ROW_C}
    s |= {(cu.M_LARGE[MB], C, xu.GRAM_CHUNKS_L) for MB in xu.X3_CLASSES for C in xu.GRAM_CHUNKS}
    s |= {(M, C, 3) for M in (cu.M_SMALL[2], cu.M_LARGE[13]) for C in xu.GRAM_C + xu.GRAM_DELTA_C}
    s |= {(cu.M_SMALL[MB] if MB % 2 else cu.M_LARGE[MB], C, 3) for MB in xu.X3_CLASSES for C in xu.GRAM_DELTA_C}
    s |= {(cu.M_SMALL[2], 68, 3), (cu.M_LARGE[13], 580, 3), (cu.M_SMALL[7], 265, 3)}  # misaligned operands
    return s | set(xu.GRAM_SPLITS) | {(21, 1, 1), (57, 300, 3), (64, 300, 3)}


def elbo_shapes():
    s = {(M, C, xu.ROW_L) for M in xu.ELBO_ROWS + xu.DELTA_M + xu.DELTA_REFUSED for C in xu.elbo_columns(mb_for(M))}
    return s | {c[:3] for MB in xu.X3_CLASSES for c in xu.elbo_split_cases(MB)} | {(57, 300, 3), (1, 133, 1)}


# ---- 1. the restatement against the library's pure queries ----------------------------------------------------------------
def test_elbo_restatement_matches_the_library(lib):
    """NCT (hence the tile width) from the slab term of gpsa_quadform_elbo_x3_f32_workspace - slabs for num_cus() workgroups,
    one per CU, where the fp32 query lays out 2 num_cus(); the whole query at every shape of the GPU file; takes_delta"""
    for MB, (nct, w, kb) in {2: (2, 128, 1), 4: (2, 128, 2), 7: (2, 128, 4), 13: (1, 64, 7), 16: (1, 64, 8)}.items():
        M, MP = 16 * MB - 3, 16 * MB
        assert mb_for(M) == MB and xu.X3_NCT[MB] == nct and xu.x3_width(MB) == w and xu.x3_kb(MB) == kb
        pk = cdiv(kb * MB * 3 * 1024, 256) * 256
        slab = int(lib.gpsa_quadform_elbo_x3_f32_workspace(M, 1, 1)) - pk - 2 * MB * 3 * 1024
        assert slab == CUS * 2 * MP * 64 * nct * 4, (MB, slab)
    for (M, C, L) in sorted(elbo_shapes()):
        assert int(lib.gpsa_quadform_elbo_x3_f32_workspace(M, C, L)) == xu.x3_elbo_workspace(M, C, L) > 0, (M, C, L)
    assert int(lib.gpsa_quadform_elbo_x3_f32_workspace(257, 100, 3)) == xu.x3_elbo_workspace(257, 100, 3) == 0
    big = xu.PANEL_MAX_C + 1
    assert int(lib.gpsa_quadform_elbo_x3_f32_workspace(57, big, 3)) == xu.x3_elbo_workspace(57, big, 3) == 0
    assert int(lib.gpsa_quadform_elbo_x3_f32_workspace(57, big - 1, 3)) == xu.x3_elbo_workspace(57, big - 1, 3) > 0
    for M in range(1, 300):
        assert lib.gpsa_quadform_elbo_takes_delta(M) == int(xu.x3_takes_delta(M)), M


def test_gram_restatement_matches_the_library(lib):
    for (M, C, L) in sorted(gram_shapes()):
        assert int(lib.gpsa_quadform_bwd_omega_x3_workspace(M, C, L)) == xu.x3_gram_workspace(M, C, L) > 0, (M, C, L)
    assert int(lib.gpsa_quadform_bwd_omega_x3_workspace(257, 100, 3)) == xu.x3_gram_workspace(257, 100, 3) == 0
    assert int(lib.gpsa_quadform_bwd_omega_x3_workspace(17, 100, 65536)) == xu.x3_gram_workspace(17, 100, 65536) == 0


def test_kidx_is_a_permutation_of_each_k_block():
    """lane group kq of K block b holds rows 4 kq .. + 3 of row tile 2b, then of tile 2b + 1: the accumulator's own rows"""
    for b in range(8):
        ks = [xu.x3_kidx(b, kq, e) for kq in range(4) for e in range(8)]
        assert sorted(ks) == list(range(32 * b, 32 * b + 32))
        assert [xu.x3_kidx(b, 1, e) for e in range(8)] == [32 * b + k for k in (4, 5, 6, 7, 20, 21, 22, 23)]


# ---- the shapes' claims --------------------------------------------------------------------------------------------------
def test_row_list_reaches_every_class_and_its_empty_k_blocks():
    """five shapes; 65 is MB 7 with two padding tiles, so K block 3 (rows 96 ..) is all padding and block 2 half; 113 is MB 13
    with K blocks 4 .. 6 wholly empty; 192 fills twelve tiles: the half-empty last block is wholly empty"""
    assert {mb_for(M) for M in xu.ELBO_ROWS} == set(xu.X3_CLASSES)
    for MB in xu.X3_CLASSES:
        assert {M - 16 * (MB - 1) for M in xu.ELBO_ROWS if mb_for(M) == MB} >= {1, 8, 9, 15, 16}
    assert mb_for(65) == 7 and cdiv(65, 32) == 3 and xu.x3_kb(7) == 4
    assert mb_for(113) == 13 and cdiv(113, 32) == 4 and xu.x3_kb(13) == 7
    assert mb_for(192) == 13 and 192 == 32 * 6
    for M in xu.ELBO_ROWS:
        for i, C in enumerate(xu.elbo_columns(mb_for(M))):
            S, N = fu.sample_split(C)
            assert C == S * N and N % 16 != 0 and (S in (3, 7), C % 4) == ((True, 1) if i == 0 else (False, 0)), (M, C, S, N)
            assert xu.x3_plan(M, C, xu.ROW_L)[:3] == (2, 6, 6)
    assert [xu.elbo_columns(MB) for MB in (2, 13)] == [[133, 132], [69, 68]]
    # the gather: NCT = 2 is two operations with 32 surplus lanes, NCT = 1 one with 16
    assert {MB: (cdiv(48 * xu.X3_NCT[MB], 64), -48 * xu.X3_NCT[MB] % 64) for MB in (7, 13)} == {7: (2, 32), 13: (1, 16)}


def test_named_rows_sit_on_both_sides_of_the_k_block_edges():
    for M in (200, 253, 109, 57, 31):
        MB = mb_for(M)
        rows, kb = set(xu.x3_named_rows(M)), 32 * (xu.x3_kb(MB) - 1)
        want = {M - 1, 16 * (MB - 1), 16 * (MB - 1) + 7, 16 * (MB - 1) + 8, 15, 16, 31, 32, kb, kb + 3, kb + 4, kb + 16}
        assert rows == {r for r in want if r < M}, (M, rows ^ want)
    assert xu.x3_named_rows(200) == [15, 16, 31, 32, 192, 195, 196, 199] and xu.x3_named_rows(1) == [0]
    assert max(len(xu.x3_named_rows(M)) for M in range(1, 257)) == 11


def test_delta_list_covers_the_row_shuffle():
    pairs = {((M - 16) & 3, (M - 16) >> 2) for M in xu.DELTA_M if mb_for(M) == 2}
    assert pairs == {(a, b) for a in range(4) for b in range(4)} - {(0, 0)}
    for MB in (4, 7, 13, 16):
        assert {M - 16 * (MB - 1) for M in xu.DELTA_M if mb_for(M) == MB} == {1, 8, 9, 15}
    assert all(xu.x3_takes_delta(M) for M in xu.DELTA_M) and not any(xu.x3_takes_delta(M) for M in xu.DELTA_REFUSED)
    assert xu.DELTA_REFUSED == [16 * MB for MB in xu.X3_CLASSES]


def test_split_cases_are_what_they_are_called():
    for MB in xu.X3_CLASSES:
        G = CUS
        cases = {c[3]: c for c in xu.elbo_split_cases(MB)}
        assert all(xu.x3_takes_delta(c[0]) and c[1] % xu.x3_width(MB) == xu.x3_width(MB) - 3 for c in cases.values())
        nt, T, g, kinds, both = xu.x3_plan(*cases["T=G"][:3])
        assert T == g == G and cases["T=G"][2] == 4 and kinds == {(True, 0, False), (False, 0, True)}  # one item each
        nt, T, g, kinds, both = xu.x3_plan(*cases["T=G+"][:3])
        assert g == G and T - G in (1, 2) and both == 0 and not any(k[1] for k in kinds)  # ranges of one and two items
        rng = cu.item_ranges(T, G)
        assert {b - a for (a, b) in rng} == {1, 2}
        nt, T, g, kinds, both = xu.x3_plan(*cases["T=G++"][:3])
        assert g == G and T - G in (5, 7) and both >= 1 and (True, 0, True) in kinds  # ``which`` 0 and 1 in one workgroup
        nt, T, g, kinds, both = xu.x3_plan(*cases["T=2G"][:3])
        assert g == G and T == 2 * G and cases["T=2G"][2] == 2 and kinds == {(False, 1, False)}
        nt, T, g, kinds, both = xu.x3_plan(*cases["L=1"][:3])
        assert (nt, T, g) == (2, 2, 2) and kinds == {(False, 1, False)}
    for MB, C in ((7, 54653), (13, 27325)):
        M, c, L, what = xu.elbo_split_cases(MB)[-1]
        nt, T, g, kinds, both = xu.x3_plan(M, c, L)
        assert what == "T=5G+" and c == C and T == 5 * g + 1 and both >= 1 and M <= 250
        assert kinds == {(False, 2, False), (True, 1, False), (True, 1, True), (False, 1, True)}  # all four range kinds
    assert max(c[1] for MB in xu.X3_CLASSES for c in xu.elbo_split_cases(MB)) == 54653


def test_gram_lists_reach_chunks_and_splits():
    ns, bounds = xu.x3_gram_nsplit, xu.x3_gram_bounds
    assert [cdiv(C, 32) for C in xu.GRAM_C] == [1, 1, 1, 1, 1, 2, 2, 2, 3]
    assert [ns(C, 3) for C in xu.GRAM_C] == [1, 1, 1, 1, 1, 2, 2, 2, 3]  # one chunk per workgroup
    # 17 chunks in 4 splits of 4, 4, 4, 5 and 19 in 4 of 4, 5, 5, 5: several chunks per workgroup, both ring slots reused
    assert (ns(523, 64), bounds(523, 64)) == (4, [0, 4, 8, 12, 17]) and (ns(580, 64), bounds(580, 64)) == (4, [0, 4, 9, 14, 19])
    assert ns(8192, 1) == 256 and set(np.diff(bounds(8192, 1))) == {1}
    assert ns(8193, 1) == 129 and set(np.diff(bounds(8193, 1))) == {1, 2}
    assert ns(260, 257) == 1 and cdiv(260, 32) == 9
    assert [ns(C, 3) for C in xu.GRAM_ROW_C] == [9, 9]
    for (M, C, L) in gram_shapes():
        cols = xu.gram_named_cols(M, C, L)
        assert len(cols) <= 15 and all(0 <= c < C for c in cols)
        inner = bounds(C, L)[1:-1]
        assert not inner or any(b * 32 in cols and b * 32 - 1 in cols for b in inner)
    # the fp32 delta entry refuses what the x3 one takes
    assert [cu.takes_delta(21, C) for C in xu.GRAM_DELTA_C + [265]] == [False, False, False, False]


# ---- 2. the split and the bounds ----------------------------------------------------------------------------------------------
def test_the_split_is_exact():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(10 ** 6, generator=g) * 2.0 ** torch.randint(-20, 21, (10 ** 6,), generator=g)).float()
    (a1, a2, a3), left = xu.split3(x)
    assert float(left.abs().max()) == 0.0 and bool(((a1 + a2) + a3 == x).all())
    ax = x.abs().double()
    assert bool((a2.abs().double() <= 2.0 ** -8 * ax).all()) and bool((a3.abs().double() <= 2.0 ** -17 * ax).all())
    assert bool((a1.abs().double() <= (1 + 2.0 ** -8) * ax).all())
    kept = sum(p.abs().double() for p in (a1, a2, a3))
    assert bool((kept * kept <= xu.X3_ABS * ax * ax).all())  # the six kept products are among the nine of this square
    assert abs(xu.bar_x3(1, 1.0) / xu.U - 21.3) < 0.1


ELBO_SMALL = [(1, 37), (21, 70), (29, 69), (57, 70), (109, 69), (200, 70), (253, 69)]


@pytest.mark.parametrize("M,C", ELBO_SMALL)
def test_elbo_bounds_hold_for_the_emulated_contraction(M, C):
    L = 3
    for fam in ("plain", "edge", "graded"):
        for delta in ((False, True) if xu.x3_takes_delta(M) else (False,)):
            inp = xu.elbo_inputs(M, C, L, fam, delta=delta)
            for om in ("Om32", "Om64"):
                ref = xu.elbo_reference(inp, M, C, L, om, delta)
                assert float(ref["var"].min()) >= 0.25 and bool((ref["E_var"] < 0.1 * ref["var"]).all())
                for other in (False, True):
                    out = xu.elbo_np(inp, M, C, L, om, delta, other)
                    got = {k: _t(v) for k, v in out.items() if k not in ("part", "u")}
                    got["part"] = torch.tensor([out["part"]])
                    ratios, cl = xu.elbo_ratios(inp, ref, M, C, L, got)
                    for k, r in ratios.items():
                        worst(f"elbo {k}", r)
                if fam == "edge":
                    xu.elbo_visibility(inp, ref, cl, got, M, C, L, om)


GRAM_SMALL = [(1, 37, 3), (21, 70, 3), (29, 261, 2), (109, 69, 3), (200, 580, 2), (253, 33, 3)]


@pytest.mark.parametrize("M,C,L", GRAM_SMALL)
def test_gram_bounds_hold_for_the_emulated_contraction(M, C, L):
    cols = xu.gram_named_cols(M, C, L)
    bo, bd = xu.gram_bars(C, L)
    for fam in ("plain", "edge", "graded"):
        inp = xu.gram_inputs(M, C, L, fam, cols)
        al, g, dm = inp["al"], inp["g"], inp["dm"]
        w64, b64 = cu.ref_gram(al, g, False, prod_bar=bo)
        w32, b32 = cu.ref_gram(al, g, True, prod_bar=bo)
        wd, bdd = cu.ref_ddelta(al, dm, prod_bar=bd)
        for other in (False, True):
            got = _t(cu.np_gram(al, g, other, chunk=32, matmul=xu.mm(other)))
            worst("gram dOmega fp32", cu.ratio(got, w32, b32))
            worst("gram dOmega fp64", cu.ratio(got, w64, b64))
            worst("gram ddelta", cu.ratio(_t(cu.np_ddelta(al, dm, other, chunk=32, matmul=xu.mm(other))), wd, bdd))
        if fam == "edge":
            for c in cols:
                assert cu.visible(cu.drop_col_gram(al, g, c), b32), ("dOmega", M, C, c)
                assert cu.visible(cu.drop_col_ddelta(al, dm, c), bdd), ("ddelta", M, C, c)


# ---- 3. the three-piece case ---------------------------------------------------------------------------------------------------
def test_three_piece_values_split_as_built():
    x = xu.three(torch.tensor([0.0, 3.0, -2.0])).float()
    (a1, a2, a3), left = xu.split3(x)
    s = 2.0 ** torch.tensor([0.0, 3.0, -2.0])
    assert torch.equal(a1, s.float()) and torch.equal(a2.double(), s * xu.C1 * 2.0 ** -8)
    assert torch.equal(a3.double(), s * xu.C2 * 2.0 ** -17) and float(left.abs().max()) == 0.0


def test_three_piece_elbo_sees_what_the_bound_lets_it_see():
    """M = 1.  Losing a first- or second-order product moves FT and abar by thousands of bounds, losing a2 b2 by 5.7 (FT) and
    7.4 (abar) bounds at the worst column: seen under the condition (more than 4 bounds at every column).  Losing a1 b3 or
    a3 b1 moves FT by 2.95 and abar by 3.81 bounds at the worst column: outside the bound, so the kernel test fails without
    one of them unless its other roundings cancel two bounds' worth, but short of the condition's 4 - DESIGN 2h says so, and
    tests/test_contraction_x3.py's norm comparison remains their hold.  The emulation, whole, is inside the bound; with any
    one product left out it is outside it"""
    C, L = 133, 1
    inp = xu.three_piece_elbo(C, L)
    ref = xu.elbo_reference(inp, 1, C, L, "Om32", False)
    assert float((ref["v"] / ref["var"]).min()) > 0.96, "v does not dominate the variance"
    moves = xu.three_piece_elbo_moves(inp, ref, L)
    seen = {p for p, (dF, dab) in moves.items() if bool(((dF > 4) | (dab > 4)).all())}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen
    for p in ((2, 0), (0, 2)):
        dF, dab = moves[p]
        assert 2.9 < float(dF.min()) < 4 and 3.7 < float(dab.min()) < 4, (p, float(dF.min()), float(dab.min()))
    for drop in [None] + xu.PRODUCTS:
        out = fu.elbo_np(inp, 1, C, L, fu.GAUSS, matmul=lambda A, B: xu.x3_matmul(A, B, drop=drop))
        got = {k: _t(v) for k, v in out.items() if k not in ("part", "u")}
        got["part"] = torch.tensor([out["part"]])
        ratios, _ = xu.elbo_ratios(inp, ref, 1, C, L, got)
        if drop is None:
            for k, r in ratios.items():
                worst(f"three-piece elbo {k}", r)
        else:
            assert ratios["FT"] > 1 or ratios["abar"] > 1, (drop, ratios)


def test_three_piece_gram_sees_all_six_products():
    """C = 1, L = 1, one split: the bound is 6 terms and one addition deep, and every lost product moves every element of
    dOmega and of ddelta by more than 4 bounds (4.85 / 5.05 for the third-order ones)"""
    inp = xu.three_piece_gram()
    assert xu.x3_gram_nsplit(1, 1) == 1
    for p, (dOm, ddd) in xu.three_piece_gram_moves(inp).items():
        assert float(dOm.min()) > 4 and float(ddd.min()) > 4, (p, float(dOm.min()), float(ddd.min()))
    bo, bd = xu.gram_bars(1, 1)
    want, bound = cu.ref_gram(inp["al"], inp["g"], True, prod_bar=bo)
    wd, bdd = cu.ref_ddelta(inp["al"], inp["dm"], prod_bar=bd)
    for drop in [None] + xu.PRODUCTS:
        f = lambda A, B: xu.x3_matmul(A, B, drop=drop)  # noqa: E731
        r = cu.ratio(_t(cu.np_gram(inp["al"], inp["g"], chunk=32, matmul=f)), want, bound)
        rd = cu.ratio(_t(cu.np_ddelta(inp["al"], inp["dm"], chunk=32, matmul=f)), wd, bdd)
        if drop is None:
            worst("three-piece gram dOmega", r)
            worst("three-piece gram ddelta", rd)
        else:
            assert r > 1 and rd > 1, (drop, r, rd)
