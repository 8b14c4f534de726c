"""The arithmetic behind tests/test_contraction_gpu.py, without a GPU.

1. tests/contraction_util.py restates the launchers of the register-resident fp32 contraction kernels (row-tile class,
   tile width, persistent grid, item ranges, TileOrder, gram_nl, gram_nsplit, the workspace layouts) for 256 compute
   units.  The restatement is held to what the library's pure queries reveal, and every claim the GPU tests make about a
   shape ("this one has a partial first tile, whole tiles and a partial last tile") is asserted from it here.
2. The bounds are honest: a plain fp32 NumPy evaluation of each operation, in the natural order and in a deliberately
   different one (reversed l, reversed rows, 64-column chunks last first), stays inside every bound on every input family.
3. The edge-weighted family does what it is for: removing the terms of any one named index from the reference changes at
   least half of the elements it feeds by more than 4 x their bound.
"""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import contraction_util as cu
from contraction_util import CUS, EWORKSPACE, GR_KC, cdiv, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
        print(f"[contraction shapes] fp32 NumPy restatement, largest error / bound  {k:24s} {WORST[k]:.3f}")


def _all_gpu_shapes():
    """every (M, C, L) the GPU file hands to a gpsa_quadform_workspace-sized entry"""
    s = set()
    for M in cu.ROWS_512:
        s |= {(M, C, cu.ROW_L) for C in cu.row_class_columns(cu.mb_for(M))}
    for MB in cu.MB_CLASSES:
        s |= {c[:3] for c in cu.split_cases(MB)}
    s |= set(cu.SOFF_SHAPES) | set(cu.GRAM_SPLITS)
    for MB in (2, 4, 7, 13, 16):
        s |= {(cu.M_LARGE[MB], C, cu.GRAM_CHUNKS_L) for C in cu.GRAM_CHUNKS_C}
        s |= {(cu.M_LARGE[MB], cu.GRAM_NL_C, L) for L in cu.GRAM_NL_L}
    s |= {(M, C, 3) for M in (cu.M_SMALL[2], cu.M_LARGE[13]) for C in cu.GRAM_NL_EDGE + cu.GRAM_TAIL_C}
    return sorted(s)


# ---- 1. the restatement against the library's pure queries ---------------------------------------------------------------
def test_tile_width_grid_and_workspaces_match_the_library(lib):
    """width from gpsa_quadform_keep_f32_bytes (one column is one tile), G from the slab term of
    gpsa_quadform_workspace at C = 1 (where the accumulate layout is the largest), 2 CUs of ELBO parts, and the whole
    restated query at every shape of the GPU file and of tests/golden/quadform_workspaces.json"""
    assert lib.gpsa_quadform_elbo_parts() == 2 * CUS
    table = {2: (256, 512), 4: (256, 512), 7: (256, 256), 13: (192, 256), 16: (128, 256), 24: (64, 256), 32: (64, 256)}
    for MB, (w, G) in table.items():
        M, MP = 16 * MB - 3, 16 * MB
        assert cu.mb_for(M) == MB and cu.mb_for(16 * MB) == MB and cu.mb_for(16 * MB + 1) != MB
        assert cu.width(MB) == w and cu.full_grid(MB) == G
        if MB <= 16:
            assert int(lib.gpsa_quadform_keep_f32_bytes(M, 1, 1)) == w * MP * 4
            assert int(lib.gpsa_quadform_keep_f32_bytes(M, w + 1, 3)) == 3 * 2 * w * MP * 4 == cu.keep_bytes(M, w + 1, 3)
            assert int(lib.gpsa_quadform_keep_f32_workspace(M, 3)) == cu.keep_workspace(M, 3)
        slab = int(lib.gpsa_quadform_workspace(0, M, 1, 1)) - 256 - MP * MP * 4
        assert slab == G * 2 * MP * w * 4, (MB, slab)
    for (M, C, L) in _all_gpu_shapes():
        assert int(lib.gpsa_quadform_workspace(0, M, C, L)) == cu.quadform_workspace_f32(M, C, L), (M, C, L)
    with open(os.path.join(ROOT, "tests", "golden", "quadform_workspaces.json")) as f:
        rec = json.load(f)
    assert rec["cus"] == CUS
    ax = rec["axes"]
    for (M, C, L), want in zip(itertools.product(ax["M"], ax["C"], ax["L"]), rec["values"]["gpsa_quadform_workspace/f32"]):
        if M <= 512:
            assert cu.quadform_workspace_f32(M, C, L) == want, (M, C, L)
    for (M, C), want in zip(itertools.product(ax["M"], ax["C"]), rec["values"]["gpsa_quadform_bwd_omega_takes_delta"]):
        assert int(cu.takes_delta(M, C)) == want == lib.gpsa_quadform_bwd_omega_takes_delta(M, C), (M, C)


def test_gram_split_and_outputs_per_workgroup_match_the_library(lib):
    """gram_nsplit is the function behind gpsa_quadform_bwd_omega_x3_workspace too (chunks of 32 there): the restatement
    must reproduce that query.  gram_nl shows in gpsa_quadform_workspace where the Gram layout is the largest term:
    MB = 13, L = 4 on the two sides of C = 8192 - with two outputs per workgroup the partial sums double and pass the
    accumulate layout, with one they stay below it"""
    for M, C, L in [(17, 260, 3), (200, 12500, 50), (100, 100000, 2), (250, 8252, 16), (57, 16385, 1), (17, 260, 257)]:
        MB = cu.mb_for(M)
        want = cdiv(C, 32) * MB * 3 * 1024 + L * cu.gram_nsplit(C, L, 32) * (16 * MB) ** 2 * 4
        assert int(lib.gpsa_quadform_bwd_omega_x3_workspace(M, C, L)) == want, (M, C, L)
    M, L, MB = 200, 4, 13
    lo, hi = cu.GRAM_NL_EDGE
    assert (cu.gram_nl(MB, L, lo), cu.gram_nl(MB, L, hi)) == (1, 2)
    assert int(lib.gpsa_quadform_workspace(0, M, hi, L)) == cu.gram_ws(MB, hi, L) + 256 > cu.accum_ws(MB, L) + 256
    assert int(lib.gpsa_quadform_workspace(0, M, lo, L)) == cu.accum_ws(MB, L) + 256 > cu.gram_ws(MB, lo, L) + 256
    one_output = cdiv(L * hi, 64) * 64 * 4 + L * cu.gram_nsplit(hi, L) * 208 * 208 * 4  # what NL = 1 would ask for
    assert one_output < cu.accum_ws(MB, L)
    for MB in (2, 4, 7, 13):
        assert cu.gram_nl(MB, 2, 8192) == 2 and cu.gram_nl(MB, 1, 10 ** 6) == 1
    assert cu.gram_nl(16, 50, 10 ** 6) == 1


def test_panel_mm_refuses_a_workspace_without_ring_slack(lib):
    """panel_mfma_kernel<STORE> stages two chunks ahead and its last two requests lie behind the packed operand (never
    multiplied); gpsa_panel_mm used to accept the packed operand's size alone.  The refusal returns before any launch"""
    for MB in (2, 4, 7, 13, 16):
        for M in (16 * (MB - 1) + 1, 16 * MB):
            need = cu.panel_mm_workspace(M)
            assert need == 4 * 16 * MB * (16 * MB + 64)
            for short in (need - 1, (16 * MB) ** 2 * 4):
                assert lib.gpsa_panel_mm(0, 0, 0, 8, 8, M, 100, 8, 0, 8, short, None) == EWORKSPACE, (M, short)


# ---- the shapes' claims ------------------------------------------------------------------------------------------------
def test_row_class_lists():
    assert cu.TILE_EDGE_M == [17, 24, 25, 31, 32, 49, 56, 57, 63, 64, 97, 104, 105, 111, 112, 193, 200, 201, 207, 208,
                              241, 248, 249, 255, 256]
    for M in cu.ROWS_512:
        MB = cu.mb_for(M)
        assert MB and (M in cu.TILE_EDGE_M_BIG or M == 1 or M > 16 * (MB - 1))
        cols = cu.row_class_columns(MB)
        assert cols[0] % 4 != 0 and cols[1] % 4 == 0 and all(cdiv(c, cu.width(MB)) == 2 for c in cols)
    for MB in (2, 4, 7, 13, 16):
        rl = [cu.last_tile_rl(16 * (MB - 1) + d, MB) for d in (1, 8, 9, 15, 16)]
        pad = [cu.has_padding_row(16 * (MB - 1) + d, MB) for d in (1, 8, 9, 15, 16)]
        assert rl == [2, 2, 4, 4, 4] and pad == [True, True, True, True, False]
    assert max(cu.ROWS_384) == 384 and cu.mb_for(384) == 24 and cu.mb_for(385) == 32 and cu.mb_for(513) == 0
    for MB in cu.MB_CLASSES:
        s, l_ = cu.M_SMALL[MB], cu.M_LARGE[MB]
        assert cu.mb_for(s) == cu.mb_for(l_) == MB and cu.has_padding_row(s, MB) and cu.has_padding_row(l_, MB)
        assert cu.last_tile_rl(s, MB) == 2 and cu.last_tile_rl(l_, MB) == 4
    # kept_wsum_kernel's groups of four row tiles: MB 2 leaves two of four masked, 7 is 4 + 3, 13 is 4 + 4 + 4 + 1
    assert [(cdiv(MB, 4), MB - 4 * (cdiv(MB, 4) - 1)) for MB in (2, 4, 7, 13, 16)] == [(1, 2), (1, 4), (2, 3), (4, 1), (4, 4)]
    assert {L % 2 for L in cu.KEPT_L} == {0, 1} and {L % 4 for L in cu.KEPT_L} == {0, 1, 2, 3} and max(cu.KEPT_L) > 4


def test_item_split_shapes():
    """T = G: one item per workgroup; just above: ranges of 1 and 2 items and every tile shared (it leaves through the
    slabs); T = 5 G + 1 or + 2: the four kinds of range; L = 1: two tiles, none shared"""
    big_c = {2: 218621, 4: 218621, 7: 109309, 13: 81981, 16: 54653, 24: 27325, 32: 27325}
    for MB in cu.MB_CLASSES:
        G = cu.full_grid(MB)
        cases = cu.split_cases(MB)
        assert [c[3] for c in cases] == ["T=G", "T=G+", "T=G", "T=G+", "T=5G+", "L=1"]
        for (M, C, L, what) in cases:
            assert cu.mb_for(M) == MB and C % 4 != 0
            ntiles, T, Gr, kinds, share = cu.split_plan(MB, C, L)
            sizes = {b - a for (a, b) in cu.item_ranges(T, Gr)}
            if what == "T=G":
                assert T == G == Gr and sizes == {1} and L == 4 and share == 4
            elif what == "T=G+":
                assert G < T <= G + 2 and Gr == G and sizes == {1, 2} and L == 3 and share >= 3
                assert all(w == 0 for (_, w, _) in kinds) or kinds <= {(True, 0, False), (True, 0, True), (False, 1, False),
                                                                      (False, 0, True)}
                # no workgroup owns a whole tile alone here: 3 items per tile against ranges of at most 2
            elif what == "T=5G+":
                assert 5 * G < T <= 5 * G + 2 and C == big_c[MB] and sizes == {5, 6}
                assert {(True, 1, False), (True, 1, True), (False, 1, True), (False, 2, False)} <= kinds, (MB, kinds)
            else:
                assert L == 1 and ntiles == 2 == T == Gr and share == 1 and kinds == {(False, 1, False)}
    for (M, C, L) in cu.SOFF_SHAPES:
        MB = cu.mb_for(M)
        ntiles, T, Gr, kinds, share = cu.split_plan(MB, C, L)
        assert ntiles == 1 and Gr == 512 and share == 512 and MB <= 4  # panel_slab_reduce_kernel's soff[512] exactly full
    assert cu.split_plan(2, 200, 512)[1] == 512 and cu.split_plan(4, 200, 513)[1] == 513
    for MB in (2, 4, 7, 13, 16):
        assert [cdiv(C, cu.width(MB)) for C in cu.STORE_C(MB)] == [1, 1, 1, 2]


def test_tile_order_visits_whole_tiles_then_last_then_first():
    assert cu.tile_order(2, 13, 3) == [(1, 0, 2), (2, 0, 2), (3, 0, 2), (4, 0, 0), (0, 2, 2)]
    assert cu.tile_order(3, 9, 3) == [(1, 0, 2), (2, 0, 2)] and cu.tile_order(4, 5, 3) == [(1, 1, 1)]
    assert cu.tile_order(1, 6, 3) == [(1, 0, 2), (0, 1, 2)] and cu.tile_order(0, 5, 3) == [(0, 0, 2), (1, 0, 1)]
    for T, G, L in [(2562, 512, 3), (1281, 256, 3), (513, 512, 513), (258, 256, 3)]:
        seen = sorted((t, l) for (a, b) in cu.item_ranges(T, G) for (t, lo, hi) in (cu.tile_order(a, b, L) if b > a else [])
                      for l in range(lo, hi + 1))
        assert seen == [(t, l) for t in range(T // L) for l in range(L)]  # every item once


def test_gram_shapes():
    for MB in (2, 4, 7, 13, 16):
        M = cu.M_LARGE[MB]
        _, nl, ns, b = cu.gram_plan(M, 523, cu.GRAM_CHUNKS_L)
        assert (nl, ns, b) == (1, 3, [0, 3, 6, 9])
        _, nl, ns, b = cu.gram_plan(M, 580, cu.GRAM_CHUNKS_L)
        assert (nl, ns, [y - x for x, y in zip(b, b[1:])]) == (1, 4, [2, 3, 2, 3])
        for L in cu.GRAM_NL_L:
            _, nl, ns, b = cu.gram_plan(M, cu.GRAM_NL_C, L)
            assert cdiv(cu.GRAM_NL_C, GR_KC) == 129
            assert (nl, ns) == ((2, 26) if MB <= 13 else (1, 9 if L == 16 else 9)) or (MB == 16 and nl == 1), (MB, L, nl, ns)
            if MB <= 13:
                assert {y - x for x, y in zip(b, b[1:])} == {4, 5} and cdiv(L, nl) == 8
        # L = 15 with two outputs per workgroup: the last workgroup's second output is the clamped surplus
        assert cdiv(15, 2) * 2 == 16
        # the 260-column row-class shapes never sweep more than one chunk per workgroup (why the 523 / 580 shapes exist)
        _, _, ns, b = cu.gram_plan(M, 260, 3)
        assert ns == 5 and all(y - x == 1 for x, y in zip(b, b[1:]))
    assert cu.gram_plan(17, 16384, 1)[1:3] == (1, 256) and cu.gram_plan(17, 16385, 1)[1:3] == (1, 129)
    assert cu.gram_plan(17, 260, 257)[1:3] == (1, 1) and cu.gram_plan(17, 260, 257)[3] == [0, 5]
    assert [cu.gram_aligned(C) for C in cu.GRAM_TAIL_C] == [False, False, False, True, True, True, True, True]
    assert cu.gram_aligned(64, alpha_off=1) is False
    for (M, C, L) in cu.GRAM_SPLITS + [(cu.M_LARGE[13], cu.GRAM_NL_C, 16), (cu.M_LARGE[2], 580, 64)]:
        cols = cu.named_cols_gram(M, C, L)
        assert len(cols) <= 13 and C - 1 in cols and all(0 <= c < C for c in cols)


# ---- 2. an honest fp32 evaluation stays inside every bound ---------------------------------------------------------------
SMALL = [(17, 261, 3), (57, 260, 3), (100, 261, 3), (200, 197, 3), (250, 133, 3), (380, 69, 3), (20, 200, 40)]


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def _r(got, want, bound):
    return cu.ratio(torch.from_numpy(np.ascontiguousarray(got)), want, bound)


@pytest.mark.parametrize("family", ["plain", "edge", "graded"])
@pytest.mark.parametrize("M,C,L", SMALL)
def test_fp32_numpy_meets_the_row_contraction_bounds(family, M, C, L):
    for other in (False, True):
        inp = cu.make_inputs(M, C, L, family, out="cols" if family == "graded" else "rows")
        for om in ("Om32", "Om64"):
            want, bound = cu.ref_v(inp["al"], inp[om])
            assert _note("v", _r(cu.np_v(inp["al"], inp[om], other), want, bound)) <= 1
        inp = cu.make_inputs(M, C, L, family, out="rows")
        want, bound = cu.ref_dalpha(inp["al"], inp["Om32"], inp["g"])
        assert _note("dalpha", _r(cu.np_dalpha(inp["al"], inp["Om32"], inp["g"], other=other), want, bound)) <= 1
        want, bound = cu.ref_dalpha(inp["al"], inp["Om64"], inp["g"], kept=True)
        assert _note("dalpha kept", _r(cu.np_dalpha(inp["al"], inp["Om64"], inp["g"], kept=True, other=other), want, bound)) <= 1
        want, bound = cu.ref_dalpha(inp["al"], inp["Om32"], inp["g"], kept=True, dc=inp["dc"], dm=inp["dm"])
        got = cu.np_dalpha(inp["al"], inp["Om32"], inp["g"], kept=True, dc=inp["dc"], dm=inp["dm"], other=other)
        assert _note("dalpha kept + mean", _r(got, want, bound)) <= 1
        if M <= 256:
            pan = cu.make_panel(M, C, family)
            for tp in (0, 1):
                Y, E, q, bq = cu.ref_mm(pan["P32"], pan["X"], tp)
                gY, gq = cu.np_mm(pan["P32"], pan["X"], tp, other)
                assert _note("Y", _r(gY, Y, E)) <= 1 and _note("colsq", _r(gq, q, bq)) <= 1


@pytest.mark.parametrize("family", ["plain", "edge", "graded"])
@pytest.mark.parametrize("M,C,L", [(17, 523, 5), (57, 580, 3), (200, 523, 2), (250, 260, 3), (17, 4100, 2)])
def test_fp32_numpy_meets_the_gram_bounds(family, M, C, L):
    cols = cu.named_cols_gram(M, C, L)
    inp = cu.make_inputs(M, C, L, family, out="gram", gram_cols=cols)
    base = torch.from_numpy(np.random.default_rng(M).standard_normal((M, L)).astype(np.float32))
    for other in (False, True):
        for stored32 in (True, False):
            want, bound = cu.ref_gram(inp["al"], inp["g"], stored32)
            assert _note("dOmega", _r(cu.np_gram(inp["al"], inp["g"], other), want, bound)) <= 1
        want, bound = cu.ref_ddelta(inp["al"], inp["dm"], base, 1.0)
        got = base.numpy() + cu.np_ddelta(inp["al"], inp["dm"], other)
        assert _note("ddelta", _r(got, want, bound)) <= 1


# ---- 3. the visibility condition, and the removed-term formulas it uses --------------------------------------------------
@pytest.mark.parametrize("M,C,L", SMALL)
def test_a_lost_named_row_is_visible(M, C, L):
    inp = cu.make_inputs(M, C, L, "edge")
    al, Om, g = inp["al"], inp["Om32"], inp["g"]
    rows = cu.named_rows(M)
    assert M - 1 in rows and (M <= 16 or {15, 16} <= set(rows))
    v, bv = cu.ref_v(al, Om)
    da, bda = cu.ref_dalpha(al, Om, g)
    dk, bdk = cu.ref_dalpha(al, Om, g, kept=True, dc=inp["dc"], dm=inp["dm"])
    for r in rows:
        gone = al.clone()
        gone[r] = 0
        # the removed terms, written out, are the difference of the two references
        d = cu.drop_row_v(al, Om, r)
        assert torch.allclose(d, v - cu.ref_v(gone, Om)[0], rtol=1e-9, atol=1e-12 * float(v.abs().max()))
        assert cu.visible(d, bv), ("v", M, r)
        d = cu.drop_row_dalpha(al, Om, g, r)
        assert torch.allclose(d, da - cu.ref_dalpha(gone, Om, g)[0], rtol=1e-9, atol=1e-12 * float(da.abs().max()))
        assert cu.visible(d, bda) and cu.visible(d, bdk), ("dalpha", M, r)
    if M <= 256:
        pan = cu.make_panel(M, C, "edge")
        for tp in (0, 1):
            Y, E, q, bq = cu.ref_mm(pan["P32"], pan["X"], tp)
            for r in rows:
                gone = pan["X"].clone()
                gone[r] = 0
                d = cu.drop_row_mm(pan["P32"], pan["X"], tp, r)
                Y2, _, q2, _ = cu.ref_mm(pan["P32"], gone, tp)
                assert torch.allclose(d, Y - Y2, rtol=1e-9, atol=1e-12 * float(Y.abs().max()))
                assert cu.visible(d, E) and cu.visible(q - q2, bq), ("Y", M, r, tp)


@pytest.mark.parametrize("M,C,L", [(1, 260, 3), (1, 261, 3), (17, 523, 5), (57, 580, 64), (200, 523, 2), (17, 4100, 2),
                                   (29, 8252, 15), (17, 16384, 1), (17, 16385, 1), (17, 260, 257)])
def test_a_lost_named_column_is_visible(M, C, L):
    cols = cu.named_cols_gram(M, C, L)
    inp = cu.make_inputs(M, C, L, "edge", gram_cols=cols)
    al, g, dm = inp["al"], inp["g"], inp["dm"]
    want, b32 = cu.ref_gram(al, g, True)
    dd, bdd = cu.ref_ddelta(al, dm)
    for c in cols:
        d = cu.drop_col_gram(al, g, c)
        if c in (cols[0], cols[-1]):
            gone = g.clone()
            gone[:, c] = 0
            assert torch.allclose(d, want - cu.ref_gram(al, gone, True)[0], rtol=1e-9, atol=1e-12 * float(want.abs().max()))
        assert cu.visible(d, b32), ("dOmega", M, C, c)
        assert cu.visible(cu.drop_col_ddelta(al, dm, c), bdd), ("ddelta", M, C, c)


@pytest.mark.parametrize("M,C,L", cu.SOFF_SHAPES)
def test_a_lost_contributor_of_512_is_visible(M, C, L):
    """the slab reduce's sum over 512 / 513 outputs: the named outputs of g are weighted, and both a lost output and a
    lost named row then show (with plain g the sum over l cancels like a random walk and hides either)"""
    C = 64  # (the shape's tile is one whatever C: fewer columns for the CPU)
    outs = cu.named_outputs(L)
    assert outs == [0, 3, 4, L - 2, L - 1]
    inp = cu.make_inputs(M, C, L, "edge", outputs=outs)
    al, Om, g = inp["al"], inp["Om32"], inp["g"]
    want, bound = cu.ref_dalpha(al, Om, g)
    assert cu.ratio(torch.from_numpy(cu.np_dalpha(al, Om, g)), want, bound) <= 1
    for l in outs:
        gone = g.clone()
        gone[l] = 0
        d = cu.drop_output_dalpha(al, Om, g, l)
        assert torch.allclose(d, want - cu.ref_dalpha(al, Om, gone)[0], rtol=1e-9, atol=1e-12 * float(want.abs().max()))
        assert cu.visible(d, bound), (M, L, l)
    for r in cu.named_rows(M):
        assert cu.visible(cu.drop_row_dalpha(al, Om, g, r), bound), (M, L, r)
    plain = cu.make_inputs(M, C, L, "plain")
    _, b = cu.ref_dalpha(plain["al"], plain["Om32"], plain["g"])
    assert not cu.visible(cu.drop_output_dalpha(plain["al"], plain["Om32"], plain["g"], 0), b)


def test_plain_inputs_would_hide_a_column_of_a_long_gram_sum():
    """why the family exists: at C = 16384 one column of plain inputs is 6e-5 of an element's absolute sum, the bound
    2e-3 of it"""
    M, C, L = 17, 16384, 1
    inp = cu.make_inputs(M, C, L, "plain")
    _, b = cu.ref_gram(inp["al"], inp["g"], True)
    assert not cu.visible(cu.drop_col_gram(inp["al"], inp["g"], C - 1), b)
