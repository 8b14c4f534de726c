"""Helpers shared by tests/test_x3_elbo_gpu.py, tests/test_x3_gram_gpu.py and tests/test_x3_shapes.py (DESIGN.md section
2h): the bf16x3 pair of csrc/qf_x3.hip - panel_elbo_x3_kernel behind gpsa_quadform_elbo_x3_f32 / _delta_x3_f32 and
gram_x3_kernel behind gpsa_quadform_bwd_omega_x3 / _delta_x3 - held as sections 2e / 2g hold the fp32 kernels.  The
references, input families, frames, closings and stage comparison are contraction_util's and fused_lik_util's (with the
contraction's own element bound passed in); here are only what differs: the launch arithmetic of the x3 launchers restated
for 256 compute units (csrc/qf_common.hpp: GPSA_ELBO_X3_SHAPES; csrc/quadform.hip: elbo_ws(true, ..), elbo_launch(x3),
gram_nsplit(C, L, 32), gram_x3_ws), the bound of a three-piece product, an emulation of the contraction on the CPU, the
kernel's own named rows, and the three-piece case.

The bound (derived, never measured; u = 2^-24, bar(K, S) = 2 (K + 4) u S as in section 2b).  Every fp32 operand is split
a = a1 + a2 + a3, each piece the bf16 rounding (8 significant bits, round to nearest even) of what the earlier ones left:
the two differences are exact (Sterbenz), |a2| <= 2^-8 |a|, |a3| <= 2^-17 |a|, and what a3 leaves is at most 2^-26 |a| and
is 0 for every fp32 value whose three pieces fit in its 24 bits (test_x3_shapes.py: none of 10^6 leaves anything).  The
kernels add the six products a_i b_j with i + j <= 4.  The three they drop are at most (2^-25 + 2^-25 + 2^-34) |a b| per
term.  A kept product has 16 significant bits: exact in fp32.  |a1| <= (1 + 2^-8) |a|, so the absolute sum of the six is
at most ((1 + 2^-8)^2 + 2^-7 (1 + 2^-8) + 2^-16 (1 + 2^-8) + 2^-16) S <= (1 + 2^-6 + 2^-13) S - the issue's (1 + 2^-7)
counted a1 b1 alone above S; the two second-order products are another 2^-7.  Hence, for K terms with absolute sum S and
``adds`` further fp32 additions of partial sums,

    bar_x3(K, S, adds) = bar(6 K + adds, (1 + 2^-6 + 2^-13) S) + 1.001 u S.
"""
import math

import numpy as np
import torch

import contraction_util as cu
import fused_lik_util as fu
from contraction_util import CUS, U32, bar, cdiv, f32, f64, has_padding_row, item_ranges, mb_for, range_kind, tile_order  # noqa: F401

U = U32

# ---- the launchers, restated ---------------------------------------------------------------------------------------------
X3_CLASSES = (2, 4, 7, 13, 16)
X3_NCT = {2: 2, 4: 2, 7: 2, 13: 1, 16: 1}  # GPSA_ELBO_X3_SHAPES
PANEL_MAX_C = 1 << 26


def x3_width(MB):
    """columns of one workgroup's tile: four waves of NCT column tiles of 16"""
    return 64 * X3_NCT[MB]


def x3_kb(MB):
    """32-deep K blocks (the last one half empty when MB is odd)"""
    return (MB + 1) // 2


def x3_kidx(b, kq, e):
    """row of alpha (= column of Omega) of element e of lane group kq in K block b"""
    return 32 * b + (4 * kq + e if e < 4 else 16 + 4 * kq + e - 4)


def x3_grid(T):
    """one workgroup per CU, at most one per item"""
    return min(CUS, T)


def x3_elbo_workspace(M, C, L):
    """gpsa_quadform_elbo_x3_f32_workspace: [three-plane bf16 image of Omega, rounded to 256 bytes | two slabs for each of
    num_cus() workgroups | two chunks of ring slack]"""
    MB = mb_for(M)
    if M < 1 or C < 1 or L < 1 or not MB or MB > 16 or C > PANEL_MAX_C:
        return 0
    pk = cdiv(L * x3_kb(MB) * MB * 3 * 1024, 256) * 256
    return pk + CUS * 2 * MB * 16 * x3_width(MB) * 4 + 2 * MB * 3 * 1024


def x3_plan(M, C, L):
    """(ntiles, T, G, the set of range kinds, workgroups that write both slab halves: ``which`` 0 and 1)"""
    MB = mb_for(M)
    ntiles = cdiv(C, x3_width(MB))
    T = ntiles * L
    G = x3_grid(T)
    rng = item_ranges(T, G)
    kinds = {range_kind(a, b, L) for (a, b) in rng} - {None}
    both = sum(1 for (a, b) in rng if b > a and sum(1 for (_, lo, hi) in tile_order(a, b, L) if (lo, hi) != (0, L - 1)) >= 2)
    return ntiles, T, G, kinds, both


def x3_gram_nsplit(C, L):
    return cu.gram_nsplit(C, L, 32)


def x3_gram_bounds(C, L):
    """chunk boundaries of the splits (workgroup (l, s) sweeps chunks [s nch / ns, (s + 1) nch / ns))"""
    nch, ns = cdiv(C, 32), x3_gram_nsplit(C, L)
    return [s * nch // ns for s in range(ns + 1)]


def x3_gram_workspace(M, C, L):
    """gpsa_quadform_bwd_omega_x3_workspace: [alpha's three-plane image, whole 32-column chunks | partials [L][ns][MP][MP]]"""
    MB = mb_for(M)
    if M < 1 or C < 1 or L < 1 or L > 65535 or not MB or MB > 16:
        return 0
    return cdiv(C, 32) * MB * 3 * 1024 + L * x3_gram_nsplit(C, L) * (16 * MB) ** 2 * 4


def x3_takes_delta(M):
    MB = mb_for(M)
    return M >= 1 and bool(MB) and MB <= 16 and has_padding_row(M, MB)


# ---- the bound -------------------------------------------------------------------------------------------------------------
X3_ABS = 1 + 2.0 ** -6 + 2.0 ** -13


def bar_x3(K, S, adds=0):
    return bar(6 * K + adds, X3_ABS * S, u=U) + 1.001 * U * S


def gram_bars(C, L):
    """(dOmega's, ddelta's) element bound: C terms in ns partial sums (ns - 1 additions, fp32 or wider); dOmega's row
    fragment is fp32(g alpha) before its split: one more u per term (1.001: the rounded fragment's own absolute sum)"""
    ns = x3_gram_nsplit(C, L)
    return (lambda K, S: bar_x3(K, S, adds=ns) + 1.001 * U * S), (lambda K, S: bar_x3(K, S, adds=ns))


# ---- the contraction on the CPU -----------------------------------------------------------------------------------------------
def split3(x):
    """fp32 tensor -> its three bf16 pieces (as fp32 tensors) and what they leave"""
    a1 = x.bfloat16().float()
    r1 = x - a1
    a2 = r1.bfloat16().float()
    r2 = r1 - a2
    a3 = r2.bfloat16().float()
    return (a1, a2, a3), r2 - a3


PRODUCTS = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]  # the kernels' order per K block: smallest first


def x3_matmul(A, B, other=False, drop=None):
    """A [m, k] @ B [k, n] (fp32 NumPy) as the kernels form it: both operands split, per 32-deep block of k the six products
    in the kernels' order, each block product and every addition in fp32.  other: blocks backwards, products largest first,
    k backwards inside a block.  drop: one (i, j) of PRODUCTS left out"""
    Ap = [t.numpy() for t in split3(torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)))[0]]
    Bp = [t.numpy() for t in split3(torch.from_numpy(np.ascontiguousarray(B, dtype=np.float32)))[0]]
    K = A.shape[1]
    blocks = [(k0, min(k0 + 32, K)) for k0 in range(0, K, 32)]
    prods = [p for p in PRODUCTS if p != drop]
    if other:
        blocks, prods = blocks[::-1], prods[::-1]
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for (k0, k1) in blocks:
        ks = slice(k0, k1)
        for (i, j) in prods:
            a, b = Ap[i][:, ks], Bp[j][ks]
            if other:
                a, b = np.ascontiguousarray(a[:, ::-1]), np.ascontiguousarray(b[::-1])
            acc = acc + a @ b
    return acc


def mm(other):
    return lambda A, B: x3_matmul(A, B, other)


# ---- named rows and the families ---------------------------------------------------------------------------------------------
def x3_named_rows(M):
    """sections 2e / 2g's rows, and both sides of a K-block edge (31, 32), the last K block's first row and both sides of
    the x3_kidx halves in it (element 3 / 4 of lane group 0; row 16: the second row tile of the block)"""
    kb = 32 * (x3_kb(mb_for(M)) - 1)
    return cu.named_rows(M, extra=(31, 32, kb, kb + 3, kb + 4, kb + 16))


def elbo_inputs(M, C, L, family, delta=False, seed=0):
    """fused_lik_util's Gaussian case with this kernel's named rows (scaled by section 2e's s, s^2 >= M: the visibility
    condition holds under the x3 bounds at every shape of the GPU file without raising it); "OmR32" / "OmR64": what the reference
    multiplies - the fp32 rounding of Omega widened (pack_x3_kernel splits that rounding of an fp64 Omega)"""
    inp = fu.elbo_inputs(M, C, L, fu.GAUSS, family, delta=delta, seed=seed, rows=x3_named_rows(M))
    inp["OmR32"], inp["OmR64"] = inp["Om32"], inp["Om64"].float()
    return inp


def elbo_reference(inp, M, C, L, om, delta):
    return fu.elbo_reference(inp, M, C, L, fu.GAUSS, om="OmR" + om[-2:], delta=delta, prod_bar=bar_x3)


def elbo_ratios(inp, ref, M, C, L, got):
    return fu.elbo_stage_ratios(inp, ref, M, C, L, fu.GAUSS, got, prod_bar=bar_x3, nct=X3_NCT[mb_for(M)])


def elbo_visibility(inp, ref, cl, got, M, C, L, om):
    fu.elbo_visibility(inp, ref, cl, got, M, C, L, fu.GAUSS, "OmR" + om[-2:], prod_bar=bar_x3, nct=X3_NCT[mb_for(M)],
                       rows=x3_named_rows(M))


def elbo_np(inp, M, C, L, om, delta, other):
    return fu.elbo_np(inp, M, C, L, fu.GAUSS, om=om, delta=delta, other=other, matmul=mm(other))


def gram_named_cols(M, C, L):
    """both sides of (at most four) split boundaries in 32-column chunks, the first chunk edge, an 8-column lane-group
    edge, the last column and the last group of four"""
    return cu.named_cols_gram(M, C, L, extra=(7, 8), chunk=32, bounds=x3_gram_bounds(C, L))


def gram_inputs(M, C, L, family, cols):
    """contraction_util's Gram families; alpha's entries in the named columns are raised to one standard deviation (0.5 in
    section 2e): up to fifteen named columns share an element's absolute sum, the bound is six times section 2e's, and a
    column that drew small entries fell below the visibility condition at (17, 8193, 1)"""
    return cu.make_inputs(M, C, L, family, out="gram", gram_cols=cols, col_floor=1.0)


# ---- shapes (issue "Pin the bf16x3 ELBO and Gram kernels ..."; every claim is held by tests/test_x3_shapes.py) -------------------
ELBO_ROWS = fu.ELBO_ROWS  # 1, 16 (MB - 1) + {1, 8, 9, 15, 16}, 65, 113, 192
ROW_L = 3
DELTA_M = fu.DELTA_M
DELTA_REFUSED = fu.DELTA_REFUSED
GRAM_C = [1, 7, 8, 31, 32, 33, 63, 64, 65]
GRAM_DELTA_C = [1, 4, 7]
GRAM_CHUNKS = [523, 580]
GRAM_CHUNKS_L = 64
GRAM_SPLITS = [(17, 8192, 1), (17, 8193, 1), (17, 260, 257)]
GRAM_ROW_C = [265, 264]


def elbo_columns(MB):
    """one full tile and a 5-column tail, and a 4-column tail"""
    return [x3_width(MB) + 5, x3_width(MB) + 4]


def elbo_split_cases(MB):
    """(M, C, L, what), G = 256 for every class: T = G (L = 4, one item each), T = G + 1 / + 2 (L = 3; at G = 256 no two-item
    range crosses a tile edge), the fewest tiles above that at which one workgroup ends one tile and begins the next
    (T = G + 5: ``which`` 0 and 1), T = 2G at L = 2 (one whole tile each, stored plainly, the output loop twice), two tiles at
    L = 1, and T = 5G + 1 at L = 3 for one class of each width (MB 7 at 128, MB 13 at 64)"""
    G, w = CUS, x3_width(MB)
    Ms, Ml = 16 * (MB - 1) + 5, 16 * (MB - 1) + 13
    out = [(Ms, (G // 4) * w - 3, 4, "T=G"), (Ml, cdiv(G + 1, 3) * w - 3, 3, "T=G+"), (Ms if MB % 2 else Ml, 2 * w - 3, 1, "L=1")]
    nt = next(n for n in range(cdiv(G + 1, 3), G) if x3_plan(Ms, n * w - 3, 3)[4] >= 1)
    out.append((Ms, nt * w - 3, 3, "T=G++"))
    out.append((Ml, G * w - 3, 2, "T=2G"))
    if MB in (7, 13):
        out.append((Ml, cdiv(5 * G + 1, 3) * w - 3, 3, "T=5G+"))
    return out


# ---- the three-piece case ------------------------------------------------------------------------------------------------------
C1 = C2 = 0.96875


def three(e):
    """2^e (1 + c1 2^-8 + c2 2^-17): an fp32 value whose three pieces are all positive and as large as they can be"""
    return torch.as_tensor(2.0, dtype=f64) ** torch.as_tensor(e, dtype=f64) * (1 + C1 * 2.0 ** -8 + C2 * 2.0 ** -17)


def pieces64(x):
    return [p.double() for p in split3(x.float())[0]]


def three_piece_elbo(C=133, L=1):
    """M = 1: Omega_l = three(0), alpha_c = +- three(2 or 3), so v = alpha^2 Omega is 16 .. 64 against resid <= 0.5; meanT = 0,
    |eps| in [1, 2]: the draw is sd eps and carries half of v's relative error"""
    g = torch.Generator().manual_seed(133)
    S, N = fu.sample_split(C)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    al = (sign * three(2 + (torch.arange(C) % 2)))[None, :]
    Om = three(torch.zeros(L, 1, 1))
    var_u = torch.tensor([math.log(0.8)], dtype=f32)
    resid = 0.3 + 0.2 * torch.rand(C, generator=g, dtype=f64)
    eps = (1 + torch.rand(C, L, generator=g, dtype=f64)) * torch.where(torch.rand(C, L, generator=g) < 0.5, -1.0, 1.0)
    inp = {"al": al.float(), "Om32": Om.float(), "Om64": Om.clone(), "q": math.exp(float(var_u)) - resid, "var_u": var_u,
           "eps": eps.float(), "S": S, "N": N, "named_cols": fu.elbo_named_cols(C, N), "meanT": torch.zeros(L, C, dtype=f32),
           "noise_u": torch.tensor([math.log(0.7)], dtype=f32)}
    assert torch.equal(inp["al"].double(), al) and torch.equal(inp["Om32"].double(), Om), "not fp32 values"
    inp["OmR32"], inp["OmR64"] = inp["Om32"], inp["Om64"].float()
    sd = torch.sqrt(resid[None, :] + (al * al * Om[:, 0]) + 2e-5)
    inp["Y"] = ((sd * eps.t())[:, :N].t() + 0.7 * torch.randn(N, L, generator=g, dtype=f64)).float()
    return inp


def three_piece_elbo_moves(inp, ref, L):
    """{(i, j): (|change of FT| / E_F, |change of abar| / its bound)} [L or 1, C] when product Omega_i alpha_j is lost; g from
    the reference's own closing"""
    a, Om = inp["al"].double(), inp["Om32"].double()
    cl = fu.elbo_closing(inp, ref, fu.GAUSS, ref["F"])
    g = cl["d"] * ref["e"] / (2 * ref["sd"])
    b_ab = fu.abar_bound(1, L, 2 * (g.abs()[:, None, :] * ref["absW"]).sum(0), 2 * (g[:, None, :] * ref["W"]).sum(0), bar_x3)
    Op, ap = pieces64(inp["Om32"]), pieces64(inp["al"])
    out = {}
    for (i, j) in PRODUCTS:
        lost = Op[i][:, 0] * ap[j]  # [L, C]: what W_l loses
        F2 = inp["meanT"].double() + torch.sqrt(ref["var"] - a * lost) * ref["e"]
        out[(i, j)] = ((ref["F"] - F2).abs() / ref["E_F"], (2 * (g * lost).sum(0, keepdim=True)).abs() / b_ab)
    return out


def three_piece_gram(M=21):
    """C = 1, L = 1, g = 1 (the row fragment g alpha is alpha itself): dOmega[i, j] = a_i a_j, ddelta[m] = a_m dm"""
    al = three((torch.arange(M) % 5) - 2.0)[:, None] * torch.where(torch.arange(M) % 3 == 0, -1.0, 1.0).double()[:, None]
    inp = {"al": al.float(), "g": torch.ones(1, 1, dtype=f32), "dm": three(torch.ones(1, 1)).float()}
    assert torch.equal(inp["al"].double(), al)
    return inp


def three_piece_gram_moves(inp):
    """{(i, j): (|lost product| / dOmega's fp32 bound, |lost| / ddelta's bound)}: row fragment piece i, column fragment j"""
    al, dm = inp["al"], inp["dm"]
    bo, bd = gram_bars(1, 1)
    _, b_om = cu.ref_gram(al, inp["g"], True, prod_bar=bo)
    _, b_dd = cu.ref_ddelta(al, dm, prod_bar=bd)
    ap, dp = pieces64(al), pieces64(dm)
    out = {}
    for (i, j) in PRODUCTS:
        lost = ap[i] @ ap[j].t()
        lost = torch.minimum(lost.abs(), lost.abs().t())[None]
        # ddelta[m]: the row fragment is dmean (row M of the last tile), the column fragment alpha_m
        out[(i, j)] = (lost / b_om, (ap[j] @ dp[i].t()).abs() / b_dd)
    return out
