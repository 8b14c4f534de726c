"""Helpers shared by tests/test_contraction_gpu.py and tests/test_contraction_shapes.py: the fp64
references and derived bounds of the register-resident fp32 contraction kernels, the three input families with their
named edge indices, NaN frames for inputs and outputs, and a Python restatement of the launchers' grid arithmetic
(csrc/quadform.hip, csrc/qf_common.hpp) for 256 compute units - kept here so that the shape test without a GPU and the
GPU tests cannot drift apart.

Bounds, element by element (derived, never measured; u = 2^-24, bar(K, S) = 2 (K + 4) u S as in fp64_products_util):

  v[l,c]            bar(2M, |a_c|^T |Om_l| |a_c|)            M products + M - 1 adds per row of Om_l a_c, M more of each
                                                             in the closing dot product: 2M terms deep
  dalpha (ACCUM)    bar(L (M + 2), 2 sum_l |Om_l| (|g_l| o |a|)) + u |want|
                                                             one accumulator runs over all l: L M terms, + 1 product
                                                             g a and + 1 scaling per l; then at most L slab addends,
                                                             re-associated, hence the storage term
  dalpha (kept)     bar(M + L + 4, 2 sum_l |g_l| (|Om_l| |a|))   [+ bar(L, |dcT| |dmeanT|) with the mean term]
                                                             M terms per kept product, L products g W added, the scale
                                                             and the fused add of the mean term
  Y = op(P) X       bar(M, |op P| |X|)
  colsq             sum_m (2 |Y| E + E^2) + bar(M + 1, sum_m (|Y| + E)^2),   E = Y's bound
                                                             (Y + e)^2 = Y^2 + 2 Y e + e^2 carries Y's error through the
                                                             squaring; the squaring itself and the M-long sum are M + 1
                                                             operations on the computed squares.  With |Y| <= |P||X| =: A
                                                             this is at most (6M + 26) u sum A^2, the relative form
                                                             bar(2M, sum A^2) up to the factor 2 that E already carries
  dOmega_l[i,j]     bar(C + 256, sum_c |g| |a_i| |a_j|)  [+ u |want| stored as fp32]
                                                             C terms in at most 256 partial sums, added afterwards
  ddelta[m,l]       bar(C + 256, sum_c |a_m| |dmean_l|) + |dbeta| u |ddelta0| + u |want|   (fp64 sum, fp32 store)
"""
import functools
import math

import numpy as np
import torch

from fp64_products_util import EINVAL, EUNSUPPORTED, EWORKSPACE, U32, bar, f32, f64, poisoned, ratio, same_bits  # noqa: F401

NAN = float("nan")
CUS = 256
PAD = 64  # guard elements on either side of a framed tensor (64 * 4 bytes: the view stays 16-byte aligned)
GR_KC = 64  # columns per staged chunk of gram_mfma_kernel
NSPLIT_MAX = 256

# ---- the launchers, restated (csrc/quadform.hip: mfma_mb_for, persistent_grid, gram_nl, gram_nsplit, the workspace
# layouts; csrc/qf_common.hpp: GPSA_PANEL_SHAPES, panel_wgs_per_cu, TileOrder) --------------------------------------------
MB_CLASSES = (2, 4, 7, 13, 16, 24, 32)
NCT = {2: 4, 4: 4, 7: 4, 13: 3, 16: 2, 24: 1, 32: 1}  # column tiles of 16 per wave
MB_MAX = {"fwd": 24, "keep": 16, "accum": 32, "store": 16, "gram": 16}


def cdiv(a, b):
    return -(-a // b)


def mb_for(M):
    mb = cdiv(M, 16)
    return next((k for k in MB_CLASSES if mb <= k), 0)


def width(MB):
    """columns of one workgroup's tile"""
    return 64 * NCT[MB]


def wgs_per_cu(MB):
    return 1 if MB * NCT[MB] >= 24 else 2


def full_grid(MB):
    return CUS * wgs_per_cu(MB)


def persistent_grid(MB, T):
    return min(full_grid(MB), T)


def item_ranges(T, G):
    return [(b * T // G, (b + 1) * T // G) for b in range(G)]


def tile_order(it0, it1, L):
    """TileOrder: the (tile, first l, last l) steps of the item range [it0, it1) in visiting order - whole tiles, then
    the partial last tile, then the partial first tile"""
    t0, t1 = it0 // L, (it1 - 1) // L
    lo0, hi1 = it0 - t0 * L, it1 - 1 - t1 * L
    if t0 == t1:
        return [(t0, lo0, hi1)]
    fp, lp = int(lo0 != 0), int(hi1 != L - 1)
    steps = [(t, 0, L - 1) for t in range(t0 + fp, t1 - lp + 1)]
    if lp:
        steps.append((t1, 0, hi1))
    if fp:
        steps.append((t0, lo0, L - 1))
    return steps


def range_kind(it0, it1, L):
    """(partial first tile?, whole tiles, partial last tile?) of an item range; a range inside one tile that does not
    cover it counts as a partial first tile"""
    if it1 <= it0:
        return None
    steps = tile_order(it0, it1, L)
    whole = sum(1 for (_, a, b) in steps if a == 0 and b == L - 1)
    first = any(a != 0 for (_, a, b) in steps)
    last = any(a == 0 and b != L - 1 for (_, a, b) in steps)
    return (first, whole, last)


def split_plan(MB, C, L):
    """(ntiles, T, G, the set of range kinds, contributors of the most shared tile)"""
    ntiles = cdiv(C, width(MB))
    T = ntiles * L
    G = persistent_grid(MB, T)
    rng = item_ranges(T, G)
    kinds = {range_kind(a, b, L) for (a, b) in rng} - {None}
    share = {}
    for (a, b) in rng:
        for (t, _, _) in (tile_order(a, b, L) if b > a else []):
            share[t] = share.get(t, 0) + 1
    return ntiles, T, G, kinds, max(share.values())


def last_tile_rl(M, MB):
    return 2 if M - 16 * (MB - 1) <= 8 else 4


def has_padding_row(M, MB):
    return 16 * (MB - 1) < M < 16 * MB


def gram_nl(MB, L, C):
    return 2 if (L >= 2 and MB <= 13 and C >= 8192) else 1


def gram_nsplit(C, groups, chunk=GR_KC):
    nch = cdiv(C, chunk)
    W = max(CUS // max(groups, 1), 1)
    c = cdiv(nch, W)
    return max(1, min(NSPLIT_MAX, cdiv(nch, c)))


def gram_plan(M, C, L):
    """(MB, outputs per workgroup, splits, chunk boundaries of the splits)"""
    MB = mb_for(M)
    nl = gram_nl(MB, L, C)
    ns = gram_nsplit(C, cdiv(L, nl))
    nch = cdiv(C, GR_KC)
    return MB, nl, ns, [s * nch // ns for s in range(ns + 1)]


def gram_aligned(C, alpha_off=0):
    return C % 4 == 0 and C >= 8 and alpha_off % 4 == 0


def takes_delta(M, C):
    MB = mb_for(M)
    return bool(MB) and MB <= 16 and has_padding_row(M, MB) and C % 4 == 0 and C >= 8


def _gram_splitk(C, M):
    t = cdiv(M, 64) ** 2
    return max(1, min(cdiv(512, t), max(C // 256, 1), 256))


def _big_accum_ws(M, C, L):
    wgs, slots = cdiv(M, 128) * cdiv(C, 128), 2 * CUS
    best, beff, s = 1, 0.0, 1
    while s <= 4 and (s == 1 or L // s >= 8):
        eff = (wgs * s) / (cdiv(wgs * s, slots) * slots)
        if eff > beff:
            beff, best = eff, s
        if eff >= 0.9:
            break
        s += 1
    return best * M * C * 4 if best > 1 else 0


def accum_ws(MB, L):
    MP = 16 * MB
    return L * MP * MP * 4 + full_grid(MB) * 2 * MP * width(MB) * 4


def gram_ws(MB, C, L):
    nl = gram_nl(MB, L, C)
    ns = gram_nsplit(C, cdiv(L, nl))
    return cdiv(L * cdiv(C, GR_KC) * GR_KC, 64) * 64 * 4 + L * ns * (16 * MB) ** 2 * 4


def quadform_workspace_f32(M, C, L):
    """gpsa_quadform_workspace(GPSA_F32, M, C, L) for M <= 512, 256 compute units"""
    if M > 256 and C >= 128 and C % 4:  # padded copies of alpha, g and the result panel beside the padded shape's own
        Cp = cdiv(C, 4) * 4
        return quadform_workspace_f32(M, Cp, L) + (M * Cp + L * Cp + max(L, M) * Cp) * 4 + 4096
    MB = mb_for(M)
    mfma = max(accum_ws(MB, L), gram_ws(MB, C, L) if MB <= 16 else 0) if MB else 0
    lc = min(L, 4)
    r = max(M * C * 4 * lc, (M * C * 4 + _gram_splitk(C, M) * M * M * 4) * lc) + L * M * M * 4 + 256
    if M > 128:
        r = max(r, L * M * cdiv(M, 16) * 16 * 4 + _big_accum_ws(M, C, L) + 512)
    return max(r, mfma) + 256


def keep_workspace(M, L):
    MB = mb_for(M)
    return L * (16 * MB) ** 2 * 4 + 4 * MB * 16 * 16 * 4


def keep_bytes(M, C, L):
    MB = mb_for(M)
    return L * cdiv(C, width(MB)) * width(MB) * MB * 16 * 4


def panel_mm_workspace(M):
    """what gpsa_panel_mm needs below 257 rows: the packed operand and the staging ring's slack behind it"""
    MB = mb_for(M)
    return (16 * MB) ** 2 * 4 + 4 * MB * 16 * 16 * 4


# ---- shapes (issue "Pin the fp32 contraction kernels ..."; every claim is held by tests/test_contraction_shapes.py) ----
TILE_EDGE_M = [16 * (mb - 1) + d for mb in (2, 4, 7, 13, 16) for d in (1, 8, 9, 15, 16)]  # as tests/test_hip_kernels.py
TILE_EDGE_M_BIG = [376, 377, 384, 385, 504, 505, 512]
ROWS_256 = [1] + TILE_EDGE_M
ROWS_384 = ROWS_256 + [m for m in TILE_EDGE_M_BIG if m <= 384]
ROWS_512 = ROWS_256 + TILE_EDGE_M_BIG
ROW_L = 3
# a ragged M of every class with a padding row: at most 8 rows in the last tile (the RL = 2 kernels), and more than 8
M_SMALL = {mb: 16 * (mb - 1) + 5 for mb in MB_CLASSES}
M_LARGE = {mb: 16 * (mb - 1) + 13 for mb in MB_CLASSES}
KEPT_L = [1, 2, 3, 4, 5]
STORE_C = lambda MB: [1, width(MB) - 1, width(MB), width(MB) + 1]  # noqa: E731
SOFF_SHAPES = [(20, 200, 512), (50, 200, 513)]
GRAM_CHUNKS_C, GRAM_CHUNKS_L = [523, 580], 64
GRAM_NL_C, GRAM_NL_L = 8252, [16, 15]
GRAM_NL_EDGE = [8188, 8192]
GRAM_SPLITS = [(17, 16384, 1), (17, 16385, 1), (17, 260, 257)]
GRAM_TAIL_C = [1, 4, 7, 8, 12, 60, 64, 68]


def row_class_columns(MB):
    """one full tile and a 5-column tail (not a multiple of 4), and a 4-column tail"""
    return [width(MB) + 5, width(MB) + 4]


def split_cases(MB):
    """(M, C, L, what) of the item-split list for one row-tile class.  G is a power of two, so L = 3 cannot give T = G:
    ceil(G / 3) tiles give T = G + 1 or G + 2 (ranges of 1 and 2 items), and the T = G case (one item each) runs with
    L = 4"""
    G, w = full_grid(MB), width(MB)
    out = []
    for M in (M_SMALL[MB], M_LARGE[MB]):
        out.append((M, (G // 4) * w - 3, 4, "T=G"))
        out.append((M, cdiv(G + 1, 3) * w - 3, 3, "T=G+"))
    out.append((M_LARGE[MB] if MB % 2 else M_SMALL[MB], cdiv(5 * G + 1, 3) * w - 3, 3, "T=5G+"))
    out.append((M_SMALL[MB] if MB % 2 else M_LARGE[MB], 2 * w - 3, 1, "L=1"))
    return out


# ---- named edge indices ------------------------------------------------------------------------------------------------
def named_rows(M, extra=()):
    """rows of the contracted dimension at which a row-tile kernel can go wrong: the last row, the first row of the last
    tile, both sides of its 8-row edge (RL = 2 against 4), and both sides of the first tile edge; ``extra``: a kernel's own"""
    base = 16 * (mb_for(M) - 1) if mb_for(M) else 0
    return sorted({r for r in (M - 1, base, base + 7, base + 8, 15, 16) + tuple(extra) if 0 <= r < M})


def named_cols_gram(M, C, L, extra=(), chunk=GR_KC, bounds=None):
    """columns of the Gram sum's contracted dimension: the last column and the last aligned group's first, the first
    chunk edge, and both sides of (at most four, evenly spread) split boundaries.  At most 13 columns: every named
    column weighs four times the whole unnamed panel (col_scale), so each carries about 1/13 of an element's absolute
    sum, against a bound of at most 1/500 of it - with 510 named columns (both sides of 255 boundaries) none of them
    would be visible.  chunk, bounds: another Gram kernel's chunk width and split boundaries (in chunks)"""
    if bounds is None:
        bounds = gram_plan(M, C, L)[3]
    inner = bounds[1:-1]
    if len(inner) > 4:
        inner = [inner[i * (len(inner) - 1) // 3] for i in range(4)]
    cols = {C - 1, C - 4, 0, chunk - 1, chunk} | set(extra)
    for b in inner:
        cols |= {b * chunk - 1, b * chunk}
    return sorted(c for c in cols if 0 <= c < C)


def row_scale(M):
    """power of two s with s^2 >= M: a named row's term Om[m,r] a[r] then weighs as much as the other M - 1 together"""
    return 2.0 ** math.ceil(math.log2(M) / 2) if M > 1 else 1.0


def col_scale(C):
    """power of two >= 4 C: a named column of g weighs four times the whole unnamed panel"""
    return 2.0 ** (math.ceil(math.log2(C)) + 2) if C > 1 else 1.0


def _weigh(x, idx, s, dim=1, floor=0.5):
    """scale the named columns (dim = 1) or rows (dim = 0) by s; entries below ``floor`` in magnitude are raised to it
    first (a named index must not draw a weight near zero)"""
    v = x[:, idx] if dim == 1 else x[idx]
    v = torch.where(v < 0, -1.0, 1.0) * v.abs().clamp_min(floor) * s
    if dim == 1:
        x[:, idx] = v
    else:
        x[idx] = v


def named_outputs(L):
    """contributors of a sum over many outputs l (the slab reduce with up to 512 of them): the first, both sides of its
    unroll by four, the last two"""
    return sorted({l for l in (0, 3, 4, L - 2, L - 1) if 0 <= l < L})


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=f64)


def _grades(seed, n):
    return 2.0 ** torch.randint(-10, 11, (n,), generator=torch.Generator().manual_seed(seed)).double()


@functools.lru_cache(maxsize=4)
def _base(M, C, L, seed):
    al = _randn(seed, M, C) / M ** 0.5
    A = _randn(seed + 1, L, M, M)
    Om = A @ A.transpose(1, 2) / M
    Om = (Om + Om.transpose(1, 2)) / 2 + 1e-5 * torch.eye(M, dtype=f64)
    return al, Om, _randn(seed + 2, L, C), _randn(seed + 3, L, C), _randn(seed + 4, M, L)


def make_inputs(M, C, L, family, out="rows", seed=0, gram_cols=None, outputs=None, rows=None, col_floor=0.5):
    """dict of CPU fp64 tensors: al [M,C], Om [L,M,M] (symmetric), g, dm [L,C], dc [M,L].  family: "plain", "edge"
    (named rows of al and the matching rows and columns of Om scaled by row_scale; the columns ``gram_cols`` of g and dm
    by col_scale(C), with al's entries in those columns at least 0.5 / sqrt(M); the rows ``outputs`` of g by col_scale(L):
    a sum over hundreds of outputs hides one of them as a long Gram sum hides a column), "graded" (powers of two 2^U{-10..10} such that the output named by ``out`` scales with them and its
    bound likewise: "rows" - dalpha: Om -> D Om D, al -> D^-1 al, dc -> D dc; "gram" - dOmega, ddelta: al -> D al;
    "cols" - v: al -> al D_c).  Every scaling is a power of two, so rounding to fp32 commutes with it.  rows: the edge
    family's named rows where they are not named_rows(M); col_floor: al's entries in the named columns are at least
    col_floor / sqrt(M)."""
    al, Om, g, dm, dc = [t.clone() for t in _base(M, C, L, 1000 * seed + 7 * M + C % 997 + 13 * L)]
    if family == "edge":
        rows, s = (named_rows(M) if rows is None else list(rows)), row_scale(M)
        if gram_cols:
            _weigh(g, gram_cols, col_scale(C))
            _weigh(dm, gram_cols, col_scale(C))
            _weigh(al, gram_cols, 1.0, floor=col_floor / M ** 0.5)
        if outputs:
            _weigh(g, outputs, col_scale(L), dim=0)
        al[rows] *= s
        Om[:, rows, :] *= s
        Om[:, :, rows] *= s
    elif family == "graded":
        if out == "cols":
            al *= _grades(seed + 5, C)[None, :]
        else:
            d = _grades(seed + 5, M)
            if out == "rows":
                Om *= d[None, :, None] * d[None, None, :]
                al /= d[:, None]
                dc *= d[:, None]
            else:
                al *= d[:, None]
    else:
        assert family == "plain", family
    # as stored: fp32 (Om in both precisions; the fp64 one is NOT the widened fp32 one)
    return {"al": al.float(), "Om32": Om.float(), "Om64": Om, "g": g.float(), "dm": dm.float(), "dc": dc.float()}


def make_panel(M, C, family, seed=0):
    """P [M,M] (not symmetric: a transposed read shows), X [M,C]; "edge": named rows of X, rows and columns of P;
    "graded": P -> D P, so that Y's rows scale"""
    P = _randn(seed + 11 * M, M, M) / M ** 0.5
    X = _randn(seed + 11 * M + 1, M, C)
    if family == "edge":
        rows, s = named_rows(M), row_scale(M)
        X[rows] *= s
        P[rows, :] *= s
        P[:, rows] *= s
    elif family == "graded":
        P *= _grades(seed + 5, M)[:, None]
    return {"P32": P.float(), "P64": P, "X": X.float()}


# ---- references and bounds (torch, fp64, on the device the operands are given on) -----------------------------------
def ref_v(al, Om):
    a = al.double()
    Om = Om.double()
    want = torch.stack([((Om[l] @ a) * a).sum(0) for l in range(Om.shape[0])])
    ab = torch.stack([((Om[l].abs() @ a.abs()) * a.abs()).sum(0) for l in range(Om.shape[0])])
    return want, bar(2 * a.shape[0], ab, u=U32)


def drop_row_v(al, Om, r):
    """the terms of v that contain row r of alpha: 2 a_r (Om[r,:] a) - Om[r,r] a_r^2 (Om symmetric)"""
    a, Om = al.double(), Om.double()
    return 2 * a[r][None, :] * (Om[:, r, :] @ a) - Om[:, r, r][:, None] * a[r][None, :] ** 2


def ref_dalpha(al, Om, g, kept=False, dc=None, dm=None):
    """2 sum_l g_l o (Om_l a) [+ dc dm] and its bound: the recomputing kernel (ACCUM) or the kept products' consumer"""
    a, Om, g = al.double(), Om.double(), g.double()
    M, L = a.shape[0], g.shape[0]
    want, ab = torch.zeros_like(a), torch.zeros_like(a)
    for l in range(L):
        want += 2 * g[l][None, :] * (Om[l] @ a)
        ab += 2 * (g[l].abs()[None, :] * (Om[l].abs() @ a.abs()) if kept else Om[l].abs() @ (g[l].abs()[None, :] * a.abs()))
    if not kept:
        return want, bar(L * (M + 2), ab, u=U32, want32=want)
    bound = bar(M + L + 4, ab, u=U32)
    if dc is not None:
        want = want + dc.double() @ dm.double()
        bound = bound + bar(L, dc.double().abs() @ dm.double().abs(), u=U32)
    return want, bound


def drop_row_dalpha(al, Om, g, r):
    a, Om, g = al.double(), Om.double(), g.double()
    return 2 * torch.einsum("lc,lm->mc", g * a[r][None, :], Om[:, :, r])


def drop_output_dalpha(al, Om, g, l):
    return 2 * g.double()[l][None, :] * (Om.double()[l] @ al.double())


def ref_mm(P, X, transP):
    Pm, Xd = (P.double().t() if transP else P.double()), X.double()
    M = Xd.shape[0]
    Y, A = Pm @ Xd, Pm.abs() @ Xd.abs()
    E = bar(M, A, u=U32)
    bq = (2 * Y.abs() * E + E * E).sum(0) + bar(M + 1, ((Y.abs() + E) ** 2).sum(0), u=U32)
    return Y, E, (Y * Y).sum(0), bq


def drop_row_mm(P, X, transP, r):
    Pm = P.double().t() if transP else P.double()
    return Pm[:, r][:, None] * X.double()[r][None, :]


def ref_gram(al, g, stored32, prod_bar=None):
    """prod_bar(C, S): another contraction's bound of a C-term element (its partial sums' additions included)"""
    a, g = al.double(), g.double()
    C = a.shape[1]
    want = torch.stack([(a * g[l][None, :]) @ a.t() for l in range(g.shape[0])])
    ab = torch.stack([(a.abs() * g[l].abs()[None, :]) @ a.abs().t() for l in range(g.shape[0])])
    if prod_bar is not None:
        return want, prod_bar(C, ab) + (U32 * want.abs() if stored32 else 0.0)
    return want, bar(C + NSPLIT_MAX, ab, u=U32, want32=want if stored32 else None)


def drop_col_gram(al, g, c):
    a = al.double()[:, c]
    return g.double()[:, c][:, None, None] * (a[:, None] * a[None, :])[None]


def ref_ddelta(al, dm, dd0=None, dbeta=0.0, prod_bar=None):
    a, d = al.double(), dm.double()
    want = a @ d.t()
    S = a.abs() @ d.abs().t()
    bound = bar(a.shape[1] + NSPLIT_MAX, S, u=U32) if prod_bar is None else prod_bar(a.shape[1], S)
    if dd0 is not None and dbeta != 0.0:
        want = want + dbeta * dd0.double()
        bound = bound + abs(dbeta) * U32 * dd0.double().abs()
    return want, bound + U32 * want.abs()


def drop_col_ddelta(al, dm, c):
    return al.double()[:, c][:, None] * dm.double()[:, c][None, :]


def visible(delta, bound):
    """the visibility condition: removing one named index changes at least half of the elements it feeds (those whose
    removed term is not exactly zero) by more than 4 x their bound"""
    fed = delta != 0
    if not bool(fed.any()):
        return False
    return float((delta.abs()[fed] > 4 * bound[fed]).double().mean()) >= 0.5


# ---- frames ------------------------------------------------------------------------------------------------------------
class Frame:
    """a tensor of ``shape`` in the middle of a larger device buffer filled with NaN (PAD elements on either side, so a
    16-byte aligned view; ``off`` extra elements move it off that alignment).  An input is copied in (``src``); an
    output stays NaN until the kernel writes it."""

    def __init__(self, shape, dtype, dev, src=None, off=0):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = int(np.prod(shape))
        self.lo, self.n = PAD + off, n
        self.buf = torch.full((self.lo + n + PAD,), NAN, dtype=dtype, device=dev)
        self.view = self.buf[self.lo: self.lo + n].view(shape)
        assert (self.view.data_ptr() % 16 == 0) == (off * self.buf.element_size() % 16 == 0)
        if src is not None:
            assert tuple(src.shape) == shape and src.dtype == dtype, (src.shape, shape, src.dtype, dtype)
            self.view.copy_(src)

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool(torch.isnan(self.buf[: self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())

    def untouched(self):
        """nothing was written at all (error returns)"""
        return bool(torch.isnan(self.buf).all())

    def written(self):
        return not bool(torch.isnan(self.view).any())


# ---- the operations in plain fp32 NumPy (tests/test_contraction_shapes.py: an honest fp32 evaluation, in the natural
# order and in a deliberately different one, must stay inside every bound) ---------------------------------------------
def np_v(al, Om, other=False):
    a, Om = al.numpy(), Om.float().numpy()
    if other:  # rows visited backwards
        a, Om = a[::-1].copy(), Om[:, ::-1, ::-1].copy()
    return np.stack([((Om[l] @ a) * a).sum(0, dtype=np.float32) for l in range(Om.shape[0])])


def np_dalpha(al, Om, g, kept=False, dc=None, dm=None, other=False):
    a, Om, g = al.numpy(), Om.float().numpy(), g.numpy()
    acc = np.zeros_like(a)
    for l in (range(g.shape[0] - 1, -1, -1) if other else range(g.shape[0])):  # other: reversed l
        acc += g[l][None, :] * (Om[l] @ a) if kept else Om[l] @ (g[l][None, :] * a)
    out = np.float32(2) * acc
    return out + dc.numpy() @ dm.numpy() if dc is not None else out


def np_mm(P, X, transP, other=False):
    Pm, Xn = (P.float().numpy().T if transP else P.float().numpy()), X.numpy()
    if other:  # contracted index backwards
        Pm, Xn = Pm[:, ::-1].copy(), Xn[::-1].copy()
    Y = Pm @ Xn
    return Y, (Y * Y).sum(0, dtype=np.float32)


def _chunks(C, other, chunk=GR_KC):
    edges = list(range(0, C, chunk)) + [C]
    pairs = list(zip(edges[:-1], edges[1:]))
    return pairs[::-1] if other else [(0, C)]


def np_gram(al, g, other=False, chunk=GR_KC, matmul=None):
    """matmul(A, B): the product of two fp32 arrays as another contraction forms it (default: NumPy's)"""
    mm = matmul or (lambda A, B: A @ B)
    a, g = al.numpy(), g.numpy()
    out = np.zeros((g.shape[0], a.shape[0], a.shape[0]), np.float32)
    for (c0, c1) in _chunks(a.shape[1], other, chunk):  # other: chunks, last first
        for l in range(g.shape[0]):
            out[l] += mm(a[:, c0:c1] * g[l, c0:c1][None, :], a[:, c0:c1].T)
    return out


def np_ddelta(al, dm, other=False, chunk=GR_KC, matmul=None):
    mm = matmul or (lambda A, B: A @ B)
    a, d = al.numpy(), dm.numpy()
    out = np.zeros((a.shape[0], d.shape[0]), np.float32)
    for (c0, c1) in _chunks(a.shape[1], other, chunk):
        out += mm(a[:, c0:c1], d[:, c0:c1].T)
    return out
