"""Helpers shared by tests/test_factor_gpu.py and tests/test_factor_shapes.py: the longdouble reference of the batched fp64
factorisations (csrc/linalg.hip), the derived element-wise bounds, the seeded input families and the shape lists (kept here
so the non-GPU shape test and the GPU tests cannot drift apart).

Reference: a plain right-looking Cholesky and a forward-substitution inverse in numpy.longdouble (64-bit mantissa), of the
same fp64 input the kernels get: L, X = L^-1, logdet.

Bounds, element by element on the lower triangle (u = 2^-53, g = 2 (M + 4) u: the ``bar`` of fp64_products_util with K = M;
the factor 2 covers the reference's and the residual products' own rounding), nothing tuned to the kernels:

  Cholesky factor Lh (backward error; Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3 - any order of the
  operations, any conditioning):                      |Lh Lh^T - A| <= g |Lh| |Lh|^T
  inverse Xh of a given triangular L (Thm 8.5, column by column; L is the exact input, no conditioning enters):
                                                      |L Xh - I|    <= g |L| |Xh|
  Xh of the fused entries (first-order forward error: the Cholesky perturbation dL = L low(X dA X^T) with
  |dA| <= g |L| |L|^T, low(B) = strict lower triangle + half the diagonal, plus the inversion residual; x 1.01 for the
  higher orders), with S = |X| |L| |L|^T |X|^T:       |Xh - X|      <= 1.01 g (|X| |L| low(S) |X| + |X| |L| |X|)
  every logdet:                                       |ldh - ld|    <= (M + 4) u (2 tr S + 2 sum_j |log L_jj|)

Residual products are formed in longdouble up to M = 600 and in fp64 above that.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from fp64_products_util import PAD, U64, f64, ratio, rnd

LD = np.longdouble
LD_MAX = 600  # longdouble references and residual products stop here (about 1 s at this size)
ISENTINEL = -7777  # the int32 frame around info
HIGHER_ORDERS = 1.01

# ---- shapes (read from the launchers of csrc/linalg.hip) -------------------------------------------------------------
# gpsa_chol_inv_f64, M <= 208: chol_inv_blk_kernel<NT> for ceil(M / 16) <= NT; first, last and a ragged member of each
PANEL_M = {2: [1, 17, 32], 4: [33, 49, 64], 7: [65, 100, 112], 10: [113, 150, 160], 13: [161, 199, 200, 208]}
# ... 208 < M <= 256: chol_inv_reg_kernel<NT, 32> for ceil(M / 32) <= NT
REG32_M = {7: [209, 224], 8: [225, 241, 256]}
FUSED_M = [M for ms in PANEL_M.values() for M in ms] + [M for ms in REG32_M.values() for M in ms]
# gpsa_chol_inv_blocked_f64 runs chol_inv_reg_kernel<NT, TS> on every diagonal block: TS = 16 up to 208 columns
REG_NT = {16: (2, 4, 7, 13, 16), 32: (1, 2, 4, 7, 8)}
# M > 256: the diagonal blocks each M is meant to be cut into
BLOCKED_BIG = {257: [144, 113], 417: [224, 193], 500: [256, 244], 513: [176, 176, 161], 529: [192, 192, 145]}
# gpsa_chol_f64 / gpsa_tri_inv_f64: packed (LDS) / global edge at 200, tri_inv_body's 256-column passes, and one size past
# LA_THREADS = 1024 (second trip of the strided loops).  M = 4096 (a multi-second single-workgroup sweep) is left out.
UNFUSED_M = [199, 200, 201, 256, 257, 258, 513]
UNFUSED_LONG_M = 1030
LA_PACKED_MAX, LA_GLOBAL_MAX, LA_THREADS = 200, 4096, 1024
FAMILIES = ["wishart", "rbf", "graded"]
TRI_FAMILIES = ["tri", "tri_graded"]
# gpsa_bdot: edges of the split count ceil(n / 2048) and of its cap of 32; the finish kernel has 64 threads per block
BDOT_N = [1, 2048, 2049, 65536, 65537, 100003]
BDOT_BATCH = [1, 64, 65]
BDOT_MAX_SPLITS = 32
ADD_DIAG = [(255, 1), (51, 5), (256, 1), (16, 16), (64, 4), (257, 1)]  # M * batch on both sides of one block of 256


def bdot_splits(n):
    return min(BDOT_MAX_SPLITS, -(-n // 2048))


def panel_class(M):
    """NT of chol_inv_blk_kernel for M <= 208"""
    nt = -(-M // 16)
    return next(c for c in (2, 4, 7, 10, 13) if nt <= c)


def reg_class(b):
    """(TS, NT) of chol_inv_reg_kernel for a diagonal block of b <= 256 columns"""
    ts = 16 if b <= 208 else 32
    nt = -(-b // ts)
    return ts, next(c for c in REG_NT[ts] if nt <= c)


def block_size_from_workspace(nbytes, M, batch):
    """bytes / (8 batch) = 2 M^2 + bs M"""
    per = nbytes // (8 * batch)
    assert nbytes % (8 * batch) == 0 and (per - 2 * M * M) % M == 0, (nbytes, M, batch)
    return (per - 2 * M * M) // M


def blocks(M, bs):
    return [min(bs, M - o) for o in range(0, M, bs)]


# ---- input families (seeded; matrix k of a batch is the same whatever the batch size) --------------------------------
def _seed(name, M, k):
    return 1000003 * (FAMILIES + TRI_FAMILIES).index(name) + 101 * M + k


def _wishart(M, seed):
    A = rnd(M, M, seed=seed)
    return A @ A.T / M + 0.05 * torch.eye(M, dtype=f64)


@functools.lru_cache(maxsize=256)
def matrix(name, M, k):
    """wishart: A A^T / M + 0.05 I (cond ~ 80).  rbf: the warp GP's K_uu at init, an RBF kernel on a 2-D grid + 1e-5 I
    (cond 1e6 .. 1e7; lengthscale 1, 0.9, 1.1 by k).  graded: D A D, D = diag(10^U(-6, 6)), symmetrised - Cholesky is
    scale-invariant and so are the bounds, a hidden absolute tolerance or an error in the small rows shows here alone.
    tri: lower triangular, off-diagonal N(0, 1 / M) (N(0, 1) entries would make the inverse grow like 2^M), |diag| >= 0.5
    with random signs.  tri_graded: the same with its rows scaled by 10^U(-6, 6)."""
    seed = _seed(name, M, k)
    if name == "wishart":
        return _wishart(M, seed)
    if name == "rbf":
        g = max(1, math.ceil(math.sqrt(M)))
        z = torch.linspace(0, 10, g, dtype=f64)
        Z = torch.stack(torch.meshgrid(z, z, indexing="ij"), -1).reshape(-1, 2)[:M]
        ell = (1.0, 0.9, 1.1)[k % 3]
        return torch.exp(-0.5 * torch.cdist(Z, Z) ** 2 / ell ** 2) + 1e-5 * torch.eye(M, dtype=f64)
    gen = torch.Generator().manual_seed(seed + 7)
    d = 10.0 ** (12.0 * torch.rand(M, generator=gen, dtype=f64) - 6.0)
    if name == "graded":
        A = d[:, None] * _wishart(M, seed) * d[None, :]
        return (A + A.T) / 2
    N = rnd(M, M, seed=seed)
    sign = torch.where(torch.diagonal(N) < 0, -1.0, 1.0).to(f64)
    L = torch.tril(N, -1) / math.sqrt(M) + torch.diag(sign * (0.5 + rnd(M, seed=seed + 1).abs()))
    return L if name == "tri" else d[:, None] * L


def batch_of(name, M, ks):
    return torch.stack([matrix(name, M, k) for k in ks]).contiguous()


# ---- reference ---------------------------------------------------------------------------------------------------------
def chol_ld(A):
    """right-looking Cholesky in longdouble of an fp64 (numpy) matrix; lower triangle read"""
    W = np.tril(A).astype(LD)
    M = W.shape[0]
    for j in range(M):
        W[j, j] = np.sqrt(W[j, j])
        W[j + 1:, j] /= W[j, j]
        c = W[j + 1:, j]
        W[j + 1:, j + 1:] -= np.tril(np.outer(c, c))
    return W


def tri_inv_any(L, dtype=LD):
    """forward-substitution inverse, row by row, in ``dtype``"""
    L = L.astype(dtype)
    M = L.shape[0]
    X = np.zeros((M, M), dtype)
    for i in range(M):
        X[i, i] = 1 / L[i, i]
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) * X[i, i]
    return X


def chol_f64_plain(A):
    """the same right-looking algorithm in plain fp64, scaling by the reciprocal as the kernels do"""
    W = np.tril(A).astype(np.float64)
    M = W.shape[0]
    for j in range(M):
        W[j, j] = np.sqrt(W[j, j])
        W[j + 1:, j] *= 1.0 / W[j, j]
        c = W[j + 1:, j]
        W[j + 1:, j + 1:] -= np.tril(np.outer(c, c))
    return W


def low(B):
    return np.tril(B, -1) + 0.5 * np.diag(np.diag(B))


def gfac(M):
    return 2.0 * (M + 4) * U64


Ref = namedtuple("Ref", "A L X logdet bX bld")


@functools.lru_cache(maxsize=40)
def reference(name, M, k):
    """L, X, logdet in longdouble and the bounds on X (lower triangle; zero above: must be exact) and on logdet"""
    assert M <= LD_MAX
    A = matrix(name, M, k).numpy()
    L = chol_ld(A)
    X = tri_inv_any(L)
    logL = np.log(np.diag(L))
    aL, aX = np.abs(L).astype(np.float64), np.abs(X).astype(np.float64)
    P = aX @ aL
    S = P @ P.T
    g = gfac(M)
    bX = np.tril(HIGHER_ORDERS * g * (P @ low(S) @ aX + P @ aX))
    bld = (M + 4) * U64 * (2.0 * np.trace(S) + 2.0 * float(np.sum(np.abs(logL))))
    return Ref(A, L, X, 2 * np.sum(logL), bX, bld)


# ---- checks: each returns the largest error / bound (inf for NaN, or for an error where the bound is zero) -------------
def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _ratio(err, bound):
    err = torch.from_numpy(np.ascontiguousarray(np.asarray(err, dtype=np.float64)))
    return ratio(err, torch.zeros_like(err), torch.from_numpy(np.ascontiguousarray(bound, dtype=np.float64)))


def x_ratio(Xh, ref):
    """forward error of a fused entry's inverse factor; the strict upper triangle must be exact zeros"""
    return _ratio(np.abs(_np(Xh).astype(LD) - ref.X), ref.bX)


def logdet_ratio(ldh, ref):
    return _ratio(np.abs(LD(float(ldh)) - ref.logdet).reshape(1), np.array([ref.bld]))


def chol_residual_ratio(Lh, A):
    """|Lh Lh^T - A| <= g |Lh| |Lh|^T on the lower triangle; Lh's strict upper triangle must be exact zeros"""
    Lh, A = _np(Lh), _np(A)
    M = A.shape[0]
    if not np.isfinite(Lh).all() or np.triu(Lh, 1).any():
        return float("inf")
    wide = LD if M <= LD_MAX else np.float64
    Lw = Lh.astype(wide)
    res = np.abs(Lw @ Lw.T - A.astype(wide)).astype(np.float64)
    aL = np.abs(Lh)
    return _ratio(np.tril(res), np.tril(gfac(M) * (aL @ aL.T)))


def tri_inv_residual_ratio(Xh, L):
    """|L Xh - I| <= g |L| |Xh| on the lower triangle; Xh's strict upper triangle must be exact zeros"""
    Xh, L = _np(Xh), _np(L)
    M = L.shape[0]
    if not np.isfinite(Xh).all() or np.triu(Xh, 1).any():
        return float("inf")
    wide = LD if M <= LD_MAX else np.float64
    res = np.abs(L.astype(wide) @ Xh.astype(wide) - np.eye(M, dtype=wide)).astype(np.float64)
    return _ratio(np.tril(res), np.tril(gfac(M) * (np.abs(L) @ np.abs(Xh))))


# ---- indefinite inputs ---------------------------------------------------------------------------------------------------
def bad_pivot(name, M, k, j):
    """matrix k of the family with pivot j made negative (A[j,j] -= L[j,j]^2 (1 + 1e-3)); the earlier pivots are unchanged"""
    ref = reference(name, M, k)
    A = torch.from_numpy(ref.A.copy())
    A[j, j] -= float(ref.L[j, j]) ** 2 * (1 + 1e-3)
    return A


def want_info(A):
    """what LAPACK reports for the lower triangle of each matrix of the batch (0, or 1 + the first bad pivot)"""
    return torch.linalg.cholesky_ex(A).info.to(torch.int32)


def nan_above(A):
    """the same matrices with NaN in the strict upper triangle"""
    M = A.shape[-1]
    up = torch.triu(torch.ones(M, M, dtype=torch.bool), 1)
    return torch.where(up, torch.full_like(A, float("nan")), A).contiguous()


class GuardedInt:
    """fp64_products_util.Guarded for an int32 output (info): n elements inside a buffer pre-filled with ISENTINEL"""

    def __init__(self, n, dev):
        self.n, self.lo = int(n), PAD
        self.buf = torch.full((self.lo + self.n + PAD,), ISENTINEL, dtype=torch.int32, device=dev)
        self.view = self.buf[self.lo: self.lo + self.n]

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.buf[: self.lo] == ISENTINEL).all()) and bool((self.buf[self.lo + self.n:] == ISENTINEL).all())

    def untouched(self):
        return bool((self.buf == ISENTINEL).all())
