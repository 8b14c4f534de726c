"""Shape lists, references and bounds of tests/test_mm_stage_gpu.py and tests/test_mm_stage_shapes.py: the kernels that
build a step's M x M stage - the covariance matrices and their backward (csrc/kmat.hip), Omega = A A^T + jitter I and its
adjoint (csrc/gemm.hip, csrc/qf_big.hip), the KL terms (csrc/kl.hip).  The guards (Guarded, poisoned, same_bits, ratio,
bar, SENTINEL) are those of tests/fp64_products_util.py.

References.  The covariance family is evaluated in numpy.longdouble (64-bit mantissa here, asserted below: its own error
is 2^-11 of an fp64 kernel's) from the explicit formulas of csrc/kmat_cov.hpp - the 1e-10 inside the Matern square root,
the 0.5 factor of matern12 - in column chunks, never through autograd.  Omega and KL references are fp64 torch on the CPU.

Bounds.  Every bound is derived from the arithmetic the kernel is written in, first order in the unit roundoff u (2^-53,
or 2^-24 for the fp32 instantiation) with a factor HIGHER = 1.01 for the terms of higher order, and checked element by
element.  ASSUMPTION (no ROCm math accuracy table is installed with the toolchain the tests run on): exp errs by at most
2 ulp, sqrt and divide by at most 1 ulp; 1 ulp is 2 u relative, a plain +, -, * is 1 u.  Inputs are exact in the type the
kernel computes in (fp32 widened to fp64, or read as they are).

  ell = exp(ls): 4 u; 1 / ell: 6 u; var = exp(lv): 4 u.
  rbf       u_d = (z_d - x_d) / ell: 8 u; s = sum u_d^2: (16 + D) u; a = s / 2 is the exponent's argument, so its relative
            error delta = (16 + D) u becomes a delta in exp.  k = var exp(-a): (9 + a (16 + D)) u.
            cd = -k / ell^2: + 14;   pl = k s: + 17 + D.
  Matern    s = sum (z_d - x_d)^2: (2 + D) u; dist = sqrt(s + 1e-10): at most n_dist = (4 + D) u.
  matern12  a = dist / (2 ell): (n_dist + 7) u.  k = var exp(-a): (9 + a (n_dist + 7)) u.
            cd = -k / (2 ell dist): + 9 + n_dist;   pl = k dist / (2 ell): + 8 + n_dist.
  matern32  a = zz = sqrt(3) dist / ell: n_zz = (n_dist + 9) u.  e = var exp(-zz): c_e = (9 + a n_zz) u.
            k = (1 + zz) e: c_e + n_zz + 2;   cd = -3 e / ell^2: c_e + 15;   pl = e zz^2: c_e + 2 n_zz + 2.

So a covariance entry is within (c_fn + a n_a) u |k| (c_fn: the function calls and roundings outside the exponent, n_a u:
the relative error of the argument), plus |jitter| u on the diagonal.  A backward sum of n terms, each a product of the
gradient panel, one coefficient above and at most two more roundings (three more when the panel comes in two pieces), is
within  u sum_i (n + c_i) |term_i|  in whatever order it is added, plus 2^-24 |want| where the gradient is stored as fp32.
The references return these weighted absolute sums next to the values.

  Omega forward   bar(M, |A| |A|^T + |jitter| I)
  Omega adjoint   bar(M, 2 |G| |A|)  or  bar(M, (|G| + |G^T|) |A|),  plus 2^-24 |want|
  KL forward      bar(M M + M, sum |Kinv o Omega| + sum |KD o d|) + u (|logdet_p| + |logdet_o| + M)
  KD              bar(M, |Kinv| |d|)
  KL backward     dOmega: 4 u (|old| + 0.5 |g| (|Kinv| + |Oinv|));   dD: 2 u |want|
                  S: bar(n_group, |gs| |K| + sum |g| (|Omega| + |d_i d_j|))       (g > 0 in these tests)

Inputs: points in the unit box, lengthscale about exp(-0.7), variance about exp(0.3): the largest exponent argument is
0.5 D exp(1.4) = 8.2 for rbf at D = 4, sqrt(3 D) exp(0.7) = 7 for matern32 and a quarter of that for matern12; every test
asserts a_max <= 20 from its reference (tests/test_mm_stage_shapes.py checks the box on the CPU).
"""
import numpy as np
import torch

from fp64_products_util import U32, U64, bar, f32, f64, rnd  # noqa: F401  (re-exported with the guards)

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the covariance references need a 64-bit mantissa"
HIGHER = 1.01
A_MAX = 20.0
KINDS = {"rbf": 0, "matern12": 1, "matern32": 2}
LS, LV = -0.7, 0.3
JITTER = 1e-5
CUS = 256
KM_MAXB = 16

# ---- A. covariance forward -------------------------------------------------------------------------------------------
FWD_M = [1, 15, 16, 17, 33]
FWD_C = [1, 255, 256, 257, 513]
FWD_D = [1, 2, 3, 4]
# (dtype, in_dtype) codes of gpsa_kmat -> (storage of Z / parameters, storage of X, type of K)
FWD_TYPES = {"f32/f32": (0, 0, f32, f32, f32), "f64/f64": (1, 1, f64, f64, f64), "f64/f32": (1, 0, f32, f32, f64),
             "f64/f32_x64": (1, 2, f32, f64, f64)}
FWD_BATCHED = [(17, 513, 2), (16, 257, 3), (33, 513, 1)]  # (M, C, D); batch 4


def fwd_n_live(C):
    return sorted({0, 1, 255, 256, 257, C} & set(range(C + 1)))


# ---- B. covariance backward ------------------------------------------------------------------------------------------
# generic kernel (D != 2); the three long shapes straddle kb_rows()'s threshold cdiv(C, 256) cdiv(M, 32) >= 1024
GEN_BELOW = (40, 130560)  # 510 x 2 = 1020: 8-row chunks
GEN_ABOVE = (40, 130817)  # 512 x 2 = 1024: 32-row chunks, one full and one of 8
GEN_WALK = (9, 262401)  # 1026 column blocks over KB_MAXBX = 1024 workgroups; the last block holds one column
GEN_SMALL = (200, 777)
GEN_D = [1, 3, 4]
# gpsa_kmat_bwd's (dtype, in_dtype) -> (storage of inputs, arithmetic, storage of gradients, storage of Kbar)
BWD_MODES = {"f32": (0, 0, f32, f32, f32, f32), "f64": (1, 1, f64, f64, f64, f64), "f64/f32": (1, 0, f32, f64, f32, f64),
             "out64": (1, 3, f32, f64, f64, f64), "acc64": (1, 4, f32, f64, f64, f32)}
X64_ENTRIES = ["x64", "x64_axpy", "x64_f64", "x64_f64_axpy"]  # fp32 Z, fp64 X; Kbar fp32 / fp32 / fp64 / fp64
# (shape, D, kind, entry, two-piece panel, dX requested): every long shape with every D, kind and entry rotating
GEN_LONG_CASES = [
    (GEN_BELOW, 1, "rbf", "x64", False, True), (GEN_BELOW, 3, "matern12", "out64", False, True),
    (GEN_BELOW, 4, "matern32", "x64_f64", False, True),
    (GEN_ABOVE, 1, "matern32", "acc64", False, True), (GEN_ABOVE, 3, "rbf", "x64_f64_axpy", True, True),
    (GEN_ABOVE, 4, "matern12", "x64_axpy", True, False),
    (GEN_WALK, 1, "matern12", "f64", False, True), (GEN_WALK, 3, "matern32", "x64_axpy", True, True),
    (GEN_WALK, 4, "rbf", "f64/f32", False, False),
]
D2_M = [1, 16, 17, 33, 49, 200, 257]
D2_C = 777
D2_PER = (200, 10241)  # 41 column blocks x 13 row chunks = 533 > 512 slots: two blocks per workgroup
D2_FINISH = (16, 12545)  # 50 column blocks x 1 row chunk: nbx = 50 >= 49, the finish kernel's unrolled loop
D2_SAME = [17, 200]
BATCHED_B = [1, 3, 16]
BATCHED_SHAPES = [(33, 513, 3), (17, 513, 2)]  # (M, C, D)


def bwd_n_live(C, B):
    """ragged live counts: 0, a block edge, C, then in between"""
    base = [0, 256, C, 1, 257, C - 1, 255]
    return [base[b % len(base)] for b in range(B)] if B > 1 else [256]


def kb_rows(M, C):
    """csrc/kmat.hip, kb_rows(), restated"""
    return 8 if -(-C // 256) * -(-M // 32) < 1024 else 32


def row_chunks_from_workspace(nbytes, esize, M, C, D):
    """the row chunks gpsa_kmat_bwd_workspace counted: bytes / esize = nbx M D + nby C D + 2 nbx nby"""
    nbx = -(-C // 256)
    num, den = nbytes // esize - nbx * M * D, C * D + 2 * nbx
    assert nbytes % esize == 0 and num % den == 0, (nbytes, M, C, D)
    return num // den


def d2_grid(M, C, batch=1, cus=CUS):
    """(per, nbx, nby, rows) of the D = 2 launcher (csrc/kmat.hip, kmat_bwd_launch)"""
    ncb, nby = -(-C // 256), -(-M // 16)
    per = 1
    while per < ncb and -(-ncb // per) * nby * batch > 2 * cus:
        per += 1
    return per, -(-ncb // per), nby, -(-M // nby)


# ---- C. Omega --------------------------------------------------------------------------------------------------------
OMEGA_DMA = [16, 20, 28, 60, 64, 68, 124, 128, 132, 200, 252, 256, 260]
OMEGA_GENERIC = [1, 3, 15, 17, 18, 63, 65, 130, 201, 233]
OMEGA_SEGMENTS = [(1, 0), (3, 0), (2, 3), (1, 1)]
OMEGA_OFFSET_M = [20, 64, 200]  # DMA-eligible sizes run with a pointer one element off its 16-byte alignment
OMEGA_JITTER = 0.375


def omega_dma(M, aligned=True):
    """the predicate of omega_fwd_dma_launch / omega_bwd_dma_launch (csrc/qf_big.hip), restated"""
    return M % 4 == 0 and M >= 16 and aligned


# ---- D. KL -----------------------------------------------------------------------------------------------------------
KL_SLICED_M = [1, 15, 16, 17, 63, 64, 65, 128, 129, 255, 256, 257, 449, 512, 513]
KL_SLICES = {1: 1, 64: 1, 65: 2, 128: 2, 129: 3, 448: 7, 449: 8, 1000: 8}
KL_BWD_M = [1, 15, 16, 17, 200, 257]
KL_GROUPS = [0, 1, 7, 8, 9, 17]
KL_ABSENT = [0, 2]
KL_PLAIN_M = [1, 31, 32, 33, 257]
KL_PLAIN_L = [1, 3]


def kl_slices(M):
    """csrc/kl.hip, mvn_kl_grouped_fwd_slices(), restated"""
    return min(-(-M // 64), 8) if M > 64 else 1


# ------------------------------------------------------------------------------------------------------------------------
# covariance references
# ------------------------------------------------------------------------------------------------------------------------
def points(n, D, dtype, seed):
    """n points in the unit box, drawn in fp64 and stored as dtype"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, D, generator=g, dtype=f64).to(dtype)


def hyper(dtype, n=1, seed=0):
    """(log lengthscale, log variance) [n] each, a little apart per problem"""
    g = torch.Generator().manual_seed(9000 + seed)
    j = 0.05 * torch.rand(2, n, generator=g, dtype=f64)
    return (LS + j[0]).to(dtype), (LV + j[1]).to(dtype)


def _ld(t):
    return t.detach().cpu().double().numpy().astype(LD)


def cov_terms(kind, Z, X, ls, lv):
    """k, cd, pl (longdouble, [M, c]) and a, c_k, c_cd, c_pl (float64: the exponent's argument and the three
    error counts in units of u) for X's columns; Z [M, D], X [c, D] longdouble, ls / lv python floats as stored"""
    D = Z.shape[1]
    ell, var = np.exp(LD(ls)), np.exp(LD(lv))
    diff = Z[:, None, :] - X[None, :, :]
    if kind == "rbf":
        s = ((diff / ell) ** 2).sum(-1)
        a = (LD(0.5) * s).astype(np.float64)
        k = var * np.exp(LD(-0.5) * s)
        ck = 9.0 + a * (16 + D)
        return k, -k / (ell * ell), k * s, a, ck, ck + 14.0, ck + 17.0 + D
    nd = 4.0 + D
    dist = np.sqrt((diff ** 2).sum(-1) + LD(1e-10))
    if kind == "matern12":
        arg = LD(0.5) * dist / ell
        a = arg.astype(np.float64)
        k = var * np.exp(-arg)
        ck = 9.0 + a * (nd + 7)
        return k, LD(-0.5) * k / (ell * dist), LD(0.5) * k * dist / ell, a, ck, ck + 9.0 + nd, ck + 8.0 + nd
    assert kind == "matern32"
    zz = LD(1.7320508075688772) * dist / ell
    a, nzz = zz.astype(np.float64), nd + 9.0
    e = var * np.exp(-zz)
    ce = 9.0 + a * nzz
    return (1 + zz) * e, LD(-3) * e / (ell * ell), e * zz * zz, a, ce + nzz + 2.0, ce + 15.0, ce + 2 * nzz + 2.0


def cov_fwd_ref(kind, Z, X, ls, lv, jitter=0.0, u=U64, n_live=None):
    """(K, bound, a_max) as fp64 torch [M, C]; columns from n_live on are exact zeros"""
    M, C = Z.shape[0], X.shape[0]
    live = C if n_live is None else int(n_live)
    K, B, amax = np.zeros((M, C)), np.zeros((M, C)), 0.0
    if live:
        k, _, _, a, ck, _, _ = cov_terms(kind, _ld(Z), _ld(X[:live]), float(ls), float(lv))
        bound = HIGHER * u * ck * np.abs(k).astype(np.float64)
        n = min(M, live)
        k[np.arange(n), np.arange(n)] += LD(jitter)
        bound[np.arange(n), np.arange(n)] += HIGHER * u * abs(jitter)
        K[:, :live], B[:, :live], amax = k.astype(np.float64), bound, float(a.max())
    return torch.from_numpy(K), torch.from_numpy(B), amax


def cov_bwd_ref(kind, Z, X, ls, lv, Kbar, same=False, axX=None, axd=None, axs=0.0, n_live=None, u=U64, store32=False,
                chunk=8192):
    """the backward sums and their bounds, in column chunks: dict of fp64 torch tensors dZ [M, D], dX [C, D], dpar [2]
    and bZ, bX, bpar, plus a_max.  Kbar [M, C] (and the optional second piece axs * axd[c] * axX[m, c]) as stored;
    same: the X-side sums are folded into dZ (gz + gx) as the K_uu form does."""
    M, D = Z.shape
    C = X.shape[0]
    live = C if n_live is None else int(n_live)
    two = axX is not None
    Zl = _ld(Z)
    gz, gx, gp = np.zeros((M, D), LD), np.zeros((C, D), LD), np.zeros(2, LD)
    bz, bx, bp = np.zeros((M, D)), np.zeros((C, D)), np.zeros(2)
    amax = 0.0
    extra = 3.0 if two else 0.0
    nz, nx, npar = float(live + (M if same else 0)), float(M + (C if same else 0)), float(M) * live
    for c0 in range(0, live, chunk):
        c1 = min(live, c0 + chunk)
        Xl = _ld(X[c0:c1])
        k, cd, pl, a, ck, ccd, cpl = cov_terms(kind, Zl, Xl, float(ls), float(lv))
        amax = max(amax, float(a.max()))
        kb = _ld(Kbar[:, c0:c1])
        kabs = np.abs(kb).astype(np.float64)
        if two:
            piece = LD(float(np.float32(axs))) * _ld(axd[c0:c1])[None, :] * _ld(axX[:, c0:c1])
            kb = kb + piece
            kabs = kabs + np.abs(piece).astype(np.float64)
        w = kb * cd
        wabs = kabs * np.abs(cd).astype(np.float64)
        diff = Zl[:, None, :] - Xl[None, :, :]
        t = w[:, :, None] * diff
        tabs = wabs[:, :, None] * np.abs(diff).astype(np.float64)
        cz = (ccd + 3.0 + extra)[:, :, None]
        gz += t.sum(1)
        gx[c0:c1] -= t.sum(0)
        bz += ((nz + cz) * tabs).sum(1)
        bx[c0:c1] += ((nx + cz) * tabs).sum(0)
        gp[0] += (kb * pl).sum()
        gp[1] += (kb * k).sum()
        bp[0] += ((npar + cpl + 1.0 + extra) * kabs * np.abs(pl).astype(np.float64)).sum()
        bp[1] += ((npar + ck + 1.0 + extra) * kabs * np.abs(k).astype(np.float64)).sum()
    if same:
        assert M == C
        gz, bz = gz + gx, bz + bx
    out = {"dZ": gz, "dX": gx, "dpar": gp}
    out = {n: torch.from_numpy(v.astype(np.float64)) for n, v in out.items()}
    for n, b in (("bZ", bz), ("bX", bx), ("bpar", bp)):
        want = out["d" + n[1:]]
        out[n] = torch.from_numpy(HIGHER * u * b) + (U32 * want.abs() if store32 else 0.0)
    out["a_max"] = amax
    return out


# ------------------------------------------------------------------------------------------------------------------------
# Omega and KL references (fp64 torch, CPU)
# ------------------------------------------------------------------------------------------------------------------------
def omega_fwd_ref(A, jitter):
    """A [n, M, M] fp32 -> (want, bound)"""
    Ad = A.double()
    M = A.shape[-1]
    eye = torch.eye(M, dtype=f64)
    return Ad @ Ad.transpose(-1, -2) + jitter * eye, bar(M, Ad.abs() @ Ad.abs().transpose(-1, -2) + abs(jitter) * eye)


def omega_bwd_ref(G, A, symmetric):
    Ad = A.double()
    M = A.shape[-1]
    if symmetric:
        want, ab = 2.0 * (G @ Ad), 2.0 * (G.abs() @ Ad.abs())
    else:
        want, ab = (G + G.transpose(-1, -2)) @ Ad, (G.abs() + G.abs().transpose(-1, -2)) @ Ad.abs()
    return want, bar(M, ab, want32=want)


def spd_batch(n, M, seed):
    """n well-conditioned symmetric positive definite matrices with their CPU inverses and log-determinants"""
    R = rnd(n, M, M, seed=seed)
    mats = R @ R.transpose(-1, -2) / M + torch.eye(M, dtype=f64)
    mats = 0.5 * (mats + mats.transpose(-1, -2))
    inv = torch.linalg.inv(mats)
    return mats.contiguous(), (0.5 * (inv + inv.transpose(-1, -2))).contiguous(), torch.logdet(mats).contiguous()


def kl_fwd_ref(Kinv, ldp, Om, ldo, d, KD=None):
    """one term -> (kl, its bound, KD, KD's bound); KD given: the plain entry reads it as an input"""
    M = d.shape[0]
    kd = Kinv @ d if KD is None else KD
    s1, s2 = (Kinv * Om).sum(), (kd * d).sum()
    a1, a2 = (Kinv * Om).abs().sum(), (kd * d).abs().sum()
    kl = 0.5 * (ldp - ldo + s1 + s2 - M)
    bound = bar(M * M + M, a1 + a2) + U64 * (ldp.abs() + ldo.abs() + M)
    return kl, bound, kd, bar(M, Kinv.abs() @ d.abs())
