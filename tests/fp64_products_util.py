"""Helpers shared by tests/test_fp64_products_gpu.py, tests/test_fp64_products_shapes.py and test_longk_f64: the derived
bar, sentinel-guarded outputs, poisoned workspaces, and the shape lists (kept here so the non-GPU shape test and the GPU
tests cannot drift apart).

The bar, element by element (Higham, Accuracy and Stability of Numerical Algorithms, sec. 3.5: a length-K inner product in
any order errs by at most gamma_K |a|.|b|; + 4 for the alpha / beta scaling and the forming of an operand on the fly):

    |got - want| <= 2 (K + 4) u (|alpha| |A| |B| + |beta| |C0|)   [+ 2^-24 |want| for an fp32-stored result]

with u = 2^-53 (fp64 accumulation) or 2^-24 (the fp32 instantiation of gpsa_gemm).  The factor 2 covers the fp64 CPU
reference's own rounding and accumulation inside the matrix instruction, which is not documented as round-to-nearest.
"""
import ctypes as C

import torch

f64, f32 = torch.float64, torch.float32
U64, U32 = 2.0 ** -53, 2.0 ** -24
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
SENTINEL = -7777.25  # exact in fp32 and fp64
PAD = 64  # guard elements on either side of an output (64 * 4 bytes: the view stays 16-byte aligned)

# row counts (issue "Pin the fp64 product kernels ..."): ceil(M / 16) is rounded up to 2, 4, 7, 13, 16 (24: whiten only)
CLASS_FIRSTS = [1, 33, 65, 113, 209]
CLASS_LASTS = [32, 64, 112, 208, 256]
RAGGED = [17, 49, 100, 199, 241]
WHITEN_STREAMED = [257, 370, 384]
ROWS_256 = CLASS_FIRSTS + CLASS_LASTS + RAGGED
ROWS_WHITEN = ROWS_256 + WHITEN_STREAMED

# test_longk_f64 (tests/test_hip_batched.py): every shape must be taken by the kernel on 256 CUs
LONGK_SHAPES = [(200, 100000, 1), (200, 10048, 2), (25, 1030, 3), (100, 4098, 2), (256, 3074, 1), (200, 1282, 6),
                (50, 20000, 4)]
LONGK_MODES = ["G+dB/f32", "G+dB/f64", "dB/sym", "G"]
LONGK_NPROB = [1, 4, 48]

# gpsa_gemm: 25 (m, n, k) in which every listed value appears for each dimension
GEMM_MN = [1, 15, 16, 17, 31, 33, 63, 64, 65, 129]
GEMM_K = [1, 3, 4, 5, 15, 16, 17, 31, 33, 65]
GEMM_TRIPLES = [(1, 129, 1), (15, 65, 3), (16, 64, 4), (17, 63, 5), (31, 33, 15), (33, 31, 16), (63, 17, 17),
                (64, 16, 31), (65, 15, 33), (129, 1, 65), (1, 1, 4), (16, 16, 16), (17, 17, 1), (64, 64, 65),
                (65, 65, 5), (129, 129, 33), (15, 31, 17), (31, 15, 3), (63, 129, 16), (129, 63, 15), (33, 64, 31),
                (64, 33, 65), (1, 65, 33), (65, 1, 16), (33, 33, 4)]


def rnd(*shape, dtype=f64, seed=0):
    """seeded standard normals, drawn in fp64 and stored as dtype"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=f64).to(dtype)


def sym_inverse(M, seed, batch=None):
    """a symmetric stand-in for K_uu^-1 (R + R^T, as tests/test_hip_kernels.py builds it)"""
    R = rnd(*((M, M) if batch is None else (batch, M, M)), seed=seed)
    return (R + R.transpose(-1, -2)).contiguous()


def bar(K, absprod, u=U64, c0=None, beta=0.0, want32=None):
    """the bound above; absprod = |alpha| |A| |B| (fp64, CPU).  want32: the reference of an fp32-stored result"""
    b = absprod if c0 is None or beta == 0.0 else absprod + abs(beta) * c0.abs().double()
    b = 2.0 * (K + 4) * u * b
    return b if want32 is None else b + U32 * want32.abs()


def ratio(got, want, bound):
    """largest |got - want| / bound; an element whose bound is 0 must be exact.  NaN / inf in got -> inf"""
    got = got.double()  # compared where the result lives (the large panels stay on the device)
    want, bound = want.double().to(got.device), bound.double().to(got.device)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - want).abs()
    if bool(((bound <= 0) & (err > 0)).any()):
        return float("inf")
    r = err / bound.clamp_min(1e-300)
    return float(r.max()) if r.numel() else 0.0


class Guarded:
    """an output of n elements in the middle of a larger device buffer pre-filled with SENTINEL; ``off`` extra elements
    move the view off its 16-byte alignment (tests about alignment only)"""

    def __init__(self, n, dtype, dev, fill=SENTINEL, off=0):
        self.n, self.lo = int(n), PAD + off
        self.buf = torch.full((self.lo + self.n + PAD,), SENTINEL, dtype=dtype, device=dev)
        self.view = self.buf[self.lo: self.lo + self.n]
        if fill != SENTINEL:
            self.view.fill_(fill)
        assert off or self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.buf[: self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        """nothing was written at all (error returns)"""
        return bool((self.buf == SENTINEL).all())


def poisoned(nbytes, dev):
    """a fresh workspace of exactly nbytes, every byte 0xFF (NaN in either float type)"""
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=dev)


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def doubles(xs):
    return (C.c_double * len(xs))(*xs)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int64 if a.dtype == f64 else torch.int32),
        b.contiguous().view(torch.int64 if b.dtype == f64 else torch.int32))


def longk_k0(lib, M, nprob, limit=8192):
    """the smallest even K >= 512 the long-K kernel takes for nprob products, found by stepping the query"""
    for K in range(512, limit, 2):
        if int(lib.gpsa_longk_f64_workspace(M, K, nprob)) > 0:
            return K
    raise AssertionError(f"no K below {limit} is taken at M = {M}, nprob = {nprob}")


def whiten_threshold_columns(cus):
    """A2: both sides of row-split / resident (32 columns per workgroup) and of resident / streaming (64)"""
    return [32 * cus - 31, 32 * cus, 32 * cus + 1, 64 * cus, 64 * cus + 1]


def persistent_c0(cus, batch=1):
    """A3: the shortest panel whose batch * ceil(C / 64) column tiles reach 6 per CU (last tile one column wide)"""
    assert (6 * cus) % batch == 0
    return 64 * (6 * cus // batch - 1) + 1
