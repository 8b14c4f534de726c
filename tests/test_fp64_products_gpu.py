"""The fp64 matrix-core product kernels through the C ABI alone, against the same operation in fp64 on the CPU, at the
edges of their row-tile classes, dispatch thresholds and layouts:

  A. the projection alpha = K^-1 K_uf (csrc/whiten.hip, csrc/proj64.hip);
  B. the long-K square products (csrc/longk64.hip);
  C. gemm_mfma_kernel (csrc/gemm.hip) and what rests on it.

Bar (tests/fp64_products_util.py, derived and not measured): element by element
    |got - want| <= 2 (K + 4) u (|alpha| |A| |B| + |beta| |C0|)  [+ 2^-24 |want| for an fp32-stored result],
u = 2^-53, or 2^-24 for the fp32 instantiation of gpsa_gemm; K = 2 M for q and for the quadratic form v.  Every test
prints the largest ratio of error to bound next to its shape and asserts <= 1.

Guards in every test: each output is a view into the middle of a larger buffer filled with a sentinel, which must be
intact on both sides afterwards; each workspace is a fresh buffer of exactly the queried size filled with 0xFF bytes, and
the result must be NaN-free; each call runs twice and the two results must be equal bit for bit.  No test here skips:
the shape lists are chosen so that the kernel named takes them (tests/test_fp64_products_shapes.py holds the lists to
that without a GPU), and the query is asserted before comparing.  Which kernel ran cannot be observed from here: the
threshold shapes are chosen by reading the launchers ("fp64 product tests").
"""
import functools

import pytest
import torch

import fp64_products_util as fu
from fake_ops import FakeOps
from fp64_products_util import (EINVAL, EUNSUPPORTED, EWORKSPACE, SENTINEL, U32, U64, Guarded, bar, f32, f64, poisoned,
                                ratio, rnd, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CODE = {f32: 0, f64: 1}  # GPSA_F32 / GPSA_F64
KIND = {"rbf": 0, "matern12": 1, "matern32": 2}
FK = FakeOps()


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    return _lib.load()


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def note(family, what, r):
    print(f"[fp64-products] {family}: {what}: error / bound {r:.3f}")
    return r


def p(t):
    return 0 if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------
# A. the projection family
# ------------------------------------------------------------------------------------------------------------------------
def _whiten_ref(M, C, in_dt, batch=None):
    """(Kinv, X, want, |Kinv| |X|, q, its abs form) on the CPU in fp64, from the inputs as stored"""
    Kinv = fu.sym_inverse(M, seed=1000 + M, batch=batch)
    X = rnd(*((M, C) if batch is None else (batch, M, C)), dtype=in_dt, seed=2000 + M + C % 1000)
    Xw = X.double()
    want, ab = Kinv @ Xw, Kinv.abs() @ Xw.abs()
    return Kinv, X, want, ab, (Xw * want).sum(-2), (Xw.abs() * ab).sum(-2)


_whiten_ref_small = functools.lru_cache(maxsize=8)(_whiten_ref)


def _check_whiten(family, what, M, outs, want, ab, qwant, qab, out_dt):
    """outs: the two repetitions' (alpha, q or None) on the device"""
    (a0, q0), (a1, q1) = outs
    assert same_bits(a0, a1) and (q0 is None or same_bits(q0, q1)), f"{what}: not repeatable"
    r = note(family, what, ratio(a0, want.reshape(a0.shape), bar(M, ab.reshape(a0.shape),
                                                                  want32=want.reshape(a0.shape) if out_dt == f32 else None)))
    assert r <= 1, (what, r)
    if q0 is not None:
        rq = note(family, what + " q", ratio(q0, qwant.reshape(q0.shape), bar(2 * M, qab.reshape(q0.shape))))
        assert rq <= 1, (what, rq)
        r = max(r, rq)
    return r


def _run_whiten(lib, M, C, Kd, Xd, in_dt, out_dt, want_q):
    outs = []
    for _ in range(2):
        out, q = Guarded(M * C, out_dt, DEV), (Guarded(C, f64, DEV) if want_q else None)  # q pre-filled with the sentinel
        wsb = int(lib.gpsa_whiten_workspace(M))
        assert wsb > 0
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_whiten_f64(p(Kd), CODE[in_dt], p(Xd), M, C, CODE[out_dt], out.ptr(), q.ptr() if q else 0, p(ws),
                                 wsb, stream())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() and (q is None or q.intact()), (M, C, rc)
        outs.append((out.view, q.view if q else None))
    return outs


@pytest.mark.parametrize("M", fu.ROWS_WHITEN)
def test_whiten_rows(lib, M):
    """A1: gpsa_whiten_f64 at every class first / last / ragged row count, all four type pairs, with q (resident or
    row-split kernel) and without (streaming kernel)"""
    for C in (260, 263):
        for in_dt in (f64, f32):
            Kinv, X, want, ab, qw, qab = _whiten_ref_small(M, C, in_dt)
            Kd, Xd = Kinv.to(DEV), X.to(DEV)
            for out_dt in (f64, f32):
                for want_q in (True, False):
                    outs = _run_whiten(lib, M, C, Kd, Xd, in_dt, out_dt, want_q)
                    _check_whiten("whiten", f"whiten_f64 M={M} C={C} {in_dt}->{out_dt} q={want_q}", M, outs, want, ab, qw,
                                  qab, out_dt)


def _run_dual(lib, M, C, Kd, Xd, reuse=True):
    """gpsa_whiten_f64_dual twice (fresh poisoned workspace each), each followed by a Kinv == NULL call on the same
    workspace -> [(a64, q)] x 2 after asserting alpha32 == alpha64.float() and the reuse call's bits"""
    outs = []
    wsb = int(lib.gpsa_whiten_workspace(M))
    assert wsb > 0
    for _ in range(2):
        ws = poisoned(wsb, DEV)
        got = []
        for kinv in ((Kd, None) if reuse else (Kd,)):
            a64, a32, q = Guarded(M * C, f64, DEV), Guarded(M * C, f32, DEV), Guarded(C, f64, DEV)
            rc = lib.gpsa_whiten_f64_dual(p(kinv), p(Xd), M, C, a64.ptr(), a32.ptr(), q.ptr(), p(ws), wsb, stream())
            torch.cuda.synchronize()
            assert rc == 0 and a64.intact() and a32.intact() and q.intact(), (M, C, rc)
            assert same_bits(a32.view, a64.view.float()), f"dual M={M} C={C}: alpha32 is not alpha64 rounded"
            got.append((a64.view, q.view))
        if reuse:
            assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1]), f"dual M={M} C={C}: Kinv == NULL"
        outs.append(got[0])
        del got
    return outs


@pytest.mark.parametrize("M", fu.ROWS_WHITEN)
def test_whiten_dual_rows(lib, M):
    for C in (260, 263):
        Kinv, X, want, ab, qw, qab = _whiten_ref_small(M, C, f64)
        outs = _run_dual(lib, M, C, Kinv.to(DEV), X.to(DEV))
        _check_whiten("whiten", f"whiten_f64_dual M={M} C={C}", M, outs, want, ab, qw, qab, f64)


@pytest.mark.parametrize("M", fu.ROWS_WHITEN)
def test_whiten_axpy_rows(lib, M):
    """out = Kinv X + s d o X2 (fp32 panels, fp64 arithmetic): the bar with s d o X2 as its beta C0 term, plus the fp32
    rounding of the result"""
    s = 2.0
    for C in (260, 263):
        Kinv, X, want, ab, _, _ = _whiten_ref_small(M, C, f32)
        X2, d = rnd(M, C, dtype=f32, seed=31 + M), rnd(C, dtype=f32, seed=32 + M)
        upd = s * d.double()[None, :] * X2.double()
        want = want + upd
        bound = bar(M, ab, c0=upd, beta=1.0, want32=want)
        Kd, Xd, X2d, dd = Kinv.to(DEV), X.to(DEV), X2.to(DEV), d.to(DEV)
        outs = []
        for _ in range(2):
            out = Guarded(M * C, f32, DEV)
            wsb = int(lib.gpsa_whiten_workspace(M))
            ws = poisoned(wsb, DEV)
            rc = lib.gpsa_whiten_axpy_f32(p(Kd), p(Xd), M, C, p(X2d), p(dd), s, out.ptr(), p(ws), wsb, stream())
            torch.cuda.synchronize()
            assert rc == 0 and wsb > 0 and out.intact()
            outs.append(out.view.view(M, C))
        assert same_bits(outs[0], outs[1])
        r = note("whiten", f"whiten_axpy_f32 M={M} C={C}", ratio(outs[0], want, bound))
        assert r <= 1, (M, C, r)


def _run_batched(lib, M, C, B, Kd, Xd):
    outs = []
    wsb = int(lib.gpsa_whiten_workspace(M)) * B
    assert wsb > 0
    for _ in range(2):
        out, q = Guarded(B * M * C, f64, DEV), Guarded(B * C, f64, DEV)
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_whiten_batched_f64(p(Kd), M * M, p(Xd), M, C, M * C, out.ptr(), q.ptr(), B, p(ws), wsb, stream())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact() and q.intact(), (M, C, B, rc)
        outs.append((out.view.view(B, M, C), q.view.view(B, C)))
    return outs


@pytest.mark.parametrize("M", fu.ROWS_WHITEN)
def test_whiten_batched_rows(lib, M):
    for C in (260, 263):
        Kinv, X, want, ab, qw, qab = _whiten_ref(M, C, f64, batch=3)  # a different inverse per problem
        outs = _run_batched(lib, M, C, 3, Kinv.to(DEV), X.to(DEV))
        _check_whiten("whiten", f"whiten_batched_f64 M={M} C={C} batch=3", M, outs, want, ab, qw, qab, f64)


def test_whiten_declines_385_rows(lib):
    """M = 385 is one row past the streamed class: GPSA_EUNSUPPORTED from every entry, nothing written"""
    M, C = 385, 260
    assert int(lib.gpsa_whiten_workspace(M)) == 0
    Kd, Xd, X32 = fu.sym_inverse(M, 1).to(DEV), rnd(M, C, seed=2).to(DEV), rnd(M, C, dtype=f32, seed=2).to(DEV)
    dd = rnd(C, dtype=f32, seed=3).to(DEV)
    Z, ls = rnd(M, 2, dtype=f32, seed=4).to(DEV), torch.tensor([0.3], device=DEV)
    X64 = rnd(C, 2, seed=5).to(DEV)
    ws = poisoned(1 << 20, DEV)
    a, a32, q = Guarded(M * C, f64, DEV), Guarded(M * C, f32, DEV), Guarded(C, f64, DEV)
    st = stream()
    rcs = [lib.gpsa_whiten_f64(p(Kd), 1, p(Xd), M, C, 1, a.ptr(), q.ptr(), p(ws), ws.numel(), st),
           lib.gpsa_whiten_f64(p(Kd), 0, p(X32), M, C, 0, a32.ptr(), q.ptr(), p(ws), ws.numel(), st),
           lib.gpsa_whiten_f64_dual(p(Kd), p(Xd), M, C, a.ptr(), a32.ptr(), q.ptr(), p(ws), ws.numel(), st),
           lib.gpsa_whiten_axpy_f32(p(Kd), p(X32), M, C, p(X32), p(dd), 2.0, a32.ptr(), p(ws), ws.numel(), st),
           lib.gpsa_whiten_batched_f64(p(Kd), 0, p(Xd), M, C, 0, a.ptr(), q.ptr(), 1, p(ws), ws.numel(), st),
           lib.gpsa_whiten_gen_f64_dual(p(Kd), 0, p(Z), p(X64), 2, p(ls), p(ls), M, C, a.ptr(), a32.ptr(), q.ptr(), p(ws),
                                        ws.numel(), st)]
    torch.cuda.synchronize()
    assert rcs == [EUNSUPPORTED] * 6, rcs
    assert a.untouched() and a32.untouched() and q.untouched() and bool((ws == 0xFF).all())


@pytest.mark.parametrize("M", [20, 49, 100, 199, 241])
def test_whiten_dispatch_thresholds(lib, M):
    """A2: q wanted, the column counts on both sides of row-split / resident (ceil(C / 32) = CUs) and of resident /
    streaming (ceil(C / 64) = CUs); M = 20's class has no row-split kernel"""
    for C in fu.whiten_threshold_columns(cus()):
        for in_dt, out_dt in ((f64, f64), (f32, f32)):
            Kinv, X, want, ab, qw, qab = _whiten_ref(M, C, in_dt)
            outs = _run_whiten(lib, M, C, Kinv.to(DEV), X.to(DEV), in_dt, out_dt, True)
            _check_whiten("whiten", f"threshold whiten_f64 M={M} C={C} {in_dt}->{out_dt}", M, outs, want, ab, qw, qab,
                          out_dt)


@pytest.mark.parametrize("M", [20, 49, 100, 199, 241])
def test_whiten_batched_dispatch_threshold(lib, M):
    """A2, batch = 3: the longest panel whose ceil(C / 32) * 3 workgroups still fit the CUs (CUs need not be a multiple of
    3: the last C with ceil(C / 32) = CUs // 3), and 32 columns more"""
    C0 = 32 * (cus() // 3)
    for C in (C0, C0 + 32):
        Kinv, X, want, ab, qw, qab = _whiten_ref(M, C, f64, batch=3)
        outs = _run_batched(lib, M, C, 3, Kinv.to(DEV), X.to(DEV))
        _check_whiten("whiten", f"threshold whiten_batched_f64 M={M} C={C} batch=3", M, outs, want, ab, qw, qab, f64)


A3_ROWS = [65, 112, 113, 208]


@pytest.mark.parametrize("side", ["streaming", "persistent"])
@pytest.mark.parametrize("in_dt", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", A3_ROWS)
def test_whiten_persistent_threshold(lib, M, in_dt, side):
    """A3: C0 = 64 (6 CUs - 1) + 1 is the shortest panel the persistent kernel takes (its last tile one column wide);
    C0 - 1 stays with the streaming kernel.  fp64 output from either input type, and the dual store on the fp64 panel"""
    C = fu.persistent_c0(cus()) - (side == "streaming")
    Kinv, X, want, ab, qw, qab = _whiten_ref(M, C, in_dt)
    Kd, Xd = Kinv.to(DEV), X.to(DEV)
    want, ab = want.to(DEV), ab.to(DEV)
    outs = _run_whiten(lib, M, C, Kd, Xd, in_dt, f64, True)
    _check_whiten("proj64", f"{side} whiten_f64 M={M} C={C} {in_dt}->f64", M, outs, want, ab, qw, qab, f64)
    del outs
    if in_dt == f64:
        outs = _run_dual(lib, M, C, Kd, Xd)  # (Kinv == NULL: the persistent kernel then zeroes q itself)
        _check_whiten("proj64", f"{side} whiten_f64_dual M={M} C={C}", M, outs, want, ab, qw, qab, f64)
        del outs
    del Kd, Xd, want, ab
    torch.cuda.empty_cache()


@pytest.mark.parametrize("side", ["streaming", "persistent"])
@pytest.mark.parametrize("M", A3_ROWS)
def test_whiten_batched_persistent_threshold(lib, M, side):
    """A3, batch = 2: the same threshold in column tiles, 2 ceil(C / 64) = 6 CUs, at half the panel length"""
    C = fu.persistent_c0(cus(), batch=2) - (side == "streaming")
    Kinv, X, want, ab, qw, qab = _whiten_ref(M, C, f64, batch=2)
    outs = _run_batched(lib, M, C, 2, Kinv.to(DEV), X.to(DEV))
    _check_whiten("proj64", f"{side} whiten_batched_f64 M={M} C={C} batch=2", M, outs, want.to(DEV), ab.to(DEV), qw, qab,
                  f64)
    del outs
    torch.cuda.empty_cache()


def _gen_call(lib, Kd, kind, Z, X64, D, ls, var, M, C, a64, a32, q, ws):
    return lib.gpsa_whiten_gen_f64_dual(p(Kd), KIND[kind], p(Z), p(X64), D, p(ls), p(var), M, C, a64.ptr(), a32.ptr(),
                                        q.ptr(), p(ws), ws.numel(), stream())


@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("kind", ["rbf", "matern12", "matern32"])
def test_whiten_gen_at_the_persistent_threshold(lib, kind, D):
    """gpsa_whiten_gen_f64_dual (K_uf formed inside the persistent kernel) at M = 113 and C0, against the fp64 CPU
    reference built from FakeOps.kmat; C0 - 1 is declined with nothing written"""
    M, C = 113, fu.persistent_c0(cus())
    Z, X64 = rnd(M, D, dtype=f32, seed=40 + D), rnd(C, D, seed=41 + D)
    ls, var = torch.tensor([0.3], dtype=f32), torch.tensor([-0.2], dtype=f32)
    Kinv = fu.sym_inverse(M, seed=42)
    Kuf = FK.kmat(kind, Z.double(), X64, ls.double(), var.double())
    want, ab = (Kinv @ Kuf).to(DEV), (Kinv.abs() @ Kuf.abs()).to(DEV)
    qw, qab = (Kuf * want.cpu()).sum(0), (Kuf.abs() * ab.cpu()).sum(0)
    Kd, Zd, Xd, lsd, vd = Kinv.to(DEV), Z.to(DEV), X64.to(DEV), ls.to(DEV), var.to(DEV)
    wsb = int(lib.gpsa_whiten_workspace(M))
    outs = []
    for _ in range(2):
        a64, a32, q, ws = Guarded(M * C, f64, DEV), Guarded(M * C, f32, DEV), Guarded(C, f64, DEV), poisoned(wsb, DEV)
        rc = _gen_call(lib, Kd, kind, Zd, Xd, D, lsd, vd, M, C, a64, a32, q, ws)
        torch.cuda.synchronize()
        assert rc == 0 and a64.intact() and a32.intact() and q.intact()
        assert same_bits(a32.view, a64.view.float())
        outs.append((a64.view, q.view))
    _check_whiten("proj64", f"whiten_gen_f64_dual {kind} D={D} M={M} C={C}", M, outs, want, ab, qw, qab, f64)
    del outs
    a64, a32, q, ws = Guarded(M * C, f64, DEV), Guarded(M * C, f32, DEV), Guarded(C, f64, DEV), poisoned(wsb, DEV)
    assert _gen_call(lib, Kd, kind, Zd, Xd, D, lsd, vd, M, C - 1, a64, a32, q, ws) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert a64.untouched() and a32.untouched() and q.untouched() and bool((ws == 0xFF).all())
    del a64, a32, q
    torch.cuda.empty_cache()


def test_whiten_gen_declines_209_rows(lib):
    """M = 209 is the first row count of the class the persistent kernel does not have"""
    M, D, C = 209, 2, fu.persistent_c0(cus())
    Zd, Xd = rnd(M, D, dtype=f32, seed=1).to(DEV), rnd(C, D, seed=2).to(DEV)
    ls, Kd = torch.tensor([0.3], device=DEV), fu.sym_inverse(M, 3).to(DEV)
    wsb = int(lib.gpsa_whiten_workspace(M))
    a64, a32, q, ws = Guarded(M * C, f64, DEV), Guarded(M * C, f32, DEV), Guarded(C, f64, DEV), poisoned(wsb, DEV)
    assert wsb > 0 and _gen_call(lib, Kd, "rbf", Zd, Xd, D, ls, ls, M, C, a64, a32, q, ws) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert a64.untouched() and a32.untouched() and q.untouched() and bool((ws == 0xFF).all())
    del a64, a32, q
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# B. the long-K products
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _longk_pool(nprob, K, seed):
    """[nprob, 256, K + 6] panels with NaN in the six padding columns; a case takes the leading M rows"""
    ld = K + 6
    Bm, G = rnd(nprob, 256, ld, seed=seed), rnd(nprob, 256, ld, seed=seed + 1)
    Bm[..., K:], G[..., K:] = NAN, NAN
    d = rnd(nprob, K, seed=seed + 2)
    out0 = rnd(nprob, 256, 256, seed=seed + 3)
    return Bm, G, d, out0


def _longk_call(lib, nprob, G, Bm, d, d_dt, M, K, ld, sym, alpha, beta, outs, wsb=None, ws=None):
    """G / Bm / d: lists of device tensors or None; outs: Guarded.  Fresh poisoned workspace of the queried size"""
    need = int(lib.gpsa_longk_f64_workspace(M, K, nprob))
    wsb = need if wsb is None else wsb
    ws = poisoned(wsb, DEV) if ws is None else ws
    rc = lib.gpsa_longk_f64(nprob, fu.ptrs(G) if G is not None else None, fu.ptrs(Bm), fu.ptrs(d) if d is not None else None,
                            CODE[d_dt], M, K, ld, int(sym), fu.doubles(alpha), fu.doubles(beta),
                            (fu.C.c_void_p * nprob)(*[o.ptr() for o in outs]), p(ws), wsb, stream())
    torch.cuda.synchronize()
    return rc, need


def _longk_case(lib, M, K, nprob, mode):
    ld, sym = K + 6, mode == "dB/sym"
    Bp, Gp, dp, o0 = _longk_pool(nprob, K, 50 + nprob)
    Bm = Bp[:, :M].contiguous()
    G = None if sym else Gp[:, :M].contiguous()
    d_dt = f32 if mode == "G+dB/f32" else f64
    d = None if mode == "G" else dp.to(d_dt)
    out0 = o0[:, :M, :M].contiguous()
    if sym:  # the caller's promise of a symmetric result covers what beta keeps
        out0 = 0.5 * (out0 + out0.transpose(1, 2))
    alpha = [(-1.0) ** i * (1.0 + 0.5 * (i % 5)) for i in range(nprob)]  # different per product
    beta = [0.0 if i % 2 == 0 else 0.75 for i in range(nprob)]
    # the reference: fp64 on the CPU from the inputs as stored
    Bv = Bm[..., :K]
    A = (G[..., :K] if G is not None else 0.0) + (d.double()[:, None, :] * Bv if d is not None else 0.0)
    Aab = (G[..., :K].abs() if G is not None else 0.0) + (d.double().abs()[:, None, :] * Bv.abs() if d is not None else 0.0)
    al, be = torch.tensor(alpha, dtype=f64)[:, None, None], torch.tensor(beta, dtype=f64)[:, None, None]
    want = be * out0 + al * (A @ Bv.transpose(1, 2))
    bound = 2.0 * (K + 4) * U64 * (al.abs() * (Aab @ Bv.abs().transpose(1, 2)) + be.abs() * out0.abs())
    Bd, Gd = Bm.to(DEV), (G.to(DEV) if G is not None else None)
    dd = d.to(DEV) if d is not None else None
    res = []
    for _ in range(2):
        outs = [Guarded(M * M, f64, DEV, fill=NAN) for _ in range(nprob)]  # NaN where beta == 0: never read there
        for i in range(nprob):
            if beta[i] != 0.0:
                outs[i].view.copy_(out0[i].reshape(-1))
        rc, need = _longk_call(lib, nprob, list(Gd) if Gd is not None else None, list(Bd), list(dd) if dd is not None else None,
                               d_dt, M, K, ld, sym, alpha, beta, outs)
        assert need > 0, f"M={M} K={K} nprob={nprob}: the shape is not taken by the long-K kernel"
        assert rc == 0 and all(o.intact() for o in outs), (M, K, nprob, mode, rc)
        res.append(torch.stack([o.view.view(M, M) for o in outs]))
    what = f"longk_f64 {mode} M={M} K={K} ld={ld} nprob={nprob}"
    assert same_bits(res[0], res[1]), what + ": not repeatable"
    r = note("longk64", what, ratio(res[0], want, bound))
    assert r <= 1, (what, r)
    if sym:
        assert same_bits(res[0], res[0].transpose(1, 2).contiguous()), what + ": out != out^T"
    return r


@pytest.mark.parametrize("M", fu.ROWS_256)
@pytest.mark.parametrize("mode", fu.LONGK_MODES)
def test_longk_rows(lib, mode, M):
    """every row count, four products per launch, at the shortest K the kernel takes and at K tails of 2 and 14"""
    K0 = fu.longk_k0(lib, M, 4)
    for K in (K0, K0 + 2, K0 + 14):
        _longk_case(lib, M, K, 4, mode)


@pytest.mark.parametrize("nprob", [1, 48])
@pytest.mark.parametrize("mode", fu.LONGK_MODES)
def test_longk_class_edges_one_and_48_products(lib, mode, nprob):
    for M in fu.CLASS_FIRSTS + fu.CLASS_LASTS:
        _longk_case(lib, M, fu.longk_k0(lib, M, nprob), nprob, mode)


def test_longk_declined_shapes_leave_out_untouched(lib):
    """K odd, K < 512, odd ld, a base pointer off 16 bytes, too few workgroups, M = 257: GPSA_EUNSUPPORTED or a zero
    workspace, nothing written"""
    M, n = 100, 1
    K0 = fu.longk_k0(lib, M, n)
    big = rnd(M * (K0 + 8) + 2, seed=7).to(DEV)
    big257 = rnd(257 * (K0 + 8) + 2, seed=8).to(DEV)
    d = rnd(K0 + 8, seed=9).to(DEV)
    ws = poisoned(int(lib.gpsa_longk_f64_workspace(M, K0, n)), DEV)
    # (M, K, ld, element offset of the panels, zero workspace expected)
    cases = {"K odd": (M, K0 + 1, K0 + 2, 0, True), "K < 512": (M, 510, 510, 0, True), "odd ld": (M, K0, K0 + 1, 0, False),
             "base off 16 bytes": (M, K0, K0, 1, False), "too few workgroups": (M, K0 - 2, K0 - 2, 0, True),
             "M = 257": (257, K0, K0, 0, True)}
    for what, (m, K, ld, off, zero) in cases.items():
        src = big257 if m == 257 else big
        out = Guarded(m * m, f64, DEV)
        need = int(lib.gpsa_longk_f64_workspace(m, K, n))
        assert (need == 0) == zero, (what, need)
        rc, _ = _longk_call(lib, n, [src[off:]], [src[off:]], [d], f64, m, K, ld, False, [1.0], [1.0], [out], wsb=ws.numel(),
                            ws=ws)
        assert rc == EUNSUPPORTED and out.untouched() and bool((ws == 0xFF).all()), (what, rc)
    out = Guarded(M * M, f64, DEV)  # and the same call is taken once nothing is wrong with it
    rc, need = _longk_call(lib, n, [big], [big], [d], f64, M, K0, K0, False, [1.0], [0.0], [out])
    assert rc == 0 and need > 0 and not out.untouched() and out.intact()


# ------------------------------------------------------------------------------------------------------------------------
# C. gpsa_gemm and what rests on it
# ------------------------------------------------------------------------------------------------------------------------
def _operand(rows, width, dt, batch, extra, off, stride, seed):
    """a [batch] x rows x width operand stored with leading dimension width + extra at element offset ``off``; stride
    "0": one matrix for every problem, "odd": an odd number of elements between problems.  NaN everywhere the kernel has
    no business reading.  -> (storage, ld, stride in elements, the logical [batch, rows, width] matrices)"""
    ld = width + extra
    span = (rows - 1) * ld + width
    st = 0 if stride == "0" else (rows * ld if stride is None else (rows * ld) | 1)
    store = torch.full((off + st * (batch - 1) + span,), NAN, dtype=dt)
    vals = rnd(1 if stride == "0" else batch, rows, width, dtype=dt, seed=seed)
    torch.as_strided(store, tuple(vals.shape), (st, ld, 1), off).copy_(vals)
    return store, ld, st, vals.expand(batch, rows, width)


def _gemm_case(lib, dt, ta, tb, m, n, k, alpha=1.5, beta=-0.75, extra=0, off=0, ldc_extra=0, batch=1, strideA=None,
               strideB=None, splitk=1, c_nan=False, seed=0):
    """-> error / bound of one gpsa_gemm call (run twice, guards asserted)"""
    As, lda, sA, Av = _operand(k if ta else m, m if ta else k, dt, batch, extra, off, strideA, seed + 1)
    Bs, ldb, sB, Bv = _operand(n if tb else k, k if tb else n, dt, batch, extra, off, strideB, seed + 2)
    opA = (Av.transpose(1, 2) if ta else Av).double()
    opB = (Bv.transpose(1, 2) if tb else Bv).double()
    C0 = rnd(batch, m, n, dtype=dt, seed=seed + 3)
    want = alpha * (opA @ opB) + (beta * C0.double() if beta != 0.0 else 0.0)
    bound = bar(k, abs(alpha) * (opA.abs() @ opB.abs()), u=U64 if dt == f64 else U32, c0=C0, beta=beta)
    Ad, Bd = As.to(DEV), Bs.to(DEV)
    isz = 8 if dt == f64 else 4
    ldc = n + ldc_extra
    wsb = int(lib.gpsa_gemm_workspace(CODE[dt], m, n, batch, splitk))
    assert (wsb > 0) == (splitk > 1)
    res = []
    for _ in range(2):
        out = Guarded(batch * m * ldc, dt, DEV)
        Cv = out.view.view(batch, m, ldc)
        Cv[:, :, :n] = NAN if c_nan else C0.to(DEV)
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_gemm(CODE[dt], ta, tb, m, n, k, alpha, Ad.data_ptr() + off * isz, lda, sA, Bd.data_ptr() + off * isz,
                           ldb, sB, beta, out.ptr(), ldc, m * ldc, batch, splitk, p(ws), wsb, stream())
        torch.cuda.synchronize()
        assert rc == 0 and out.intact(), (m, n, k, rc)
        assert bool((Cv[:, :, n:] == SENTINEL).all()), f"({m}, {n}, {k}): a store past column n of a row (ldc = n + {ldc_extra})"
        res.append(Cv[:, :, :n].contiguous())
    assert same_bits(res[0], res[1]), (m, n, k, "not repeatable")
    return ratio(res[0], want, bound)


GEMM_PAIRS = [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("dt", [f32, f64], ids=["f32", "f64"])
@pytest.mark.parametrize("ta,tb", GEMM_PAIRS)
def test_gemm_shapes(lib, ta, tb, dt):
    """C1: 25 (m, n, k) covering 1, 15, 16, 17, 31, 33, 63, 64, 65, 129 in m and n and 1 .. 65 in k"""
    worst = 0.0
    for i, (m, n, k) in enumerate(fu.GEMM_TRIPLES):
        r = _gemm_case(lib, dt, ta, tb, m, n, k, beta=-0.75 if i % 2 else 0.0, c_nan=i % 2 == 0, seed=10 * i)
        print(f"[fp64-products] gemm: {dt} ta={ta} tb={tb} (m, n, k) = ({m}, {n}, {k}): error / bound {r:.3f}")
        assert r <= 1, f"{dt} ta={ta} tb={tb} (m, n, k) = ({m}, {n}, {k}): error / bound {r}"
        worst = max(worst, r)
    note("gemm", f"shapes {dt} ta={ta} tb={tb}", worst)


@pytest.mark.parametrize("dt", [f32, f64], ids=["f32", "f64"])
@pytest.mark.parametrize("ta,tb", GEMM_PAIRS)
def test_gemm_layouts(lib, ta, tb, dt):
    """C2: leading dimensions, base offsets (the 16-byte load path and the guarded scalar one), ldc = n + 5, broadcast
    and odd batch strides, beta = 0 over a NaN-filled C, alpha = 0"""
    worst = 0.0
    for m, n, k in ((33, 65, 37), (64, 64, 64)):
        cases = [dict(extra=e, off=o) for e in (0, 1, 3, 4) for o in (0, 1, 2)]
        cases += [dict(batch=3, strideA="0"), dict(batch=3, strideB="0"), dict(batch=3, strideA="odd", strideB="odd"),
                  dict(beta=0.0, c_nan=True), dict(alpha=0.0)]
        for i, kw in enumerate(cases):
            r = _gemm_case(lib, dt, ta, tb, m, n, k, ldc_extra=5, seed=100 + i, **kw)
            print(f"[fp64-products] gemm: {dt} ta={ta} tb={tb} ({m}, {n}, {k}) {kw}: error / bound {r:.3f}")
            assert r <= 1, f"{dt} ta={ta} tb={tb} ({m}, {n}, {k}) {kw}: error / bound {r}"
            worst = max(worst, r)
    note("gemm", f"layouts {dt} ta={ta} tb={tb}", worst)


@pytest.mark.parametrize("dt", [f32, f64], ids=["f32", "f64"])
@pytest.mark.parametrize("ta,tb", GEMM_PAIRS)
def test_gemm_splitk(lib, ta, tb, dt):
    """C3: seven slices over k = 33 leave four empty, 64 leave 61; the partials live in a poisoned workspace of exactly
    gpsa_gemm_workspace bytes; beta = 0 must not read the NaN-filled C"""
    worst = 0.0
    for k in (33, 1000):
        for splitk in (2, 7, 64):
            for beta in (0.0, -0.75):
                for batch in (1, 3):
                    r = _gemm_case(lib, dt, ta, tb, 33, 65, k, beta=beta, c_nan=beta == 0.0, batch=batch, splitk=splitk,
                                   seed=200 + k + splitk)
                    what = f"{dt} ta={ta} tb={tb} (33, 65, {k}) splitk={splitk} beta={beta} batch={batch}"
                    print(f"[fp64-products] gemm: {what}: error / bound {r:.3f}")
                    assert r <= 1, f"{what}: error / bound {r}"
                    worst = max(worst, r)
    note("gemm", f"split-K {dt} ta={ta} tb={tb}", worst)


@pytest.mark.parametrize("dt", [f32, f64], ids=["f32", "f64"])
def test_gemm_errors_leave_c_untouched(lib, dt):
    m, n, k = 33, 65, 37
    A, B = rnd(m, k, dtype=dt, seed=1).to(DEV), rnd(k, n, dtype=dt, seed=2).to(DEV)
    wsb = int(lib.gpsa_gemm_workspace(CODE[dt], m, n, 1, 7))
    assert wsb == 7 * m * n * (8 if dt == f64 else 4)
    ws = poisoned(wsb, DEV)

    def call(m_=m, batch=1, splitk=1, bytes_=wsb):
        out = Guarded(m * n, dt, DEV)
        rc = lib.gpsa_gemm(CODE[dt], 0, 0, m_, n, k, 1.0, p(A), k, 0, p(B), n, 0, 1.0, out.ptr(), n, m * n, batch, splitk,
                           p(ws), bytes_, stream())
        torch.cuda.synchronize()
        return rc, out.untouched() and bool((ws == 0xFF).all())

    assert call(splitk=7, bytes_=wsb - 1) == (EWORKSPACE, True)
    assert call(m_=0) == (EINVAL, True)
    assert call(splitk=0) == (EINVAL, True)
    assert call(batch=2, splitk=32768) == (EINVAL, True)  # batch * splitk = 65536
    rc, untouched = call(splitk=7)
    assert rc == 0 and not untouched


@pytest.mark.parametrize("M", [33, 64, 65, 113, 200])
def test_batched_forms(lib, M):
    """C5: the warp GPs' batched Gram, keep and column-update forms against the einsum reference.  L M rows share 64-row
    tiles whenever M is no multiple of 64"""
    worst = {"gram": 0.0, "keep": 0.0}
    for L in (1, 3):
        for B in (1, 3):
            for Cc in (64, 321, 1030):
                tag = f"M={M} L={L} batch={B} C={Cc}"
                alpha, g = rnd(B, M, Cc, seed=1), rnd(B, L, Cc, seed=4)
                Om = rnd(B, L, M, M, seed=2)
                Om = (Om + Om.transpose(-1, -2)).contiguous()
                dcT, dm, d = rnd(B, M, L, seed=3), rnd(B, L, Cc, seed=5), rnd(B, Cc, seed=6)
                ad, gd, Od, dcd, dmd, ddv = (t.to(DEV) for t in (alpha, g, Om, dcT, dm, d))
                # forward: W = Omega alpha, v = alpha . W, meanT = dcT^T alpha
                wW = torch.einsum("blmk,bkc->blmc", Om, alpha)
                aW = torch.einsum("blmk,bkc->blmc", Om.abs(), alpha.abs())
                wv, av = torch.einsum("bmc,blmc->blc", alpha, wW), torch.einsum("bmc,blmc->blc", alpha.abs(), aW)
                wm, am = dcT.transpose(1, 2) @ alpha, dcT.abs().transpose(1, 2) @ alpha.abs()
                fw = []
                for _ in range(2):
                    v, W, mT = Guarded(B * L * Cc, f64, DEV), Guarded(B * L * M * Cc, f64, DEV), Guarded(B * L * Cc, f64, DEV)
                    rc = lib.gpsa_quadform_fwd_keep_batched_f64(p(ad), p(Od), M, Cc, L, v.ptr(), W.ptr(), p(dcd), mT.ptr(),
                                                                B, stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and v.intact() and W.intact() and mT.intact(), tag
                    fw.append((v.view.view(B, L, Cc), W.view.view(B, L, M, Cc), mT.view.view(B, L, Cc)))
                assert all(same_bits(x, y) for x, y in zip(*fw)), tag
                rs = [ratio(fw[0][1], wW, bar(M, aW)), ratio(fw[0][0], wv, bar(2 * M, av)), ratio(fw[0][2], wm, bar(M, am))]
                # backward on W as the device stored it: dalpha = 2 sum_l g W + dcT dmeanT (2 L terms)
                Wd = fw[0][1].contiguous()
                Wh = Wd.cpu()
                wd = 2.0 * torch.einsum("blc,blmc->bmc", g, Wh) + dcT @ dm
                adl = 2.0 * torch.einsum("blc,blmc->bmc", g.abs(), Wh.abs()) + dcT.abs() @ dm.abs()
                bw = []
                for _ in range(2):
                    dal = Guarded(B * M * Cc, f64, DEV)
                    rc = lib.gpsa_quadform_bwd_alpha_kept_batched_f64(p(Wd), p(gd), M, Cc, L, p(dcd), p(dmd), dal.ptr(), B,
                                                                      stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and dal.intact(), tag
                    bw.append(dal.view.view(B, M, Cc))
                assert same_bits(bw[0], bw[1]), tag
                rs.append(ratio(bw[0], wd, bar(2 * L, adl)))
                # out = Y + s d o X (one product per element)
                Y = bw[0].contiguous()
                upd = 0.7 * d[:, None, :] * alpha
                ax = []
                for _ in range(2):
                    o = Guarded(B * M * Cc, f64, DEV)
                    rc = lib.gpsa_col_axpy_batched_f64(p(Y), p(ad), p(ddv), 0.7, M, Cc, o.ptr(), B, stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and o.intact(), tag
                    ax.append(o.view.view(B, M, Cc))
                assert same_bits(ax[0], ax[1]), tag
                rs.append(ratio(ax[0], Y.cpu() + upd, bar(1, upd.abs(), c0=Y.cpu(), beta=1.0)))
                worst["keep"] = max(worst["keep"], *rs)
                print(f"[fp64-products] keep forms: {tag}: error / bound W {rs[0]:.3f}, v {rs[1]:.3f}, meanT {rs[2]:.3f}, "
                      f"dalpha {rs[3]:.3f}, col_axpy {rs[4]:.3f}")
                assert max(rs) <= 1, (tag, rs)
                # dOmega[l] = sum_c g a a^T
                wg = torch.einsum("blc,bmc,bkc->blmk", g, alpha, alpha)
                ag = torch.einsum("blc,bmc,bkc->blmk", g.abs(), alpha.abs(), alpha.abs())
                wsb = int(lib.gpsa_gram_batched_workspace(M, Cc, L, B))
                gr = []
                for _ in range(2):
                    dOm, ws = Guarded(B * L * M * M, f64, DEV), poisoned(wsb, DEV)
                    rc = lib.gpsa_gram_batched_f64(p(ad), p(gd), M, Cc, L, dOm.ptr(), B, p(ws), wsb, stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and dOm.intact(), tag
                    gr.append(dOm.view.view(B, L, M, M))
                assert same_bits(gr[0], gr[1]), tag
                r = ratio(gr[0], wg, bar(Cc, ag))
                print(f"[fp64-products] gram_batched_f64: {tag}: error / bound {r:.3f}")
                assert r <= 1, (tag, r)
                worst["gram"] = max(worst["gram"], r)
    note("gram_batched", f"M={M}", worst["gram"])
    note("keep forms", f"M={M}", worst["keep"])


@pytest.mark.parametrize("M", [33, 65, 113, 256, 257])
def test_exact_dkuu(lib, M):
    """C6: dK += -(G + d o A) A^T into a non-zero dK; C = 63 / 64 run unsplit (63: the scalar load path), 4097 in 64
    slices"""
    for Cc in (63, 64, 4097):
        G, A, d, dK0 = rnd(M, Cc, seed=1), rnd(M, Cc, seed=2), rnd(Cc, dtype=f32, seed=3), rnd(M, M, seed=4)
        want = dK0 - (G + d.double()[None, :] * A) @ A.t()
        bound = bar(Cc, (G.abs() + d.double().abs()[None, :] * A.abs()) @ A.abs().t(), c0=dK0, beta=1.0)
        Gd, Ad, dd = G.to(DEV), A.to(DEV), d.to(DEV)
        wsb = int(lib.gpsa_exact_dkuu_workspace(M, Cc))
        res = []
        for _ in range(2):
            dK, ws = Guarded(M * M, f64, DEV), poisoned(wsb, DEV)
            dK.view.copy_(dK0.reshape(-1))
            rc = lib.gpsa_exact_dkuu_f64(p(Gd), p(Ad), p(dd), M, Cc, dK.ptr(), p(ws), wsb, stream())
            torch.cuda.synchronize()
            assert rc == 0 and dK.intact(), (M, Cc, rc)
            res.append(dK.view.view(M, M))
        assert same_bits(res[0], res[1]), (M, Cc)
        r = note("exact_dkuu", f"M={M} C={Cc} workspace={wsb}", ratio(res[0], want, bound))
        assert r <= 1, (M, Cc, r)


@pytest.mark.parametrize("M", [15, 16, 17, 20, 60, 63, 64, 65, 68, 128, 132, 255, 256, 260])
def test_omega_products(lib, M):
    """C7: Omega = A A^T + jitter I and its adjoint dA = (G + G^T) A, both sides of the direct-load kernel's acceptance
    (M % 4 == 0, M >= 16) and of its 64-row blocks; batch 3, A a full matrix"""
    B, jit = 3, 1e-5
    A = rnd(B, M, M, dtype=f32, seed=1)
    Aw = A.double()
    Ad = A.to(DEV)
    want = Aw @ Aw.transpose(1, 2) + jit * torch.eye(M, dtype=f64)
    bound = bar(M, Aw.abs() @ Aw.abs().transpose(1, 2), c0=jit * torch.eye(M, dtype=f64).expand(B, M, M), beta=1.0)
    res = []
    for _ in range(2):
        Om = Guarded(B * M * M, f64, DEV)
        rc = lib.gpsa_omega_fwd(p(Ad), M, B, jit, Om.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0 and Om.intact(), M
        res.append(Om.view.view(B, M, M))
    assert same_bits(res[0], res[1]), M
    r = note("omega", f"omega_fwd M={M}", ratio(res[0], want, bound))
    assert r <= 1, (M, r)
    for symmetric in (0, 1):
        G = rnd(B, M, M, seed=2)
        if symmetric:
            G = (G + G.transpose(1, 2)).contiguous()
        Gs = G + G.transpose(1, 2)
        want = Gs @ Aw
        bound = bar(M, (G.abs() + G.abs().transpose(1, 2)) @ Aw.abs(), want32=want)
        Gd = G.to(DEV)
        res = []
        for _ in range(2):
            dA = Guarded(B * M * M, f32, DEV)
            rc = lib.gpsa_omega_bwd(p(Gd), p(Ad), M, B, symmetric, dA.ptr(), stream())
            torch.cuda.synchronize()
            assert rc == 0 and dA.intact(), M
            res.append(dA.view.view(B, M, M))
        assert same_bits(res[0], res[1]), M
        r = note("omega", f"omega_bwd M={M} symmetric={symmetric}", ratio(res[0], want, bound))
        assert r <= 1, (M, symmetric, r)
