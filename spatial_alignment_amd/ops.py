"""Tensor-level wrappers over the C ABI (include/gpsa_hip.h).

PyTorch is used here only as plumbing: it owns device memory (torch.empty), the HIP stream
(torch.cuda.current_stream) and autograd bookkeeping.  Every numerical kernel below is a
hand-written HIP kernel in csrc/, reached through ctypes with raw device pointers.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._args import describe

F32, F64 = 0, 1
KINDS = {"rbf": 0, "matern12": 1, "matern32": 2}


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise TypeError(f"unsupported dtype {t.dtype}")


def _p(t):
    return 0 if t is None else t.data_ptr()


_raw_stream = torch._C._cuda_getCurrentRawStream  # (device index) -> hipStream_t as int


class HipOps:
    """All ops run on the current HIP stream of the tensors' device; outputs are freshly allocated."""

    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self._scratch = {}
        self._wsq_cache = {}
        if not torch.cuda.is_available():
            raise _lib.GpsaHipError("no HIP device visible: the GPSA hot path has no CPU fallback")

    # ------------------------------------------------------------------ plumbing
    # (host time per launch matters: a 1/8 shard of the headline step is bound by the ~250 launches'
    #  host cost, not by the GPU - so no Stream objects and no allocator round trip per call)
    @staticmethod
    def _stream(t):
        """raw hipStream_t of the current stream of t's device"""
        return _raw_stream(t.get_device())

    def _wsq(self, name, *args):
        """memoised *_workspace(...) query: the sizes depend on the arguments only, and a step asks the same
        two dozen questions every time (an FFI call each otherwise)"""
        key = (name,) + args
        v = self._wsq_cache.get(key)
        if v is None:
            v = self._wsq_cache[key] = int(getattr(self.lib, name)(*args))
        return v

    def _ws(self, nbytes, like):
        """scratch of >= nbytes for ONE launch sequence on the current stream.  One buffer per
        (device, stream), grown on demand: launches on a stream are ordered, scratch never outlives its
        call, so consecutive calls can share it."""
        dev = like.get_device()
        stream = _raw_stream(dev)
        # Inside a stream capture the buffer is the CAPTURE's own (round 6): a block allocated while capturing lives in
        # that graph's private pool; cached per stream alone, the next capture on the same stream baked it into a second
        # graph, and once the first graph was destroyed the allocator handed the block out again under the second
        # one's replays.  Nor may a capture bake the eager buffer: a later, larger request frees that one.  Entries of
        # finished captures are dropped here - that only returns their blocks to their own graphs' pools.
        cid = int(self.lib.gpsa_stream_capture_id(stream))
        key = (dev, stream, cid)
        if cid and key not in self._scratch:
            for k in [k for k in self._scratch if k[2] not in (0, cid)]:
                del self._scratch[k]
            self.__dict__["_retired"] = []
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < nbytes:
            # doubling only while that is cheap: the large-M plans ask for tens of GB
            grow = max(int(nbytes), 1 << 20, 0 if buf is None else min(2 * buf.numel(), int(nbytes) + (256 << 20)))
            if buf is not None:
                if cid:
                    # a block must not go back to the allocator inside a capture (its stream bookkeeping records
                    # events): the old buffer outlives the capture in this list
                    self.__dict__.setdefault("_retired", []).append(buf)
                else:
                    self._scratch[key] = None  # returned before the larger one is requested
                del buf
            buf = self._scratch[key] = torch.empty(grow, dtype=torch.uint8, device=like.device)
        return buf

    @staticmethod
    def _c(t):
        return t if t.is_contiguous() else t.contiguous()

    @staticmethod
    def _f64(t):
        t = t if t.dtype == torch.float64 else t.double()
        return t if t.is_contiguous() else t.contiguous()

    @staticmethod
    def _f32(t):
        t = t if t.dtype == torch.float32 else t.float()
        return t if t.is_contiguous() else t.contiguous()

    @staticmethod
    def _contiguous(what, dtype, **tensors):
        """name=(tensor, shape): every tensor contiguous, of ``dtype`` (fp64 or fp32) and of the named shape; an extent
        given as a string ("n >= 1", "P >= 1": how the refusal writes it) stands for any extent >= 1"""
        for name, (t, shape) in tensors.items():
            ok = torch.is_tensor(t) and t.dtype == dtype and t.is_contiguous() and t.dim() == len(shape) and all(
                (s == want) if isinstance(want, int) else (s >= 1) for s, want in zip(t.shape, shape))
            if not ok:
                want = ", ".join(str(s) for s in shape)
                raise ValueError(f"{what}: {name} must be a contiguous {'fp64' if dtype == torch.float64 else 'fp32'} "
                                 f"[{want}], not {describe(t)}")

    # ------------------------------------------------------------------ covariance matrices
    @staticmethod
    def _cov_args(Z, X, ls_u, var_u):
        """coordinates and hyper-parameters in ONE storage dtype (fp32 parameters pass through)"""
        dt = Z.dtype
        fix = lambda t: t if t.dtype == dt else t.to(dt)
        return HipOps._c(Z), HipOps._c(fix(X)), fix(ls_u), fix(var_u)

    def kmat(self, kind, Z, X, ls_u, var_u, jitter=0.0, dtype=None, out=None):
        """K = k(Z, X) computed and stored in ``dtype`` (default: Z's) from inputs of Z's dtype"""
        in_dt = None
        if X.dtype == torch.float64 and Z.dtype == torch.float32 and dtype == torch.float64:
            # fp32 parameters next to the warp GP's unrounded fp64 draws: read both as stored
            Z, X, in_dt = self._c(Z), self._c(X), 2  # GPSA_F32_X64
        else:
            Z, X, ls_u, var_u = self._cov_args(Z, X, ls_u, var_u)
        dtype = dtype or Z.dtype
        M, D = Z.shape
        Cn = X.shape[0]
        K = torch.empty(M, Cn, dtype=dtype, device=Z.device) if out is None else out
        assert K.shape == (M, Cn) and K.dtype == dtype and K.is_contiguous()
        rc = self.lib.gpsa_kmat(_dt(K), _dt(Z) if in_dt is None else in_dt, KINDS[kind], _p(Z), M, _p(X), Cn, D,
                                _p(ls_u), _p(var_u), float(jitter), _p(K), self._stream(Z))
        _lib.check(rc, "gpsa_kmat")
        return K

    def kmat_bwd(self, kind, Z, X, ls_u, var_u, Kbar, need_dX=True, same=False, out_dtype=None):
        """gradients in Z's dtype (``out_dtype`` = fp64 with fp32 inputs and an fp64 Kbar: stored as fp64);
        the arithmetic and partial sums run in Kbar's dtype.  ``same``: Z and X are the same points (K_uu):
        returns dZ + dX as dZ, and None for dX."""
        Z, X, ls_u, var_u = self._cov_args(Z, X, ls_u, var_u)
        Kbar = self._c(Kbar)
        M, D = Z.shape
        Cn = X.shape[0]
        odt, in_dt, kdt = Z.dtype, _dt(Z), _dt(Kbar)
        if out_dtype == torch.float64 and Z.dtype == torch.float32:
            # fp64 arithmetic and gradients from fp32 inputs; Kbar in either precision
            odt, in_dt, kdt = torch.float64, (3 if Kbar.dtype == torch.float64 else 4), F64
        dZ = torch.empty(Z.shape, dtype=odt, device=Z.device)
        dX = torch.empty(X.shape, dtype=odt, device=Z.device) if (need_dX and not same) else None
        dpar = torch.empty(2, dtype=odt, device=Z.device)
        wsb = self._wsq("gpsa_kmat_bwd_workspace", kdt, M, Cn, D)
        ws = self._ws(wsb, Z)
        rc = self.lib.gpsa_kmat_bwd(kdt, in_dt, KINDS[kind], _p(Z), M, _p(X), Cn, D, _p(ls_u),
                                    _p(var_u), _p(Kbar), int(bool(same)), _p(dZ), _p(dX), _p(dpar), _p(ws),
                                    ws.numel(), self._stream(Z))
        _lib.check(rc, "gpsa_kmat_bwd")
        return dZ, dX, dpar

    # ------------------------------------------------------------------ dense products
    def gemm(self, A, B, transA=False, transB=False, alpha=1.0, beta=0.0, out=None, splitk=1):
        """out = alpha * op(A) @ op(B) + beta * out.  A, B: 2-D, or 3-D batched (a 2-D operand is
        broadcast over the batch).  Last-dim stride must be 1."""
        batched = A.dim() == 3 or B.dim() == 3
        nb = (A.shape[0] if A.dim() == 3 else B.shape[0]) if batched else 1
        A = A if A.stride(-1) == 1 else A.contiguous()
        B = B if B.stride(-1) == 1 else B.contiguous()
        ar, ac = A.shape[-2], A.shape[-1]
        br, bc = B.shape[-2], B.shape[-1]
        m, k = (ac, ar) if transA else (ar, ac)
        k2, n = (bc, br) if transB else (br, bc)
        assert k == k2, (A.shape, B.shape, transA, transB)
        if out is None:
            assert beta == 0.0
            out = torch.empty((nb, m, n) if batched else (m, n), dtype=A.dtype, device=A.device)
        if splitk == 1 and nb == 1 and 128 <= k <= 1024 and ((m + 63) // 64) * ((n + 63) // 64) <= 32:
            splitk = min(4, k // 48)  # small M x M x M products are latency-bound: spread the k loop
        sA = A.stride(0) if A.dim() == 3 else 0
        sB = B.stride(0) if B.dim() == 3 else 0
        sC = out.stride(0) if out.dim() == 3 else 0
        wsb = self._wsq("gpsa_gemm_workspace", _dt(A), m, n, nb, splitk) if splitk > 1 else 0
        ws = self._ws(wsb, A) if splitk > 1 else None
        rc = self.lib.gpsa_gemm(_dt(A), int(transA), int(transB), m, n, k, float(alpha), _p(A),
                                A.stride(-2), sA, _p(B), B.stride(-2), sB, float(beta), _p(out),
                                out.stride(-2), sC, nb, splitk, _p(ws), wsb if ws is not None else 0,
                                self._stream(A))
        _lib.check(rc, "gpsa_gemm")
        return out

    @staticmethod
    def pick_splitk(k, m, n):
        """split the reduction dim so that a skinny product still fills the chip"""
        tiles = ((m + 63) // 64) * ((n + 63) // 64)
        s = max(1, min(256, -(-512 // max(tiles, 1)), k // 64))
        return int(s)

    # ------------------------------------------------------------------ variational covariances
    def omega_fwd(self, A, jitter, out=None):
        """A [B,M,M] fp32 -> A A^T + jitter I [B,M,M] fp64 (written into ``out`` when given)"""
        A = self._f32(A)
        Bn, M = A.shape[0], A.shape[-1]
        if out is None:
            out = torch.empty(Bn, M, M, dtype=torch.float64, device=A.device)
        assert out.is_contiguous() and out.dtype == torch.float64 and out.shape == (Bn, M, M)
        rc = self.lib.gpsa_omega_fwd(_p(A), M, Bn, float(jitter), _p(out), self._stream(A))
        _lib.check(rc, "gpsa_omega_fwd")
        return out

    def omega_bwd(self, G, A, symmetric=False):
        """dA = (G + G^T) A : G [B,M,M] fp64, A [B,M,M] fp32 -> fp32; ``symmetric`` promises G = G^T"""
        G = self._c(G if G.dtype == torch.float64 else G.double())
        A = self._f32(A)
        Bn, M = A.shape[0], A.shape[-1]
        dA = torch.empty(Bn, M, M, dtype=torch.float32, device=A.device)
        rc = self.lib.gpsa_omega_bwd(_p(G), _p(A), M, Bn, int(bool(symmetric)), _p(dA), self._stream(A))
        _lib.check(rc, "gpsa_omega_bwd")
        return dA

    # ------------------------------------------------------------------ factorisations (fp64)
    def chol(self, A):
        """A [B,M,M] fp64 (not modified) -> L, logdet [B], info [B] (int32)"""
        L = A.contiguous().clone()
        Bn, M = L.shape[0], L.shape[-1]
        logdet = torch.empty(Bn, dtype=torch.float64, device=A.device)
        info = torch.empty(Bn, dtype=torch.int32, device=A.device)
        rc = self.lib.gpsa_chol_f64(_p(L), M, Bn, _p(logdet), _p(info), self._stream(A))
        _lib.check(rc, "gpsa_chol_f64")
        return L, logdet, info

    def tri_inv(self, L):
        L = self._c(L)
        out = torch.empty_like(L)
        rc = self.lib.gpsa_tri_inv_f64(_p(L), _p(out), L.shape[-1], L.shape[0], self._stream(L))
        _lib.check(rc, "gpsa_tri_inv_f64")
        return out

    def chol_inv(self, A):
        """A [B,M,M] fp64 (not modified) -> L^-1 [B,M,M], logdet [B], info [B]; one fused register-resident
        sweep for M <= 256, the blocked factorisation (that sweep per diagonal block + fp64-MFMA
        products) above that."""
        A = self._c(A)
        Bn, M = A.shape[0], A.shape[-1]
        Linv = torch.empty_like(A)
        logdet = torch.empty(Bn, dtype=torch.float64, device=A.device)
        info = torch.empty(Bn, dtype=torch.int32, device=A.device)
        if M > 256:
            ws = self._ws(self._wsq("gpsa_chol_inv_blocked_workspace", M, Bn), A)
            rc = self.lib.gpsa_chol_inv_blocked_f64(_p(A), _p(Linv), M, Bn, _p(logdet), _p(info), _p(ws),
                                                    ws.numel(), self._stream(A))
            _lib.check(rc, "gpsa_chol_inv_blocked_f64")
            return Linv, logdet, info
        rc = self.lib.gpsa_chol_inv_f64(_p(A), _p(Linv), M, Bn, _p(logdet), _p(info), self._stream(A))
        _lib.check(rc, "gpsa_chol_inv_f64")
        return Linv, logdet, info

    def chol_inv_sel(self, A, n_always, keep_lo, keep_hi, Linv=None, logdet=None, info=None):
        """``chol_inv`` for a SELECTION of the batch in one launch (gpsa_chol_inv_sel_f64; M <= 256): the matrices
        b < n_always and keep_lo <= b < keep_hi; the other entries of Linv / logdet / info are left as they are"""
        A = self._c(A)
        Bn, M = A.shape[0], A.shape[-1]
        Linv = torch.empty_like(A) if Linv is None else Linv
        logdet = torch.empty(Bn, dtype=torch.float64, device=A.device) if logdet is None else logdet
        info = torch.empty(Bn, dtype=torch.int32, device=A.device) if info is None else info
        rc = self.lib.gpsa_chol_inv_sel_f64(_p(A), _p(Linv), M, Bn, int(n_always), int(keep_lo), int(keep_hi),
                                            _p(logdet), _p(info), self._stream(A))
        _lib.check(rc, "gpsa_chol_inv_sel_f64")
        return Linv, logdet, info

    # ------------------------------------------------------------------ quadratic forms
    def _qf_ws(self, alpha, L):
        M, Cn = alpha.shape
        return self._ws(self._wsq("gpsa_quadform_workspace", _dt(alpha), M, Cn, L), alpha)

    def quadform_fwd(self, alpha, Omega):
        alpha, Omega = self._c(alpha), self._c(Omega)
        M, Cn = alpha.shape
        L = Omega.shape[0]
        v = torch.empty(L, Cn, dtype=alpha.dtype, device=alpha.device)
        ws = self._qf_ws(alpha, L)
        rc = self.lib.gpsa_quadform_fwd(_dt(alpha), _dt(Omega), _p(alpha), _p(Omega), M, Cn, L, _p(v),
                                        _p(ws), ws.numel(), self._stream(alpha))
        _lib.check(rc, "gpsa_quadform_fwd")
        return v

    def quadform_bwd_alpha(self, alpha, Omega, g):
        alpha, Omega, g = self._c(alpha), self._c(Omega), self._c(g)
        M, Cn = alpha.shape
        L = Omega.shape[0]
        out = torch.empty_like(alpha)
        ws = self._qf_ws(alpha, L)
        rc = self.lib.gpsa_quadform_bwd_alpha(_dt(alpha), _dt(Omega), _p(alpha), _p(Omega), _p(g), M, Cn,
                                              L, _p(out), _p(ws), ws.numel(), self._stream(alpha))
        _lib.check(rc, "gpsa_quadform_bwd_alpha")
        return out

    def quadform_fwd_keep(self, alpha, Omega, dcT=None):
        """(v, W[, meanT]): the form, the products W[l] = Omega[l] alpha it is made of (few-output layers)
        and, with ``dcT`` [M,L], the mean term meanT = dcT^T alpha from the same pass over alpha"""
        alpha, Omega = self._c(alpha), self._c(Omega.to(alpha.dtype))
        M, Cn = alpha.shape
        L = Omega.shape[0]
        v = torch.empty(L, Cn, dtype=alpha.dtype, device=alpha.device)
        W = torch.empty(L, M, Cn, dtype=alpha.dtype, device=alpha.device)
        meanT = None
        if dcT is not None:
            dcT = self._c(dcT.to(alpha.dtype))
            assert dcT.shape == (M, L)
            meanT = torch.empty(L, Cn, dtype=alpha.dtype, device=alpha.device)
        rc = self.lib.gpsa_quadform_fwd_keep(_dt(alpha), _p(alpha), _p(Omega), M, Cn, L, _p(v), _p(W),
                                             _p(dcT), _p(meanT), self._stream(alpha))
        _lib.check(rc, "gpsa_quadform_fwd_keep")
        return (v, W) if dcT is None else (v, W, meanT)

    def quadform_elbo(self, alpha, Omega, meanT, q, var_u, eps, Y, noise_u, want_draws=False, delta=None):
        """The data GP's variance, draw, Gaussian likelihood and the backward's abar in one pass over the products
        Omega_l alpha (gpsa_quadform_elbo_f32; alpha fp32 [M,C], Omega [L,M,M], meanT [L,C], q fp64 [C], eps [S,N,L] or
        [C,L], Y [N,L]).  Returns (g [L,C], dmeanT [L,C], abar [M,C], z2 = sum ((Y - F)/s)^2 as an fp64 0-dim tensor), all at
        upstream gradient 1 of loss = -LL; with ``want_draws`` also the draws, transposed: FT [L,C].
        ``delta`` [M,L] instead of ``meanT`` (None): the kernel forms mean = delta^T alpha itself, in the padding row of its
        product (gpsa_quadform_elbo_delta_f32; only where gpsa_quadform_elbo_takes_delta(M))."""
        alpha, Omega = self._c(alpha), self._c(Omega)
        M, Cn = alpha.shape
        L = Omega.shape[0]
        q, eps, Y = self._c(q), self._c(eps), self._c(Y)
        meanT = self._c(meanT) if meanT is not None else None
        delta = self._c(delta) if delta is not None else None
        N = Y.shape[0]
        assert Cn % N == 0 and eps.numel() == Cn * L and Y.shape == (N, L) and q.dtype == torch.float64
        S = Cn // N
        dev = alpha.device
        g = torch.empty(L, Cn, dtype=torch.float32, device=dev)
        dm = torch.empty(L, Cn, dtype=torch.float32, device=dev)
        abar = torch.empty(M, Cn, dtype=torch.float32, device=dev)
        part = torch.empty(self.lib.gpsa_quadform_elbo_parts(), dtype=torch.float64, device=dev)
        wsb = self.lib.gpsa_quadform_elbo_f32_workspace(M, Cn, L)
        if wsb <= 0:
            raise _lib.GpsaHipError("gpsa_quadform_elbo_f32: more than 16 row tiles (M > 256)")
        ws = self._ws(wsb, alpha)
        FT = torch.empty(L, Cn, dtype=torch.float32, device=dev) if want_draws else None
        if delta is not None:
            assert meanT is None and tuple(delta.shape) == (M, L) and delta.dtype == torch.float32
            rc = self.lib.gpsa_quadform_elbo_delta_f32(_dt(Omega), _p(alpha), _p(Omega), M, Cn, L, _p(delta), _p(q),
                                                       _p(var_u), _p(eps), _p(Y), N, S, _p(noise_u), _p(g), _p(dm),
                                                       _p(abar), _p(part), _p(FT), _p(ws), ws.numel(), self._stream(alpha))
            _lib.check(rc, "gpsa_quadform_elbo_delta_f32")
            return (g, dm, abar, part.sum(), FT) if want_draws else (g, dm, abar, part.sum())
        rc = self.lib.gpsa_quadform_elbo_f32(_dt(Omega), _p(alpha), _p(Omega), M, Cn, L, _p(meanT), _p(q), _p(var_u),
                                             _p(eps), _p(Y), N, S, _p(noise_u), _p(g), _p(dm), _p(abar), _p(part),
                                             _p(FT), _p(ws), ws.numel(), self._stream(alpha))
        _lib.check(rc, "gpsa_quadform_elbo_f32")
        return (g, dm, abar, part.sum(), FT) if want_draws else (g, dm, abar, part.sum())

    def lmc_loglik_fused(self, F, W, Y, noise_u):
        """gpsa_lmc_loglik_fused_f32: (sum z^2 as an fp64 0-dim tensor, dLoss/dF [S,N,L], dLoss/dW [L,P]) of the LMC
        likelihood loss = -sum log N(Y; F W, s) / S at upstream gradient 1, F_obs never formed"""
        F, W, Y = self._c(F), self._c(W), self._c(Y)
        S, N, L = F.shape
        P = W.shape[1]
        assert W.shape[0] == L and Y.shape == (N, P)
        dev = F.device
        nparts = int(self.lib.gpsa_quadform_elbo_parts())
        zpart = torch.empty(nparts, dtype=torch.float64, device=dev)
        dF, dW = torch.empty_like(F), torch.empty_like(W)
        wsb = self.lib.gpsa_lmc_loglik_workspace(S * N, L, P, nparts)
        ws = self._ws(wsb, F)
        rc = self.lib.gpsa_lmc_loglik_fused_f32(_p(F), _p(W), _p(Y), _p(noise_u), S, N, L, P, _p(zpart), nparts, _p(dF),
                                                _p(dW), _p(ws), ws.numel(), self._stream(F))
        _lib.check(rc, "gpsa_lmc_loglik_fused_f32")
        return zpart.sum(), dF, dW

    def quadform_bwd_alpha_kept(self, W, g, dcT=None, dmeanT=None):
        """2 sum_l g_l o W_l  (+ dcT dmeanT, the mean term's share of the alpha-gradient, in the same pass)"""
        W, g = self._c(W), self._c(g)
        L, M, Cn = W.shape
        if dcT is not None:
            dcT, dmeanT = self._c(dcT.to(W.dtype)), self._c(dmeanT.to(W.dtype))
            assert dcT.shape == (M, L) and dmeanT.shape == (L, Cn)
        out = torch.empty(M, Cn, dtype=W.dtype, device=W.device)
        rc = self.lib.gpsa_quadform_bwd_alpha_kept(_dt(W), _p(W), _p(g), M, Cn, L, _p(dcT), _p(dmeanT), _p(out),
                                                   self._stream(W))
        _lib.check(rc, "gpsa_quadform_bwd_alpha_kept")
        return out

    def quadform_bwd_omega(self, alpha, g, out_dtype=None):
        """``out_dtype``: storage type of the result (fp64 from fp32 inputs: the MFMA path widens its
        partial sums while adding them; elsewhere a converted copy)"""
        alpha, g = self._c(alpha), self._c(g)
        M, Cn = alpha.shape
        L = g.shape[0]
        odt = alpha.dtype if out_dtype is None else out_dtype
        out = torch.empty(L, M, M, dtype=odt, device=alpha.device)
        ws = self._qf_ws(alpha, L)
        rc = self.lib.gpsa_quadform_bwd_omega(_dt(alpha), _dt(out), _p(alpha), _p(g), M, Cn, L, _p(out),
                                              _p(ws), ws.numel(), self._stream(alpha))
        if rc == _lib.GPSA_EUNSUPPORTED and odt != alpha.dtype:
            return self.quadform_bwd_omega(alpha, g).to(odt)
        _lib.check(rc, "gpsa_quadform_bwd_omega")
        return out

    def quadform_bwd_omega_delta(self, alpha, g, dmeanT, ddelta=None, beta=0.0, out_dtype=torch.float64):
        """gpsa_quadform_bwd_omega_delta_f32: (dOmega [L,M,M], ddelta [M,L] = beta ddelta + alpha dmeanT^T) from one Gram
        launch (the mean term's gradient in the padding row of the kernel's last row tile); None where the shape does not
        allow it (gpsa_quadform_bwd_omega_takes_delta)"""
        alpha, g, dmeanT = self._c(alpha), self._c(g), self._c(dmeanT)
        M, Cn = alpha.shape
        L = g.shape[0]
        if not self.lib.gpsa_quadform_bwd_omega_takes_delta(M, Cn):
            return None
        out = torch.empty(L, M, M, dtype=out_dtype, device=alpha.device)
        if ddelta is None:
            ddelta = torch.zeros(M, L, dtype=torch.float32, device=alpha.device)
        ws = self._qf_ws(alpha, L)
        rc = self.lib.gpsa_quadform_bwd_omega_delta_f32(_dt(out), _p(alpha), _p(g), _p(dmeanT), M, Cn, L, _p(out),
                                                        _p(ddelta), float(beta), _p(ws), ws.numel(), self._stream(alpha))
        _lib.check(rc, "gpsa_quadform_bwd_omega_delta_f32")
        return out, ddelta

    def panel_mm(self, P, X, want_colsq=False, transP=False):
        """Y = op(P) @ X in X's dtype; P [M,M] may be stored in either precision"""
        P, X = self._c(P), self._c(X)
        M, Cn = X.shape
        Y = torch.empty_like(X)
        q = torch.empty(Cn, dtype=X.dtype, device=X.device) if want_colsq else None
        ws = self._ws(max(4 * 256 * 256, 8 * M * M) + 512, X)
        rc = self.lib.gpsa_panel_mm(_dt(X), _dt(P), int(bool(transP)), _p(P), _p(X), M, Cn, _p(Y), _p(q),
                                    _p(ws), ws.numel(), self._stream(X))
        _lib.check(rc, "gpsa_panel_mm")
        return Y, q

    def whiten(self, Kinv, Kuf, out_dtype, want_q=True):
        """alpha = Kinv @ Kuf (fp64 MFMA; Kuf fp32 or fp64, widened on the fly) stored as ``out_dtype``,
        q[c] = Kuf[:,c] . alpha[:,c] (fp64).  Returns None when M is beyond the register-resident kernel
        (callers chain panel_mm)."""
        Kinv, Kuf = self._c(Kinv), self._c(Kuf)
        assert Kinv.dtype == torch.float64
        M, Cn = Kuf.shape
        nbytes = self._wsq("gpsa_whiten_workspace", M)
        if nbytes == 0:
            return None
        alpha = torch.empty(M, Cn, dtype=out_dtype, device=Kuf.device)
        q = torch.empty(Cn, dtype=torch.float64, device=Kuf.device) if want_q else None
        ws = self._ws(nbytes, Kuf)
        rc = self.lib.gpsa_whiten_f64(_p(Kinv), _dt(Kuf), _p(Kuf), M, Cn, _dt(alpha), _p(alpha), _p(q),
                                      _p(ws), nbytes, self._stream(Kuf))
        _lib.check(rc, "gpsa_whiten_f64")
        return alpha, q

    def col_axpy(self, Y, X, d, s=1.0, out=None):
        Y, X, d = self._c(Y), self._c(X), self._c(d)
        M, Cn = X.shape
        out = torch.empty_like(Y) if out is None else out
        rc = self.lib.gpsa_col_axpy(_dt(X), _p(Y), _p(X), _p(d), float(s), M, Cn, _p(out),
                                    self._stream(X))
        _lib.check(rc, "gpsa_col_axpy")
        return out

    # ------------------------------------------------------------------ sampling
    def data_sample_fwd(self, meanT, v, q, var_u, eps):
        meanT, v, q, eps = self._c(meanT), self._c(v), self._c(q.double()), self._c(eps)
        L, Cn = meanT.shape
        F = torch.empty(Cn, L, dtype=torch.float32, device=meanT.device)
        Sigma = torch.empty_like(meanT)
        rc = self.lib.gpsa_data_sample_fwd(_p(meanT), _p(v), _p(q), _p(var_u), _p(eps), Cn, L, _p(F),
                                           _p(Sigma), self._stream(meanT))
        _lib.check(rc, "gpsa_data_sample_fwd")
        return F, Sigma

    def data_sample_bwd(self, dF, eps, Sigma, var_u):
        """-> g_ext [L+1, C] (rows 0..L-1: g[l,c]; row L: qbar[c] = -sum_l g), dmeanT [L,C], dvar [1].
        (one buffer for both; qbar is exactly minus the column sums of g, which the layer backward uses)"""
        dF, eps = self._c(dF), self._c(eps)
        L, Cn = Sigma.shape
        g_ext = torch.empty(L + 1, Cn, dtype=torch.float32, device=Sigma.device)
        dmeanT = torch.empty_like(Sigma)
        dvar = torch.empty(1, dtype=torch.float32, device=Sigma.device)
        ws = self._ws(8 * (Cn // 32 + 2), Sigma)
        rc = self.lib.gpsa_data_sample_bwd(_p(dF), _p(eps), _p(Sigma), _p(var_u), Cn, L, _p(g_ext),
                                           _p(dmeanT), g_ext.data_ptr() + 4 * L * Cn, 0, _p(dvar), _p(ws),  # (0 = GPSA_F32)
                                           ws.numel(), self._stream(Sigma))
        _lib.check(rc, "gpsa_data_sample_bwd")
        return g_ext, dmeanT, dvar

    def predict_moments(self, meanT, v, q, var_u, S, W=None, noise_u=None, include_noise=False, Y=None,
                        latent=False, out=None):
        """gpsa_predict_moments_f32: the data GP's closing as moments instead of a draw.  meanT, v [L, S*c] fp32 (column
        s*c + r), q [S*c] fp64, var_u / noise_u device scalars (unconstrained), W [L,P] or None (then P = L), Y [c,P] or
        None.  -> (F_mean, F_var [c,P] fp32, Fl_mean, Fl_var [c,L] fp32 or None, lpd [c] fp64 or None); ``out``: the same
        five, preallocated (contiguous row slices of the caller's result tensors; None where nothing is wanted)."""
        meanT, v, q = self._c(meanT), self._c(v), self._c(q.double())
        L, SC = meanT.shape
        S = int(S)
        if S < 1 or SC % S != 0 or tuple(v.shape) != (L, SC) or q.numel() != SC:
            raise ValueError(f"predict_moments: meanT {tuple(meanT.shape)}, v {tuple(v.shape)}, q {tuple(q.shape)} do not "
                             f"hold S = {S} samples of the same rows")
        c = SC // S
        var_u = self._f32(var_u).reshape(-1)
        W = None if W is None else self._f32(W)
        if W is not None and W.shape[0] != L:
            raise ValueError(f"predict_moments: W has {W.shape[0]} rows, the data GP {L} latent outputs")
        P = L if W is None else int(W.shape[1])
        noise_u = None if noise_u is None else self._f32(noise_u).reshape(-1)
        Y = None if Y is None else self._f32(Y)
        if Y is not None and tuple(Y.shape) != (c, P):
            raise ValueError(f"predict_moments: Y has shape {tuple(Y.shape)}, the chunk needs ({c}, {P})")
        dev, f32 = meanT.device, torch.float32
        if out is None:
            new = lambda *sh, dt=f32: torch.empty(*sh, dtype=dt, device=dev)
            out = (new(c, P), new(c, P), new(c, L) if latent else None, new(c, L) if latent else None,
                   new(c, dt=torch.float64) if Y is not None else None)
        Fm, Fv, Lm, Lv, lpd = out
        for t, sh, dt in ((Fm, (c, P), f32), (Fv, (c, P), f32), (Lm, (c, L), f32), (Lv, (c, L), f32),
                          (lpd, (c,), torch.float64)):
            assert t is None or (tuple(t.shape) == sh and t.dtype == dt and t.is_contiguous()), (sh, dt)
        rc = self.lib.gpsa_predict_moments_f32(_p(meanT), _p(v), _p(q), _p(var_u), c, S, L, P, _p(W), _p(noise_u),
                                               int(bool(include_noise)), _p(Y), _p(Fm), _p(Fv), _p(Lm), _p(Lv), _p(lpd),
                                               self._stream(meanT))
        if rc == _lib.GPSA_EUNSUPPORTED:
            raise _lib.GpsaHipError(f"gpsa_predict_moments_f32: an LMC mix of {L} latent outputs (more than 64, the "
                                    "limit the LDS-resident W shares with the training kernels)")
        _lib.check(rc, "gpsa_predict_moments_f32")
        return Fm, Fv, Lm, Lv, lpd

    def predict_counts(self, meanT, v, q, var_u, S, W=None, log_offset=None, Y=None, out=None):
        """gpsa_predict_counts_f32: the same layer closed under a Poisson likelihood (log link).  meanT, v, q, var_u, S, W
        as ``predict_moments`` takes them; log_offset [c] fp32 or None (= 0), Y [c,P] counts (NaN = missing) or None.
        -> (Y_mean, Y_var [c,P] fp32, lpd [c] fp64 or None); ``out``: the same three, preallocated."""
        meanT, v, q = self._c(meanT), self._c(v), self._c(q.double())
        L, SC = meanT.shape
        S = int(S)
        if S < 1 or SC % S != 0 or tuple(v.shape) != (L, SC) or q.numel() != SC:
            raise ValueError(f"predict_counts: meanT {tuple(meanT.shape)}, v {tuple(v.shape)}, q {tuple(q.shape)} do not "
                             f"hold S = {S} samples of the same rows")
        c = SC // S
        var_u = self._f32(var_u).reshape(-1)
        W = None if W is None else self._f32(W)
        if W is not None and W.shape[0] != L:
            raise ValueError(f"predict_counts: W has {W.shape[0]} rows, the data GP {L} latent outputs")
        P = L if W is None else int(W.shape[1])
        log_offset = None if log_offset is None else self._f32(log_offset)
        if log_offset is not None and tuple(log_offset.shape) != (c,):
            raise ValueError(f"predict_counts: log_offset has shape {tuple(log_offset.shape)}, the chunk needs ({c},)")
        Y = None if Y is None else self._f32(Y)
        if Y is not None and tuple(Y.shape) != (c, P):
            raise ValueError(f"predict_counts: Y has shape {tuple(Y.shape)}, the chunk needs ({c}, {P})")
        dev, f32 = meanT.device, torch.float32
        if out is None:
            out = (torch.empty(c, P, dtype=f32, device=dev), torch.empty(c, P, dtype=f32, device=dev),
                   torch.empty(c, dtype=torch.float64, device=dev) if Y is not None else None)
        Ym, Yv, lpd = out
        for t, sh, dt in ((Ym, (c, P), f32), (Yv, (c, P), f32), (lpd, (c,), torch.float64)):
            assert t is None or (tuple(t.shape) == sh and t.dtype == dt and t.is_contiguous()), (sh, dt)
        rc = self.lib.gpsa_predict_counts_f32(_p(meanT), _p(v), _p(q), _p(var_u), c, S, L, P, _p(W), _p(log_offset),
                                              _p(Y), _p(Ym), _p(Yv), _p(lpd), self._stream(meanT))
        if rc == _lib.GPSA_EUNSUPPORTED:
            raise _lib.GpsaHipError(f"gpsa_predict_counts_f32: an LMC mix of {L} latent outputs (more than 64, the "
                                    "limit the LDS-resident W shares with the training kernels)")
        _lib.check(rc, "gpsa_predict_counts_f32")
        return Ym, Yv, lpd

    def _warp_model_args(self, what, kind, Z, beta, A, b, ls_u, var_u):
        """the model side of the two warp entries as contiguous fp64 tensors, shapes checked -> (tensors, M, D)"""
        if kind not in KINDS:
            raise ValueError(f"{what}: kind must be one of {sorted(KINDS)}, not {kind!r}")
        Z, beta, A, b, ls_u, var_u = (self._f64(t) for t in (Z, beta, A, b, ls_u, var_u))
        if Z.dim() != 2:
            raise ValueError(f"{what}: Z has shape {tuple(Z.shape)}, [M, D] is needed")
        M, D = (int(s) for s in Z.shape)
        for name, t, sh in (("beta", beta, (M, D)), ("A", A, (D, D)), ("b", b, (D,))):
            if tuple(t.shape) != sh:
                raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, Z gives {sh}")
        return (Z, beta, A, b, ls_u.reshape(-1), var_u.reshape(-1)), M, D

    def warp_field(self, kind, Z, beta, A, b, ls_u, var_u, X, jacobian=True, out=None):
        """gpsa_warp_field_f64: the warp mean g(x) = x A + b + k(x, Z) beta at X [n, D] and, with ``jacobian``, its
        Jacobian J [n, D, D] (J[n, j, d] = d g_j / d x_d) and det J [n]; all fp64.  -> (G, J or None, det or None);
        ``out``: the same three, preallocated (contiguous row slices of the caller's results)."""
        mdl, M, D = self._warp_model_args("warp_field", kind, Z, beta, A, b, ls_u, var_u)
        X = self._f64(X)
        if X.dim() != 2 or X.shape[1] != D or X.shape[0] < 1:
            raise ValueError(f"warp_field: X has shape {tuple(X.shape)}, [n >= 1, {D}] is needed")
        n = int(X.shape[0])
        f64, dev = torch.float64, X.device
        if out is None:
            out = (torch.empty(n, D, dtype=f64, device=dev),
                   torch.empty(n, D, D, dtype=f64, device=dev) if jacobian else None,
                   torch.empty(n, dtype=f64, device=dev) if jacobian else None)
        G, J, det = out
        for t, sh in ((G, (n, D)), (J, (n, D, D)), (det, (n,))):
            assert t is None or (tuple(t.shape) == sh and t.dtype == f64 and t.is_contiguous()), sh
        rc = self.lib.gpsa_warp_field_f64(KINDS[kind], *(_p(t) for t in mdl), _p(X), n, M, D, _p(G), _p(J), _p(det),
                                          self._stream(X))
        _lib.check(rc, "gpsa_warp_field_f64")
        return G, J, det

    def warp_invert(self, kind, Z, beta, A, b, ls_u, var_u, target, x0, iters, out=None):
        """gpsa_warp_invert_f64: exactly ``iters`` Newton updates of g(x) = target [n, D] from x0 [n, D] in one launch
        -> (X [n, D], residual [n] = |g(X) - target|_2 at the returned X); a failed row is NaN / +inf.  All fp64."""
        mdl, M, D = self._warp_model_args("warp_invert", kind, Z, beta, A, b, ls_u, var_u)
        target, x0 = self._f64(target), self._f64(x0)
        if target.dim() != 2 or target.shape[1] != D or target.shape[0] < 1 or tuple(x0.shape) != tuple(target.shape):
            raise ValueError(f"warp_invert: target {tuple(target.shape)} and x0 {tuple(x0.shape)} must both be "
                             f"[n >= 1, {D}]")
        iters = int(iters)
        if iters < 0:
            raise ValueError(f"warp_invert: iters must be >= 0, not {iters}")
        n = int(target.shape[0])
        f64, dev = torch.float64, target.device
        if out is None:
            out = (torch.empty(n, D, dtype=f64, device=dev), torch.empty(n, dtype=f64, device=dev))
        X, res = out
        for t, sh in ((X, (n, D)), (res, (n,))):
            assert tuple(t.shape) == sh and t.dtype == f64 and t.is_contiguous(), sh
        rc = self.lib.gpsa_warp_invert_f64(KINDS[kind], *(_p(t) for t in mdl), _p(target), _p(x0), iters, n, M, D, _p(X),
                                           _p(res), self._stream(target))
        _lib.check(rc, "gpsa_warp_invert_f64")
        return X, res

    def knn(self, Q, R, k, exclude_self=False, parts=0, out=None):
        """gpsa_knn_f64: for every row of Q [nq, D] the k rows of R [nr, D] with the smallest key (squared distance in
        fp64, index), ascending -> (idx [nq, k] int32, d2 [nq, k] fp64).  ``exclude_self`` skips a query's own row of
        R (Q is then R itself or a contiguous row slice of R's storage: a chunk); ``parts``: slices of the reference axis, 0 = auto - the result is the
        same bits for every value.  ``out``: the same two, preallocated."""
        Q, R = self._f64(Q), self._f64(R)
        if Q.dim() != 2 or R.dim() != 2 or Q.shape[0] < 1 or R.shape[0] < 1 or Q.shape[1] != R.shape[1]:
            raise ValueError(f"knn: Q {tuple(Q.shape)} and R {tuple(R.shape)} must be [nq >= 1, D] and [nr >= 1, D]")
        (nq, D), nr = (int(s) for s in Q.shape), int(R.shape[0])
        k, parts, excl = int(k), int(parts), 1 if exclude_self else 0
        if D < 1 or D > 4:
            raise ValueError(f"knn: D = {D}; 1 to 4 coordinates are supported")
        if k < 1 or k > 32:
            raise ValueError(f"knn: k = {k}; 1 to 32 neighbours are supported")
        if k > nr - excl:
            raise ValueError(f"knn: k = {k} neighbours asked of {nr - excl} reference rows"
                             + (" (the point itself is excluded)" if excl else ""))
        if excl and nq > nr:
            raise ValueError(f"knn: exclude_self needs Q to be R or a row slice of it, not {nq} rows against {nr}")
        if parts < 0:
            raise ValueError(f"knn: parts must be >= 0, not {parts}")
        dev = Q.device
        if out is None:
            out = (torch.empty(nq, k, dtype=torch.int32, device=dev), torch.empty(nq, k, dtype=torch.float64, device=dev))
        idx, d2 = out
        for t, dt in ((idx, torch.int32), (d2, torch.float64)):
            assert tuple(t.shape) == (nq, k) and t.dtype == dt and t.is_contiguous(), (nq, k)
        nbytes = self._wsq("gpsa_knn_workspace", nq, nr, k, parts)
        ws = self._ws(nbytes, Q) if nbytes else None
        rc = self.lib.gpsa_knn_f64(_p(Q), nq, _p(R), nr, D, k, excl, parts, _p(idx), _p(d2), _p(ws), nbytes,
                                   self._stream(Q))
        _lib.check(rc, "gpsa_knn_f64")
        return idx, d2

    def knn_average(self, idx, d2, Y, weights="uniform", out=None):
        """gpsa_knn_average_f32: out[i, p] = sum_j w_ij Y[idx[i, j], p] / sum_j w_ij over the neighbours whose Y entry
        is not NaN (none: NaN), fp64 accumulation in neighbour order -> [nq, P] fp32 (an fp64 Y goes through
        gpsa_knn_average_f64 and gives fp64; every other dtype is taken to fp32).  ``weights``: "uniform" (d2 may be
        None) or "distance" (1 / sqrt(d2); a row with zero distances averages exactly those neighbours).  The indices
        are not validated: they must be rows of Y."""
        if weights not in ("uniform", "distance"):
            raise ValueError(f"knn_average: weights must be 'uniform' or 'distance', not {weights!r}")
        if idx.dim() != 2 or idx.dtype != torch.int32 or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise ValueError(f"knn_average: idx must be int32 [nq >= 1, k >= 1], not {idx.dtype} {tuple(idx.shape)}")
        if Y.dim() != 2 or Y.shape[0] < 1 or Y.shape[1] < 1:
            raise ValueError(f"knn_average: Y has shape {tuple(Y.shape)}, [nr >= 1, P >= 1] is needed")
        wcode = 1 if weights == "distance" else 0
        if wcode:
            if d2 is None or tuple(d2.shape) != tuple(idx.shape):
                raise ValueError("knn_average: weights='distance' needs d2 of idx's shape "
                                 f"{tuple(idx.shape)}, not {None if d2 is None else tuple(d2.shape)}")
            d2 = self._f64(d2)
        else:
            d2 = None
        wide = Y.dtype == torch.float64
        idx, Y = self._c(idx), (self._f64(Y) if wide else self._f32(Y))
        (nq, k), (nr, P) = (int(s) for s in idx.shape), (int(s) for s in Y.shape)
        if out is None:
            out = torch.empty(nq, P, dtype=Y.dtype, device=Y.device)
        assert tuple(out.shape) == (nq, P) and out.dtype == Y.dtype and out.is_contiguous(), (nq, P)
        name = "gpsa_knn_average_f64" if wide else "gpsa_knn_average_f32"
        rc = getattr(self.lib, name)(_p(idx), _p(d2), nq, k, _p(Y), nr, P, wcode, _p(out), self._stream(Y))
        _lib.check(rc, name)
        return out

    # ------------------------------------------------------------------ rigid pre-registration (csrc/register.hip)
    def rigid_scores(self, XA, YA, XB, YB, T, max_d2, parts=0, return_nn=False):
        """gpsa_rigid_scores_f64: for every candidate k of T [K, 6] (R row-major, then t) the rows of XB [n, 2] are taken
        to q = R x + t, matched to their nearest row of XA [m, 2] by the key (fp64 squared distance, index) where that
        distance is <= max_d2, and scored on the expression YA [m, P] / YB [n, P] (fp32) -> (sse [K] fp64,
        n_matched [K] int64, d2_sum [K] fp64, nn [K, n] int32 or None, d2 [K, n] fp64 or None).  ``parts``: slices of
        the A axis, 0 = auto - the result is the same bits for every value, every K and every repeat."""
        XA, XB, T = self._f64(XA), self._f64(XB), self._f64(T)
        YA, YB = self._f32(YA), self._f32(YB)
        if XA.dim() != 2 or XB.dim() != 2 or XA.shape[0] < 1 or XB.shape[0] < 1:
            raise ValueError(f"rigid_scores: XA {tuple(XA.shape)} and XB {tuple(XB.shape)} must be [m >= 1, 2] and "
                             "[n >= 1, 2]")
        if XA.shape[1] != 2 or XB.shape[1] != 2:
            raise ValueError(f"rigid_scores: D = {int(XA.shape[1])} and {int(XB.shape[1])}; the candidates are transforms "
                             "of the plane, D = 2 is needed")
        m, n = int(XA.shape[0]), int(XB.shape[0])
        if YA.dim() != 2 or YB.dim() != 2 or YA.shape[0] != m or YB.shape[0] != n or YA.shape[1] < 1 \
                or YA.shape[1] != YB.shape[1]:
            raise ValueError(f"rigid_scores: YA {tuple(YA.shape)} and YB {tuple(YB.shape)} must be [{m}, P] and [{n}, P] "
                             "with one P >= 1")
        P = int(YA.shape[1])
        if T.dim() != 2 or T.shape[0] < 1 or T.shape[1] != 6:
            raise ValueError(f"rigid_scores: T has shape {tuple(T.shape)}; [K >= 1, 6] (R row-major, then t) is needed")
        K, parts, max_d2 = int(T.shape[0]), int(parts), float(max_d2)
        if K > 65535 or K * n > 2**38:
            raise ValueError(f"rigid_scores: K = {K} candidates of {n} rows; at most 65535 candidates and 2^38 (candidate, "
                             "row) pairs per call are supported - pass the table in chunks")
        if not (0.0 <= max_d2 < float("inf")):
            raise ValueError(f"rigid_scores: max_d2 must be finite and >= 0, not {max_d2}")
        if parts < 0:
            raise ValueError(f"rigid_scores: parts must be >= 0, not {parts}")
        dev, i64, f64 = XB.device, torch.int64, torch.float64
        sse, d2_sum = torch.empty(K, dtype=f64, device=dev), torch.empty(K, dtype=f64, device=dev)
        n_matched = torch.empty(K, dtype=i64, device=dev)
        nn = torch.empty(K, n, dtype=torch.int32, device=dev) if return_nn else None
        d2 = torch.empty(K, n, dtype=f64, device=dev) if return_nn else None
        nbytes = self._wsq("gpsa_rigid_scores_workspace", n, m, K, P, parts, 1 if return_nn else 0)
        ws = self._ws(nbytes, XB)
        rc = self.lib.gpsa_rigid_scores_f64(_p(XA), _p(YA), m, _p(XB), _p(YB), n, P, _p(T), K, max_d2, parts, _p(sse),
                                            _p(n_matched), _p(d2_sum), _p(nn), _p(d2), _p(ws), nbytes, self._stream(XB))
        _lib.check(rc, "gpsa_rigid_scores_f64")
        return sse, n_matched, d2_sum, nn, d2

    # ------------------------------------------------------------------ exact GP regression (csrc/gpr.hip)
    def _gpr_args(self, what, kind, theta, *coords):
        """-> (kind code, theta, D) after the checks the three gpr entries share: the kernel's name, theta = three fp64
        values on the device, coordinates fp64 [n >= 1, D] with one D in 1 .. 4"""
        if kind not in KINDS:
            raise ValueError(f"{what}: kernel must be one of {sorted(KINDS)}, not {kind!r}")
        if theta.dim() != 1 or theta.shape[0] != 3 or theta.dtype != torch.float64 or not theta.is_contiguous():
            raise ValueError(f"{what}: theta must be a contiguous fp64 [3] (log a, log l, log tau2), not {theta.dtype} "
                             f"{tuple(theta.shape)}")
        D = int(coords[0].shape[1]) if coords[0].dim() == 2 else 0
        for X in coords:
            if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] != D or X.dtype != torch.float64 or not X.is_contiguous():
                raise ValueError(f"{what}: coordinates must be contiguous fp64 [n >= 1, D] with one D, not {X.dtype} "
                                 f"{tuple(X.shape)}")
        if D < 1 or D > 4:
            raise ValueError(f"{what}: D = {D}; 1 to 4 coordinates are supported")
        return KINDS[kind], theta, D

    def gpr_cov(self, kind, XA, XB, theta, amplitude=False, same=False, jitter=0.0, out=None):
        """gpsa_gpr_cov_f64: K [na, nb] = a k(XA, XB) in sklearn's kernel forms, fp64; ``same`` (XB is XA): plus
        (tau2 + jitter) on the diagonal, exactly symmetric.  theta [3] fp64 on the device: log a, log l, log tau2."""
        kd, theta, D = self._gpr_args("gpr_cov", kind, theta, XA, XB)
        na, nb = int(XA.shape[0]), int(XB.shape[0])
        if same and (XA.data_ptr() != XB.data_ptr() or na != nb):
            raise ValueError("gpr_cov: same=True takes one array as XA and XB")
        if out is None:
            out = torch.empty(na, nb, dtype=torch.float64, device=XA.device)
        assert tuple(out.shape) == (na, nb) and out.dtype == torch.float64 and out.is_contiguous(), (na, nb)
        rc = self.lib.gpsa_gpr_cov_f64(kd, _p(XA), na, _p(XB), nb, D, _p(theta), int(bool(amplitude)), int(bool(same)),
                                       float(jitter), _p(out), self._stream(XA))
        _lib.check(rc, "gpsa_gpr_cov_f64")
        return out

    def gpr_lml_grad(self, kind, X, theta, alpha, Kinv, amplitude=False, out=None):
        """gpsa_gpr_lml_grad_f64: dLML / d(log a, log l, log tau2) [3] fp64 from X [N, D], alpha = K^-1 Y [N, P] and
        Kinv [N, N]: 1/2 sum_ij (alpha alpha^T - P Kinv)_ij dK_ij, fused (nothing of N x N is written), fixed order."""
        kd, theta, D = self._gpr_args("gpr_lml_grad", kind, theta, X)
        N = int(X.shape[0])
        self._contiguous("gpr_lml_grad", torch.float64, alpha=(alpha, (N, "P >= 1")), Kinv=(Kinv, (N, N)))
        P = int(alpha.shape[1])
        if out is None:
            out = torch.empty(3, dtype=torch.float64, device=X.device)
        assert tuple(out.shape) == (3,) and out.dtype == torch.float64 and out.is_contiguous()
        nbytes = self._wsq("gpsa_gpr_lml_grad_workspace", N, P)
        ws = self._ws(nbytes, X)
        rc = self.lib.gpsa_gpr_lml_grad_f64(kd, _p(X), N, D, _p(theta), int(bool(amplitude)), _p(alpha), P, _p(Kinv),
                                            _p(out), _p(ws), nbytes, self._stream(X))
        _lib.check(rc, "gpsa_gpr_lml_grad_f64")
        return out

    def gpr_mean(self, kind, XS, X, theta, alpha, amplitude=False, out=None):
        """gpsa_gpr_mean_f64: [ns, P] = a k(XS, X) alpha, fp64, the kernel tile generated into the MFMA operand (no
        [ns, N] matrix); a row's result does not depend on the rows passed with it."""
        kd, theta, D = self._gpr_args("gpr_mean", kind, theta, XS, X)
        ns, N = int(XS.shape[0]), int(X.shape[0])
        self._contiguous("gpr_mean", torch.float64, alpha=(alpha, (N, "P >= 1")))
        P = int(alpha.shape[1])
        if out is None:
            out = torch.empty(ns, P, dtype=torch.float64, device=XS.device)
        assert tuple(out.shape) == (ns, P) and out.dtype == torch.float64 and out.is_contiguous(), (ns, P)
        rc = self.lib.gpsa_gpr_mean_f64(kd, _p(XS), ns, _p(X), N, D, _p(theta), int(bool(amplitude)), _p(alpha), P,
                                        _p(out), self._stream(XS))
        _lib.check(rc, "gpsa_gpr_mean_f64")
        return out

    # ------------------------------------------------------------------ optimal-transport alignment (csrc/ot.hip)
    OT_MODES = {"kl": 0, "euclidean": 1}

    def ot_dist(self, X, out=None):
        """gpsa_ot_dist_f64: X [n, D <= 4] fp64 -> [n, n] Euclidean distances, symmetric to the bit, zero diagonal"""
        self._contiguous("ot_dist", torch.float64, X=(X, ("n >= 1", "n >= 1")))
        n, D = int(X.shape[0]), int(X.shape[1])
        if D > 4:
            raise ValueError(f"ot_dist: D = {D}; 1 to 4 coordinates are supported")
        if out is None:
            out = torch.empty(n, n, dtype=torch.float64, device=X.device)
        self._contiguous("ot_dist", torch.float64, out=(out, (n, n)))
        _lib.check(self.lib.gpsa_ot_dist_f64(_p(X), n, D, _p(out), self._stream(X)), "gpsa_ot_dist_f64")
        return out

    def ot_sqmatvec(self, Cm, v):
        """gpsa_ot_sqmatvec_f64: [n] = sum_k Cm_ik^2 v_k for Cm [n, ncol], v [ncol] fp64"""
        self._contiguous("ot_sqmatvec", torch.float64, Cm=(Cm, ("n >= 1", "n >= 1")))
        n, ncol = int(Cm.shape[0]), int(Cm.shape[1])
        self._contiguous("ot_sqmatvec", torch.float64, v=(v, (ncol,)))
        out = torch.empty(n, dtype=torch.float64, device=Cm.device)
        _lib.check(self.lib.gpsa_ot_sqmatvec_f64(_p(Cm), n, ncol, _p(v), _p(out), self._stream(Cm)), "gpsa_ot_sqmatvec_f64")
        return out

    def ot_expr_rows(self, Y, mode="kl"):
        """gpsa_ot_expr_rows_f32: Y [n, P] fp32 -> (Pm [n, P], Lg [n, P], term [n] fp64, n_invalid [1] int64 on the device);
        "kl": Pm = (y + 0.01) / row sum, Lg = log Pm, term = sum Pm Lg; "euclidean": Pm = y, Lg is Pm, term = sum y^2"""
        if mode not in self.OT_MODES:
            raise ValueError(f"ot_expr_rows: dissimilarity must be one of {sorted(self.OT_MODES)}, not {mode!r}")
        self._contiguous("ot_expr_rows", torch.float32, Y=(Y, ("n >= 1", "P >= 1")))
        n, P = int(Y.shape[0]), int(Y.shape[1])
        Pm = torch.empty(n, P, dtype=torch.float64, device=Y.device)
        Lg = torch.empty_like(Pm) if mode == "kl" else None
        term = torch.empty(n, dtype=torch.float64, device=Y.device)
        bad = torch.empty(1, dtype=torch.int64, device=Y.device)
        nbytes = self._wsq("gpsa_ot_expr_rows_workspace", n)
        ws = self._ws(nbytes, Y)
        rc = self.lib.gpsa_ot_expr_rows_f32(self.OT_MODES[mode], _p(Y), n, P, _p(Pm), _p(Lg), _p(term), _p(bad), _p(ws),
                                            nbytes, self._stream(Y))
        _lib.check(rc, "gpsa_ot_expr_rows_f32")
        return Pm, (Pm if Lg is None else Lg), term, bad

    def ot_expr_cost(self, G, ra, rb=None, mode="kl"):
        """gpsa_ot_expr_cost_f64, in place over G [n, m]: "kl" M = ra_i - G_ij; "euclidean" M = max(0, ra_i + rb_j - 2 G_ij)"""
        if mode not in self.OT_MODES:
            raise ValueError(f"ot_expr_cost: dissimilarity must be one of {sorted(self.OT_MODES)}, not {mode!r}")
        self._contiguous("ot_expr_cost", torch.float64, G=(G, ("n >= 1", "n >= 1")))
        n, m = int(G.shape[0]), int(G.shape[1])
        self._contiguous("ot_expr_cost", torch.float64, ra=(ra, (n,)))
        if mode == "euclidean":
            self._contiguous("ot_expr_cost", torch.float64, rb=(rb, (m,)))
        else:
            rb = None
        rc = self.lib.gpsa_ot_expr_cost_f64(self.OT_MODES[mode], _p(G), n, m, _p(ra), _p(rb), self._stream(G))
        _lib.check(rc, "gpsa_ot_expr_cost_f64")
        return G

    def ot_cost(self, G, M, T, cA, cB, cAt, cBt, alpha, sums=None):
        """gpsa_ot_cost_f64, in place over G = C1 T C2 [n, m]: cost = (1 - alpha) M + 2 alpha (cA 1^T + 1 cB^T - 2 G);
        -> (G, sums [3] fp64 on the device: sum |cost|, <M, T>, <cAt 1^T + 1 cBt^T - 2 G, T>)"""
        self._contiguous("ot_cost", torch.float64, G=(G, ("n >= 1", "n >= 1")))
        n, m = int(G.shape[0]), int(G.shape[1])
        self._contiguous("ot_cost", torch.float64, M=(M, (n, m)), T=(T, (n, m)), cA=(cA, (n,)), cB=(cB, (m,)), cAt=(cAt, (n,)),
                         cBt=(cBt, (m,)))
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"ot_cost: alpha = {alpha} is outside [0, 1]")
        if sums is None:
            sums = torch.empty(3, dtype=torch.float64, device=G.device)
        self._contiguous("ot_cost", torch.float64, sums=(sums, (3,)))
        nbytes = self._wsq("gpsa_ot_cost_workspace", n, m)
        ws = self._ws(nbytes, G)
        rc = self.lib.gpsa_ot_cost_f64(_p(G), _p(M), _p(T), _p(cA), _p(cB), _p(cAt), _p(cBt), alpha, n, m, _p(sums), _p(ws),
                                       nbytes, self._stream(G))
        _lib.check(rc, "gpsa_ot_cost_f64")
        return G, sums

    def ot_sinkhorn(self, cost, loga, logb, eps, f, g, iters):
        """gpsa_ot_sinkhorn_f64: ``iters`` log-domain sweeps, f [n] and g [m] updated in place; eps [1] fp64 on the device"""
        self._contiguous("ot_sinkhorn", torch.float64, cost=(cost, ("n >= 1", "n >= 1")))
        n, m = int(cost.shape[0]), int(cost.shape[1])
        self._contiguous("ot_sinkhorn", torch.float64, loga=(loga, (n,)), logb=(logb, (m,)), eps=(eps, (1,)), f=(f, (n,)),
                         g=(g, (m,)))
        iters = int(iters)
        if iters < 0:
            raise ValueError(f"ot_sinkhorn: iters = {iters} is negative")
        nbytes = self._wsq("gpsa_ot_sinkhorn_workspace", n, m)
        ws = self._ws(nbytes, cost)
        rc = self.lib.gpsa_ot_sinkhorn_f64(_p(cost), n, m, _p(loga), _p(logb), _p(eps), _p(f), _p(g), iters, _p(ws), nbytes,
                                           self._stream(cost))
        _lib.check(rc, "gpsa_ot_sinkhorn_f64")
        return f, g

    def ot_plan(self, cost, f, g, a, b, eps, T):
        """gpsa_ot_plan_f64: T_ij = a_i b_j exp((f_i + g_j - cost_ij) / eps) written over T (the previous plan) ->
        (T, rowsum [n], colsum [m], sums [3]: |T 1 - a|_1, |T^T 1 - b|_1, |T - T_old|_1)"""
        self._contiguous("ot_plan", torch.float64, cost=(cost, ("n >= 1", "n >= 1")))
        n, m = int(cost.shape[0]), int(cost.shape[1])
        self._contiguous("ot_plan", torch.float64, f=(f, (n,)), g=(g, (m,)), a=(a, (n,)), b=(b, (m,)), eps=(eps, (1,)),
                         T=(T, (n, m)))
        rowsum = torch.empty(n, dtype=torch.float64, device=cost.device)
        colsum = torch.empty(m, dtype=torch.float64, device=cost.device)
        sums = torch.empty(3, dtype=torch.float64, device=cost.device)
        nbytes = self._wsq("gpsa_ot_plan_workspace", n, m)
        ws = self._ws(nbytes, cost)
        rc = self.lib.gpsa_ot_plan_f64(_p(cost), n, m, _p(f), _p(g), _p(a), _p(b), _p(eps), _p(T), _p(rowsum), _p(colsum),
                                       _p(sums), _p(ws), nbytes, self._stream(cost))
        _lib.check(rc, "gpsa_ot_plan_f64")
        return T, rowsum, colsum, sums

    def chol_inv_blocked(self, A):
        """gpsa_chol_inv_blocked_f64 for ONE matrix A [N, N] fp64 of any size (not modified) -> L^-1 [N, N] (upper part
        zero), logdet [1] = log det A, info [1] int32 (0, or the 1-based column where the factorisation broke down)"""
        A = self._c(A)
        N = int(A.shape[-1])
        Linv = torch.empty_like(A)
        logdet = torch.empty(1, dtype=torch.float64, device=A.device)
        info = torch.empty(1, dtype=torch.int32, device=A.device)
        nbytes = self._wsq("gpsa_chol_inv_blocked_workspace", N, 1)
        ws = self._ws(nbytes, A)
        rc = self.lib.gpsa_chol_inv_blocked_f64(_p(A), _p(Linv), N, 1, _p(logdet), _p(info), _p(ws), ws.numel(),
                                                self._stream(A))
        _lib.check(rc, "gpsa_chol_inv_blocked_f64")
        return Linv, logdet, info

    # ------------------------------------------------------------------ count preprocessing (csrc/counts.hip)
    COUNT_MODES ={"pearson": 0, "nb_deviance": 1, "poisson_deviance": 2, "log1p": 3}

    @staticmethod
    def _count_matrix(Y, what):
        if Y.dim() != 2 or Y.shape[0] < 1 or Y.shape[1] < 1 or Y.dtype != torch.float32 or not Y.is_contiguous():
            raise ValueError(f"{what}: Y must be a contiguous fp32 [N >= 1, P >= 1], not {Y.dtype} {tuple(Y.shape)}")
        return int(Y.shape[0]), int(Y.shape[1])

    @staticmethod
    def _count_out(out, N, P, what):
        if tuple(out.shape) != (N, P) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous fp32 [{N}, {P}], not {out.dtype} {tuple(out.shape)}")

    def _count_ws(self, N, P, like):
        nbytes = self._wsq("gpsa_count_workspace", N, P)
        return self._ws(nbytes, like), nbytes

    @staticmethod
    def _margin_outputs(N, P, dev):
        f, i = torch.float64, torch.int64  # row_sum, col_sum, row_nnz, col_nnz, n_invalid
        return tuple(torch.empty(n, dtype=dt, device=dev) for n, dt in ((N, f), (P, f), (N, i), (P, i), (1, i)))

    @staticmethod
    def _view_offsets(what, view_off, N):
        off = [int(v) for v in view_off]  # V + 1 of them
        if len(off) < 2 or off[0] != 0 or off[-1] != N or any(b <= a for a, b in zip(off, off[1:])):
            raise ValueError(f"{what}: view_off {off} must rise strictly from 0 to N = {N}")
        return off, len(off) - 1

    def count_margins(self, Y):
        """gpsa_count_margins_f32: one read of Y [N, P] fp32 -> (row_sum [N] fp64, col_sum [P] fp64, row_nnz [N] int64,
        col_nnz [P] int64, n_invalid [1] int64 on the device: the entries that are NaN, +-inf or < 0)"""
        N, P = self._count_matrix(Y, "count_margins")
        out = self._margin_outputs(N, P, Y.device)
        ws, nbytes = self._count_ws(N, P, Y)
        rc = self.lib.gpsa_count_margins_f32(_p(Y), N, P, *map(_p, out), _p(ws), nbytes, self._stream(Y))
        _lib.check(rc, "gpsa_count_margins_f32")
        return out

    def count_deviance(self, Y, log_sz):
        """gpsa_count_deviance_f32: (ll_sat, abs_sat) [P] fp64 with ll_sat[g] = sum_i y log y - y log_sz_i and
        abs_sat[g] = sum_i |y log y| + |y log_sz_i|; log_sz [N] fp64"""
        N, P = self._count_matrix(Y, "count_deviance")
        if log_sz.dim() != 1 or log_sz.shape[0] != N:
            raise ValueError(f"count_deviance: log_sz has shape {tuple(log_sz.shape)}, [{N}] is needed")
        log_sz = self._f64(log_sz)
        ll, ab = (torch.empty(P, dtype=torch.float64, device=Y.device) for _ in range(2))
        ws, nbytes = self._count_ws(N, P, Y)
        rc = self.lib.gpsa_count_deviance_f32(_p(Y), N, P, _p(log_sz), _p(ll), _p(ab), _p(ws), nbytes, self._stream(Y))
        _lib.check(rc, "gpsa_count_deviance_f32")
        return ll, ab

    def count_transform(self, Y, mode, row_sum, col_sum=None, total=1.0, theta=1.0, clip=0.0, target=1.0, out=None):
        """gpsa_count_transform_f32: ``mode`` "pearson" | "nb_deviance" | "poisson_deviance" | "log1p", elementwise in
        fp64, rounded once to fp32 -> [N, P] fp32.  ``out`` may be Y itself."""
        N, P = self._count_matrix(Y, "count_transform")
        if mode not in self.COUNT_MODES:
            raise ValueError(f"count_transform: mode must be one of {sorted(self.COUNT_MODES)}, not {mode!r}")
        if row_sum.dim() != 1 or row_sum.shape[0] != N:
            raise ValueError(f"count_transform: row_sum has shape {tuple(row_sum.shape)}, [{N}] is needed")
        if mode != "log1p" and (col_sum is None or col_sum.dim() != 1 or col_sum.shape[0] != P):
            raise ValueError(f"count_transform: col_sum must be [{P}] for mode {mode!r}")
        row_sum = self._f64(row_sum)
        col_sum = None if mode == "log1p" else self._f64(col_sum)
        if out is None:
            out = torch.empty_like(Y)
        self._count_out(out, N, P, "count_transform")
        rc = self.lib.gpsa_count_transform_f32(self.COUNT_MODES[mode], _p(Y), N, P, _p(row_sum), _p(col_sum), float(total),
                                               float(theta), float(clip), float(target), _p(out), self._stream(Y))
        _lib.check(rc, "gpsa_count_transform_f32")
        return out

    def standardize_views(self, Y, view_off, out=None):
        """gpsa_standardize_views_f32: (y - mean) / std per (view, column) over the row ranges view_off (a list of V + 1
        ints, 0 ... N) -> (out [N, P] fp32, n_constant [V] int64 on the device); a column constant within a view: 0"""
        N, P = self._count_matrix(Y, "standardize_views")
        off, V = self._view_offsets("standardize_views", view_off, N)
        if out is None:
            out = torch.empty_like(Y)
        self._count_out(out, N, P, "standardize_views")
        nconst = torch.empty(V, dtype=torch.int64, device=Y.device)
        ws, nbytes = self._count_ws(N, P, Y)
        rc = self.lib.gpsa_standardize_views_f32(_p(Y), N, P, (C.c_longlong * (V + 1))(*off), V, _p(out), _p(nconst),
                                                 _p(ws), nbytes, self._stream(Y))
        _lib.check(rc, "gpsa_standardize_views_f32")
        return out, nconst

    # ------------------------------------------------------------------ ... from a CSR matrix (csrc/counts_sparse.hip)
    @staticmethod
    def _csr_arrays(crow, col, val, N, P, what):
        """crow [N + 1] int64, col [nnz] int32, val [nnz] fp32, contiguous, on one device -> nnz"""
        N, P = int(N), int(P)
        ok = (N >= 1 and P >= 1 and crow.dtype == torch.int64 and tuple(crow.shape) == (N + 1,) and col.dtype == torch.int32
              and col.dim() == 1 and val.dtype == torch.float32 and val.shape == col.shape
              and crow.is_contiguous() and col.is_contiguous() and val.is_contiguous())
        if not ok:
            raise ValueError(f"{what}: a CSR matrix [{N}, {P}] needs contiguous crow int64 [{N + 1}], col int32 [nnz] and "
                             f"val fp32 [nnz], not {crow.dtype} {tuple(crow.shape)}, {col.dtype} {tuple(col.shape)}, "
                             f"{val.dtype} {tuple(val.shape)}")
        return int(col.numel())

    @staticmethod
    def _csr_keep(keep, N, what):
        if keep is None:
            return None
        if tuple(keep.shape) != (N,) or keep.dtype not in (torch.bool, torch.uint8) or not keep.is_contiguous():
            raise ValueError(f"{what}: keep must be a contiguous bool / uint8 [{N}], not {keep.dtype} {tuple(keep.shape)}")
        return keep.view(torch.uint8) if keep.dtype == torch.bool else keep

    def _csr_ws(self, N, P, like):
        nbytes = self._wsq("gpsa_count_csr_workspace", N, P)
        return self._ws(nbytes, like), nbytes

    def csr_check(self, crow, col, val, N, P):
        """gpsa_csr_check -> [4] int64 on the device: crow violations, column indices outside [0, P), places inside a
        row where the column index does not strictly increase, stored zeros"""
        nnz = self._csr_arrays(crow, col, val, N, P, "csr_check")
        out = torch.empty(4, dtype=torch.int64, device=crow.device)
        ws, nbytes = self._csr_ws(N, P, crow)
        rc = self.lib.gpsa_csr_check(_p(crow), _p(col), _p(val), N, P, nnz, _p(out), _p(ws), nbytes, self._stream(crow))
        _lib.check(rc, "gpsa_csr_check")
        return out

    def count_margins_csr(self, crow, col, val, N, P, keep=None):
        """gpsa_count_margins_csr_f32: count_margins of the CSR matrix [N, P]; ``keep`` [N] bool: rows to take"""
        nnz = self._csr_arrays(crow, col, val, N, P, "count_margins_csr")
        keep = self._csr_keep(keep, N, "count_margins_csr")
        out = self._margin_outputs(N, P, crow.device)
        ws, nbytes = self._csr_ws(N, P, crow)
        rc = self.lib.gpsa_count_margins_csr_f32(_p(crow), _p(col), _p(val), _p(keep), N, P, nnz, *map(_p, out), _p(ws),
                                                 nbytes, self._stream(crow))
        _lib.check(rc, "gpsa_count_margins_csr_f32")
        return out

    def count_deviance_csr(self, crow, col, val, N, P, log_sz, keep=None):
        """gpsa_count_deviance_csr_f32: count_deviance of the CSR matrix; log_sz [N] fp64 by the original row"""
        nnz = self._csr_arrays(crow, col, val, N, P, "count_deviance_csr")
        keep = self._csr_keep(keep, N, "count_deviance_csr")
        if log_sz.dim() != 1 or log_sz.shape[0] != N:
            raise ValueError(f"count_deviance_csr: log_sz has shape {tuple(log_sz.shape)}, [{N}] is needed")
        log_sz = self._f64(log_sz)
        ll, ab = (torch.empty(P, dtype=torch.float64, device=crow.device) for _ in range(2))
        ws, nbytes = self._csr_ws(N, P, crow)
        rc = self.lib.gpsa_count_deviance_csr_f32(_p(crow), _p(col), _p(val), _p(keep), N, P, nnz, _p(log_sz), _p(ll),
                                                  _p(ab), _p(ws), nbytes, self._stream(crow))
        _lib.check(rc, "gpsa_count_deviance_csr_f32")
        return ll, ab

    def csr_gather_dense(self, crow, col, val, N, P, rows, slot, G):
        """gpsa_csr_gather_dense_f32: rows [n_rows] int64, slot [P] int32 (the output column of each gene or -1) ->
        [n_rows, G] fp32 with zeros where nothing is stored"""
        nnz = self._csr_arrays(crow, col, val, N, P, "csr_gather_dense")
        G = int(G)
        if rows.dtype != torch.int64 or rows.dim() != 1 or rows.numel() < 1 or not rows.is_contiguous():
            raise ValueError(f"csr_gather_dense: rows must be a contiguous int64 [n_rows >= 1], not {rows.dtype} "
                             f"{tuple(rows.shape)}")
        if slot.dtype != torch.int32 or tuple(slot.shape) != (P,) or not slot.is_contiguous() or not 1 <= G <= P:
            raise ValueError(f"csr_gather_dense: slot must be a contiguous int32 [{P}] and 1 <= G <= {P}, not {slot.dtype} "
                             f"{tuple(slot.shape)}, G = {G}")
        out = torch.empty(rows.numel(), G, dtype=torch.float32, device=crow.device)
        rc = self.lib.gpsa_csr_gather_dense_f32(_p(crow), _p(col), _p(val), N, P, nnz, _p(rows), rows.numel(), _p(slot), G,
                                                _p(out), self._stream(crow))
        _lib.check(rc, "gpsa_csr_gather_dense_f32")
        return out

    # ------------------------------------------------------------------ spatial autocorrelation (csrc/autocorr.hip)
    GRAPH_KINDS = {"none": 0, "union": 1, "mutual": 2}
    AUTOCORR_MODES = {"moran": 0, "geary": 1}

    @staticmethod
    def _graph_arrays(crow, col, w, n, what):
        """crow [n + 1] int64, col [nnz] int32, w [nnz] fp64, contiguous, on a device -> nnz"""
        n = int(n)
        ok = (n >= 1 and all(torch.is_tensor(t) for t in (crow, col, w)) and crow.dtype == torch.int64
              and tuple(crow.shape) == (n + 1,) and col.dtype == torch.int32 and col.dim() == 1
              and w.dtype == torch.float64 and w.shape == col.shape
              and crow.is_contiguous() and col.is_contiguous() and w.is_contiguous())
        if not ok:
            raise ValueError(f"{what}: a graph on {n} rows needs contiguous crow int64 [{n + 1}], col int32 [nnz] and "
                             f"w fp64 [nnz], not {describe(crow)}, {describe(col)}, {describe(w)}")
        for name, t in (("crow", crow), ("col", col), ("w", w)):
            if not t.is_cuda:
                raise ValueError(f"{what}: {name} is on device {str(t.device)!r}; the graph kernels run on the GPU only")
        return int(col.numel())

    def graph_merge(self, out_sorted, in_ptr, in_src, kind="none", row_standardize=True):
        """gpsa_graph_merge_count / _write: the kNN lists out_sorted [n, k] int32 (each row ascending) and, for "union" /
        "mutual", the in-lists in_src [n k] int32 at in_ptr [n + 1] int64 -> (crow [n + 1] int64, col [nnz] int32,
        w [nnz] fp64).  One host read (nnz) between the two passes."""
        if kind not in self.GRAPH_KINDS:
            raise ValueError(f"graph_merge: kind must be 'none', 'union' or 'mutual', not {kind!r}")
        code = self.GRAPH_KINDS[kind]
        if out_sorted.dim() != 2 or out_sorted.dtype != torch.int32 or not out_sorted.is_contiguous() \
                or out_sorted.shape[0] < 1 or out_sorted.shape[1] < 1:
            raise ValueError(f"graph_merge: out_sorted must be a contiguous int32 [n >= 1, k >= 1], not {out_sorted.dtype} "
                             f"{tuple(out_sorted.shape)}")
        n, k = (int(s) for s in out_sorted.shape)
        if code:
            if (in_ptr is None or in_src is None or in_ptr.dtype != torch.int64 or tuple(in_ptr.shape) != (n + 1,)
                    or in_src.dtype != torch.int32 or tuple(in_src.shape) != (n * k,) or not in_ptr.is_contiguous()
                    or not in_src.is_contiguous()):
                raise ValueError(f"graph_merge: kind {kind!r} needs in_ptr int64 [{n + 1}] and in_src int32 [{n * k}]")
        else:
            in_ptr = in_src = None
        dev, st = out_sorted.device, self._stream(out_sorted)
        crow = torch.empty(n + 1, dtype=torch.int64, device=dev)
        rc = self.lib.gpsa_graph_merge_count(_p(out_sorted), _p(in_ptr), _p(in_src), n, k, code, _p(crow), st)
        _lib.check(rc, "gpsa_graph_merge_count")
        nnz = int(crow[n])
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        w = torch.empty(nnz, dtype=torch.float64, device=dev)
        rc = self.lib.gpsa_graph_merge_write(_p(out_sorted), _p(in_ptr), _p(in_src), n, k, code, int(bool(row_standardize)),
                                             _p(crow), nnz, _p(col), _p(w), st)
        _lib.check(rc, "gpsa_graph_merge_write")
        return crow, col, w

    def graph_check(self, crow, col, w, n):
        """gpsa_graph_check_f64 -> [5] int64 on the device: crow violations, columns outside [0, n), places where the
        column does not strictly increase within a row, self edges, weights that are not finite or < 0"""
        nnz = self._graph_arrays(crow, col, w, n, "graph_check")
        out = torch.empty(5, dtype=torch.int64, device=crow.device)
        nbytes = self._wsq("gpsa_graph_workspace", int(n))
        ws = self._ws(nbytes, crow)
        rc = self.lib.gpsa_graph_check_f64(_p(crow), _p(col), _p(w), int(n), nnz, _p(out), _p(ws), nbytes, self._stream(crow))
        _lib.check(rc, "gpsa_graph_check_f64")
        return out

    def graph_sums(self, crow, col, w, n, tptr, tperm):
        """gpsa_graph_sums_f64 -> [3] fp64 on the device: S0, S1, S2; tperm [nnz] int64: the entries' positions in the
        order of a stable sort by column, tptr [n + 1] int64: where each column starts in it"""
        nnz = self._graph_arrays(crow, col, w, n, "graph_sums")
        n = int(n)
        if (tptr.dtype != torch.int64 or tuple(tptr.shape) != (n + 1,) or tperm.dtype != torch.int64
                or tuple(tperm.shape) != (nnz,) or not tptr.is_contiguous() or not tperm.is_contiguous()):
            raise ValueError(f"graph_sums: tptr must be int64 [{n + 1}] and tperm int64 [{nnz}], not {tptr.dtype} "
                             f"{tuple(tptr.shape)}, {tperm.dtype} {tuple(tperm.shape)}")
        out = torch.empty(3, dtype=torch.float64, device=crow.device)
        nbytes = self._wsq("gpsa_graph_workspace", n)
        ws = self._ws(nbytes, crow)
        rc = self.lib.gpsa_graph_sums_f64(_p(crow), _p(col), _p(w), _p(tptr), _p(tperm), n, nnz, _p(out), _p(ws), nbytes,
                                          self._stream(crow))
        _lib.check(rc, "gpsa_graph_sums_f64")
        return out

    def autocorr_perm(self, Z, crow, col, w, perms, mode="moran", out=None):
        """gpsa_autocorr_perm_f64: Z [n, P] fp64 (centred columns), the graph in CSR, perms [R, n] int32 ->
        (num [R, P] fp64, n_bad [1] int64 on the device: the entries of perms and col outside [0, n), none of which is
        followed).  ``mode`` "moran": sum_i z_i sum_j w_ij z_j, "geary": sum_ij w_ij (z_i - z_j)^2, z = Z's rows taken
        through the permutation.  ``out``: num, preallocated."""
        if mode not in self.AUTOCORR_MODES:
            raise ValueError(f"autocorr_perm: mode must be 'moran' or 'geary', not {mode!r}")
        if Z.dim() != 2 or Z.dtype != torch.float64 or not Z.is_contiguous() or Z.shape[0] < 1 or Z.shape[1] < 1:
            raise ValueError(f"autocorr_perm: Z must be a contiguous fp64 [n >= 1, P >= 1], not {Z.dtype} {tuple(Z.shape)}")
        n, P = (int(s) for s in Z.shape)
        nnz = self._graph_arrays(crow, col, w, n, "autocorr_perm")
        if perms.dim() != 2 or perms.dtype != torch.int32 or not perms.is_contiguous() or perms.shape[0] < 1 \
                or perms.shape[1] != n:
            raise ValueError(f"autocorr_perm: perms must be a contiguous int32 [R >= 1, {n}], not {perms.dtype} "
                             f"{tuple(perms.shape)}")
        R = int(perms.shape[0])
        if out is None:
            out = torch.empty(R, P, dtype=torch.float64, device=Z.device)
        assert tuple(out.shape) == (R, P) and out.dtype == torch.float64 and out.is_contiguous(), (R, P)
        n_bad = torch.empty(1, dtype=torch.int64, device=Z.device)
        nbytes = self._wsq("gpsa_autocorr_perm_workspace", n, P, R)
        ws = self._ws(nbytes, Z)
        rc = self.lib.gpsa_autocorr_perm_f64(_p(Z), n, P, _p(crow), _p(col), _p(w), nnz, _p(perms), R,
                                             self.AUTOCORR_MODES[mode], _p(out), _p(n_bad), _p(ws), nbytes, self._stream(Z))
        _lib.check(rc, "gpsa_autocorr_perm_f64")
        return out, n_bad

    # ------------------------------------------------------------------ histology images (csrc/image.hip)
    @staticmethod
    def _image(img, what):
        """img [H, W, C] contiguous uint8 or fp32 on a device, C in 1..4 -> (H, W, C, "u8" | "f32")"""
        if (not torch.is_tensor(img) or img.dim() != 3 or img.dtype not in (torch.uint8, torch.float32)
                or not img.is_contiguous() or min(img.shape) < 1 or img.shape[2] > 4):
            raise ValueError(f"{what}: img must be a contiguous uint8 or fp32 [H >= 1, W >= 1, C in 1..4], not "
                             f"{describe(img)}")
        if not img.is_cuda:
            raise ValueError(f"{what}: img is on {img.device}; the image kernels run on the device")
        H, W, Cn = (int(s) for s in img.shape)
        return H, W, Cn, "u8" if img.dtype == torch.uint8 else "f32"

    def image_select(self, img, bin=1, background=None, bbox=None):
        """gpsa_image_select_count_* / _write_*: the pixels of img [H, W, C] (uint8: u / 255; or fp32), reduced by the mean
        over ``bin`` x ``bin`` blocks, that are not ``background`` (every channel rounds to it at one decimal; None: the
        rule is off) and lie strictly inside ``bbox`` = (xmin, xmax, ymin, ymax) (None: off), in row-major order ->
        (coords [n, 2] fp32 = (x, y), pixels [n, C] fp32, counts [3] int64 on the HOST = (kept, background, outside)).
        One small host read (the counts) between the two passes; n = 0 skips the second."""
        H, W, Cn, sfx = self._image(img, "image_select")
        if isinstance(bin, bool) or int(bin) != bin or not 1 <= bin <= 64 or bin > min(H, W):
            raise ValueError(f"image_select: bin must be an integer in 1..64 and at most min(H, W) = {min(H, W)}, "
                             f"not {bin!r}")
        bin = int(bin)
        if (H // bin) * (W // bin) >= 2 ** 31:
            raise ValueError(f"image_select: {H // bin} x {W // bin} output pixels; fewer than 2^31 are supported "
                             "(raise bin)")
        has_bg = background is not None
        bg = float(background) if has_bg else 0.0
        if has_bg and bg != bg:
            raise ValueError("image_select: background is NaN (None switches the rule off)")
        box = None
        if bbox is not None:
            vals = [float(v) for v in bbox]
            if len(vals) != 4 or any(v != v for v in vals):
                raise ValueError(f"image_select: bbox must be four numbers (xmin, xmax, ymin, ymax) without a NaN, "
                                 f"not {bbox!r}")
            box = (C.c_double * 4)(*vals)
        nbytes = self._wsq("gpsa_image_select_workspace", H, W, bin)
        ws = self._ws(nbytes, img)
        args = (_p(img), H, W, Cn, bin, int(has_bg), bg, int(box is not None), box, _p(ws), nbytes)
        name = f"gpsa_image_select_count_{sfx}"
        _lib.check(getattr(self.lib, name)(*args, self._stream(img)), name)
        counts = ws[:24].view(torch.int64).cpu()
        n = int(counts[0])
        coords = torch.empty(n, 2, dtype=torch.float32, device=img.device)
        pixels = torch.empty(n, Cn, dtype=torch.float32, device=img.device)
        if n:
            name = f"gpsa_image_select_write_{sfx}"
            _lib.check(getattr(self.lib, name)(*args, _p(coords), _p(pixels), n, self._stream(img)), name)
        return coords, pixels, counts

    def image_sample(self, img, xy, order=1, fill=float("nan"), out=None):
        """gpsa_image_sample_*: img [H, W, C] read at xy [n, 2] fp64 = (x, y) in pixel coordinates (x the column) ->
        (out [n, C] fp32, valid [n] uint8); order 1 bilinear in fp64, order 0 nearest; a row outside
        [0, W - 1] x [0, H - 1] (or NaN) is ``fill`` and valid = 0.  ``out``: the same two, preallocated."""
        H, W, Cn, sfx = self._image(img, "image_sample")
        if order not in (0, 1) or isinstance(order, bool):
            raise ValueError(f"image_sample: order must be 0 (nearest) or 1 (bilinear), not {order!r}")
        if not torch.is_tensor(xy) or xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
            shape = tuple(xy.shape) if torch.is_tensor(xy) else type(xy).__name__
            raise ValueError(f"image_sample: xy has shape {shape}, [n >= 1, 2] is needed")
        if xy.device != img.device:
            raise ValueError(f"image_sample: xy is on {xy.device}, img on {img.device}")
        xy = self._f64(xy)
        n = int(xy.shape[0])
        if n >= 2 ** 31:
            raise ValueError(f"image_sample: n = {n} rows; fewer than 2^31 per call are supported")
        if out is None:
            out = (torch.empty(n, Cn, dtype=torch.float32, device=img.device),
                   torch.empty(n, dtype=torch.uint8, device=img.device))
        vals, valid = out
        for t, sh, dt in ((vals, (n, Cn), torch.float32), (valid, (n,), torch.uint8)):
            assert tuple(t.shape) == sh and t.dtype == dt and t.is_contiguous(), sh
        name = f"gpsa_image_sample_{sfx}"
        rc = getattr(self.lib, name)(_p(img), H, W, Cn, _p(xy), n, int(order), float(fill), _p(vals), _p(valid),
                                     self._stream(img))
        _lib.check(rc, name)
        return vals, valid

    # ------------------------------------------------------------------ per-view column moments (csrc/moments.hip)
    MOMENT_MODES ={"identity": 0, "expm1": 1, "normalize": 2}

    def _moment_args(self, what, mode, N, view_off, scale):
        """-> (mode number, offsets, V, scale as a contiguous fp64 [N] or None)"""
        if mode not in self.MOMENT_MODES:
            raise ValueError(f"{what}: mode must be one of {sorted(self.MOMENT_MODES)}, not {mode!r}")
        off, V = self._view_offsets(what, view_off, N)
        if mode == "normalize":
            if scale is None or scale.dim() != 1 or scale.shape[0] != N:
                raise ValueError(f"{what}: mode 'normalize' needs scale [{N}]")
            scale = self._f64(scale)
        else:
            scale = None
        return self.MOMENT_MODES[mode], off, V, scale

    @staticmethod
    def _moment_outputs(V, P, dev):
        s1, s2, ab = (torch.empty(V, P, dtype=torch.float64, device=dev) for _ in range(3))
        return s1, s2, ab, torch.empty(1, dtype=torch.int64, device=dev)

    def column_moments(self, Y, mode, view_off, scale=None, own_workspace=False):
        """gpsa_column_moments_f32: Y [N, P] fp32, ``mode`` "identity" | "expm1" | "normalize" (t = y, expm1(y), y scale_i),
        view_off a list of V + 1 ints 0 ... N -> (s1, s2, abs1 [V, P] fp64: the sums of t, t^2, |t| per (view, column),
        n_nonfinite [1] int64 on the device).  ``own_workspace``: the planes live in a buffer of this call, freed with it,
        not in the stream's shared scratch (which keeps its largest size)."""
        N, P = self._count_matrix(Y, "column_moments")
        m, off, V, scale = self._moment_args("column_moments", mode, N, view_off, scale)
        s1, s2, ab, bad = self._moment_outputs(V, P, Y.device)
        nbytes = self._wsq("gpsa_column_moments_workspace", N, P, V)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=Y.device) if own_workspace else self._ws(nbytes, Y)
        rc = self.lib.gpsa_column_moments_f32(m, _p(Y), N, P, _p(scale), (C.c_longlong * (V + 1))(*off), V, _p(s1), _p(s2),
                                              _p(ab), _p(bad), _p(ws), nbytes, self._stream(Y))
        _lib.check(rc, "gpsa_column_moments_f32")
        return s1, s2, ab, bad

    def column_moments_csr(self, crow, col, val, N, P, mode, view_off, scale=None, keep=None):
        """gpsa_column_moments_csr_f32: column_moments of the CSR matrix [N, P] over its stored entries; scale [N] by the
        original row; ``keep`` [N] bool: rows to take"""
        nnz = self._csr_arrays(crow, col, val, N, P, "column_moments_csr")
        N, P = int(N), int(P)
        keep = self._csr_keep(keep, N, "column_moments_csr")
        m, off, V, scale = self._moment_args("column_moments_csr", mode, N, view_off, scale)
        s1, s2, ab, bad = self._moment_outputs(V, P, crow.device)
        nbytes = self._wsq("gpsa_column_moments_csr_workspace", N, P, V)
        ws = self._ws(nbytes, crow)
        rc = self.lib.gpsa_column_moments_csr_f32(m, _p(crow), _p(col), _p(val), _p(keep), N, P, nnz, _p(scale),
                                                  (C.c_longlong * (V + 1))(*off), V, _p(s1), _p(s2), _p(ab), _p(bad),
                                                  _p(ws), nbytes, self._stream(crow))
        _lib.check(rc, "gpsa_column_moments_csr_f32")
        return s1, s2, ab, bad

    # ------------------------------------------------------------------ expression PCA (csrc/pca.hip)
    # the Gram kernel's tile edge, the rows of its chunk, the cap on its row groups, the tile pairs from which the row
    # split is off; the projection's cap on the components
    PCA_TILE, PCA_ROW_CHUNK, PCA_MAX_GROUPS, PCA_FILL, PCA_MAX_K = 64, 32, 32, 256, 128

    def _pca_args(self, what, Y, mean, inv_scale, view_off):
        """-> (N, P, offsets, V, mean, inv_scale): mean / inv_scale contiguous fp64 [V, P] on Y's device"""
        N, P = self._count_matrix(Y, what)
        off, V = self._view_offsets(what, view_off, N)
        for t, name in ((mean, "mean"), (inv_scale, "inv_scale")):
            if t is None and name == "inv_scale":
                continue
            if not torch.is_tensor(t) or tuple(t.shape) != (V, P) or t.dtype != torch.float64 or not t.is_contiguous() \
                    or t.device != Y.device:
                got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"{what}: {name} must be a contiguous fp64 [{V}, {P}] on {Y.device}, not {got}")
        return N, P, off, V, mean, inv_scale

    def pca_gram_groups(self, N, P):
        """the row groups gpsa_pca_gram_f32 cuts a view into, at most: a function of (N, P) alone"""
        return self._wsq("gpsa_pca_gram_groups", int(N), int(P))

    def pca_gram_workspace(self, N, P, V=1):
        return self._wsq("gpsa_pca_gram_workspace", int(N), int(P), int(V))

    def pca_gram(self, Y, mean, view_off, inv_scale=None, out=None):
        """gpsa_pca_gram_f32: G [P, P] fp64 = sum_i z_ia z_ib with z = (y - mean[v]) * inv_scale[v] formed in fp64 from
        Y [N, P] fp32; mean / inv_scale [V, P] fp64, view_off a list of V + 1 ints 0 ... N.  Symmetric to the bit, the
        same bits on a repeated call.  The workspace is this call's own and is freed with it."""
        N, P, off, V, mean, inv_scale = self._pca_args("pca_gram", Y, mean, inv_scale, view_off)
        if N < 2:
            raise ValueError(f"pca_gram: Y has {N} row; at least 2 are needed")
        if out is None:
            out = torch.empty(P, P, dtype=torch.float64, device=Y.device)
        assert tuple(out.shape) == (P, P) and out.dtype == torch.float64 and out.is_contiguous(), (P, P)
        nbytes = self.pca_gram_workspace(N, P, V)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=Y.device) if nbytes else None
        rc = self.lib.gpsa_pca_gram_f32(_p(Y), N, P, _p(mean), _p(inv_scale), (C.c_longlong * (V + 1))(*off), V, _p(out),
                                        _p(ws), nbytes, self._stream(Y))
        _lib.check(rc, "gpsa_pca_gram_f32")
        return out

    def pca_project(self, Y, mean, view_off, comp, inv_scale=None, out_dtype=torch.float32, out=None):
        """gpsa_pca_project_f32: scores [N, k] = z comp^T with z as in ``pca_gram`` and comp [k <= 128, P] fp64; fp64
        accumulation, stored as fp32 (rounded once) or fp64.  A row's result does not depend on the other rows."""
        N, P, off, V, mean, inv_scale = self._pca_args("pca_project", Y, mean, inv_scale, view_off)
        if not torch.is_tensor(comp) or comp.dim() != 2 or comp.shape[1] != P or not 1 <= comp.shape[0] <= self.PCA_MAX_K \
                or comp.dtype != torch.float64 or not comp.is_contiguous() or comp.device != Y.device:
            raise ValueError(f"pca_project: comp must be a contiguous fp64 [1 <= k <= {self.PCA_MAX_K}, {P}] on "
                             f"{Y.device}, not {describe(comp)}")
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError(f"pca_project: out_dtype must be torch.float32 or torch.float64, not {out_dtype}")
        k = int(comp.shape[0])
        if out is None:
            out = torch.empty(N, k, dtype=out_dtype, device=Y.device)
        assert tuple(out.shape) == (N, k) and out.dtype == out_dtype and out.is_contiguous(), (N, k)
        rc = self.lib.gpsa_pca_project_f32(_p(Y), N, P, _p(mean), _p(inv_scale), (C.c_longlong * (V + 1))(*off), V,
                                           _p(comp), k, _p(out), int(out_dtype == torch.float64), self._stream(Y))
        _lib.check(rc, "gpsa_pca_project_f32")
        return out

    def warp_sample_fwd(self, meanT, v, q, var_u, X, slopes, intercept, eps):
        """-> Gmean [n,D], Gs [S,n,D] (fp32), bad [blocks] (int32 flags), Gs64 [S,n,D] (the draws unrounded)"""
        meanT, v, q, eps = self._c(meanT), self._c(v), self._c(q), self._c(eps)
        var_u, X, slopes, intercept = (self._f32(t) for t in (var_u, X, slopes, intercept))
        D, n = meanT.shape
        S = eps.shape[0]
        Gmean = torch.empty(n, D, dtype=torch.float32, device=meanT.device)
        Gs = torch.empty(S, n, D, dtype=torch.float32, device=meanT.device)
        Gs64 = torch.empty(S, n, D, dtype=torch.float64, device=meanT.device)
        bad = torch.empty((n + 255) // 256, dtype=torch.int32, device=meanT.device)
        rc = self.lib.gpsa_warp_sample_fwd(_p(meanT), _p(v), _p(q), _p(var_u), _p(X), _p(slopes),
                                           _p(intercept), _p(eps), n, D, S, _p(Gmean), _p(Gs), _p(Gs64),
                                           _p(bad), self._stream(meanT))
        _lib.check(rc, "gpsa_warp_sample_fwd")
        return Gmean, Gs, bad, Gs64

    def warp_sample_bwd(self, dGmean, dGs, eps, var_u, X, dGs64=None):
        """-> dmeanT, g [D,n], qbar [n] (fp64); dvar_u [1], dslopes [D,D], dintercept [D] (fp32).
        The draws' gradient is dGs (fp32, may be None) + dGs64 (fp64, may be None)."""
        eps = self._c(eps)
        dGs = None if dGs is None else self._f32(dGs)
        dGs64 = None if dGs64 is None else self._c(dGs64)
        dGmean = None if dGmean is None else self._c(dGmean)
        var_u, X = self._f32(var_u), self._f32(X)
        S, n, D = eps.shape
        dev = eps.device
        f64, f32 = torch.float64, torch.float32
        dmeanT = torch.empty(D, n, dtype=f64, device=dev)
        g = torch.empty(D, n, dtype=f64, device=dev)
        qbar = torch.empty(n, dtype=f64, device=dev)
        dvar = torch.empty(1, dtype=f32, device=dev)
        dslopes = torch.empty(D, D, dtype=f32, device=dev)
        dint = torch.empty(D, dtype=f32, device=dev)
        ws = self._ws(8 * 21 * ((n + 255) // 256) + 64, eps)
        rc = self.lib.gpsa_warp_sample_bwd(_p(dGmean), _p(dGs), _p(dGs64), _p(eps), _p(var_u), _p(X), n, D, S,
                                           _p(dmeanT), _p(g), _p(qbar), _p(dvar), _p(dslopes), _p(dint),
                                           _p(ws), ws.numel(), self._stream(eps))
        _lib.check(rc, "gpsa_warp_sample_bwd")
        return dmeanT, g, qbar, dvar, dslopes, dint

    # ------------------------------------------------------------------ mean function at Z
    def mean_resid_fwd(self, Z, slopes, intercept, delta, scale=1.0):
        """-> mu_z = scale (Z slopes + intercept) [M,D] fp32, resid = delta - mu_z [M,D] fp64"""
        Z, slopes, intercept, delta = (self._f32(t) for t in (Z, slopes, intercept, delta))
        M, D = Z.shape
        mu = torch.empty(M, D, dtype=torch.float32, device=Z.device)
        resid = torch.empty(M, D, dtype=torch.float64, device=Z.device)
        rc = self.lib.gpsa_mean_resid_fwd(_p(Z), _p(slopes), _p(intercept), _p(delta), M, D, float(scale),
                                          _p(mu), _p(resid), self._stream(Z))
        _lib.check(rc, "gpsa_mean_resid_fwd")
        return mu, resid

    def mean_resid_bwd(self, dresid, Z, slopes, scale=1.0):
        """-> ddelta, dZ [M,D], dslopes [D,D], dintercept [D] (fp32)"""
        dresid = self._c(dresid if dresid.dtype == torch.float64 else dresid.double())
        Z, slopes = self._f32(Z), self._f32(slopes)
        M, D = Z.shape
        f32, dev = torch.float32, Z.device
        ddelta = torch.empty(M, D, dtype=f32, device=dev)
        dZ = torch.empty(M, D, dtype=f32, device=dev)
        dslopes = torch.empty(D, D, dtype=f32, device=dev)
        dint = torch.empty(D, dtype=f32, device=dev)
        rc = self.lib.gpsa_mean_resid_bwd(_p(dresid), _p(Z), _p(slopes), M, D, float(scale), _p(ddelta),
                                          _p(dZ), _p(dslopes), _p(dint), self._stream(Z))
        _lib.check(rc, "gpsa_mean_resid_bwd")
        return ddelta, dZ, dslopes, dint

    # ------------------------------------------------------------------ likelihood
    def loglik_fwd(self, F, Y, noise_u):
        F, Y = self._c(F), self._c(Y)
        S, N, P = F.shape
        out = torch.empty(1, dtype=torch.float64, device=F.device)
        ws = self._ws(8 * 4100, F)
        rc = self.lib.gpsa_loglik_fwd(_p(F), _p(Y), _p(noise_u), S, N, P, _p(out), _p(ws), ws.numel(),
                                      self._stream(F))
        _lib.check(rc, "gpsa_loglik_fwd")
        return out

    def loglik_bwd(self, F, Y, noise_u, gout):
        F, Y = self._c(F), self._c(Y)
        S, N, P = F.shape
        dF = torch.empty_like(F)
        dn = torch.empty(1, dtype=torch.float32, device=F.device)
        ws = self._ws(8 * 4100, F)
        rc = self.lib.gpsa_loglik_bwd(_p(F), _p(Y), _p(noise_u), _p(gout), S, N, P, _p(dF), _p(dn),
                                      _p(ws), ws.numel(), self._stream(F))
        _lib.check(rc, "gpsa_loglik_bwd")
        return dF, dn

    # ------------------------------------------------------------------ small helpers
    def bdot(self, A, B):
        """A, B: [batch, ...] or un-batched (broadcast): out[b] = <A[b], B[b]>"""
        nb = A.shape[0] if A.dim() == 3 else B.shape[0]
        A2 = self._c(A)
        B2 = self._c(B)
        n = A2.shape[-1] * A2.shape[-2]
        sA = n if A2.dim() == 3 else 0
        sB = n if B2.dim() == 3 else 0
        out = torch.empty(nb, dtype=A2.dtype, device=A2.device)
        ws = self._ws(8 * 32 * nb, A2)
        rc = self.lib.gpsa_bdot(_dt(A2), _p(A2), sA, _p(B2), sB, n, nb, _p(out), _p(ws), ws.numel(),
                                self._stream(A2))
        _lib.check(rc, "gpsa_bdot")
        return out

    # ------------------------------------------------------------------ KL terms (fp64)
    @staticmethod
    def _lstride(t):
        """(tensor usable as [L, M, M] with row-major M x M blocks, stride between blocks)"""
        M = t.shape[-1]
        if t.stride(-1) == 1 and t.stride(-2) == M:
            return t, t.stride(0)
        t = t.contiguous()
        return t, M * M

    def mvn_kl_fwd(self, Kinv, logdetK, Omega, logdetO, Dm):
        Omega, so = self._lstride(Omega)
        L, M = Omega.shape[0], Omega.shape[-1]
        Kinv, Dm = self._c(Kinv), self._c(Dm)
        kl = torch.empty(L, dtype=torch.float64, device=Kinv.device)
        KD = self.gemm(Kinv, Dm)
        rc = self.lib.gpsa_mvn_kl_fwd(_p(Kinv), _p(logdetK), _p(Omega), so, _p(logdetO), logdetO.stride(0),
                                      _p(Dm), _p(KD), M, L, _p(kl), self._stream(Kinv))
        _lib.check(rc, "gpsa_mvn_kl_fwd")
        return kl, KD

    def mvn_kl_bwd(self, Kuu, Kinv, Omega, Oinv, Dm, KD, g):
        Omega, so = self._lstride(Omega)
        Oinv, si = self._lstride(Oinv)
        L, M = Omega.shape[0], Omega.shape[-1]
        Kuu, Kinv, Dm, KD, g = self._c(Kuu), self._c(Kinv), self._c(Dm), self._c(KD), self._c(g)
        dev = Kinv.device
        dOm = torch.empty(L, M, M, dtype=torch.float64, device=dev)
        dDm = torch.empty(M, L, dtype=torch.float64, device=dev)
        Sp = torch.empty(M, M, dtype=torch.float64, device=dev)
        rc = self.lib.gpsa_mvn_kl_bwd(_p(Kuu), _p(Kinv), _p(Omega), so, _p(Oinv), si, _p(Dm), _p(KD), _p(g),
                                      M, L, _p(dOm), _p(dDm), _p(Sp), self._stream(Kinv))
        _lib.check(rc, "gpsa_mvn_kl_bwd")
        return dOm, dDm, Sp

    def mvn_kl_grouped_fwd(self, mats, inv, logdet, plan, D):
        """all KL terms of a step: -> kl [T], KD [T,M] (see include/gpsa_hip.h; ``plan``: KLPlan)"""
        T, M = D.shape
        kl = torch.empty(T, dtype=torch.float64, device=D.device)
        KD = torch.empty(T, M, dtype=torch.float64, device=D.device)
        rc = self.lib.gpsa_mvn_kl_grouped_fwd(_p(mats), _p(inv), _p(logdet), _p(plan.om_idx), _p(plan.pr_idx),
                                              _p(D), M, T, _p(kl), _p(KD), self._stream(D))
        _lib.check(rc, "gpsa_mvn_kl_grouped_fwd")
        return kl, KD

    def mvn_kl_grouped_bwd(self, mats, inv, plan, D, KD, g):
        """-> dOmega [T,M,M], dD [T,M], S [P,M,M]  (dK_p = 0.5 K_p^-1 S_p K_p^-1)"""
        T, M = D.shape
        dev = D.device
        dOm = torch.empty(T, M, M, dtype=torch.float64, device=dev)
        dD = torch.empty(T, M, dtype=torch.float64, device=dev)
        S = torch.empty(plan.P, M, M, dtype=torch.float64, device=dev)
        rc = self.lib.gpsa_mvn_kl_grouped_bwd(_p(mats), _p(inv), _p(plan.om_idx), _p(plan.pr_list),
                                              _p(plan.grp_off), _p(plan.order), _p(D), _p(KD), _p(g), M, T,
                                              plan.P, _p(dOm), _p(dD), _p(S), self._stream(D))
        _lib.check(rc, "gpsa_mvn_kl_grouped_bwd")
        return dOm, dD, S

    # ------------------------------------------------------------------ ELBO glue
    def elbo_fwd(self, ll, kl, kl_scale):
        """loss [1] fp32 = -sum(ll) + kl_scale * sum(kl);  ll, kl: fp64 vectors"""
        ll, kl = self._c(ll), self._c(kl)
        loss = torch.empty(1, dtype=torch.float32, device=ll.device)
        rc = self.lib.gpsa_elbo_fwd(_p(ll), ll.numel(), _p(kl), kl.numel(), float(kl_scale), _p(loss),
                                    self._stream(ll))
        _lib.check(rc, "gpsa_elbo_fwd")
        return loss

    def elbo_bwd(self, gloss, n_ll, n_kl, kl_scale):
        gloss = self._f32(gloss.reshape(1))
        dll = torch.empty(n_ll, dtype=torch.float64, device=gloss.device)
        dkl = torch.empty(max(n_kl, 1), dtype=torch.float64, device=gloss.device)[:n_kl]
        rc = self.lib.gpsa_elbo_bwd(_p(gloss), n_ll, n_kl, float(kl_scale), _p(dll), _p(dkl),
                                    self._stream(gloss))
        _lib.check(rc, "gpsa_elbo_bwd")
        return dll, dkl

    # ------------------------------------------------------------------ k-means (initialisation)
    def kmeans_assign(self, X, centres, want_d2=False):
        X, centres = self._c(X), self._c(centres)
        N, D = X.shape
        K = centres.shape[0]
        assign = torch.empty(N, dtype=torch.int32, device=X.device)
        d2 = torch.empty(N, dtype=torch.float32, device=X.device) if want_d2 else None
        rc = self.lib.gpsa_kmeans_assign(_p(X), N, D, _p(centres), K, _p(assign), _p(d2), self._stream(X))
        _lib.check(rc, "gpsa_kmeans_assign")
        return assign, d2

    def kmeans_update(self, X, assign, centres):
        """in place: centres[k] <- mean of the points assigned to k; returns counts [K] (int32)"""
        X = self._c(X)
        assert centres.is_contiguous()
        N, D = X.shape
        K = centres.shape[0]
        counts = torch.empty(K, dtype=torch.int32, device=X.device)
        ws = self._ws(self.lib.gpsa_kmeans_workspace(N, D, K), X)
        rc = self.lib.gpsa_kmeans_update(_p(X), _p(assign), N, D, K, _p(centres), _p(counts), _p(ws),
                                         ws.numel(), self._stream(X))
        _lib.check(rc, "gpsa_kmeans_update")
        return counts

    def add_diag(self, A, s):
        assert A.is_contiguous()
        M = A.shape[-1]
        nb = A.numel() // (M * M)
        rc = self.lib.gpsa_add_diag(_dt(A), _p(A), M, nb, float(s), self._stream(A))
        _lib.check(rc, "gpsa_add_diag")
        return A


_ops = None


def get_ops():
    """The process-wide ops backend (HIP).  Fails loudly without the extension or a device."""
    global _ops
    if _ops is None:
        _ops = HipOps()
    return _ops


def set_ops(obj):
    """Test hook: tests/ may install a fake backend to exercise the host logic without a GPU."""
    global _ops
    _ops = obj
