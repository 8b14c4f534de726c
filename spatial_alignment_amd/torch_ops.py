"""The hot path's entry points as PyTorch-ROCm custom ops: ``torch.ops.gpsa.*``.

SURVEY.md §8(b) asks for the replacement to be reachable "through PyTorch-ROCm custom ops": every op family of
that row is registered with the dispatcher here (``torch.library.custom_op``, device type "cuda" = HIP on ROCm),
each with

* an implementation that forwards to the SAME C ABI the ctypes binding calls (``ops.HipOps`` ->
  ``libgpsa_hip.so``; the ctypes layer stays the documented non-torch binding),
* a fake-tensor (meta) function, so shapes and dtypes propagate under ``FakeTensorMode`` / ``torch.compile``
  tracing without a device,
* an autograd formula made of the family's own backward op where the family is differentiable.

   family                       op(s)
   (1) covariance matrices                  gpsa::kmat, gpsa::kmat_bwd                 (util.py:8-66)
   (2) factorisation / whitening            gpsa::chol_inv, gpsa::whiten               (vgpsa.py:177-180, 257, 320, 394)
   (3) quadratic form (the star kernel)     gpsa::quadform, gpsa::quadform_bwd_alpha,  (vgpsa.py:192-196)
                                            gpsa::quadform_bwd_omega
   (4) reparameterised draws                gpsa::gauss_sample_F (+ _bwd)              (vgpsa.py:423-426)
       ... closed as moments (prediction)   gpsa::predict_moments                      (predict.py)
       ... closed as counts (prediction)    gpsa::predict_counts                       (predict.py, scale="response")
       the warp as a function of the point  gpsa::warp_field, gpsa::warp_invert        (warp.py; csrc/warp_field.hip)
       neighbour statistics                 gpsa::knn, gpsa::knn_average               (neighbors.py; csrc/neighbors.hip)
       spatial autocorrelation              gpsa::graph_merge, gpsa::graph_check,      (autocorr.py; csrc/autocorr.hip)
                                            gpsa::graph_sums, gpsa::autocorr_perm
       rigid pre-registration               gpsa::rigid_scores                         (register.py; csrc/register.hip)
       count preprocessing                  gpsa::count_margins, gpsa::count_deviance, (counts.py; csrc/counts.hip)
                                            gpsa::count_transform, gpsa::standardize_views
       ... from a CSR matrix                gpsa::csr_check, gpsa::count_margins_csr,  (counts.py; csrc/counts_sparse.hip)
                                            gpsa::count_deviance_csr, gpsa::csr_gather_dense
       per-view column moments              gpsa::column_moments, gpsa::column_moments_csr (counts.py; csrc/moments.hip)
       exact GP regression                  gpsa::gpr_cov, gpsa::gpr_lml_grad,         (gpr.py; csrc/gpr.hip)
                                            gpsa::gpr_mean
       optimal-transport alignment          gpsa::ot_dist, ot_sqmatvec, ot_expr_rows, ot_expr_cost, ot_cost, ot_sinkhorn, ot_plan (ot.py; csrc/ot.hip)
   (5) KL between Gaussians                 gpsa::mvn_kl                                (vgpsa.py:498-530)
   (6) Gaussian log-likelihood              gpsa::gauss_loglik_sum (+ _bwd)             (vgpsa.py:532-538)
   the whole step                           gpsa::step_forward, gpsa::step_backward,   (vgpsa.py:212-540,
                                            gpsa::elbo_loss_fwd / _bwd, gpsa::adam_step  grid_example.py:59-78)
   minibatch training (opt-in)              gpsa::row_sample_gather,                   (minibatch.py)
                                            gpsa::elbo_loss_weighted_fwd / _bwd        (csrc/loss_views.hip)
   partly observed outputs (opt-in)         gpsa::count_observed, gpsa::elbo_loss_skip_fwd / _bwd (csrc/loss_views.hip),
                                            gpsa::lmc_loglik_fused_skip                (model.skip_missing)
   count outputs (opt-in)                   gpsa::lgamma_sum, gpsa::elbo_loss_pois_fwd / _bwd (csrc/poisson.hip,
                                            csrc/loss_views.hip), gpsa::lmc_loglik_fused_pois  (model.likelihood)
   overdispersed counts (opt-in)            gpsa::nb_const, gpsa::elbo_loss_nb_fwd / _bwd, gpsa::lmc_loglik_fused_nb
                                            (csrc/negbin.hip, csrc/loss_views.hip, csrc/lmc.hip; model.likelihood = "negative_binomial")

The eight elbo_loss ops share their table builders (``_ll_arrays``, ``_grad_arrays``, ``_view_tables``) and are what the
one loss node, ``step_engine.ElboLossFn``, chooses among.

The step-engine ops are the ones ``VariationalGPSA.forward`` / ``loss_fn`` / ``FusedAdam`` go through
(step_engine.py, optim.py): they mutate caller-allocated tensors (outputs, arenas, the flat gradient buffer) and
take the non-tensor part of the call (plan handle, pointer structs) as an integer key into ``CALLS``.
"""
import ctypes as C
from typing import Optional

import torch

from . import _lib
from . import ops as _ops_mod

_raw_stream = torch._C._cuda_getCurrentRawStream
KIND_NAMES = ("rbf", "matern12", "matern32")

# non-tensor arguments of an in-flight step-engine call (ctypes structs cannot cross the dispatcher)
CALLS = {}
_next = [0]


def stash(obj):
    _next[0] += 1
    CALLS[_next[0]] = obj
    return _next[0]


def _o():
    return _ops_mod.get_ops()


# ---------------------------------------------------------------------------------------------------------
# (1) covariance matrices
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::kmat", mutates_args=(), device_types="cuda")
def kmat(Z: torch.Tensor, X: torch.Tensor, ls_u: torch.Tensor, var_u: torch.Tensor, kind: str,
         jitter: float = 0.0) -> torch.Tensor:
    """K[m, c] = k(Z[m], X[c]) + jitter [Z is X]; kind in rbf | matern12 | matern32 (the plugin API's built-ins)"""
    return _o().kmat(kind, Z, X, ls_u, var_u, jitter)


@kmat.register_fake
def _(Z, X, ls_u, var_u, kind, jitter=0.0):
    return Z.new_empty(Z.shape[0], X.shape[0])


@torch.library.custom_op("gpsa::kmat_bwd", mutates_args=(), device_types="cuda")
def kmat_bwd(Z: torch.Tensor, X: torch.Tensor, ls_u: torch.Tensor, var_u: torch.Tensor, Kbar: torch.Tensor,
             kind: str) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    dZ, dX, dpar = _o().kmat_bwd(kind, Z, X, ls_u, var_u, Kbar, need_dX=True)
    return dZ, dX, dpar


@kmat_bwd.register_fake
def _(Z, X, ls_u, var_u, Kbar, kind):
    return Z.new_empty(Z.shape), X.new_empty(X.shape), Z.new_empty(2)


def _kmat_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:4])
    ctx.kind = inputs[4]


def _kmat_backward(ctx, Kbar):
    Z, X, ls_u, var_u = ctx.saved_tensors
    dZ, dX, dpar = torch.ops.gpsa.kmat_bwd(Z, X, ls_u, var_u, Kbar.contiguous(), ctx.kind)
    return dZ, dX, dpar[0].reshape(ls_u.shape), dpar[1].reshape(var_u.shape), None, None


kmat.register_autograd(_kmat_backward, setup_context=_kmat_setup)


# ---------------------------------------------------------------------------------------------------------
# (2) factorisation and whitening
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::chol_inv", mutates_args=(), device_types="cuda")
def chol_inv(A: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A [B, M, M] fp64 -> (L^-1, logdet A, info): the fused batched Cholesky + inverse of the factor"""
    return _o().chol_inv(A)


@chol_inv.register_fake
def _(A):
    return A.new_empty(A.shape), A.new_empty(A.shape[0]), A.new_empty(A.shape[0], dtype=torch.int32)


@torch.library.custom_op("gpsa::whiten", mutates_args=(), device_types="cuda")
def whiten(Kinv: torch.Tensor, Kuf: torch.Tensor, fp32_out: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """alpha = K^-1 K_uf (fp64 matrix cores), q[c] = K_uf[:, c] . alpha[:, c]; M <= 256"""
    r = _o().whiten(Kinv, Kuf, torch.float32 if fp32_out else torch.float64)
    if r is None:
        raise _lib.GpsaHipError("gpsa::whiten: M beyond the projection kernel (chain gpsa_panel_mm / gpsa_gemm)")
    return r


@whiten.register_fake
def _(Kinv, Kuf, fp32_out=True):
    return (Kuf.new_empty(Kuf.shape, dtype=torch.float32 if fp32_out else torch.float64),
            Kuf.new_empty(Kuf.shape[1], dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------
# (3) the quadratic form  v[l, c] = alpha_c^T Omega_l alpha_c
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::quadform", mutates_args=(), device_types="cuda")
def quadform(alpha: torch.Tensor, Omega: torch.Tensor) -> torch.Tensor:
    return _o().quadform_fwd(alpha, Omega)


@quadform.register_fake
def _(alpha, Omega):
    return alpha.new_empty(Omega.shape[0], alpha.shape[1])


@torch.library.custom_op("gpsa::quadform_bwd_alpha", mutates_args=(), device_types="cuda")
def quadform_bwd_alpha(alpha: torch.Tensor, Omega: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    return _o().quadform_bwd_alpha(alpha, Omega, g)


@quadform_bwd_alpha.register_fake
def _(alpha, Omega, g):
    return alpha.new_empty(alpha.shape)


@torch.library.custom_op("gpsa::quadform_bwd_omega", mutates_args=(), device_types="cuda")
def quadform_bwd_omega(alpha: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    return _o().quadform_bwd_omega(alpha, g)


@quadform_bwd_omega.register_fake
def _(alpha, g):
    return alpha.new_empty(g.shape[0], alpha.shape[0], alpha.shape[0])


def _qf_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _qf_backward(ctx, g):
    alpha, Omega = ctx.saved_tensors
    g = g.contiguous()
    da = torch.ops.gpsa.quadform_bwd_alpha(alpha, Omega, g) if ctx.needs_input_grad[0] else None
    dO = torch.ops.gpsa.quadform_bwd_omega(alpha, g).to(Omega.dtype) if ctx.needs_input_grad[1] else None
    return da, dO


quadform.register_autograd(_qf_backward, setup_context=_qf_setup)


# ---------------------------------------------------------------------------------------------------------
# (4) reparameterised draw of the data GP: F = mean + sqrt(sigma^2 - q + v + 2e-5) eps
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::gauss_sample_F", mutates_args=(), device_types="cuda")
def gauss_sample_F(meanT: torch.Tensor, v: torch.Tensor, q: torch.Tensor, var_u: torch.Tensor,
                   eps: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """meanT, v [L, C]; q [C]; eps [C, L] -> (F [C, L], Sigma [L, C])"""
    return _o().data_sample_fwd(meanT, v, q, var_u, eps)


@gauss_sample_F.register_fake
def _(meanT, v, q, var_u, eps):
    return meanT.new_empty(meanT.shape[1], meanT.shape[0]), meanT.new_empty(meanT.shape)


@torch.library.custom_op("gpsa::gauss_sample_F_bwd", mutates_args=(), device_types="cuda")
def gauss_sample_F_bwd(dF: torch.Tensor, eps: torch.Tensor, Sigma: torch.Tensor,
                       var_u: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (g_ext [L+1, C]: d/dv rows and qbar = d/dq, dmeanT [L, C], dvar_u [1])"""
    return _o().data_sample_bwd(dF, eps, Sigma, var_u)


@gauss_sample_F_bwd.register_fake
def _(dF, eps, Sigma, var_u):
    L, Cn = Sigma.shape
    return Sigma.new_empty(L + 1, Cn), Sigma.new_empty(L, Cn), Sigma.new_empty(1)


def _gs_setup(ctx, inputs, output):
    meanT, v, q, var_u, eps = inputs
    ctx.save_for_backward(eps, output[1], var_u)
    ctx.qdtype = q.dtype


def _gs_backward(ctx, dF, dSigma):
    eps, Sigma, var_u = ctx.saved_tensors
    g_ext, dmeanT, dvar = torch.ops.gpsa.gauss_sample_F_bwd(dF.contiguous(), eps, Sigma, var_u)
    L = Sigma.shape[0]
    return dmeanT, g_ext[:L], g_ext[L].to(ctx.qdtype), dvar.reshape(var_u.shape).to(var_u.dtype), None


gauss_sample_F.register_autograd(_gs_backward, setup_context=_gs_setup)


# ---------------------------------------------------------------------------------------------------------
# (4b) the same layer closed as moments (prediction): mixture over S warp samples, reduced in the kernel
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::predict_moments", mutates_args=(), device_types="cuda")
def predict_moments(meanT: torch.Tensor, v: torch.Tensor, q: torch.Tensor, var_u: torch.Tensor, S: int,
                    W: Optional[torch.Tensor] = None, noise_u: Optional[torch.Tensor] = None,
                    include_noise: bool = False, Y: Optional[torch.Tensor] = None,
                    latent: bool = False) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """meanT, v [L, S*c]; q [S*c] -> (F_mean, F_var [c, P], Fl_mean, Fl_var [c, L], lpd [c] fp64); the latent pair and
    lpd are empty tensors when not asked for (predict.py; slideseq_prediction.py:360-368 in closed form)"""
    Fm, Fv, Lm, Lv, lpd = _o().predict_moments(meanT, v, q, var_u, S, W, noise_u, include_noise, Y, latent)
    none = lambda t, dt: meanT.new_empty(0, dtype=dt) if t is None else t
    return Fm, Fv, none(Lm, torch.float32), none(Lv, torch.float32), none(lpd, torch.float64)


@predict_moments.register_fake
def _(meanT, v, q, var_u, S, W=None, noise_u=None, include_noise=False, Y=None, latent=False):
    L, c = meanT.shape[0], meanT.shape[1] // S
    P = L if W is None else W.shape[1]
    lat = (c, L) if latent else (0,)
    return (meanT.new_empty(c, P), meanT.new_empty(c, P), meanT.new_empty(lat), meanT.new_empty(lat),
            meanT.new_empty(c if Y is not None else 0, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------
# (4c) the same layer closed under a Poisson likelihood: moments of the counts and the Poisson-lognormal log density
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::predict_counts", mutates_args=(), device_types="cuda")
def predict_counts(meanT: torch.Tensor, v: torch.Tensor, q: torch.Tensor, var_u: torch.Tensor, S: int,
                   W: Optional[torch.Tensor] = None, log_offset: Optional[torch.Tensor] = None,
                   Y: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """meanT, v [L, S*c]; q [S*c]; log_offset [c] -> (Y_mean, Y_var [c, P], lpd [c] fp64); lpd is an empty tensor without
    Y (predict.py with scale="response"; csrc/predict_counts.hip)"""
    Ym, Yv, lpd = _o().predict_counts(meanT, v, q, var_u, S, W, log_offset, Y)
    return Ym, Yv, meanT.new_empty(0, dtype=torch.float64) if lpd is None else lpd


@predict_counts.register_fake
def _(meanT, v, q, var_u, S, W=None, log_offset=None, Y=None):
    L, c = meanT.shape[0], meanT.shape[1] // S
    P = L if W is None else W.shape[1]
    return (meanT.new_empty(c, P), meanT.new_empty(c, P),
            meanT.new_empty(c if Y is not None else 0, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------
# (4d) the warp as a function of the point: mean, Jacobian, determinant; and its Newton inverse (warp.py)
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::warp_field", mutates_args=(), device_types="cuda")
def warp_field(Z: torch.Tensor, beta: torch.Tensor, A: torch.Tensor, b: torch.Tensor, ls_u: torch.Tensor,
               var_u: torch.Tensor, X: torch.Tensor, kind: str,
               jacobian: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """g(x) = x A + b + k(x, Z) beta at X [n, D] -> (G [n, D], J [n, D, D], det [n]), fp64; J and det are empty tensors
    without ``jacobian`` (csrc/warp_field.hip)"""
    G, J, det = _o().warp_field(kind, Z, beta, A, b, ls_u, var_u, X, jacobian)
    none = lambda t: G.new_empty(0) if t is None else t
    return G, none(J), none(det)


@warp_field.register_fake
def _(Z, beta, A, b, ls_u, var_u, X, kind, jacobian=True):
    n, D = X.shape
    f64 = torch.float64
    return (X.new_empty(n, D, dtype=f64), X.new_empty((n, D, D) if jacobian else (0,), dtype=f64),
            X.new_empty(n if jacobian else 0, dtype=f64))


@torch.library.custom_op("gpsa::warp_invert", mutates_args=(), device_types="cuda")
def warp_invert(Z: torch.Tensor, beta: torch.Tensor, A: torch.Tensor, b: torch.Tensor, ls_u: torch.Tensor,
                var_u: torch.Tensor, target: torch.Tensor, x0: torch.Tensor, kind: str,
                iters: int) -> tuple[torch.Tensor, torch.Tensor]:
    """exactly ``iters`` Newton updates of g(x) = target from x0 -> (X [n, D], residual [n]), fp64; a failed row is
    NaN / +inf (csrc/warp_field.hip)"""
    return _o().warp_invert(kind, Z, beta, A, b, ls_u, var_u, target, x0, iters)


@warp_invert.register_fake
def _(Z, beta, A, b, ls_u, var_u, target, x0, kind, iters):
    n, D = target.shape
    return target.new_empty(n, D, dtype=torch.float64), target.new_empty(n, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------
# (4e) neighbour statistics: exact k nearest neighbours and the neighbours' weighted average (neighbors.py)
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::knn", mutates_args=(), device_types="cuda")
def knn(Q: torch.Tensor, R: torch.Tensor, k: int, exclude_self: bool = False,
        parts: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """the k rows of R [nr, D] nearest each row of Q [nq, D] by the key (fp64 squared distance, index), ascending ->
    (idx [nq, k] int32, d2 [nq, k] fp64); the same bits for every ``parts`` (csrc/neighbors.hip)"""
    return _o().knn(Q, R, k, exclude_self, parts)


@knn.register_fake
def _(Q, R, k, exclude_self=False, parts=0):
    nq = Q.shape[0]
    return Q.new_empty(nq, k, dtype=torch.int32), Q.new_empty(nq, k, dtype=torch.float64)


@torch.library.custom_op("gpsa::knn_average", mutates_args=(), device_types="cuda")
def knn_average(idx: torch.Tensor, d2: Optional[torch.Tensor], Y: torch.Tensor, weights: str = "uniform") -> torch.Tensor:
    """the NaN-skipping weighted average of Y's rows idx [nq, k] -> [nq, P] fp32 (fp64 for an fp64 Y); weights "uniform"
    or "distance" (csrc/neighbors.hip)"""
    return _o().knn_average(idx, d2, Y, weights)


@knn_average.register_fake
def _(idx, d2, Y, weights="uniform"):
    return Y.new_empty(idx.shape[0], Y.shape[1], dtype=torch.float64 if Y.dtype == torch.float64 else torch.float32)


# ... spatial autocorrelation: the weight graph in CSR, its sums, the permuted numerators (autocorr.py; csrc/autocorr.hip)
@torch.library.custom_op("gpsa::graph_merge", mutates_args=(), device_types="cuda")
def graph_merge(out_sorted: torch.Tensor, in_ptr: Optional[torch.Tensor], in_src: Optional[torch.Tensor],
                kind: str = "none", row_standardize: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the kNN lists (rows ascending) and their in-lists merged per row: "none" | "union" | "mutual" ->
    (crow [n + 1] int64, col [nnz] int32, w [nnz] fp64); nnz depends on the data"""
    return _o().graph_merge(out_sorted, in_ptr, in_src, kind, row_standardize)


@graph_merge.register_fake
def _(out_sorted, in_ptr, in_src, kind="none", row_standardize=True):
    n, k = out_sorted.shape
    nnz = n * k if kind == "none" else torch.library.get_ctx().new_dynamic_size()
    return (out_sorted.new_empty(n + 1, dtype=torch.int64), out_sorted.new_empty(nnz, dtype=torch.int32),
            out_sorted.new_empty(nnz, dtype=torch.float64))


@torch.library.custom_op("gpsa::graph_check", mutates_args=(), device_types="cuda")
def graph_check(crow: torch.Tensor, col: torch.Tensor, w: torch.Tensor, n: int) -> torch.Tensor:
    """[5] int64: crow violations, columns outside [0, n), places out of order within a row, self edges, bad weights"""
    return _o().graph_check(crow, col, w, n)


@graph_check.register_fake
def _(crow, col, w, n):
    return crow.new_empty(5, dtype=torch.int64)


@torch.library.custom_op("gpsa::graph_sums", mutates_args=(), device_types="cuda")
def graph_sums(crow: torch.Tensor, col: torch.Tensor, w: torch.Tensor, n: int, tptr: torch.Tensor,
               tperm: torch.Tensor) -> torch.Tensor:
    """[3] fp64: S0, S1, S2 of the graph, fixed-order sums; tptr / tperm: the transposed structure"""
    return _o().graph_sums(crow, col, w, n, tptr, tperm)


@graph_sums.register_fake
def _(crow, col, w, n, tptr, tperm):
    return w.new_empty(3, dtype=torch.float64)


@torch.library.custom_op("gpsa::autocorr_perm", mutates_args=(), device_types="cuda")
def autocorr_perm(Z: torch.Tensor, crow: torch.Tensor, col: torch.Tensor, w: torch.Tensor, perms: torch.Tensor,
                  mode: str = "moran") -> tuple[torch.Tensor, torch.Tensor]:
    """the Moran / Geary numerator of Z [n, P] fp64 under every row of perms [R, n] int32 -> (num [R, P] fp64,
    n_bad [1] int64); the permuted matrix is never formed"""
    return _o().autocorr_perm(Z, crow, col, w, perms, mode)


@autocorr_perm.register_fake
def _(Z, crow, col, w, perms, mode="moran"):
    return Z.new_empty(perms.shape[0], Z.shape[1], dtype=torch.float64), Z.new_empty(1, dtype=torch.int64)


# ... rigid pre-registration: K candidate transforms of one slice scored against another (register.py; csrc/register.hip)
@torch.library.custom_op("gpsa::rigid_scores", mutates_args=(), device_types="cuda")
def rigid_scores(XA: torch.Tensor, YA: torch.Tensor, XB: torch.Tensor, YB: torch.Tensor, T: torch.Tensor, max_d2: float,
                 parts: int = 0, return_nn: bool = False
                 ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """per row of T [K, 6]: B's rows at R x + t matched to their nearest row of A within max_d2 -> (sse [K] fp64,
    n_matched [K] int64, d2_sum [K] fp64, nn [K, n] int32, d2 [K, n] fp64; the last two empty without ``return_nn``);
    the same bits for every ``parts``, K and repeat"""
    sse, n_matched, d2_sum, nn, d2 = _o().rigid_scores(XA, YA, XB, YB, T, max_d2, parts, return_nn)
    if not return_nn:
        nn, d2 = XB.new_empty(0, dtype=torch.int32), XB.new_empty(0, dtype=torch.float64)
    return sse, n_matched, d2_sum, nn, d2


@rigid_scores.register_fake
def _(XA, YA, XB, YB, T, max_d2, parts=0, return_nn=False):
    K, n = T.shape[0], XB.shape[0]
    f64 = torch.float64
    return (XB.new_empty(K, dtype=f64), XB.new_empty(K, dtype=torch.int64), XB.new_empty(K, dtype=f64),
            XB.new_empty((K, n) if return_nn else (0,), dtype=torch.int32),
            XB.new_empty((K, n) if return_nn else (0,), dtype=f64))


# ---------------------------------------------------------------------------------------------------------
# (4f) count preprocessing: margins, Poisson deviance, residual transforms, per-view z-score (counts.py)
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::count_margins", mutates_args=(), device_types="cuda")
def count_margins(Y: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """one read of Y [N, P] fp32 -> (row_sum [N] fp64, col_sum [P] fp64, row_nnz [N] int64, col_nnz [P] int64,
    n_invalid [1] int64) (csrc/counts.hip)"""
    return _o().count_margins(Y)


@count_margins.register_fake
def _(Y):
    N, P = Y.shape
    return (Y.new_empty(N, dtype=torch.float64), Y.new_empty(P, dtype=torch.float64), Y.new_empty(N, dtype=torch.int64),
            Y.new_empty(P, dtype=torch.int64), Y.new_empty(1, dtype=torch.int64))


@torch.library.custom_op("gpsa::count_deviance", mutates_args=(), device_types="cuda")
def count_deviance(Y: torch.Tensor, log_sz: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(ll_sat, abs_sat) [P] fp64: sum_i y log y - y log_sz_i and the sum of the terms' magnitudes (csrc/counts.hip)"""
    return _o().count_deviance(Y, log_sz)


@count_deviance.register_fake
def _(Y, log_sz):
    P = Y.shape[1]
    return Y.new_empty(P, dtype=torch.float64), Y.new_empty(P, dtype=torch.float64)


@torch.library.custom_op("gpsa::count_transform", mutates_args=(), device_types="cuda")
def count_transform(Y: torch.Tensor, mode: str, row_sum: torch.Tensor, col_sum: Optional[torch.Tensor] = None,
                    total: float = 1.0, theta: float = 1.0, clip: float = 0.0, target: float = 1.0) -> torch.Tensor:
    """"pearson" | "nb_deviance" | "poisson_deviance" | "log1p" of Y [N, P] fp32, fp64 per element -> [N, P] fp32
    (csrc/counts.hip; the in-place form is ops.count_transform(..., out=Y))"""
    return _o().count_transform(Y, mode, row_sum, col_sum, total, theta, clip, target)


@count_transform.register_fake
def _(Y, mode, row_sum, col_sum=None, total=1.0, theta=1.0, clip=0.0, target=1.0):
    return Y.new_empty(Y.shape, dtype=torch.float32)


@torch.library.custom_op("gpsa::standardize_views", mutates_args=(), device_types="cuda")
def standardize_views(Y: torch.Tensor, view_off: list[int]) -> tuple[torch.Tensor, torch.Tensor]:
    """(y - mean) / std per (view, column) over the row ranges view_off [V + 1] -> ([N, P] fp32, n_constant [V] int64)
    (csrc/counts.hip)"""
    return _o().standardize_views(Y, view_off)


@standardize_views.register_fake
def _(Y, view_off):
    return Y.new_empty(Y.shape, dtype=torch.float32), Y.new_empty(len(view_off) - 1, dtype=torch.int64)


# ... from a CSR matrix [N, P] on the device: crow [N + 1] int64, col [nnz] int32, val [nnz] fp32 (csrc/counts_sparse.hip)
@torch.library.custom_op("gpsa::csr_check", mutates_args=(), device_types="cuda")
def csr_check(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, N: int, P: int) -> torch.Tensor:
    """[4] int64: crow violations, column indices outside [0, P), places inside a row where the column index does not
    strictly increase, stored zeros"""
    return _o().csr_check(crow, col, val, N, P)


@csr_check.register_fake
def _(crow, col, val, N, P):
    return crow.new_empty(4, dtype=torch.int64)


@torch.library.custom_op("gpsa::count_margins_csr", mutates_args=(), device_types="cuda")
def count_margins_csr(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, N: int, P: int,
                      keep: Optional[torch.Tensor] = None
                      ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """gpsa::count_margins of the CSR matrix in one read; ``keep`` [N] bool: the rows to take (None: all)"""
    return _o().count_margins_csr(crow, col, val, N, P, keep)


@count_margins_csr.register_fake
def _(crow, col, val, N, P, keep=None):
    return (val.new_empty(N, dtype=torch.float64), val.new_empty(P, dtype=torch.float64),
            val.new_empty(N, dtype=torch.int64), val.new_empty(P, dtype=torch.int64), val.new_empty(1, dtype=torch.int64))


@torch.library.custom_op("gpsa::count_deviance_csr", mutates_args=(), device_types="cuda")
def count_deviance_csr(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, N: int, P: int, log_sz: torch.Tensor,
                       keep: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """gpsa::count_deviance of the CSR matrix; log_sz [N] by the original row"""
    return _o().count_deviance_csr(crow, col, val, N, P, log_sz, keep)


@count_deviance_csr.register_fake
def _(crow, col, val, N, P, log_sz, keep=None):
    return val.new_empty(P, dtype=torch.float64), val.new_empty(P, dtype=torch.float64)


@torch.library.custom_op("gpsa::csr_gather_dense", mutates_args=(), device_types="cuda")
def csr_gather_dense(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, N: int, P: int, rows: torch.Tensor,
                     slot: torch.Tensor, G: int) -> torch.Tensor:
    """[len(rows), G] fp32: out[j, slot[g]] = the value stored at (rows[j], g), zeros elsewhere; slot [P] int32, -1: dropped"""
    return _o().csr_gather_dense(crow, col, val, N, P, rows, slot, G)


@csr_gather_dense.register_fake
def _(crow, col, val, N, P, rows, slot, G):
    return val.new_empty(rows.shape[0], G, dtype=torch.float32)


# ... and the per-view column moments, dense and CSR (csrc/moments.hip)
@torch.library.custom_op("gpsa::column_moments", mutates_args=(), device_types="cuda")
def column_moments(Y: torch.Tensor, mode: str, view_off: list[int], scale: Optional[torch.Tensor] = None
                   ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(s1, s2, abs1 [V, P] fp64, n_nonfinite [1] int64): the sums of t, t^2, |t| per (view, column) of Y [N, P] fp32 with
    t = y ("identity"), expm1(y) ("expm1") or y scale_i ("normalize"); view_off [V + 1]"""
    return _o().column_moments(Y, mode, view_off, scale)


@column_moments.register_fake
def _(Y, mode, view_off, scale=None):
    V, P = len(view_off) - 1, Y.shape[1]
    return tuple(Y.new_empty(V, P, dtype=torch.float64) for _ in range(3)) + (Y.new_empty(1, dtype=torch.int64),)


@torch.library.custom_op("gpsa::column_moments_csr", mutates_args=(), device_types="cuda")
def column_moments_csr(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, N: int, P: int, mode: str,
                       view_off: list[int], scale: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None
                       ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """gpsa::column_moments of the CSR matrix over its stored entries; scale [N] by the original row; ``keep`` [N] bool"""
    return _o().column_moments_csr(crow, col, val, N, P, mode, view_off, scale, keep)


@column_moments_csr.register_fake
def _(crow, col, val, N, P, mode, view_off, scale=None, keep=None):
    V = len(view_off) - 1
    return tuple(val.new_empty(V, P, dtype=torch.float64) for _ in range(3)) + (val.new_empty(1, dtype=torch.int64),)


# ... and expression PCA's two passes over the data (csrc/pca.hip)
@torch.library.custom_op("gpsa::pca_gram", mutates_args=(), device_types="cuda")
def pca_gram(Y: torch.Tensor, mean: torch.Tensor, view_off: list[int], inv_scale: Optional[torch.Tensor] = None
             ) -> torch.Tensor:
    """G [P, P] fp64 = sum_i z_ia z_ib, z = (y - mean[v]) * inv_scale[v] in fp64 from Y [N, P] fp32; mean / inv_scale
    [V, P] fp64, view_off [V + 1]; symmetric to the bit"""
    return _o().pca_gram(Y, mean, view_off, inv_scale)


@pca_gram.register_fake
def _(Y, mean, view_off, inv_scale=None):
    return Y.new_empty(Y.shape[1], Y.shape[1], dtype=torch.float64)


@torch.library.custom_op("gpsa::pca_project", mutates_args=(), device_types="cuda")
def pca_project(Y: torch.Tensor, mean: torch.Tensor, view_off: list[int], comp: torch.Tensor,
                inv_scale: Optional[torch.Tensor] = None, out_f64: bool = False) -> torch.Tensor:
    """scores [N, k] = z comp^T with z as in gpsa::pca_gram and comp [k <= 128, P] fp64; fp32 (rounded once) or fp64"""
    return _o().pca_project(Y, mean, view_off, comp, inv_scale, torch.float64 if out_f64 else torch.float32)


@pca_project.register_fake
def _(Y, mean, view_off, comp, inv_scale=None, out_f64=False):
    return Y.new_empty(Y.shape[0], comp.shape[0], dtype=torch.float64 if out_f64 else torch.float32)


# ---------------------------------------------------------------------------------------------------------
# (4g) exact GP regression: covariance assembly, the LML gradient's reduction, the predictive mean (gpr.py)
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::gpr_cov", mutates_args=(), device_types="cuda")
def gpr_cov(XA: torch.Tensor, XB: torch.Tensor, theta: torch.Tensor, kind: str, amplitude: bool = False,
            same: bool = False, jitter: float = 0.0) -> torch.Tensor:
    """K [na, nb] = a k(XA, XB) in sklearn's kernel forms, fp64; theta [3] = (log a, log l, log tau2) on the device;
    ``same``: XB is XA, (tau2 + jitter) on the diagonal, symmetric to the bit (csrc/gpr.hip)"""
    return _o().gpr_cov(kind, XA, XA if same else XB, theta, amplitude, same, jitter)


@gpr_cov.register_fake
def _(XA, XB, theta, kind, amplitude=False, same=False, jitter=0.0):
    return XA.new_empty(XA.shape[0], XB.shape[0], dtype=torch.float64)


@torch.library.custom_op("gpsa::gpr_lml_grad", mutates_args=(), device_types="cuda")
def gpr_lml_grad(X: torch.Tensor, theta: torch.Tensor, alpha: torch.Tensor, Kinv: torch.Tensor, kind: str,
                 amplitude: bool = False) -> torch.Tensor:
    """dLML / d(log a, log l, log tau2) [3] fp64 = 1/2 sum_ij (alpha alpha^T - P Kinv)_ij dK_ij, fused, in a fixed order
    (csrc/gpr.hip)"""
    return _o().gpr_lml_grad(kind, X, theta, alpha, Kinv, amplitude)


@gpr_lml_grad.register_fake
def _(X, theta, alpha, Kinv, kind, amplitude=False):
    return X.new_empty(3, dtype=torch.float64)


@torch.library.custom_op("gpsa::gpr_mean", mutates_args=(), device_types="cuda")
def gpr_mean(XS: torch.Tensor, X: torch.Tensor, theta: torch.Tensor, alpha: torch.Tensor, kind: str,
             amplitude: bool = False) -> torch.Tensor:
    """[ns, P] = a k(XS, X) alpha, fp64, without the [ns, N] matrix (csrc/gpr.hip)"""
    return _o().gpr_mean(kind, XS, X, theta, alpha, amplitude)


@gpr_mean.register_fake
def _(XS, X, theta, alpha, kind, amplitude=False):
    return XS.new_empty(XS.shape[0], alpha.shape[1], dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------
# (4h) optimal-transport slice alignment: the pieces of an entropic fused Gromov-Wasserstein solve (ot.py; csrc/ot.hip)
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::ot_dist", mutates_args=(), device_types="cuda")
def ot_dist(X: torch.Tensor) -> torch.Tensor:
    """[n, n] Euclidean distances of X [n, D <= 4] fp64: symmetric to the bit, zero diagonal"""
    return _o().ot_dist(X)


@ot_dist.register_fake
def _(X):
    return X.new_empty(X.shape[0], X.shape[0], dtype=torch.float64)


@torch.library.custom_op("gpsa::ot_sqmatvec", mutates_args=(), device_types="cuda")
def ot_sqmatvec(Cm: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """[n] = sum_k Cm_ik^2 v_k"""
    return _o().ot_sqmatvec(Cm, v)


@ot_sqmatvec.register_fake
def _(Cm, v):
    return Cm.new_empty(Cm.shape[0], dtype=torch.float64)


@torch.library.custom_op("gpsa::ot_expr_rows", mutates_args=(), device_types="cuda")
def ot_expr_rows(Y: torch.Tensor, mode: str = "kl") -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Y [n, P] fp32 -> (Pm [n, P], Lg, term [n] fp64, n_invalid [1] int64); "kl": rows on the simplex after the 0.01
    shift, Lg [n, P] their logs, term = sum Pm Lg; "euclidean": Pm = y, Lg is empty [0, P], term = sum y^2"""
    Pm, Lg, term, bad = _o().ot_expr_rows(Y, mode)
    return Pm, (Pm.new_empty(0, Pm.shape[1]) if Lg is Pm else Lg), term, bad


@ot_expr_rows.register_fake
def _(Y, mode="kl"):
    n, P = Y.shape
    return (Y.new_empty(n, P, dtype=torch.float64), Y.new_empty(n if mode == "kl" else 0, P, dtype=torch.float64),
            Y.new_empty(n, dtype=torch.float64), Y.new_empty(1, dtype=torch.int64))


@torch.library.custom_op("gpsa::ot_expr_cost", mutates_args=("G",), device_types="cuda")
def ot_expr_cost(G: torch.Tensor, ra: torch.Tensor, rb: Optional[torch.Tensor] = None, mode: str = "kl") -> None:
    """in place over G [n, m]: "kl" M = ra_i - G_ij; "euclidean" M = max(0, ra_i + rb_j - 2 G_ij)"""
    _o().ot_expr_cost(G, ra, rb, mode)


@ot_expr_cost.register_fake
def _(G, ra, rb=None, mode="kl"):
    return None


@torch.library.custom_op("gpsa::ot_cost", mutates_args=("G",), device_types="cuda")
def ot_cost(G: torch.Tensor, M: torch.Tensor, T: torch.Tensor, cA: torch.Tensor, cB: torch.Tensor, cAt: torch.Tensor,
            cBt: torch.Tensor, alpha: float) -> torch.Tensor:
    """in place over G = C1 T C2: the outer step's cost; -> sums [3]: sum |cost|, <M, T>, <cAt 1^T + 1 cBt^T - 2 G, T>"""
    return _o().ot_cost(G, M, T, cA, cB, cAt, cBt, alpha)[1]


@ot_cost.register_fake
def _(G, M, T, cA, cB, cAt, cBt, alpha):
    return G.new_empty(3, dtype=torch.float64)


@torch.library.custom_op("gpsa::ot_sinkhorn", mutates_args=("f", "g"), device_types="cuda")
def ot_sinkhorn(cost: torch.Tensor, loga: torch.Tensor, logb: torch.Tensor, eps: torch.Tensor, f: torch.Tensor,
                g: torch.Tensor, iters: int) -> None:
    """``iters`` log-domain Sinkhorn sweeps on the stream; f [n], g [m] in place; eps [1] fp64 on the device"""
    _o().ot_sinkhorn(cost, loga, logb, eps, f, g, iters)


@ot_sinkhorn.register_fake
def _(cost, loga, logb, eps, f, g, iters):
    return None


@torch.library.custom_op("gpsa::ot_plan", mutates_args=("T",), device_types="cuda")
def ot_plan(cost: torch.Tensor, f: torch.Tensor, g: torch.Tensor, a: torch.Tensor, b: torch.Tensor, eps: torch.Tensor,
            T: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """T = a_i b_j exp((f_i + g_j - cost_ij) / eps) over the previous plan; -> (T 1 [n], T^T 1 [m], sums [3]: the two
    marginal errors and |T - T_old|_1)"""
    return _o().ot_plan(cost, f, g, a, b, eps, T)[1:]


@ot_plan.register_fake
def _(cost, f, g, a, b, eps, T):
    n, m = cost.shape
    return (cost.new_empty(n, dtype=torch.float64), cost.new_empty(m, dtype=torch.float64),
            cost.new_empty(3, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------
# (5) KL(N(d, Omega) || N(0, K)) for a batch sharing one prior
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::mvn_kl", mutates_args=(), device_types="cuda")
def mvn_kl(Kinv: torch.Tensor, logdetK: torch.Tensor, Omega: torch.Tensor, logdetO: torch.Tensor,
           Dm: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (kl [B], K^-1 d [B, M]); Kinv [M, M], Omega [B, M, M], Dm [B, M] mean differences (fp64)"""
    return _o().mvn_kl_fwd(Kinv, logdetK, Omega, logdetO, Dm)


@mvn_kl.register_fake
def _(Kinv, logdetK, Omega, logdetO, Dm):
    return Dm.new_empty(Dm.shape[0]), Dm.new_empty(Dm.shape)


# ---------------------------------------------------------------------------------------------------------
# (6) Gaussian log-likelihood  sum log N(Y; F, scale = exp(noise_u) + 1e-5) / S
# ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op("gpsa::gauss_loglik_sum", mutates_args=(), device_types="cuda")
def gauss_loglik_sum(F: torch.Tensor, Y: torch.Tensor, noise_u: torch.Tensor) -> torch.Tensor:
    return _o().loglik_fwd(F, Y, noise_u)


@gauss_loglik_sum.register_fake
def _(F, Y, noise_u):
    return F.new_empty(1, dtype=torch.float64)


@torch.library.custom_op("gpsa::gauss_loglik_sum_bwd", mutates_args=(), device_types="cuda")
def gauss_loglik_sum_bwd(F: torch.Tensor, Y: torch.Tensor, noise_u: torch.Tensor,
                         gout: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    return _o().loglik_bwd(F, Y, noise_u, gout)


@gauss_loglik_sum_bwd.register_fake
def _(F, Y, noise_u, gout):
    return F.new_empty(F.shape), F.new_empty(1)


def _ll_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _ll_backward(ctx, gout):
    F, Y, noise_u = ctx.saved_tensors
    dF, dn = torch.ops.gpsa.gauss_loglik_sum_bwd(F, Y, noise_u, gout.contiguous())
    return dF, None, dn.reshape(noise_u.shape).to(noise_u.dtype)


gauss_loglik_sum.register_autograd(_ll_backward, setup_context=_ll_setup)


# ---------------------------------------------------------------------------------------------------------
# the step engine (what the model classes call)
#
# These five run once or twice per training step, also on problems whose whole step is under a millisecond, so they
# are registered through the low-level ``torch.library.Library`` interface (schema string + CUDA kernel + fake
# function): ~10 us of dispatch per call instead of the ~35 us of a ``custom_op`` object (the reference example's
# own 2 x 100-spot problem ran 920 -> 720 steps/s with the latter).  Mutated arguments are declared in the schema.
# ---------------------------------------------------------------------------------------------------------
_ENGINE = torch.library.Library("gpsa", "FRAGMENT")


def _engine_op(schema, fn):
    name = schema.split("(", 1)[0]
    _ENGINE.define(schema)
    _ENGINE.impl(name, fn, "CUDA")
    torch.library.register_fake(f"gpsa::{name}", lambda *a, **k: None, lib=_ENGINE)
    return fn


def _step_forward(params, ins, outs, saved, scratch, call, stages):
    """gpsa_step_forward: warp GPs (stage 1) and data GPs (stage 2) of VariationalGPSA.forward into ``outs``"""
    c = CALLS[call]
    _lib.check(c["lib"].gpsa_step_forward(c["handle"], C.byref(c["prm"]), C.byref(c["io"]), saved.data_ptr(),
                                          scratch.data_ptr(), int(stages), _raw_stream(saved.device.index)),
               "gpsa_step_forward")


_engine_op("step_forward(Tensor[] params, Tensor[] ins, Tensor(a!)[] outs, Tensor(b!) saved, Tensor(c!) scratch, "
           "int call, int stages) -> ()", _step_forward)


def _step_backward(params, grads_out, saved, flat, scratch, call):
    """gpsa_step_backward: every parameter gradient of the step into the flat buffer ``flat``"""
    c = CALLS[call]
    _lib.check(c["lib"].gpsa_step_backward(c["handle"], C.byref(c["prm"]), C.byref(c["io"]), C.byref(c["og"]),
                                           saved.data_ptr(), scratch.data_ptr(), C.byref(c["grads"]),
                                           _raw_stream(saved.device.index)), "gpsa_step_backward")


_engine_op("step_backward(Tensor[] params, Tensor[] grads_out, Tensor saved, Tensor(a!) flat, Tensor(b!) scratch, "
           "int call) -> ()", _step_backward)


def loss_workspace_bytes(n):  # n likelihood terms, LL_SLOT_DOUBLES (csrc/common.hpp) doubles each; tests/test_cabi.py
    return 8 * 4100 * n + 64


def _ll_arrays(Fs, Ys, noise, noise_idx, shapes=None, fused=None):
    """-> (n, (F, Y, noise_u, S, N, P), zpart, nparts) as the gpsa_elbo_loss_* entries take them.  shapes: [S, N, P] per
    term, flattened (default: those of Fs); fused: per term, whether its "F" is its partial-sum vector (ll_part)"""
    n = len(Fs)
    arr = lambda vals: (C.c_void_p * n)(*vals)
    sh = [int(f.shape[k]) for f in Fs for k in range(3)] if shapes is None else shapes[:3 * n]
    if fused is None:
        Fp, Zp, nparts = arr([f.data_ptr() for f in Fs]), None, 0
    else:
        Fp = arr([0 if z else f.data_ptr() for f, z in zip(Fs, fused)])
        Zp = arr([f.data_ptr() if z else 0 for f, z in zip(Fs, fused)])
        nparts = max([int(f.numel()) for f, z in zip(Fs, fused) if z] or [0])
    terms = (Fp, arr([y.data_ptr() for y in Ys]), arr([noise.data_ptr() + 4 * j for j in noise_idx]),
             (C.c_int * n)(*sh[0::3]), (C.c_longlong * n)(*sh[1::3]), (C.c_int * n)(*sh[2::3]))
    return n, terms, Zp, nparts


def _grad_arrays(dFs, dnoise, noise_idx, fused=None):
    n = len(dFs)  # -> dF pointers (NULL for a fused term), pointers to the terms' noise gradients, dnoise_all, n_noise
    return ((C.c_void_p * n)(*[0 if (fused and fused[i]) else t.data_ptr() for i, t in enumerate(dFs)]),
            (C.c_void_p * n)(*[dnoise.data_ptr() + 4 * j for j in noise_idx]), dnoise.data_ptr(), dnoise.numel())


def _kl_args(kl):
    return (0, 0) if kl is None else (kl.data_ptr(), kl.numel())


def _elbo_loss_fwd(Fs, Ys, noise, noise_idx, kl, kl_scale, loss, ll, ws):
    """loss = -(sum_i LL_i) + kl_scale * sum(kl): log-likelihood partials, finish and the ELBO glue
    (gpsa_elbo_loss_fwd; contiguous fp32 F / Y / noise, fp64 kl)"""
    n, terms, _, _ = _ll_arrays(Fs, Ys, noise, noise_idx)
    _lib.check(_lib.load().gpsa_elbo_loss_fwd(n, *terms, *_kl_args(kl), float(kl_scale), loss.data_ptr(),
                                              ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _raw_stream(loss.device.index)), "gpsa_elbo_loss_fwd")


_engine_op("elbo_loss_fwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, Tensor? kl, float kl_scale, "
           "Tensor(a!) loss, Tensor(b!) ll, Tensor(c!) ws) -> ()", _elbo_loss_fwd)


def _elbo_loss_bwd(Fs, Ys, noise, noise_idx, gloss, n_kl, kl_scale, dFs, dnoise, dkl, ws):
    n, terms, _, _ = _ll_arrays(Fs, Ys, noise, noise_idx)
    grads = _grad_arrays(dFs, dnoise, noise_idx)
    _lib.check(_lib.load().gpsa_elbo_loss_bwd(n, *terms, gloss.data_ptr(), int(n_kl), float(kl_scale), *grads,
                                              0 if dkl is None else dkl.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _raw_stream(gloss.device.index)), "gpsa_elbo_loss_bwd")


_engine_op("elbo_loss_bwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, Tensor gloss, int n_kl, "
           "float kl_scale, Tensor(a!)[] dFs, Tensor(b!) dnoise, Tensor(c!)? dkl, Tensor(d!) ws) -> ()", _elbo_loss_bwd)


def _elbo_loss_fused_fwd(Fs, Ys, noise, noise_idx, shapes, fused, kl, kl_scale, loss, ll, ws):
    """gpsa_elbo_loss_fused_fwd: the loss with some likelihood terms already reduced to partial sums by the step"""
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes, fused)
    _lib.check(_lib.load().gpsa_elbo_loss_fused_fwd(n, *terms, Zp, nparts, *_kl_args(kl), float(kl_scale),
                                                    loss.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    _raw_stream(loss.device.index)), "gpsa_elbo_loss_fused_fwd")


_engine_op("elbo_loss_fused_fwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "Tensor? kl, float kl_scale, Tensor(a!) loss, Tensor(b!) ll, Tensor(c!) ws) -> ()", _elbo_loss_fused_fwd)


def _elbo_loss_fused_bwd(Fs, Ys, noise, noise_idx, shapes, fused, gloss, n_kl, kl_scale, dFs, dnoise, dkl, ws):
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes, fused)
    grads = _grad_arrays(dFs, dnoise, noise_idx, fused)
    _lib.check(_lib.load().gpsa_elbo_loss_fused_bwd(n, *terms, Zp, nparts, gloss.data_ptr(), int(n_kl), float(kl_scale),
                                                    *grads, 0 if dkl is None else dkl.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), _raw_stream(gloss.device.index)),
               "gpsa_elbo_loss_fused_bwd")


_engine_op("elbo_loss_fused_bwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "Tensor gloss, int n_kl, float kl_scale, Tensor(a!)[] dFs, Tensor(b!) dnoise, Tensor(c!)? dkl, "
           "Tensor(d!) ws) -> ()", _elbo_loss_fused_bwd)


def _lmc_loglik_fused(F, W, Y, noise, noise_idx, zpart, dF, dW, ws):
    """gpsa_lmc_loglik_fused_f32: an LMC modality's likelihood partial sums, dLoss/dF_latent and dLoss/dW in one pass
    over (F_latent [S,N,L], W [L,P], Y [N,P]) - F_obs = F_latent W is never formed"""
    S, N, L = (int(d) for d in F.shape)
    _lib.check(_lib.load().gpsa_lmc_loglik_fused_f32(F.data_ptr(), W.data_ptr(), Y.data_ptr(),
                                                     noise.data_ptr() + 4 * int(noise_idx), S, N, L, int(W.shape[1]),
                                                     zpart.data_ptr(), zpart.numel(), dF.data_ptr(), dW.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), _raw_stream(F.device.index)),
               "gpsa_lmc_loglik_fused_f32")


_engine_op("lmc_loglik_fused(Tensor F, Tensor W, Tensor Y, Tensor noise, int noise_idx, Tensor(a!) zpart, Tensor(b!) dF, "
           "Tensor(c!) dW, Tensor(d!) ws) -> ()", _lmc_loglik_fused)


def _adam_step(params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps):
    """torch.optim.Adam's update over all tensors in one launch, step counter on the device (gpsa_adam_step)"""
    n = len(params)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    numel = (C.c_longlong * n)(*[p.numel() for p in params])
    _lib.check(_lib.load().gpsa_adam_step(n, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq), numel, float(lr),
                                          float(beta1), float(beta2), float(eps), step.data_ptr(),
                                          _raw_stream(step.device.index)), "gpsa_adam_step")


_engine_op("adam_step(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] exp_avg, Tensor(c!)[] exp_avg_sq, "
           "Tensor(d!) step, float lr, float beta1, float beta2, float eps) -> ()", _adam_step)


# ---------------------------------------------------------------------------------------------------------
# minibatch (stochastic variational) training: the batch sampler-gather (minibatch.py, csrc/minibatch.hip) and the
# per-view weighted likelihood (csrc/loss_views.hip)
# ---------------------------------------------------------------------------------------------------------
def _row_sample_gather(Xs, Ys, n_views, n_rows, batch, seed, counter, rows, Xb, Yb):
    """gpsa_row_sample_gather: step counter[0]'s batch of every (modality, view) - row numbers, coordinates and
    observations gathered into rows / Xb / Yb - and counter[0] += 1, all on the device"""
    n = len(Xs)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    ints = lambda vals: (C.c_int * len(vals))(*[int(x) for x in vals])
    lls = lambda vals: (C.c_longlong * len(vals))(*[int(x) for x in vals])
    _lib.check(_lib.load().gpsa_row_sample_gather(n, ints(n_views), lls(n_rows), lls(batch),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, counter.data_ptr(), arr(Xs),
                                                  ints([x.shape[1] for x in Xs]), arr(Ys),
                                                  ints([y.shape[1] for y in Ys]), arr(rows), arr(Xb), arr(Yb),
                                                  _raw_stream(counter.device.index)), "gpsa_row_sample_gather")


_engine_op("row_sample_gather(Tensor[] Xs, Tensor[] Ys, int[] n_views, int[] n_rows, int[] batch, int seed, "
           "Tensor(a!) counter, Tensor(b!)[] rows, Tensor(c!)[] Xb, Tensor(d!)[] Yb) -> ()", _row_sample_gather)


def _view_tables(n, n_views, view_off, weights=(), nobs=()):
    """the per-view tables of n terms as the C entries take them -> (n_views, view_off, w, nobs, keep): the int array of
    the terms' view counts, a host array of pointers to each term's row offsets (view_off: every term's n_views + 1
    offsets, concatenated), host arrays of the terms' weight and count pointers, and what keeps the offsets alive.  An
    absent table (empty list) is NULL"""
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts]) if ts else None
    nv, offp, offs = None, None, []
    if n_views:
        at = 0
        for v in n_views:
            offs.append((C.c_longlong * (int(v) + 1))(*[int(x) for x in view_off[at:at + int(v) + 1]]))
            at += int(v) + 1
        nv, offp = (C.c_int * n)(*[int(x) for x in n_views]), (C.c_void_p * n)(*[C.addressof(o) for o in offs])
    return nv, offp, ptrs(weights), ptrs(nobs), offs


def _elbo_loss_weighted_fwd(Fs, Ys, noise, noise_idx, n_views, view_off, weights, kl, kl_scale, loss, ll, ws):
    """gpsa_elbo_loss_fwd with per-view fp64 weights: loss = -sum_m sum_v w_mv LL_mv + kl_scale * sum(kl)
    (view_off: every term's n_views + 1 row offsets, concatenated)"""
    n, terms, _, _ = _ll_arrays(Fs, Ys, noise, noise_idx)
    nv, offp, Wp, _, _keep = _view_tables(n, n_views, view_off, weights)
    _lib.check(_lib.load().gpsa_elbo_loss_weighted_fwd(n, *terms, nv, offp, Wp, *_kl_args(kl), float(kl_scale),
                                                       loss.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       _raw_stream(loss.device.index)), "gpsa_elbo_loss_weighted_fwd")


_engine_op("elbo_loss_weighted_fwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] n_views, "
           "int[] view_off, Tensor[] weights, Tensor? kl, float kl_scale, Tensor(a!) loss, Tensor(b!) ll, "
           "Tensor(c!) ws) -> ()", _elbo_loss_weighted_fwd)


def _elbo_loss_weighted_bwd(Fs, Ys, noise, noise_idx, n_views, view_off, weights, gloss, n_kl, kl_scale, dFs, dnoise,
                            dkl, ws):
    n, terms, _, _ = _ll_arrays(Fs, Ys, noise, noise_idx)
    nv, offp, Wp, _, _keep = _view_tables(n, n_views, view_off, weights)
    grads = _grad_arrays(dFs, dnoise, noise_idx)
    _lib.check(_lib.load().gpsa_elbo_loss_weighted_bwd(n, *terms, nv, offp, Wp, gloss.data_ptr(), int(n_kl),
                                                       float(kl_scale), *grads, 0 if dkl is None else dkl.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), _raw_stream(gloss.device.index)),
               "gpsa_elbo_loss_weighted_bwd")


_engine_op("elbo_loss_weighted_bwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] n_views, "
           "int[] view_off, Tensor[] weights, Tensor gloss, int n_kl, float kl_scale, Tensor(a!)[] dFs, "
           "Tensor(b!) dnoise, Tensor(c!)? dkl, Tensor(d!) ws) -> ()", _elbo_loss_weighted_bwd)


# ---------------------------------------------------------------------------------------------------------
# partly observed outputs (model.skip_missing; csrc/missing.hip, csrc/loss_views.hip): a NaN in Y is a missing observation
# ---------------------------------------------------------------------------------------------------------
def count_workspace_bytes():
    return int(_lib.load().gpsa_count_observed_workspace()) + 64


def _count_observed(Ys, n_views, view_off, nobs, ws):
    """gpsa_count_observed: nobs[i][v] = the non-NaN entries of Ys[i] in view v's rows (empty n_views: one view per term),
    device doubles written without a host read"""
    n = len(Ys)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    nv, offp, _, _, _keep = _view_tables(n, n_views, view_off)
    _lib.check(_lib.load().gpsa_count_observed(n, arr(Ys), (C.c_longlong * n)(*[int(y.shape[0]) for y in Ys]),
                                               (C.c_int * n)(*[int(y.shape[1]) for y in Ys]), nv, offp, arr(nobs),
                                               ws.data_ptr(), ws.numel(), _raw_stream(ws.device.index)),
               "gpsa_count_observed")


_engine_op("count_observed(Tensor[] Ys, int[] n_views, int[] view_off, Tensor(a!)[] nobs, Tensor(b!) ws) -> ()",
           _count_observed)


def _elbo_loss_skip_fwd(Fs, Ys, noise, noise_idx, shapes, fused, n_views, view_off, weights, nobs, kl, kl_scale, loss, ll,
                        ws):
    """gpsa_elbo_loss_skip_fwd: the ELBO loss over the observed entries (fused: per term, "F" is its partial sums of z^2;
    shapes as elbo_loss_fused_fwd, both empty without fused terms; n_views / view_off / weights empty: none)"""
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes or None, fused or None)
    nv, offp, Wp, Np, _keep = _view_tables(n, n_views, view_off, weights, nobs)
    _lib.check(_lib.load().gpsa_elbo_loss_skip_fwd(n, *terms, Zp, nparts, nv, offp, Wp, Np, *_kl_args(kl), float(kl_scale),
                                                   loss.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _raw_stream(loss.device.index)), "gpsa_elbo_loss_skip_fwd")


_engine_op("elbo_loss_skip_fwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "int[] n_views, int[] view_off, Tensor[] weights, Tensor[] nobs, Tensor? kl, float kl_scale, Tensor(a!) loss, "
           "Tensor(b!) ll, Tensor(c!) ws) -> ()", _elbo_loss_skip_fwd)


def _elbo_loss_skip_bwd(Fs, Ys, noise, noise_idx, shapes, fused, n_views, view_off, weights, nobs, gloss, n_kl, kl_scale,
                        dFs, dnoise, dkl, ws):
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes or None, fused or None)
    nv, offp, Wp, Np, _keep = _view_tables(n, n_views, view_off, weights, nobs)
    grads = _grad_arrays(dFs, dnoise, noise_idx, fused or None)
    _lib.check(_lib.load().gpsa_elbo_loss_skip_bwd(n, *terms, Zp, nparts, nv, offp, Wp, Np, gloss.data_ptr(), int(n_kl),
                                                   float(kl_scale), *grads, 0 if dkl is None else dkl.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), _raw_stream(gloss.device.index)),
               "gpsa_elbo_loss_skip_bwd")


_engine_op("elbo_loss_skip_bwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "int[] n_views, int[] view_off, Tensor[] weights, Tensor[] nobs, Tensor gloss, int n_kl, float kl_scale, "
           "Tensor(a!)[] dFs, Tensor(b!) dnoise, Tensor(c!)? dkl, Tensor(d!) ws) -> ()", _elbo_loss_skip_bwd)


def _lmc_loglik_fused_skip(F, W, Y, noise, noise_idx, zpart, dF, dW, ws):
    """gpsa_lmc_loglik_fused_skip_f32: lmc_loglik_fused with the NaN entries of Y left out of all three products"""
    S, N, L = (int(d) for d in F.shape)
    _lib.check(_lib.load().gpsa_lmc_loglik_fused_skip_f32(F.data_ptr(), W.data_ptr(), Y.data_ptr(),
                                                          noise.data_ptr() + 4 * int(noise_idx), S, N, L,
                                                          int(W.shape[1]), zpart.data_ptr(), zpart.numel(),
                                                          dF.data_ptr(), dW.data_ptr(), ws.data_ptr(), ws.numel(),
                                                          _raw_stream(F.device.index)),
               "gpsa_lmc_loglik_fused_skip_f32")


_engine_op("lmc_loglik_fused_skip(Tensor F, Tensor W, Tensor Y, Tensor noise, int noise_idx, Tensor(a!) zpart, "
           "Tensor(b!) dF, Tensor(c!) dW, Tensor(d!) ws) -> ()", _lmc_loglik_fused_skip)


# ---------------------------------------------------------------------------------------------------------
# count outputs (model.likelihood; csrc/poisson.hip, csrc/loss_views.hip): the Poisson likelihood term
# ---------------------------------------------------------------------------------------------------------
def lgamma_workspace_bytes():
    return int(_lib.load().gpsa_lgamma_sum_workspace()) + 64


def _opt_ptrs(n, ts):
    """host array of n device pointers, NULL for None; an absent table (empty list) is NULL"""
    return (C.c_void_p * n)(*[0 if t is None else t.data_ptr() for t in ts]) if ts else None


def _lgamma_sum(Ys, n_views, view_off, skip, out, ws):
    """gpsa_lgamma_sum: out[i][v] = sum of lgamma(Ys[i] + 1) over view v's rows (empty n_views: one view per term; skip:
    NaN entries left out), device doubles written without a host read"""
    n = len(Ys)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    nv, offp, _, _, _keep = _view_tables(n, n_views, view_off)
    _lib.check(_lib.load().gpsa_lgamma_sum(n, arr(Ys), (C.c_longlong * n)(*[int(y.shape[0]) for y in Ys]),
                                           (C.c_int * n)(*[int(y.shape[1]) for y in Ys]), nv, offp, int(skip), arr(out),
                                           ws.data_ptr(), ws.numel(), _raw_stream(ws.device.index)), "gpsa_lgamma_sum")


_engine_op("lgamma_sum(Tensor[] Ys, int[] n_views, int[] view_off, int skip, Tensor(a!)[] out, Tensor(b!) ws) -> ()",
           _lgamma_sum)


def _pois_tables(n, n_views, view_off, weights, nobs, kinds, lgam, offsets):
    nv, offp, Wp, _, keep = _view_tables(n, n_views, view_off, weights)
    return (nv, offp, Wp, _opt_ptrs(n, nobs), (C.c_int * n)(*[int(k) for k in kinds]), _opt_ptrs(n, lgam),
            _opt_ptrs(n, offsets)), keep


def _elbo_loss_pois_fwd(Fs, Ys, noise, noise_idx, shapes, fused, n_views, view_off, weights, nobs, kinds, lgam, offsets,
                        skip, kl, kl_scale, loss, ll, ws):
    """gpsa_elbo_loss_pois_fwd: the ELBO loss of a model with Poisson terms (kinds: GPSA_LIK_* per term; lgam / offsets /
    nobs: per term a tensor or None; the other tables as elbo_loss_skip_fwd)"""
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes or None, fused or None)
    tabs, _keep = _pois_tables(n, n_views, view_off, weights, nobs, kinds, lgam, offsets)
    _lib.check(_lib.load().gpsa_elbo_loss_pois_fwd(n, *terms, Zp, nparts, *tabs, int(skip), *_kl_args(kl), float(kl_scale),
                                                   loss.data_ptr(), ll.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _raw_stream(loss.device.index)), "gpsa_elbo_loss_pois_fwd")


_engine_op("elbo_loss_pois_fwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "int[] n_views, int[] view_off, Tensor[] weights, Tensor?[] nobs, int[] kinds, Tensor?[] lgam, "
           "Tensor?[] offsets, int skip, Tensor? kl, float kl_scale, Tensor(a!) loss, Tensor(b!) ll, Tensor(c!) ws) -> ()",
           _elbo_loss_pois_fwd)


def _elbo_loss_pois_bwd(Fs, Ys, noise, noise_idx, shapes, fused, n_views, view_off, weights, nobs, kinds, lgam, offsets,
                        skip, gloss, n_kl, kl_scale, dFs, dnoise, dkl, ws):
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes or None, fused or None)
    tabs, _keep = _pois_tables(n, n_views, view_off, weights, nobs, kinds, lgam, offsets)
    grads = _grad_arrays(dFs, dnoise, noise_idx, fused or None)
    _lib.check(_lib.load().gpsa_elbo_loss_pois_bwd(n, *terms, Zp, nparts, *tabs, int(skip), gloss.data_ptr(), int(n_kl),
                                                   float(kl_scale), *grads, 0 if dkl is None else dkl.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), _raw_stream(gloss.device.index)),
               "gpsa_elbo_loss_pois_bwd")


_engine_op("elbo_loss_pois_bwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "int[] n_views, int[] view_off, Tensor[] weights, Tensor?[] nobs, int[] kinds, Tensor?[] lgam, "
           "Tensor?[] offsets, int skip, Tensor gloss, int n_kl, float kl_scale, Tensor(a!)[] dFs, Tensor(b!) dnoise, "
           "Tensor(c!)? dkl, Tensor(d!) ws) -> ()", _elbo_loss_pois_bwd)


def _lmc_loglik_fused_pois(F, W, Y, offset, skip, zpart, dF, dW, ws):
    """gpsa_lmc_loglik_fused_pois_f32: lmc_loglik_fused for a Poisson modality - F W is the log rate, zpart sums
    y eta - exp(eta), eta = F W + offset[row] (offset: [N] or None)"""
    S, N, L = (int(d) for d in F.shape)
    _lib.check(_lib.load().gpsa_lmc_loglik_fused_pois_f32(F.data_ptr(), W.data_ptr(), Y.data_ptr(),
                                                          0 if offset is None else offset.data_ptr(), int(skip), S, N, L,
                                                          int(W.shape[1]), zpart.data_ptr(), zpart.numel(),
                                                          dF.data_ptr(), dW.data_ptr(), ws.data_ptr(), ws.numel(),
                                                          _raw_stream(F.device.index)),
               "gpsa_lmc_loglik_fused_pois_f32")


_engine_op("lmc_loglik_fused_pois(Tensor F, Tensor W, Tensor Y, Tensor? offset, int skip, Tensor(a!) zpart, "
           "Tensor(b!) dF, Tensor(c!) dW, Tensor(d!) ws) -> ()", _lmc_loglik_fused_pois)


# ---------------------------------------------------------------------------------------------------------
# count outputs (model.likelihood = "negative_binomial"; csrc/negbin.hip, csrc/loss_views.hip): the negative binomial term
# ---------------------------------------------------------------------------------------------------------
def nb_const_workspace_bytes(Ys, n_views):
    lib = _lib.load()
    return max(int(lib.gpsa_nb_const_workspace(int(y.shape[0]), int(y.shape[1]), int(n_views[i]) if n_views else 1))
               for i, y in enumerate(Ys)) + 64


def nb_loss_workspace_bytes(shapes, n_views, kinds):
    """gpsa_elbo_loss_nb_workspace for the terms' [S, N, P] (flattened), view counts (empty: one view each) and kinds"""
    n = len(shapes) // 3
    nv = (C.c_int * n)(*[int(v) for v in n_views]) if n_views else None
    return int(_lib.load().gpsa_elbo_loss_nb_workspace(n, (C.c_int * n)(*shapes[0::3]), (C.c_longlong * n)(*shapes[1::3]),
                                                       (C.c_int * n)(*shapes[2::3]), nv,
                                                       (C.c_int * n)(*[int(k) for k in kinds]))) + 64


def _nb_const(Ys, disp, n_views, view_off, weights, skip, csum, dconst, ws):
    """gpsa_nb_const: per NB term, csum[i][v] = sum of lgamma(y + r) - lgamma(r) over view v's rows and dconst[i][p] = the
    view-weighted sum over rows of r (psi(y + r) - psi(r)), r = exp(disp[i]); device doubles, no host read"""
    n = len(Ys)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    nv, offp, Wp, _, _keep = _view_tables(n, n_views, view_off, weights)
    _lib.check(_lib.load().gpsa_nb_const(n, arr(Ys), (C.c_longlong * n)(*[int(y.shape[0]) for y in Ys]),
                                         (C.c_int * n)(*[int(y.shape[1]) for y in Ys]), arr(disp), nv, offp, Wp, int(skip),
                                         arr(csum), arr(dconst), ws.data_ptr(), ws.numel(),
                                         _raw_stream(ws.device.index)), "gpsa_nb_const")


_engine_op("nb_const(Tensor[] Ys, Tensor[] disp, int[] n_views, int[] view_off, Tensor[] weights, int skip, "
           "Tensor(a!)[] csum, Tensor(b!)[] dconst, Tensor(c!) ws) -> ()", _nb_const)


def _elbo_loss_nb_fwd(Fs, Ys, noise, noise_idx, shapes, fused, n_views, view_off, weights, nobs, kinds, lgam, offsets,
                      disp, csum, skip, kl, kl_scale, loss, ll, ws):
    """gpsa_elbo_loss_nb_fwd: the ELBO loss of a model with negative binomial terms (elbo_loss_pois_fwd's tables; disp /
    csum: per term a tensor or None - rho and gpsa_nb_const's per-view table)"""
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes or None, fused or None)
    tabs, _keep = _pois_tables(n, n_views, view_off, weights, nobs, kinds, lgam, offsets)
    _lib.check(_lib.load().gpsa_elbo_loss_nb_fwd(n, *terms, Zp, nparts, *tabs, _opt_ptrs(n, disp), _opt_ptrs(n, csum),
                                                 int(skip), *_kl_args(kl), float(kl_scale), loss.data_ptr(), ll.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _raw_stream(loss.device.index)),
               "gpsa_elbo_loss_nb_fwd")


_engine_op("elbo_loss_nb_fwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "int[] n_views, int[] view_off, Tensor[] weights, Tensor?[] nobs, int[] kinds, Tensor?[] lgam, "
           "Tensor?[] offsets, Tensor?[] disp, Tensor?[] csum, int skip, Tensor? kl, float kl_scale, Tensor(a!) loss, "
           "Tensor(b!) ll, Tensor(c!) ws) -> ()", _elbo_loss_nb_fwd)


def _elbo_loss_nb_bwd(Fs, Ys, noise, noise_idx, shapes, fused, n_views, view_off, weights, nobs, kinds, lgam, offsets,
                      disp, dconst, usum, skip, gloss, n_kl, kl_scale, dFs, dnoise, dkl, ddisp, ws):
    """gpsa_elbo_loss_nb_bwd (dconst: gpsa_nb_const's per-output table; usum: a fused NB term's per-output sums of u;
    ddisp: per term the gradient of rho, written for the NB terms - the other terms' entries are not touched)"""
    n, terms, Zp, nparts = _ll_arrays(Fs, Ys, noise, noise_idx, shapes or None, fused or None)
    tabs, _keep = _pois_tables(n, n_views, view_off, weights, nobs, kinds, lgam, offsets)
    grads = _grad_arrays(dFs, dnoise, noise_idx, fused or None)
    _lib.check(_lib.load().gpsa_elbo_loss_nb_bwd(n, *terms, Zp, nparts, *tabs, _opt_ptrs(n, disp),
                                                 _opt_ptrs(n, dconst), _opt_ptrs(n, usum), int(skip), gloss.data_ptr(),
                                                 int(n_kl), float(kl_scale), *grads, 0 if dkl is None else dkl.data_ptr(),
                                                 _opt_ptrs(n, ddisp), ws.data_ptr(), ws.numel(),
                                                 _raw_stream(gloss.device.index)), "gpsa_elbo_loss_nb_bwd")


_engine_op("elbo_loss_nb_bwd(Tensor[] Fs, Tensor[] Ys, Tensor noise, int[] noise_idx, int[] shapes, int[] fused, "
           "int[] n_views, int[] view_off, Tensor[] weights, Tensor?[] nobs, int[] kinds, Tensor?[] lgam, "
           "Tensor?[] offsets, Tensor?[] disp, Tensor?[] dconst, Tensor?[] usum, int skip, Tensor gloss, int n_kl, "
           "float kl_scale, Tensor(a!)[] dFs, Tensor(b!) dnoise, Tensor(c!)? dkl, Tensor(d!)[] ddisp, Tensor(e!) ws) -> ()",
           _elbo_loss_nb_bwd)


def _lmc_loglik_fused_nb(F, W, Y, offset, disp, skip, zpart, dF, dW, usum, ws):
    """gpsa_lmc_loglik_fused_nb_f32: lmc_loglik_fused for a negative binomial modality - F W is the log mean, zpart sums
    t = y a - (y + r) softplus(a), a = F W + offset[row] - disp[p] (offset: [N] or None), usum [P] fp64 receives the
    per-output sums of u (elbo_loss_nb_bwd's usum)"""
    S, N, L = (int(d) for d in F.shape)
    _lib.check(_lib.load().gpsa_lmc_loglik_fused_nb_f32(F.data_ptr(), W.data_ptr(), Y.data_ptr(),
                                                        0 if offset is None else offset.data_ptr(), disp.data_ptr(),
                                                        int(skip), S, N, L, int(W.shape[1]), zpart.data_ptr(),
                                                        zpart.numel(), dF.data_ptr(), dW.data_ptr(), usum.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), _raw_stream(F.device.index)),
               "gpsa_lmc_loglik_fused_nb_f32")


_engine_op("lmc_loglik_fused_nb(Tensor F, Tensor W, Tensor Y, Tensor? offset, Tensor disp, int skip, Tensor(a!) zpart, "
           "Tensor(b!) dF, Tensor(c!) dW, Tensor(d!) usum, Tensor(e!) ws) -> ()", _lmc_loglik_fused_nb)
