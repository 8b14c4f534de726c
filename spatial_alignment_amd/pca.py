"""Expression PCA on the device: the step between ``prepare_counts`` / ``standardize_views`` and ``fit()`` that reduces the
selected genes to a few components.

    pca = expression_pca(Y, n_samples_list, n_components=20, center="view")
    scores = pca.transform(Y, n_samples_list)            # [N, 20] fp32: the outputs to align on
    Y_hat = pca.inverse_transform(scores, n_samples_list)  # predictions mapped back through the loadings

Two passes over ``Y`` [N, P] fp32 are HIP kernels of their own (csrc/pca.hip): the P x P Gram of the centred (and scaled)
matrix on the fp64 matrix cores, and the projection on the components.  Both form ``z = (y - mean) * inv_scale`` in fp64
from the stored fp32 value as the operand is staged: nothing of N x P elements is allocated.  The means (and the count
of non-finite values) come from the ``column_moments`` pass.  The solver on C = G / (N - 1) is orthogonal iteration built
from the dense product and the small factorisation that exist (``gpsa_gemm``, ``gpsa_chol_inv_f64``):

    Z = C Q;   Q = Z L^-T with L L^T = Z^T Z, applied twice (Cholesky-QR 2);
    every ``check_every`` iterations and at the end, Rayleigh-Ritz: B = Q^T C Q ((k + oversample)^2 doubles) is read to
    the host, decomposed with numpy.linalg.eigh, and the rotation uploaded - one host round trip per check.

The checks sit at fixed iteration numbers and every sum runs in a fixed order: a repeated call gives the same bits.
``solver="host"`` reads C to the host and calls numpy.linalg.eigh on it: the fallback, and the layer that separates an
error of the covariance from an error of the solver.

Conventions are sklearn's PCA: ``explained_variance`` has N - 1 in the denominator, and in each component the entry of
largest magnitude is positive (ties: the lower index).  ``center="view"`` subtracts each view's own column mean and, with
``scale=True``, divides by each view's own standard deviation (ddof = 0): the reference's per-slice
``(Y - Y.mean(0)) / Y.std(0)`` folded into the decomposition.  ``center="pooled"`` treats all rows as one view.  A column
whose variance inside a view is at most ``4 n eps`` times its mean square there counts as constant and contributes 0
(the variance is the difference of two fp64 moments: below that bound it is rounding).
"""
import numpy as np
import torch

from ._args import describe, ops as _ops, view_counts, view_offsets
from .predict import Prediction

f64, f32 = torch.float64, torch.float32
CENTERS = ("pooled", "view")
SOLVERS = ("subspace", "host")
MAX_K = 128         # components per launch of the projection (csrc/pca.hip: PCA_MAX_K)
MAX_BLOCK = 256     # columns of the iteration's block: gpsa_chol_inv_f64 factorises up to 256 x 256 in one sweep
EPS = float(np.finfo(np.float64).eps)


class ExpressionPCA(Prediction):
    """The result of ``expression_pca``: ``components`` [k, P] fp64, ``explained_variance`` [k] (N - 1 in the denominator),
    ``explained_variance_ratio``, ``singular_values``, ``mean`` [V, P] (one row with ``center="pooled"``), ``inv_scale``
    [V, P] or None, ``total_variance`` (the trace of the covariance), ``n_rows``, ``residual`` [k] = |C v_i - l_i v_i|_2 /
    l_1, ``n_iter``, ``converged``, ``center``, ``n_views``."""

    def _offsets(self, N, n_samples_list, what):
        if self.center == "pooled":
            return [0, N]
        ns = _views(n_samples_list, N, what)
        if len(ns) != self.n_views:
            raise ValueError(f"{what}: the decomposition was centred on {self.n_views} views; n_samples_list has "
                             f"{len(ns)}")
        return view_offsets(ns)

    @torch.no_grad()
    def transform(self, Y, n_samples_list=None, out_dtype=torch.float32):
        """scores [N, k] of ``Y`` [N, P] fp32 on the device: ``(y - mean) * inv_scale`` on the components, with the
        training means (``center="view"``: the means of the view a row belongs to, so ``n_samples_list`` must name as
        many views as the training call).  fp64 accumulation; fp32 (rounded once) or fp64 out."""
        what = "ExpressionPCA.transform"
        N, P = _check_matrix(Y, what)
        if P != self.components.shape[1]:
            raise ValueError(f"{what}: Y has {P} columns, the components {self.components.shape[1]}")
        off = self._offsets(N, n_samples_list, what)
        o, k = _ops(), int(self.components.shape[0])
        if k <= MAX_K:
            return o.pca_project(Y, self.mean, off, self.components, self.inv_scale, out_dtype)
        out = torch.empty(N, k, dtype=out_dtype, device=Y.device)
        for j0 in range(0, k, MAX_K):
            out[:, j0:j0 + MAX_K] = o.pca_project(Y, self.mean, off, self.components[j0:j0 + MAX_K].contiguous(),
                                                  self.inv_scale, out_dtype)
        return out

    @torch.no_grad()
    def inverse_transform(self, scores, n_samples_list=None):
        """[N, P] fp32 = scores components, un-scaled and un-centred with the training means, through ``gpsa_gemm`` in
        fp64 over blocks of rows (at most 32 MiB of fp64 at a time), rounded to fp32 once; ``center="view"`` needs
        ``n_samples_list`` (whose means and scales to put back)."""
        what = "ExpressionPCA.inverse_transform"
        k, P = (int(s) for s in self.components.shape)
        if not torch.is_tensor(scores) or scores.dim() != 2 or scores.shape[1] != k or scores.shape[0] < 1 \
                or not scores.is_floating_point():
            raise ValueError(f"{what}: scores must be a floating [N >= 1, {k}], not {describe(scores)}")
        if scores.device != self.components.device:
            raise ValueError(f"{what}: scores are on {scores.device}, the components on {self.components.device}")
        N = int(scores.shape[0])
        off = self._offsets(N, n_samples_list, what)
        o = _ops()
        S = scores.detach()
        out = torch.empty(N, P, dtype=f32, device=S.device)
        step = max(1, (1 << 22) // P)  # rows per product: the fp64 block stays at 32 MiB, then it is rounded once
        for v in range(len(off) - 1):
            W = self.components
            if self.inv_scale is not None:
                inv = self.inv_scale[v]
                W = (W * torch.where(inv > 0, 1.0 / inv, torch.zeros_like(inv))).contiguous()  # a constant column: its mean
            for a in range(off[v], off[v + 1], step):
                b = min(a + step, off[v + 1])
                blk = o.gemm(S[a:b].to(f64).contiguous(), W)
                out[a:b] = blk.add_(self.mean[v])
        return out


def _check_matrix(Y, what, on_device=True):
    if not torch.is_tensor(Y) or Y.dim() != 2 or Y.shape[0] < 1 or Y.shape[1] < 1:
        raise ValueError(f"{what}: Y must be a dense [N, P] matrix, not {describe(Y)}")
    if Y.dtype != f32:
        raise ValueError(f"{what}: Y is {Y.dtype}; the kernels read fp32 as stored (what prepare_counts returns)")
    if not Y.is_contiguous():
        raise ValueError(f"{what}: Y is not contiguous (strides {tuple(Y.stride())}); pass Y.contiguous()")
    if on_device:
        _check_device(Y, what)
    return int(Y.shape[0]), int(Y.shape[1])


def _check_device(Y, what):
    if Y.device.type != "cuda":
        raise ValueError(f"{what}: Y is on device {str(Y.device)!r}; the PCA kernels run on the GPU only and there is no "
                         "host path - move the matrix to the device first")


def _views(n_samples_list, N, what):
    ns, ok = view_counts([N] if n_samples_list is None else n_samples_list, N)
    if not ok:
        raise ValueError(f"{what}: n_samples_list {ns} must hold positive row counts that sum to N = {N}")
    return ns


def _check_args(Y, n_samples_list, n_components, center, scale, solver, oversample, tol, max_iter, check_every, what):
    """every refusal of ``expression_pca`` that needs no launch -> (N, P, the view sizes the centring uses)"""
    if center not in CENTERS:
        raise ValueError(f"{what}: center must be one of {CENTERS}, not {center!r}")
    if solver not in SOLVERS:
        raise ValueError(f"{what}: solver must be one of {SOLVERS}, not {solver!r}")
    if not isinstance(scale, bool):
        raise ValueError(f"{what}: scale must be True or False, not {scale!r}")
    N, P = _check_matrix(Y, what, on_device=False)  # (the rules of the call first: they hold on any device)
    ns = _views(n_samples_list, N, what)
    if min(ns) < 2:
        raise ValueError(f"{what}: the views have {ns} rows; centring and a variance need at least 2 in every view")
    if center == "pooled":
        ns = [N]
    V = len(ns)
    kmax = min(P, N - V)
    if isinstance(n_components, bool) or not isinstance(n_components, int) or not 1 <= n_components <= kmax:
        raise ValueError(f"{what}: n_components = {n_components!r}; an int in 1 .. min(P, N - V) = {kmax} is needed "
                         f"(P = {P}, N = {N}, V = {V}: centring takes one degree of freedom per view)")
    if isinstance(oversample, bool) or not isinstance(oversample, int) or oversample < 0:
        raise ValueError(f"{what}: oversample must be an int >= 0, not {oversample!r}")
    if not (isinstance(tol, float) and tol > 0.0 and tol < float("inf")):
        raise ValueError(f"{what}: tol must be a positive float, not {tol!r}")
    for name, val in (("max_iter", max_iter), ("check_every", check_every)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 1:
            raise ValueError(f"{what}: {name} must be an int >= 1, not {val!r}")
    if solver == "subspace" and n_components > MAX_BLOCK:
        raise ValueError(f"{what}: solver='subspace' iterates on a block of at most {MAX_BLOCK} columns; n_components = "
                         f"{n_components} needs solver='host'")
    _check_device(Y, what)
    return N, P, ns


def block_width(n_components, oversample, P, N, V):
    """columns of the iteration's block: ``n_components + oversample`` with the oversampling reduced so that the block
    stays inside the covariance's rank bound min(P, N - V) (beyond it the block's Gram is singular) and inside what the
    small factorisation takes"""
    return min(n_components + oversample, P, N - V, MAX_BLOCK)


def start_block(P, m, seed):
    """the iteration's start [P, m] fp64: numpy's seeded generator on the host (the same numbers on every device)"""
    return np.random.default_rng(seed).standard_normal((P, m))


def sign_flip(components):
    """sklearn's rule (>= 1.5): in each row the entry of largest magnitude is positive, ties to the lower index"""
    a = components.abs()
    P = a.shape[1]
    idx = torch.arange(P, device=a.device).expand_as(a)
    first = torch.where(a == a.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, P)).min(dim=1).values
    sgn = torch.where(components.gather(1, first[:, None]) < 0, -1.0, 1.0).to(components.dtype)
    return components * sgn


def close_moments(s1, s2, ns, scale):
    """(mean [V, P], inv_scale [V, P] or None) from the sums of y and y^2 per (view, column); ddof = 0; a column with
    var <= 4 n eps mean(y^2) is constant: inv_scale 0"""
    n = torch.tensor(ns, dtype=f64, device=s1.device)[:, None]
    mean = s1 / n
    if not scale:
        return mean, None
    msq = s2 / n
    var = msq - mean * mean
    const = var <= 4.0 * n * EPS * msq
    inv = torch.where(const, torch.zeros_like(var), torch.rsqrt(torch.where(const, torch.ones_like(var), var)))
    return mean, inv.contiguous()


def _cholqr2(o, Z):
    """Z [P, m] fp64 -> an orthonormal basis of its columns: Z L^-T with L L^T = Z^T Z, twice"""
    for _ in range(2):
        Gm = o.gemm(Z, Z, transA=True)
        Linv, _, _ = o.chol_inv(Gm[None])
        Z = o.gemm(Z, Linv[0], transB=True)
    return Z


def _subspace(o, Cm, k, m, tol, max_iter, check_every, seed, what):
    """orthogonal iteration on Cm [P, P] -> (vectors [P, k], values [k], residual [k], n_iter, converged)"""
    P = int(Cm.shape[0])
    Q = torch.from_numpy(start_block(P, m, seed)).to(Cm.device)
    it, converged = 0, False
    while True:
        it += 1
        Q = _cholqr2(o, o.gemm(Cm, Q))
        if it % check_every and it < max_iter:
            continue
        # Rayleigh-Ritz: B = Q^T C Q to the host, its eigenvectors back
        Z = o.gemm(Cm, Q)
        B = o.gemm(Q, Z, transA=True).cpu().numpy()
        w, S = np.linalg.eigh(0.5 * (B + B.T))
        w, S = w[::-1].copy(), S[:, ::-1].copy()
        Sd = torch.from_numpy(S).to(Cm.device)
        Q, Z = o.gemm(Q, Sd), o.gemm(Z, Sd)
        wd = torch.from_numpy(w).to(Cm.device)
        R = Z - Q * wd
        res = np.sqrt(np.diagonal(o.gemm(R, R, transA=True).cpu().numpy())[:k].copy()) / w[0]
        if not np.all(np.isfinite(res)):
            raise RuntimeError(f"{what}: the iteration's block lost rank at iteration {it} (a non-finite residual); "
                               "use solver='host'")
        converged = bool(res.max() <= tol)
        if converged or it >= max_iter:
            return Q[:, :k], wd[:k], torch.from_numpy(res).to(Cm.device), it, converged


@torch.no_grad()
def expression_pca(Y, n_samples_list=None, n_components=50, center="pooled", scale=False, solver="subspace",
                   oversample=10, tol=1e-9, max_iter=300, check_every=10, seed=0):
    """Principal components of the dense fp32 matrix ``Y`` [N, P] on the device -> ``ExpressionPCA``.

    ``n_samples_list``: the views' row counts (consecutive row ranges; None: one view).  ``center``: "pooled" (one mean
    per column: plain PCA) or "view" (each view's own mean; with ``scale=True`` also each view's own standard deviation,
    ddof = 0, a constant column contributing 0).  ``solver``: "subspace" (orthogonal iteration on the device on a block of
    ``n_components + oversample`` columns, Rayleigh-Ritz every ``check_every`` iterations, until the largest residual
    |C v - l v| / l_1 is at most ``tol`` or ``max_iter`` is reached - ``converged`` says which) or "host" (the covariance
    read to the host, numpy.linalg.eigh).  ``oversample`` is reduced silently so that the block stays within
    min(P, N - V) columns.  ``seed`` fixes the start of the iteration.

    Refused with a ValueError before any launch: a ``Y`` that is not a contiguous fp32 device matrix, ``n_components``
    outside 1 .. min(P, N - V), a view of fewer than 2 rows; and after the moments pass: non-finite values."""
    what = "expression_pca"
    N, P, ns = _check_args(Y, n_samples_list, n_components, center, scale, solver, oversample, tol, max_iter,
                           check_every, what)
    V, off, k = len(ns), view_offsets(ns), n_components
    o = _ops()
    s1, s2, _, bad = o.column_moments(Y, "identity", off, own_workspace=True)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"{what}: Y holds {nbad} values that are NaN or infinite; a covariance needs finite values")
    mean, inv_scale = close_moments(s1, s2, ns, scale)
    del s1, s2
    Cm = o.pca_gram(Y, mean, off, inv_scale)
    Cm.mul_(1.0 / (N - 1))
    total = Cm.diagonal().sum()
    if solver == "host":
        w, U = np.linalg.eigh(Cm.cpu().numpy())
        lam = torch.from_numpy(w[::-1][:k].copy()).to(Cm.device)
        vec = torch.from_numpy(U[:, ::-1][:, :k].copy()).to(Cm.device)
        R = o.gemm(Cm, vec) - vec * lam
        res = torch.sqrt(o.gemm(R, R, transA=True).diagonal()) / lam[0]
        n_iter, converged = 0, True
    else:
        m = block_width(k, oversample, P, N, V)
        vec, lam, res, n_iter, converged = _subspace(o, Cm, k, m, tol, max_iter, check_every, seed, what)
    del Cm
    comps = sign_flip(vec.t().contiguous())
    return ExpressionPCA(components=comps, explained_variance=lam, explained_variance_ratio=lam / total,
                         singular_values=torch.sqrt(lam.clamp_min(0.0) * (N - 1)), mean=mean, inv_scale=inv_scale,
                         total_variance=float(total), n_rows=N, residual=res, n_iter=n_iter, converged=converged,
                         center=center, n_views=V)


def init_lmc_from_pca(model, pca, modality="expression"):
    """Opt-in start of the LMC loadings: ``components * sqrt(explained_variance)[:, None]`` copied into
    ``model.W_dict[modality]`` ([n_latent_gps, P]).  The default ``torch.randn`` start is untouched unless this is
    called.  ValueError for a model without LMC on the modality or a shape that does not match."""
    what = "init_lmc_from_pca"
    W = getattr(model, "W_dict", None)
    if W is None or modality not in W:
        raise ValueError(f"{what}: the model has no LMC loadings for modality {modality!r} (n_latent_gps is None there)")
    comps, lam = pca["components"], pca["explained_variance"]
    if tuple(W[modality].shape) != tuple(comps.shape):
        raise ValueError(f"{what}: W_dict[{modality!r}] is {tuple(W[modality].shape)} = [n_latent_gps, P]; the "
                         f"decomposition has components {tuple(comps.shape)}")
    with torch.no_grad():
        load = comps * torch.sqrt(lam.clamp_min(0.0))[:, None]
        W[modality].copy_(load.to(device=W[modality].device, dtype=W[modality].dtype))
    return model
