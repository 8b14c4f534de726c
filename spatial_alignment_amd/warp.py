"""``warp_field`` / ``unwarp`` / ``transfer``: the learned alignment itself, as a function of the point.

After a fit the model holds, per non-fixed view ``v``, a warp whose mean is closed form in the point - the function
``predict`` evaluates as ``G_mean`` at the training rows (vgpsa.py:174-204, mean only):

    g_v(x) = x A_v + b_v + k(x, Z_v) beta_v,      beta_v = K_uu^-1 (delta_G[v] - (Z_v A_v + b_v))        [M, D]

with ``A_v = mean_slopes[v]``, ``b_v = mean_intercepts[v]``, ``Z_v = Xtilde[v]`` and ``K_uu`` the warp prior with
``diagonal_offset``, factorised as ``predict`` factorises it.  This module evaluates, at ANY points of a view's native
coordinates (a lattice for a plot, the pixels of an image - no data stage, no row-to-view bookkeeping, no [M, C] panels):

* ``warp_field``: ``g_v``, its Jacobian ``J[n, j, d] = d g_j / d x_d`` and ``det J`` - the local area / volume change; a
  ``det <= 0`` means the warp folds the slice there (the reference's experiments plot this from finite differences of
  scattered points: plot_slideseq_deformation_field.py, warp_parameter_demo.py);
* ``unwarp``: the way back - where a location of the aligned system lies in view ``v``'s own coordinates - by Newton's
  iteration on ``g_v(x) = G`` with the exact Jacobian, a fixed number of updates in one launch;
* ``transfer``: a point of view a in view b's coordinates, ``unwarp(warp_field(X, a).G_mean, b)``.

``beta`` is formed once per call in fp64 from the fp32 parameters (``delta - (Z A + b)`` by gpsa_mean_resid_fwd, which
rounds nothing through fp32; ``K_uu^-1`` from engine.factor_batch); the per-point work is csrc/warp_field.hip, all fp64.
A row's result does not depend on the other rows, on their number or on ``rows_per_chunk``, bit for bit.  Fixed views
are the identity (``J = I``, ``det = 1``, ``residual = 0``) without any device work, so they also answer on a CPU model.

Everything here runs without gradients and leaves the model as it found it (no ``eval()``, nothing of the forward ->
``loss_fn`` hand-off, no generator touched).  Not offered: derivatives of ``G_scale``, sampled warps, gradients through
these calls.
"""
import operator

import torch

from . import engine as E
from .kernels import builtin_kind
from .predict import Prediction, _fixed_splitk

DEFAULT_MAX_ITER = 12
REL_TOL = 1e-8  # unwarp's default tolerance, relative to the extent of the view's inducing points

f64 = torch.float64


def _check_view(model, view, what):
    V = int(model.n_views)
    try:
        idx = None if isinstance(view, bool) else operator.index(view)
    except TypeError:
        idx = None
    if idx is None or not 0 <= idx < V:
        raise ValueError(f"{what}: view must be an integer in [0, {V}), not {view!r}")
    return idx


def _check_points(model, t, name, what):
    D = int(model.n_spatial_dims)
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != D:
        shape = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} has shape {shape}, [n, {D}] is needed")
    return t.detach().to(device=model.Xtilde.device, dtype=f64).contiguous()


def _check_kind(model, what):
    kind = builtin_kind(model.kernel_func_warp)
    if kind is None:
        raise ValueError(f"{what}: the warp kernel is not one of the built-ins (rbf_kernel, matern12_kernel, "
                         "matern32_kernel); no derivative of a plug-in covariance is available")
    return kind


def _extent(model, view):
    """largest coordinate range of the view's inducing points"""
    Z = model.Xtilde[view].detach().double()
    return float((Z.max(0).values - Z.min(0).values).max())


def _warp_model(model, view, o):
    """(kind, Z, beta, A, b, ls_u, var_u) of a non-fixed view, fp64 on the device; once per call"""
    kind = _check_kind(model, "warp")
    Z32 = model.Xtilde[view].detach()
    Z = Z32.double().contiguous()
    ls_u = model.warp_kernel_lengthscales[view].detach().double().reshape(1)
    var_u = model.warp_kernel_variances[view].detach().double().reshape(1)
    slopes, icpt = model.mean_slopes[view].detach(), model.mean_intercepts[view].detach()
    Kuu = model._kmat("warp", Z, Z, ls_u, var_u, model.diagonal_offset, f64, True)
    parts = E.factor_batch([Kuu.unsqueeze(0)])[0]
    if model.check_numerics and int(parts[3].reshape(-1).max()) != 0:
        raise torch.linalg.LinAlgError(f"GPSA warp_field: the warp prior of view {view} is not positive-definite "
                                       "(forward raises here too)")
    fac = E.Factor(parts=parts)
    _, dc = o.mean_resid_fwd(Z32, slopes, icpt, model.delta_G_list[view].detach(), 1.0)  # fp64 from the fp32 parameters
    beta = o.gemm(fac.Kinv, dc, splitk=_fixed_splitk(int(Z.shape[0])))
    return kind, Z, beta, slopes.double().contiguous(), icpt.double().contiguous(), ls_u, var_u


def _chunk(rows_per_chunk, n):
    if rows_per_chunk is None:
        return max(n, 1)
    if int(rows_per_chunk) != rows_per_chunk or rows_per_chunk < 1:
        raise ValueError(f"rows_per_chunk must be a positive integer, not {rows_per_chunk!r}")
    return int(rows_per_chunk)


@torch.no_grad()
def warp_field(model, X, view, *, jacobian=True, rows_per_chunk=None):
    """The mean of view ``view``'s learned warp at ``X`` [n, D] (any points in that view's native coordinates), with its
    Jacobian and the folding check; see the module docstring.

    Returns a ``Prediction`` (a dict whose entries also read as attributes), everything fp64 on the model's device:
    ``G_mean`` [n, D], ``jacobian`` [n, D, D] (``jacobian[n, j, d] = d G_mean[n, j] / d X[n, d]``), ``det`` [n] (the local
    area / volume change; ``det <= 0``: the warp folds there) and ``n_folded`` (0-dim int64: the count of ``det <= 0``).
    ``jacobian=False``: ``G_mean`` alone, the other three are None.
    rows_per_chunk: rows per launch (default: all at once; the result does not depend on it, bit for bit).
    Raises ValueError for a bad ``view``, an ``X`` that is not [n, D], or a warp kernel that is not a built-in.
    """
    view = _check_view(model, view, "warp_field")
    X = _check_points(model, X, "X", "warp_field")
    c = _chunk(rows_per_chunk, X.shape[0])
    n, D, dev = int(X.shape[0]), int(X.shape[1]), X.device
    if model._is_fixed(view):  # vgpsa.py:262-273: the identity
        G = X.clone()
        J = torch.eye(D, dtype=f64, device=dev).expand(n, D, D).contiguous() if jacobian else None
        det = torch.ones(n, dtype=f64, device=dev) if jacobian else None
    else:
        _check_kind(model, "warp_field")
        G = torch.empty(n, D, dtype=f64, device=dev)
        J = torch.empty(n, D, D, dtype=f64, device=dev) if jacobian else None
        det = torch.empty(n, dtype=f64, device=dev) if jacobian else None
        if n:
            o = E.ops()
            mdl = _warp_model(model, view, o)
            for a in range(0, n, c):
                cut = lambda t: None if t is None else t[a: a + c]
                o.warp_field(*mdl, X[a: a + c], jacobian=jacobian, out=(G[a: a + c], cut(J), cut(det)))
    return Prediction(G_mean=G, jacobian=J, det=det, n_folded=(det <= 0).sum() if jacobian else None)


@torch.no_grad()
def unwarp(model, G, view, *, max_iter=DEFAULT_MAX_ITER, tol=None, x0=None, rows_per_chunk=None):
    """Where the aligned locations ``G`` [n, D] lie in view ``view``'s own coordinates: ``X`` with ``g_view(X) = G``.

    Exactly ``max_iter`` undamped Newton updates ``x <- x - J(x)^-1 (g(x) - G)`` per row in one launch (no early exit),
    from ``x0`` [n, D] (default: the affine part alone, ``x0 = (G - b) A^-1``), with the exact Jacobian.

    Returns a ``Prediction``: ``X`` [n, D] fp64, ``residual`` [n] fp64 = ``|g(X) - G|_2`` evaluated at the returned ``X``,
    ``converged`` [n] bool = ``residual <= tol``, and ``tol`` (a float; default ``1e-8 *`` the largest coordinate range of
    the view's inducing points).  A row whose iteration met a singular or non-finite Jacobian or left the finite numbers
    is ``X = NaN``, ``residual = +inf``, ``converged = False``.

    The update is plain Newton: where the warp does not fold (``warp_field``'s ``n_folded == 0``) it converges
    quadratically from the default start.  UNDER A FOLDED WARP THE PREIMAGE IS NOT UNIQUE: the one returned depends on the
    start (the iteration is chaotic near a fold), and a row may fail to converge; ``residual`` / ``converged`` are honest
    either way.  Raises ValueError for a bad ``view``, a ``G`` or ``x0`` that is not [n, D], ``max_iter < 0``, ``tol <= 0``
    or a warp kernel that is not a built-in.
    """
    view = _check_view(model, view, "unwarp")
    G = _check_points(model, G, "G", "unwarp")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 0:
        raise ValueError(f"unwarp: max_iter must be an integer >= 0, not {max_iter!r}")
    if tol is not None and not float(tol) > 0.0:
        raise ValueError(f"unwarp: tol must be positive, not {tol!r}")
    if x0 is not None:
        x0 = _check_points(model, x0, "x0", "unwarp")
        if tuple(x0.shape) != tuple(G.shape):
            raise ValueError(f"unwarp: x0 has shape {tuple(x0.shape)}, G has {tuple(G.shape)}")
    c = _chunk(rows_per_chunk, G.shape[0])
    n, dev = int(G.shape[0]), G.device
    tol = REL_TOL * _extent(model, view) if tol is None else float(tol)
    if model._is_fixed(view):
        X, res = G.clone(), torch.zeros(n, dtype=f64, device=dev)
    else:
        _check_kind(model, "unwarp")
        X = torch.empty_like(G)
        res = torch.empty(n, dtype=f64, device=dev)
        if n:
            o = E.ops()
            mdl = _warp_model(model, view, o)
            if x0 is None:  # the affine part alone; A is D x D: inverted on the host
                A, b = mdl[3], mdl[4]
                x0 = ((G - b) @ torch.linalg.inv(A.cpu()).to(dev)).contiguous()
            for a in range(0, n, c):
                o.warp_invert(*mdl, G[a: a + c], x0[a: a + c], int(max_iter), out=(X[a: a + c], res[a: a + c]))
    return Prediction(X=X, residual=res, converged=res <= tol, tol=tol)


@torch.no_grad()
def transfer(model, X, view_from, view_to, **unwarp_kw):
    """``X`` [n, D], points of view ``view_from``, in view ``view_to``'s coordinates: through the aligned system and back,
    ``unwarp(warp_field(X, view_from).G_mean, view_to, **unwarp_kw)``.  Returns ``unwarp``'s result."""
    _check_view(model, view_to, "transfer")
    G = warp_field(model, X, view_from, jacobian=False).G_mean
    return unwarp(model, G, view_to, **unwarp_kw)
