"""Exact GP regression on the device: fit, log marginal likelihood, predict - the reference's prediction baselines.

``sklearn.gaussian_process.GaussianProcessRegressor`` with ``RBF() + WhiteKernel()`` or ``Matern(nu=1.5) + WhiteKernel()``
is what every GPSA prediction figure is held against (the "union" GP on the unaligned coordinates, the "separate" GP per
view, the GP on the aligned coordinates: experiments/simulations/two_dimensional_prediction.py:126-155, 238,
one_dimensional_prediction.py:128-139, expression/st/st_prediction.py:142-156, 251) and what gives the data kernel's
starting length scale (two_dimensional.py:84-91).  With the coordinates and the outputs already in HBM this is thin
Python over three HIP entries (csrc/gpr.hip: ``gpsa_gpr_cov_f64``, ``gpsa_gpr_lml_grad_f64``, ``gpsa_gpr_mean_f64``) and
what existed: ``gpsa_chol_inv_blocked_f64`` and the fp64 ``gpsa_gemm``.

The model is sklearn's ``GaussianProcessRegressor(kernel, alpha=jitter, normalize_y=False)`` for ``[C *] k + WhiteKernel``:

    K(theta) = a k(X, X; l) + (tau2 + jitter) I,      theta = (log a, log l, log tau2),   a = 1 unless ``amplitude``
    LML = -1/2 sum_p y_p^T K^-1 y_p - P sum_i log L_ii - 1/2 N P log 2 pi            (the P outputs share one theta)
    dLML / dtheta_k = 1/2 sum_ij (alpha alpha^T - P K^-1)_ij dK_ij / dtheta_k,     alpha = K^-1 Y

in sklearn's kernel forms (rbf ``exp(-d^2 / (2 l^2))``, matern32 ``(1 + r) exp(-r)`` with ``r = sqrt(3) d / l``, matern12
``exp(-d / l)``), which are not the forms of ``kernels.py``.  Everything is fp64, runs under ``torch.no_grad()`` and
touches no model state.  Tensors on the CPU are refused with a ``ValueError`` that names the device: there is no host path.

Memory: one evaluation holds K, L^-1 and K^-1 (8 N^2 bytes each) and the factorisation's workspace (16 N^2 + 8 * 256 N
bytes): about 40 N^2 bytes, 1 GB at N = 5000 (``gpr_bytes``); a size that does not fit the device's free memory is refused
before anything is allocated.  A fitted ``GPRegression`` keeps X, alpha and L^-1.

The optimiser is host code (no scipy): a projected BFGS ascent in theta with a dense inverse Hessian and Armijo
backtracking; one host read of five doubles per evaluation (value, gradient, the factorisation's ``info``).
"""
import math

import numpy as np
import torch

from ._args import as_device, chunk_rows, coords, on_device, require_finite, values, view_counts, view_offsets
from ._args import ops as _ops
from .predict import Prediction

f64 = torch.float64
KERNELS = ("rbf", "matern32", "matern12")
MAX_D = 4  # csrc/gpr.hip: MAXD
NOT_FINITE = "{name} has NaN or infinite entries"
ARMIJO_C = 1e-4
MAX_STEP = 2.0       # log units, per coordinate and step
VAR_CHUNK = 4096     # test rows per chunk of the predictive variance (two [N, chunk] panels)


# ------------------------------------------------------------------------------------------------------------------------
# argument checks (all of them before any device work)
# ------------------------------------------------------------------------------------------------------------------------
def _kernel(kernel, what):
    if kernel not in KERNELS:
        raise ValueError(f"{what}: kernel must be one of {KERNELS}, not {kernel!r}")
    return kernel


def _bounds(bounds, what):
    try:
        lo, hi = (float(b) for b in bounds)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: bounds must be a pair (low, high), not {bounds!r}") from None
    if not (0.0 < lo < hi < math.inf):
        raise ValueError(f"{what}: bounds must satisfy 0 < low < high < inf, not {bounds!r}")
    return math.log(lo), math.log(hi)


def _theta(theta, name, what):
    """three finite log values (log a, log l, log tau2) -> numpy [3]"""
    try:
        th = np.asarray(theta.detach().cpu() if torch.is_tensor(theta) else theta, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be three log values (log a, log l, log tau2), not {theta!r}") from None
    if th.shape != (3,) or not np.all(np.isfinite(th)):
        raise ValueError(f"{what}: {name} must be three finite log values (log a, log l, log tau2), not {theta!r}")
    return th


def gpr_bytes(N, P):
    """device bytes of one evaluation at N training rows and P outputs: K, L^-1, K^-1, the factorisation's workspace
    (``gpsa_chol_inv_blocked_workspace``) and the [N, P] panels (Y, L^-1 Y, alpha)"""
    from . import _lib

    N, P = int(N), int(P)
    return 3 * 8 * N * N + int(_lib.load().gpsa_chol_inv_blocked_workspace(N, 1)) + 3 * 8 * N * P


def _refuse_if_too_large(what, N, P, free_bytes):
    need = gpr_bytes(N, P)
    if need > free_bytes:
        raise ValueError(f"{what}: N = {N} training rows with P = {P} outputs need {need} bytes on the device (K, L^-1, "
                         f"K^-1 and the factorisation's workspace: about 40 N^2), {int(free_bytes)} are free")
    return need


def _free_bytes(dev):
    free, _ = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


# ------------------------------------------------------------------------------------------------------------------------
# the optimiser (host code; works on any ``fun(theta [3]) -> (value, gradient [3])``)
# ------------------------------------------------------------------------------------------------------------------------
def maximize(fun, theta0, free, lo, hi, max_iter=100, gtol=1e-5):
    """Projected BFGS ascent of ``fun`` over the coordinates ``free`` of theta inside the box [lo, hi].

    Dense inverse Hessian (of -fun), Armijo backtracking with c = 1e-4 from the full quasi-Newton step, no step moves a
    coordinate by more than 2 (log units).  A point where ``fun`` is not finite (the covariance did not factorise; sklearn
    returns -inf there too) is backtracked from.  Stops when the largest component of the projected gradient is <= gtol,
    or after max_iter iterations.  Returns a dict: theta, value, grad, n_iter, n_eval, converged."""
    free = np.asarray(free, dtype=np.int64)
    n = len(free)
    theta = np.array(theta0, dtype=np.float64)
    theta[free] = np.clip(theta[free], lo, hi)
    f, g = fun(theta)
    n_eval, n_iter, converged = 1, 0, False
    if not np.isfinite(f):
        raise ValueError(f"gp_regress: the covariance at the starting point theta = {theta.tolist()} does not factorise")
    g = np.asarray(g, dtype=np.float64)
    H, fresh = np.eye(n), True

    def projected(x, grad):
        pg = grad.copy()
        pg[(x <= lo) & (grad < 0)] = 0.0
        pg[(x >= hi) & (grad > 0)] = 0.0
        return pg

    while True:
        x, gx = theta[free], g[free]
        pg = projected(x, gx)
        if np.max(np.abs(pg)) <= gtol:
            converged = True
            break
        if n_iter >= max_iter:
            break
        inactive = pg != 0.0
        d = np.zeros(n)
        d[inactive] = (H[np.ix_(inactive, inactive)] @ pg[inactive])
        if not np.all(np.isfinite(d)) or d @ pg <= 0.0:
            H, fresh = np.eye(n), True
            d = pg.copy()
        m = np.max(np.abs(d))
        if m > MAX_STEP:
            d *= MAX_STEP / m
        t, accepted = 1.0, None
        for _ in range(40):
            xc = np.clip(x + t * d, lo, hi)
            s = xc - x
            if np.max(np.abs(s)) <= 1e-14 * max(1.0, np.max(np.abs(x))):
                break
            cand = theta.copy()
            cand[free] = xc
            fc, gc = fun(cand)
            n_eval += 1
            if np.isfinite(fc) and fc >= f + ARMIJO_C * (gx @ s):
                accepted = (cand, fc, np.asarray(gc, dtype=np.float64), s)
                break
            t *= 0.5
        if accepted is None:
            if fresh:
                break  # no ascent along the projected gradient itself: rounding level
            H, fresh = np.eye(n), True
            continue
        cand, fc, gc, s = accepted
        y = gx - gc[free]  # the gradient change of -fun
        sy = s @ y
        if sy > 1e-10 * np.linalg.norm(s) * np.linalg.norm(y):
            if fresh:
                H, fresh = np.eye(n) * (sy / (y @ y)), False
            rho = 1.0 / sy
            V = np.eye(n) - rho * np.outer(s, y)
            H = V @ H @ V.T + rho * np.outer(s, s)
        theta, f, g = cand, fc, gc
        n_iter += 1
    return dict(theta=theta, value=float(f), grad=g, n_iter=n_iter, n_eval=n_eval, converged=converged)


# ------------------------------------------------------------------------------------------------------------------------
# one evaluation on the device
# ------------------------------------------------------------------------------------------------------------------------
class _Evaluator:
    """K, L^-1, K^-1 and the five-double result buffer of the LML at a theta; X [N, D] and Y [N, P] fp64 on the device"""

    def __init__(self, kernel, X, Y, amplitude, jitter):
        self.kernel, self.X, self.Y, self.amplitude, self.jitter = kernel, X, Y, bool(amplitude), float(jitter)
        N, dev = int(X.shape[0]), X.device
        self.K = torch.empty(N, N, dtype=f64, device=dev)
        self.Kinv = None  # allocated by the first evaluation that asks for the gradient
        self.buf = torch.zeros(5, dtype=f64, device=dev)  # value, dLML / d(log a, log l, log tau2), info
        self.Linv = self.alpha = self.theta_dev = None
        self.at = None

    def __call__(self, theta, gradient=True):
        """-> (value, gradient [3]); -inf where the factorisation reports info != 0"""
        o = _ops()
        X, Y = self.X, self.Y
        N, P = int(Y.shape[0]), int(Y.shape[1])
        th = np.asarray(theta, dtype=np.float64)
        self.theta_dev = torch.tensor(th, dtype=f64, device=X.device)
        self.Linv = self.alpha = None  # the previous point's L^-1 goes back to the allocator before the next one is asked for
        o.gpr_cov(self.kernel, X, X, self.theta_dev, self.amplitude, same=True, jitter=self.jitter, out=self.K)
        self.Linv, logdet, info = o.chol_inv_blocked(self.K)
        B = o.gemm(self.Linv, Y)                         # L^-1 Y
        self.alpha = o.gemm(self.Linv, B, transA=True)   # L^-T L^-1 Y
        self.buf.zero_()
        if gradient:
            if self.Kinv is None:
                self.Kinv = torch.empty(N, N, dtype=f64, device=X.device)
            o.gemm(self.Linv, self.Linv, transA=True, out=self.Kinv)
            o.gpr_lml_grad(self.kernel, X, self.theta_dev, self.alpha, self.Kinv, self.amplitude, out=self.buf[1:4])
        self.buf[0] = -0.5 * (B * B).sum() - 0.5 * P * logdet[0] - 0.5 * N * P * math.log(2.0 * math.pi)
        self.buf[4] = info[0].to(f64)
        host = self.buf.cpu().numpy()  # the evaluation's one host read
        self.at = th.copy()
        grad = host[1:4].copy()
        if not self.amplitude:
            grad[0] = 0.0
        if host[4] != 0.0 or not np.isfinite(host[0]):
            return -math.inf, np.zeros(3)
        return float(host[0]), grad


class GPRegression:
    """A fitted exact GP (``gp_regress``).  ``amplitude``, ``length_scale``, ``noise_level``: a, l, tau2; ``theta``: their
    logs, numpy [3]; ``lml``, ``lml_grad`` [3] at theta (the entry of a parameter that is not fitted is 0); ``n_iter``,
    ``n_eval``, ``converged``: the optimiser's account (0, 1, True with ``optimize=False``).  Keeps X [N, D], alpha =
    K^-1 Y [N, P] and L^-1 [N, N] on the device."""

    def __init__(self, kernel, fit_amplitude, jitter, X, Y, theta, lml, lml_grad, alpha, Linv, n_iter, n_eval, converged):
        self.kernel, self.fit_amplitude, self.jitter = kernel, bool(fit_amplitude), float(jitter)
        self.X, self.Y, self.alpha, self.Linv = X, Y, alpha, Linv
        self.theta = np.array(theta, dtype=np.float64)
        self.amplitude = float(math.exp(self.theta[0])) if self.fit_amplitude else 1.0
        self.length_scale, self.noise_level = float(math.exp(self.theta[1])), float(math.exp(self.theta[2]))
        self.lml, self.lml_grad = float(lml), np.array(lml_grad, dtype=np.float64)
        self.n_iter, self.n_eval, self.converged = int(n_iter), int(n_eval), bool(converged)
        self._theta_dev = torch.tensor(self.theta, dtype=f64, device=X.device)

    def __repr__(self):
        return (f"GPRegression(kernel={self.kernel!r}, amplitude={self.amplitude:.6g}, length_scale={self.length_scale:.6g}, "
                f"noise_level={self.noise_level:.6g}, lml={self.lml:.6f}, n_iter={self.n_iter}, n_eval={self.n_eval}, "
                f"converged={self.converged})")

    @torch.no_grad()
    def log_marginal_likelihood(self, theta=None, eval_gradient=False):
        """The LML at ``theta`` (log a, log l, log tau2; default: the fitted one), with ``eval_gradient`` also its
        gradient [3] (numpy) - ``GaussianProcessRegressor.log_marginal_likelihood``.  -inf where K(theta) does not
        factorise.  The fitted state is not touched."""
        what = "GPRegression.log_marginal_likelihood"
        if theta is None:
            return (self.lml, self.lml_grad.copy()) if eval_gradient else self.lml
        th = _theta(theta, "theta", what)
        if not self.fit_amplitude:
            th[0] = 0.0
        N, P = int(self.Y.shape[0]), int(self.Y.shape[1])
        _refuse_if_too_large(what, N, P, _free_bytes(self.X.device))
        value, grad = _Evaluator(self.kernel, self.X, self.Y, self.fit_amplitude, self.jitter)(th, gradient=eval_gradient)
        return (value, grad) if eval_gradient else value

    @torch.no_grad()
    def predict(self, Xs, return_var=False, include_noise=True, rows_per_chunk=None):
        """Predictive mean [n, P] fp64 at ``Xs`` [n, D], with ``return_var`` also the variance [n] fp64 (one per row: the
        outputs share theta): ``a + [tau2] - sum_i (L^-1 a k(X, x*))_i^2``, the bracket with ``include_noise`` - sklearn's
        ``return_std`` convention with a WhiteKernel.  The mean is one fused kernel (no [n, N] matrix) and does not depend
        on ``rows_per_chunk``, bit for bit; the variance goes by chunks of rows (4096 by default) through a
        cross-covariance panel and the dense product with L^-1."""
        what = "GPRegression.predict"
        coords(Xs, "Xs", what, MAX_D, int(self.X.shape[1]), own_max_message=True)
        c = chunk_rows(rows_per_chunk, what)
        require_finite(what, NOT_FINITE, Xs=Xs)
        on_device(what, "GP regression", X_train=self.X, Xs=Xs)
        Q = as_device(Xs, f64)
        o = _ops()
        n, P = int(Q.shape[0]), int(self.alpha.shape[1])
        mean = torch.empty(n, P, dtype=f64, device=Q.device)
        step = n if c is None else c
        for a in range(0, n, step):
            o.gpr_mean(self.kernel, Q[a: a + step], self.X, self._theta_dev, self.alpha, self.fit_amplitude,
                       out=mean[a: a + step])
        if not return_var:
            return mean
        var = torch.empty(n, dtype=f64, device=Q.device)
        prior = self.amplitude + (self.noise_level if include_noise else 0.0)
        step = min(n, VAR_CHUNK) if c is None else c
        for a in range(0, n, step):
            Ks = o.gpr_cov(self.kernel, self.X, Q[a: a + step], self._theta_dev, self.fit_amplitude)  # [N, chunk]
            V = o.gemm(self.Linv, Ks)
            var[a: a + step] = prior - (V * V).sum(0)
        return mean, var


# ------------------------------------------------------------------------------------------------------------------------
# the public calls
# ------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def gp_regress(X, Y, kernel="rbf", amplitude=False, optimize=True, theta0=None, bounds=(1e-5, 1e5), max_iter=100,
               gtol=1e-5, jitter=1e-10):
    """Fit an exact GP to ``Y`` [N, P] at ``X`` [N, D <= 4]: ``GaussianProcessRegressor(kernel=[ConstantKernel() *] k +
    WhiteKernel(), alpha=jitter).fit(X, Y)`` with k = ``RBF()`` ("rbf"), ``Matern(nu=1.5)`` ("matern32") or
    ``Matern(nu=0.5)`` ("matern12"), isotropic; the P outputs share the hyper-parameters.

    amplitude: fit the constant factor a too (sklearn's ``ConstantKernel() * k``); otherwise a = 1.
    optimize:  maximise the log marginal likelihood over the log parameters from ``theta0`` (log a, log l, log tau2;
               default 0: sklearn's start) inside ``bounds`` = (low, high) for each parameter (default sklearn's 1e-5 ..
               1e5) by the projected BFGS ascent of ``maximize``; False: factorise at theta0 and stop.
    Returns a ``GPRegression``.  Raises ValueError for a bad shape, D > 4, NaN or infinite entries, tensors on the CPU, an
    unknown kernel, or a size whose matrices do not fit the device's free memory (the message states the bytes needed)."""
    what = "gp_regress"
    coords(X, "X", what, MAX_D, own_max_message=True)
    N = int(X.shape[0])
    values(Y, "Y", what, N)
    _kernel(kernel, what)
    lo, hi = _bounds(bounds, what)
    th0 = np.zeros(3) if theta0 is None else _theta(theta0, "theta0", what)
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 0:
        raise ValueError(f"{what}: max_iter must be a non-negative integer, not {max_iter!r}")
    if not (float(gtol) > 0.0):
        raise ValueError(f"{what}: gtol must be > 0, not {gtol!r}")
    if not (float(jitter) >= 0.0) or not math.isfinite(float(jitter)):
        raise ValueError(f"{what}: jitter must be >= 0 and finite, not {jitter!r}")
    require_finite(what, NOT_FINITE, X=X, Y=Y)
    on_device(what, "GP regression", X=X, Y=Y)
    _refuse_if_too_large(what, N, int(Y.shape[1]), _free_bytes(X.device))  # before the fit's first allocation
    Xd, Yd = as_device(X, f64), as_device(Y, f64)

    amplitude = bool(amplitude)
    if not amplitude:
        th0[0] = 0.0
    ev = _Evaluator(kernel, Xd, Yd, amplitude, jitter)
    if optimize:
        free = [0, 1, 2] if amplitude else [1, 2]
        res = maximize(ev, th0, free, lo, hi, max_iter=int(max_iter), gtol=float(gtol))
        theta, n_eval = res["theta"], res["n_eval"]
        if ev.at is None or not np.array_equal(ev.at, theta):  # the last point tried was a rejected one
            res["value"], res["grad"] = ev(theta)
            n_eval += 1
        out = (theta, res["value"], res["grad"], ev.alpha, ev.Linv, res["n_iter"], n_eval, res["converged"])
    else:
        value, grad = ev(th0)
        if not math.isfinite(value):
            raise ValueError(f"{what}: the covariance at theta0 = {th0.tolist()} does not factorise")
        out = (th0, value, grad, ev.alpha, ev.Linv, 0, 1, True)
    return GPRegression(kernel, amplitude, jitter, Xd, Yd, *out)


def _view_rows(n_samples_list, total, name, what):
    try:
        ns, ok = view_counts(n_samples_list, total, least_rows=0)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a list of row counts, not {n_samples_list!r}") from None
    if not ok:
        raise ValueError(f"{what}: {name} = {ns} does not partition the {total} rows")
    off = view_offsets(ns)
    return list(zip(off, off[1:]))


def _mse(pred, Y):
    """the reference's error: mean over rows of the sum over outputs of the squared error"""
    return float((pred - Y).square().sum(1).mean())


@torch.no_grad()
def prediction_baselines(X_train, Y_train, X_test, Y_test, n_samples_list_train, n_samples_list_test, kernel="rbf",
                         amplitude=False):
    """The reference's two GP baselines (two_dimensional_prediction.py:126-155): the "union" GP fitted to all training
    rows at their unaligned coordinates, and a "separate" GP per view, each scored on the test rows by the mean over rows
    of the summed squared error.  Views are consecutive row ranges (``n_samples_list_*``, as the model's data dict has
    them); a view without test rows is skipped, as the reference does (:145).

    Returns a ``Prediction``: ``error_union``, ``error_separate`` (floats), ``preds_union`` [n_test, P] and
    ``preds_separate`` [rows of the views that were not skipped, P] fp64, ``fit_union`` and ``fits_separate`` (a list with
    one ``GPRegression`` per view, None for a skipped one), ``views`` (the views scored)."""
    what = "prediction_baselines"
    coords(X_train, "X_train", what, MAX_D, own_max_message=True)
    D = int(X_train.shape[1])
    values(Y_train, "Y_train", what, int(X_train.shape[0]))
    coords(X_test, "X_test", what, MAX_D, D, own_max_message=True)
    values(Y_test, "Y_test", what, int(X_test.shape[0]))
    if Y_test.shape[1] != Y_train.shape[1]:
        raise ValueError(f"{what}: Y_test has shape {tuple(Y_test.shape)} and Y_train {tuple(Y_train.shape)}: the same P "
                         "is needed")
    _kernel(kernel, what)
    tr = _view_rows(n_samples_list_train, int(X_train.shape[0]), "n_samples_list_train", what)
    te = _view_rows(n_samples_list_test, int(X_test.shape[0]), "n_samples_list_test", what)
    if len(tr) != len(te):
        raise ValueError(f"{what}: {len(tr)} training views and {len(te)} test views")
    for v, ((a, b), (c, d)) in enumerate(zip(tr, te)):
        if d > c and b == a:
            raise ValueError(f"{what}: view {v} has test rows and no training rows")
    if all(d == c for c, d in te):
        raise ValueError(f"{what}: no view has test rows")
    require_finite(what, NOT_FINITE, X_train=X_train, Y_train=Y_train, X_test=X_test, Y_test=Y_test)
    on_device(what, "GP regression", X_train=X_train, Y_train=Y_train, X_test=X_test, Y_test=Y_test)
    Xtr, Ytr, Xte, Yte = (as_device(t, f64) for t in (X_train, Y_train, X_test, Y_test))

    fit_union = gp_regress(Xtr, Ytr, kernel=kernel, amplitude=amplitude)
    preds_union = fit_union.predict(Xte)
    fits, preds, truth, views = [], [], [], []
    for v, ((a, b), (c, d)) in enumerate(zip(tr, te)):
        if d == c:
            fits.append(None)
            continue
        fit = gp_regress(Xtr[a:b], Ytr[a:b], kernel=kernel, amplitude=amplitude)
        fits.append(fit)
        preds.append(fit.predict(Xte[c:d]))
        truth.append(Yte[c:d])
        views.append(v)
    preds_separate = torch.cat(preds, 0)
    return Prediction(error_union=_mse(preds_union, Yte), error_separate=_mse(preds_separate, torch.cat(truth, 0)),
                      preds_union=preds_union, preds_separate=preds_separate, fit_union=fit_union, fits_separate=fits,
                      views=views)
