"""Host-side helpers that user training scripts import next to the model (the reference exports them
from gpsa/__init__.py:3-10).  Small, dependency-free re-implementations; the count-data preprocessing
(``compute_size_factors`` ... ``pearson_residuals``, gpsa/util/util.py:155-254) keeps the reference's names, orientations
and return types here and runs on the device through ``spatial_alignment_amd.counts``; the plotting callbacks of the
reference are outside the hot path's scope.
"""
import numpy as np


def rbf_kernel_numpy(x, xp, kernel_params):
    """numpy RBF of the data simulators; ``kernel_params = [log variance, log lengthscale(s)...]``"""
    scale = 1.0 / np.exp(np.asarray(kernel_params[1:]))
    a, b = x * scale, xp * scale
    sq = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
    return np.exp(kernel_params[0]) * np.exp(-0.5 * np.maximum(sq, 0.0))


def polar_warp(X, r, theta):
    """displace 2-D points by the polar offsets (r, theta)"""
    out = np.array(X[:, :2], dtype=float, copy=True)
    out[:, 0] += r * np.cos(theta)
    out[:, 1] += r * np.sin(theta)
    return out


def get_st_coordinates(df):
    """spot names of the form 'AxB' (index of an ST data frame) -> float array [[A, B], ...]"""
    return np.asarray([tuple(map(float, str(label).split("x"))) for label in df.index])


def compute_distance(X1, X2):
    """mean Euclidean distance between matched rows"""
    return float(np.linalg.norm(np.asarray(X1) - np.asarray(X2), axis=1).mean())


class ConvergenceChecker:
    """Fits a cubic to the last ``span`` loss values (least squares through an orthonormal basis) and
    reports the relative change between the last two fitted values."""

    def __init__(self, span, dtp="float64"):
        self.span = span
        t = np.arange(span, dtype=dtp) - (span - 1) / 2.0
        self.U, _, _ = np.linalg.svd(np.vander(t, 4, increasing=True), full_matrices=False)

    def smooth(self, y):
        return self.U @ (self.U.T @ y)

    def subset(self, y, idx=-1):
        first = idx - self.span + 1
        return y[first:] if idx == -1 else y[first : idx + 1]

    def relative_change(self, y, idx=-1, smooth=True):
        window = self.subset(y, idx=idx)
        fitted = self.smooth(window) if smooth else window
        return (fitted[-1] - fitted[-2]) / (0.1 + abs(fitted[-2]))

    def converged(self, y, tol=1e-4, **kwargs):
        return abs(self.relative_change(y, **kwargs)) < tol

    def relative_change_all(self, y, smooth=True):
        changes = np.full(len(y), np.nan)
        for i in range(self.span, len(y)):
            changes[i] = self.relative_change(y, idx=i, smooth=smooth)
        return changes

    def converged_all(self, y, tol=1e-4, smooth=True):
        return np.abs(self.relative_change_all(y, smooth=smooth)) < tol


class LossNotDecreasingChecker:
    """``check_loss(i, trace)`` turns True once the mean per-step decrease of the loss over the last
    ``window_size - 1`` steps drops below ``atol``."""

    def __init__(self, max_epochs, atol=1e-2, window_size=10):
        self.max_epochs, self.atol, self.window_size = max_epochs, atol, window_size
        self.decrease_in_loss = np.zeros(max_epochs)
        self.average_decrease_in_loss = np.zeros(max_epochs)

    def check_loss(self, iternum, loss_trace):
        if iternum < 1:
            return False
        self.decrease_in_loss[iternum] = loss_trace[iternum - 1] - loss_trace[iternum]
        if iternum < self.window_size:
            return False
        recent = self.decrease_in_loss[iternum - self.window_size + 1 : iternum]
        self.average_decrease_in_loss[iternum] = recent.mean()
        return bool(self.average_decrease_in_loss[iternum] < self.atol)


# ------------------------------------------------------------------------------------------------------------------------
# count preprocessing under the reference's names (gpsa/util/util.py:155-254): thin wrappers that move the matrix to the
# device, call spatial_alignment_amd.counts and return numpy.  pandas is duck-typed (``.values`` / ``.index``), never imported.
# ------------------------------------------------------------------------------------------------------------------------
class _Labelled:
    """what a call returns for a plain array where the reference, given a data frame, returns a pandas Series"""

    def __init__(self, values, index):
        self.values, self.index = values, index


def _count_device(device):
    import torch

    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _to_device(a, device, transpose=False):
    import torch

    a = np.asarray(getattr(a, "values", a))
    if a.ndim != 2:
        raise ValueError(f"a 2-D matrix of counts is needed, not an array of shape {a.shape}")
    a = np.ascontiguousarray(a.T if transpose else a, dtype=np.float32)
    return torch.from_numpy(a).to(_count_device(device))


def _like_series(m, values):
    """per-gene values labelled as the rows of ``m`` are: a Series of m's own pandas when m is a data frame"""
    if hasattr(m, "iloc") and hasattr(m, "index"):
        s = m.iloc[:, 0].astype("float64").copy()
        s.name = None
        s[:] = values
        return s
    return _Labelled(values, np.arange(len(values)))


def compute_size_factors(m, device=None):
    """size factors with geometric mean 1 for a genes x cells matrix ``m`` (``.values`` or an array): numpy [cells]"""
    from .. import counts

    return counts.size_factors(_to_device(m, device, transpose=True)).cpu().numpy()


def poisson_deviance(X, sz, device=None):
    """Poisson deviance per gene of a genes x cells matrix ``X`` given the cells' size factors ``sz``: labelled like
    X's rows (``.values`` / ``.index``)"""
    import torch

    from .. import counts

    Y = _to_device(X, device, transpose=True)
    log_sz = torch.log(torch.as_tensor(np.asarray(sz, dtype=np.float64), device=Y.device))
    return _like_series(X, counts.poisson_deviance(Y, log_sz).cpu().numpy())


def deviance_feature_selection(X, device=None):
    """(deviances, gene names) of the genes of a genes x cells matrix ``X`` that have counts, in X's row order"""
    from .. import counts

    Y = _to_device(X, device, transpose=True)
    some = (Y.sum(0) > 0).cpu().numpy()
    dev = counts.poisson_deviance(Y).cpu().numpy()
    names = np.asarray(X.index.values) if hasattr(X, "index") else np.arange(Y.shape[1])
    return dev[some], names[some]


def deviance_residuals(x, theta, mu=None, device=None):
    """deviance residuals of a spots x genes array for a negative binomial (``theta=np.inf``: Poisson) null with the
    margins' ``mu``: numpy [spots, genes] (fp32 values).  A ``mu`` of the caller's is not supported."""
    from .. import counts

    if mu is not None:
        raise ValueError("deviance_residuals: only mu=None (the product of the margins) is supported")
    return counts.deviance_residuals(_to_device(x, device), float(theta)).cpu().numpy().astype(np.float64)


def pearson_residuals(counts, theta, clipping=True, device=None):
    """analytic Pearson residuals of a spots x genes array, clipped to +-sqrt(spots): numpy [spots, genes] (fp32 values)"""
    from .. import counts as _counts

    return _counts.pearson_residuals(_to_device(counts, device), float(theta), clipping).cpu().numpy().astype(np.float64)
