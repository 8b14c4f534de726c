"""The yardstick for the neighbour statistics (spatial_alignment_amd/neighbors.py, csrc/neighbors.hip), all numpy fp64 on
the host and never fed from the code under test: brute-force distances in difference form, the neighbours by np.lexsort
on (index, d2), the weighted NaN-skipping average, R^2 and Pearson's r per column, and Moran's I from the DENSE weight
matrix (S0 / S1 / S2 summed from W itself, not from the closed forms the package uses).  Shared by tests/test_neighbors.py
(CPU, where it is itself held against sklearn) and tests/test_neighbors_gpu.py."""
import math

import numpy as np


def dist2(Q, R):
    """[nq, nr] squared distances, sum_d (q_d - r_d)^2 accumulated over d in order"""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    s = np.zeros((Q.shape[0], R.shape[0]))
    for d in range(Q.shape[1]):
        u = Q[:, d, None] - R[None, :, d]
        s += u * u
    return s


def knn(Q, R, k, exclude_self=False, extra=0):
    """-> (idx [nq, k + extra] int64, d2 [nq, k + extra]): per row the smallest keys (d2, index), ascending;
    exclude_self leaves reference i out for query i.  ``extra`` further neighbours for the caller's gap checks (fewer
    where the references run out: then as many as there are)"""
    D2 = dist2(Q, R)
    nq, nr = D2.shape
    take = min(k + extra, nr - (1 if exclude_self else 0))
    idx = np.empty((nq, take), np.int64)
    for i in range(nq):
        order = np.lexsort((np.arange(nr), D2[i]))  # last key is primary: by d2, then by index
        if exclude_self:
            order = order[order != i]
        idx[i] = order[:take]
    return idx, np.take_along_axis(D2, idx, 1)


def rows_with_clear_order(d2_ext, k, rel=1e-12):
    """rows whose consecutive distances among the first k + 1 (fewer where there are no more) differ by more than
    ``rel`` relative: their neighbour order cannot turn on how a product was rounded"""
    d = d2_ext[:, : k + 1]
    gap = np.diff(d, axis=1)
    return np.all(gap > rel * np.maximum(d[:, 1:], 1e-300), axis=1) if d.shape[1] > 1 else np.ones(len(d), bool)


def average(idx, d2, Y, weights="uniform"):
    """[nq, P] fp64: sum_j w_ij Y[idx_ij, p] / sum_j w_ij over the neighbours whose Y entry is not NaN (0 / 0 = NaN).
    "distance": w = 1 / sqrt(d2), and in a row with a zero distance w = 1 there and 0 elsewhere (sklearn's rule)"""
    Y = np.asarray(Y, np.float64)
    idx = np.asarray(idx)
    nq, k = idx.shape
    if weights == "uniform":
        w = np.ones((nq, k))
    else:
        d2 = np.asarray(d2, np.float64)
        zero = d2 == 0.0
        with np.errstate(divide="ignore"):
            w = np.where(zero.any(1, keepdims=True), zero.astype(np.float64), 1.0 / np.sqrt(d2))
    num, den = np.zeros((nq, Y.shape[1])), np.zeros((nq, Y.shape[1]))
    for j in range(k):
        y = Y[idx[:, j]]
        ok = ~np.isnan(y)
        num += np.where(ok, w[:, j, None] * y, 0.0)
        den += np.where(ok, w[:, j, None], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, np.nan)


def regress(X_train, Y_train, X_test, k, weights="uniform", exclude_self=False):
    idx, d2 = knn(X_test, X_train, k, exclude_self)
    return average(idx, d2, Y_train, weights)


def _used(Y, pred):
    Y, pred = np.asarray(Y, np.float64), np.asarray(pred, np.float64)
    return Y, pred, ~(np.isnan(Y) | np.isnan(pred))


def r2(Y, pred):
    """per column: 1 - SS_res / SS_tot around the mean of the rows used (neither side NaN); SS_tot == 0: NaN"""
    Y, pred, use = _used(Y, pred)
    out = np.full(Y.shape[1], np.nan)
    for p in range(Y.shape[1]):
        y, f = Y[use[:, p], p], pred[use[:, p], p]
        if y.size:
            tot = float(((y - y.mean()) ** 2).sum())
            if tot > 0:
                out[p] = 1.0 - float(((y - f) ** 2).sum()) / tot
    return out


def pearson(Y, pred):
    Y, pred, use = _used(Y, pred)
    out = np.full(Y.shape[1], np.nan)
    for p in range(Y.shape[1]):
        y, f = Y[use[:, p], p], pred[use[:, p], p]
        if y.size:
            yc, fc = y - y.mean(), f - f.mean()
            den = math.sqrt(float((yc * yc).sum()) * float((fc * fc).sum()))
            if den > 0:
                out[p] = float((yc * fc).sum()) / den
    return out


def dense_weights(X, k, row_standardize=True):
    """W [n, n]: w_ij = 1 where j is among i's k nearest other points (ties to the lower index), / k when standardised"""
    n = len(X)
    idx, _ = knn(X, X, k, exclude_self=True)
    W = np.zeros((n, n))
    W[np.arange(n)[:, None], idx] = 1.0 / k if row_standardize else 1.0
    return W


def moran(X, Y, k, row_standardize=True):
    """-> dict of I, expected, variance, z, p_norm ([P] each) from the dense W; a constant column is NaN"""
    Y = np.asarray(Y, np.float64)
    n, P = Y.shape
    W = dense_weights(X, k, row_standardize)
    S0 = W.sum()
    S1 = 0.5 * ((W + W.T) ** 2).sum()
    S2 = ((W.sum(1) + W.sum(0)) ** 2).sum()
    EI = -1.0 / (n - 1)
    var = (n * n * S1 - n * S2 + 3.0 * S0 * S0) / ((n * n - 1.0) * S0 * S0) - EI * EI
    I = np.full(P, np.nan)
    for p in range(P):
        if Y[:, p].max() == Y[:, p].min():
            continue
        z = Y[:, p] - Y[:, p].mean()
        I[p] = (n / S0) * float(z @ (W @ z)) / float(z @ z)
    zs = (I - EI) / math.sqrt(var)
    pn = np.array([0.5 * math.erfc(v / math.sqrt(2.0)) if v == v else np.nan for v in zs])
    return dict(I=I, expected=np.full(P, EI), variance=np.full(P, var), z=zs, p_norm=pn, S0=S0, S1=S1, S2=S2)


def lattice(nx=13, ny=11, h=0.5):
    """nx x ny lattice with spacing h (exact in fp64): every point has ties across the 6th place"""
    gx, gy = np.meshgrid(np.arange(nx) * h, np.arange(ny) * h, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], 1)
