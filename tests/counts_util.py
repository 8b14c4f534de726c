"""The yardstick of the count-preprocessing tests: the formulas of spatial_alignment_amd/counts.py written out plainly in
fp64 numpy, the seeded count recipe the tests share, and the pipeline of ``prepare_counts`` step by step.  Held against
the reference's own functions by tests/golden/reference_counts.npz (tests/test_counts.py)."""
import math

import numpy as np

F64 = np.float64
# the C library's log, element by element: what the reference's deviance residuals go through (scipy's xlogy); numpy's
# vectorised log differs from it in the last bit on a few entries in a thousand, and the fixture is held to ==
_libm_log = np.vectorize(math.log, otypes=[F64])


def recipe(N, P, seed=0, depth=0.0, zero_column=True):
    """negative binomial counts (size 3) with mean exp(0.6 z_i + 1 + depth) exp(1.2 z_g - 0.5) exp(0.7 z_ig [u_g < 0.4]),
    one column forced to zero (P >= 3) -> [N, P] fp64 holding integers"""
    rng = np.random.default_rng(seed)
    zi, zg = rng.standard_normal(N), rng.standard_normal(P)
    zig, ug = rng.standard_normal((N, P)), rng.random(P)
    mean = np.exp(0.6 * zi + 1.0 + depth)[:, None] * np.exp(1.2 * zg - 0.5)[None, :] * np.exp(0.7 * zig * (ug < 0.4)[None, :])
    Y = rng.poisson(mean * rng.gamma(3.0, 1.0 / 3.0, size=(N, P))).astype(F64)
    if zero_column and P >= 3:
        Y[:, P // 2] = 0.0
    return Y


def margins(Y):
    Y = np.asarray(Y, F64)
    bad = ~np.isfinite(Y) | (Y < 0)
    with np.errstate(invalid="ignore"):
        return dict(row_sum=Y.sum(1), col_sum=Y.sum(0), row_nnz=(Y > 0).sum(1).astype(np.int64),
                    col_nnz=(Y > 0).sum(0).astype(np.int64), n_invalid=int(bad.sum()), total=float(Y.sum()))


def log_size_factors(row_sum):
    lrs = np.log(np.asarray(row_sum, F64))
    return lrs - lrs.mean()


def size_factors(Y):
    return np.exp(log_size_factors(np.asarray(Y, F64).sum(1)))


def poisson_deviance(Y, log_sz=None):
    """-> dict(deviance, ll_sat, abs_sat, ll_null) per column; a column without counts: 0"""
    Y = np.asarray(Y, F64)
    log_sz = log_size_factors(Y.sum(1)) if log_sz is None else np.asarray(log_sz, F64)
    sz = np.exp(log_sz)
    pos = Y > 0
    ylogy = np.where(pos, Y * np.log(np.where(pos, Y, 1.0)), 0.0)
    ylsz = Y * log_sz[:, None]
    sat = np.where(pos, Y * np.log(np.where(pos, Y, 1.0) / sz[:, None]), 0.0).sum(0)
    cs = Y.sum(0)
    some = cs > 0
    null = np.where(some, cs * np.log(np.where(some, cs, 1.0) / sz.sum()), 0.0)
    return dict(deviance=np.where(some, 2.0 * (sat - null), 0.0), ll_sat=sat, ll_null=null,
                abs_sat=(np.abs(ylogy) + np.abs(ylsz)).sum(0))


def order(dev, mask=None, n_top=None):
    """descending, equal values by the lower index"""
    o = np.argsort(-np.asarray(dev, F64), kind="stable")
    if mask is not None:
        o = o[mask[o]]
    return o if n_top is None else o[:n_top]


def smallest_relative_gap(dev):
    d = np.sort(np.asarray(dev, F64))[::-1]
    d = d[d > 0]
    return float(((d[:-1] - d[1:]) / d[:-1]).min()) if d.size > 1 else np.inf


def _mu(Y):
    return Y.sum(1, keepdims=True) @ Y.sum(0, keepdims=True) / Y.sum()


def pearson_residuals(Y, theta=100.0, clipping=True):
    Y = np.asarray(Y, F64)
    mu = _mu(Y)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (Y - mu) / np.sqrt(mu + mu**2 / theta)
    z = np.where(mu > 0, z, 0.0)
    if clipping:
        z = np.clip(z, -np.sqrt(Y.shape[0]), np.sqrt(Y.shape[0]))
    return z


def deviance_residuals(Y, theta):
    Y = np.asarray(Y, F64)
    mu = _mu(Y)
    pos = Y > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        xl = np.where(pos, Y * _libm_log(np.where(pos & (mu > 0), Y / np.where(mu > 0, mu, 1.0), 1.0)), 0.0)
        if np.isinf(theta):
            t = 2.0 * (xl - (Y - mu))
        else:
            t = 2.0 * (xl - (Y + theta) * np.log((Y + theta) / (mu + theta)))
        z = np.sign(Y - mu) * np.sqrt(np.maximum(t, 0.0))
    return np.where(mu > 0, z, 0.0), np.where(mu > 0, t, np.inf)


def median_target(row_sum):
    return float(np.median(row_sum[row_sum > 0]))


def normalize_log1p(Y, target_sum=None, row_sum=None):
    Y = np.asarray(Y, F64)
    rs = Y.sum(1) if row_sum is None else np.asarray(row_sum, F64)
    target = median_target(rs) if target_sum is None else float(target_sum)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.log1p(Y * target / rs[:, None])
    return np.where(rs[:, None] > 0, out, 0.0)


def standardize_views(Y, ns):
    """-> (out, n_constant): population std (numpy.std); a column constant within a view -> 0, counted"""
    Y = np.asarray(Y, F64)
    out, nconst, a = np.empty_like(Y), [], 0
    for n in ns:
        blk = Y[a: a + n]
        mean, std = blk.mean(0), blk.std(0)
        const = (blk == blk[:1]).all(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            z = (blk - mean) / std
        out[a: a + n] = np.where(const[None, :], 0.0, z)
        nconst.append(int(const.sum()))
        a += n
    return out, np.asarray(nconst, np.int64)


def prepare(Y, ns, min_counts=None, max_counts=None, min_cells=None, n_top_genes=None, transform="pearson", theta=100.0,
            standardize=True):
    """the pipeline of counts.prepare_counts, step by step"""
    Y = np.asarray(Y, F64)
    rs = Y.sum(1)
    keep = np.ones(len(Y), bool)
    if min_counts is not None:
        keep &= rs >= min_counts
    if max_counts is not None:
        keep &= rs <= max_counts
    rows = np.nonzero(keep)[0]
    off = np.concatenate([[0], np.cumsum(ns)])
    ns_kept = [int(keep[a:b].sum()) for a, b in zip(off[:-1], off[1:])]
    Yr = Y[rows]
    passed = None if min_cells is None else (Yr > 0).sum(0) >= min_cells
    log_sz = log_size_factors(Yr.sum(1))
    dev = poisson_deviance(Yr, log_sz)["deviance"]
    genes = np.sort(order(dev, passed, n_top_genes))
    Ys = Yr[:, genes]
    log_offset, nconst = None, None
    if transform == "counts":
        out, log_offset = Ys, log_sz
    elif transform == "log1p":
        out = normalize_log1p(Ys, None, row_sum=Yr.sum(1))
    elif transform == "pearson":
        out = pearson_residuals(Ys, theta, True)
    else:
        out = deviance_residuals(Ys, theta)[0]
    if transform != "counts" and standardize:
        out, nconst = standardize_views(out.astype(np.float32).astype(F64), ns_kept)
    return dict(outputs=out, log_offset=log_offset, rows=rows, genes=genes, n_samples_list=ns_kept, deviance=dev,
                n_constant=nconst)
