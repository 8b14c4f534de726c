"""The yardstick of the highly-variable-gene tests: the per-view column moments of csrc/moments.hip and scanpy's
Seurat-flavoured dispersion ranking (``highly_variable_genes(flavor="seurat")``), written out plainly in fp64 numpy, no
pandas.  The binning and the per-bin statistics are held against pandas' own ``cut`` / ``groupby`` by
tests/golden/reference_hvg.npz (tests/test_hvg.py).  scanpy itself is not part of any check."""
import numpy as np

import counts_util as cu

F64 = np.float64
MODES = ("identity", "expm1", "normalize")
DEFAULTS = dict(min_mean=0.0125, max_mean=3, min_disp=0.5, max_disp=np.inf, n_bins=20)


def offsets(ns):
    return np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)


def scale_of(row_sum, target=None):
    """target / row sum per row (0 for a row without counts); target: the median of the positive row sums"""
    rs = np.asarray(row_sum, F64)
    target = cu.median_target(rs) if target is None else float(target)
    return np.where(rs > 0, target / np.where(rs > 0, rs, 1.0), 0.0)


def values(Y, mode, scale=None):
    """t per element, fp64, from the matrix as stored (the caller passes what fp32 holds)"""
    Y = np.asarray(Y, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == "identity":
            return Y
        if mode == "expm1":
            return np.expm1(Y)
        return Y * np.asarray(scale, F64)[:, None]


def sums(Y, ns, mode, scale=None, keep=None, stored=None):
    """-> dict(s1, s2, abs1 [V, P], term2 [V, P]: the sum of t^2's magnitudes = s2, n_nonfinite).  ``keep``: rows that
    count; ``stored``: the positions a CSR matrix stores (None: all) - the others contribute nothing, not even to
    n_nonfinite"""
    t = values(Y, mode, scale)
    on = np.ones(t.shape, bool) if stored is None else np.asarray(stored, bool).copy()
    if keep is not None:
        on &= np.asarray(keep, bool)[:, None]
    bad = on & ~np.isfinite(t)
    t = np.where(on, t, 0.0)
    off = offsets(ns)
    with np.errstate(over="ignore", invalid="ignore"):
        s1 = np.stack([t[a:b].sum(0) for a, b in zip(off[:-1], off[1:])])
        s2 = np.stack([(t[a:b] ** 2).sum(0) for a, b in zip(off[:-1], off[1:])])
        ab = np.stack([np.abs(t[a:b]).sum(0) for a, b in zip(off[:-1], off[1:])])
    return dict(s1=s1, s2=s2, abs1=ab, n_nonfinite=int(bad.sum()))


def close(s1, s2, n):
    """mean and scanpy's variance: (mean of squares - mean^2) n / (n - 1)"""
    n = np.asarray(n, F64).reshape(-1, 1)
    mean = s1 / n
    return mean, (s2 / n - mean * mean) * (n / (n - 1.0))


def cut(x, n_bins):
    """``pandas.cut(x, bins=n_bins)`` (right-closed): -> (bin of every x in [0, n_bins), edges [n_bins + 1])"""
    x = np.asarray(x, F64)
    mn, mx = x.min(), x.max()
    if mn == mx:
        mn -= 0.001 * abs(mn) if mn != 0 else 0.001
        mx += 0.001 * abs(mx) if mx != 0 else 0.001
        edges = np.linspace(mn, mx, n_bins + 1)
    else:
        edges = np.linspace(mn, mx, n_bins + 1)
        edges[0] -= (mx - mn) * 0.001
    return np.clip(np.searchsorted(edges, x, side="left") - 1, 0, n_bins - 1), edges


def seurat(mean, var, n_bins=20, mask=None):
    """one view: -> dict(means, dispersions, dispersions_norm, bin (-1 outside the mask), edges, bin_mean, bin_std)"""
    mean, var = np.array(mean, F64), np.asarray(var, F64)
    P = mean.size
    mask = np.ones(P, bool) if mask is None else np.asarray(mask, bool)
    mean[mean == 0] = 1e-12
    with np.errstate(invalid="ignore", divide="ignore"):
        disp = var / mean
        disp[disp == 0] = np.nan
        disp = np.log(disp)
    means = np.log1p(mean)
    idx = np.full(P, -1, np.int64)
    idx[mask], edges = cut(means[mask], n_bins)
    bmean, bstd = np.full(n_bins, np.nan), np.full(n_bins, np.nan)
    for b in range(n_bins):
        d = disp[(idx == b) & ~np.isnan(disp)]
        if d.size >= 1:
            bmean[b] = d.mean()
        if d.size >= 2:
            bstd[b] = np.sqrt(((d - d.mean()) ** 2).sum() / (d.size - 1))
    one = np.isnan(bstd)
    bstd[one] = bmean[one]
    bmean[one] = 0.0
    dnorm = np.full(P, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        dnorm[mask] = (disp[mask] - bmean[idx[mask]]) / bstd[idx[mask]]
    return dict(means=means, dispersions=disp, dispersions_norm=dnorm, bin=idx, edges=edges, bin_mean=bmean, bin_std=bstd)


def select(means, dnorm, mask=None, n_top_genes=None, min_mean=0.0125, max_mean=3, min_disp=0.5, max_disp=np.inf):
    """-> highly_variable [P] bool"""
    mask = np.ones(means.size, bool) if mask is None else np.asarray(mask, bool)
    if n_top_genes is None:
        dn = np.where(np.isnan(dnorm), 0.0, dnorm)
        return mask & (means > min_mean) & (means < max_mean) & (dn > min_disp) & (dn < max_disp)
    d = np.sort(dnorm[mask & ~np.isnan(dnorm)])[::-1]
    cutoff = d[min(n_top_genes, d.size) - 1]
    return mask & (np.nan_to_num(dnorm) >= cutoff)


def decisive(r, mask, n_top_genes, n_bins):
    """the two conditions under which the selection is decided by the values alone: no gene's ``means`` within 1e-9 of
    the range of an interior bin edge; the normalised dispersions just above and just below the cutoff more than 1e-6
    apart (exact ties excepted; without ``n_top_genes``: every value more than that from the default bound it is
    compared with).  -> (distance to the nearest interior edge / range, gap at the cutoff)"""
    mask = np.ones(r["means"].size, bool) if mask is None else np.asarray(mask, bool)
    x, edges = r["means"][mask], r["edges"]
    span = (x.max() - x.min()) or 1.0
    near = np.abs(x[:, None] - edges[None, 1:-1]).min() / span if n_bins > 1 else np.inf
    gap = np.inf
    if n_top_genes is None:  # the default bounds: the distance of any value to the bound it is compared with
        dn = np.where(np.isnan(r["dispersions_norm"][mask]), 0.0, r["dispersions_norm"][mask])
        gap = min(np.abs(dn - DEFAULTS["min_disp"]).min(), np.abs(x - DEFAULTS["min_mean"]).min(),
                  np.abs(x - DEFAULTS["max_mean"]).min())
    else:
        d = np.sort(r["dispersions_norm"][mask & ~np.isnan(r["dispersions_norm"])])[::-1]
        cutoff = d[min(n_top_genes, d.size) - 1]
        below = d[d < cutoff]
        above = d[d > cutoff]
        gap = min(cutoff - below.max() if below.size else np.inf, above.min() - cutoff if above.size else np.inf)
    return float(near), float(gap)


def hvg(Y, ns, mode="expm1", scale=None, mask=None, combine="intersection", n_top_genes=None, n_bins=20, **bounds):
    """``highly_variable_genes`` view by view -> dict of [V, P] arrays, ``genes``, ``views`` (the per-view dicts)"""
    s = sums(Y, ns, mode, scale)
    mean, var = close(s["s1"], s["s2"], ns)
    views = [seurat(mean[v], var[v], n_bins, mask) for v in range(len(ns))]
    hv = np.stack([select(r["means"], r["dispersions_norm"], mask, n_top_genes, **bounds) for r in views])
    genes = np.nonzero(hv.all(0) if combine == "intersection" else hv.any(0))[0]
    out = {k: np.stack([r[k] for r in views]) for k in ("means", "dispersions", "dispersions_norm")}
    return dict(out, highly_variable=hv, genes=genes, views=views, n_nonfinite=s["n_nonfinite"], mean=mean, var=var)


def prepare_seurat(Y, ns, min_counts=None, max_counts=None, min_cells=None, n_top_genes=None, transform="pearson",
                   theta=100.0, standardize=True):
    """the pipeline of counts.prepare_counts(selection="seurat"), step by step"""
    Y = np.asarray(Y, F64)
    rs = Y.sum(1)
    keep = np.ones(len(Y), bool)
    if min_counts is not None:
        keep &= rs >= min_counts
    if max_counts is not None:
        keep &= rs <= max_counts
    rows = np.nonzero(keep)[0]
    off = offsets(ns)
    ns_kept = [int(keep[a:b].sum()) for a, b in zip(off[:-1], off[1:])]
    Yr = Y[rows]
    passed = None if min_cells is None else (Yr > 0).sum(0) >= min_cells
    log_sz = cu.log_size_factors(Yr.sum(1))
    s = sums(Yr, [len(rows)], "normalize", scale_of(Yr.sum(1)))
    mean, var = close(s["s1"], s["s2"], [len(rows)])
    r = seurat(mean[0], var[0], DEFAULTS["n_bins"], passed)
    genes = np.nonzero(select(r["means"], r["dispersions_norm"], passed, n_top_genes))[0]
    Ys = Yr[:, genes]
    log_offset, nconst = None, None
    if transform == "counts":
        out, log_offset = Ys, log_sz
    elif transform == "log1p":
        out = cu.normalize_log1p(Ys, None, row_sum=Yr.sum(1))
    elif transform == "pearson":
        out = cu.pearson_residuals(Ys, theta, True)
    else:
        out = cu.deviance_residuals(Ys, theta)[0]
    if transform != "counts" and standardize:
        out, nconst = cu.standardize_views(out.astype(np.float32).astype(F64), ns_kept)
    return dict(outputs=out, log_offset=log_offset, rows=rows, genes=genes, n_samples_list=ns_kept, n_constant=nconst,
                dispersions_norm=r["dispersions_norm"], seurat=r, passed=passed)
