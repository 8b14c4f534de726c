"""Generate tests/golden/reference_hvg.npz: the bins and the per-bin statistics of scanpy's Seurat-flavoured gene
ranking as PANDAS computes them (build machine only; the GPU box reads the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hvg_golden.py

scanpy's ``highly_variable_genes(flavor="seurat")`` bins the genes with ``pandas.cut(means, bins=n_bins)`` and normalises
the dispersions with ``groupby(...).mean()`` / ``.std(ddof=1)``; tests/hvg_util.py restates both in plain numpy, and this
script records what pandas itself returns on seeded inputs, so that the restatement is held to the real thing.  scanpy is
not installed here and is not run.  Per case the file holds the inputs (``mean``, ``var`` [P] fp64 of the normalised
counts, ``mask`` [P] bool, ``n_bins``, ``n_top``: -1 for the default bounds) and pandas' results (``bin`` [P] int64, -1
outside the mask; ``dispersions_norm`` [P]; ``highly_variable`` [P] bool).  Arrays only.  (The name does not start with
"c": tests/golden_io.py takes every c*.npz in this directory for a model case.)

The cases: "base" (counts_util.recipe, 200 x 300, its all-zero gene included, one gene with a single non-zero entry),
"outlier" (one gene far above the rest: a bin with exactly one gene and empty bins below it), "ties" (two identical genes
and a cutoff that falls on them), "masked" (a gene_mask), "bounds" (no n_top: scanpy's default bounds), "flat" (every gene
the same mean: pandas' zero-range rule), "tiny" (P = 3, more bins than genes)."""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import counts_util as cu  # noqa: E402
import hvg_util as hu  # noqa: E402


def moments_of(Y):
    """mean / var [P] of the normalised counts, from the fp32 log1p matrix as scanpy sees it (expm1 in fp64)"""
    X = cu.normalize_log1p(Y).astype(np.float32)
    s = hu.sums(X, [len(X)], "expm1")
    mean, var = hu.close(s["s1"], s["s2"], [len(X)])
    return mean[0], var[0]


def pandas_seurat(mean, var, mask, n_bins, n_top):
    mean = np.array(mean, np.float64)
    mean[mean == 0] = 1e-12
    with np.errstate(invalid="ignore", divide="ignore"):
        disp = var / mean
        disp[disp == 0] = np.nan
        disp = np.log(disp)
    means = np.log1p(mean)
    df = pd.DataFrame({"means": means[mask], "dispersions": disp[mask]})
    df["mean_bin"] = pd.cut(df["means"], bins=n_bins)
    grouped = df.groupby("mean_bin", observed=False)["dispersions"]
    bin_mean, bin_std = grouped.mean(), grouped.std(ddof=1)
    one = bin_std.isnull().to_numpy()
    bin_std[one] = bin_mean[one].to_numpy()
    bin_mean[one] = 0
    codes = df["mean_bin"].cat.codes.to_numpy().astype(np.int64)
    assert (codes >= 0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = (df["dispersions"].to_numpy() - bin_mean.to_numpy()[codes]) / bin_std.to_numpy()[codes]
    P = mean.size
    bins, dnorm = np.full(P, -1, np.int64), np.full(P, np.nan)
    bins[mask], dnorm[mask] = codes, dn
    if n_top < 0:
        d0 = np.where(np.isnan(dn), 0.0, dn)
        sub = (df["means"].to_numpy() > 0.0125) & (df["means"].to_numpy() < 3) & (d0 > 0.5) & (d0 < np.inf)
    else:
        d = np.sort(dn[~np.isnan(dn)])[::-1]
        sub = np.nan_to_num(dn) >= d[min(n_top, d.size) - 1]
    hv = np.zeros(P, bool)
    hv[mask] = sub
    return bins, dnorm, hv


def cases():
    Y = cu.recipe(200, 300, seed=21, depth=0.0)
    Y[:, 7] = 0.0
    Y[11, 7] = 3.0  # a gene with a single non-zero entry
    mean, var = moments_of(Y)
    every = np.ones(300, bool)
    yield "base", mean, var, every, 20, 40
    Yo = Y.copy()
    Yo[:, 5] = Yo[:, 5] * 0 + np.random.default_rng(1).poisson(4000.0, 200)  # far above every other gene
    m2, v2 = moments_of(Yo)
    yield "outlier", m2, v2, every, 20, 40
    Yt = Y.copy()
    Yt[:, 31] = Yt[:, 30]
    m3, v3 = moments_of(Yt)
    r = hu.seurat(m3, v3, 20)
    assert r["dispersions_norm"][30] == r["dispersions_norm"][31]
    rank = int((r["dispersions_norm"] > r["dispersions_norm"][30]).sum())  # genes ahead of the pair
    yield "ties", m3, v3, every, 20, rank + 1
    mask = (Y > 0).sum(0) >= 100
    assert 100 < mask.sum() < 280
    yield "masked", mean, var, mask, 20, 30
    yield "bounds", mean, var, every, 20, -1
    rng = np.random.default_rng(2)
    yield "flat", np.full(6, 2.5), rng.uniform(1.0, 9.0, 6), np.ones(6, bool), 5, 2
    yield "tiny", np.array([0.5, 3.0, 0.0]), np.array([1.0, 2.0, 0.0]), np.ones(3, bool), 20, 2


def main():
    out = {}
    for name, mean, var, mask, n_bins, n_top in cases():
        bins, dnorm, hv = pandas_seurat(mean, var, mask, n_bins, n_top)
        for key, v in (("mean", mean), ("var", var), ("mask", mask), ("n_bins", np.int64(n_bins)), ("n_top", np.int64(n_top)),
                       ("bin", bins), ("dispersions_norm", dnorm), ("highly_variable", hv)):
            out[f"{name}/{key}"] = np.asarray(v)
        sizes = np.bincount(bins[mask], minlength=n_bins)
        print(f"{name}: P {mean.size}, masked in {int(mask.sum())}, bins of one gene {int((sizes == 1).sum())}, empty bins "
              f"{int((sizes == 0).sum())}, NaN dispersions_norm {int(np.isnan(dnorm[mask]).sum())}, selected {int(hv.sum())}")
    path = os.path.join(HERE, "reference_hvg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
