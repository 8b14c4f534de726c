"""Writes tests/golden/reference_pca.npz: sklearn's own results on the seeded inputs of tests/pca_util.py, the record that
tests/test_pca.py holds the numpy yardstick against (the GPU box needs only the npz).

    python tests/golden/make_pca_golden.py

Per variant of pca_util.VARIANTS: each view goes through sklearn.preprocessing.StandardScaler (with_std = the variant's
``scale``; a constant column comes out 0), the views are stacked and decomposed with
sklearn.decomposition.PCA(n_components=k, svd_solver="full").  sklearn >= 1.5 is needed for the sign rule (written with
1.7.2).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pca_util as pu  # noqa: E402


def main():
    import sklearn
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler

    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in pu.VARIANTS:
        Y, ns, center, scale, k = pu.variant(name)
        Yd = np.asarray(Y, dtype=np.float64)
        if center == "pooled":
            ns = [Yd.shape[0]]
        off = pu.offsets(ns)
        Z = np.concatenate([StandardScaler(with_mean=True, with_std=scale).fit_transform(Yd[a:b])
                            for a, b in zip(off, off[1:])])
        p = PCA(n_components=k, svd_solver="full").fit(Z)
        out[f"{name}/components"] = p.components_
        out[f"{name}/explained_variance"] = p.explained_variance_
        out[f"{name}/explained_variance_ratio"] = p.explained_variance_ratio_
        out[f"{name}/singular_values"] = p.singular_values_
    path = os.path.join(HERE, "reference_pca.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
