"""Generate tests/golden/reference_counts.npz by RUNNING THE REFERENCE's count preprocessing (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_counts_golden.py

Loads the unmodified /root/reference/gpsa/util/util.py by file path (the package import needs the absent plotting
dependency), runs ``compute_size_factors``, ``deviance_feature_selection`` (which runs ``poisson_deviance``),
``pearson_residuals`` (theta 100 and 1) and ``deviance_residuals`` (theta 100 and inf) on the seeded counts of
tests/counts_util.recipe, and stores the inputs (int16) and the results - arrays only, no reference source travels.  The
residuals of the largest case are kept for every 32nd row, which keeps the file below 300 KB.  The GPU box never runs this
script: the tests read the committed file.  (The name does not start with "c": tests/golden_io.py takes every c*.npz in
this directory for a model case.)
"""
import importlib.util
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import counts_util as cu  # noqa: E402

CASES = {"a": (33, 65, 11, 1), "b": (97, 45, 12, 1), "c": (257, 130, 13, 32)}  # N, P, seed, row stride of the residuals


def main():
    spec = importlib.util.spec_from_file_location("reference_util", "/root/reference/gpsa/util/util.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, (N, P, seed, stride) in CASES.items():
        Y = cu.recipe(N, P, seed=seed, depth=0.5)
        assert Y.max() < 2**15 and (Y.sum(1) > 0).all() and (Y.sum(0) == 0).sum() == 1
        frame = pd.DataFrame(Y.T, index=[f"g{g}" for g in range(P)])  # genes x cells, as the reference takes it
        out[f"{name}/counts"] = Y.astype(np.int16)
        out[f"{name}/stride"] = np.int64(stride)
        out[f"{name}/size_factors"] = np.asarray(ref.compute_size_factors(frame), np.float64)
        devs, names = ref.deviance_feature_selection(frame)
        out[f"{name}/deviance"] = np.asarray(devs, np.float64)
        out[f"{name}/deviance_genes"] = np.asarray([int(str(g)[1:]) for g in names], np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            for theta in (100.0, 1.0):
                out[f"{name}/pearson_{theta:g}"] = np.asarray(ref.pearson_residuals(Y.copy(), theta), np.float64)[::stride]
            for theta in (100.0, np.inf):
                out[f"{name}/deviance_residuals_{theta:g}"] = np.asarray(ref.deviance_residuals(Y.copy(), theta),
                                                                         np.float64)[::stride]
    path = os.path.join(HERE, "reference_counts.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
