"""Writes tests/golden/reference_gpr.npz: what sklearn's GaussianProcessRegressor gives on a few seeded jittered lattices,
for every (data set, kernel, amplitude) - the fixture of tests/test_gpr.py and tests/test_gpr_gpu.py.

    python tests/golden/make_gpr_golden.py          (CPU, needs scikit-learn; run once, the result is committed)

Per data set: X [N <= 400, D], Y [N, P], Xs [40, D].  Per case ``<data>/<kernel>/<amp|noamp>``: sklearn's optimum
``theta_hat`` (log a, log l, log tau2; log a = 0 without the amplitude) and ``lml_hat``, the LML and its gradient at
``theta1`` = theta0 + 0.3, the predictive mean and standard deviation at ``Xs`` from the fitted model, and ``bound``: 1 where
the optimum sits on a bound of the search box (1e-5 .. 1e5 per parameter).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpr_util as U  # noqa: E402

# name: (n_side, D, P, true length scale, noise variance, seed); the first three are the sets the optimiser was
# prototyped on
DATA = {
    "lat17": (17, 2, 4, 1.5, 0.1, 3),
    "lat20": (20, 2, 8, 0.8, 0.5, 7),
    "lat15": (15, 2, 1, 3.0, 0.01, 5),
    "line60": (60, 1, 2, 1.0, 0.05, 11),
    "cube6": (6, 3, 3, 2.5, 0.2, 13),
}
BOUNDS = (1e-5, 1e5)


def sk_kernel(kind, amplitude):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel

    k = RBF(1.0, BOUNDS) if kind == "rbf" else Matern(1.0, BOUNDS, nu=1.5 if kind == "matern32" else 0.5)
    if amplitude:
        k = ConstantKernel(1.0, BOUNDS) * k
    return k + WhiteKernel(1.0, BOUNDS)


def theta3(theta, amplitude):
    return np.asarray(theta, np.float64) if amplitude else np.concatenate([[0.0], theta])


def main():
    from sklearn.gaussian_process import GaussianProcessRegressor

    out, keys = {}, []
    lo, hi = np.log(BOUNDS[0]), np.log(BOUNDS[1])
    for name, (n_side, D, P, ell, noise, seed) in DATA.items():
        X, Y, Xs = U.lattice(n_side, D, P, ell, noise, seed)
        assert X.shape[0] <= 400
        out[f"{name}/X"], out[f"{name}/Y"], out[f"{name}/Xs"] = X, Y, Xs
        for kind in U.KERNELS:
            for amplitude in (False, True):
                key = f"{name}/{kind}/{'amp' if amplitude else 'noamp'}"
                gp = GaussianProcessRegressor(sk_kernel(kind, amplitude), alpha=1e-10, normalize_y=False).fit(X, Y)
                th = np.asarray(gp.kernel_.theta)
                n = len(th)
                v1, g1 = gp.log_marginal_likelihood(np.full(n, 0.3), eval_gradient=True)
                mean, std = gp.predict(Xs, return_std=True)
                std = std if std.ndim == 1 else std[:, 0]
                out[f"{key}/theta_hat"] = theta3(th, amplitude)
                out[f"{key}/lml_hat"] = np.float64(gp.log_marginal_likelihood(th))
                out[f"{key}/theta1"] = theta3(np.full(n, 0.3), amplitude)
                out[f"{key}/lml1"] = np.float64(v1)
                out[f"{key}/grad1"] = theta3(g1, amplitude)
                out[f"{key}/mean"] = mean.reshape(Xs.shape[0], P)
                out[f"{key}/std"] = std
                bound = bool(np.any(th < lo + 1e-3) or np.any(th > hi - 1e-3))
                out[f"{key}/bound"] = np.int64(bound)
                keys.append(key)
                print(key, "theta_hat", np.round(th, 4), "lml", float(out[f"{key}/lml_hat"]), "BOUND" if bound else "")
    out["keys"] = np.array(keys)
    np.savez_compressed(U.GOLDEN, **out)
    print("wrote", U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
