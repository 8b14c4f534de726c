"""Time exact GP regression (spatial_alignment_amd/gpr.py) against the same mathematics in fp64 torch on the same device.

N training points uniform in [0, 10]^2, P outputs (smooth functions of the point plus noise), the rbf kernel with a noise
term (``RBF() + WhiteKernel()``), three stages:
  eval:     one log marginal likelihood with its gradient at theta = (0, 0.3, -1)
  fit:      a whole ``gp_regress`` from sklearn's start (theta = 0)
  predict:  the predictive mean at --test rows (10 000) from the fitted model
Route B (this package): gpsa_gpr_cov_f64 + gpsa_chol_inv_blocked_f64 + gpsa_gemm + gpsa_gpr_lml_grad_f64 / gpsa_gpr_mean_f64.
Route A (torch): torch.cdist, linalg.cholesky, cholesky_solve, autograd for the gradient; its fit runs the package's own
host optimiser (``gpr.maximize``) on that evaluation, so both fits take the same kind of steps; its predict is one
cdist panel times alpha.

One process, device events around synchronised work, every leg warmed up first, the legs alternating in blocks (median and
min-max over the blocks are reported); peak memory per leg from torch's allocator statistics (the package's scratch lives
in a torch tensor and is counted).  If sklearn is importable its CPU time for the eval and predict stages (and, with
--sklearn-fit-max N, the fit at sizes up to N) is added as context, with the thread count it ran on.

  python tools/gpr_timing.py                  # N = 2000 and N = 5000, P = 50
Appends one JSON line per N to --out (default profiles/gpr_timing.jsonl).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_alignment_amd import engine as E  # noqa: E402
from spatial_alignment_amd import gpr  # noqa: E402

f64 = torch.float64
JITTER = 1e-10
LO, HI = math.log(1e-5), math.log(1e5)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2**20


def torch_eval(X, Y, theta):
    """(LML, gradient [3]) of the rbf + noise model (a = 1) in fp64 torch with autograd"""
    N, P = Y.shape
    th = torch.tensor(theta, dtype=f64, device=X.device, requires_grad=True)
    with torch.enable_grad():
        ell, tau2 = th[1].exp(), th[2].exp()
        K = torch.exp(-0.5 * torch.cdist(X, X).square() / (ell * ell))
        K = K + (tau2 + JITTER) * torch.eye(N, dtype=f64, device=X.device)
        L, info = torch.linalg.cholesky_ex(K)
        alpha = torch.cholesky_solve(Y, L)
        lml = -0.5 * (Y * alpha).sum() - P * L.diagonal().log().sum() - 0.5 * N * P * math.log(2.0 * math.pi)
        lml.backward()
    out = torch.cat([lml.detach().reshape(1), th.grad, info.to(f64).reshape(1)]).cpu().numpy()
    if out[4] != 0 or not np.isfinite(out[0]):
        return -math.inf, np.zeros(3)
    g = out[1:4].copy()
    g[0] = 0.0
    return float(out[0]), g


def torch_fit(X, Y):
    res = gpr.maximize(lambda th: torch_eval(X, Y, th), np.zeros(3), [1, 2], LO, HI)
    N = Y.shape[0]
    ell, tau2 = math.exp(res["theta"][1]), math.exp(res["theta"][2])
    K = torch.exp(-0.5 * torch.cdist(X, X).square() / (ell * ell)) + (tau2 + JITTER) * torch.eye(N, dtype=f64, device=X.device)
    res["alpha"] = torch.cholesky_solve(Y, torch.linalg.cholesky(K))
    return res


def torch_predict(Xs, X, alpha, ell):
    return torch.exp(-0.5 * torch.cdist(Xs, X).square() / (ell * ell)) @ alpha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000, 5000])
    ap.add_argument("--p", type=int, default=50)
    ap.add_argument("--test", type=int, default=10000)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per block of the eval and predict legs (the fits: 1)")
    ap.add_argument("--sklearn-fit-max", type=int, default=0, help="also time sklearn's fit for N up to this (CPU, slow)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "gpr_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    for N in args.n:
        gen = torch.Generator().manual_seed(N)
        Xh = torch.rand(N, 2, generator=gen, dtype=f64) * 10
        W, phase = torch.randn(2, args.p, generator=gen, dtype=f64) * 0.8, torch.rand(args.p, generator=gen, dtype=f64) * 6.28
        Yh = torch.sin(Xh @ W + phase) + 0.3 * torch.randn(N, args.p, generator=gen, dtype=f64)
        Xsh = torch.rand(args.test, 2, generator=gen, dtype=f64) * 10
        X, Y, Xs = Xh.to(dev), Yh.to(dev), Xsh.to(dev)
        theta = np.array([0.0, 0.3, -1.0])

        ev = gpr._Evaluator("rbf", X, Y, False, JITTER)
        fit = gpr.gp_regress(X, Y)
        v_pkg, g_pkg = ev(theta)
        del ev
        agree = dict(fit_lml_package=fit.lml, fit_theta_package=fit.theta.tolist(), fit_evals_package=fit.n_eval)
        legs = {"eval": lambda: gpr._Evaluator("rbf", X, Y, False, JITTER)(theta), "fit": lambda: gpr.gp_regress(X, Y),
                "predict": lambda: fit.predict(Xs)}
        torch_failed = None
        try:
            v_t, g_t = torch_eval(X, Y, theta)
            tfit = torch_fit(X, Y)
            alpha_t, ell_t = tfit["alpha"], math.exp(tfit["theta"][1])
            agree.update(eval_lml_rel_diff=abs(v_pkg - v_t) / abs(v_t),
                         eval_grad_max_abs_diff=float(np.max(np.abs(g_pkg - g_t))), fit_lml_torch=tfit["value"],
                         fit_theta_torch=tfit["theta"].tolist(), fit_evals_torch=tfit["n_eval"])
            legs["torch_eval"] = lambda: torch_eval(X, Y, theta)
            legs["torch_fit"] = lambda: torch_fit(X, Y)
        except RuntimeError as e:  # the torch route itself gave up at this size: recorded, its two legs are left out
            torch_failed = str(e).splitlines()[0][:300]
            torch.cuda.synchronize()
            alpha_t, ell_t = fit.alpha, fit.length_scale
        legs["torch_predict"] = lambda: torch_predict(Xs, X, alpha_t, ell_t)
        agree["predict_max_abs_diff"] = float((fit.predict(Xs) - legs["torch_predict"]()).abs().max())
        peaks = {k: peak_mb(fn) for k, fn in legs.items()}  # also the warm-up of every leg
        times = {k: [] for k in legs}
        for _ in range(args.blocks):
            for k, fn in legs.items():
                times[k].append(timed(fn, 1 if "fit" in k else args.calls))
        ms = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}
        line = dict(tool="gpr_timing", N=N, P=args.p, D=2, kernel="rbf", test_rows=args.test, blocks=args.blocks,
                    calls=args.calls, device=torch.cuda.get_device_name(0), ms=ms,
                    speedup_over_torch={k: ms["torch_" + k]["median"] / ms[k]["median"] for k in ("eval", "fit", "predict")
                                        if "torch_" + k in ms},
                    peak_mb={k: round(v, 1) for k, v in peaks.items()}, agree=agree, gpr_bytes_mb=round(gpr.gpr_bytes(N, args.p) / 2**20, 1),
                    package_scratch_mb=round(sum(b.numel() for b in E.ops()._scratch.values() if b is not None) / 2**20, 1))
        if torch_failed:
            line["torch_eval_failed"] = torch_failed
        try:
            from sklearn.gaussian_process import GaussianProcessRegressor
            from sklearn.gaussian_process.kernels import RBF, WhiteKernel

            Xn, Yn, Xsn = Xh.numpy(), Yh.numpy(), Xsh.numpy()
            k = RBF(math.exp(theta[1])) + WhiteKernel(math.exp(theta[2]))
            gp = GaussianProcessRegressor(k, alpha=JITTER, optimizer=None).fit(Xn, Yn)
            t0 = time.perf_counter()
            v_sk, _ = gp.log_marginal_likelihood(gp.kernel_.theta, eval_gradient=True)
            t1 = time.perf_counter()
            gp.predict(Xsn)
            t2 = time.perf_counter()
            sk = {"eval": 1e3 * (t1 - t0), "predict": 1e3 * (t2 - t1), "threads": os.environ.get("OMP_NUM_THREADS"),
                  "eval_lml_rel_diff_to_package": abs(v_sk - v_pkg) / abs(v_sk)}
            if N <= args.sklearn_fit_max:
                t0 = time.perf_counter()
                gpf = GaussianProcessRegressor(RBF() + WhiteKernel(), alpha=JITTER).fit(Xn, Yn)
                sk["fit"] = 1e3 * (time.perf_counter() - t0)
                sk["fit_lml"] = float(gpf.log_marginal_likelihood_value_)
            line["sklearn_cpu_ms"] = sk
        except ImportError:
            pass
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del legs, fit, alpha_t, X, Y, Xs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
