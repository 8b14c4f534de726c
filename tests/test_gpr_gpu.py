"""Exact GP regression on the device: the three entries of csrc/gpr.hip through the C ABI (ops.py) and through
``torch.ops.gpsa.*``, and ``gp_regress`` / ``GPRegression`` / ``prediction_baselines`` of spatial_alignment_amd/gpr.py,
against the numpy fp64 yardstick of tests/gpr_util.py (itself held against sklearn and the fixture in tests/test_gpr.py).

Bars (derived, none fitted; every comparison prints what it measures):
* kernel contracts - alpha and Kinv come from the yardstick, so conditioning does not enter and only fp64 rounding is left:
  - covariance: max |err| <= 1e-14 max(1, a) (one exp, one or two products: a few ulp of values <= a); exactly symmetric;
    the diagonal is EQUAL to (a + tau2) + jitter at theta = 0, where exp is exact on host and device alike, and at a general
    theta all diagonal entries are one value within the bar (the device's exp(theta) may differ from the host's by an ulp);
  - gradient reduction: each output <= 1e-12 of its 1/2 sum |W_ij dK_ij| (N^2 <= 7e4 terms, eps sqrt(N^2) ~ 6e-14);
    a repeated call gives the same bits;
  - mean: <= 1e-12 of sum_j |a k_j alpha_j|; ``rows_per_chunk`` in {7, 64, None} gives the same bits;
* the whole call at a fixed theta - 1e-8 for the LML (relative), the gradient (of its scale), the mean (of its scale) and
  the variance (of a + tau2): cond(K) <= 1 + a N / tau2 <= 1e6 for every case used (asserted in tests/test_gpr.py), so the
  expected error is cond * eps ~ 1e-10; the bar is the project's whole-call fp64 bar (tests/test_warp_gpu.py);
* the optimiser - converged, n_eval <= 60, inside the bounds, LML >= sklearn's - 1e-6 max(1, |LML|); on the cases that end at
  a bound: finite, inside the bounds, LML >= sklearn's - 1e-4.
The factorisation (gpsa_chol_inv_blocked_f64) is run here at N = 60 .. 400, on both sides of its 256-column block.
"""
import functools

import numpy as np
import pytest
import torch

import gpr_util as U
import spatial_alignment_amd as pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = torch.float64
LO, HI = np.log(1e-5), np.log(1e5)
CASES = U.cases()
INTERIOR = [c for c in CASES if not c.bound]
BOUND = [c for c in CASES if c.bound]
WHOLE = INTERIOR + U.block_edge_cases()
SIZES = (1, 15, 16, 17, 63, 64, 65, 130)
THETA = np.array([0.7, 0.2, -0.5])  # a = 2.01, l = 1.22, tau2 = 0.61


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=f64, device=DEV).contiguous()


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _points(n, D, seed=0):
    """n points in [0, 10]^D, the second a copy of the first (d = 0 off the diagonal)"""
    X = np.random.RandomState(1000 * D + n + seed).uniform(0.0, 10.0, (n, D))
    if n >= 2:
        X[1] = X[0]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _problem(kind, N, P, D):
    """the yardstick's alpha, Kinv and L at THETA for N random points and P random outputs (computed once, shared)"""
    X = _points(N, D, seed=7)
    Y = np.random.RandomState(N * 53 + P).normal(size=(N, P))
    r = U.lml(kind, X, Y, THETA, True, full=True)
    return X, Y, r


# ------------------------------------------------------------------------------------------------------------------------
# kernel contracts
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", U.KERNELS)
def test_covariance(kind, D):
    o, worst = _ops(), 0.0
    th = _dev(THETA)
    for amplitude in (False, True):
        a, _, tau2 = U.params(THETA, amplitude)
        bar = 1e-14 * max(1.0, a)
        for n in SIZES:
            X = _points(n, D)
            Xd = _dev(X)
            K = _np(o.gpr_cov(kind, Xd, Xd, th, amplitude, same=True, jitter=1e-10))
            ref = U.cov(kind, X, X, THETA, amplitude, same=True, jitter=1e-10)
            err = np.max(np.abs(K - ref))
            worst = max(worst, err / bar)
            assert np.all(np.isfinite(K)) and err <= bar, (n, amplitude, err)
            assert np.array_equal(K, K.T), (n, amplitude)
            assert np.all(np.diag(K) == K[0, 0]), (n, amplitude)
            if n >= 2:  # the duplicated point: k(0) = 1 exactly in every form
                assert K[0, 1] == K[1, 0] and abs(K[0, 1] - a) <= bar
        for na in SIZES:
            for nb in SIZES:
                XA, XB = _points(na, D), _points(nb, D, seed=3)
                K = _np(o.gpr_cov(kind, _dev(XA), _dev(XB), th, amplitude))
                err = np.max(np.abs(K - U.cov(kind, XA, XB, THETA, amplitude)))
                worst = max(worst, err / bar)
                assert K.shape == (na, nb) and err <= bar, (na, nb, amplitude, err)
    # theta = 0: a = tau2 = 1 exactly on both sides
    for amplitude in (False, True):
        for n in SIZES:
            Xd = _dev(_points(n, D))
            K = _np(o.gpr_cov(kind, Xd, Xd, _dev(np.zeros(3)), amplitude, same=True, jitter=1e-10))
            assert np.all(np.diag(K) == 1.0 + 1.0 + 1e-10), n
    print(f"covariance {kind} D = {D}: largest error / bar = {worst:.3f}")


def test_derivative_at_a_duplicated_point_is_zero_not_nan():
    """d = 0 off the diagonal in both Matern forms: the gradient reduction stays finite and equals the yardstick's"""
    o = _ops()
    for kind in U.KERNELS:
        X, Y, r = _problem(kind, 17, 3, 2)
        assert np.array_equal(X[0], X[1])
        g = _np(o.gpr_lml_grad(kind, _dev(X), _dev(THETA), _dev(r["alpha"]), _dev(r["Kinv"]), True))
        ref, scale = U.grad_from(kind, X, THETA, True, r["alpha"], r["Kinv"])
        assert np.all(np.isfinite(g)) and np.all(np.abs(g - ref) <= 1e-12 * scale), (kind, g, ref)


@pytest.mark.parametrize("kind", U.KERNELS)
def test_gradient_reduction(kind):
    o, worst = _ops(), 0.0
    th = _dev(THETA)
    for N in (1, 2, 15, 16, 17, 64, 65, 257):
        for P in (1, 3, 4, 5, 50):
            D = 1 + (N + P) % 4
            X, _, r = _problem(kind, N, P, D)
            Xd, al, Ki = _dev(X), _dev(r["alpha"]), _dev(r["Kinv"])
            for amplitude in (True, False):
                # (alpha and Kinv are the amplitude model's in both calls: the entry is a reduction over what it is given)
                g = _np(o.gpr_lml_grad(kind, Xd, th, al, Ki, amplitude))
                again = _np(o.gpr_lml_grad(kind, Xd, th, al, Ki, amplitude))
                ref, scale = U.grad_from(kind, X, THETA, amplitude, r["alpha"], r["Kinv"])
                err = np.abs(g - ref)  # (a scale is 0 where every pair is at d = 0: N = 1, N = 2 with the duplicate)
                worst = max(worst, np.max(err[scale > 0] / scale[scale > 0], initial=0.0))
                assert np.all(err <= 1e-12 * scale), (N, P, amplitude, g, ref, scale)
                assert g.tobytes() == again.tobytes(), (N, P, amplitude)
    print(f"gradient reduction {kind}: largest error / scale = {worst:.2e} (bar 1e-12)")


@pytest.mark.parametrize("kind", U.KERNELS)
def test_mean(kind):
    o, worst = _ops(), 0.0
    th = _dev(THETA)
    for N in (1, 17, 65, 300):
        for P in (1, 3, 50):
            D = 1 + (N + P) % 4
            X, _, r = _problem(kind, N, P, D)
            Xd, al = _dev(X), _dev(r["alpha"])
            for ns in (1, 17, 130):
                Xs = _points(ns, D, seed=11)
                for amplitude in (True, False):
                    m = _np(o.gpr_mean(kind, _dev(Xs), Xd, th, al, amplitude))
                    ref, scale = U.mean(kind, Xs, X, THETA, amplitude, r["alpha"])
                    e = np.max(np.abs(m - ref) / scale)
                    worst = max(worst, e)
                    assert m.shape == (ns, P) and e <= 1e-12, (N, P, ns, amplitude, e)
    print(f"mean {kind}: largest error / scale = {worst:.2e} (bar 1e-12)")


@pytest.mark.parametrize("kind", U.KERNELS)
def test_mean_does_not_depend_on_the_chunking(kind):
    X, Y, _ = _problem(kind, 300, 50, 2)
    fit = pkg.gp_regress(_dev(X), _dev(Y), kernel=kind, amplitude=True, optimize=False, theta0=THETA)
    Xs = _dev(_points(130, 2, seed=11))
    whole = _np(fit.predict(Xs))
    for c in (7, 64):
        assert _np(fit.predict(Xs, rows_per_chunk=c)).tobytes() == whole.tobytes(), c
    mv, vv = fit.predict(Xs, return_var=True, rows_per_chunk=64)
    assert _np(mv).tobytes() == whole.tobytes() and vv.shape == (130,)


def test_dispatcher_ops_equal_the_ops_forms():
    from spatial_alignment_amd import torch_ops  # noqa: F401

    o = _ops()
    for kind in U.KERNELS:
        X, _, r = _problem(kind, 65, 5, 3)
        Xd, th, al, Ki = _dev(X), _dev(THETA), _dev(r["alpha"]), _dev(r["Kinv"])
        Xs = _dev(_points(17, 3, seed=11))
        pairs = [
            (torch.ops.gpsa.gpr_cov(Xd, Xd, th, kind, True, True, 1e-10), o.gpr_cov(kind, Xd, Xd, th, True, True, 1e-10)),
            (torch.ops.gpsa.gpr_cov(Xs, Xd, th, kind), o.gpr_cov(kind, Xs, Xd, th)),
            (torch.ops.gpsa.gpr_lml_grad(Xd, th, al, Ki, kind, True), o.gpr_lml_grad(kind, Xd, th, al, Ki, True)),
            (torch.ops.gpsa.gpr_mean(Xs, Xd, th, al, kind, True), o.gpr_mean(kind, Xs, Xd, th, al, True)),
        ]
        for a, b in pairs:
            assert a.dtype == f64 and _np(a).tobytes() == _np(b).tobytes(), kind


# ------------------------------------------------------------------------------------------------------------------------
# the whole call at a fixed theta
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", WHOLE, ids=repr)
def test_whole_call_at_fixed_theta(c):
    Xd, Yd, Xsd = _dev(c.X), _dev(c.Y), _dev(c.Xs)
    for name, th in (("theta0 + 0.3", c.theta1), ("sklearn's optimum", c.theta_hat)):
        assert U.cond_bound(c.X.shape[0], th, c.amplitude) <= 1e6
        fit = pkg.gp_regress(Xd, Yd, kernel=c.kernel, amplitude=c.amplitude, optimize=False, theta0=th)
        r = U.lml(c.kernel, c.X, c.Y, th, c.amplitude, full=True)
        a, ell, tau2 = U.params(th, c.amplitude)
        assert (fit.n_iter, fit.n_eval, fit.converged) == (0, 1, True)
        assert (fit.amplitude, fit.length_scale, fit.noise_level) == pytest.approx((a, ell, tau2), rel=1e-14)
        e_v = abs(fit.lml - r["value"]) / abs(r["value"])
        e_g = np.abs(fit.lml_grad - r["grad"]) / r["grad_scale"]
        if not c.amplitude:
            assert fit.lml_grad[0] == 0.0
            e_g[0] = 0.0
        mean, var = fit.predict(Xsd, return_var=True)
        m, ms = U.mean(c.kernel, c.Xs, c.X, th, c.amplitude, r["alpha"])
        e_m = np.max(np.abs(_np(mean) - m) / ms)
        e_s = np.max(np.abs(_np(var) - U.variance(c.kernel, c.Xs, c.X, th, c.amplitude, r["L"]))) / (a + tau2)
        _, latent = fit.predict(Xsd, return_var=True, include_noise=False)
        e_l = np.max(np.abs(_np(latent) - U.variance(c.kernel, c.Xs, c.X, th, c.amplitude, r["L"], False))) / (a + tau2)
        print(f"{c.key} at {name}: lml {e_v:.1e} grad {np.max(e_g):.1e} mean {e_m:.1e} var {e_s:.1e} / {e_l:.1e} (bar 1e-8)")
        assert e_v <= 1e-8 and np.max(e_g) <= 1e-8 and e_m <= 1e-8 and e_s <= 1e-8 and e_l <= 1e-8
        assert np.max(np.abs(_np(fit.alpha) - r["alpha"])) <= 1e-8 * np.max(np.abs(r["alpha"]))
    # the method at another theta: the same evaluation, and the fitted state stays what it was
    v, g = fit.log_marginal_likelihood(c.theta1, eval_gradient=True)
    first = pkg.gp_regress(Xd, Yd, kernel=c.kernel, amplitude=c.amplitude, optimize=False, theta0=c.theta1)
    assert v == first.lml and g.tobytes() == first.lml_grad.tobytes()
    assert fit.log_marginal_likelihood() == fit.lml and np.array_equal(fit.theta, np.where([c.amplitude, True, True],
                                                                                           c.theta_hat, 0.0))


# ------------------------------------------------------------------------------------------------------------------------
# the optimiser
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", INTERIOR, ids=repr)
def test_optimiser(c):
    fit = pkg.gp_regress(_dev(c.X), _dev(c.Y), kernel=c.kernel, amplitude=c.amplitude)
    print(f"{c.key}: n_iter {fit.n_iter} n_eval {fit.n_eval} LML - sklearn's {fit.lml - c.lml_hat:+.2e} theta {fit.theta} "
          f"(sklearn {c.theta_hat})")
    assert fit.converged and fit.n_eval <= 60
    free = [0, 1, 2] if c.amplitude else [1, 2]
    assert np.all(fit.theta[free] >= LO) and np.all(fit.theta[free] <= HI)
    assert fit.lml >= c.lml_hat - 1e-6 * max(1.0, abs(c.lml_hat))
    assert np.max(np.abs(fit.lml_grad)) <= 1e-5


@pytest.mark.parametrize("c", BOUND, ids=repr)
def test_optimiser_at_a_bound(c):
    fit = pkg.gp_regress(_dev(c.X), _dev(c.Y), kernel=c.kernel, amplitude=c.amplitude)
    print(f"{c.key}: n_iter {fit.n_iter} n_eval {fit.n_eval} converged {fit.converged} LML - sklearn's "
          f"{fit.lml - c.lml_hat:+.2e} theta {fit.theta} (sklearn {c.theta_hat})")
    free = [0, 1, 2] if c.amplitude else [1, 2]
    assert np.isfinite(fit.lml) and np.all(np.isfinite(fit.theta)) and bool(torch.isfinite(fit.alpha).all())
    assert np.all(fit.theta[free] >= LO) and np.all(fit.theta[free] <= HI)
    assert fit.lml >= c.lml_hat - 1e-4


# ------------------------------------------------------------------------------------------------------------------------
# memory, baselines
# ------------------------------------------------------------------------------------------------------------------------
def test_predict_holds_no_panel():
    """N = 256, 20 000 test rows, P = 2: a materialised [ns, N] panel alone would be 41 MB"""
    X, Y, _ = _problem("rbf", 256, 2, 2)
    fit = pkg.gp_regress(_dev(X), _dev(Y), optimize=False, theta0=THETA)
    Xs = torch.rand(20000, 2, device=DEV, dtype=torch.float32) * 10.0
    fit.predict(Xs[:64])  # (nothing lazy left to allocate inside the measured call)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mean = fit.predict(Xs)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = 2 * (mean.numel() * 8 + Xs.numel() * 8) + (1 << 20)
    print(f"predict: peak rise {rise} bytes, allowed {allowed}")
    assert mean.shape == (20000, 2) and rise <= allowed
    ref, scale = U.mean("rbf", _np(Xs[:500]).astype(np.float64), X, THETA, False,
                        U.lml("rbf", X, Y, np.array([0.0, THETA[1], THETA[2]]), False, full=True)["alpha"])
    assert np.max(np.abs(_np(mean[:500]) - ref) / scale) <= 1e-8


def test_prediction_baselines():
    c = next(c for c in CASES if c.key == "lat17/rbf/noamp")
    n_train, n_test = [170, 119], [40, 0]  # unequal views; the second has no test rows
    Yt = np.random.RandomState(5).normal(size=(40, c.Y.shape[1])) + c.mean
    res = pkg.prediction_baselines(_dev(c.X), _dev(c.Y), _dev(c.Xs), _dev(Yt), n_train, n_test, kernel="rbf")
    assert res.views == [0] and res.fits_separate[1] is None and res.fits_separate[0].converged and res.fit_union.converged
    assert res.preds_union.shape == res.preds_separate.shape == (40, c.Y.shape[1])

    def yard(X, Y, fit):
        r = U.lml("rbf", X, Y, fit.theta, False, full=True)
        return U.prediction_error(U.mean("rbf", c.Xs, X, fit.theta, False, r["alpha"])[0], Yt)

    e_u, e_s = yard(c.X, c.Y, res.fit_union), yard(c.X[:170], c.Y[:170], res.fits_separate[0])
    print(f"union {res.error_union:.6f} (yardstick {e_u:.6f}), separate {res.error_separate:.6f} (yardstick {e_s:.6f})")
    assert abs(res.error_union - e_u) <= 1e-8 * e_u and abs(res.error_separate - e_s) <= 1e-8 * e_s
    assert res.fit_union.lml >= c.lml_hat - 1e-6 * abs(c.lml_hat)
