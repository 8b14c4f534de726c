"""Exact GP regression without a device: the numpy yardstick of tests/gpr_util.py against sklearn and the committed fixture
(tests/golden/reference_gpr.npz, written by tests/golden/make_gpr_golden.py), the host optimiser of
spatial_alignment_amd/gpr.py on the yardstick's LML, the C declarations, the refusals, the exports, and what the register
allocator made of csrc/gpr.hip.

Bars: the yardstick against sklearn / the fixture - LML <= 1e-12 relative, gradient <= 1e-10 of its scale
(1/2 sum |W dK|), mean and standard deviation <= 1e-12 (of the mean's scale sum_j |a k_j alpha_j| and of sqrt(a + tau2)); both
sides are fp64 restatements of the same formulas; measured on the 30 fixture cases: 2.3e-14 / 3.8e-15 / 2.5e-16 / 1.1e-14.
The optimiser: converged, <= 60 evaluations, inside the bounds, LML >= sklearn's - 1e-6 max(1, |LML|).
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

import gpr_util as U
import spatial_alignment_amd as pkg
from spatial_alignment_amd import _lib, gpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = np.log(1e-5), np.log(1e5)
CASES = U.cases()
INTERIOR = [c for c in CASES if not c.bound]


def test_fixture_has_the_cases_it_must():
    keys = {c.key for c in CASES}
    assert len(CASES) == 30 and len(INTERIOR) >= 15
    for data, (n, P) in {"lat17": (289, 4), "lat20": (400, 8), "lat15": (225, 1)}.items():
        for kind in U.KERNELS:
            for amp in ("amp", "noamp"):
                assert f"{data}/{kind}/{amp}" in keys
        c = next(c for c in CASES if c.data == data)
        assert c.X.shape == (n, 2) and c.Y.shape == (n, P)
    assert {c.X.shape[1] for c in CASES} == {1, 2, 3}
    assert all(c.X.shape[0] <= 400 for c in CASES)
    # the bound case: the third data set with matern12 and no amplitude ends at the noise bound
    b = next(c for c in CASES if c.key == "lat15/matern12/noamp")
    assert b.bound and abs(b.theta_hat[2] - LO) < 1e-3
    assert os.path.getsize(U.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_yardstick_equals_the_fixture(c):
    r = U.lml(c.kernel, c.X, c.Y, c.theta1, c.amplitude, full=True)
    e_v = abs(r["value"] - c.lml1) / abs(c.lml1)
    e_g = np.abs(r["grad"] - c.grad1) / r["grad_scale"]
    if not c.amplitude:
        e_g[0] = 0.0
    h = U.lml(c.kernel, c.X, c.Y, c.theta_hat, c.amplitude, full=True)
    e_h = abs(h["value"] - c.lml_hat) / max(1.0, abs(c.lml_hat))
    m, ms = U.mean(c.kernel, c.Xs, c.X, c.theta_hat, c.amplitude, h["alpha"])
    e_m = np.max(np.abs(m - c.mean) / ms)
    a, _, tau2 = U.params(c.theta_hat, c.amplitude)
    sd = np.sqrt(U.variance(c.kernel, c.Xs, c.X, c.theta_hat, c.amplitude, h["L"]))
    e_s = np.max(np.abs(sd - c.std)) / np.sqrt(a + tau2)
    print(f"{c.key}: lml {e_v:.1e} lml_hat {e_h:.1e} grad {np.max(e_g):.1e} mean {e_m:.1e} std {e_s:.1e}")
    assert e_v <= 1e-12 and e_h <= 1e-12
    assert np.max(e_g) <= 1e-10
    assert e_m <= 1e-12 and e_s <= 1e-12


@pytest.mark.parametrize("kind", U.KERNELS)
@pytest.mark.parametrize("amplitude", [False, True])
def test_yardstick_equals_sklearn(kind, amplitude):
    pytest.importorskip("sklearn")
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel

    X, Y, Xs = U.lattice(9, 2, 3, 1.2, 0.1, 21, n_test=17)
    th = np.array([0.4, -0.2, -1.1])
    k = RBF(np.exp(th[1])) if kind == "rbf" else Matern(np.exp(th[1]), nu=1.5 if kind == "matern32" else 0.5)
    if amplitude:
        k = ConstantKernel(np.exp(th[0])) * k
    gp = GaussianProcessRegressor(k + WhiteKernel(np.exp(th[2])), alpha=1e-10, optimizer=None).fit(X, Y)
    v, g = gp.log_marginal_likelihood(gp.kernel_.theta, eval_gradient=True)
    r = U.lml(kind, X, Y, th, amplitude, full=True)
    assert abs(r["value"] - v) <= 1e-12 * abs(v)
    g3 = g if amplitude else np.concatenate([[0.0], g])
    assert np.all(np.abs(r["grad"] - g3) <= 1e-10 * r["grad_scale"])
    mean, std = gp.predict(Xs, return_std=True)
    std = std if std.ndim == 1 else std[:, 0]
    m, ms = U.mean(kind, Xs, X, th, amplitude, r["alpha"])
    assert np.max(np.abs(m - mean) / ms) <= 1e-12
    a, _, tau2 = U.params(th, amplitude)
    sd = np.sqrt(U.variance(kind, Xs, X, th, amplitude, r["L"]))
    assert np.max(np.abs(sd - std)) <= 1e-12 * np.sqrt(a + tau2)


def test_conditioning_of_the_whole_call_cases():
    """cond(K) <= 1 + a N / tau2 <= 1e6 at every theta the device's whole-call test is run at (tests/test_gpr_gpu.py)"""
    worst = 0.0
    edge = U.block_edge_cases()
    assert [c.X.shape[0] for c in edge] == [257, 300]
    for c in INTERIOR + edge:
        for th in (c.theta1, c.theta_hat):
            worst = max(worst, U.cond_bound(c.X.shape[0], th, c.amplitude))
    print(f"largest bound on cond(K): {worst:.3g}")
    assert worst <= 1e6


@pytest.mark.parametrize("c", INTERIOR, ids=repr)
def test_optimiser_on_the_yardstick(c):
    free = [0, 1, 2] if c.amplitude else [1, 2]
    r = gpr.maximize(lambda th: U.lml(c.kernel, c.X, c.Y, th, c.amplitude)[:2], np.zeros(3), free, LO, HI)
    print(f"{c.key}: n_iter {r['n_iter']} n_eval {r['n_eval']} LML - sklearn's {r['value'] - c.lml_hat:+.2e}")
    assert r["converged"] and r["n_eval"] <= 60
    assert np.all(r["theta"][free] >= LO) and np.all(r["theta"][free] <= HI)
    assert r["value"] >= c.lml_hat - 1e-6 * max(1.0, abs(c.lml_hat))


def test_optimiser_backtracks_from_minus_infinity_and_respects_the_box():
    calls = []

    def fun(th):  # a concave bowl with its top outside the box and a region that "does not factorise"
        calls.append(th.copy())
        if th[1] > 2.5:
            return -np.inf, np.zeros(3)
        d = th - np.array([0.0, 2.4, -20.0])
        return -0.5 * d @ (np.array([1.0, 3.0, 0.5]) * d), -np.array([1.0, 3.0, 0.5]) * d

    r = gpr.maximize(fun, np.zeros(3), [1, 2], LO, HI)
    assert r["converged"] and abs(r["theta"][1] - 2.4) < 1e-5 and r["theta"][2] == LO and r["theta"][0] == 0.0
    # no step moves a coordinate by more than 2 log units: every point tried is that close to an earlier one (its base)
    assert len(calls) > 3
    for i in range(1, len(calls)):
        assert min(np.max(np.abs(calls[i] - c)) for c in calls[:i]) <= 2.0 + 1e-12, i
    with pytest.raises(ValueError, match="does not factorise"):
        gpr.maximize(lambda th: (-np.inf, np.zeros(3)), np.zeros(3), [1, 2], LO, HI)


def _declaration(name):
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"([a-z ]+?)\b" + name + r"\s*\(([^;]*?)\)\s*;", src)
    assert m, name
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def test_c_declarations_equal_signatures():
    import ctypes as C

    def ctype(arg):
        if "*" in arg:
            return C.c_void_p
        base = arg.rsplit(" ", 1)[0].replace("const ", "").strip() if " " in arg else arg
        return {"int": C.c_int, "long long": C.c_longlong, "double": C.c_double}[base]

    names = ("gpsa_gpr_cov_f64", "gpsa_gpr_lml_grad_workspace", "gpsa_gpr_lml_grad_f64", "gpsa_gpr_mean_f64")
    for name in names:
        ret, args = _declaration(name)
        res, argtypes = _lib.SIGNATURES[name]
        assert res is {"int": C.c_int, "long long": C.c_longlong}[ret], name
        assert [ctype(a) for a in args] == list(argtypes), name
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)


def test_workspace_query_is_pure():
    lib = _lib.load()
    q = lib.gpsa_gpr_lml_grad_workspace
    tiles = lambda N: (-(-N // 64)) * (-(-N // 64) + 1) // 2
    for N in (1, 64, 65, 257, 5000):
        for P in (1, 50):
            assert q(N, P) == 24 * tiles(N) == q(N, P)
    assert q(0, 1) == 0 and q(5, 0) == 0
    assert gpr.gpr_bytes(5000, 50) == 3 * 8 * 5000 ** 2 + lib.gpsa_chol_inv_blocked_workspace(5000, 1) + 3 * 8 * 5000 * 50


def test_entries_refuse_bad_arguments_before_any_launch():
    """NULL pointers, sizes, kinds and a short workspace are refused by the C entries (no device is touched)"""
    import ctypes as C

    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    E, U_, W = _lib.GPSA_EINVAL, _lib.GPSA_EUNSUPPORTED, _lib.GPSA_EWORKSPACE
    assert lib.gpsa_gpr_cov_f64(0, None, 4, p, 4, 2, p, 0, 0, 0.0, p, None) == E
    assert lib.gpsa_gpr_cov_f64(7, p, 4, p, 4, 2, p, 0, 0, 0.0, p, None) == E
    assert lib.gpsa_gpr_cov_f64(0, p, 4, p, 5, 2, p, 0, 1, 0.0, p, None) == E      # same with na != nb
    assert lib.gpsa_gpr_cov_f64(0, p, 4, p, 4, 2, p, 0, 0, -1.0, p, None) == E
    assert lib.gpsa_gpr_cov_f64(0, p, 4, p, 4, 5, p, 0, 0, 0.0, p, None) == U_
    assert lib.gpsa_gpr_lml_grad_f64(0, p, 4, 2, p, 0, p, 0, p, p, p, 1 << 20, None) == E   # P = 0
    assert lib.gpsa_gpr_lml_grad_f64(0, p, 4, 5, p, 0, p, 1, p, p, p, 1 << 20, None) == U_
    assert lib.gpsa_gpr_lml_grad_f64(0, p, 4, 2, p, 0, p, 1, p, p, p, 23, None) == W
    assert lib.gpsa_gpr_lml_grad_f64(0, p, 4, 2, p, 0, p, 1, p, p, None, 1 << 20, None) == W
    assert lib.gpsa_gpr_mean_f64(0, p, 0, p, 4, 2, p, 0, p, 1, p, None) == E
    assert lib.gpsa_gpr_mean_f64(3, p, 4, p, 4, 2, p, 0, p, 1, p, None) == E
    assert lib.gpsa_gpr_mean_f64(0, p, 4, p, 4, 6, p, 0, p, 1, p, None) == U_


def test_refusals():
    X, Y = torch.rand(12, 2, dtype=torch.float64), torch.rand(12, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="device 'cpu'"):
        pkg.gp_regress(X, Y)
    bad = Y.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="Y has NaN"):
        pkg.gp_regress(X, bad)
    badx = X.clone()
    badx[0, 0] = float("inf")
    with pytest.raises(ValueError, match="X has NaN or infinite"):
        pkg.gp_regress(badx, Y)
    with pytest.raises(ValueError, match="D = 5"):
        pkg.gp_regress(torch.rand(12, 5), Y)
    for Xb, Yb in ((X[:, 0], Y), (X, Y[:11]), (X, Y[:, 0]), (X.long(), Y), (X[:0], Y[:0]), (np.zeros((12, 2)), Y)):
        with pytest.raises(ValueError, match="has shape"):
            pkg.gp_regress(Xb, Yb)
    with pytest.raises(ValueError, match="kernel must be one of"):
        pkg.gp_regress(X, Y, kernel="matern52")
    for kw in (dict(bounds=(1.0, 0.5)), dict(bounds=3), dict(theta0=[0.0, 1.0]), dict(theta0=[0.0, np.nan, 0.0]),
               dict(max_iter=-1), dict(gtol=0.0), dict(jitter=-1e-3)):
        with pytest.raises(ValueError):
            pkg.gp_regress(X, Y, **kw)
    with pytest.raises(ValueError, match="need .* bytes on the device"):
        gpr._refuse_if_too_large("gp_regress", 5000, 50, 10 ** 9)
    assert gpr._refuse_if_too_large("gp_regress", 5000, 50, 2 * 10 ** 9) == gpr.gpr_bytes(5000, 50)
    # prediction_baselines: the views must partition the rows, P must agree, some view must have test rows
    Xt, Yt = torch.rand(5, 2, dtype=torch.float64), torch.rand(5, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="does not partition"):
        pkg.prediction_baselines(X, Y, Xt, Yt, [6, 5], [5, 0])
    with pytest.raises(ValueError, match="the same P"):
        pkg.prediction_baselines(X, Y, Xt, Yt[:, :2], [6, 6], [5, 0])
    with pytest.raises(ValueError, match="test rows and no training rows"):
        pkg.prediction_baselines(X, Y, Xt, Yt, [12, 0], [3, 2])
    with pytest.raises(ValueError, match="device 'cpu'"):
        pkg.prediction_baselines(X, Y, Xt, Yt, [6, 6], [5, 0])


def test_exports_and_alias():
    import gpsa

    for name in ("gp_regress", "GPRegression", "prediction_baselines"):
        assert name in pkg.__all__ and name in gpsa.__all__
        assert getattr(gpsa, name) is getattr(pkg, name)
    from spatial_alignment_amd import torch_ops  # noqa: F401  (registers the dispatcher ops)

    for name in ("gpr_cov", "gpr_lml_grad", "gpr_mean"):
        assert hasattr(torch.ops.gpsa, name)


def test_dispatcher_ops_propagate_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from spatial_alignment_amd import torch_ops  # noqa: F401

    with FakeTensorMode():
        X, Xs = torch.empty(70, 2, dtype=torch.float64), torch.empty(9, 2, dtype=torch.float64)
        th, al = torch.empty(3, dtype=torch.float64), torch.empty(70, 5, dtype=torch.float64)
        K = torch.ops.gpsa.gpr_cov(X, X, th, "rbf", True, True, 1e-10)
        assert K.shape == (70, 70) and K.dtype == torch.float64
        assert torch.ops.gpsa.gpr_cov(Xs, X, th, "matern32").shape == (9, 70)
        assert torch.ops.gpsa.gpr_lml_grad(X, th, al, K, "rbf", True).shape == (3,)
        assert torch.ops.gpsa.gpr_mean(Xs, X, th, al, "matern12").shape == (9, 5)


def test_kernel_resources():
    """the three kernel families of csrc/gpr.hip in the built library: the launch bounds reached every instantiation
    (256 threads) and nothing lives in scratch (tools/kernel_meta.py, as tests/test_cabi.py::test_kernel_resources)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    ks = library_kernels(_lib.LIB_PATH)
    by = dict(zip(demangle([k["name"] for k in ks]), ks))
    families = ("gpr_cov_kernel<", "gpr_grad_kernel<", "gpr_mean_kernel<", "gpr_grad_close_kernel(")
    seen = {f: 0 for f in families}
    for nm, k in by.items():
        for f in families:
            if f in nm:
                seen[f] += 1
                assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0, (nm, k)
                assert k["lds"] <= 64 * 1024, (nm, k)
    assert seen == {"gpr_cov_kernel<": 3, "gpr_grad_kernel<": 3, "gpr_mean_kernel<": 3, "gpr_grad_close_kernel(": 1}, seen
