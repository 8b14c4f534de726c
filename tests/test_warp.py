"""warp_field / unwarp / transfer without a device: the yardstick of tests/warp_util.py held against the oracle's forward
and its Newton reference shown to converge, the C ABI's declarations, the argument refusals, the fixed-view identity on a
CPU model and the exports.  The kernels are exercised by tests/test_warp_gpu.py."""
import os
import re

import pytest
import torch

import gpsa
import spatial_alignment_amd as pkg
from golden_io import CASES, Golden
from model_util import build_model
from spatial_alignment_amd import _lib, warp
from warp_util import WarpRef, forward_G_means, free_views, relerr, view_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64


@pytest.mark.parametrize("name", CASES)
def test_the_yardstick_restates_the_forward_and_its_newton_converges(name):
    """g_v as a function of the point equals forward_pass's G_means at the views' own rows (1e-9, both associations of
    the yardstick), and the reference Newton from the affine start reaches 1e-8 * extent within 6 updates on every row"""
    g = Golden(name)
    want = forward_G_means(g)
    for v in free_views(g):
        ref = WarpRef(g.full_state(), g.cfg["kernel_warp"], v)
        X = view_rows(g, v)
        G = ref.g(X)
        e1, e2 = relerr(G, want[v]), relerr(ref.g_like_forward(X), want[v])
        _, J = ref.g_and_J(X)
        det = torch.linalg.det(J)
        print(f"[warp yardstick] {name} view {v}: g vs forward {e1:.2e} / {e2:.2e} (bar 1e-09); displacement "
              f"{float((G - X).norm(dim=1).max()):.3f} of extent {ref.extent:.2f}; det in [{float(det.min()):.3f}, "
              f"{float(det.max()):.3f}]")
        assert e1 <= 1e-9 and e2 <= 1e-9, (name, v, e1, e2)
        assert bool((det > 0).all()), (name, v)
        xs = ref.newton(G, ref.x0(G), 6)
        res = ref.residual(xs[-1], G)
        back = float((xs[-1] - X).norm(dim=1).max())
        print(f"[warp yardstick] {name} view {v}: residual after 6 reference updates {float(res.max()):.2e} (bar "
              f"{1e-8 * ref.extent:.2e}); round trip {back:.2e}")
        assert bool((res <= 1e-8 * ref.extent).all()), (name, v, float(res.max()))


def _declaration(name):
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/gpsa_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("gpsa_warp_field_f64", 15), ("gpsa_warp_invert_f64", 16)])
def test_the_entries_are_declared_and_bound(name, n_args):
    args = _declaration(name)
    assert len(args) == n_args, args
    res, argtypes = _lib.SIGNATURES[name]
    assert len(argtypes) == n_args
    for a, t in zip(args, argtypes):  # pointers bind as void*, long long as c_longlong, int as c_int
        want = _lib._vp if "*" in a else (_lib._ll if a.startswith("long long") else _lib._i)
        assert t is want, (name, a, t)
    src = open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "warp_field.hip")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", src)
    code = re.sub(r"//[^\n]*", "", src)
    assert "cov_eval<double, KIND>" in code and "atomic" not in code.lower()


def _cpu_model(name="c1_example_fixed0"):
    g = Golden(name)
    model, _ = build_model(g, device="cpu")
    return g, model


def test_arguments_are_refused_before_any_device_work():
    g, model = _cpu_model()
    free = free_views(g)[0]
    D = model.n_spatial_dims
    X = torch.rand(5, D)
    for bad in (-1, model.n_views, 1.0, "0", None, True):
        with pytest.raises(ValueError, match="view"):
            warp.warp_field(model, X, bad)
        with pytest.raises(ValueError, match="view"):
            warp.unwarp(model, X, bad)
    with pytest.raises(ValueError, match="view"):
        warp.transfer(model, X, free, model.n_views)
    with pytest.raises(ValueError, match="view"):
        warp.transfer(model, X, -1, free)
    for Xbad in (torch.rand(5, D + 1), torch.rand(5), torch.rand(2, 5, D)):
        with pytest.raises(ValueError, match="shape"):
            warp.warp_field(model, Xbad, free)
        with pytest.raises(ValueError, match="shape"):
            warp.unwarp(model, Xbad, free)
    with pytest.raises(ValueError, match="max_iter"):
        warp.unwarp(model, X, free, max_iter=-1)
    with pytest.raises(ValueError, match="max_iter"):
        warp.unwarp(model, X, free, max_iter=2.5)
    for tol in (0.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            warp.unwarp(model, X, free, tol=tol)
    with pytest.raises(ValueError, match="x0"):
        warp.unwarp(model, X, free, x0=torch.rand(4, D))
    with pytest.raises(ValueError, match="rows_per_chunk"):
        warp.warp_field(model, X, free, rows_per_chunk=0)


def test_a_fixed_view_is_the_identity_on_a_cpu_model():
    g, model = _cpu_model()
    fixed = g.cfg["fixed_view_idx"]
    fixed = fixed if isinstance(fixed, int) else list(fixed)[0]
    D = model.n_spatial_dims
    before = torch.is_grad_enabled()
    X = torch.rand(7, D) * 10
    r = model.warp_field(X, fixed)
    assert r.G_mean.dtype == f64 and torch.equal(r.G_mean, X.double())
    assert torch.equal(r.jacobian, torch.eye(D, dtype=f64).expand(7, D, D)) and torch.equal(r.det, torch.ones(7, dtype=f64))
    assert r.n_folded.dtype == torch.int64 and r.n_folded.dim() == 0 and int(r.n_folded) == 0
    r = model.warp_field(X, fixed, jacobian=False)
    assert torch.equal(r.G_mean, X.double()) and r.jacobian is None and r.det is None and r.n_folded is None
    u = model.unwarp(X, fixed)
    assert torch.equal(u.X, X.double()) and torch.equal(u.residual, torch.zeros(7, dtype=f64))
    assert u.converged.dtype == torch.bool and bool(u.converged.all()) and u.tol > 0
    Z = model.Xtilde[fixed].detach().double()
    assert u.tol == 1e-8 * float((Z.max(0).values - Z.min(0).values).max())
    assert model.unwarp(X, fixed, tol=0.5).tol == 0.5
    assert torch.is_grad_enabled() == before and not r.G_mean.requires_grad


def test_a_plug_in_warp_kernel_is_refused():
    g, model = _cpu_model()
    free = free_views(g)[0]
    model.kernel_func_warp = lambda x1, x2, **kw: pkg.rbf_kernel(x1, x2, **kw)  # the same numbers, no derivative
    X = torch.rand(3, model.n_spatial_dims)
    for call in (lambda: model.warp_field(X, free), lambda: model.unwarp(X, free),
                 lambda: model.transfer(X, free, free)):
        with pytest.raises(ValueError, match="built-in"):
            call()


def test_the_custom_ops_propagate_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the ops)

    M, D, n = 200, 3, 1000
    with FakeTensorMode():
        e = lambda *sh: torch.empty(*sh, dtype=f64, device="cuda")
        mdl = (e(M, D), e(M, D), e(D, D), e(D), e(1), e(1))
        G, J, det = torch.ops.gpsa.warp_field(*mdl, e(n, D), "rbf")
        assert (G.shape, J.shape, det.shape) == ((n, D), (n, D, D), (n,)) and G.dtype == J.dtype == det.dtype == f64
        G, J, det = torch.ops.gpsa.warp_field(*mdl, e(n, D), "matern32", False)
        assert (G.shape, J.numel(), det.numel()) == ((n, D), 0, 0)
        X, res = torch.ops.gpsa.warp_invert(*mdl, e(n, D), e(n, D), "matern12", 12)
        assert (X.shape, res.shape) == ((n, D), (n,)) and X.dtype == res.dtype == f64


def test_exports():
    for name in ("warp_field", "unwarp", "transfer"):
        assert getattr(gpsa, name) is getattr(pkg, name) is getattr(warp, name)
        assert name in pkg.__all__ and name in gpsa.__all__
        assert callable(getattr(pkg.VariationalGPSA, name))
