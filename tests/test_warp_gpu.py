"""warp_field / unwarp / transfer on the device: the two kernels of csrc/warp_field.hip through the C ABI alone, then the
calls on every golden fixture, on folded states, a non-identity mean and a trained state, against the fp64 yardstick of
tests/warp_util.py (the oracle's covariance functions, autograd for the Jacobian, a reference Newton iteration).

Bars (every comparison prints what it measures next to its bar):
* kernel contract, 1e-10 norm-wise: about 10 fp64 operations per term at 1.1e-16 each, M <= 257 terms and the
  sqrt(M) ~ 16 cancellation of a random-sign sum give about 5e-12;
* goldens / trained state, 1e-8 norm-wise: fp64 epsilon times the suite's worst conditioning (2e7) times a small factor;
  the yardstick's own two associations differ by 1.2e-11;
* Newton iterates and residuals, in units of extent = the largest coordinate range of the view's inducing points.
"""
import functools
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

import spatial_alignment_amd as gp
from golden_io import CASES, Golden
from model_util import build_model, run_step
from warp_util import WarpRef, folded_state, forward_G_means, free_views, relerr, view_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = torch.float64
KERNEL_BAR = 1e-10
GOLDEN_BAR = 1e-8
FOLDED = (("c6_one_dim", 0, 10), ("c6_one_dim", 1, 21), ("c4_3d_gtest", 1, 33))  # fixture, view, folded rows


def _show(tag, what, e, bar):
    print(f"[warp] {tag} {what}: {e:.2e} (bar {bar:.0e})")
    return e


# ------------------------------------------------------------------------------------------------------------------------
# 1. the kernels' contract, through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
KIND = {"rbf": 0, "matern12": 1, "matern32": 2}


def _lib():
    from spatial_alignment_amd import _lib as L

    return L.load()


def _parts(gen, kind, M, D, beta_scale=1.0):
    r = lambda *sh: torch.randn(*sh, generator=gen, dtype=f64)
    Z = torch.rand(M, D, generator=gen, dtype=f64) * 10
    beta = beta_scale * r(M, D)
    A = torch.eye(D, dtype=f64) + 0.1 * r(D, D)
    b = 0.5 * r(D)
    ls, var = torch.tensor([math.log(2.0)], dtype=f64), torch.tensor([math.log(1.3)], dtype=f64)
    return Z, beta, A, b, ls, var


def _field(kind, parts, X, jacobian=True):
    lib = _lib()
    dv = [t.to(DEV).contiguous() for t in parts]
    Xd = X.to(DEV).contiguous()
    n, D = X.shape
    nan = float("nan")
    G = torch.full((n, D), nan, dtype=f64, device=DEV)
    J = torch.full((n, D, D), nan, dtype=f64, device=DEV) if jacobian else None
    det = torch.full((n,), nan, dtype=f64, device=DEV) if jacobian else None
    p = lambda t: 0 if t is None else t.data_ptr()
    rc = lib.gpsa_warp_field_f64(KIND[kind], *(p(t) for t in dv), p(Xd), n, parts[0].shape[0], D, p(G), p(J), p(det),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu()
    return rc, host(G), host(J), host(det)


def _invert(kind, parts, target, x0, iters):
    lib = _lib()
    dv = [t.to(DEV).contiguous() for t in parts]
    td, xd = target.to(DEV).contiguous(), x0.to(DEV).contiguous()
    n, D = target.shape
    X = torch.full((n, D), 12345.0, dtype=f64, device=DEV)
    res = torch.full((n,), 12345.0, dtype=f64, device=DEV)
    rc = lib.gpsa_warp_invert_f64(KIND[kind], *(t.data_ptr() for t in dv), td.data_ptr(), xd.data_ptr(), iters, n,
                                  parts[0].shape[0], D, X.data_ptr(), res.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, X.cpu(), res.cpu()


@pytest.mark.parametrize("kind,D", list(itertools.product(KIND, (1, 2, 3, 4))))
def test_kernel_contract(kind, D):
    """G, J and det against the yardstick at M in {1, 7, 64, 200, slab + 1} x n in {1, 31, 33, 100}; row 0 coincides with
    an inducing point (Matern's sqrt(r^2 + 1e-10)).  And the inverse's iterates on a gentle warp, D = 4 included."""
    worst = {"G": 0.0, "J": 0.0, "det": 0.0}
    for M, n in itertools.product((1, 7, 64, 200, 257), (1, 31, 33, 100)):
        gen = torch.Generator().manual_seed(10000 * D + 100 * M + n)
        parts = _parts(gen, kind, M, D)
        X = torch.rand(n, D, generator=gen, dtype=f64) * 10
        X[0] = parts[0][M // 2]
        ref = WarpRef.from_parts(kind, *parts)
        Gr, Jr = ref.g_and_J(X)
        rc, G, J, det = _field(kind, parts, X)
        assert rc == 0
        for k, got, want in (("G", G, Gr), ("J", J, Jr), ("det", det, torch.linalg.det(Jr))):
            assert torch.isfinite(got).all(), (k, M, n)
            e = relerr(got, want)
            worst[k] = max(worst[k], e)
            assert e <= KERNEL_BAR, (kind, D, M, n, k, e)
        rc, G2, _, _ = _field(kind, parts, X, jacobian=False)
        assert rc == 0 and relerr(G2, Gr) <= KERNEL_BAR
    for k, e in worst.items():
        _show(f"kernel {kind} D={D}", f"worst {k} over the shapes", e, KERNEL_BAR)
    # the inverse: 0, 1 and 3 updates against the reference Newton on a gentle warp (|beta| small: J near A, no fold, so
    # an update does not amplify the 1e-12 differences of g and J beyond a small factor); bar 1e-8 * extent per row
    for M, n in ((7, 1), (257, 33)):
        gen = torch.Generator().manual_seed(77 * D + M)
        parts = _parts(gen, kind, M, D, beta_scale=0.02)
        ref = WarpRef.from_parts(kind, *parts)
        Xt = torch.rand(n, D, generator=gen, dtype=f64) * 10
        target = ref.g(Xt)
        x0 = ref.x0(target)
        its = ref.newton(target, x0, 3)
        for k in (0, 1, 3):
            rc, Xk, res = _invert(kind, parts, target, x0, k)
            assert rc == 0
            want = x0 if k == 0 else its[k - 1]
            e = float((Xk - want).norm(dim=1).max()) / ref.extent
            eres = float((res - ref.residual(Xk, target)).abs().max()) / ref.extent
            _show(f"kernel {kind} D={D} M={M} n={n}", f"iterate after {k} updates / extent", e, 1e-8)
            assert e <= 1e-8 and eres <= 1e-9, (kind, D, M, n, k, e, eres)


def test_kernels_refuse_what_they_cannot_take():
    lib = _lib()
    EINVAL, EUNSUPPORTED = -1, -3
    buf = torch.zeros(256, dtype=f64, device=DEV)  # every input: zeros (a singular A: the inverse's rows fail, no more)
    outs = [torch.zeros(64, dtype=f64, device=DEV) for _ in range(3)]
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    q0, q1, q2 = (t.data_ptr() for t in outs)
    ok_f = dict(kind=0, Z=p, beta=p, A=p, b=p, ls=p, var=p, X=p, n=3, M=2, D=2, G=q0, J=q1, det=q2)
    ok_i = dict(kind=0, Z=p, beta=p, A=p, b=p, ls=p, var=p, target=p, x0=p, iters=2, n=3, M=2, D=2, X=q0, res=q1)
    field = lambda **kw: lib.gpsa_warp_field_f64(*{**ok_f, **kw}.values(), st)
    invert = lambda **kw: lib.gpsa_warp_invert_f64(*{**ok_i, **kw}.values(), st)
    assert field() == 0 and field(J=0, det=0) == 0 and field(J=0) == 0 and invert() == 0 and invert(iters=0) == 0
    for call, ok in ((field, ok_f), (invert, ok_i)):
        for name in ok:
            if name in ("kind", "n", "M", "D", "iters", "J", "det"):
                continue
            assert call(**{name: 0}) == EINVAL, name
        for name in ("n", "M", "D"):
            assert call(**{name: 0}) == EINVAL and call(**{name: -1}) == EINVAL, name
        assert call(D=5) == EUNSUPPORTED
        assert call(kind=3) == EINVAL and call(kind=-1) == EINVAL
    assert invert(iters=-1) == EINVAL
    torch.cuda.synchronize()


def test_the_dispatcher_ops_are_the_same_calls():
    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the ops)
    from spatial_alignment_amd import engine as E

    gen = torch.Generator().manual_seed(12)
    parts = [t.to(DEV) for t in _parts(gen, "matern32", 70, 2, beta_scale=0.02)]
    X = (torch.rand(45, 2, generator=gen, dtype=f64) * 10).to(DEV)
    o = E.ops()
    G, J, det = o.warp_field("matern32", *parts, X)
    G2, J2, det2 = torch.ops.gpsa.warp_field(*parts, X, "matern32")
    assert torch.equal(G, G2) and torch.equal(J, J2) and torch.equal(det, det2)
    G3, J3, det3 = torch.ops.gpsa.warp_field(*parts, X, "matern32", False)
    assert J3.numel() == 0 and det3.numel() == 0 and relerr(G3, G) <= 1e-14
    Xb, res = o.warp_invert("matern32", *parts, G, X + 0.05, 5)
    Xb2, res2 = torch.ops.gpsa.warp_invert(*parts, G, X + 0.05, "matern32", 5)
    assert torch.equal(Xb, Xb2) and torch.equal(res, res2)
    e = _show("dispatcher ops", "round trip after 5 updates / extent", float((Xb - X).norm(dim=1).max()) / 10, 1e-8)
    assert e <= 1e-8 and float(res.max()) <= 1e-7
    with pytest.raises(ValueError, match="kind"):
        o.warp_field("cosine", *parts, X)
    with pytest.raises(ValueError, match="beta"):
        o.warp_field("rbf", parts[0], parts[1][:-1], *parts[2:], X)
    with pytest.raises(ValueError, match="iters"):
        o.warp_invert("rbf", *parts, G, X, -1)


def test_new_kernels_have_no_scratch_and_no_spills():
    """register allocation of every warp_field / warp_invert kernel, read from the code objects inside the built library"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from kernel_meta import demangle, library_kernels

    from spatial_alignment_amd import _lib as L

    ks = library_kernels(L.LIB_PATH)
    mine = [(n, k) for n, k in zip(demangle([k["name"] for k in ks]), ks)
            if "warp_field_kernel<" in n or "warp_invert_kernel<" in n]
    assert len(mine) == 3 * 4 * 2 + 3 * 4, [n for n, _ in mine]  # kinds x D x (with / without J) + kinds x D
    for n, k in mine:
        assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
        assert k["lds"] <= 64 * 1024, (n, k)


# ------------------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------------------
class _Case:
    """a golden fixture on the device with, per non-fixed view, its own rows, the yardstick and the yardstick's values
    there (computed once, shared by the tests, never changed)"""

    def __init__(self, name, state=None, prepare=None):
        self.g = g = Golden(name)
        self.model, self.dd = build_model(g, device=DEV)
        self.state = g.full_state() if state is None else state
        if prepare is not None:
            with torch.no_grad():
                prepare(self.model)
        self.views = free_views(g)
        self.ref = {v: WarpRef(self.state, g.cfg["kernel_warp"], v) for v in self.views}
        self.X = {v: view_rows(g, v) for v in self.views}
        self.GJ = {v: self.ref[v].g_and_J(self.X[v]) for v in self.views}

    def field(self, v, **kw):
        return self.model.warp_field(self.X[v].to(DEV), v, **kw)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


@functools.lru_cache(maxsize=None)
def _folded_case(name, v):
    g = Golden(name)
    st = folded_state(g, v)

    def prepare(model):
        model.delta_G_list[v].copy_(st["delta_G_list"][v])

    return _Case(name, st, prepare)


def _check_field(c, v, r, tag, want_G=None):
    Gr, Jr = c.GJ[v]
    bad = []
    for k, got, want in (("G_mean", r.G_mean, Gr if want_G is None else want_G), ("jacobian", r.jacobian, Jr),
                         ("det", r.det, torch.linalg.det(Jr))):
        assert got.dtype == f64 and got.device.type == "cuda"
        e = _show(tag, k, relerr(got, want), GOLDEN_BAR)
        if not e <= GOLDEN_BAR:
            bad.append((k, e))
    return bad


@pytest.mark.parametrize("name", CASES)
def test_goldens_match_the_forward_and_autograd(name):
    c = _case(name)
    g, model = c.g, c.model
    want = forward_G_means(g)
    view_idx, Ns, _, _ = model.create_view_idx_dict(c.dd)
    Xs = {m: c.dd[m]["spatial_coords"] for m in g.mods}
    pred = model.predict(Xs, view_idx, Ns, warp="mean")
    from oracle import gpsa_oracle as orc

    vi, _ = orc.make_view_index(g.cfg["n_samples"])
    for v in c.views:
        r = c.field(v)
        assert not _check_field(c, v, r, f"{name} view {v}", want_G=want[v])
        assert r.n_folded.dtype == torch.int64 and r.n_folded.dim() == 0 and int(r.n_folded) == 0
        assert tuple(r.jacobian.shape) == (c.X[v].shape[0], model.n_spatial_dims, model.n_spatial_dims)
        Gp = torch.cat([pred[m].G_mean[vi[m][v].to(DEV)] for m in g.mods], 0)
        e = _show(f"{name} view {v}", "G_mean.float() vs predict's G_mean", relerr(r.G_mean.float(), Gp), 1e-6)
        assert e <= 1e-6
        only = c.field(v, jacobian=False)
        assert torch.equal(only.G_mean, r.G_mean) or relerr(only.G_mean, r.G_mean) <= 1e-14
        assert only.jacobian is None and only.det is None and only.n_folded is None


def test_a_non_identity_mean_enters_the_jacobian_the_start_and_the_residual():
    name, v = "c2_three_free_views", 1
    g = Golden(name)
    V, D = g.cfg["n_views"], g.cfg["n_spatial_dims"]
    gen = torch.Generator().manual_seed(4)
    st = dict(g.full_state())
    st["mean_slopes"] = torch.eye(D).repeat(V, 1, 1)
    st["mean_intercepts"] = torch.zeros(V, D)
    st["mean_slopes"][v] += 0.1 * torch.randn(D, D, generator=gen)
    st["mean_intercepts"][v] += 0.3 * torch.randn(D, generator=gen)

    def prepare(model):
        model.mean_slopes.copy_(st["mean_slopes"])
        model.mean_intercepts.copy_(st["mean_intercepts"])

    c = _Case(name, st, prepare)
    want = forward_G_means(g, st)[v]
    r = c.field(v)
    assert not _check_field(c, v, r, f"{name} view {v} A != I", want_G=want)
    ref, X = c.ref[v], c.X[v]
    G = ref.g(X)
    its = ref.newton(G, ref.x0(G), 3)
    for k in (1, 2, 3):
        u = c.model.unwarp(G.to(DEV), v, max_iter=k)
        e = _show(f"{name} A != I", f"iterate after {k} updates / extent",
                  float((u.X.cpu() - its[k - 1]).norm(dim=1).max()) / ref.extent, 1e-8)
        assert e <= 1e-8
    assert not _check_round_trip(c, v, c.model.unwarp(G.to(DEV), v), G, X, f"{name} A != I")


@pytest.mark.parametrize("name,v,n_folded", FOLDED)
def test_folded_states_are_counted_row_for_row(name, v, n_folded):
    c = _folded_case(name, v)
    r = c.field(v)
    det_ref = torch.linalg.det(c.GJ[v][1])
    print(f"[warp] folded {name} view {v}: {int(r.n_folded)} of {det_ref.numel()} rows folded, min |det| "
          f"{float(det_ref.abs().min()):.1e} (yardstick: {int((det_ref <= 0).sum())})")
    assert int((det_ref <= 0).sum()) == n_folded  # the yardstick itself
    assert torch.equal(r.det.cpu() <= 0, det_ref <= 0)
    assert int(r.n_folded) == n_folded
    assert not _check_field(c, v, r, f"folded {name} view {v}")


@pytest.mark.parametrize("name", ["c1_example_fixed0", "c4_3d_gtest", "c6_one_dim", "c7_m200_conditioning",
                                  "c3_lmc_matern12_warp"])
def test_the_iteration_follows_the_reference_newton(name):
    c = _case(name)
    for v in c.views:
        ref, X = c.ref[v], c.X[v]
        G = c.GJ[v][0]
        its = ref.newton(G, ref.x0(G), 3)
        for k in (1, 2, 3):
            u = c.model.unwarp(G.to(DEV), v, max_iter=k)
            e = _show(f"{name} view {v}", f"iterate after {k} updates / extent",
                      float((u.X.cpu() - its[k - 1]).norm(dim=1).max()) / ref.extent, 1e-8)
            assert e <= 1e-8, (name, v, k, e)


def _check_round_trip(c, v, u, G, X_true, tag):
    """every row converged, |X - X_true| <= 2 tol / sigma_min(J_ref), the returned residual honest"""
    ref = c.ref[v]
    bad = []
    assert u.tol == 1e-8 * ref.extent or abs(u.tol - 1e-8 * ref.extent) <= 1e-15 * ref.extent
    Xg, res = u.X.cpu(), u.residual.cpu()
    if not bool(u.converged.all()):
        bad.append(("converged", int((~u.converged).sum())))
    smin = torch.linalg.svdvals(c.GJ[v][1])[:, -1] if X_true is c.X[v] else torch.linalg.svdvals(ref.g_and_J(X_true)[1])[:, -1]
    ratio = float(((Xg - X_true).norm(dim=1) * smin / (2 * u.tol)).max())
    _show(tag, "|X - X_true| sigma_min / (2 tol), worst row", ratio, 1.0)
    if not ratio <= 1.0:
        bad.append(("round trip", ratio))
    e = float((res - ref.residual(Xg, G)).abs().max()) / ref.extent
    _show(tag, "|residual - yardstick's at the returned X| / extent", e, 1e-9)
    if not e <= 1e-9:
        bad.append(("residual", e))
    print(f"[warp] {tag}: worst residual {float(res.max()):.2e}, tol {u.tol:.2e}")
    return bad


@pytest.mark.parametrize("name", CASES)
def test_round_trip_and_honest_residual(name):
    c = _case(name)
    for v in c.views:
        G = c.GJ[v][0]
        u = c.model.unwarp(G.to(DEV), v, max_iter=12)
        assert u.X.dtype == f64 and u.residual.dtype == f64 and u.converged.dtype == torch.bool
        assert not _check_round_trip(c, v, u, G, c.X[v], f"{name} view {v}")
        assert torch.equal(u.converged, u.residual <= u.tol)


@pytest.mark.parametrize("name,v,n_folded", FOLDED)
def test_folded_states_report_an_honest_residual(name, v, n_folded):
    """the preimage is not unique and the iteration is chaotic there: only honesty is checked"""
    c = _folded_case(name, v)
    ref, G = c.ref[v], c.GJ[v][0]
    u = c.model.unwarp(G.to(DEV), v, max_iter=12)
    Xg, res, conv = u.X.cpu(), u.residual.cpu(), u.converged.cpu()
    finite = torch.isfinite(Xg).all(1)
    assert torch.equal(conv, res <= u.tol)
    failed = ~finite
    assert bool(torch.isnan(Xg[failed]).all()) and bool((res[failed] == float("inf")).all()) and not bool(conv[failed].any())
    assert bool(torch.isfinite(res[finite]).all())
    e = float((res[finite] - ref.residual(Xg[finite], G[finite])).abs().max()) / ref.extent
    _show(f"folded {name} view {v}", "|residual - yardstick's| / extent on finite rows", e, 1e-9)
    print(f"[warp] folded {name} view {v}: {int(conv.sum())} of {conv.numel()} rows converged, {int(failed.sum())} failed, "
          f"largest |X| {float(Xg[finite].abs().max()):.2e}")
    assert e <= 1e-9


def _equal(a, b):
    same = lambda x, y: (x is None and y is None) or (not torch.is_tensor(x) and x == y) or \
        (torch.is_tensor(x) and torch.equal(x.nan_to_num(12345.0), y.nan_to_num(12345.0)))
    return all(same(a[k], b[k]) for k in a)


def test_a_row_does_not_depend_on_its_chunk_or_its_neighbours():
    c = _case("c2_three_free_views")
    v = c.views[0]
    gen = torch.Generator().manual_seed(8)
    X = (torch.rand(150, 2, generator=gen, dtype=f64) * 12 - 1).to(DEV)  # a lattice's worth of points, some outside
    model = c.model
    whole = model.warp_field(X, v)
    assert _equal(whole, model.warp_field(X, v, rows_per_chunk=61))
    assert torch.equal(model.warp_field(X, v, jacobian=False, rows_per_chunk=61).G_mean,
                       model.warp_field(X, v, jacobian=False).G_mean)
    G = whole.G_mean
    back = model.unwarp(G, v)
    assert _equal(back, model.unwarp(G, v, rows_per_chunk=61))
    for i in (0, 37, 149):
        one = model.warp_field(X[i: i + 1], v)
        for k in ("G_mean", "jacobian", "det"):
            assert torch.equal(one[k], whole[k][i: i + 1]), (i, k)
        ub = model.unwarp(G[i: i + 1], v)
        for k in ("X", "residual", "converged"):
            assert torch.equal(ub[k], back[k][i: i + 1]), (i, k)


def test_transfer():
    c = _case("c2_three_free_views")
    v = c.views[1]
    X = c.X[v]
    t = c.model.transfer(X.to(DEV), v, v)
    assert not _check_round_trip(c, v, t, c.GJ[v][0], X, "transfer(v -> v)")
    t2 = c.model.transfer(X.to(DEV), v, c.views[0], max_iter=12)
    ref0 = c.ref[c.views[0]]
    conv = t2.converged.cpu()
    e = float((ref0.g(t2.X.cpu()[conv]) - c.GJ[v][0][conv]).norm(dim=1).max())
    _show(f"transfer(view {v} -> view {c.views[0]}), {int(conv.sum())} of {conv.numel()} rows converged",
          "|g_to(X) - g_from(X_from)| worst converged row", e, t2.tol)
    assert bool(conv.any()) and e <= 2 * t2.tol  # converged means what it says, against the yardstick
    c1 = _case("c1_example_fixed0")  # into a fixed view: the aligned system IS that view's coordinates
    v1 = c1.views[0]
    fixed = [u for u in range(c1.g.cfg["n_views"]) if u not in c1.views][0]
    Xd = c1.X[v1].to(DEV)
    t3 = c1.model.transfer(Xd, v1, fixed)
    assert torch.equal(t3.X, c1.model.warp_field(Xd, v1, jacobian=False).G_mean)
    assert bool(t3.converged.all()) and float(t3.residual.max()) == 0.0


def test_no_side_effects_on_predict_and_training():
    name = "c5_two_modalities"
    runs = []
    for with_warp in (False, True):
        g = Golden(name)
        model, dd = build_model(g, device=DEV)
        X = {m: dd[m]["spatial_coords"] for m in g.mods}
        pts = view_rows(g, 0).to(DEV)
        grad_was = torch.is_grad_enabled()

        def calls():
            if with_warp:
                for v in free_views(g):
                    r = model.warp_field(pts, v)
                    model.unwarp(r.G_mean, v)
                    model.transfer(pts, v, 0, max_iter=3)
                assert torch.is_grad_enabled() == grad_was

        calls()
        gen = torch.Generator(device=DEV).manual_seed(5)
        pred = model.predict(X, S=3, generator=gen, latent=True)
        calls()
        step = run_step(model, dd, g, device=DEV)
        calls()
        step2 = run_step(model, dd, g, device=DEV)
        runs.append((pred, step, step2, model.training))
    (pa, sa, sa2, ta), (pb, sb, sb2, tb) = runs
    assert ta == tb
    for m in pa:
        for k in pa[m]:
            assert (pa[m][k] is None and pb[m][k] is None) or torch.equal(pa[m][k], pb[m][k]), (m, k)
    for a, b in ((sa, sb), (sa2, sb2)):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_trained_state_matches_the_yardstick():
    from spatial_alignment_amd import train
    from spatial_alignment_amd.synthetic import make_grid_problem

    dd = make_grid_problem(side=20, n_views=2, n_outputs=6, device="cpu")
    m = "expression"
    torch.manual_seed(5)
    np.random.seed(5)
    model = gp.VariationalGPSA(dd, m_X_per_view=64, m_G=64, data_init=False, n_latent_gps={m: None},
                               kernel_func_warp=gp.rbf_kernel, kernel_func_data=gp.rbf_kernel, fixed_view_idx=None)
    model = model.to(DEV)
    ddd = {m: {"spatial_coords": dd[m]["spatial_coords"].to(DEV), "outputs": dd[m]["outputs"].to(DEV),
               "n_samples_list": dd[m]["n_samples_list"]}}
    torch.manual_seed(11)
    trace = train.fit(model, ddd, 300, lr=1e-2, S=3)
    assert trace[-1] < trace[0]
    st = {k: t.detach().cpu().clone() for k, t in model.state_dict().items()}
    for nm in ("mean_slopes", "mean_intercepts"):
        st.setdefault(nm, getattr(model, nm).detach().cpu().clone())
    n0 = dd[m]["n_samples_list"][0]
    Xall = dd[m]["spatial_coords"].double()
    for v, X in ((0, Xall[:n0]), (1, Xall[n0:])):
        ref = WarpRef(st, "rbf", v)
        Gr, Jr = ref.g_and_J(X)
        r = model.warp_field(X.to(DEV), v)
        print(f"[warp] trained view {v}: displacement {float((Gr - X).norm(dim=1).max()):.3f} of extent {ref.extent:.2f}, "
              f"det in [{float(r.det.min()):.3f}, {float(r.det.max()):.3f}], folded {int(r.n_folded)}")
        for k, got, want in (("G_mean", r.G_mean, Gr), ("jacobian", r.jacobian, Jr), ("det", r.det, torch.linalg.det(Jr))):
            e = _show(f"trained view {v}", k, relerr(got, want), GOLDEN_BAR)
            assert e <= GOLDEN_BAR, (v, k, e)
