"""Neighbour statistics without a device: the yardstick of tests/neighbors_util.py held against sklearn, the C ABI's
declarations, the argument refusals on CPU tensors and CPU models, the torch-only scores, the closed forms of Moran's
S1 / S2, and the exports.  The kernels are exercised by tests/test_neighbors_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import gpsa
import neighbors_util as nu
import spatial_alignment_amd as pkg
from golden_io import Golden
from model_util import build_model
from spatial_alignment_amd import _lib, neighbors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64
NAMES = ("knn", "knn_regress", "spatial_r2", "kth_neighbor_distance", "moran_i", "alignment_score")


# ------------------------------------------------------------------------------------------------------------------------
# the yardstick against sklearn
# ------------------------------------------------------------------------------------------------------------------------
def test_the_yardstick_finds_sklearns_neighbours():
    skn = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 10, (1000, 2))
    Q = rng.uniform(0, 10, (300, 2))
    k = 10
    nn = skn.NearestNeighbors(n_neighbors=k + 1, algorithm="kd_tree").fit(X)
    d, i = nn.kneighbors(X)
    idx, d2 = nu.knn(X, X, k, exclude_self=True)
    assert np.array_equal(idx, i[:, 1:])  # leave-one-out: sklearn's k + 1 with column 0 (the point itself) dropped
    err = np.abs(np.sqrt(d2) - d[:, 1:]).max()
    d, i = skn.NearestNeighbors(n_neighbors=k, algorithm="kd_tree").fit(X).kneighbors(Q)
    idx, d2 = nu.knn(Q, X, k)
    assert np.array_equal(idx, i)
    err = max(err, np.abs(np.sqrt(d2) - d).max())
    print(f"[neighbors yardstick] distances vs sklearn: {err:.2e} (bar 1e-12)")
    assert err <= 1e-12


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_the_yardstick_regresses_like_sklearn_with_duplicated_points(weights):
    skn = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(1)
    X = rng.uniform(0, 10, (1000, 2))
    X[500:520] = X[:20]  # duplicated training points
    Y = rng.normal(size=(1000, 3))
    Q = np.concatenate([rng.uniform(0, 10, (200, 2)), X[:30]])  # 30 queries AT training points: zero distances
    k = 10
    # kd_tree: distances in difference form (sklearn's brute force expands |q|^2 + |r|^2 - 2 q.r, which leaves 1e-8 where
    # a query sits on a training point).  sklearn does not say which of two equidistant points it takes, so the rows
    # where a duplicated pair straddles the k-th place are set aside: 1 of 230 here
    want = skn.KNeighborsRegressor(n_neighbors=k, weights=weights, algorithm="kd_tree").fit(X, Y).predict(Q)
    got = nu.regress(X, Y, Q, k, weights)
    _, d2 = nu.knn(Q, X, k, extra=1)
    clear = d2[:, k] > d2[:, k - 1]
    assert clear.sum() >= 0.9 * len(Q) and (d2[200:, 0] == 0).all()
    err = np.abs(got - want)[clear].max()
    print(f"[neighbors yardstick] {weights} regression vs sklearn: {err:.2e} (bar 1e-14) on {clear.sum()} of {len(Q)} rows")
    assert err <= 1e-14


def test_the_yardsticks_r2_is_sklearns():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(2)
    Y = rng.normal(size=(400, 5))
    pred = Y + 0.5 * rng.normal(size=Y.shape)
    want = skm.r2_score(Y, pred, multioutput="raw_values")
    err = np.abs(nu.r2(Y, pred) - want).max()
    print(f"[neighbors yardstick] r2 vs sklearn: {err:.2e} (bar 1e-14)")
    assert err <= 1e-14
    cor = np.array([np.corrcoef(Y[:, p], pred[:, p])[0, 1] for p in range(5)])
    assert np.abs(nu.pearson(Y, pred) - cor).max() <= 1e-14


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def _declaration(name, res):
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/gpsa_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,res,n_args", [("gpsa_knn_workspace", "long long", 4), ("gpsa_knn_f64", "int", 13),
                                             ("gpsa_knn_average_f32", "int", 10),
                                             ("gpsa_knn_average_f64", "int", 10)])
def test_the_entries_are_declared_and_bound(name, res, n_args):
    args = _declaration(name, res)
    assert len(args) == n_args, args
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is (_lib._ll if res == "long long" else _lib._i)
    assert len(argtypes) == n_args
    for a, t in zip(args, argtypes):  # pointers bind as void*, long long as c_longlong, int as c_int
        want = _lib._vp if "*" in a else (_lib._ll if a.startswith("long long") else _lib._i)
        assert t is want, (name, a, t)
    src = open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "neighbors.hip")).read()
    assert re.search(r"\b" + res + r"\s+" + name + r"\s*\(", src)
    assert "atomic" not in src.lower()  # comments included


def test_the_custom_ops_propagate_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        e = lambda *sh, dt=f64: torch.empty(*sh, dtype=dt, device="cuda")
        idx, d2 = torch.ops.gpsa.knn(e(700, 2), e(900, 2), 10)
        assert (idx.shape, d2.shape, idx.dtype, d2.dtype) == ((700, 10), (700, 10), torch.int32, f64)
        out = torch.ops.gpsa.knn_average(idx, d2, e(900, 50, dt=torch.float32), "distance")
        assert out.shape == (700, 50) and out.dtype == torch.float32
        assert torch.ops.gpsa.knn_average(idx, None, e(900, 3)).dtype == f64


# ------------------------------------------------------------------------------------------------------------------------
# refusals: every one on CPU tensors, before any device work
# ------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused_by_name_of_the_device():
    X, Y = torch.rand(50, 2), torch.rand(50, 3)
    for call in (lambda: neighbors.knn(X), lambda: neighbors.knn(X, torch.rand(20, 2), k=3),
                 lambda: neighbors.knn_regress(X, Y, torch.rand(7, 2)), lambda: neighbors.spatial_r2(X, Y),
                 lambda: neighbors.kth_neighbor_distance(X), lambda: neighbors.moran_i(X, Y)):
        with pytest.raises(ValueError, match="device 'cpu'"):
            call()


def test_arguments_are_refused_before_any_device_work():
    X, Y = torch.rand(50, 2), torch.rand(50, 3)
    for bad in (torch.rand(50), torch.rand(50, 5), torch.rand(2, 50, 2), torch.zeros(50, 2, dtype=torch.int64), None,
                torch.rand(0, 2)):
        with pytest.raises(ValueError, match="shape"):
            neighbors.kth_neighbor_distance(bad)
        with pytest.raises(ValueError, match="shape"):
            neighbors.knn(X, bad if bad is not None else torch.rand(5, 3))
    with pytest.raises(ValueError, match="same D"):
        neighbors.knn(X, torch.rand(20, 3))
    with pytest.raises(ValueError, match="same D"):
        neighbors.knn_regress(X, Y, torch.rand(20, 3))
    for k in (0, -1, 33, 2.0, "3", True):
        with pytest.raises(ValueError, match="k must be"):
            neighbors.knn(X, k=k)
        with pytest.raises(ValueError, match="k must be"):
            neighbors.moran_i(X, Y, k=k)
    with pytest.raises(ValueError, match="k = 11 neighbours asked of 10"):
        neighbors.knn(X, torch.rand(10, 2), k=11)
    with pytest.raises(ValueError, match="k = 10 neighbours asked of 9 .*left out"):
        neighbors.knn(torch.rand(10, 2), k=10)
    with pytest.raises(ValueError, match="k = 10 neighbours asked of 9 .*left out"):
        neighbors.spatial_r2(torch.rand(10, 2), torch.rand(10, 1), k=10)
    with pytest.raises(ValueError, match="exclude_self"):
        neighbors.knn(X, torch.rand(50, 2), exclude_self=True)
    with pytest.raises(ValueError, match="exclude_self"):
        neighbors.knn_regress(X, Y, torch.rand(50, 2), exclude_self=True)
    for Ybad in (torch.rand(49, 3), torch.rand(50), torch.rand(50, 0)):
        with pytest.raises(ValueError, match="shape"):
            neighbors.knn_regress(X, Ybad, X)
        with pytest.raises(ValueError, match="shape"):
            neighbors.moran_i(X, Ybad)
    with pytest.raises(ValueError, match="weights"):
        neighbors.knn_regress(X, Y, X, weights="inverse")
    with pytest.raises(ValueError, match="weights"):
        neighbors.spatial_r2(X, Y, weights=None)
    for c in (0, -3, 2.5):
        with pytest.raises(ValueError, match="rows_per_chunk"):
            neighbors.knn(X, rows_per_chunk=c)
    Yn = Y.clone()
    Yn[3, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        neighbors.moran_i(X, Yn)
    with pytest.raises(ValueError, match="shape"):
        neighbors.r2_score(Y, Y[:-1])
    with pytest.raises(ValueError, match="shape"):
        neighbors.pearson(Y[:, 0], Y[:, 0])


def _cpu_model(name="c1_example_fixed0"):
    g = Golden(name)
    model, dd = build_model(g, device="cpu")
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    Y = {m: dd[m]["outputs"] for m in g.mods}
    return g, model, X, Y


def test_alignment_score_refuses_on_a_cpu_model():
    g, model, X, Y = _cpu_model()
    m = g.mods[0]
    N = X[m].shape[0]
    with pytest.raises(ValueError, match="device 'cpu'"):
        model.alignment_score(X, Y)
    with pytest.raises(ValueError, match=r"X_spatial.*row counts"):
        model.alignment_score({m: X[m][:-1]}, Y)
    with pytest.raises(ValueError, match=r"Y\[.*row counts"):
        model.alignment_score(X, {m: Y[m][:-1]})
    with pytest.raises(ValueError, match=r"G\[.*row counts"):
        model.alignment_score(X, Y, G={m: torch.rand(N, model.n_spatial_dims + 1)})
    with pytest.raises(ValueError, match="weights"):
        model.alignment_score(X, Y, weights="gaussian")
    small_view = {m: [np.arange(5), np.arange(5, N)] + [np.arange(0)] * (model.n_views - 2)}
    with pytest.raises(ValueError, match="k = 6 neighbours asked of 5"):
        model.alignment_score(X, Y, small_view, k=6)
    one_view = {m: [np.arange(N)] + [np.arange(0)] * (model.n_views - 1)}
    with pytest.raises(ValueError, match="two non-empty views"):
        model.alignment_score(X, Y, one_view)
    # a plug-in warp kernel: warp_field's refusal, unless the aligned coordinates are handed in
    model.kernel_func_warp = lambda x1, x2, **kw: pkg.rbf_kernel(x1, x2, **kw)
    with pytest.raises(ValueError, match="built-in"):
        model.alignment_score(X, Y)
    with pytest.raises(ValueError, match="device 'cpu'"):  # past that check with G given
        model.alignment_score(X, Y, G={m: X[m].double()})


# ------------------------------------------------------------------------------------------------------------------------
# what runs in torch alone
# ------------------------------------------------------------------------------------------------------------------------
def test_r2_and_pearson_leave_nan_entries_out_per_column():
    rng = np.random.default_rng(3)
    Y = rng.normal(size=(200, 4))
    pred = Y + 0.3 * rng.normal(size=Y.shape)
    Y[rng.random(Y.shape) < 0.1] = np.nan
    pred[rng.random(Y.shape) < 0.1] = np.nan
    Y[:, 3] = 2.5  # a constant column: SS_tot == 0 -> NaN (sklearn: 0 or 1)
    r = neighbors.r2_score(torch.tensor(Y), torch.tensor(pred))
    c = neighbors.pearson(torch.tensor(Y), torch.tensor(pred))
    assert r.dtype == f64 and c.dtype == f64 and r.shape == (4,)
    wr, wc = nu.r2(Y, pred), nu.pearson(Y, pred)
    assert np.isnan(wr[3]) and np.isnan(wc[3]) and bool(torch.isnan(r[3])) and bool(torch.isnan(c[3]))
    er, ec = np.abs(r.numpy()[:3] - wr[:3]).max(), np.abs(c.numpy()[:3] - wc[:3]).max()
    print(f"[neighbors] r2 {er:.2e}, pearson {ec:.2e} vs the yardstick (bar 1e-13)")
    assert er <= 1e-13 and ec <= 1e-13
    allnan = torch.full((5, 1), float("nan"), dtype=f64)
    assert bool(torch.isnan(neighbors.r2_score(allnan, allnan)).all())


def test_morans_closed_forms_of_s1_and_s2_equal_the_dense_sums():
    """S1 = w^2 (E + mutual) and S2 = w^2 sum_i (k + indegree_i)^2, as neighbors.moran_i forms them from bincount and
    idx[idx] == i, against the sums over the dense W"""
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 10, (300, 2))
    k = 6
    idx, _ = nu.knn(X, X, k, exclude_self=True)
    n = len(X)
    mutual = float((idx[idx] == np.arange(n)[:, None, None]).any(-1).sum())
    indeg = np.bincount(idx.ravel(), minlength=n).astype(np.float64)
    for std in (True, False):
        w = 1.0 / k if std else 1.0
        ref = nu.moran(X, rng.normal(size=(n, 1)), k, std)
        S0, S1, S2 = w * n * k, w * w * (n * k + mutual), w * w * float(((indeg + k) ** 2).sum())
        assert abs(S0 - ref["S0"]) <= 1e-9 * ref["S0"] and abs(S1 - ref["S1"]) <= 1e-9 * ref["S1"]
        assert abs(S2 - ref["S2"]) <= 1e-9 * ref["S2"]


def test_exports():
    for name in NAMES:
        assert getattr(gpsa, name) is getattr(pkg, name) is getattr(neighbors, name)
        assert name in pkg.__all__ and name in gpsa.__all__
    assert callable(pkg.VariationalGPSA.alignment_score)
