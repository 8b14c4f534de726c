"""Spatial autocorrelation without a device: the yardstick (tests/autocorr_util.py) held to exact facts - the mean of the
permuted statistic over ALL permutations, scipy's Benjamini-Hochberg, moran_i's closed forms of S1 / S2, neighbors_util's
Moran's I - and the host side of the feature: argument refusals, exports, header / table agreement, fake-tensor shapes."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import autocorr_util as au
import gpsa
import neighbors_util as nu
import spatial_alignment_amd as pkg
from spatial_alignment_amd import _lib, autocorr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64
NAMES = ("spatial_graph", "SpatialGraph", "spatial_autocorr", "fdr_bh")
ENTRIES = ("gpsa_graph_workspace", "gpsa_graph_merge_count", "gpsa_graph_merge_write", "gpsa_graph_check_f64",
           "gpsa_graph_sums_f64", "gpsa_autocorr_perm_workspace", "gpsa_autocorr_perm_f64")


# six points whose mutual graph at k = 2 leaves a vertex isolated (checked below)
SIX = np.array([[0.0, 0.0], [1.0, 0.1], [0.4, 0.9], [5.0, 5.0], [5.6, 5.2], [2.6, 2.4]])


def test_exact_means_over_all_permutations_of_six_points():
    """E[I] = -1 / (n - 1) and E[C] = 1 under the permutation distribution, for any weights: the mean over all 720
    permutations of the yardstick's statistic, three graph kinds, both weightings, an isolated vertex under "mutual"."""
    n = len(SIX)
    perms = np.array(list(itertools.permutations(range(n))))
    assert perms.shape == (720, n)
    Z = au.centre(np.random.default_rng(0).normal(size=(n, 3)))
    assert (au.adjacency(SIX, 2, "mutual").sum(1) == 0).any()
    worst = 0.0
    for kind in ("none", "union", "mutual"):
        for std in (True, False):
            W = au.dense_weights(SIX, 2, kind, std)
            for mode, want in (("moran", -1.0 / (n - 1)), ("geary", 1.0)):
                got = au.statistic(W, Z, perms, mode).mean(0)
                worst = max(worst, float(np.abs(got - want).max()))
    print(f"[autocorr] yardstick: mean over all 720 permutations off by {worst:.2e} (bar 1e-14)")
    assert worst <= 1e-14


def test_yardstick_bh_is_scipys():
    from scipy.stats import false_discovery_control

    rng = np.random.default_rng(1)
    for m in (1, 2, 17, 500):
        p = rng.uniform(size=m) ** 3
        p[: m // 5] = p[m // 5: 2 * (m // 5)]  # ties
        assert np.abs(au.bh(p) - false_discovery_control(p, method="bh")).max() <= 1e-15
    p = rng.uniform(size=40)
    p[[3, 7]] = np.nan
    got = au.bh(p)
    ok = ~np.isnan(p)
    assert np.isnan(got[~ok]).all() and np.abs(got[ok] - false_discovery_control(p[ok], method="bh")).max() <= 1e-15


def test_fdr_bh_is_the_yardsticks():
    """fdr_bh is plain torch, so it runs here: against the yardstick, NaN left out and kept"""
    rng = np.random.default_rng(2)
    p = rng.uniform(size=300) ** 2
    p[::50] = np.nan
    p[10] = p[11]
    got = pkg.fdr_bh(torch.tensor(p)).numpy()
    want = au.bh(p)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-15
    assert bool(torch.isnan(pkg.fdr_bh(torch.full((4,), float("nan"), dtype=f64))).all())
    assert pkg.fdr_bh(torch.tensor([0.5], dtype=torch.float32)).dtype == f64
    with pytest.raises(ValueError, match="fdr_bh"):
        pkg.fdr_bh(torch.rand(3, 2))


def test_yardstick_sums_equal_moran_is_closed_forms_on_the_directed_graph():
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 10, (300, 2))
    k, n = 6, 300
    idx, _ = nu.knn(X, X, k, exclude_self=True)
    mutual = float((idx[idx] == np.arange(n)[:, None, None]).any(-1).sum())
    indeg = np.bincount(idx.ravel(), minlength=n).astype(np.float64)
    for std in (True, False):
        wt = 1.0 / k if std else 1.0
        S0, S1, S2 = au.graph_sums(au.dense_weights(X, k, "none", std))
        want = (wt * n * k, wt * wt * (n * k + mutual), wt * wt * float(((indeg + k) ** 2).sum()))
        for a, b in zip((S0, S1, S2), want):
            assert abs(a - b) <= 1e-12 * b, (a, b)


def test_yardstick_morans_i_is_neighbors_utils():
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 10, (120, 2))
    Y = np.concatenate([au.expression(X, 3, 6), rng.normal(size=(120, 9)).astype(np.float32)], 1)  # smooth, then noise
    Y[:, 2] = 1.5
    for std in (True, False):
        ref = nu.moran(X, Y.astype(np.float64), 6, std)
        got = au.table(au.dense_weights(X, 6, "none", std), Y, None, "moran")
        assert np.isnan(got["stat"][2]) and np.isnan(ref["I"][2])
        assert np.nanmax(np.abs(got["stat"] - ref["I"])) <= 1e-13
        assert abs(got["var_norm"] - ref["variance"][0]) <= 1e-15 and got["expected"] == ref["expected"][0]
        # the folded tail is the upper tail where z > 0, its complement's mirror where z < 0
        z = ref["z"]
        up = z > 0
        assert up.any() and (z < 0).any()
        assert np.abs(got["pval_norm"][up] - ref["p_norm"][up]).max() <= 1e-15
        dn = z < 0
        assert np.abs(got["pval_norm"][dn] - (1.0 - ref["p_norm"][dn])).max() <= 1e-15


def test_yardstick_csr_round_trip_and_star():
    W = au.dense_weights(au.points(40, 2, 0), 3, "union", True)
    crow, col, w = au.csr(W)
    assert np.array_equal(au.dense_from_csr(crow, col, w, 40), W)
    crow, col, w, n = au.star(500)
    assert n == 501 and crow[-1] == len(col) == 1000 and crow[1] == 500
    Ws = au.dense_from_csr(crow, col, w, n)
    assert np.allclose(Ws.sum(1), 1.0) and (np.diag(Ws) == 0).all()


# ------------------------------------------------------------------------------------------------------------------------
# the host side
# ------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_on_cpu_tensors():
    X, Y = torch.rand(50, 2, dtype=f64), torch.rand(50, 3)
    with pytest.raises(ValueError, match="device 'cpu'"):
        pkg.spatial_graph(X)
    with pytest.raises(ValueError, match="device 'cpu'"):
        pkg.spatial_autocorr(X, Y)
    with pytest.raises(ValueError, match="symmetric"):
        pkg.spatial_graph(X, symmetric="both")
    with pytest.raises(ValueError, match="symmetric"):
        pkg.spatial_autocorr(X, Y, symmetric=True)
    with pytest.raises(ValueError, match="mode"):
        pkg.spatial_autocorr(X, Y, mode="getis")
    for k in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="k must be an integer"):
            pkg.spatial_graph(X, k=k)
    with pytest.raises(ValueError, match="k = 10 neighbours asked of 9"):
        pkg.spatial_graph(torch.rand(10, 2), k=10)
    for Xbad in (torch.rand(50), torch.rand(50, 5), torch.zeros(50, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="shape"):
            pkg.spatial_graph(Xbad)
    for Ybad in (torch.rand(49, 3), torch.rand(50), torch.rand(50, 0)):
        with pytest.raises(ValueError, match="shape"):
            pkg.spatial_autocorr(X, Ybad)
    for r in (-1, 2.5, True):
        with pytest.raises(ValueError, match="n_perms"):
            pkg.spatial_autocorr(X, Y, n_perms=r)
    for c in (0, 1.5):
        with pytest.raises(ValueError, match="perms_per_chunk"):
            pkg.spatial_autocorr(X, Y, perms_per_chunk=c)
    for pbad in (torch.zeros(3, 49, dtype=torch.int64), torch.zeros(50, dtype=torch.int64), torch.rand(3, 50)):
        with pytest.raises(ValueError, match="perms is"):
            pkg.spatial_autocorr(X, Y, perms=pbad)
    with pytest.raises(ValueError, match="rows_per_chunk"):
        pkg.spatial_graph(X, rows_per_chunk=0)
    Yn = Y.clone()
    Yn[3, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        pkg.spatial_autocorr(X, Yn)
    crow, col, w, n = (torch.tensor(a) if isinstance(a, np.ndarray) else a for a in au.star(5))
    with pytest.raises(ValueError, match="device 'cpu'"):
        pkg.SpatialGraph.from_csr(crow, col, w, n)
    with pytest.raises(ValueError, match="crow is"):
        pkg.SpatialGraph.from_csr(crow[:-1], col, w, n)
    with pytest.raises(ValueError, match="w is"):
        pkg.SpatialGraph.from_csr(crow, col, col, n)
    with pytest.raises(ValueError, match="n must be"):
        pkg.SpatialGraph.from_csr(crow, col, w, 0)


def test_exports():
    for name in NAMES:
        assert getattr(gpsa, name) is getattr(pkg, name) is getattr(autocorr, name)
        assert name in pkg.__all__ and name in gpsa.__all__


def test_header_and_table_agree_on_the_new_entries():
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        m = re.search(r"\b(long long|int)\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert len([a for a in m.group(2).split(",") if a.strip()]) == len(args), name
        assert (res is _lib._ll) == (m.group(1) == "long long"), name
        assert hasattr(lib, name)


def test_workspace_queries_and_refusals_before_any_launch():
    """host only: the queries are pure, and every refusal returns before a stream is touched (the device pointers are the
    dummy address 8, never dereferenced)"""
    lib = _lib.load()
    q = lib.gpsa_autocorr_perm_workspace
    groups = lambda n: -(-n // max(32, -(-n // 32)))
    for n, P, R in ((63, 1, 2), (64, 64, 7), (65, 65, 1), (1301, 200, 10), (10_000, 2000, 101), (99_856, 50, 3)):
        assert q(n, P, R) == 8 * (groups(n) * R * P + 256), (n, P, R)
    assert groups(64) == 2 and groups(65) == 3 and groups(1301) == 32 and groups(99_856) == 32
    assert q(0, 1, 1) == q(1, 0, 1) == q(1, 1, 0) == 0
    assert lib.gpsa_graph_workspace(0) == 0 and lib.gpsa_graph_workspace(257) == 128
    d, big = 8, 1 << 40
    good = dict(Z=d, n=10, P=3, crow=d, col=d, w=d, nnz=20, perms=d, R=2, mode=0, num=d, n_bad=d, ws=d, nbytes=big)
    call = lambda **kw: lib.gpsa_autocorr_perm_f64(*{**good, **kw}.values(), None)
    for bad in (dict(Z=None), dict(crow=None), dict(col=None), dict(w=None), dict(perms=None), dict(num=None),
                dict(n_bad=None), dict(n=0), dict(P=0), dict(R=0), dict(nnz=-1), dict(mode=2), dict(mode=-1)):
        assert call(**bad) == _lib.GPSA_EINVAL, bad
    assert call(n=1 << 31) == _lib.GPSA_EUNSUPPORTED and call(P=1 << 31) == _lib.GPSA_EUNSUPPORTED
    assert call(R=16 * 65535 + 1) == _lib.GPSA_EUNSUPPORTED
    assert call(ws=None) == _lib.GPSA_EWORKSPACE
    assert call(nbytes=q(10, 3, 2) - 1) == _lib.GPSA_EWORKSPACE
    assert lib.gpsa_graph_check_f64(None, d, d, 5, 4, d, d, big, None) == _lib.GPSA_EINVAL
    assert lib.gpsa_graph_check_f64(d, d, d, 5, 4, d, d, 63, None) == _lib.GPSA_EWORKSPACE
    assert lib.gpsa_graph_sums_f64(d, d, d, None, d, 5, 4, d, d, big, None) == _lib.GPSA_EINVAL
    assert lib.gpsa_graph_merge_count(d, None, None, 5, 2, 1, d, None) == _lib.GPSA_EINVAL
    assert lib.gpsa_graph_merge_count(d, d, d, 5, 2, 3, d, None) == _lib.GPSA_EINVAL
    assert lib.gpsa_graph_merge_write(d, d, d, 5, 0, 1, 1, d, 4, d, d, None) == _lib.GPSA_EINVAL


def test_fake_tensor_shapes_of_the_new_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        e = lambda *sh, dt=f64: torch.empty(*sh, dtype=dt, device="cuda")
        i32, i64 = torch.int32, torch.int64
        crow, col, w = torch.ops.gpsa.graph_merge(e(700, 6, dt=i32), None, None, "none", True)
        assert (crow.shape, col.shape, w.shape) == ((701,), (4200,), (4200,))
        assert (crow.dtype, col.dtype, w.dtype) == (i64, i32, f64)
        chk = torch.ops.gpsa.graph_check(crow, col, w, 700)
        assert chk.shape == (5,) and chk.dtype == i64
        sums = torch.ops.gpsa.graph_sums(crow, col, w, 700, e(701, dt=i64), e(4200, dt=i64))
        assert sums.shape == (3,) and sums.dtype == f64
        num, bad = torch.ops.gpsa.autocorr_perm(e(700, 50), crow, col, w, e(11, 700, dt=i32), "geary")
        assert num.shape == (11, 50) and num.dtype == f64 and bad.shape == (1,) and bad.dtype == i64
