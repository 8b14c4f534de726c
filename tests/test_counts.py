"""Count preprocessing without a device: the yardstick of tests/counts_util.py held against the reference's own results
(tests/golden/reference_counts.npz), the C ABI's declarations and refusals, the custom ops' shapes, the refusals on CPU
tensors, the host logic of ``prepare_counts`` through a fake backend of this file's own, the drop-in names, the exports
and what the register allocator did with the new kernels.  The kernels run in tests/test_counts_gpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import counts_util as cu
import gpsa
import gpsa.util
import spatial_alignment_amd as pkg
from spatial_alignment_amd import _lib, counts
from spatial_alignment_amd.util import util as pkg_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64, f32 = torch.float64, torch.float32
NAMES = ("count_stats", "size_factors", "poisson_deviance", "deviance_feature_selection", "pearson_residuals",
         "deviance_residuals", "normalize_log1p", "standardize_views", "prepare_counts")
DROP_IN = ("compute_size_factors", "poisson_deviance", "deviance_feature_selection", "deviance_residuals",
           "pearson_residuals")
ENTRIES = [("gpsa_count_workspace", "long long", 2), ("gpsa_count_margins_f32", "int", 11),
           ("gpsa_count_deviance_f32", "int", 9), ("gpsa_count_transform_f32", "int", 12),
           ("gpsa_standardize_views_f32", "int", 10)]


# ------------------------------------------------------------------------------------------------------------------------
# the yardstick against the reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_the_yardstick_equals_the_reference(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_counts.npz"))
    Y = g[f"{case}/counts"].astype(np.float64)
    stride = int(g[f"{case}/stride"])
    some = Y.sum(0) > 0
    assert (~some).sum() == 1 and (Y.sum(1) > 0).all()
    assert np.array_equal(cu.size_factors(Y), g[f"{case}/size_factors"])
    genes = g[f"{case}/deviance_genes"]
    assert np.array_equal(genes, np.nonzero(some)[0])  # the reference drops the gene without counts
    d = cu.poisson_deviance(Y)
    want = g[f"{case}/deviance"]
    err = float(np.abs((d["deviance"][genes] - want) / want).max())
    print(f"[counts yardstick] {case}: deviance vs the reference {err:.2e} relative (bar 1e-12)")
    assert err <= 1e-12 and (d["deviance"][~some] == 0).all()
    for theta in (100.0, 1.0):
        want = g[f"{case}/pearson_{theta:g}"]
        got = cu.pearson_residuals(Y, theta)[::stride]
        assert np.array_equal(got[:, some], want[:, some]) and np.isnan(want[:, ~some]).all() and (got[:, ~some] == 0).all()
    for theta in (100.0, np.inf):
        want = g[f"{case}/deviance_residuals_{theta:g}"]
        got, term = cu.deviance_residuals(Y, theta)
        assert term.min() > 0  # the reference's handling of a negative term does not run under numpy 2: none here
        assert np.array_equal(got[::stride][:, some], want[:, some]) and (got[:, ~some] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def _declaration(name, res):
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/gpsa_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,res,n_args", ENTRIES)
def test_the_entries_are_declared_and_bound(name, res, n_args):
    args = _declaration(name, res)
    assert len(args) == n_args, args
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is (_lib._ll if res == "long long" else _lib._i)
    assert len(argtypes) == n_args
    for a, t in zip(args, argtypes):
        if a.startswith("const long long*"):  # a host array
            want = C.POINTER(_lib._ll)
        elif "*" in a:
            want = _lib._vp
        else:
            want = _lib._ll if a.startswith("long long") else (_lib._d if a.startswith("double") else _lib._i)
        assert t is want or t == want, (name, a, t)
    src = open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "counts.hip")).read()
    assert re.search(r"\b" + res + r"\s+" + name + r"\s*\(", src)
    assert "atomic" not in src.lower()  # comments included
    assert "atomic" not in open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "row_walk.hpp")).read().lower()  # ... and the header the count units share


def test_the_constants_python_exports_are_the_kernels():
    src = open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "counts.hip")).read()
    for py, c in (("ROWS_MIN", "COUNT_ROWS_MIN"), ("ROWS_MAX", "COUNT_ROWS_MAX"), ("MAX_GROUPS", "COUNT_MAX_GROUPS"),
                  ("COL_TILE", "COUNT_COL_TILE")):
        m = re.search(r"constexpr int " + c + r" = (\d+);", src)
        assert m and int(m.group(1)) == getattr(counts, py), c


def test_the_workspace_query_is_pure():
    lib = _lib.load()
    G = lambda N: min(-(-N // counts.ROWS_MIN), counts.MAX_GROUPS) if N <= counts.MAX_GROUPS * counts.ROWS_MAX \
        else -(-N // counts.ROWS_MAX)
    for N, P in ((1, 1), (33, 65), (16384, 7), (16385, 7), (100000, 20000), (counts.MAX_GROUPS * counts.ROWS_MAX + 1, 3)):
        assert lib.gpsa_count_workspace(N, P) == 8 * (2 * G(N) * P + G(N) + 2 * P), (N, P)
    assert lib.gpsa_count_workspace(0, 5) == 0 and lib.gpsa_count_workspace(5, 0) == 0
    # 2 x 50 000 x 20 000: the partials are 4 % of the 8 GB matrix
    assert lib.gpsa_count_workspace(100000, 20000) < 0.05 * 100000 * 20000 * 4


def test_the_entries_refuse_before_any_launch():
    """NULL pointers, N or P < 1, an unknown mode, theta <= 0 and a short workspace come back with the documented code;
    the pointers handed in are host memory, which a launch would not survive"""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    off = (C.c_longlong * 3)(0, 2, 4)
    need = lib.gpsa_count_workspace(4, 5)
    EINVAL, EWS = _lib.GPSA_EINVAL, _lib.GPSA_EWORKSPACE
    margins = lambda Y=p, N=4, P=5, rs=p, cs=p, rn=p, cn=p, bad=p, ws=p, nb=need: \
        lib.gpsa_count_margins_f32(Y, N, P, rs, cs, rn, cn, bad, ws, nb, None)
    for kw in (dict(Y=None), dict(rs=None), dict(cs=None), dict(rn=None), dict(cn=None), dict(bad=None), dict(N=0),
               dict(P=0), dict(N=-1), dict(P=2**31)):
        assert margins(**kw) == EINVAL, kw
    assert margins(nb=need - 8) == EWS and margins(ws=None) == EWS
    dev = lambda Y=p, N=4, P=5, ls=p, a=p, b=p, ws=p, nb=need: lib.gpsa_count_deviance_f32(Y, N, P, ls, a, b, ws, nb, None)
    for kw in (dict(Y=None), dict(ls=None), dict(a=None), dict(b=None), dict(N=0), dict(P=0)):
        assert dev(**kw) == EINVAL, kw
    assert dev(nb=need - 8) == EWS and dev(ws=None) == EWS
    tr = lambda mode=0, Y=p, N=4, P=5, rs=p, cs=p, total=10.0, theta=100.0, clip=2.0, target=1.0, out=p: \
        lib.gpsa_count_transform_f32(mode, Y, N, P, rs, cs, total, theta, clip, target, out, None)
    for kw in (dict(mode=-1), dict(mode=4), dict(Y=None), dict(out=None), dict(rs=None), dict(cs=None), dict(N=0), dict(P=0),
               dict(theta=0.0), dict(theta=-1.0), dict(theta=float("nan")), dict(mode=1, theta=0.0),
               dict(mode=1, theta=float("inf")), dict(total=0.0), dict(total=float("inf")), dict(clip=-1.0),
               dict(mode=3, target=0.0), dict(mode=3, target=float("inf")), dict(mode=3, rs=None)):
        assert tr(**kw) == EINVAL, kw
    std = lambda Y=p, N=4, P=5, vo=off, V=2, out=p, nc=p, ws=p, nb=need: \
        lib.gpsa_standardize_views_f32(Y, N, P, vo, V, out, nc, ws, nb, None)
    for kw in (dict(Y=None), dict(vo=None), dict(out=None), dict(nc=None), dict(V=0), dict(N=0), dict(P=0),
               dict(vo=(C.c_longlong * 3)(1, 2, 4)), dict(vo=(C.c_longlong * 3)(0, 2, 5)),
               dict(vo=(C.c_longlong * 3)(0, 0, 4)), dict(vo=(C.c_longlong * 3)(0, 4, 4))):
        assert std(**kw) == EINVAL, kw
    assert std(nb=need - 8) == EWS and std(ws=None) == EWS


def test_the_custom_ops_propagate_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        Y = torch.empty(700, 45, dtype=f32, device="cuda")
        rs, cs, rn, cn, bad = torch.ops.gpsa.count_margins(Y)
        assert (rs.shape, cs.shape, rn.shape, cn.shape, bad.shape) == ((700,), (45,), (700,), (45,), (1,))
        assert (rs.dtype, cs.dtype, rn.dtype, cn.dtype, bad.dtype) == (f64, f64, torch.int64, torch.int64, torch.int64)
        ll, ab = torch.ops.gpsa.count_deviance(Y, rs)
        assert ll.shape == ab.shape == (45,) and ll.dtype == ab.dtype == f64
        out = torch.ops.gpsa.count_transform(Y, "pearson", rs, cs, 10.0, 100.0, 3.0)
        assert out.shape == (700, 45) and out.dtype == f32
        assert torch.ops.gpsa.count_transform(Y, "log1p", rs, None, target=5.0).shape == (700, 45)
        out, nc = torch.ops.gpsa.standardize_views(Y, [0, 300, 500, 700])
        assert out.shape == (700, 45) and out.dtype == f32 and nc.shape == (3,) and nc.dtype == torch.int64


def test_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    ks = library_kernels(_lib.LIB_PATH)
    mine = [(n, k) for n, k in zip(demangle([k["name"] for k in ks]), ks) if any(f"gpsa::{f}" in n for f in ("count_walk_kernel<", "count_fold_kernel<", "count_transform_kernel<",
                                                "count_constant_kernel("))]
    # walks: 3 modes x 2 paths; folds: 3 modes; transforms: 5 modes x 2 paths; the constant count
    assert len(mine) == 6 + 3 + 10 + 1, [n for n, _ in mine]
    for n, k in mine:
        assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k)
        assert k["lds"] <= 40 * 1024, (n, k)  # four workgroups of the walk per compute unit


# ------------------------------------------------------------------------------------------------------------------------
# refusals: every one on CPU tensors, before any device work
# ------------------------------------------------------------------------------------------------------------------------
def _Y(N=40, P=6, seed=0):
    return torch.tensor(cu.recipe(N, P, seed=seed, depth=1.0), dtype=f32)


def test_cpu_tensors_are_refused_by_name_of_the_device():
    Y = _Y()
    for call in (lambda: counts.count_stats(Y), lambda: counts.size_factors(Y), lambda: counts.poisson_deviance(Y),
                 lambda: counts.poisson_deviance(Y, torch.zeros(40, dtype=f64)),
                 lambda: counts.deviance_feature_selection(Y, 3), lambda: counts.pearson_residuals(Y),
                 lambda: counts.deviance_residuals(Y, 10.0), lambda: counts.deviance_residuals(Y, math_inf()),
                 lambda: counts.normalize_log1p(Y), lambda: counts.normalize_log1p(Y, 1e4, inplace=True),
                 lambda: counts.standardize_views(Y, [20, 20]), lambda: counts.prepare_counts(Y, [20, 20]),
                 lambda: counts.prepare_counts(Y.to(torch.int32), [40], transform="counts")):
        with pytest.raises(ValueError, match="device 'cpu'"):
            call()


def math_inf():
    return float("inf")


def test_arguments_are_refused_before_any_device_work():
    Y = _Y()
    for bad in (torch.rand(40), torch.rand(2, 40, 6), torch.rand(0, 6), torch.rand(40, 0), None, np.zeros((4, 4)),
                torch.zeros(4, 4, dtype=torch.bool)):
        for call in (counts.count_stats, counts.size_factors, counts.poisson_deviance, counts.pearson_residuals,
                     counts.normalize_log1p, lambda t: counts.deviance_residuals(t, 1.0),
                     lambda t: counts.standardize_views(t, [2, 2]), lambda t: counts.prepare_counts(t, [2, 2])):
            with pytest.raises(ValueError, match="shape"):
                call(bad)
    for theta in (0, -1.0, float("nan"), "3", None, True):
        with pytest.raises(ValueError, match="theta"):
            counts.pearson_residuals(Y, theta=theta)
        with pytest.raises(ValueError, match="theta"):
            counts.deviance_residuals(Y, theta)
        with pytest.raises(ValueError, match="theta"):
            counts.prepare_counts(Y, [40], theta=theta)
    for ns in ([20, 19], [40, 0], [], [20.5, 19.5], None, [-1, 41], "ab"):
        with pytest.raises(ValueError, match="n_samples_list"):
            counts.standardize_views(Y, ns)
        with pytest.raises(ValueError, match="n_samples_list"):
            counts.prepare_counts(Y, ns)
    with pytest.raises(ValueError, match="transform"):
        counts.prepare_counts(Y, [40], transform="sqrt")
    for kw in (dict(min_counts=-1), dict(max_counts="9"), dict(min_cells=float("nan")), dict(min_counts=True)):
        with pytest.raises(ValueError, match="must be None or a number"):
            counts.prepare_counts(Y, [40], **kw)
    for n in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="n_top_genes"):
            counts.prepare_counts(Y, [40], n_top_genes=n)
    for n in (0, 7, 2.0, True):
        with pytest.raises(ValueError, match="n_top"):
            counts.deviance_feature_selection(Y, n_top=n)
    for t in (0, -5.0, float("inf"), "1e4", True):
        with pytest.raises(ValueError, match="target_sum"):
            counts.normalize_log1p(Y, target_sum=t)
    with pytest.raises(ValueError, match="log_sz"):
        counts.poisson_deviance(Y, torch.zeros(39, dtype=f64))
    with pytest.raises(ValueError, match="log_sz"):
        counts.poisson_deviance(Y, [0.0] * 40)
    for call in (lambda t: counts.pearson_residuals(t, inplace=True), lambda t: counts.normalize_log1p(t, inplace=True),
                 lambda t: counts.standardize_views(t, [40], inplace=True)):
        with pytest.raises(ValueError, match="inplace"):
            call(Y.double())
        with pytest.raises(ValueError, match="inplace"):
            call(Y[:, ::2])  # not contiguous


# ------------------------------------------------------------------------------------------------------------------------
# prepare_counts' host logic through a fake backend: the yardstick's formulas behind the interface of ops.HipOps
# ------------------------------------------------------------------------------------------------------------------------
class FakeCountOps:
    """what csrc/counts.hip computes, from tests/counts_util.py, on CPU tensors; records what each call was given"""

    def __init__(self):
        self.calls = []

    def count_margins(self, Y):
        m = cu.margins(Y.numpy())
        self.calls.append(("margins", tuple(Y.shape)))
        return (torch.tensor(m["row_sum"]), torch.tensor(m["col_sum"]), torch.tensor(m["row_nnz"]),
                torch.tensor(m["col_nnz"]), torch.tensor([m["n_invalid"]]))

    def count_deviance(self, Y, log_sz):
        d = cu.poisson_deviance(Y.numpy(), log_sz.numpy())
        self.calls.append(("deviance", tuple(Y.shape)))
        return torch.tensor(d["ll_sat"]), torch.tensor(d["abs_sat"])

    def count_transform(self, Y, mode, row_sum, col_sum=None, total=1.0, theta=1.0, clip=0.0, target=1.0, out=None):
        y, rs = Y.numpy().astype(np.float64), row_sum.numpy()
        self.calls.append(("transform", mode, tuple(Y.shape), rs.copy(), None if col_sum is None else col_sum.numpy().copy(),
                           total, theta, clip, target, out is not None and out.data_ptr() == Y.data_ptr()))
        if mode == "log1p":
            res = cu.normalize_log1p(y, target, row_sum=rs)
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                mu = rs[:, None] * col_sum.numpy()[None, :] / total
                if mode == "pearson":
                    z = (y - mu) / np.sqrt(mu + mu**2 / theta)
                    z = np.clip(z, -clip, clip) if clip > 0 else z
                else:
                    xl = np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0) / mu), 0.0)
                    t = 2 * (xl - (y - mu)) if mode == "poisson_deviance" else \
                        2 * (xl - (y + theta) * np.log((y + theta) / (mu + theta)))
                    z = np.sign(y - mu) * np.sqrt(np.maximum(t, 0.0))
                res = np.where(mu > 0, z, 0.0)
        res = torch.tensor(res, dtype=f32)
        if out is not None:
            out.copy_(res)
            return out
        return res

    def standardize_views(self, Y, view_off, out=None):
        ns = [b - a for a, b in zip(view_off, view_off[1:])]
        self.calls.append(("standardize", tuple(Y.shape), list(view_off)))
        z, nc = cu.standardize_views(Y.numpy().astype(np.float64), ns)
        z = torch.tensor(z, dtype=f32)
        if out is not None:
            out.copy_(z)
            z = out
        return z, torch.tensor(nc)


def _pipeline_input():
    Y = cu.recipe(120, 40, seed=5, depth=0.3)
    Y[7] = 0.0       # a spot without counts in view 0
    Y[100] = 0.0     # ... and one in view 2
    Y[50] *= 40.0    # a spot far above the rest
    Y[:, 3] = Y[:, 9]  # two genes with the same counts: equal deviances
    return Y, [45, 35, 40]


def _run(Y, ns, **kw):
    fake = FakeCountOps()
    args = dict(min_counts=None, max_counts=None, min_cells=None, n_top_genes=None, transform="pearson", theta=100.0,
                standardize=True)
    args.update(kw)
    before = Y.copy()
    res = counts._prepare(fake, torch.tensor(Y, dtype=f32), ns, **args)
    assert np.array_equal(Y, before)
    return fake, res, cu.prepare(Y, ns, **args)


@pytest.mark.parametrize("transform", counts.TRANSFORMS)
def test_prepare_counts_follows_the_yardsticks_pipeline(transform):
    Y, ns = _pipeline_input()
    kw = dict(min_counts=1, max_counts=float(np.sort(Y.sum(1))[-2]), min_cells=5, n_top_genes=12, transform=transform)
    fake, res, want = _run(Y, ns, **kw)
    assert res.rows.dtype == torch.int64 and res.genes.dtype == torch.int64
    assert np.array_equal(res.rows.numpy(), want["rows"]) and len(want["rows"]) == 117
    assert np.array_equal(res.genes.numpy(), want["genes"]) and len(want["genes"]) == 12
    assert res.n_samples_list == want["n_samples_list"] == [44, 34, 39]
    assert np.abs(res.deviance.numpy() - want["deviance"]).max() <= 1e-9 * np.abs(want["deviance"]).max()
    assert res.outputs.dtype == f32 and tuple(res.outputs.shape) == (117, 12)
    err = np.abs(res.outputs.numpy() - want["outputs"]) / np.maximum(1.0, np.abs(want["outputs"]))
    assert err.max() <= 1e-6, err.max()
    kinds = [c[0] for c in fake.calls]
    tr = [c for c in fake.calls if c[0] == "transform"]
    rs_all = Y[want["rows"]].sum(1)
    if transform == "counts":
        assert res.log_offset.dtype == f32 and res.n_constant is None and not tr and "standardize" not in kinds
        assert np.abs(res.log_offset.numpy() - want["log_offset"]).max() <= 1e-6
        assert np.array_equal(res.outputs.numpy(), Y[want["rows"]][:, want["genes"]])
    else:
        assert res.log_offset is None and len(tr) == 1 and tr[0][2] == (117, 12)
        assert tr[0][9], "the transform runs in place on the pipeline's own copy"
        assert kinds[-1] == "standardize" and fake.calls[-1][2] == [0, 44, 78, 117]
        assert np.array_equal(res.n_constant.numpy(), want["n_constant"])
        sub = Y[want["rows"]][:, want["genes"]]
        if transform == "log1p":  # row sums over ALL genes of the kept rows, their median as the target
            assert np.array_equal(tr[0][3], rs_all) and tr[0][8] == float(np.median(rs_all))
        else:                     # margins of the SELECTED sub-matrix
            assert np.array_equal(tr[0][3], sub.sum(1)) and np.array_equal(tr[0][4], sub.sum(0)) and tr[0][5] == sub.sum()
            assert tr[0][1] == ("pearson" if transform == "pearson" else "nb_deviance")
            assert tr[0][7] == (np.sqrt(117) if transform == "pearson" else 0.0)
    # the order of the reads: all rows, the kept rows, the deviance of the kept rows over all genes, then the selection
    assert fake.calls[0] == ("margins", (120, 40)) and fake.calls[1] == ("margins", (117, 40))
    assert fake.calls[2] == ("deviance", (117, 40))


def test_prepare_counts_without_filters_keeps_everything_and_the_callers_matrix():
    Y = cu.recipe(60, 20, seed=6, depth=1.0)
    fake, res, want = _run(Y, [30, 30], transform="deviance", theta=float("inf"), standardize=False)
    assert np.array_equal(res.rows.numpy(), np.arange(60)) and np.array_equal(res.genes.numpy(), np.arange(20))
    tr = [c for c in fake.calls if c[0] == "transform"]
    assert tr[0][1] == "poisson_deviance" and not tr[0][9]  # out of place: the matrix is the caller's
    assert res.n_constant is None and [c[0] for c in fake.calls].count("margins") == 1
    assert np.abs(res.outputs.numpy() - want["outputs"]).max() <= 1e-6 * max(1.0, np.abs(want["outputs"]).max())


def test_prepare_counts_ranks_equal_deviances_by_the_lower_index():
    Y, ns = _pipeline_input()
    dev = cu.poisson_deviance(Y[Y.sum(1) > 0])["deviance"]
    assert dev[3] == dev[9]
    rank = int((dev > dev[3]).sum())  # genes ahead of the pair
    _, res, want = _run(Y, ns, min_counts=1, n_top_genes=rank + 1, transform="counts")
    assert 3 in res.genes.tolist() and 9 not in res.genes.tolist()
    assert np.array_equal(res.genes.numpy(), want["genes"])
    o = counts._order(torch.tensor([1.0, 5.0, 5.0, 0.0, 5.0, 7.0], dtype=f64))
    assert o.tolist() == [5, 1, 2, 4, 0, 3]
    mask = torch.tensor([True, False, True, True, True, True])
    assert counts._order(torch.tensor([1.0, 5.0, 5.0, 0.0, 5.0, 7.0], dtype=f64), mask, 3).tolist() == [5, 2, 4]


def test_prepare_counts_refusals_in_the_host_logic():
    Y, ns = _pipeline_input()
    with pytest.raises(ValueError, match=r"2 of 120 rows have no counts.*min_counts"):
        _run(Y, ns)
    with pytest.raises(ValueError, match=r"1 of 75 rows have no counts.*min_counts"):
        counts._prepare(FakeCountOps(), torch.tensor(Y[:75], dtype=f32), [45, 30], None, None, None, None, "pearson", 100.0,
                        True)
    for bad, n in ((float("nan"), 1), (-1.0, 1), (float("inf"), 1)):
        Yb = Y.copy()
        Yb[5, 5] = bad
        with pytest.raises(ValueError, match=f"{n} entries that are NaN, infinite or negative"):
            _run(Yb, ns, min_counts=1)
    with pytest.raises(ValueError, match="every view needs at least one"):
        _run(Y, ns, min_counts=float(Y[:45].sum(1).max()) + 1)
    with pytest.raises(ValueError, match="no gene passes"):
        _run(Y, ns, min_counts=1, min_cells=1000)


# ------------------------------------------------------------------------------------------------------------------------
# the drop-in names and the exports
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def yardstick_behind_the_wrappers(monkeypatch):
    """the device functions the drop-in names call, replaced by the yardstick on CPU tensors: what is left under test is
    the wrappers' own work - orientation, labels, return types"""
    monkeypatch.setattr(pkg_util, "_count_device", lambda device: torch.device("cpu"))
    monkeypatch.setattr(counts, "size_factors", lambda Y, log=False: torch.tensor(cu.size_factors(Y.numpy())))
    monkeypatch.setattr(counts, "poisson_deviance", lambda Y, log_sz=None: torch.tensor(
        cu.poisson_deviance(Y.numpy(), None if log_sz is None else log_sz.numpy())["deviance"]))
    monkeypatch.setattr(counts, "pearson_residuals", lambda Y, theta, clipping=True: torch.tensor(
        cu.pearson_residuals(Y.numpy(), theta, clipping), dtype=f32))
    monkeypatch.setattr(counts, "deviance_residuals", lambda Y, theta: torch.tensor(
        cu.deviance_residuals(Y.numpy(), theta)[0], dtype=f32))


def test_the_drop_in_names_take_plain_arrays_in_the_references_orientations(yardstick_behind_the_wrappers):
    """genes x cells arrays for the first three, spots x genes for the residuals; numpy (or a labelled result) out"""
    Y = cu.recipe(33, 65, seed=11, depth=0.5)  # spots x genes
    some = Y.sum(0) > 0
    sz = gpsa.util.compute_size_factors(Y.T)
    assert isinstance(sz, np.ndarray) and sz.shape == (33,) and np.array_equal(sz, cu.size_factors(Y))
    want = cu.poisson_deviance(Y, np.log(sz))["deviance"]
    plain = gpsa.util.poisson_deviance(Y.T, sz)
    assert np.allclose(plain.values, want, rtol=1e-13, atol=0) and list(plain.index) == list(range(65))
    devs, names = gpsa.util.deviance_feature_selection(Y.T)
    assert devs.shape == names.shape == (64,) and np.array_equal(names, np.nonzero(some)[0])
    assert np.allclose(devs, want[some], rtol=1e-13, atol=0)
    z = gpsa.util.pearson_residuals(Y, 100.0)
    assert isinstance(z, np.ndarray) and z.shape == (33, 65) and z.dtype == np.float64
    assert np.abs(z - cu.pearson_residuals(Y, 100.0)).max() <= 1e-6 * np.sqrt(33)
    d = gpsa.util.deviance_residuals(Y, np.inf)
    assert d.shape == (33, 65) and d.dtype == np.float64 and np.abs(d - cu.deviance_residuals(Y, np.inf)[0]).max() <= 1e-5
    with pytest.raises(ValueError, match="mu=None"):
        gpsa.util.deviance_residuals(Y, 10.0, mu=np.ones_like(Y))
    with pytest.raises(ValueError, match="2-D"):
        gpsa.util.compute_size_factors(np.ones(5))
    assert not re.search(r"^\s*(import|from)\s+pandas", open(pkg_util.__file__).read(), flags=re.M)


def test_the_drop_in_names_take_data_frames_and_keep_their_labels(yardstick_behind_the_wrappers):
    """a genes x cells data frame in (.values / .index), a series labelled like its rows / (deviances, gene names) out"""
    pd = pytest.importorskip("pandas")
    Y = cu.recipe(33, 65, seed=11, depth=0.5)
    frame = pd.DataFrame(Y.T, index=[f"g{g}" for g in range(65)])
    sz = gpsa.util.compute_size_factors(frame)
    assert isinstance(sz, np.ndarray) and np.array_equal(sz, cu.size_factors(Y))
    dev = gpsa.util.poisson_deviance(frame, sz)
    want = cu.poisson_deviance(Y, np.log(sz))["deviance"]
    assert isinstance(dev, pd.Series) and list(dev.index) == list(frame.index)
    assert np.allclose(dev.values, want, rtol=1e-13, atol=0)
    assert np.array_equal(gpsa.util.poisson_deviance(Y.T, sz).values, dev.values)
    devs, names = gpsa.util.deviance_feature_selection(frame)
    some = Y.sum(0) > 0
    assert devs.shape == names.shape == (64,) and list(names) == [f"g{g}" for g in np.nonzero(some)[0]]
    assert np.allclose(devs, want[some], rtol=1e-13, atol=0)


def test_exports():
    for name in NAMES:
        assert getattr(gpsa, name) is getattr(pkg, name) is getattr(counts, name)
        assert name in pkg.__all__ and name in gpsa.__all__
    for name in DROP_IN:
        assert getattr(gpsa.util, name) is getattr(pkg.util, name) is getattr(pkg_util, name)
    assert "outside the hot path" not in (pkg_util.__doc__ or "").split("plotting")[0]
