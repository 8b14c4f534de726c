"""Highly variable genes without a device: the numpy yardstick of tests/hvg_util.py and the package's own torch ranking
held against what pandas returns (tests/golden/reference_hvg.npz), the declarations, bindings and refusals of
csrc/moments.hip's entries, the custom ops' shapes, what the register allocator did, the exports, the refusals before
any device work, and the host logic of ``column_moments`` / ``highly_variable_genes`` / ``prepare_counts(selection=
"seurat")`` through a fake backend of this file's own.  The kernels run in tests/test_hvg_gpu.py."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

import counts_util as cu
import gpsa
import hvg_util as hu
import spatial_alignment_amd as pkg
from spatial_alignment_amd import _lib, counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64, f32, i64, i32 = torch.float64, torch.float32, torch.int64, torch.int32
ENTRIES = [("gpsa_column_moments_workspace", "long long", 3), ("gpsa_column_moments_csr_workspace", "long long", 3),
           ("gpsa_column_moments_f32", "int", 14), ("gpsa_column_moments_csr_f32", "int", 18)]
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_hvg.npz"))
CASES = sorted({k.split("/")[0] for k in GOLDEN.files})


def _case(name):
    g = {k.split("/")[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "/")}
    g["n_bins"], g["n_top"] = int(g["n_bins"]), (None if int(g["n_top"]) < 0 else int(g["n_top"]))
    return g


def _same(got, want, bar=1e-12):
    """NaN in the same places, the rest within ``bar`` of max(1, |value|) -> the largest deviation"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    same_inf = np.isinf(want[fin]) & (got[fin] == want[fin])
    err = np.where(same_inf, 0.0, np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))
    worst = float(err.max()) if err.size else 0.0
    assert worst <= bar, worst
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# the yardstick and the package's ranking against pandas
# ------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_cases_the_ranking_can_go_wrong_on():
    assert CASES == ["base", "bounds", "flat", "masked", "outlier", "ties", "tiny"]
    sizes = lambda g: np.bincount(g["bin"][g["mask"]], minlength=g["n_bins"])
    out = _case("outlier")
    assert (sizes(out) == 1).any() and (sizes(out) == 0).any()  # a bin with exactly one gene, an empty bin
    base = _case("base")
    assert (base["mean"] == 0).sum() == 1 and np.isnan(base["dispersions_norm"][base["mean"] == 0]).all()  # an all-zero gene
    ties = _case("ties")
    d = ties["dispersions_norm"]
    assert d[30] == d[31] and ties["highly_variable"][30] and ties["highly_variable"][31]
    assert int(ties["highly_variable"].sum()) == ties["n_top"] + 1  # the tie at the cutoff keeps one gene more
    assert 0 < _case("masked")["mask"].sum() < 300 and _case("bounds")["n_top"] is None
    assert np.ptp(np.log1p(_case("flat")["mean"])) == 0  # pandas' zero-range rule


@pytest.mark.parametrize("name", CASES)
def test_the_yardstick_equals_pandas(name):
    g = _case(name)
    r = hu.seurat(g["mean"], g["var"], g["n_bins"], g["mask"])
    assert np.array_equal(r["bin"], g["bin"])
    worst = _same(r["dispersions_norm"], g["dispersions_norm"])
    hv = hu.select(r["means"], r["dispersions_norm"], g["mask"], g["n_top"])
    assert np.array_equal(hv, g["highly_variable"])
    print(f"[hvg yardstick] {name}: dispersions_norm vs pandas {worst:.2e} (bar 1e-12)")


@pytest.mark.parametrize("name", CASES)
def test_the_packages_ranking_equals_pandas_on_cpu_tensors(name):
    """counts._seurat_rank / _seurat_select are plain torch: the same code that runs on the device, here on the CPU"""
    g = _case(name)
    mask = torch.tensor(g["mask"])
    means, disp, dnorm, idx = counts._seurat_rank(torch.tensor(g["mean"]), torch.tensor(g["var"]), mask, g["n_bins"])
    assert means.dtype == disp.dtype == dnorm.dtype == f64 and idx.dtype == i64
    assert np.array_equal(idx.numpy()[g["mask"]], g["bin"][g["mask"]])
    _same(dnorm.numpy(), g["dispersions_norm"])
    r = hu.seurat(g["mean"], g["var"], g["n_bins"], g["mask"])
    _same(means.numpy(), r["means"], 1e-15)
    _same(disp.numpy(), r["dispersions"], 1e-14)
    kw = {k: hu.DEFAULTS[k] for k in ("min_mean", "max_mean", "min_disp", "max_disp")}
    hv = counts._seurat_select(means, dnorm, mask, g["n_top"], what="t", **kw)
    assert hv.dtype == torch.bool and np.array_equal(hv.numpy(), g["highly_variable"])


def test_n_top_genes_beyond_the_ranked_genes_warns_and_takes_them_all():
    g = _case("tiny")
    mask = torch.tensor(g["mask"])
    means, _, dnorm, _ = counts._seurat_rank(torch.tensor(g["mean"]), torch.tensor(g["var"]), mask, g["n_bins"])
    kw = {k: hu.DEFAULTS[k] for k in ("min_mean", "max_mean", "min_disp", "max_disp")}
    with pytest.warns(UserWarning, match="n_top_genes = 5 is more than the 2 genes"):
        hv = counts._seurat_select(means, dnorm, mask, 5, what="t", **kw)
    assert np.array_equal(hv.numpy(), hu.select(means.numpy(), dnorm.numpy(), g["mask"], 5))
    with pytest.raises(ValueError, match="nothing to rank"):
        counts._seurat_select(means, torch.full_like(dnorm, float("nan")), mask, 2, what="t", **kw)


def test_the_variance_is_scanpys():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(7, 5))
    s = hu.sums(X, [3, 4], "identity")
    mean, var = hu.close(s["s1"], s["s2"], [3, 4])
    assert np.allclose(mean, [X[:3].mean(0), X[3:].mean(0)], rtol=1e-13)
    assert np.allclose(var, [X[:3].var(0, ddof=1), X[3:].var(0, ddof=1)], rtol=1e-12)
    m2, v2 = counts._close_moments(torch.tensor(s["s1"]), torch.tensor(s["s2"]), [3, 4])
    assert np.array_equal(m2.numpy(), mean) and np.array_equal(v2.numpy(), var)


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def _source():
    return open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "moments.hip")).read()


@pytest.mark.parametrize("name,res,n_args", ENTRIES)
def test_the_entries_are_declared_bound_and_defined(name, res, n_args):
    raw = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, f"{name} is not declared in include/gpsa_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == n_args, args
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is (_lib._ll if res == "long long" else _lib._i) and len(argtypes) == n_args
    for a, t in zip(args, argtypes):
        if a.startswith("const long long* view_off"):  # the one host array
            want = C.POINTER(_lib._ll)
        elif "*" in a:
            want = _lib._vp
        else:
            want = _lib._ll if a.startswith("long long") else _lib._i
        assert t is want or t == want, (name, a, t)
    assert raw.index("gpsa_csr_gather_dense_f32(const") < raw.index("csrc/moments.hip") < raw.index(name + "(")
    src = _source()
    assert re.search(r"\b" + res + r"\s+" + name + r"\s*\(", src)
    assert "atomic" not in src.lower()  # comments included
    assert "atomic" not in open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "row_walk.hpp")).read().lower()  # ... and the header the count units share


def test_the_constants_python_exports_are_the_kernels():
    src = _source()
    for py, c in (("MOM_ROWS_MIN", "MOM_ROWS_MIN"), ("MOM_MAX_GROUPS", "MOM_MAX_GROUPS"),
                  ("MOM_CSR_MAX_GROUPS", "MOM_CSR_MAX_GROUPS"), ("MOM_COL_TILE", "MOM_COL_TILE")):
        m = re.search(r"constexpr int " + c + r" = (\d+);", src)
        assert m and int(m.group(1)) == getattr(counts, py), c


def test_the_workspace_queries_are_pure_and_small():
    lib = _lib.load()
    RM, MG, CG, CT = counts.MOM_ROWS_MIN, counts.MOM_MAX_GROUPS, counts.MOM_CSR_MAX_GROUPS, counts.MOM_COL_TILE
    for N, P, V in ((1, 1, 1), (33, 65, 2), (RM * MG, CT, 1), (RM * MG + 1, CT + 1, 3), (4000, 20000, 1), (100000, 20000, 2)):
        gd, gc, T = min(-(-N // RM), MG), min(-(-N // RM), CG), -(-P // CT)
        assert lib.gpsa_column_moments_workspace(N, P, V) == 8 * (3 * gd * P + gd + V), (N, P, V)
        assert lib.gpsa_column_moments_csr_workspace(N, P, V) == 8 * (3 * gc * P + gc * T + V), (N, P, V)
    for N, P, V in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (-1, 5, 1)):
        assert lib.gpsa_column_moments_workspace(N, P, V) == 0 == lib.gpsa_column_moments_csr_workspace(N, P, V)
    # below 5 % of the dense matrix's bytes, and the CSR planes inside the margins' workspace: prepare_counts on a CSR
    # matrix holds one scratch buffer, which the seurat route must not grow
    assert lib.gpsa_column_moments_workspace(100000, 20000, 2) < 0.05 * 100000 * 20000 * 4
    for N, P in ((4000, 20000), (100000, 20000), (512, 1024)):
        assert lib.gpsa_column_moments_csr_workspace(N, P, 1) <= lib.gpsa_count_csr_workspace(N, P), (N, P)


def test_the_entries_refuse_before_any_launch():
    """the pointers handed in are host memory, which a launch would not survive"""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    off = (C.c_longlong * 3)(0, 2, 4)
    EINVAL, EWS = _lib.GPSA_EINVAL, _lib.GPSA_EWORKSPACE
    bad_off = [(C.c_longlong * 3)(1, 2, 4), (C.c_longlong * 3)(0, 2, 5), (C.c_longlong * 3)(0, 0, 4),
               (C.c_longlong * 3)(0, 4, 4), (C.c_longlong * 3)(0, 3, 2)]
    need = lib.gpsa_column_moments_workspace(4, 5, 2)
    dense = lambda mode=0, Y=p, N=4, P=5, sc=p, vo=off, V=2, s1=p, s2=p, ab=p, bad=p, ws=p, nb=need: \
        lib.gpsa_column_moments_f32(mode, Y, N, P, sc, vo, V, s1, s2, ab, bad, ws, nb, None)
    for kw in [dict(mode=-1), dict(mode=3), dict(Y=None), dict(N=0), dict(P=0), dict(N=-1), dict(P=2**31),
               dict(mode=2, sc=None), dict(vo=None), dict(V=0), dict(s1=None), dict(s2=None), dict(ab=None),
               dict(bad=None)] + [dict(vo=o) for o in bad_off]:
        assert dense(**kw) == EINVAL, kw
    assert dense(nb=need - 8) == EWS and dense(ws=None) == EWS and dense(mode=1, sc=None, nb=need - 8) == EWS
    need = lib.gpsa_column_moments_csr_workspace(4, 5, 2)
    csr = lambda mode=0, crow=p, col=p, val=p, keep=None, N=4, P=5, nnz=6, sc=p, vo=off, V=2, s1=p, s2=p, ab=p, bad=p, ws=p, \
        nb=need: lib.gpsa_column_moments_csr_f32(mode, crow, col, val, keep, N, P, nnz, sc, vo, V, s1, s2, ab, bad, ws, nb,
                                                 None)
    for kw in [dict(mode=-1), dict(mode=3), dict(crow=None), dict(col=None), dict(val=None), dict(N=0), dict(P=0),
               dict(N=2**31), dict(P=2**31), dict(nnz=-1), dict(nnz=21), dict(mode=2, sc=None), dict(vo=None), dict(V=0),
               dict(s1=None), dict(s2=None), dict(ab=None), dict(bad=None)] + [dict(vo=o) for o in bad_off]:
        assert csr(**kw) == EINVAL, kw
    assert csr(nb=need - 8) == EWS and csr(ws=None) == EWS


def test_the_custom_ops_propagate_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        Y = torch.empty(700, 45, dtype=f32, device="cuda")
        sc = torch.empty(700, dtype=f64, device="cuda")
        out = torch.ops.gpsa.column_moments(Y, "normalize", [0, 300, 700], sc)
        assert [tuple(t.shape) for t in out] == [(2, 45)] * 3 + [(1,)]
        assert [t.dtype for t in out] == [f64] * 3 + [i64]
        crow = torch.empty(701, dtype=i64, device="cuda")
        col, val = torch.empty(900, dtype=i32, device="cuda"), torch.empty(900, dtype=f32, device="cuda")
        keep = torch.empty(700, dtype=torch.bool, device="cuda")
        out = torch.ops.gpsa.column_moments_csr(crow, col, val, 700, 45, "expm1", [0, 100, 300, 700], None, keep)
        assert [tuple(t.shape) for t in out] == [(3, 45)] * 3 + [(1,)]
        assert [t.dtype for t in out] == [f64] * 3 + [i64]


def test_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    ks = library_kernels(_lib.LIB_PATH)
    mine = [(n, k) for n, k in zip(demangle([k["name"] for k in ks]), ks) if "gpsa::moments_" in n]
    # the dense walk in three modes x two load paths, the CSR walk in three modes, the fold, the finish
    assert len(mine) == 6 + 3 + 1 + 1, [n for n, _ in mine]
    for n, k in mine:
        assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k)
        # the dense walk: four workgroups per compute unit; the CSR walk's three planes: three
        assert k["lds"] <= (49 if "csr_walk" in n else 17) * 1024, (n, k)


def test_exports_and_aliases():
    for name in ("column_moments", "highly_variable_genes"):
        assert getattr(gpsa, name) is getattr(pkg, name) is getattr(counts, name)
        assert name in pkg.__all__ and name in gpsa.__all__
    from spatial_alignment_amd import ops

    for name in ("column_moments", "column_moments_csr"):
        assert callable(getattr(ops.HipOps, name)) and hasattr(torch.ops.gpsa, name)
    assert set(ops.HipOps.MOMENT_MODES) == set(counts.MOMENT_TRANSFORMS) == set(hu.MODES)


# ------------------------------------------------------------------------------------------------------------------------
# refusals: every one on CPU tensors, before any device work
# ------------------------------------------------------------------------------------------------------------------------
def _Y(N=40, P=6, seed=0):
    return torch.tensor(cu.recipe(N, P, seed=seed, depth=1.0), dtype=f32)


def test_cpu_tensors_are_refused_by_name_of_the_device():
    Y = _Y()
    for call in (lambda: counts.column_moments(Y), lambda: counts.column_moments(Y, [20, 20], transform="normalize"),
                 lambda: counts.highly_variable_genes(Y), lambda: counts.highly_variable_genes(Y, [10, 30], n_top_genes=3),
                 lambda: counts.prepare_counts(Y, [20, 20], selection="seurat")):
        with pytest.raises(ValueError, match="device 'cpu'"):
            call()


def test_arguments_are_refused_before_any_device_work():
    Y = _Y()
    for bad in (torch.rand(40), torch.rand(0, 6), None, np.zeros((4, 4)), torch.zeros(4, 4, dtype=torch.bool)):
        for call in (counts.column_moments, counts.highly_variable_genes):
            with pytest.raises(ValueError, match="shape"):
                call(bad)
    for call in (counts.column_moments, counts.highly_variable_genes):
        for ns in ([20, 19], [40, 0], [], [20.5, 19.5], "ab"):
            with pytest.raises(ValueError, match="n_samples_list"):
                call(Y, ns)
        with pytest.raises(ValueError, match=r"the views have \[39, 1\] rows.*at least 2"):
            call(Y, [39, 1])
        with pytest.raises(ValueError, match="at least 2"):
            call(Y[:1])
        with pytest.raises(ValueError, match="transform must be one of"):
            call(Y, transform="log1p")
        for t in (0, -5.0, float("inf"), "1e4", True):
            with pytest.raises(ValueError, match="target_sum"):
                call(Y, transform="normalize", target_sum=t)
        with pytest.raises(ValueError, match="target_sum goes with transform='normalize'"):
            call(Y, transform="expm1", target_sum=1e4)
    for n in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="n_top_genes"):
            counts.highly_variable_genes(Y, n_top_genes=n)
    for kw in (dict(min_mean="0"), dict(max_mean=None), dict(min_disp=float("nan")), dict(max_disp=True)):
        with pytest.raises(ValueError, match="must be a number"):
            counts.highly_variable_genes(Y, **kw)
    for n in (0, 2.0, True, None):
        with pytest.raises(ValueError, match="n_bins"):
            counts.highly_variable_genes(Y, n_bins=n)
    with pytest.raises(ValueError, match="combine"):
        counts.highly_variable_genes(Y, combine="both")
    for mask in (torch.ones(5, dtype=torch.bool), torch.ones(6), np.ones((6, 1), bool)):
        with pytest.raises(ValueError, match="gene_mask must be a bool"):
            counts.highly_variable_genes(Y, gene_mask=mask)
    with pytest.raises(ValueError, match="selection must be one of"):
        counts.prepare_counts(Y, [40], selection="dispersion")


# ------------------------------------------------------------------------------------------------------------------------
# the host logic through a fake backend: the yardstick's sums behind the interface of ops.HipOps
# ------------------------------------------------------------------------------------------------------------------------
def _moment_tensors(s):
    return (torch.tensor(s["s1"]), torch.tensor(s["s2"]), torch.tensor(s["abs1"]), torch.tensor([s["n_nonfinite"]]))


class FakeMomentOps:
    """column_moments / column_moments_csr of ops.HipOps from tests/hvg_util.py on CPU tensors; every other method from
    the fakes of tests/test_counts_sparse.py (which holds the dense ones of tests/test_counts.py)"""

    def __init__(self):
        from test_counts_sparse import FakeSparseOps

        self.base = FakeSparseOps()
        self.calls = []

    def __getattr__(self, name):
        return getattr(self.base, name)

    def column_moments(self, Y, mode, view_off, scale=None):
        self.calls.append(("moments", tuple(Y.shape), mode, list(view_off), None if scale is None else scale.numpy().copy()))
        ns = [b - a for a, b in zip(view_off, view_off[1:])]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return _moment_tensors(hu.sums(Y.numpy(), ns, mode, None if scale is None else scale.numpy()))

    def column_moments_csr(self, crow, col, val, N, P, mode, view_off, scale=None, keep=None):
        from test_counts_sparse import _dense_of

        self.calls.append(("moments_csr", (N, P), mode, list(view_off), None if scale is None else scale.numpy().copy(),
                           None if keep is None else int(keep.sum())))
        ns = [b - a for a, b in zip(view_off, view_off[1:])]
        stored = _dense_of(crow, col, torch.ones_like(val), N, P) > 0
        Y = _dense_of(crow, col, val, N, P)
        return _moment_tensors(hu.sums(Y, ns, mode, None if scale is None else scale.numpy(),
                                       None if keep is None else keep.numpy(), stored))


def _pipeline_input():
    Y = cu.recipe(120, 60, seed=5, depth=-0.5)
    Y[7] = 0.0       # a spot without counts in view 0
    Y[100] = 0.0     # ... and one in view 2
    Y[50] = Y[50] * 40.0 + 1.0    # a spot far above the rest
    return Y, [45, 35, 40]


ARGS = dict(min_counts=None, max_counts=None, min_cells=None, n_top_genes=None, transform="pearson", theta=100.0,
            standardize=True)


def _check_prepared(res, want, Y):
    assert np.array_equal(res.rows.numpy(), want["rows"]) and np.array_equal(res.genes.numpy(), want["genes"])
    assert res.genes.dtype == i64 and res.n_samples_list == want["n_samples_list"]
    assert res.deviance is None
    _same(res.dispersions_norm.numpy(), want["dispersions_norm"], 1e-10)
    assert res.outputs.dtype == f32 and tuple(res.outputs.shape) == (len(want["rows"]), len(want["genes"]))
    err = np.abs(res.outputs.numpy() - want["outputs"]) / np.maximum(1.0, np.abs(want["outputs"]))
    assert err.max() <= 1e-6, err.max()


@pytest.mark.parametrize("transform", counts.TRANSFORMS)
@pytest.mark.parametrize("n_top", [15, None])
def test_prepare_counts_seurat_follows_the_yardsticks_pipeline(transform, n_top):
    from test_counts_sparse import _to_csr

    Y, ns = _pipeline_input()
    kw = dict(ARGS, min_counts=1, max_counts=float(np.sort(Y.sum(1))[-2]), min_cells=5, n_top_genes=n_top,
              transform=transform)
    want = hu.prepare_seurat(Y, ns, **kw)
    assert len(want["rows"]) == 117 and 0 < want["passed"].sum() < 60  # both filters bite
    assert 3 <= len(want["genes"]) < want["passed"].sum() and (n_top is None or len(want["genes"]) == n_top)
    near, gap = hu.decisive(want["seurat"], want["passed"], n_top, 20)
    assert near > 1e-9 and gap > 1e-6
    rs_all = Y[want["rows"]].sum(1)
    scale = np.median(rs_all) / rs_all
    # the dense route
    fake = FakeMomentOps()
    before = Y.copy()
    res = counts._prepare(fake, torch.tensor(Y, dtype=f32), ns, selection="seurat", **kw)
    assert np.array_equal(Y, before)
    _check_prepared(res, want, Y)
    assert len(fake.calls) == 1 and fake.calls[0][:4] == ("moments", (117, 60), "normalize", [0, 117])
    assert np.allclose(fake.calls[0][4], scale, rtol=1e-15)
    assert not [c for c in fake.base.dense.calls if c[0] == "deviance"]  # the deviance is not computed on this route
    # the sparse route: the row filter is the kernel's mask, the scale is indexed by the original row
    fake = FakeMomentOps()
    crow, col, val = _to_csr(Y)
    A = counts._checked(fake, crow, col.to(i32), val, Y.shape, "csr_counts")
    res2 = counts._prepare(fake, A, ns, selection="seurat", **kw)
    _check_prepared(res2, want, Y)
    assert torch.equal(res2.outputs, res.outputs) and torch.equal(res2.genes, res.genes)
    assert len(fake.calls) == 1 and fake.calls[0][:4] == ("moments_csr", (120, 60), "normalize", [0, 120])
    assert fake.calls[0][5] == 117 and np.allclose(fake.calls[0][4][want["rows"]], scale, rtol=1e-15)
    assert [c[0] for c in fake.base.calls] == ["check", "margins_csr", "margins_csr", "gather"]


def test_prepare_counts_deviance_route_is_what_it_was():
    """selection="deviance" (the default, and what the positional callers get): the calls and the result of before"""
    Y, ns = _pipeline_input()
    kw = dict(ARGS, min_counts=1, min_cells=5, n_top_genes=12)
    want = cu.prepare(Y, ns, **kw)
    for sel in ({}, dict(selection="deviance")):
        fake = FakeMomentOps()
        res = counts._prepare(fake, torch.tensor(Y, dtype=f32), ns, **kw, **sel)
        assert not fake.calls and "dispersions_norm" not in res
        assert np.array_equal(res.genes.numpy(), want["genes"]) and np.array_equal(res.rows.numpy(), want["rows"])
        assert np.abs(res.deviance.numpy() - want["deviance"]).max() <= 1e-9 * np.abs(want["deviance"]).max()
        assert [c[0] for c in fake.base.dense.calls][:3] == ["margins", "margins", "deviance"]


def test_prepare_counts_seurat_refusals_in_the_host_logic():
    Y, ns = _pipeline_input()
    run = lambda **kw: counts._prepare(FakeMomentOps(), torch.tensor(Y, dtype=f32), ns, selection="seurat",
                                       **dict(ARGS, **kw))
    with pytest.raises(ValueError, match=r"2 of 120 rows have no counts.*min_counts"):
        run()
    with pytest.raises(ValueError, match="no gene is selected"):
        run(min_counts=1, min_cells=1000)
    with pytest.raises(ValueError, match="every view needs at least one"):
        run(min_counts=float(Y[:45].sum(1).max()) + 1)
    one = torch.tensor(Y[50:51], dtype=f32)
    with pytest.raises(ValueError, match="leaves 1 rows.*at least 2"):
        counts._prepare(FakeMomentOps(), one, [1], selection="seurat", **ARGS)


@pytest.mark.parametrize("transform", hu.MODES)
def test_the_public_calls_through_the_fake_backend(transform, monkeypatch):
    """column_moments and highly_variable_genes, dense and CSR, views, gene_mask and combine against the yardstick"""
    from test_counts_sparse import _to_csr

    fake = FakeMomentOps()
    monkeypatch.setattr(counts, "_ops", lambda: fake)
    monkeypatch.setattr(counts, "_on_device", lambda what, **t: None)
    Yc = cu.recipe(90, 50, seed=9, depth=-0.5)
    Yc[:, 0] += 1.0
    ns = [40, 50]
    scale = None
    if transform == "normalize":
        X, scale = Yc, hu.scale_of(Yc.sum(1))
    elif transform == "expm1":
        X = cu.normalize_log1p(Yc).astype(np.float32).astype(np.float64)
    else:
        X = cu.standardize_views(cu.normalize_log1p(Yc), ns)[0].astype(np.float32).astype(np.float64)
    s = hu.sums(X, ns, transform, scale)
    mean, var = hu.close(s["s1"], s["s2"], ns)
    crow, col, val = _to_csr(X)
    A = counts.csr_counts((crow, col, val, X.shape))
    for arg in (torch.tensor(X, dtype=f32), A, torch.sparse_csr_tensor(crow, col, val, size=X.shape)):
        got = counts.column_moments(arg, ns, transform=transform)
        assert got.mean.dtype == f64 and tuple(got.var.shape) == (2, 50) and got.n_nonfinite == 0
        _same(got.mean.numpy(), mean, 1e-13)
        _same(got.var.numpy(), var, 1e-11)
    pooled = counts.column_moments(torch.tensor(X, dtype=f32), transform=transform)
    assert tuple(pooled.mean.shape) == (1, 50)
    if transform == "identity":
        assert np.allclose(pooled.var.numpy()[0], X.var(0, ddof=1), rtol=1e-10)
        return
    mask = (Yc > 0).sum(0) >= 8
    for kw in (dict(n_top_genes=8), dict(), dict(n_top_genes=8, gene_mask=torch.tensor(mask), combine="union")):
        want = hu.hvg(X, ns, transform, scale, mask=mask if "gene_mask" in kw else None,
                      combine=kw.get("combine", "intersection"), n_top_genes=kw.get("n_top_genes"))
        for r in want["views"]:
            near, gap = hu.decisive(r, mask if "gene_mask" in kw else None, kw.get("n_top_genes"), 20)
            assert near > 1e-9 and gap > 1e-6
        for arg in (torch.tensor(X, dtype=f32), A):
            got = counts.highly_variable_genes(arg, ns, transform=transform, **kw)
            for key in ("means", "dispersions", "dispersions_norm"):
                _same(got[key].numpy(), want[key], 1e-10)
            assert got.highly_variable.dtype == torch.bool and got.genes.dtype == i64
            assert np.array_equal(got.highly_variable.numpy(), want["highly_variable"])
            assert np.array_equal(got.genes.numpy(), want["genes"]) and got.n_nonfinite == 0
    assert 0 < len(want["genes"])
