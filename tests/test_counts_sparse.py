"""Sparse count preprocessing without a device: the declarations and bindings of csrc/counts_sparse.hip, the workspace
query, the refusals of the C ABI on host pointers, the custom ops' shapes, the exports, the dispatch by argument type, the
refusals before any device work, and the sparse host logic of ``prepare_counts`` through a fake backend of this file's
own against the yardstick of tests/counts_util.py on the densified matrix.  The kernels run in
tests/test_counts_sparse_gpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import counts_util as cu
import gpsa
import spatial_alignment_amd as pkg
from spatial_alignment_amd import _lib, counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64, f32, i64, i32 = torch.float64, torch.float32, torch.int64, torch.int32
ENTRIES = [("gpsa_count_csr_workspace", "long long", 2), ("gpsa_csr_check", "int", 10),
           ("gpsa_count_margins_csr_f32", "int", 15), ("gpsa_count_deviance_csr_f32", "int", 13),
           ("gpsa_csr_gather_dense_f32", "int", 12)]
NEW = ("csr_counts", "CSRCounts", "densify")
SPARSE_CALLS = ("count_stats", "size_factors", "poisson_deviance", "deviance_feature_selection", "prepare_counts")
DENSE_RESULT = ("pearson_residuals", "deviance_residuals", "normalize_log1p", "standardize_views")


def _source():
    return open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "counts_sparse.hip")).read()


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,res,n_args", ENTRIES)
def test_the_entries_are_declared_bound_and_defined(name, res, n_args):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpsa_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, f"{name} is not declared in include/gpsa_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == n_args, args
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is (_lib._ll if res == "long long" else _lib._i) and len(argtypes) == n_args
    for a, t in zip(args, argtypes):  # every pointer of these entries is a device pointer
        want = _lib._vp if "*" in a else (_lib._ll if a.startswith("long long") else _lib._i)
        assert t is want, (name, a, t)
    # the section of its own, after "count preprocessing"
    raw = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    assert raw.index("gpsa_standardize_views_f32(const") < raw.index("csrc/counts_sparse.hip") < raw.index(name + "(")
    src = _source()
    assert re.search(r"\b" + res + r"\s+" + name + r"\s*\(", src)
    assert "atomic" not in src.lower()  # comments included
    assert "atomic" not in open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "row_walk.hpp")).read().lower()  # ... and the header the count units share
    assert "defence in depth" in raw.lower()


def test_the_workspace_query_is_pure_and_small():
    lib = _lib.load()
    src = _source()
    const = lambda c: int(re.search(r"constexpr int " + c + r" = (\d+);", src).group(1))
    CT, RM, MG, CB = const("CSR_COL_TILE"), const("CSR_ROWS_MIN"), const("CSR_MAX_GROUPS"), const("CSR_CHECK_BLOCKS")
    for N, P in ((1, 1), (33, 65), (RM * MG, CT), (RM * MG + 1, CT + 1), (4000, 20000), (100000, 20000)):
        R = max(RM, -(-N // MG))
        G, T = -(-N // R), -(-P // CT)
        want = 8 * (2 * G * P + T * N + (T * N + 1) // 2 + G * T + 4 * CB)
        assert lib.gpsa_count_csr_workspace(N, P) == want == lib.gpsa_count_csr_workspace(N, P), (N, P)
    for N, P in ((0, 5), (5, 0), (-1, 5), (0, 0)):
        assert lib.gpsa_count_csr_workspace(N, P) == 0
    # the condition the dense query is held to: below 5 % of the dense matrix's bytes
    assert lib.gpsa_count_csr_workspace(100000, 20000) < 0.05 * 100000 * 20000 * 4
    print(f"[counts sparse] workspace(100000, 20000) = {lib.gpsa_count_csr_workspace(100000, 20000) / 2**20:.1f} MiB, "
          f"workspace(4000, 20000) = {lib.gpsa_count_csr_workspace(4000, 20000) / 2**20:.1f} MiB")


def memory_bound(lib, N, P, n_rows, n_genes):
    """what prepare_counts on a CSR matrix may allocate above its inputs (tests/test_counts_sparse_gpu.py asserts it), in
    bytes, from three terms: the kernels' workspace; the result [n_rows, n_genes] fp32, which is also the gathered block
    (the transforms run in place on it); and 64 (N + P) doubles for everything that is a vector over the rows or the
    genes.  Those vectors, counted in doubles over N + P: two sets of margins (2 x 2), the mask, the row list and log_sz
    by kept and by original row (4 N), the deviance's sums, null term, closing temporaries and result (8 P), the sort's
    values, indices and scratch (6 P), the slot table, the selected block's own margins and the z-score's workspace on
    that block - some 32 in all; 64 leaves the allocator's rounding of each block its room."""
    return lib.gpsa_count_csr_workspace(N, P) + 4 * n_rows * n_genes + 64 * 8 * (N + P)


def test_the_memory_bound_of_the_gpu_test_can_tell_sparse_from_dense():
    lib = _lib.load()
    N, P, G = 4000, 20000, 200
    bound = memory_bound(lib, N, P, N, G)
    dense = 4 * N * P
    print(f"[counts sparse] bound {bound / 2**20:.1f} MiB against the dense matrix's {dense / 2**20:.1f} MiB")
    assert dense == 320_000_000 and dense >= 10 * bound


def test_the_entries_refuse_before_any_launch():
    """the pointers handed in are host memory, which a launch would not survive"""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    need = lib.gpsa_count_csr_workspace(4, 5)
    EINVAL, EWS = _lib.GPSA_EINVAL, _lib.GPSA_EWORKSPACE
    check = lambda crow=p, col=p, val=p, N=4, P=5, nnz=6, out=p, ws=p, nb=need: \
        lib.gpsa_csr_check(crow, col, val, N, P, nnz, out, ws, nb, None)
    shape_kw = (dict(crow=None), dict(col=None), dict(val=None), dict(N=0), dict(P=0), dict(N=-1), dict(P=2**31),
                dict(N=2**31), dict(nnz=-1), dict(nnz=21))
    for kw in shape_kw + (dict(out=None),):
        assert check(**kw) == EINVAL, kw
    assert check(nb=need - 8) == EWS and check(ws=None) == EWS
    margins = lambda crow=p, col=p, val=p, keep=None, N=4, P=5, nnz=6, rs=p, cs=p, rn=p, cn=p, bad=p, ws=p, nb=need: \
        lib.gpsa_count_margins_csr_f32(crow, col, val, keep, N, P, nnz, rs, cs, rn, cn, bad, ws, nb, None)
    for kw in shape_kw + (dict(rs=None), dict(cs=None), dict(rn=None), dict(cn=None), dict(bad=None)):
        assert margins(**kw) == EINVAL, kw
    assert margins(nb=need - 8) == EWS and margins(ws=None) == EWS
    dev = lambda crow=p, col=p, val=p, keep=None, N=4, P=5, nnz=6, ls=p, a=p, b=p, ws=p, nb=need: \
        lib.gpsa_count_deviance_csr_f32(crow, col, val, keep, N, P, nnz, ls, a, b, ws, nb, None)
    for kw in shape_kw + (dict(ls=None), dict(a=None), dict(b=None)):
        assert dev(**kw) == EINVAL, kw
    assert dev(nb=need - 8) == EWS and dev(ws=None) == EWS
    gather = lambda crow=p, col=p, val=p, N=4, P=5, nnz=6, rows=p, n_rows=2, slot=p, G=3, out=p: \
        lib.gpsa_csr_gather_dense_f32(crow, col, val, N, P, nnz, rows, n_rows, slot, G, out, None)
    for kw in shape_kw + (dict(rows=None), dict(slot=None), dict(out=None), dict(n_rows=0), dict(G=0), dict(G=6)):
        assert gather(**kw) == EINVAL, kw


def test_the_custom_ops_propagate_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        crow = torch.empty(701, dtype=i64, device="cuda")
        col, val = torch.empty(900, dtype=i32, device="cuda"), torch.empty(900, dtype=f32, device="cuda")
        keep = torch.empty(700, dtype=torch.bool, device="cuda")
        out = torch.ops.gpsa.csr_check(crow, col, val, 700, 45)
        assert out.shape == (4,) and out.dtype == i64
        rs, cs, rn, cn, bad = torch.ops.gpsa.count_margins_csr(crow, col, val, 700, 45, keep)
        assert (rs.shape, cs.shape, rn.shape, cn.shape, bad.shape) == ((700,), (45,), (700,), (45,), (1,))
        assert (rs.dtype, cs.dtype, rn.dtype, cn.dtype, bad.dtype) == (f64, f64, i64, i64, i64)
        ll, ab = torch.ops.gpsa.count_deviance_csr(crow, col, val, 700, 45, rs)
        assert ll.shape == ab.shape == (45,) and ll.dtype == ab.dtype == f64
        rows, slot = torch.empty(30, dtype=i64, device="cuda"), torch.empty(45, dtype=i32, device="cuda")
        blk = torch.ops.gpsa.csr_gather_dense(crow, col, val, 700, 45, rows, slot, 7)
        assert blk.shape == (30, 7) and blk.dtype == f32


def test_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_meta import demangle, library_kernels

    ks = library_kernels(_lib.LIB_PATH)
    mine = [(n, k) for n, k in zip(demangle([k["name"] for k in ks]), ks) if "gpsa::csr_" in n]
    # the walk and its fold in two modes, the check and its fold, the gather
    assert len(mine) == 2 + 2 + 2 + 1, [n for n, _ in mine]
    for n, k in mine:
        print(f"[counts sparse] {n.split('(')[0]}: {k}")
        assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k)
        assert k["lds"] <= 40 * 1024, (n, k)  # four workgroups per compute unit


def test_exports_and_aliases():
    for name in NEW:
        assert getattr(gpsa, name) is getattr(pkg, name) is getattr(counts, name)
        assert name in pkg.__all__ and name in gpsa.__all__
    from spatial_alignment_amd import ops

    for name in ("csr_check", "count_margins_csr", "count_deviance_csr", "csr_gather_dense"):
        assert callable(getattr(ops.HipOps, name)) and hasattr(torch.ops.gpsa, name)


# ------------------------------------------------------------------------------------------------------------------------
# a fake backend: what csrc/counts_sparse.hip computes, from the yardstick on the densified matrix, on CPU tensors
# ------------------------------------------------------------------------------------------------------------------------
def _to_csr(Y, index=i64, stored_zeros=0):
    """dense numpy -> (crow, col, val) CPU tensors, rows sorted; ``stored_zeros``: that many zeros of row 0 are stored"""
    crow, col, val = [0], [], []
    for i, row in enumerate(Y):
        js = np.nonzero(row)[0]
        if i == 0 and stored_zeros:
            js = np.sort(np.concatenate([js, np.nonzero(row == 0)[0][:stored_zeros]]))
        col += list(js)
        val += list(row[js])
        crow.append(len(col))
    return torch.tensor(crow, dtype=index), torch.tensor(col, dtype=index), torch.tensor(val, dtype=f32)


def _dense_of(crow, col, val, N, P):
    Y = np.zeros((N, P))
    for i in range(N):
        Y[i, col[crow[i]: crow[i + 1]].numpy()] = val[crow[i]: crow[i + 1]].numpy()
    return Y


class FakeSparseOps:
    """the four sparse methods of ops.HipOps by densifying on the host, the dense ones from tests/test_counts.py"""

    def __init__(self):
        from test_counts import FakeCountOps

        self.dense = FakeCountOps()
        self.calls = []

    def __getattr__(self, name):  # count_margins, count_transform, standardize_views
        return getattr(self.dense, name)

    def csr_check(self, crow, col, val, N, P):
        self.calls.append(("check", N, P))
        nnz = col.numel()
        c = crow.numpy()
        n_crow = int(c[0] != 0) + int((np.diff(c) < 0).sum()) + int(c[-1] != nnz)
        n_range = int(((col < 0) | (col >= P)).sum())
        n_order = 0
        for i in range(N):
            a, b = (min(max(int(v), 0), nnz) for v in (c[i], c[i + 1]))
            n_order += int((np.diff(col[a:max(a, b)].numpy()) <= 0).sum())
        return torch.tensor([n_crow, n_range, n_order, int((val == 0).sum())])

    def count_margins_csr(self, crow, col, val, N, P, keep=None):
        Y = _dense_of(crow, col, val, N, P)
        self.calls.append(("margins_csr", N, P, None if keep is None else int(keep.sum())))
        if keep is not None:
            Y[~keep.numpy()] = 0.0
        m = cu.margins(Y)
        return (torch.tensor(m["row_sum"]), torch.tensor(m["col_sum"]), torch.tensor(m["row_nnz"]),
                torch.tensor(m["col_nnz"]), torch.tensor([m["n_invalid"]]))

    def count_deviance_csr(self, crow, col, val, N, P, log_sz, keep=None):
        Y = _dense_of(crow, col, val, N, P)
        self.calls.append(("deviance_csr", N, P, None if keep is None else int(keep.sum())))
        assert tuple(log_sz.shape) == (N,)  # indexed by the original row
        if keep is not None:
            Y[~keep.numpy()] = 0.0
        d = cu.poisson_deviance(Y, log_sz.numpy())
        return torch.tensor(d["ll_sat"]), torch.tensor(d["abs_sat"])

    def csr_gather_dense(self, crow, col, val, N, P, rows, slot, G):
        self.calls.append(("gather", int(rows.numel()), int(G)))
        Y = _dense_of(crow, col, val, N, P)
        out = np.zeros((rows.numel(), G), np.float32)
        genes = np.nonzero(slot.numpy() >= 0)[0]
        out[:, slot.numpy()[genes]] = Y[rows.numpy()][:, genes]
        return torch.tensor(out)


def _pipeline_input():
    Y = cu.recipe(120, 40, seed=5, depth=-1.0)  # a negative depth: sparse
    Y[7] = 0.0       # a spot without counts in view 0
    Y[100] = 0.0     # ... and one in view 2
    Y[50] = Y[50] * 40.0 + 1.0    # a spot far above the rest
    Y[:, 3] = Y[:, 9]  # two genes with the same counts: equal deviances
    return Y, [45, 35, 40]


def _run(Y, ns, index=i64, **kw):
    fake = FakeSparseOps()
    args = dict(min_counts=None, max_counts=None, min_cells=None, n_top_genes=None, transform="pearson", theta=100.0,
                standardize=True)
    args.update(kw)
    crow, col, val = _to_csr(Y, index)
    A = counts._checked(fake, crow.to(i64), col.to(i32), val, Y.shape, "csr_counts")
    before = [t.clone() for t in (A.crow, A.col, A.values)]
    res = counts._prepare(fake, A, ns, **args)
    assert all(torch.equal(a, b) for a, b in zip(before, (A.crow, A.col, A.values)))
    return fake, res, cu.prepare(Y, ns, **args)


@pytest.mark.parametrize("transform", counts.TRANSFORMS)
def test_sparse_prepare_counts_follows_the_yardsticks_pipeline(transform):
    Y, ns = _pipeline_input()
    assert (Y == 0).mean() > 0.5
    kw = dict(min_counts=1, max_counts=float(np.sort(Y.sum(1))[-2]), min_cells=5, n_top_genes=12, transform=transform)
    fake, res, want = _run(Y, ns, **kw)
    assert res.rows.dtype == i64 and res.genes.dtype == i64
    assert np.array_equal(res.rows.numpy(), want["rows"]) and len(want["rows"]) == 117
    assert np.array_equal(res.genes.numpy(), want["genes"]) and len(want["genes"]) == 12
    assert res.n_samples_list == want["n_samples_list"] == [44, 34, 39]
    assert np.abs(res.deviance.numpy() - want["deviance"]).max() <= 1e-9 * np.abs(want["deviance"]).max()
    assert res.outputs.dtype == f32 and tuple(res.outputs.shape) == (117, 12)
    err = np.abs(res.outputs.numpy() - want["outputs"]) / np.maximum(1.0, np.abs(want["outputs"]))
    assert err.max() <= 1e-6, err.max()
    if transform == "counts":
        assert res.log_offset.dtype == f32 and res.n_constant is None
        assert np.abs(res.log_offset.numpy() - want["log_offset"]).max() <= 1e-6
        assert np.array_equal(res.outputs.numpy(), Y[want["rows"]][:, want["genes"]])
    else:
        assert res.log_offset is None and np.array_equal(res.n_constant.numpy(), want["n_constant"])
    # the reads: all rows, the kept rows as a MASK over the same matrix, the deviance under the mask, ONE gather; the
    # dense entries see only the selected block
    assert fake.calls[:5] == [("check", 120, 40), ("margins_csr", 120, 40, None), ("margins_csr", 120, 40, 117),
                              ("deviance_csr", 120, 40, 117), ("gather", 117, 12)]
    assert len(fake.calls) == 5
    assert all(c[2 if c[0] == "transform" else 1] == (117, 12) for c in fake.dense.calls), fake.dense.calls
    tr = [c for c in fake.dense.calls if c[0] == "transform"]
    if transform == "log1p":  # row sums over ALL genes of the kept rows
        rs_all = Y[want["rows"]].sum(1)
        assert np.array_equal(tr[0][3], rs_all) and tr[0][8] == float(np.median(rs_all)) and tr[0][9]
    elif transform != "counts":
        sub = Y[want["rows"]][:, want["genes"]]
        assert np.array_equal(tr[0][3], sub.sum(1)) and np.array_equal(tr[0][4], sub.sum(0)) and tr[0][9]


@pytest.mark.parametrize("index", [i32, i64])
def test_sparse_prepare_counts_without_filters_keeps_everything(index):
    Y = cu.recipe(60, 20, seed=6, depth=-0.5)
    Y[:, 0] += 1.0  # no empty row
    fake, res, want = _run(Y, [30, 30], index=index, transform="deviance", theta=float("inf"), standardize=False)
    assert np.array_equal(res.rows.numpy(), np.arange(60)) and np.array_equal(res.genes.numpy(), np.arange(20))
    assert [c[0] for c in fake.calls] == ["check", "margins_csr", "deviance_csr", "gather"]
    assert fake.calls[2][3] is None  # no mask where no row is dropped
    assert not [c for c in fake.dense.calls if c[0] == "margins"]  # the margins of the whole matrix are the CSR's
    assert np.abs(res.outputs.numpy() - want["outputs"]).max() <= 1e-6 * max(1.0, np.abs(want["outputs"]).max())
    assert res.n_samples_list == [30, 30] and res.n_constant is None


def test_sparse_prepare_counts_refusals_in_the_host_logic():
    Y, ns = _pipeline_input()
    with pytest.raises(ValueError, match=r"2 of 120 rows have no counts.*min_counts"):
        _run(Y, ns)
    Yb = Y.copy()
    Yb[5, 5] = -1.0
    with pytest.raises(ValueError, match="1 entries that are NaN, infinite or negative"):
        _run(Yb, ns, min_counts=1)
    with pytest.raises(ValueError, match="every view needs at least one"):
        _run(Y, ns, min_counts=float(Y[:45].sum(1).max()) + 1)
    with pytest.raises(ValueError, match="no gene passes"):
        _run(Y, ns, min_counts=1, min_cells=1000)


def test_the_check_names_the_rule_and_the_count():
    Y = cu.recipe(12, 9, seed=1, depth=0.0)
    crow, col, val = _to_csr(Y, stored_zeros=2)
    fake = FakeSparseOps()
    A = counts._checked(fake, crow, col.to(i32), val, (12, 9), "csr_counts")
    assert A.n_stored_zeros == 2 and A.nnz == col.numel() and A.shape == (12, 9)
    bad = crow.clone()
    bad[0] = 1
    with pytest.raises(ValueError, match=r"^csr_counts: crow is not a row pointer: 1 violations"):
        counts._checked(fake, bad, col.to(i32), val, (12, 9), "csr_counts")
    c2 = col.clone().to(i32)
    c2[3] = 9
    c2[5] = -1
    with pytest.raises(ValueError, match=r"2 column indices are outside \[0, 9\)"):
        counts._checked(fake, crow, c2, val, (12, 9), "csr_counts")
    c3 = col.clone().to(i32)
    a = int(crow[4])
    assert int(crow[5]) - a >= 2
    c3[a], c3[a + 1] = col[a + 1], col[a]
    with pytest.raises(ValueError, match=r"rows are not sorted / hold duplicates: at 1 places.*sum_duplicates"):
        counts._checked(fake, crow, c3, val, (12, 9), "prepare_counts")


# ------------------------------------------------------------------------------------------------------------------------
# dispatch by argument type and refusals, all before any device work
# ------------------------------------------------------------------------------------------------------------------------
def _cpu_csr(N=40, P=6):
    Y = cu.recipe(N, P, seed=0, depth=0.0)
    crow, col, val = _to_csr(Y)
    return Y, crow, col, val


def test_dispatch_happens_by_argument_type(monkeypatch):
    """a CSRCounts goes to the sparse methods of the backend, a dense tensor to the dense ones"""
    Y, crow, col, val = _cpu_csr()
    Y[:, 0] += 1.0
    crow, col, val = _to_csr(Y)
    fake = FakeSparseOps()
    monkeypatch.setattr(counts, "_ops", lambda: fake)
    monkeypatch.setattr(counts, "_on_device", lambda what, **t: None)
    A = counts.csr_counts((crow, col, val, (40, 6)))
    assert isinstance(A, counts.CSRCounts) and counts.csr_counts(A) is A and A.col.dtype == i32 and A.crow.dtype == i64
    assert A.values.data_ptr() == val.data_ptr() and A.crow.data_ptr() == crow.data_ptr()  # already in type: shared
    m = cu.margins(Y)
    st = counts.count_stats(A)
    assert np.array_equal(st.row_sum.numpy(), m["row_sum"]) and np.array_equal(st.col_nnz.numpy(), m["col_nnz"])
    assert st.total == m["total"] and st.n_invalid == 0
    assert np.allclose(counts.size_factors(A).numpy(), cu.size_factors(Y), rtol=1e-13)
    d = cu.poisson_deviance(Y)
    assert np.allclose(counts.poisson_deviance(A).numpy(), d["deviance"], rtol=1e-12)
    parts = counts.poisson_deviance(A, torch.zeros(40, dtype=f64), return_parts=True)
    assert np.allclose(parts.deviance.numpy(), cu.poisson_deviance(Y, np.zeros(40))["deviance"], rtol=1e-12)
    sel = counts.deviance_feature_selection(A, n_top=3)
    assert np.array_equal(sel.order.numpy(), cu.order(d["deviance"])[:3])
    res = counts.prepare_counts(A, [20, 20], n_top_genes=3, transform="counts")
    assert np.array_equal(res.outputs.numpy(), Y[:, np.sort(cu.order(d["deviance"])[:3])])
    assert not fake.dense.calls and {c[0] for c in fake.calls} == {"check", "margins_csr", "deviance_csr", "gather"}
    # a torch.sparse_csr tensor is checked on entry and takes the same path
    n_checks = [c[0] for c in fake.calls].count("check")
    S = torch.sparse_csr_tensor(crow, col, val, size=(40, 6))
    assert np.array_equal(counts.count_stats(S).col_sum.numpy(), m["col_sum"])
    assert [c[0] for c in fake.calls].count("check") == n_checks + 1
    # densify
    blk = counts.densify(A, rows=[3, 5, 30], genes=[4, 1])
    assert np.array_equal(blk.numpy(), Y[[3, 5, 30]][:, [4, 1]]) and blk.dtype == f32
    assert np.array_equal(counts.densify(A).numpy(), Y)
    # a dense tensor: the dense entries
    fake.calls.clear()
    counts.count_stats(torch.tensor(Y, dtype=f32))
    assert not fake.calls and fake.dense.calls[-1][0] == "margins"


def test_cpu_tensors_are_refused_by_name_of_the_device():
    Y, crow, col, val = _cpu_csr()
    S = torch.sparse_csr_tensor(crow, col, val, size=(40, 6))
    for call in (lambda: counts.csr_counts((crow, col, val, (40, 6))), lambda: counts.csr_counts(S),
                 lambda: counts.count_stats(S), lambda: counts.size_factors(S), lambda: counts.poisson_deviance(S),
                 lambda: counts.deviance_feature_selection(S, 3), lambda: counts.prepare_counts(S, [20, 20]),
                 lambda: counts.densify(S), lambda: counts.densify((crow, col, val, (40, 6)), rows=[1])):
        with pytest.raises(ValueError, match="device 'cpu'"):
            call()


def test_sparse_input_to_the_dense_result_calls_is_refused_by_name():
    Y, crow, col, val = _cpu_csr()
    A = counts.CSRCounts(crow, col.to(i32), val, (40, 6))
    S = torch.sparse_csr_tensor(crow, col, val, size=(40, 6))
    for Ysp in (A, S):
        for name, call in (("pearson_residuals", lambda y: counts.pearson_residuals(y)),
                           ("deviance_residuals", lambda y: counts.deviance_residuals(y, 10.0)),
                           ("normalize_log1p", lambda y: counts.normalize_log1p(y)),
                           ("standardize_views", lambda y: counts.standardize_views(y, [20, 20]))):
            with pytest.raises(ValueError, match=rf"^{name}: Y is sparse.*prepare_counts.*densify"):
                call(Ysp)
    assert tuple(DENSE_RESULT) == ("pearson_residuals", "deviance_residuals", "normalize_log1p", "standardize_views")


def test_the_tuple_form_is_checked_on_the_host():
    Y, crow, col, val = _cpu_csr()
    ok = (crow, col, val, (40, 6))
    for bad, match in (((crow[:-1], col, val, (40, 6)), r"crow has 40 entries.*N \+ 1 = 41"),
                       ((crow, col[:-1], val, (40, 6)), "nnz differs"),
                       ((crow, col, val[:-2], (40, 6)), "nnz differs"),
                       ((crow, col, val, (40,)), "shape"), ((crow, col, val, (0, 6)), "shape"),
                       ((crow, col, val, (40, 2**31)), "shape"), ((crow, col, val, "ab"), "shape"),
                       ((crow.double(), col, val, (40, 6)), "crow has dtype torch.float64.*int32 and int64"),
                       ((crow, col.to(torch.int16), val, (40, 6)), "col has dtype torch.int16"),
                       ((crow, col, val > 0, (40, 6)), "values has dtype torch.bool"),
                       ((crow, col.view(-1, 1), val, (40, 6)), "col must be a 1-D tensor"),
                       ((crow, col.numpy(), val, (40, 6)), "col must be a 1-D tensor"),
                       ((torch.arange(3), torch.zeros(9, dtype=i64), torch.ones(9), (2, 4)), "more than N \\* P"),
                       ((crow, col, val), "CSRCounts is needed"), (np.zeros((3, 3)), "CSRCounts is needed"),
                       (torch.eye(3).to_sparse(), "layout torch.sparse_csr.*to_sparse_csr")):
        with pytest.raises(ValueError, match=r"^csr_counts: .*" + match):
            counts.csr_counts(bad)
    with pytest.raises(ValueError, match="device is for scipy input"):
        counts.csr_counts(ok, device="cuda")
    for ns in ([20, 19], [], None):
        with pytest.raises(ValueError, match="n_samples_list"):
            counts.prepare_counts(counts.CSRCounts(crow, col.to(i32), val, (40, 6)), ns)
    with pytest.raises(ValueError, match="log_sz"):
        counts.poisson_deviance(counts.CSRCounts(crow, col.to(i32), val, (40, 6)), torch.zeros(39, dtype=f64))
    with pytest.raises(ValueError, match="n_top"):
        counts.deviance_feature_selection(counts.CSRCounts(crow, col.to(i32), val, (40, 6)), n_top=7)


def test_scipy_input_is_canonicalised_like_scipys_own(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(3)
    r, c = rng.integers(0, 30, 400), rng.integers(0, 17, 400)  # duplicates, no order
    v = rng.integers(1, 5, 400).astype(np.float64)
    coo = sp.coo_matrix((v, (r, c)), shape=(30, 17))
    want = coo.tocsr()
    want.sum_duplicates()
    want.sort_indices()
    with pytest.raises(ValueError, match="device 'cpu'"):
        counts.csr_counts(coo, device="cpu")
    fake = FakeSparseOps()
    monkeypatch.setattr(counts, "_ops", lambda: fake)
    monkeypatch.setattr(counts, "_upload_device", lambda device, what: torch.device("cpu"))  # for this test only
    for m in (coo, coo.tocsc(), coo.tolil()):
        A = counts.csr_counts(m)
        assert A.shape == (30, 17) and A.nnz == want.nnz < 400
        assert A.crow.dtype == i64 and A.col.dtype == i32 and A.values.dtype == f32
        assert np.array_equal(A.crow.numpy(), want.indptr) and np.array_equal(A.col.numpy(), want.indices)
        assert np.array_equal(A.values.numpy(), want.data)
    assert coo.nnz == 400  # the caller's matrix is not modified
