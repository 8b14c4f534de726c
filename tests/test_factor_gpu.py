"""The batched fp64 factorisations of csrc/linalg.hip, through the C ABI alone, against a longdouble reference at the edges of
their kernel classes:

  A. gpsa_chol_inv_f64 (the panel kernel chol_inv_blk_kernel<NT> up to M = 208, chol_inv_reg_kernel<NT, 32> above) and
     gpsa_chol_inv_blocked_f64 on one diagonal block (chol_inv_reg_kernel<NT, 16> / <NT, 32>);
  B. gpsa_chol_inv_blocked_f64 beyond 256 columns (two and three diagonal blocks, the fp64-MFMA products between them);
  C. gpsa_chol_f64 and gpsa_tri_inv_f64 (packed in LDS up to M = 200, in global memory above);
  D. gpsa_chol_inv_sel_f64's selection arithmetic; refusals of every entry;
  E. info and logdet on indefinite and NaN inputs, the lower-triangle contract;
  F. gpsa_bdot and gpsa_add_diag.

References, bounds, input families and shape lists: tests/factor_util.py (bounds derived element by element, nothing tuned
to the kernels).  Every bound check prints its worst error / bound and asserts <= 1.

Guards, as in tests/test_fp64_products_gpu.py: every output (info too, in an int32 frame) is a view inside a
sentinel-filled buffer that must stay intact on both sides, every workspace is exactly the queried size and filled with 0xFF,
results are NaN-free where info = 0, inputs of the fused entries are not modified, every call runs twice and must be equal
bit for bit.  Nothing skips: which kernel a shape takes is read from the launchers ("factorisation tests") and
held by tests/test_factor_shapes.py without a GPU.
"""
import math

import pytest
import torch

import factor_util as fu
from fp64_products_util import (EINVAL, EUNSUPPORTED, EWORKSPACE, SENTINEL, Guarded, bar, f32, f64, poisoned, ratio, rnd,
                                same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = 0, 1  # GPSA_F32 / GPSA_F64


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    return _lib.load()


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def note(what, r):
    print(f"[factor] {what}: error / bound {r:.3f}")
    return r


def twice(call):
    """run call() -> tuple of result tensors twice; the two must be equal bit for bit"""
    a, b = call(), call()
    for x, y in zip(a, b):
        assert same_bits(x, y), "not repeatable"
    return a


def fused_raw(lib, entry, Ad, short=0, sel=None):
    """one call of a fused entry on the device batch Ad into framed outputs -> rc, X, logdet, info (Guarded)"""
    B, M = Ad.shape[0], Ad.shape[-1]
    X, ld, info = Guarded(B * M * M, f64, DEV), Guarded(B, f64, DEV), fu.GuardedInt(B, DEV)
    if entry == "inv":
        rc = lib.gpsa_chol_inv_f64(Ad.data_ptr(), X.ptr(), M, B, ld.ptr(), info.ptr(), stream())
    elif entry == "sel":  # (the whole batch unless told otherwise: one always-matrix and the range [1, B))
        na, lo, hi = sel if sel is not None else (1, 1, B)
        rc = lib.gpsa_chol_inv_sel_f64(Ad.data_ptr(), X.ptr(), M, B, na, lo, hi, ld.ptr(), info.ptr(), stream())
    else:
        nbytes = int(lib.gpsa_chol_inv_blocked_workspace(M, B)) - short
        ws = poisoned(nbytes, DEV)
        rc = lib.gpsa_chol_inv_blocked_f64(Ad.data_ptr(), X.ptr(), M, B, ld.ptr(), info.ptr(), ws.data_ptr(), nbytes,
                                           stream())
    torch.cuda.synchronize()
    return rc, X, ld, info


def run(lib, entry, A):
    """entry on the CPU batch A [B, M, M], twice -> (X or L, logdet, info) on the CPU; frames intact, input unchanged"""
    B, M = A.shape[0], A.shape[-1]
    Ad = A.to(DEV).contiguous()
    keep = Ad.clone()

    def call():
        if entry == "chol":  # in place: the frame goes around the matrices themselves
            X, ld, info = Guarded(B * M * M, f64, DEV), Guarded(B, f64, DEV), fu.GuardedInt(B, DEV)
            X.view.copy_(Ad.reshape(-1))
            rc = lib.gpsa_chol_f64(X.ptr(), M, B, ld.ptr(), info.ptr(), stream())
            torch.cuda.synchronize()
        else:
            rc, X, ld, info = fused_raw(lib, entry, Ad)
        assert rc == 0 and X.intact() and ld.intact() and info.intact(), (entry, M, B, rc)
        return X.view.view(B, M, M), ld.view, info.view

    out = twice(call)
    assert same_bits(Ad, keep), "the input was modified"
    return tuple(t.cpu() for t in out)


def good(entry, name, M, k, out, ld, info):
    """matrix k of a family came out as `out`: info = 0 and every bound -> the largest error / bound"""
    assert int(info) == 0, (entry, name, M, k, int(info))
    ref = fu.reference(name, M, k)
    rx = fu.chol_residual_ratio(out, ref.A) if entry == "chol" else fu.x_ratio(out, ref)
    rl = fu.logdet_ratio(ld, ref)
    assert rx <= 1 and rl <= 1, (entry, name, M, k, rx, rl)
    return max(rx, rl)


# ------------------------------------------------------------------------------------------------------------------------
# A. one diagonal block: every class of the panel kernel and of the register kernel with TS = 16 and 32
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", fu.FUSED_M)
@pytest.mark.parametrize("name", fu.FAMILIES)
def test_fused_classes(lib, name, M):
    """gpsa_chol_inv_f64 and gpsa_chol_inv_blocked_f64 at the first, last and a ragged M of every kernel class, batch 3;
    the two agree within the sum of their bounds"""
    ks = (0, 1, 2)
    A = fu.batch_of(name, M, ks)
    res = {e: run(lib, e, A) for e in ("inv", "blocked")}
    for e, (X, ld, info) in res.items():
        note(f"{e} {name} M = {M}", max(good(e, name, M, k, X[b], ld[b], info[b]) for b, k in enumerate(ks)))
    for b, k in enumerate(ks):
        ref = fu.reference(name, M, k)
        assert ratio(res["inv"][0][b], res["blocked"][0][b], torch.from_numpy(2.0 * ref.bX)) <= 1
        assert abs(float(res["inv"][1][b]) - float(res["blocked"][1][b])) <= 2.0 * ref.bld


def test_more_workgroups_than_compute_units(lib):
    M, B = 20, 300
    A = fu.batch_of("wishart", M, range(B))
    X, ld, info = run(lib, "inv", A)
    note(f"inv wishart M = {M}, batch {B}", max(good("inv", "wishart", M, k, X[k], ld[k], info[k]) for k in range(B)))


# ------------------------------------------------------------------------------------------------------------------------
# B. beyond 256 columns
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", list(fu.BLOCKED_BIG))
@pytest.mark.parametrize("name", fu.FAMILIES)
def test_blocked_beyond_256(lib, name, M):
    """two and three diagonal blocks, batch 3 (the [batch][bs][M] stride of the T scratch) and batch 1"""
    ks = (0, 1, 2)
    X, ld, info = run(lib, "blocked", fu.batch_of(name, M, ks))
    note(f"blocked {name} M = {M}, batch 3", max(good("blocked", name, M, k, X[b], ld[b], info[b]) for b, k in enumerate(ks)))
    if name == "wishart":
        X, ld, info = run(lib, "blocked", fu.batch_of(name, M, (0,)))
        note(f"blocked {name} M = {M}, batch 1", good("blocked", name, M, 0, X[0], ld[0], info[0]))


@pytest.mark.parametrize("M,B", [(100, 3), (257, 1), (513, 3)])
def test_blocked_workspace_one_byte_short(lib, M, B):
    rc, X, ld, info = fused_raw(lib, "blocked", fu.batch_of("wishart", M, range(B)).to(DEV), short=1)
    assert rc == EWORKSPACE and X.untouched() and ld.untouched() and info.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# C. the unfused pair
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1] + fu.UNFUSED_M)
@pytest.mark.parametrize("name", fu.FAMILIES)
def test_chol(lib, name, M):
    """gpsa_chol_f64 in place: packed / global at 199, 200, 201 and the sizes of the inverse's column passes"""
    ks = (0, 1, 2)
    L, ld, info = run(lib, "chol", fu.batch_of(name, M, ks))
    note(f"chol {name} M = {M}", max(good("chol", name, M, k, L[b], ld[b], info[b]) for b, k in enumerate(ks)))


def _tri_inv(lib, L):
    B, M = L.shape[0], L.shape[-1]
    Ld = L.to(DEV).contiguous()
    keep = Ld.clone()

    def call():
        X = Guarded(B * M * M, f64, DEV)
        rc = lib.gpsa_tri_inv_f64(Ld.data_ptr(), X.ptr(), M, B, stream())
        torch.cuda.synchronize()
        assert rc == 0 and X.intact()
        return (X.view.view(B, M, M),)

    (X,) = twice(call)
    assert same_bits(Ld, keep)
    return X.cpu()


@pytest.mark.parametrize("M", [1] + fu.UNFUSED_M)
@pytest.mark.parametrize("name", fu.TRI_FAMILIES)
def test_tri_inv(lib, name, M):
    """gpsa_tri_inv_f64 of an exact triangular input; the last row has M - 1 columns in passes of 256: 255, 256 (one full
    pass), 257 (a second pass of one column), 512 (two full passes)"""
    ks = (0, 1, 2)
    L = fu.batch_of(name, M, ks)
    X = _tri_inv(lib, L)
    r = note(f"tri_inv {name} M = {M}", max(fu.tri_inv_residual_ratio(X[b], L[b]) for b in range(len(ks))))
    assert r <= 1


def test_chol_beyond_one_trip_of_the_strided_loops(lib):
    """M = 1030 > LA_THREADS + 1, batch 1: the column scaling and the diagonal copy take a second trip (residual in fp64)"""
    M = fu.UNFUSED_LONG_M
    A = fu.batch_of("wishart", M, (0,))
    L, ld, info = run(lib, "chol", A)
    assert int(info[0]) == 0 and math.isfinite(float(ld[0]))
    assert note(f"chol wishart M = {M}", fu.chol_residual_ratio(L[0], A[0])) <= 1
    assert float(ld[0]) == pytest.approx(2.0 * float(torch.log(torch.diagonal(L[0])).sum()), rel=1e-13)


def test_tri_inv_beyond_one_trip_of_the_strided_loops(lib):
    """M = 1030: rowL is filled in two trips, five column passes"""
    M = fu.UNFUSED_LONG_M
    L = fu.batch_of("tri", M, (0,))
    X = _tri_inv(lib, L)
    assert note(f"tri_inv tri M = {M}", fu.tri_inv_residual_ratio(X[0], L[0])) <= 1


# ------------------------------------------------------------------------------------------------------------------------
# D. refusals; the selection
# ------------------------------------------------------------------------------------------------------------------------
def test_unsupported_sizes_write_nothing(lib):
    """M = 257 on the register-resident entries, M = 4097 on the unfused pair: refused before any launch"""
    M, B = 257, 2
    Ad = fu.batch_of("wishart", M, range(B)).to(DEV)
    for entry in ("inv", "sel"):
        rc, X, ld, info = fused_raw(lib, entry, Ad)
        assert rc == EUNSUPPORTED and X.untouched() and ld.untouched() and info.untouched(), entry
    M = fu.LA_GLOBAL_MAX + 1
    A, X, ld, info = Guarded(M * M, f64, DEV), Guarded(M * M, f64, DEV), Guarded(1, f64, DEV), fu.GuardedInt(1, DEV)
    assert lib.gpsa_chol_f64(A.ptr(), M, 1, ld.ptr(), info.ptr(), stream()) == EUNSUPPORTED
    assert lib.gpsa_tri_inv_f64(A.ptr(), X.ptr(), M, 1, stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert A.untouched() and X.untouched() and ld.untouched() and info.untouched()


@pytest.mark.parametrize("M,B", [(0, 2), (-1, 2), (8, 0), (8, -3)])
def test_invalid_sizes_write_nothing(lib, M, B):
    A, X, ld, info = Guarded(256, f64, DEV), Guarded(256, f64, DEV), Guarded(4, f64, DEV), fu.GuardedInt(4, DEV)
    ws = poisoned(4096, DEV)
    st = stream()
    rcs = [lib.gpsa_chol_f64(A.ptr(), M, B, ld.ptr(), info.ptr(), st),
           lib.gpsa_tri_inv_f64(A.ptr(), X.ptr(), M, B, st),
           lib.gpsa_chol_inv_f64(A.ptr(), X.ptr(), M, B, ld.ptr(), info.ptr(), st),
           lib.gpsa_chol_inv_sel_f64(A.ptr(), X.ptr(), M, B, 0, 0, 1, ld.ptr(), info.ptr(), st),
           lib.gpsa_chol_inv_blocked_f64(A.ptr(), X.ptr(), M, B, ld.ptr(), info.ptr(), ws.data_ptr(), 4096, st),
           lib.gpsa_bdot(F64, A.ptr(), 1, X.ptr(), 1, M, B, ld.ptr(), ws.data_ptr(), 4096, st),
           lib.gpsa_add_diag(F64, A.ptr(), M, B, 1.0, st)]
    torch.cuda.synchronize()
    assert rcs == [EINVAL] * len(rcs)
    assert A.untouched() and X.untouched() and ld.untouched() and info.untouched() and bool((ws == 0xFF).all())
    assert int(lib.gpsa_chol_inv_blocked_workspace(M, B)) == 0


SEL = [(0, 3, 3), (0, 4, 2), (2, 0, 4), (1, 4, 99), (2, 5, 3), (6, 0, 0), (6, 2, 4), (0, -5, 2), (1, 3, 5)]


@pytest.mark.parametrize("M", [200, 240])
def test_selection_edges(lib, M):
    """gpsa_chol_inv_sel_f64: an empty selection touches nothing, keep_lo < n_always and keep_hi > batch are clipped,
    keep_hi < keep_lo selects the always-matrices alone, n_always = batch selects all; panel (200) and register (240)
    kernel.  Selected results equal the full call's bit for bit, the rest keeps its sentinel"""
    B = 6
    A = fu.batch_of("wishart", M, range(B))
    Ad = A.to(DEV)
    full = run(lib, "inv", A)
    for na, lo, hi in SEL:
        lo_c = max(lo, na)
        hi_c = max(min(hi, B), lo_c)
        sel = [b for b in range(B) if b < na or lo_c <= b < hi_c]
        rc, X, ld, info = fused_raw(lib, "sel", Ad, sel=(na, lo, hi))
        assert rc == 0 and X.intact() and ld.intact() and info.intact(), (na, lo, hi)
        if not sel:
            assert X.untouched() and ld.untouched() and info.untouched()
        Xv = X.view.view(B, M, M).cpu()
        for b in range(B):
            if b in sel:
                assert same_bits(Xv[b], full[0][b]) and same_bits(ld.view[b].cpu(), full[1][b]), (na, lo, hi, b)
                assert int(info.view[b]) == 0
            else:
                assert bool((Xv[b] == SENTINEL).all()) and float(ld.view[b]) == SENTINEL, (na, lo, hi, b)
                assert int(info.view[b]) == fu.ISENTINEL
    for na in (B + 1, -1):
        rc, X, ld, info = fused_raw(lib, "sel", Ad, sel=(na, 0, B))
        assert rc == EINVAL and X.untouched() and ld.untouched() and info.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# E. info and logdet
# ------------------------------------------------------------------------------------------------------------------------
CLASS_M = [17, 64, 100, 160, 208, 224, 241]  # one M of every panel class and of both TS = 32 classes, ragged and full
BAD = ([(e, M) for e in ("inv", "blocked") for M in CLASS_M] + [("blocked", M) for M in (257, 417, 513)]
       + [("sel", 200), ("sel", 240), ("chol", 17), ("chol", 199), ("chol", 201)])


def _block_edges(lib, M):
    bs = fu.block_size_from_workspace(int(lib.gpsa_chol_inv_blocked_workspace(M, 1)), M, 1)
    return sorted({c for o in range(0, M, bs) for c in (o, min(o + bs, M) - 1)})


@pytest.mark.parametrize("entry,M", BAD)
def test_one_bad_pivot(lib, entry, M):
    """pivot j made negative in one matrix each (j = 0, 15, 16, M - 1 and the first and last column of every diagonal
    block): info = what LAPACK reports, logdet NaN; the good matrices at both ends of the batch still meet their bounds"""
    js = sorted({j for j in (0, 15, 16, M - 1) if j < M} | (set(_block_edges(lib, M)) if entry == "blocked" else set()))
    mats = [fu.matrix("wishart", M, 0)] + [fu.bad_pivot("wishart", M, 0, j) for j in js] + [fu.matrix("wishart", M, 1)]
    A = torch.stack(mats).contiguous()
    want = fu.want_info(A)
    assert want.tolist() == [0] + [j + 1 for j in js] + [0]  # (the construction does what it says)
    out, ld, info = run(lib, entry, A)
    assert info.tolist() == want.tolist(), (entry, M, js)
    assert bool(torch.isnan(ld[1:-1]).all())
    note(f"{entry} wishart M = {M} next to {len(js)} indefinite matrices",
         max(good(entry, "wishart", M, 0, out[0], ld[0], info[0]), good(entry, "wishart", M, 1, out[-1], ld[-1], info[-1])))


FIRST = [("inv", 100, 3, 9), ("inv", 100, 5, 40), ("inv", 100, 15, 16), ("inv", 240, 3, 9), ("inv", 240, 5, 200),
         ("blocked", 100, 3, 9), ("blocked", 240, 31, 32), ("blocked", 513, 3, 400), ("blocked", 513, 180, 190),
         ("blocked", 513, 175, 512), ("sel", 200, 20, 25), ("chol", 199, 3, 9), ("chol", 201, 3, 9)]


@pytest.mark.parametrize("entry,M,j1,j2", FIRST)
def test_first_bad_pivot_wins(lib, entry, M, j1, j2):
    """diagonal matrices with two non-positive entries (negative, and an exact zero): inside one 16-column block (the
    LDL^T block records and goes on), in two panels, in two diagonal blocks of the blocked driver (its accumulate path)"""
    d = 1.0 + rnd(M, seed=M).abs()
    rows = []
    for v1, v2 in ((-1.5, -2.5), (0.0, -2.5), (None, 0.0), (None, -0.5), (None, None)):
        e = d.clone()
        if v1 is not None:
            e[j1] = v1
        if v2 is not None:
            e[j2] = v2
        rows.append(torch.diag(e))
    A = torch.stack(rows).contiguous()
    want = fu.want_info(A)
    assert want.tolist() == [j1 + 1, j1 + 1, j2 + 1, j2 + 1, 0]
    out, ld, info = run(lib, entry, A)
    assert info.tolist() == want.tolist(), (entry, M, j1, j2, info.tolist())
    assert bool(torch.isnan(ld[:4]).all())
    # the good one: L = diag(sqrt(d)), a square root (or a refined reciprocal square root) per entry, M logs
    wantd = torch.diag(d.sqrt() if entry == "chol" else 1.0 / d.sqrt())
    rl = abs(float(ld[4]) - float(d.log().sum())) / (fu.gfac(M) * float(d.log().abs().sum()))
    assert note(f"{entry} diagonal M = {M} next to four indefinite matrices",
                max(ratio(out[4], wantd, fu.gfac(M) * wantd.abs()), rl)) <= 1


NAN_AT = [("inv", 100, 12, 3), ("inv", 100, 40, 7), ("inv", 240, 200, 5), ("blocked", 100, 40, 7), ("blocked", 513, 100, 20),
          ("blocked", 513, 300, 7), ("sel", 200, 199, 0), ("chol", 199, 40, 7), ("chol", 201, 40, 7)]


@pytest.mark.parametrize("entry,M,i,j", NAN_AT)
def test_nan_below_the_diagonal(lib, entry, M, i, j):
    """a NaN at (i, j), j < i, reaches pivot i: info = i + 1 as LAPACK reports it; the neighbours are unaffected"""
    A = fu.batch_of("wishart", M, (0, 0, 1))
    A[1, i, j] = float("nan")
    want = fu.want_info(A)
    assert want.tolist() == [0, i + 1, 0]
    out, ld, info = run(lib, entry, A)
    assert info.tolist() == want.tolist() and math.isnan(float(ld[1]))
    note(f"{entry} wishart M = {M} next to a NaN input",
         max(good(entry, "wishart", M, 0, out[0], ld[0], info[0]), good(entry, "wishart", M, 1, out[2], ld[2], info[2])))


@pytest.mark.parametrize("entry,M", [("inv", 17), ("inv", 100), ("inv", 200), ("inv", 241), ("blocked", 100),
                                     ("blocked", 241), ("blocked", 257), ("blocked", 513), ("sel", 200), ("sel", 240),
                                     ("chol", 17), ("chol", 199), ("chol", 201)])
def test_only_the_lower_triangle_is_read(lib, entry, M):
    """NaN in the strict upper triangle of the input changes no bit of any result"""
    A = fu.batch_of("rbf" if M % 2 else "wishart", M, (0, 1))
    a = run(lib, entry, A)
    b = run(lib, entry, fu.nan_above(A))
    assert all(same_bits(x, y) for x, y in zip(a, b)) and a[2].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------------------
# F. gpsa_bdot, gpsa_add_diag
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fu.BDOT_N)
@pytest.mark.parametrize("dtype", [f32, f64])
def test_bdot(lib, dtype, n):
    """out[b] = sum_i A[b, i] B[b, i] in fp64 whatever the storage: the split count's edges and its cap, one block of the
    finish kernel and one thread more, padded rows and broadcast operands; workspace of the documented size, poisoned"""
    code = F32 if dtype == f32 else F64
    worst = 0.0
    pool_a, pool_b = rnd(65 * (n + 5), dtype=dtype, seed=n), rnd(65 * (n + 5), dtype=dtype, seed=n + 1)
    pa, pb = pool_a.to(DEV), pool_b.to(DEV)
    for B in fu.BDOT_BATCH:
        for sa, sb in ((n, n), (n + 5, n + 5), (0, n), (n + 5, 0)):
            rows_a = torch.stack([pool_a[b * sa: b * sa + n] for b in range(B)]).double()
            rows_b = torch.stack([pool_b[b * sb: b * sb + n] for b in range(B)]).double()
            want = (rows_a * rows_b).sum(1)
            bound = bar(n, (rows_a * rows_b).abs().sum(1), want32=want if dtype == f32 else None)
            nbytes = 8 * fu.BDOT_MAX_SPLITS * B

            def call():
                out, ws = Guarded(B, dtype, DEV), poisoned(nbytes, DEV)
                rc = lib.gpsa_bdot(code, pa.data_ptr(), sa, pb.data_ptr(), sb, n, B, out.ptr(), ws.data_ptr(), nbytes,
                                   stream())
                torch.cuda.synchronize()
                assert rc == 0 and out.intact(), (n, B, sa, sb, rc)
                return (out.view,)

            (out,) = twice(call)
            r = ratio(out, want, bound)
            assert r <= 1, (dtype, n, B, sa, sb, r)
            worst = max(worst, r)
    note(f"bdot {dtype} n = {n}", worst)


@pytest.mark.parametrize("n", [1, 2049, 65537])
def test_bdot_workspace_is_what_the_header_says(lib, n):
    """8 * min(32, ceil(n / 2048)) * batch bytes are taken, one element less is refused with nothing written"""
    B, ns = 3, fu.bdot_splits(n)
    a = rnd(B * n, seed=n).to(DEV)
    for nbytes, want_rc in ((8 * ns * B, 0), (8 * ns * B - 8, EWORKSPACE), (8 * ns * B - 1, EWORKSPACE)):
        out, ws = Guarded(B, f64, DEV), poisoned(max(nbytes, 8), DEV)
        rc = lib.gpsa_bdot(F64, a.data_ptr(), n, a.data_ptr(), n, n, B, out.ptr(), ws.data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        assert rc == want_rc and out.intact()
        if want_rc:
            assert out.untouched() and bool((ws == 0xFF).all())
        else:
            sq = a.view(B, n).cpu() ** 2
            assert note(f"bdot n = {n}, workspace of {nbytes} bytes", ratio(out.view, sq.sum(1), bar(n, sq.sum(1)))) <= 1


@pytest.mark.parametrize("M,B", fu.ADD_DIAG)
@pytest.mark.parametrize("dtype", [f32, f64])
def test_add_diag(lib, dtype, M, B):
    """A[b] += s I: the diagonal is fl(a + s) exactly (s rounded to fp32 first for fp32 storage), every other entry and
    the frame keep their bits; M * batch on both sides of one block of 256 threads"""
    A = rnd(B, M, M, dtype=dtype, seed=M + B)
    for s in (0.1, -3.7):
        want = A.clone()
        sv = torch.tensor(s, dtype=f64).to(dtype)
        idx = torch.arange(M)
        want[:, idx, idx] = A[:, idx, idx] + sv

        def call():
            G = Guarded(B * M * M, dtype, DEV)
            G.view.copy_(A.reshape(-1))
            rc = lib.gpsa_add_diag(F32 if dtype == f32 else F64, G.ptr(), M, B, s, stream())
            torch.cuda.synchronize()
            assert rc == 0 and G.intact()
            return (G.view.view(B, M, M),)

        (got,) = twice(call)
        assert same_bits(got.cpu(), want), (dtype, M, B, s)
