"""The kernels that build a step's M x M stage, through the C ABI alone, against a plain reference of the same operation
at the edges of their grids and dispatch:

  A. the covariance matrices (csrc/kmat.hip: gpsa_kmat, gpsa_kmat_batched);
  B. their backward in every entry (generic kernel with 8- and 32-row chunks and the column-block walk, the D = 2
     register kernel, the finish kernel's unrolled loop, the batched and the two-piece forms);
  C. Omega = A A^T + jitter I and its adjoint (csrc/gemm.hip, the LDS-DMA kernels of csrc/qf_big.hip and their fallback);
  D. the KL terms (csrc/kl.hip), the sliced forward of the step among them.

References and bounds: tests/mm_stage_util.py (longdouble for the covariance family, fp64 torch on the CPU otherwise;
bounds derived from the arithmetic, element by element).  Every check prints its worst error / bound and asserts <= 1.

Guards, as in tests/test_fp64_products_gpu.py: every output is a view inside a sentinel-filled buffer that must stay
intact on both sides, every workspace is exactly the queried size and filled with 0xFF bytes, results are NaN-free (ratio()
returns inf otherwise), every call runs twice and must be equal bit for bit.  Nothing skips: which branch a shape takes is
read from the launchers ("M x M stage tests") and held by tests/test_mm_stage_shapes.py without a GPU.
"""
import ctypes as C

import pytest
import torch

import mm_stage_util as mu
from fp64_products_util import EINVAL, EWORKSPACE, U32, U64, Guarded, bar, f32, f64, poisoned, ratio, rnd, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    assert int(torch.cuda.get_device_properties(0).multi_processor_count) == mu.CUS, "dispatch claims assume 256 CUs"
    return _lib.load()


def stream():
    return torch._C._cuda_getCurrentRawStream(0)


def note(family, what, r):
    print(f"[mm-stage] {family}: {what}: error / bound {r:.3f}")
    return r


def p(t):
    return 0 if t is None else t.data_ptr()


def lls(xs):
    return (C.c_longlong * len(xs))(*[int(x) for x in xs])


def check(family, what, got, want, bound):
    r = note(family, what, ratio(got, want.reshape(got.shape), bound.reshape(got.shape)))
    assert r <= 1, (what, r)
    return r


def twice(call):
    """run call() -> tuple of result tensors twice; the two must be equal bit for bit"""
    a, b = call(), call()
    for x, y in zip(a, b):
        assert (x is None and y is None) or same_bits(x, y), "not repeatable"
    return a


# ------------------------------------------------------------------------------------------------------------------------
# A. covariance forward
# ------------------------------------------------------------------------------------------------------------------------
def _fwd_inputs(M, Cn, D, zdt, xdt, seed):
    Z, X = mu.points(M, D, zdt, seed), mu.points(Cn, D, xdt, seed + 1)
    n = min(M, Cn)
    X[:n] = Z[:n].to(xdt)  # the diagonal pairs coincide: k = var there, and a missing or doubled jitter cannot hide
    ls, lv = mu.hyper(zdt, seed=seed)
    return Z, X, ls, lv


@pytest.mark.parametrize("types", list(mu.FWD_TYPES))
@pytest.mark.parametrize("kind", list(mu.KINDS))
def test_kmat_fwd(lib, kind, types):
    """gpsa_kmat: M in {1, 15, 16, 17, 33} x C in {1, 255, 256, 257, 513} x D in 1..4; jitter 1e-5 on exactly the
    min(M, C) main-diagonal entries (the bound off the diagonal has no room for it)"""
    dtc, itc, zdt, xdt, kdt = mu.FWD_TYPES[types]
    u = U32 if kdt == f32 else U64
    worst = 0.0
    for M in mu.FWD_M:
        for Cn in mu.FWD_C:
            for D in mu.FWD_D:
                Z, X, ls, lv = _fwd_inputs(M, Cn, D, zdt, xdt, 100 * M + Cn + D)
                want, bound, amax = mu.cov_fwd_ref(kind, Z, X, ls[0], lv[0], mu.JITTER, u)
                assert amax <= mu.A_MAX
                Zd, Xd, lsd, lvd = Z.to(DEV), X.to(DEV), ls.to(DEV), lv.to(DEV)

                def call():
                    K = Guarded(M * Cn, kdt, DEV)
                    rc = lib.gpsa_kmat(dtc, itc, mu.KINDS[kind], p(Zd), M, p(Xd), Cn, D, p(lsd), p(lvd), mu.JITTER, K.ptr(),
                                       stream())
                    torch.cuda.synchronize()
                    assert rc == 0 and K.intact(), (M, Cn, D, rc)
                    return (K.view,)

                (K,) = twice(call)
                r = ratio(K, want.reshape(-1), bound.reshape(-1))
                assert r <= 1, (kind, types, M, Cn, D, r)
                worst = max(worst, r)
    note("kmat", f"gpsa_kmat {kind} {types}, 100 shapes", worst)


@pytest.mark.parametrize("kind", list(mu.KINDS))
def test_kmat_fwd_batched(lib, kind):
    """gpsa_kmat_batched: one problem per n_live in {0, 1, 255, 256, 257, C} with exact zeros beyond it, parameter
    stride 1; then every column live (n_live = NULL)"""
    for M, Cn, D in mu.FWD_BATCHED:
        for ragged in (True, False):
            live = mu.fwd_n_live(Cn)
            B = len(live)
            Z = torch.stack([mu.points(M, D, f32, 7 * b + M) for b in range(B)])
            X = torch.stack([mu.points(Cn, D, f32, 11 * b + Cn) for b in range(B)])
            n = min(M, Cn)
            X[:, :n] = Z[:, :n]
            ls, lv = mu.hyper(f32, n=B, seed=M)
            refs = [mu.cov_fwd_ref(kind, Z[b], X[b], ls[b], lv[b], mu.JITTER, U64, live[b] if ragged else None)
                    for b in range(B)]
            assert max(r[2] for r in refs) <= mu.A_MAX
            want, bound = torch.stack([r[0] for r in refs]), torch.stack([r[1] for r in refs])
            if ragged:
                assert all(bool((bound[b][:, live[b]:] == 0).all()) for b in range(B))  # zeros beyond n_live are exact
            Zd, Xd, lsd, lvd = Z.to(DEV), X.to(DEV), ls.to(DEV), lv.to(DEV)

            def call():
                K = Guarded(B * M * Cn, f64, DEV)
                rc = lib.gpsa_kmat_batched(mu.KINDS[kind], p(Zd), M * D, M, p(Xd), Cn * D, Cn, D, p(lsd), p(lvd), 1,
                                           lls(live) if ragged else None, B, mu.JITTER, K.ptr(), M * Cn, stream())
                torch.cuda.synchronize()
                assert rc == 0 and K.intact()
                return (K.view,)

            (K,) = twice(call)
            check("kmat", f"gpsa_kmat_batched {kind} M={M} C={Cn} D={D} ragged={ragged}", K, want, bound)


def test_kmat_batch_limit(lib):
    """16 problems are taken, 17 refused with GPSA_EINVAL before anything is written (forward and backward)"""
    M, Cn, D = 3, 5, 2
    Z = torch.stack([mu.points(M, D, f32, b) for b in range(17)])
    X = torch.stack([mu.points(Cn, D, f32, 50 + b) for b in range(17)])
    ls, lv = mu.hyper(f32, n=17)
    Kbar = rnd(17, M, Cn, seed=3)
    Zd, Xd, lsd, lvd, Kbd = Z.to(DEV), X.to(DEV), ls.to(DEV), lv.to(DEV), Kbar.to(DEV)
    for B in (16, 17):
        K = Guarded(B * M * Cn, f64, DEV)
        rc = lib.gpsa_kmat_batched(0, p(Zd), M * D, M, p(Xd), Cn * D, Cn, D, p(lsd), p(lvd), 1, None, B, 0.0, K.ptr(),
                                   M * Cn, stream())
        torch.cuda.synchronize()
        wsb = int(lib.gpsa_kmat_bwd_batched_workspace(M, Cn, D, B))
        ws, dZ, dpar = poisoned(wsb, DEV), Guarded(B * M * D, f64, DEV), Guarded(2 * B, f64, DEV)
        rcb = lib.gpsa_kmat_bwd_batched(0, p(Zd), M * D, M, p(Xd), Cn * D, Cn, D, p(lsd), p(lvd), 1, None, B, p(Kbd),
                                        M * Cn, 0, dZ.ptr(), M * D, dpar.ptr(), p(ws), wsb, stream())
        torch.cuda.synchronize()
        if B == 17:
            assert rc == EINVAL and rcb == EINVAL and K.untouched() and dZ.untouched() and dpar.untouched()
            continue
        assert rc == 0 and rcb == 0 and K.intact() and dZ.intact() and dpar.intact()
        refs = [mu.cov_fwd_ref("rbf", Z[b], X[b], ls[b], lv[b]) for b in range(B)]
        check("kmat", "gpsa_kmat_batched batch=16", K.view, torch.stack([r[0] for r in refs]),
              torch.stack([r[1] for r in refs]))
        back = [mu.cov_bwd_ref("rbf", Z[b], X[b], ls[b], lv[b], Kbar[b]) for b in range(B)]
        check("kmat_bwd", "gpsa_kmat_bwd_batched batch=16 dZ", dZ.view, torch.stack([r["dZ"] for r in back]),
              torch.stack([r["bZ"] for r in back]))
        check("kmat_bwd", "gpsa_kmat_bwd_batched batch=16 dparams", dpar.view, torch.stack([r["dpar"] for r in back]),
              torch.stack([r["bpar"] for r in back]))


# ------------------------------------------------------------------------------------------------------------------------
# B. covariance backward
# ------------------------------------------------------------------------------------------------------------------------
def _entry_types(entry):
    """-> (storage of Z / parameters, of X, of Kbar, of the gradients, arithmetic u)"""
    if entry in mu.BWD_MODES:
        _, _, idt, T, odt, kdt = mu.BWD_MODES[entry]
        return idt, idt, kdt, odt, (U32 if T == f32 else U64)
    return f32, f64, (f64 if "f64" in entry else f32), f64, U64


def _bwd_case(kind, entry, M, Cn, D, same=False, two=False, seed=0):
    """inputs on the CPU as stored, and the reference"""
    zdt, xdt, kdt, odt, u = _entry_types(entry)
    Z = mu.points(M, D, zdt, 300 + seed + M)
    X = Z.to(xdt).clone() if same else mu.points(Cn, D, xdt, 400 + seed + Cn % 1000)
    ls, lv = mu.hyper(zdt, seed=seed)
    Kbar = rnd(M, Cn, dtype=kdt, seed=500 + seed)
    ax = (rnd(M, Cn, dtype=kdt, seed=600 + seed), rnd(Cn, dtype=f32, seed=700 + seed), 2.0) if two else None
    ref = mu.cov_bwd_ref(kind, Z, X, ls[0], lv[0], Kbar, same=same, axX=ax[0] if two else None,
                         axd=ax[1] if two else None, axs=ax[2] if two else 0.0, u=u, store32=odt == f32)
    assert ref["a_max"] <= mu.A_MAX
    return (Z, X, ls, lv, Kbar, ax), ref


def _run_bwd(lib, kind, entry, M, Cn, D, dev_in, same=False, want_dx=True, short=0):
    """one call of the entry on a fresh poisoned workspace of the queried size (less ``short`` bytes) -> (rc, dZ, dX,
    dparams) as Guarded"""
    Zd, Xd, lsd, lvd, Kbd, ax = dev_in
    _, _, _, odt, _ = _entry_types(entry)
    dZ, dpar = Guarded(M * D, odt, DEV), Guarded(2, odt, DEV)
    dX = Guarded(Cn * D, odt, DEV) if want_dx else None
    k = mu.KINDS[kind]
    if entry in mu.BWD_MODES:
        dtc, itc = mu.BWD_MODES[entry][:2]
        wsb = int(lib.gpsa_kmat_bwd_workspace(dtc, M, Cn, D)) - short
        ws = poisoned(wsb, DEV)
        rc = lib.gpsa_kmat_bwd(dtc, itc, k, p(Zd), M, p(Xd), Cn, D, p(lsd), p(lvd), p(Kbd), int(same), dZ.ptr(),
                               dX.ptr() if dX else 0, dpar.ptr(), p(ws), wsb, stream())
    else:
        wsb = int(lib.gpsa_kmat_bwd_workspace(1, M, Cn, D)) - short
        ws = poisoned(wsb, DEV)
        fn = getattr(lib, "gpsa_kmat_bwd_" + entry)
        head = (k, p(Zd), M, p(Xd), Cn, D, p(lsd), p(lvd), p(Kbd))
        tail = (dZ.ptr(), dX.ptr() if dX else 0, dpar.ptr(), p(ws), wsb, stream())
        if entry.endswith("axpy"):
            rc = fn(*head, p(ax[0]) if ax else 0, p(ax[1]) if ax else 0, ax[2] if ax else 0.0, *tail)
        else:
            rc = fn(*head, *tail)
    torch.cuda.synchronize()
    return rc, dZ, dX, dpar


def _bwd_check(lib, what, kind, entry, M, Cn, D, same=False, two=False, want_dx=True, seed=0):
    cpu, ref = _bwd_case(kind, entry, M, Cn, D, same=same, two=two, seed=seed)
    Z, X, ls, lv, Kbar, ax = cpu
    dev_in = (Z.to(DEV), X.to(DEV), ls.to(DEV), lv.to(DEV), Kbar.to(DEV),
              (ax[0].to(DEV), ax[1].to(DEV), ax[2]) if two else None)

    def call():
        rc, dZ, dX, dpar = _run_bwd(lib, kind, entry, M, Cn, D, dev_in, same=same, want_dx=want_dx)
        assert rc == 0 and dZ.intact() and dpar.intact() and (dX is None or dX.intact()), (what, rc)
        if same and dX is not None:
            assert dX.untouched(), "same != 0: dX is not written"
        return dZ.view, dpar.view, (dX.view if dX is not None and not same else None)

    dZ, dpar, dX = twice(call)
    rs = [check("kmat_bwd", what + " dZ", dZ, ref["dZ"], ref["bZ"]),
          check("kmat_bwd", what + " dparams", dpar, ref["dpar"], ref["bpar"])]
    if dX is not None:
        rs.append(check("kmat_bwd", what + " dX", dX, ref["dX"], ref["bX"]))
    return max(rs)


@pytest.mark.parametrize("case", mu.GEN_LONG_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-D{c[1]}-{c[2]}-{c[3]}")
def test_kmat_bwd_generic_long(lib, case):
    """kmat_bwd_kernel at both sides of kb_rows()'s threshold and on the column-block walk (see mm_stage_util)"""
    (M, Cn), D, kind, entry, two, want_dx = case
    _bwd_check(lib, f"{entry} {kind} M={M} C={Cn} D={D} two={two} dX={want_dx}", kind, entry, M, Cn, D, two=two,
               want_dx=want_dx, seed=D)


@pytest.mark.parametrize("D", mu.GEN_D)
@pytest.mark.parametrize("kind", list(mu.KINDS))
def test_kmat_bwd_generic_small(lib, kind, D):
    """every entry and type mode at (200, 777), the two-piece entries with and without their second piece"""
    M, Cn = mu.GEN_SMALL
    for entry in list(mu.BWD_MODES) + mu.X64_ENTRIES:
        for two in ((False, True) if entry.endswith("axpy") else (False,)):
            _bwd_check(lib, f"{entry} {kind} M={M} C={Cn} D={D} two={two}", kind, entry, M, Cn, D, two=two, seed=D)


@pytest.mark.parametrize("M", mu.D2_M)
def test_kmat_bwd_d2_rows(lib, M):
    """kmat_bwd_d2_kernel: the even spread of M over ceil(M / 16) row chunks at its edges, every kind and entry"""
    kinds = list(mu.KINDS)
    for i, entry in enumerate(list(mu.BWD_MODES) + mu.X64_ENTRIES):
        two = entry.endswith("axpy")
        _bwd_check(lib, f"d2 {entry} {kinds[i % 3]} M={M} C={mu.D2_C} two={two}", kinds[i % 3], entry, M, mu.D2_C, 2,
                   two=two, seed=i)
    for kind in kinds:
        _bwd_check(lib, f"d2 out64 {kind} M={M} C={mu.D2_C}", kind, "out64", M, mu.D2_C, 2, seed=9)


@pytest.mark.parametrize("shape,kind,entry", [(mu.D2_PER, "matern32", "x64"), (mu.D2_FINISH, "matern12", "x64_f64"),
                                              (mu.D2_FINISH, "rbf", "acc64")])
def test_kmat_bwd_d2_long(lib, shape, kind, entry):
    """two column blocks per workgroup (per > 1), and nbx >= 49 partial rows: the finish kernel's four-way loop"""
    M, Cn = shape
    per, nbx, _, _ = mu.d2_grid(M, Cn)
    assert (per > 1) if shape == mu.D2_PER else (per == 1 and nbx >= 49)
    _bwd_check(lib, f"d2 {entry} {kind} M={M} C={Cn}", kind, entry, M, Cn, 2, seed=1)


@pytest.mark.parametrize("M", mu.D2_SAME)
@pytest.mark.parametrize("D", [2, 3])
def test_kmat_bwd_same(lib, M, D):
    """same = 1 at M = C: the X-side partials folded into dZ equal the reference's gz + gx; dX is not written"""
    for kind in mu.KINDS:
        for entry in ("f64", "out64", "f32"):
            _bwd_check(lib, f"same {entry} {kind} M=C={M} D={D}", kind, entry, M, M, D, same=True, seed=D)


@pytest.mark.parametrize("B", mu.BATCHED_B)
@pytest.mark.parametrize("kind", list(mu.KINDS))
def test_kmat_bwd_batched(lib, kind, B):
    """gpsa_kmat_bwd_batched with ragged live counts (0, a block edge, C, ...); the padding columns of X and Kbar
    hold NaN, which the kernel must not read"""
    for M, Cn, D in mu.BATCHED_SHAPES:
        live = mu.bwd_n_live(Cn, B)
        Z = torch.stack([mu.points(M, D, f32, 13 * b + M) for b in range(B)])
        X = torch.stack([mu.points(Cn, D, f32, 17 * b + Cn) for b in range(B)])
        ls, lv = mu.hyper(f32, n=B, seed=B)
        Kbar = rnd(B, M, Cn, seed=40 + B)
        refs = [mu.cov_bwd_ref(kind, Z[b], X[b], ls[b], lv[b], Kbar[b], n_live=live[b]) for b in range(B)]
        assert max(r["a_max"] for r in refs) <= mu.A_MAX
        for b in range(B):
            X[b, live[b]:] = NAN
            Kbar[b, :, live[b]:] = NAN
        Zd, Xd, lsd, lvd, Kbd = Z.to(DEV), X.to(DEV), ls.to(DEV), lv.to(DEV), Kbar.to(DEV)

        def call():
            wsb = int(lib.gpsa_kmat_bwd_batched_workspace(M, Cn, D, B))
            ws, dZ, dpar = poisoned(wsb, DEV), Guarded(B * M * D, f64, DEV), Guarded(2 * B, f64, DEV)
            rc = lib.gpsa_kmat_bwd_batched(mu.KINDS[kind], p(Zd), M * D, M, p(Xd), Cn * D, Cn, D, p(lsd), p(lvd), 1,
                                           lls(live), B, p(Kbd), M * Cn, 0, dZ.ptr(), M * D, dpar.ptr(), p(ws), wsb,
                                           stream())
            torch.cuda.synchronize()
            assert rc == 0 and dZ.intact() and dpar.intact()
            return dZ.view, dpar.view

        dZ, dpar = twice(call)
        what = f"batched {kind} M={M} C={Cn} D={D} B={B} n_live={live}"
        check("kmat_bwd", what + " dZ", dZ, torch.stack([r["dZ"] for r in refs]), torch.stack([r["bZ"] for r in refs]))
        check("kmat_bwd", what + " dparams", dpar, torch.stack([r["dpar"] for r in refs]),
              torch.stack([r["bpar"] for r in refs]))


@pytest.mark.parametrize("D", [2, 3])
def test_kmat_bwd_workspace_refusal(lib, D):
    """a workspace one byte short: GPSA_EWORKSPACE and untouched outputs; the queried size itself is taken"""
    M, Cn = mu.GEN_SMALL
    assert D != 2 or mu.d2_grid(M, Cn)[0] == 1  # (one column block per workgroup: the query is what the launch needs)
    for entry in ("f64", "x64_f64"):
        cpu, _ = _bwd_case("rbf", entry, M, Cn, D)
        dev_in = tuple(t.to(DEV) if torch.is_tensor(t) else t for t in cpu)
        rc, dZ, dX, dpar = _run_bwd(lib, "rbf", entry, M, Cn, D, dev_in, short=1)
        assert rc == EWORKSPACE and dZ.untouched() and dX.untouched() and dpar.untouched(), (entry, rc)
        rc, dZ, dX, dpar = _run_bwd(lib, "rbf", entry, M, Cn, D, dev_in)
        assert rc == 0 and dZ.intact() and dX.intact() and dpar.intact()


# ------------------------------------------------------------------------------------------------------------------------
# C. Omega
# ------------------------------------------------------------------------------------------------------------------------
def _dev_off(t, off):
    """t on the device, ``off`` elements past the start of its allocation (off = 1: not 16-byte aligned)"""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def _omega_case(lib, M, n0, n1, offs=(0, 0, 0), sym_flags=(1, 0)):
    """forward and adjoint of one (M, n0, n1); offs: element offsets of A0, A1 and the dA outputs"""
    segs = [n for n in (n0, n1) if n]
    A = [rnd(n, M, M, dtype=f32, seed=10 * M + i) for i, n in enumerate(segs)]
    Ad = [_dev_off(a, offs[i]) for i, a in enumerate(A)]
    two = n1 > 0
    dma = mu.omega_dma(M, aligned=not any(offs[:2]))
    what = f"M={M} n=({n0},{n1}) offsets={offs} {'dma' if dma else 'generic'}"

    def fwd():
        O = [Guarded(n * M * M, f64, DEV) for n in segs]
        if two:
            rc = lib.gpsa_omega_fwd2(p(Ad[0]), n0, O[0].ptr(), p(Ad[1]), n1, O[1].ptr(), M, mu.OMEGA_JITTER, stream())
        else:
            rc = lib.gpsa_omega_fwd(p(Ad[0]), M, n0, mu.OMEGA_JITTER, O[0].ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0 and all(o.intact() for o in O), (what, rc)
        return tuple(o.view for o in O)

    for a, o in zip(A, twice(fwd)):
        want, bound = mu.omega_fwd_ref(a, mu.OMEGA_JITTER)
        check("omega", "fwd " + what, o, want, bound)
        if dma:
            o3 = o.view(-1, M, M)
            assert torch.equal(o3, o3.transpose(1, 2)), "the LDS-DMA forward is symmetric to the bit"
    for symmetric in sym_flags:
        G = [rnd(n, M, M, seed=20 * M + i + symmetric) for i, n in enumerate(segs)]
        if symmetric:
            G = [(g + g.transpose(1, 2)).contiguous() for g in G]
        Gd = [g.to(DEV) for g in G]

        def bwd():
            dA = [Guarded(n * M * M, f32, DEV, off=offs[2]) for n in segs]
            if two:
                rc = lib.gpsa_omega_bwd2(p(Gd[0]), p(Ad[0]), dA[0].ptr(), n0, p(Gd[1]), p(Ad[1]), dA[1].ptr(), n1, M,
                                         symmetric, stream())
            else:
                rc = lib.gpsa_omega_bwd(p(Gd[0]), p(Ad[0]), M, n0, symmetric, dA[0].ptr(), stream())
            torch.cuda.synchronize()
            assert rc == 0 and all(d.intact() for d in dA), (what, rc)
            return tuple(d.view for d in dA)

        for g, a, d in zip(G, A, twice(bwd)):
            want, bound = mu.omega_bwd_ref(g, a, symmetric)
            check("omega", f"bwd symmetric={symmetric} " + what, d, want, bound)


@pytest.mark.parametrize("M", mu.OMEGA_DMA + mu.OMEGA_GENERIC)
def test_omega(lib, M):
    """gpsa_omega_fwd / _fwd2 / _bwd / _bwd2: LDS-DMA sizes with a last 16-chunk of 4, 8, 12 or 16 columns, generic
    sizes, every segment count; a jitter of 0.375 must show on the diagonal exactly once"""
    for n0, n1 in mu.OMEGA_SEGMENTS:
        _omega_case(lib, M, n0, n1)


@pytest.mark.parametrize("M", mu.OMEGA_OFFSET_M)
def test_omega_unaligned_falls_back(lib, M):
    """DMA-eligible sizes with A0, A1 alone, or dA one element off 16-byte alignment: the generic product must take
    them (a 16-byte access there would fault or read shifted data)"""
    assert mu.omega_dma(M) and not mu.omega_dma(M, aligned=False)
    _omega_case(lib, M, 2, 3, offs=(1, 0, 0))
    _omega_case(lib, M, 2, 3, offs=(0, 1, 0))
    _omega_case(lib, M, 2, 3, offs=(0, 0, 1))
    _omega_case(lib, M, 3, 0, offs=(1, 0, 0))


# ------------------------------------------------------------------------------------------------------------------------
# D. KL
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", mu.KL_SLICED_M)
def test_kl_grouped_fwd_sliced(lib, M):
    """the step's forward (rows dealt to up to 8 workgroups, last-arrival counter) through
    gpsa_mvn_kl_grouped_fwd_sliced, the same entry with part = cnt = NULL, and gpsa_mvn_kl_grouped_fwd"""
    T = 5
    om_idx, pr_idx = [2, 3, 4, 5, 6], [0, 1, 0, -1, 0]
    mats, inv, logdet = mu.spd_batch(7, M, seed=M)
    D = rnd(T, M, seed=M + 1)
    ns = int(lib.gpsa_mvn_kl_grouped_fwd_slices(M))
    assert ns == mu.kl_slices(M)
    want_kl, b_kl, want_kd, b_kd = (torch.zeros(T, dtype=f64), torch.zeros(T, dtype=f64), torch.zeros(T, M, dtype=f64),
                                    torch.zeros(T, M, dtype=f64))
    for t in range(T):
        if pr_idx[t] >= 0:
            want_kl[t], b_kl[t], want_kd[t], b_kd[t] = mu.kl_fwd_ref(inv[pr_idx[t]], logdet[pr_idx[t]], mats[om_idx[t]],
                                                                     logdet[om_idx[t]], D[t])
    md, ivd, ldd, Dd = mats.to(DEV), inv.to(DEV), logdet.to(DEV), D.to(DEV)
    omd = torch.tensor(om_idx, dtype=torch.int32, device=DEV)
    prd = torch.tensor(pr_idx, dtype=torch.int32, device=DEV)
    for form in ("sliced", "one workgroup", "grouped_fwd"):
        def call():
            kl, KD, cp = Guarded(T, f64, DEV), Guarded(T * M, f64, DEV), Guarded(T, f64, DEV)
            part = Guarded(T * ns, f64, DEV, fill=NAN)
            cnt = torch.zeros(T + 2 * 64, dtype=torch.int32, device=DEV)
            if form == "grouped_fwd":
                rc = lib.gpsa_mvn_kl_grouped_fwd(p(md), p(ivd), p(ldd), p(omd), p(prd), p(Dd), M, T, kl.ptr(), KD.ptr(),
                                                 stream())
            else:
                sl = form == "sliced"
                rc = lib.gpsa_mvn_kl_grouped_fwd_sliced(p(md), p(ivd), p(ldd), p(omd), p(prd), p(Dd), M, T, kl.ptr(),
                                                        KD.ptr(), cp.ptr(), part.ptr() if sl else 0,
                                                        cnt[64:].data_ptr() if sl else 0, stream())
            torch.cuda.synchronize()
            assert rc == 0 and kl.intact() and KD.intact() and cp.intact() and part.intact()
            assert not bool(cnt.any()), "the arrival counters are zero again (and nothing next to them was counted)"
            if form == "grouped_fwd":
                assert cp.untouched()
            else:
                assert same_bits(cp.view, kl.view), "kl_copy is kl"
            if form != "sliced":
                assert bool(torch.isnan(part.view).all())
            return kl.view, KD.view

        kl, KD = twice(call)
        check("kl", f"fwd {form} M={M} slices={ns} kl", kl, want_kl, b_kl)
        check("kl", f"fwd {form} M={M} slices={ns} KD", KD, want_kd, b_kd)
        assert float(kl[3]) == 0.0 and not bool(KD.view(T, M)[3].any())  # the absent term: exact zeros


def test_kl_grouped_fwd_sliced_null_checks(lib):
    M, T = 8, 2
    mats, inv, logdet = mu.spd_batch(3, M, seed=1)
    t = [x.to(DEV) for x in (mats, inv, logdet)]
    idx = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    pr = torch.zeros(2, dtype=torch.int32, device=DEV)
    D, kl, KD = rnd(T, M).to(DEV), Guarded(T, f64, DEV), Guarded(T * M, f64, DEV)
    args = [p(t[0]), p(t[1]), p(t[2]), p(idx), p(pr), p(D), M, T, kl.ptr(), KD.ptr(), 0, 0, 0, stream()]
    for i in (0, 1, 2, 3, 4, 5, 8, 9):
        bad = list(args)
        bad[i] = 0
        assert lib.gpsa_mvn_kl_grouped_fwd_sliced(*bad) == EINVAL
    for i, v in ((6, 0), (7, 0)):
        bad = list(args)
        bad[i] = v
        assert lib.gpsa_mvn_kl_grouped_fwd_sliced(*bad) == EINVAL
    torch.cuda.synchronize()
    assert kl.untouched() and KD.untouched()
    assert lib.gpsa_mvn_kl_grouped_fwd_sliced(*args) == 0
    torch.cuda.synchronize()
    assert kl.intact() and KD.intact() and bool(torch.isfinite(kl.view).all())


@pytest.mark.parametrize("M", mu.KL_BWD_M)
def test_kl_grouped_bwd(lib, M):
    """gpsa_mvn_kl_grouped_bwd_acc: groups of 0, 1, 7, 8, 9 and 17 terms in one plan (the 8-at-a-time loop at its
    exact-8 edge, one over, and a third round), absent groups of 0 and 2, accumulate 0 and 1"""
    P, mm = len(mu.KL_GROUPS), M * M
    pr_list = [3, 0, 5, 1, 4, 2]
    for n_abs in mu.KL_ABSENT:
        T = sum(mu.KL_GROUPS) + n_abs
        perm = torch.randperm(T, generator=torch.Generator().manual_seed(T)).tolist()
        grp_off = [0]
        for s in mu.KL_GROUPS + [n_abs]:
            grp_off.append(grp_off[-1] + s)
        om_idx = [P + (5 * t + 2) % T for t in range(T)]  # a permutation of the Omegas (5 and T are coprime)
        assert sorted(om_idx) == list(range(P, P + T))
        mats, inv, _ = mu.spd_batch(P + T, M, seed=M + n_abs)
        D, KD, g = rnd(T, M, seed=1), rnd(T, M, seed=2), rnd(T, seed=3).abs() + 0.5
        old = rnd(T, M, M, seed=4)
        dev = [x.to(DEV) for x in (mats, inv, D, KD, g)]
        ints = [torch.tensor(x, dtype=torch.int32, device=DEV) for x in (om_idx, pr_list, grp_off, perm)]
        for acc in (0, 1):
            wO = old.clone() if acc else torch.zeros(T, M, M, dtype=f64)
            bO = torch.zeros(T, M, M, dtype=f64)
            wS, bS = torch.zeros(P, M, M, dtype=f64), torch.zeros(P, M, M, dtype=f64)
            wD = torch.zeros(T, M, dtype=f64)
            for pg in range(P):
                terms = perm[grp_off[pg]: grp_off[pg + 1]]
                pr = pr_list[pg]
                gs, s, sa = 0.0, torch.zeros(M, M, dtype=f64), torch.zeros(M, M, dtype=f64)
                for t in terms:
                    upd = 0.5 * g[t] * (inv[pr] - inv[om_idx[t]])
                    bO[t] = 4 * U64 * (wO[t].abs() + 0.5 * g[t] * (inv[pr].abs() + inv[om_idx[t]].abs()))
                    wO[t] = wO[t] + upd
                    wD[t] = g[t] * KD[t]
                    dd = torch.outer(D[t], D[t])
                    gs, s, sa = gs + g[t], s + g[t] * (mats[om_idx[t]] + dd), sa + g[t] * (mats[om_idx[t]].abs() + dd.abs())
                wS[pg] = gs * mats[pr] - s
                bS[pg] = bar(len(terms), abs(gs) * mats[pr].abs() + sa) if terms else 0.0

            def call():
                dO = Guarded(T * mm, f64, DEV)
                if acc:
                    dO.view.copy_(old.reshape(-1))
                dD, S = Guarded(T * M, f64, DEV), Guarded(P * mm, f64, DEV)
                rc = lib.gpsa_mvn_kl_grouped_bwd_acc(p(dev[0]), p(dev[1]), p(ints[0]), p(ints[1]), p(ints[2]), p(ints[3]),
                                                     p(dev[2]), p(dev[3]), p(dev[4]), M, T, P, dO.ptr(), dD.ptr(), S.ptr(),
                                                     acc, stream())
                torch.cuda.synchronize()
                assert rc == 0 and dO.intact() and dD.intact() and S.intact()
                return dO.view, dD.view, S.view

            dO, dD, S = twice(call)
            what = f"bwd M={M} absent={n_abs} accumulate={acc}"
            check("kl", what + " dOmega", dO, wO, bO)  # absent terms: bound 0 - zeroed, or left alone when accumulating
            check("kl", what + " S", S, wS, bS)
            check("kl", what + " dD", dD, wD, 2 * U64 * wD.abs())


@pytest.mark.parametrize("L", mu.KL_PLAIN_L)
@pytest.mark.parametrize("M", mu.KL_PLAIN_M)
def test_kl_plain_pair(lib, M, L):
    """gpsa_mvn_kl_fwd / _bwd with strided Omega, Omega^-1 and logdet"""
    mm, so, sl = M * M, M * M + 3, 2
    mats, inv, logdet = mu.spd_batch(1 + L, M, seed=M + L)
    Dm, g = rnd(M, L, seed=5), rnd(L, seed=6).abs() + 0.5
    KD = inv[0] @ Dm
    Om, Oi = torch.full((L, so), NAN, dtype=f64), torch.full((L, so), NAN, dtype=f64)
    Om[:, :mm], Oi[:, :mm] = mats[1:].reshape(L, mm), inv[1:].reshape(L, mm)
    ldo = torch.full((L, sl), NAN, dtype=f64)
    ldo[:, 0] = logdet[1:]
    refs = [mu.kl_fwd_ref(inv[0], logdet[0], mats[1 + l], logdet[1 + l], Dm[:, l], KD=KD[:, l]) for l in range(L)]
    dev = [x.to(DEV) for x in (mats[0].contiguous(), inv[0].contiguous(), logdet[:1].contiguous(), Om, Oi, ldo, Dm, KD, g)]
    Kd, Kid, ldk, Omd, Oid, ldod, Dmd, KDd, gd = dev

    def fwd():
        kl = Guarded(L, f64, DEV)
        rc = lib.gpsa_mvn_kl_fwd(p(Kid), p(ldk), p(Omd), so, p(ldod), sl, p(Dmd), p(KDd), M, L, kl.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0 and kl.intact()
        return (kl.view,)

    (kl,) = twice(fwd)
    check("kl", f"plain fwd M={M} L={L}", kl, torch.stack([r[0] for r in refs]), torch.stack([r[1] for r in refs]))
    gs = g.sum()
    dd = torch.einsum("il,jl->lij", Dm, Dm)
    wO = 0.5 * g[:, None, None] * (inv[0] - inv[1:])
    bO = 4 * U64 * 0.5 * g[:, None, None] * (inv[0].abs() + inv[1:].abs())
    wS = gs * mats[0] - (g[:, None, None] * (mats[1:] + dd)).sum(0)
    bS = bar(L, gs * mats[0].abs() + (g[:, None, None] * (mats[1:].abs() + dd.abs())).sum(0))
    wD = KD * g[None, :]

    def bwd():
        dO, dDm, Sp = Guarded(L * mm, f64, DEV), Guarded(M * L, f64, DEV), Guarded(mm, f64, DEV)
        rc = lib.gpsa_mvn_kl_bwd(p(Kd), p(Kid), p(Omd), so, p(Oid), so, p(Dmd), p(KDd), p(gd), M, L, dO.ptr(), dDm.ptr(),
                                 Sp.ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0 and dO.intact() and dDm.intact() and Sp.intact()
        return dO.view, dDm.view, Sp.view

    dO, dDm, Sp = twice(bwd)
    check("kl", f"plain bwd M={M} L={L} dOmega", dO, wO, bO)
    check("kl", f"plain bwd M={M} L={L} dD", dDm, wD, 2 * U64 * wD.abs())
    check("kl", f"plain bwd M={M} L={L} S", Sp, wS, bS)
