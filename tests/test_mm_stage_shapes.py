"""The shape arithmetic behind tests/test_mm_stage_gpu.py, without a GPU: from the library's own pure queries (256 compute
units where no device answers), every listed shape takes the branch the GPU test names for it; and the references and
bounds of tests/mm_stage_util.py are sound on the CPU (the input box keeps every exponent argument below 20, the
longdouble reference agrees with autograd of an independent fp64 restatement far inside its bound)."""
import numpy as np
import pytest
import torch

import mm_stage_util as mu
from fp64_products_util import U64, f32, f64, rnd

CUS = mu.CUS


@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, "these sums are written for 256 CUs"
    from spatial_alignment_amd import _lib

    return _lib.load()


def _chunks(lib, M, C, D, dtype=1):
    return mu.row_chunks_from_workspace(int(lib.gpsa_kmat_bwd_workspace(dtype, M, C, D)), 8 if dtype else 4, M, C, D)


def test_generic_backward_row_chunks(lib):
    """7 against 25 row chunks at M = 200 (tests/test_cabi.py's model); the two threshold neighbours fall on opposite
    sides of kb_rows(); the walk shape takes 32 rows and has 1026 column blocks, the last of one column"""
    for D in mu.GEN_D:
        assert _chunks(lib, 200, 100000, D) == 7 and _chunks(lib, *mu.GEN_SMALL, D) == 25
        for (M, C), rows in ((mu.GEN_BELOW, 8), (mu.GEN_ABOVE, 32), (mu.GEN_WALK, 32), (mu.GEN_SMALL, 8)):
            assert mu.kb_rows(M, C) == rows and _chunks(lib, M, C, D) == -(-M // rows), (M, C, D)
            assert _chunks(lib, M, C, D, dtype=0) == -(-M // rows)
    (Mb, Cb), (Ma, Ca) = mu.GEN_BELOW, mu.GEN_ABOVE
    assert Mb == Ma and -(-Cb // 256) * 2 == 1020 and -(-Ca // 256) * 2 == 1024 and Ca - Cb == 257
    assert Ma == 32 + 8  # one full 32-row chunk and a ragged one of 8
    M, C = mu.GEN_WALK
    assert -(-C // 256) == 1026 > 1024 and C % 256 == 1 and M <= 32
    # every long case: all three shapes with each D, every kind three times, two-piece and dX = NULL among them
    cases = mu.GEN_LONG_CASES
    assert {(c[0], c[1]) for c in cases} == {(s, D) for s in (mu.GEN_BELOW, mu.GEN_ABOVE, mu.GEN_WALK) for D in mu.GEN_D}
    assert all(sum(c[2] == k for c in cases) == 3 for k in mu.KINDS)
    assert any(c[4] for c in cases) and any(not c[5] for c in cases)
    assert all(c[3].endswith("axpy") for c in cases if c[4])
    # the batched query clamps the column blocks to 1024 workgroups
    per_problem = int(lib.gpsa_kmat_bwd_batched_workspace(M, C, 3, 1))
    assert per_problem == (1024 * M * 3 + 1 * C * 3 + 1024 * 2) * 8


def test_d2_backward_grids(lib):
    """the register kernel's row spread and the shapes that reach per > 1 and the finish kernel's unrolled loop"""
    spread = {M: mu.d2_grid(M, mu.D2_C)[2:] for M in mu.D2_M}
    assert spread == {1: (1, 1), 16: (1, 16), 17: (2, 9), 33: (3, 11), 49: (4, 13), 200: (13, 16), 257: (17, 16)}
    assert 257 - 16 * 16 == 1 and 17 - 9 == 8  # a last chunk of one row; 9 + 8
    for M in mu.D2_M:
        assert _chunks(lib, M, mu.D2_C, 2) == -(-M // 16) and mu.d2_grid(M, mu.D2_C)[0] == 1
    per, nbx, nby, _ = mu.d2_grid(*mu.D2_PER)
    assert per == 2 and nbx * nby <= 2 * CUS < -(-mu.D2_PER[1] // 256) * nby
    M, C = mu.D2_FINISH
    per, nbx, nby, _ = mu.d2_grid(M, C)
    assert M <= 160 and C >= 12545 and per == 1 and nbx >= 49
    # M = 200: at most 39 partial rows however long the panel (the finish kernel's unrolled loop is out of reach)
    assert max(mu.d2_grid(200, C)[1] for C in range(256, 300000, 256)) == 39
    for M in mu.D2_SAME:
        assert mu.d2_grid(M, M)[0] == 1
    for M, C, D in mu.BATCHED_SHAPES:
        for B in mu.BATCHED_B:
            live = mu.bwd_n_live(C, B)
            assert len(live) == B and all(0 <= n <= C for n in live)
            if B > 1:
                assert {0, 256, C} <= set(live)
            assert mu.kb_rows(M, C * B) == 8


def test_kl_slices(lib):
    for M, ns in mu.KL_SLICES.items():
        assert int(lib.gpsa_mvn_kl_grouped_fwd_slices(M)) == ns == mu.kl_slices(M), M
    for M in range(1, 65):
        assert int(lib.gpsa_mvn_kl_grouped_fwd_slices(M)) == 1
    got = {M: int(lib.gpsa_mvn_kl_grouped_fwd_slices(M)) for M in mu.KL_SLICED_M}
    assert got == {1: 1, 15: 1, 16: 1, 17: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 255: 4, 256: 4, 257: 5, 449: 8, 512: 8,
                   513: 8}
    assert 513 > 64 * 8  # slice 0 sweeps twice
    assert mu.KL_GROUPS == [0, 1, 7, 8, 9, 17] and mu.KL_ABSENT == [0, 2]


def test_omega_lists_split_by_the_predicate():
    assert all(mu.omega_dma(M) for M in mu.OMEGA_DMA) and not any(mu.omega_dma(M) for M in mu.OMEGA_GENERIC)
    assert {M % 16 for M in mu.OMEGA_DMA} == {0, 4, 8, 12}  # the last 16-chunk holds 4, 8, 12 or all 16 columns
    assert all(mu.omega_dma(M) and not mu.omega_dma(M, aligned=False) for M in mu.OMEGA_OFFSET_M)
    assert mu.OMEGA_SEGMENTS == [(1, 0), (3, 0), (2, 3), (1, 1)]


def test_forward_lists():
    assert mu.FWD_M == [1, 15, 16, 17, 33] and mu.FWD_C == [1, 255, 256, 257, 513] and mu.FWD_D == [1, 2, 3, 4]
    assert mu.fwd_n_live(513) == [0, 1, 255, 256, 257, 513] and mu.fwd_n_live(257) == [0, 1, 255, 256, 257]
    assert all(len(mu.fwd_n_live(C)) <= mu.KM_MAXB for _, C, _ in mu.FWD_BATCHED)


@pytest.mark.parametrize("kind", list(mu.KINDS))
def test_the_box_and_the_covariance_reference(kind):
    """the chosen box keeps a <= 20 at every D; the longdouble reference agrees with autograd of a separate fp64
    restatement (the formulas of the reference package's kernels) to a small fraction of the fp64 bound's scale"""
    for D in mu.FWD_D:
        Z, X = mu.points(33, D, f64, D), mu.points(257, D, f64, D + 1)
        Z[0], X[0] = 0.0, 1.0  # opposite corners of the box: the largest distance there is
        ls, lv = mu.hyper(f64, seed=D)
        Kbar = rnd(33, 257, seed=D)
        ref = mu.cov_bwd_ref(kind, Z, X, ls[0], lv[0], Kbar)
        K, bound, amax = mu.cov_fwd_ref(kind, Z, X, ls[0], lv[0], mu.JITTER)
        ell0 = float(torch.exp(ls[0]))  # the corners give the box's largest argument
        top = {"rbf": 0.5 * D / ell0 ** 2, "matern12": 0.5 * (D + 1e-10) ** 0.5 / ell0,
               "matern32": (3 * (D + 1e-10)) ** 0.5 / ell0}[kind]
        assert ref["a_max"] == amax <= mu.A_MAX and amax == pytest.approx(top, rel=1e-12)
        Zt, Xt, lst, lvt = (t.clone().requires_grad_(True) for t in (Z, X, ls, lv))
        d2 = ((Zt[:, None, :] - Xt[None, :, :]) ** 2).sum(-1)
        ell = torch.exp(lst[0])
        if kind == "rbf":
            Kt = torch.exp(lvt[0]) * torch.exp(-0.5 * d2 / ell ** 2)
        elif kind == "matern12":
            Kt = torch.exp(lvt[0]) * torch.exp(-0.5 * torch.sqrt(d2 + 1e-10) / ell)
        else:
            zz = np.sqrt(3.0) * torch.sqrt(d2 + 1e-10) / ell
            Kt = torch.exp(lvt[0]) * (1 + zz) * torch.exp(-zz)
        (Kt * Kbar).sum().backward()
        Kj = Kt.detach() + mu.JITTER * torch.eye(33, 257, dtype=f64)
        assert bool(((Kj - K).abs() <= bound).all()) and bool((bound > 0).all())
        for got, want, b in ((Zt.grad, ref["dZ"], ref["bZ"]), (Xt.grad, ref["dX"], ref["bX"]),
                             (torch.stack([lst.grad[0], lvt.grad[0]]), ref["dpar"], ref["bpar"])):
            assert bool(((got - want).abs() <= b).all()), (kind, D)
            assert bool((b <= 1e-9 * (1 + want.abs().max())).all())  # ... and the bound is not vacuous


def test_the_backward_reference_options():
    """live columns, the folded K_uu form and the two-piece panel of the reference against its plain form"""
    Z, X = mu.points(17, 3, f32, 1), mu.points(40, 3, f32, 2)
    ls, lv = mu.hyper(f32)
    Kbar, X2, d = rnd(17, 40, seed=1), rnd(17, 40, seed=2), rnd(40, dtype=f32, seed=3)
    full = mu.cov_bwd_ref("matern32", Z, X, ls[0], lv[0], Kbar + 2.0 * d.double()[None, :] * X2)
    two = mu.cov_bwd_ref("matern32", Z, X, ls[0], lv[0], Kbar, axX=X2, axd=d, axs=2.0, chunk=16)
    for n in ("dZ", "dX", "dpar"):
        assert torch.allclose(full[n], two[n], rtol=1e-13, atol=1e-15)
        assert bool((two["b" + n[1:]] >= full["b" + n[1:]]).all())
    cut = mu.cov_bwd_ref("matern32", Z, X, ls[0], lv[0], Kbar, n_live=25)
    part = mu.cov_bwd_ref("matern32", Z, X[:25], ls[0], lv[0], Kbar[:, :25])
    assert torch.equal(cut["dZ"], part["dZ"]) and torch.equal(cut["dpar"], part["dpar"])
    assert not bool(cut["dX"][25:].any()) and not bool(cut["bX"][25:].any())
    same = mu.cov_bwd_ref("rbf", Z, Z, ls[0], lv[0], Kbar[:, :17], same=True)
    plain = mu.cov_bwd_ref("rbf", Z, Z, ls[0], lv[0], Kbar[:, :17])
    assert torch.allclose(same["dZ"], plain["dZ"] + plain["dX"], rtol=1e-14, atol=1e-16)
    st = mu.cov_bwd_ref("rbf", Z, X, ls[0], lv[0], Kbar, store32=True)
    pl = mu.cov_bwd_ref("rbf", Z, X, ls[0], lv[0], Kbar)
    assert torch.equal(st["bZ"], pl["bZ"] + 2.0 ** -24 * pl["dZ"].abs())
    K0, b0, _ = mu.cov_fwd_ref("rbf", Z, X, ls[0], lv[0], mu.JITTER, U64, n_live=5)
    assert not bool(K0[:, 5:].any()) and not bool(b0[:, 5:].any()) and bool((K0[:, :5] > 0).all())
