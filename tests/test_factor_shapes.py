"""The shape arithmetic behind tests/test_factor_gpu.py, without a GPU: from the library's own workspace query every listed
M is cut into the diagonal blocks, and lands in the kernel class, the GPU test names it for; the lists really hold the first,
the last and a ragged member of every class; and the reference and bounds of tests/factor_util.py are sound on the CPU
(LAPACK through torch.linalg and a plain fp64 restatement of the two algorithms stay inside them on every input family)."""
import numpy as np
import pytest
import torch

import factor_util as fu
from fp64_products_util import f64


@pytest.fixture(scope="module")
def lib():
    from spatial_alignment_amd import _lib

    return _lib.load()


def _bs(lib, M, batch=1):
    return fu.block_size_from_workspace(int(lib.gpsa_chol_inv_blocked_workspace(M, batch)), M, batch)


def test_panel_and_register_classes_of_the_fused_entry():
    """gpsa_chol_inv_f64: first, last and a ragged member of every chol_inv_blk_kernel<NT> and <NT, 32> class"""
    first = 1
    for nt, ms in fu.PANEL_M.items():
        assert all(fu.panel_class(M) == nt for M in ms)
        assert ms[0] == first and ms[-1] == 16 * nt
        assert any(M % 16 and M != first for M in ms), nt  # ragged: the last tile is part padding
        first = 16 * nt + 1
    assert first == 209
    for nt, ms in fu.REG32_M.items():
        assert all(fu.reg_class(M) == (32, nt) for M in ms)
        assert ms[0] == first and ms[-1] == 32 * nt and any(M % 32 for M in ms)
        first = 32 * nt + 1
    assert first == 257  # GPSA_EUNSUPPORTED from here
    assert fu.panel_class(112) == 7 and fu.panel_class(113) == 10 and fu.panel_class(160) == 10 and fu.panel_class(161) == 13
    assert len(fu.FUSED_M) == len(set(fu.FUSED_M)) == 21


def test_one_block_up_to_256(lib):
    """gpsa_chol_inv_blocked_f64 at M <= 256 is one diagonal block: the same M list is the first, last and a ragged member
    of chol_inv_reg_kernel<2|4|7|13, 16> (M <= 208) and <7|8, 32>"""
    seen = {}
    for M in fu.FUSED_M:
        for batch in (1, 3):
            assert fu.blocks(M, _bs(lib, M, batch)) == [M]
        seen.setdefault(fu.reg_class(M), []).append(M)
    assert seen == {(16, 2): [1, 17, 32], (16, 4): [33, 49, 64], (16, 7): [65, 100, 112],
                    (16, 13): [113, 150, 160, 161, 199, 200, 208], (32, 7): [209, 224], (32, 8): [225, 241, 256]}
    for (ts, nt), ms in seen.items():
        lo = {2: 1, 4: 33, 7: 65, 13: 113}[nt] if ts == 16 else {7: 209, 8: 225}[nt]
        assert min(ms) == lo and max(ms) == (ts * nt) and fu.reg_class(lo)[1] == nt
        assert lo == 1 or fu.reg_class(lo - 1) != (ts, nt)


def test_blocks_beyond_256(lib):
    for M, want in fu.BLOCKED_BIG.items():
        for batch in (1, 3):
            assert fu.blocks(M, _bs(lib, M, batch)) == want, M
        assert sum(want) == M
    cls = {M: [fu.reg_class(b) for b in bl] for M, bl in fu.BLOCKED_BIG.items()}
    assert cls == {257: [(16, 13), (16, 13)], 417: [(32, 7), (16, 13)], 500: [(32, 8), (32, 8)],
                   513: [(16, 13)] * 3, 529: [(16, 13)] * 3}
    # 513 is the first size with three blocks (k >= 2 in the driver); 417 puts a TS = 32 block next to a col0 > 0 one
    assert min(M for M in range(257, 600) if len(fu.blocks(M, _bs(lib, M))) >= 3) == 513


def test_unreachable_instantiations(lib):
    """chol_inv_reg_kernel<1|2|4, 32> and <16, 16> are reached from no entry (TS = 32 needs a block of more than 208
    columns, so NT >= 7; TS = 16 stops at 208 = 13 tiles); the small TS = 16 classes inside an M > 256 run first appear
    at M = 2401, 3121 and 3601"""
    first = {}
    for M in range(1, fu.LA_GLOBAL_MAX + 1):
        for b in fu.blocks(M, _bs(lib, M)):
            assert 1 <= b <= 256
            c = fu.reg_class(b)
            if M > 256:
                first.setdefault(c, M)
            assert c not in ((32, 1), (32, 2), (32, 4), (16, 16)), (M, b)
    assert first[(16, 7)] == 2401 and first[(16, 4)] == 3121 and first[(16, 2)] == 3601
    assert fu.blocks(2401, _bs(lib, 2401))[-1] == 97 and fu.blocks(3121, _bs(lib, 3121))[-1] == 49
    assert fu.blocks(3601, _bs(lib, 3601))[-1] == 17


def test_unfused_and_helper_lists():
    P, T = fu.LA_PACKED_MAX, fu.LA_THREADS
    assert fu.UNFUSED_M[:3] == [P - 1, P, P + 1]
    assert fu.UNFUSED_M[3:] == [T // 4, T // 4 + 1, T // 4 + 2, 2 * (T // 4) + 1]  # tri_inv_body: 256 columns per pass
    assert T + 1 < fu.UNFUSED_LONG_M < fu.LA_GLOBAL_MAX  # rows past 1025 fill rowL, scale and copy in two trips
    assert [fu.bdot_splits(n) for n in fu.BDOT_N] == [1, 1, 2, 32, 32, 32] and fu.bdot_splits(65536 - 2048) == 31
    assert sorted({M * b for M, b in fu.ADD_DIAG}) == [255, 256, 257]
    assert fu.BDOT_BATCH == [1, 64, 65]


CPU_CASES = [("wishart", 33), ("wishart", 113), ("wishart", 208), ("wishart", 257), ("wishart", 417), ("rbf", 64),
             ("rbf", 200), ("rbf", 330), ("graded", 49), ("graded", 200)]


@pytest.mark.parametrize("name,M", CPU_CASES)
def test_reference_and_bounds_on_the_cpu(name, M):
    """LAPACK (torch.linalg, fp64) and a plain fp64 restatement of the two algorithms against the longdouble reference:
    inside every bound, and the bounds are not vacuous"""
    ref = fu.reference(name, M, 0)
    A = torch.from_numpy(ref.A)
    # LAPACK
    L = torch.linalg.cholesky(A)
    X = torch.linalg.solve_triangular(L, torch.eye(M, dtype=f64), upper=False).tril()
    # the restatement
    Lp = fu.chol_f64_plain(ref.A)
    Xp = fu.tri_inv_any(Lp, np.float64)
    got = {}
    for tag, Lh, Xh in (("lapack", L.numpy(), X.numpy()), ("plain", Lp, Xp)):
        got[tag] = (fu.chol_residual_ratio(Lh, ref.A), fu.tri_inv_residual_ratio(Xh, Lh), fu.x_ratio(Xh, ref),
                    fu.logdet_ratio(2.0 * float(np.sum(np.log(np.diag(Lh)))), ref))
        print(f"[factor] cpu {name} M = {M} {tag}: error / bound: Cholesky residual {got[tag][0]:.3f}, inverse residual "
              f"{got[tag][1]:.3f}, X {got[tag][2]:.3f}, logdet {got[tag][3]:.3f}")
        assert max(got[tag]) <= 1, (tag, got[tag])
    # the reference itself: residuals at the longdouble level, far below the fp64 bounds
    Lr, Xr = ref.L.astype(np.float64), ref.X.astype(np.float64)
    assert fu.chol_residual_ratio(Lr, ref.A) <= 1 and fu.tri_inv_residual_ratio(Xr, Lr) <= 1
    assert fu.x_ratio(Xr, ref) <= 0.5 / (M + 4) + 1e-12  # rounding the reference to fp64 is all that is left
    # not vacuous: on the diagonal (X_jj = 1 / L_jj) the bound is a relative one, and on the two families with cond(L) of
    # order 10 after scaling it is 100 times below 2^-26, the level of the hardware's rsq / rcp estimates
    rel = float((np.diag(ref.bX) / np.abs(np.diag(Xr))).max())
    print(f"[factor] cpu {name} M = {M}: largest bound / |X_jj| {rel:.2e}, |bound|_F / |X|_F "
          f"{np.linalg.norm(ref.bX) / np.linalg.norm(Xr):.2e}")
    assert rel < (2.0 ** -26 / 100 if name != "rbf" else 1e-7)


def test_triangular_families_are_tame():
    """the 1 / sqrt(M) scale keeps the triangular inputs' inverses finite and moderate at every size used"""
    for M in (fu.UNFUSED_M[-1], fu.UNFUSED_LONG_M):
        L = fu.matrix("tri", M, 0)
        X = torch.linalg.solve_triangular(L, torch.eye(M, dtype=f64), upper=False)
        assert float(torch.diagonal(L).abs().min()) >= 0.5 and float(X.abs().max()) < 1e6
    d = torch.diagonal(fu.matrix("tri_graded", 258, 0)).abs()
    assert float(d.max() / d.min()) > 1e8


def test_indefinite_inputs_are_what_lapack_reports():
    """the bad-pivot construction: LAPACK's info is j + 1 and a NaN at (i, j) below the diagonal reports i + 1"""
    M = 113
    for j in (0, 15, 16, M - 1):
        assert int(fu.want_info(fu.bad_pivot("wishart", M, 0, j))) == j + 1
    A = fu.matrix("wishart", M, 0).clone()
    A[40, 7] = float("nan")
    assert int(fu.want_info(A)) == 41
    D = torch.eye(M, dtype=f64)
    D[3, 3], D[9, 9] = -1.0, -2.0
    assert int(fu.want_info(D)) == 4
    D[3, 3] = 0.0
    assert int(fu.want_info(D)) == 4
