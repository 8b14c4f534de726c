"""The shape arithmetic behind tests/test_fp64_products_gpu.py and test_longk_f64, without a GPU: the library's own
queries, with the 256 compute units num_cus() assumes when no device answers (the MI355X's count), must take every shape
the GPU tests name for a kernel and decline every shape they name as declined.  A shape list that would make a GPU test
skip, or assert on a shape its kernel does not run, fails here first."""
import pytest
import torch

import fp64_products_util as fu

CUS = 256


@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, "these sums are written for 256 CUs"
    from spatial_alignment_amd import _lib

    return _lib.load()


def test_row_counts_are_the_edges_of_the_row_tile_classes():
    classes = [2, 4, 7, 13, 16, 24]
    assert fu.CLASS_LASTS == [16 * mb for mb in classes[:5]]
    assert fu.CLASS_FIRSTS == [1] + [16 * mb + 1 for mb in classes[:4]]
    assert fu.WHITEN_STREAMED[0] == 16 * 16 + 1 and fu.WHITEN_STREAMED[-1] == 16 * 24
    for M, mb in zip(fu.RAGGED, classes):  # one ragged last tile in each class
        assert M % 16 != 0 and (classes[classes.index(mb) - 1] if mb > 2 else 0) < -(-M // 16) <= mb


def test_whiten_workspace_covers_the_named_rows(lib):
    classes = [2, 4, 7, 13, 16, 24]
    for M in fu.ROWS_WHITEN + [20]:
        mb = next(c for c in classes if -(-M // 16) <= c)
        assert int(lib.gpsa_whiten_workspace(M)) == (16 * mb) ** 2 * 8, M
    assert int(lib.gpsa_whiten_workspace(385)) == 0


def test_longk_shapes_are_taken(lib):
    for M, K, n in fu.LONGK_SHAPES:  # test_longk_f64: none of its shapes may be declined
        assert int(lib.gpsa_longk_f64_workspace(M, K, n)) > 0, (M, K, n)
    k0 = {n: fu.longk_k0(lib, 100, n) for n in fu.LONGK_NPROB}
    assert all(k % 2 == 0 and k >= 512 for k in k0.values()) and k0[48] <= k0[4] <= k0[1], k0
    for n in fu.LONGK_NPROB:
        for M in fu.ROWS_256:
            assert fu.longk_k0(lib, M, n) == k0[n], (M, n)  # the rule does not depend on the row count
            for K in (k0[n], k0[n] + 2, k0[n] + 14):
                assert int(lib.gpsa_longk_f64_workspace(M, K, n)) > 0, (M, K, n)
    # every row-tile class is reached by a listed shape and by the sweep
    assert {2, 4, 7, 13, 16} == {next(c for c in (2, 4, 7, 13, 16) if -(-M // 16) <= c) for M, _, _ in fu.LONGK_SHAPES}


def test_longk_declined_shapes_are_declined(lib):
    k0 = fu.longk_k0(lib, 100, 1)
    assert k0 > 514
    for M, K, n in ((100, k0 + 1, 1), (100, 510, 1), (100, k0 - 2, 1), (257, k0, 1), (257, 100000, 4), (100, k0, 49),
                    (25, 1000, 3), (256, 2048, 1)):  # (the last two: the shapes test_longk_f64 used to skip on)
        assert int(lib.gpsa_longk_f64_workspace(M, K, n)) == 0, (M, K, n)


def test_whiten_threshold_columns():
    cols = fu.whiten_threshold_columns(CUS)
    cdiv = lambda a, b: -(-a // b)
    assert [cdiv(c, 32) <= CUS for c in cols] == [True, True, False, False, False]  # row-split | resident
    assert [cdiv(c, 64) <= CUS for c in cols] == [True, True, True, True, False]  # resident | streaming
    assert all(8192 < c <= 16384 + 1 for c in cols[2:])  # the resident kernel's range no other test enters
    c3 = 32 * (CUS // 3)
    assert cdiv(c3, 32) * 3 <= CUS < cdiv(c3 + 32, 32) * 3
    for batch in (1, 2):
        c0 = fu.persistent_c0(CUS, batch)
        assert batch * cdiv(c0, 64) == 6 * CUS and batch * cdiv(c0 - 1, 64) == 6 * CUS - batch and c0 % 64 == 1
    assert fu.persistent_c0(CUS) * 208 * 8 < 170e6  # "about 160 MB each"


def test_gemm_triples_cover_every_listed_size(lib):
    assert len(fu.GEMM_TRIPLES) == len(set(fu.GEMM_TRIPLES)) == 25
    assert {m for m, _, _ in fu.GEMM_TRIPLES} == set(fu.GEMM_MN) == {n for _, n, _ in fu.GEMM_TRIPLES}
    assert {k for _, _, k in fu.GEMM_TRIPLES} == set(fu.GEMM_K)
    assert int(lib.gpsa_gemm_workspace(1, 33, 65, 3, 7)) == 3 * 7 * 33 * 65 * 8
    assert int(lib.gpsa_gemm_workspace(0, 33, 65, 1, 64)) == 64 * 33 * 65 * 4
    assert int(lib.gpsa_gemm_workspace(1, 33, 65, 3, 1)) == 0
    # exact dK_uu: unsplit below 128 columns, 64 slices at 4097
    assert int(lib.gpsa_exact_dkuu_workspace(113, 63)) == 0 == int(lib.gpsa_exact_dkuu_workspace(113, 64))
    assert int(lib.gpsa_exact_dkuu_workspace(113, 4097)) == 64 * 113 * 113 * 8


def test_the_bar_and_the_ratio():
    """the helper itself: a bound of zero demands equality, NaN never passes, the fp32 term is added"""
    want = torch.tensor([1.0, 0.0, -2.0], dtype=fu.f64)
    ab = torch.tensor([1.0, 0.0, 2.0], dtype=fu.f64)
    b = fu.bar(4, ab)
    assert torch.equal(b, 16 * fu.U64 * ab)
    assert fu.ratio(want, want, b) == 0.0
    assert fu.ratio(want + torch.tensor([8 * fu.U64, 0.0, 0.0], dtype=fu.f64), want, b) == pytest.approx(0.5)
    assert fu.ratio(want + torch.tensor([0.0, 1e-300, 0.0], dtype=fu.f64), want, b) == float("inf")
    assert fu.ratio(torch.tensor([1.0, float("nan"), -2.0], dtype=fu.f64), want, b) == float("inf")
    assert torch.equal(fu.bar(4, ab, want32=want), b + fu.U32 * want.abs())
    assert torch.equal(fu.bar(4, ab, c0=want, beta=-0.5), 16 * fu.U64 * (ab + 0.5 * want.abs()))
