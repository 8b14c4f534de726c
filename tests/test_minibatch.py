"""Minibatch training, host side: the keyed permutation's restatement (minibatch.feistel_perm), the epoch rule, and the
argument errors of RowSampler and fit(batch_size=...) (no GPU)."""
import numpy as np
import pytest

from spatial_alignment_amd import minibatch as MB
from spatial_alignment_amd import parallel, train
from spatial_alignment_amd.synthetic import make_grid_problem, make_model


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 64, 97, 127, 128, 129, 600, 900, 1000, 1024, 4099,
                               65536, 99991])
def test_feistel_is_a_bijection(N):
    for seed, m, v, e in [(0, 0, 0, 0), (7, 1, 2, 3), (2**62 + 11, 3, 15, 10**9)]:
        p = MB.feistel_perm(np.arange(N), N, seed, m, v, e)
        assert p.dtype == np.int64
        assert np.array_equal(np.sort(p), np.arange(N))


def test_feistel_depends_on_every_key_part():
    N = 1000
    base = MB.feistel_perm(np.arange(N), N, 5, 0, 0, 0)
    assert not np.array_equal(base, np.arange(N))
    for args in [(6, 0, 0, 0), (5, 1, 0, 0), (5, 0, 1, 0), (5, 0, 0, 1)]:
        assert not np.array_equal(MB.feistel_perm(np.arange(N), N, *args), base), args


def test_feistel_pinned_values():
    """the rule is part of the contract (the device kernel restates it): a change shows here.  _mix64 is splitmix64's
    finaliser (its published value at 1)"""
    assert MB._mix64(0) == 0 and MB._mix64(1) == 0x5692161D100B05E5
    assert MB.feistel_perm(np.arange(10), 10, 1234, 1, 2, 3).tolist() == [9, 1, 8, 4, 2, 7, 3, 0, 5, 6]
    assert MB.batch_indices(1000, 7, 42, 0, 1, 500).tolist() == [130, 87, 322, 400, 983, 467, 883]


@pytest.mark.parametrize("N,B", [(600, 200), (900, 150), (12, 1), (12, 12), (1, 1), (1024, 256)])
def test_epoch_partitions_the_view_when_b_divides_n(N, B):
    K = N // B
    for e in range(3):
        rows = np.concatenate([MB.batch_indices(N, B, 9, 1, 0, e * K + k) for k in range(K)])
        assert np.array_equal(np.sort(rows), np.arange(N))


@pytest.mark.parametrize("N,B", [(1000, 300), (7, 2), (97, 96)])
def test_drop_last_epochs(N, B):
    """B does not divide N: every batch has distinct rows, an epoch's K batches are disjoint, and the next epoch is
    another permutation"""
    K = N // B
    ep = [np.concatenate([MB.batch_indices(N, B, 3, 0, 1, e * K + k) for k in range(K)]) for e in range(2)]
    for rows in ep:
        assert len(rows) == K * B and len(np.unique(rows)) == K * B and rows.min() >= 0 and rows.max() < N
    assert not np.array_equal(ep[0], ep[1])


def _cpu_problem():
    dd = make_grid_problem(side=6, n_views=2, n_outputs=3)
    return dd, make_model(dd, m=9)


@pytest.mark.parametrize("bad", [0, 37, -1, 2.5, True, {"expression": [4]}, {"expression": [4, 0]},
                                 {"expression": [4, 40]}, {"other": [4, 4]}])
def test_sampler_rejects_batch_sizes(bad):
    dd, model = _cpu_problem()
    with pytest.raises(ValueError):
        MB.RowSampler(model, dd, bad)


def test_sampler_rejects_data():
    dd, model = _cpu_problem()
    d = dd["expression"]
    with pytest.raises(ValueError, match="float32"):
        MB.RowSampler(model, {"expression": dict(d, outputs=d["outputs"].double())}, 4)
    with pytest.raises(ValueError, match="views"):
        MB.RowSampler(model, {"expression": dict(d, n_samples_list=[12, 12, 12])}, 4)
    with pytest.raises(ValueError, match="sums to"):
        MB.RowSampler(model, {"expression": dict(d, n_samples_list=[30, 30])}, 4)
    with pytest.raises(ValueError):
        MB.RowSampler(model, {"other": d}, 4)
    with pytest.raises(ValueError, match="seed"):
        MB.RowSampler(model, dd, 4, seed=-1)
    with pytest.raises(ValueError, match="HIP device"):  # valid arguments, but the model is not on a device
        MB.RowSampler(model, dd, 4)


def test_fit_batch_size_with_a_reducer_raises():
    dd, model = _cpu_problem()

    class R:
        with_loss = True

    with pytest.raises(ValueError, match="batch_size"):
        train.fit(model, dd, 1, batch_size=4, reducer=R())
    with pytest.raises(ValueError, match="batch_size"):
        parallel.fit(model, dd, 1, batch_size=4)


def test_host_rows_are_global_and_per_view():
    """RowSampler.host_rows on a stand-in for the device state: view v's rows sit in its own block of the modality"""
    s = MB.RowSampler.__new__(MB.RowSampler)
    s.mods, s.seed = ["a", "b"], 4
    s.views = {"a": [10, 20], "b": [5, 5]}
    s.batch_size = {"a": [5, 4], "b": [5, 2]}
    r = s.host_rows(3)
    assert r["a"].shape == (9,) and r["b"].shape == (7,)
    assert ((r["a"][:5] >= 0) & (r["a"][:5] < 10)).all() and ((r["a"][5:] >= 10) & (r["a"][5:] < 30)).all()
    assert set(r["b"][:5]) == set(range(5))  # B = N: the whole view
    assert np.array_equal(r["a"][5:], 10 + MB.batch_indices(20, 4, 4, 0, 1, 3))
    assert np.array_equal(r["b"][5:], 5 + MB.batch_indices(5, 2, 4, 1, 1, 3))
