"""Rigid pre-registration on the device: ``gpsa_rigid_scores_f64`` (csrc/register.hip) against the numpy fp64 yardstick of
tests/register_util.py on shapes around every constant its kernels introduce, then ``rigid_register`` and
``prealign_slices`` on the planted cases of tests/test_register.py.

The constants (restated in register_util): a scan workgroup takes RG_ROWS = 256 rows of B, A passes through LDS in
tiles of RG_TILE = 1024 rows, a thread carries RG_C = 8 candidates, the closing kernel's lanes run over 16 genes for
P <= 16 and 64 otherwise, the sums meet in ceil(n / max(32, ceil(n / 32))) row groups (n = 1024: 32 groups of 32 rows;
n = 1025: groups of 33, the last one short), and the A axis is cut into `parts` slices (at most 64, at most m).

Bars (tests/test_register.py shows on the CPU that every seeded input here has NO undecided row and no undecided level,
the lattice excepted, whose arithmetic is exact):
* nn: EQUAL to the yardstick's, every row;  n_matched: equal;
* d2: 1e-12 max(1, d2) (the entry's fused multiply-adds against numpy's separate roundings: a few 1.1e-16);
* sse, d2_sum: 1e-11 of the sum of the terms' magnitudes - the terms are squares, so of the value itself - the bar of
  the project's other fixed-order fp64 sums;
* repeats, every `parts`, every ``candidates_per_chunk``: ``torch.equal``;
* the lattice: equal bit for bit, ties included;
* the whole call: the chosen index of every level equal to the yardstick's, R and t within 1e-12, and the recovery bars
  of the CPU test asserted on the device's own result."""
import math

import numpy as np
import pytest
import torch

import register_util as ru
import spatial_alignment_amd as gp
from spatial_alignment_amd import _lib, register

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64, f32 = torch.float64, torch.float32
PARTS = (0, 1, 2, 3, 64)  # 0: the entry's own choice; 64: its cap (fewer where A has fewer rows)
assert (ru.RG_ROWS, ru.RG_TILE, ru.RG_C, ru.RG_LANES) == (256, 1024, 8, (16, 64))


def _ops():
    from spatial_alignment_amd import ops

    return ops.get_ops()


def _dev(case):
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()
    return t(case["XA"], f64), t(case["YA"], f32), t(case["XB"], f64), t(case["YB"], f32)


def _entry(case, parts=0, T=None):
    """the entry with its tables -> (sse, n_matched, d2_sum, nn, d2) on the device"""
    T = torch.tensor(case["T"] if T is None else T, dtype=f64, device=DEV)
    return _ops().rigid_scores(*_dev(case), T, case["max_d2"], parts=parts, return_nn=True)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _against_the_yardstick(name, got, ref):
    sse, nm, ds, nn, d2 = (t.cpu().numpy() for t in got)
    assert nn.dtype == np.int32 and nn.shape == ref["nn"].shape
    assert np.array_equal(nn, ref["nn"]), f"{name}: {(nn != ref['nn']).sum()} neighbours differ"
    fin = np.isfinite(ref["d2"])
    assert np.array_equal(np.isinf(d2), ~fin) and (d2[~fin] > 0).all()
    err_d2 = float((np.abs(d2[fin] - ref["d2"][fin]) / np.maximum(1.0, ref["d2"][fin])).max()) if fin.any() else 0.0
    assert np.array_equal(nm, ref["n_matched"])
    err_sse = float((np.abs(sse - ref["sse"]) / np.where(ref["sse"] > 0, ref["sse"], 1.0)).max())
    err_ds = float((np.abs(ds - ref["d2_sum"]) / np.where(ref["d2_sum"] > 0, ref["d2_sum"], 1.0)).max())
    print(f"[register] {name}: d2 {err_d2:.2e} (bar 1e-12), sse {err_sse:.2e}, d2_sum {err_ds:.2e} (bar 1e-11 of the "
          f"terms' sum), matched {int(nm.min())}..{int(nm.max())} of {nn.shape[1]}")
    assert err_d2 <= 1e-12
    assert err_sse <= 1e-11 and err_ds <= 1e-11  # (a sum of no terms: exactly 0)


# ------------------------------------------------------------------------------------------------------------------------
# the kernel contract
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ru.CONTRACT_SHAPES) + list(ru.CONTRACT_VARIANTS))
def test_the_entry_against_the_yardstick(name):
    case = ru.contract_case(name)
    got = _entry(case)
    _against_the_yardstick(name, got, case["ref"])
    n = len(case["XB"])
    if name.endswith("none-matched"):
        assert int(got[1].max()) == 0 and float(got[0].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
    if name.endswith("all-matched"):
        assert int(got[1].min()) == n
    if name.endswith("nan-in-B"):
        assert torch.isinf(got[4][:, 5]).all() and torch.isinf(got[4][:, n - 1]).all() and int(got[1].max()) <= n - 2
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all())
    # the same bits: a repeat, every split of the A axis
    assert _same(got, _entry(case))
    for parts in PARTS:
        assert _same(got, _entry(case, parts=parts)), parts
    # ... and every chunking of the candidates, through the public call (max_dist is squared there: within an ulp of
    # max_d2, and no row is that close to it)
    K = len(case["T"])
    XA, YA, XB, YB = _dev(case)
    T = torch.tensor(case["T"], dtype=f64, device=DEV)
    whole = None
    for chunk in sorted({1, 3, K}):
        r = gp.rigid_scores(XA, YA, XB, YB, T, math.sqrt(case["max_d2"]), return_nn=True, candidates_per_chunk=chunk)
        now = (r.sse, r.n_matched, r.d2_sum, r.nn, r.d2)
        whole = now if whole is None else whole
        assert _same(whole, now), chunk
    assert torch.equal(whole[3], got[3]) and torch.equal(whole[1], got[1]) and torch.equal(whole[0], got[0])
    # a candidate's outputs do not depend on the rows of T beside it
    k = K // 2
    alone = _entry(case, T=case["T"][k: k + 1])
    assert _same(alone, tuple(t[k: k + 1] for t in got))
    # without the tables the scores are the same bits
    lean = _ops().rigid_scores(XA, YA, XB, YB, T, case["max_d2"])
    assert lean[3] is None and lean[4] is None and _same(lean[:3], got[:3])


def test_the_lattice_bit_for_bit():
    case = ru.lattice_case()
    ref = case["ref"]
    got = _entry(case)
    sse, nm, ds, nn, d2 = (t.cpu().numpy() for t in got)
    assert np.array_equal(nn, ref["nn"]) and np.array_equal(d2, ref["d2"])
    assert np.array_equal(sse, ref["sse"]) and np.array_equal(ds, ref["d2_sum"]) and np.array_equal(nm, ref["n_matched"])
    assert sse[0] == 0.0 and np.array_equal(nn[0], np.arange(nn.shape[1]))  # the self-match: J exactly 0
    assert (d2[8:] == 0.5).all()  # every row tied (the yardstick's ties go to the lower index: tests/test_register.py)
    for parts in PARTS:
        assert _same(got, _entry(case, parts=parts)), parts


def test_the_symbol_is_in_the_header_in_signatures_and_in_the_library():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "gpsa_rigid_scores_f64(" in open(os.path.join(root, "include", "gpsa_hip.h")).read()
    assert "gpsa_rigid_scores_f64" in _lib.SIGNATURES and hasattr(_lib.load(), "gpsa_rigid_scores_f64")


# ------------------------------------------------------------------------------------------------------------------------
# the whole call
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ru.PLANTED))
def test_a_planted_pose_is_recovered_on_the_device(name):
    case, ref = ru.planted_case(name), ru.planted_reference(name)
    XA, YA, XB, YB = _dev(case)
    reg = gp.rigid_register(XA, YA, XB, YB)
    assert isinstance(reg, gp.RigidRegistration)
    # the yardstick's choices, level by level
    assert [p for p, _ in reg.path] == [p for p, _ in ref["path"]]
    R, t = reg.R.cpu().numpy(), reg.t.cpu().numpy()
    err = max(float(np.abs(R - ref["R"]).max()), float(np.abs(t - ref["t"]).max()))
    scores = [reg.score_coarse] + [s for _, s in reg.path]
    err_s = max(abs(a - b) / b for a, b in zip(scores + [reg.score_start], [ref["score_coarse"]] + [s for _, s in ref["path"]]
                                               + [ref["score_start"]]))
    print(f"[register] {name}: R, t against the yardstick {err:.2e} (bar 1e-12), scores {err_s:.2e} relative")
    assert err <= 1e-12 and err_s <= 1e-11
    assert abs(reg.spacing - ref["spacing"]) <= 1e-13 and abs(reg.max_dist - 3 * reg.spacing) == 0.0
    assert reg.reflected == ref["reflected"] and abs(reg.angle - ref["angle"]) <= 1e-12
    assert np.array_equal(reg.nn.cpu().numpy(), ref["nn"]) and reg.n_matched == ref["n_matched"]
    assert np.array_equal(reg.matched.cpu().numpy(), ref["matched"])
    assert tuple(reg.coarse_scores.shape) == (2, 360, 1, 1)
    Jc, fin = reg.coarse_scores.reshape(-1).cpu().numpy(), np.isfinite(ref["coarse"])
    assert np.array_equal(np.isinf(Jc), ~fin) and float(np.abs(Jc[fin] / ref["coarse"][fin] - 1.0).max()) <= 1e-11
    assert reg.runner_up[1] == ref["runner_up"][1] and abs(reg.runner_up[0] - ref["runner_up"][0]) <= 1e-12
    # the recovery bars, on the device's own result
    aligned = reg.apply(XB)
    assert torch.equal(aligned, XB @ reg.R.T + reg.t)
    rms = float((aligned.cpu() - torch.tensor(case["origin"])).square().sum(1).mean().sqrt()) / reg.spacing
    hit = float((reg.nn.cpu().numpy() == case["planted"]).mean())
    print(f"[register] {name}: reflected {reg.reflected}, rms {rms:.3f} spacings (bar 0.5), nn == planted on {hit:.4f}")
    assert reg.reflected == case["mirrored"] and rms < 0.5
    if name in ru.PLANTED_TIGHT:
        assert hit >= 0.98
    assert all(b <= a for a, b in zip(scores, scores[1:])) and reg.score == scores[-1]
    # apply's round trip: R is orthogonal
    back = (aligned - reg.t) @ reg.R
    assert float((back - XB).abs().max()) <= 1e-12 * float(XB.abs().max())
    # the chunking of the candidates changes nothing
    again = gp.rigid_register(XA, YA, XB, YB, candidates_per_chunk=100)
    assert torch.equal(again.R, reg.R) and torch.equal(again.t, reg.t) and again.path == reg.path
    assert torch.equal(again.coarse_scores, reg.coarse_scores)


def _three_views():
    """view 0 = A of a planted case, view 1 = its B, view 2 = rows of B turned and shifted once more"""
    case = ru.planted_case("p10-80-1.45-mirrored")
    rng = np.random.default_rng(11)
    keep = rng.permutation(len(case["XB"]))[:400]
    c, s = math.cos(2.2), math.sin(2.2)
    X2 = case["XB"][keep] @ np.array([[c, -s], [s, c]]).T + np.array([3.0, 9.0])
    Y2 = case["YB"][keep] + (0.1 * rng.normal(size=(400, case["YB"].shape[1]))).astype(np.float32)
    X = np.concatenate([case["XA"], case["XB"], X2])
    Y = np.concatenate([case["YA"], case["YB"], Y2])
    origin = np.concatenate([case["XA"], case["origin"], case["origin"][keep]])
    return X, Y, [len(case["XA"]), len(case["XB"]), 400], origin


@pytest.mark.parametrize("chain", [False, True])
def test_prealign_slices_on_three_views(chain):
    X, Y, counts, origin = _three_views()
    Xd, Yd = torch.tensor(X, dtype=f64, device=DEV), torch.tensor(Y, dtype=f32, device=DEV)
    aligned, regs = gp.prealign_slices(Xd, Yd, counts, reference=0, chain=chain)
    assert aligned.shape == Xd.shape and aligned.dtype == f64 and len(regs) == 3 and regs[0] is None
    offs = np.cumsum([0] + counts)
    assert torch.equal(aligned[: counts[0]], Xd[: counts[0]])  # the reference view stays where it is
    for v in (1, 2):
        rows = slice(int(offs[v]), int(offs[v + 1]))
        assert torch.equal(aligned[rows], regs[v].apply(Xd[rows]))
        rms = float((aligned[rows].cpu() - torch.tensor(origin[rows])).square().sum(1).mean().sqrt()) / regs[v].spacing
        print(f"[register] prealign chain={chain} view {v}: reflected {regs[v].reflected}, angle {regs[v].angle:.4f}, "
              f"rms {rms:.3f} spacings (bar 0.5), J {regs[v].score:.4f}")
        assert rms < 0.5 and regs[v].reflected
    one = gp.rigid_register(Xd[: counts[0]], Yd[: counts[0]], Xd[offs[1]: offs[2]], Yd[offs[1]: offs[2]])
    assert torch.equal(regs[1].R, one.R) and torch.equal(regs[1].t, one.t)
    if chain:  # view 2 was registered onto view 1 (a plain rotation), and the transforms composed
        assert not bool(regs[2].pair_R.det() < 0)
        assert torch.equal(regs[2].R, regs[1].R @ regs[2].pair_R)
        assert torch.equal(regs[2].t, regs[1].R @ regs[2].pair_t + regs[1].t)
    # the reference in the middle: views 0 and 2 come onto view 1
    aligned1, regs1 = gp.prealign_slices(Xd, Yd, counts, reference=1, chain=chain)
    assert regs1[1] is None and torch.equal(aligned1[offs[1]: offs[2]], Xd[offs[1]: offs[2]])
    assert regs1[0].reflected and not regs1[2].reflected


def test_every_refusal():
    case = ru.planted_case("p3-80-1.45")
    XA, YA, XB, YB = _dev(case)
    with pytest.raises(ValueError, match=r"XB has D = 3 .*slice by slice"):
        gp.rigid_register(XA, YA, torch.cat([XB, XB[:, :1]], 1), YB)
    with pytest.raises(ValueError, match=r"P = 3 outputs and YB P = 2"):
        gp.rigid_register(XA, YA, XB, YB[:, :2].contiguous())
    bad = XB.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match=r"XB has 1 entries that are NaN or infinite"):
        gp.rigid_register(XA, YA, bad, YB)
    bad = YA.clone()
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError, match=r"YA has 1 entries that are NaN or infinite"):
        gp.rigid_register(XA, bad, XB, YB)
    with pytest.raises(ValueError, match=r"min_overlap = 0.5 .*max_dist = 1e-06"):
        gp.rigid_register(XA, YA, XB, YB, max_dist=1e-6, n_angles=16)
    with pytest.raises(ValueError, match="device 'cpu'"):
        gp.rigid_register(XA.cpu(), YA, XB, YB)
    with pytest.raises(ValueError, match="max_d2 must be finite and >= 0"):
        _ops().rigid_scores(XA, YA, XB, YB, torch.zeros(1, 6, dtype=f64, device=DEV), float("inf"))
    with pytest.raises(ValueError, match=r"D = 2 is needed"):
        _ops().rigid_scores(torch.cat([XA, XA[:, :1]], 1), YA, XB, YB, torch.zeros(1, 6, dtype=f64, device=DEV), 1.0)
