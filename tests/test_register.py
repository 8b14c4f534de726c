"""Rigid pre-registration without a device: the yardstick of tests/register_util.py held to facts (exact arithmetic on a
lattice, planted poses recovered), every seeded input of tests/test_register_gpu.py shown to be DECISIVE - so that the
device comparisons there may ask for equal indices - and the plumbing: the C ABI's declaration and binding, the custom
op's shapes, the exports, the refusals that need no device.  The kernels are exercised by tests/test_register_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import gpsa
import neighbors_util as nu
import register_util as ru
import spatial_alignment_amd as pkg
from spatial_alignment_amd import _lib, register

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = torch.float64
NAMES = ("rigid_scores", "rigid_register", "RigidRegistration", "prealign_slices")


# ------------------------------------------------------------------------------------------------------------------------
# the yardstick: exact on a lattice
# ------------------------------------------------------------------------------------------------------------------------
def test_on_a_lattice_every_tie_goes_to_the_lower_index_and_the_self_match_scores_zero():
    case = ru.lattice_case()
    ref, XA, T = case["ref"], case["XA"], case["T"]
    n = len(XA)
    tied = 0
    for k in range(len(T)):
        q = ru.transform(T[k], case["XB"])
        assert np.array_equal(q * 2, np.round(q * 2))  # multiples of 1/2: every operation below is exact
        idx, d2 = nu.knn(q, XA, 2)  # np.lexsort on (index, d2): the key's order, stated another way
        assert np.array_equal(ref["nn"][k], idx[:, 0]) and np.array_equal(ref["d2"][k], d2[:, 0])
        assert np.array_equal(ref["d2_second"][k], d2[:, 1])
        ties = d2[:, 1] == d2[:, 0]
        tied += int(ties.sum())
        assert (idx[ties, 0] < idx[ties, 1]).all()
        if k >= 8:  # moved by half a cell: a row sits between four rows of A, two past a border, one past the corner
            assert ties.sum() == n - 1 and (d2[:, 0] == 0.5).all()
        else:  # a symmetry of the lattice: every row lands on a row of A
            assert (d2[:, 0] == 0.0).all() and sorted(ref["nn"][k]) == list(range(n))
    assert tied == 8 * (n - 1)
    # the identity: B's row i is A's row i, and J is exactly 0
    assert np.array_equal(T[0], [1, 0, 0, 1, 0, 0]) and np.array_equal(ref["nn"][0], np.arange(n))
    J = ru.J_of(ref["sse"], ref["n_matched"], n, 3, 0.5)
    assert J[0] == 0.0 and ref["n_matched"][0] == n and ref["d2_sum"][0] == 0.0
    assert (J[1:8] > 0).all()  # the other symmetries put other rows' expression on a spot
    assert (ref["d2_sum"][8:] == 0.5 * n).all() and (ref["n_matched"] == n).all()


def test_the_yardstick_agrees_with_the_neighbour_yardstick_on_seeded_points():
    case = ru.contract_case("typical")
    ref = case["ref"]
    for k in (0, 7, 18):
        idx, d2 = nu.knn(ru.transform(case["T"][k], case["XB"]), case["XA"], 2)
        assert np.array_equal(ref["nn"][k], idx[:, 0]) and np.array_equal(ref["d2"][k], d2[:, 0])
        hit = d2[:, 0] <= case["max_d2"]
        assert ref["n_matched"][k] == hit.sum() and 0.2 < hit.mean() < 0.95
        diff = case["YB"][hit].astype(np.float64) - case["YA"][idx[hit, 0]].astype(np.float64)
        assert abs(ref["sse"][k] - (diff**2).sum()) <= 1e-12 * ref["sse"][k]


def test_a_nan_coordinate_leaves_the_row_unmatched():
    case = ru.contract_case("typical/nan-in-B")
    ref, n = case["ref"], len(case["XB"])
    for i in (5, n - 1):
        assert (ref["d2"][:, i] == np.inf).all() and (ref["nn"][:, i] == 0).all()
    clean = ru.contract_case("typical")["ref"]
    assert (ref["n_matched"] <= clean["n_matched"]).all() and np.isfinite(ref["sse"]).all()


# ------------------------------------------------------------------------------------------------------------------------
# the yardstick: planted poses
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ru.PLANTED))
def test_a_planted_pose_is_recovered(name):
    case, ref = ru.planted_case(name), ru.planted_reference(name)
    aligned = case["XB"] @ ref["R"].T + ref["t"]
    rms = float(np.sqrt(((aligned - case["origin"]) ** 2).sum(1).mean())) / ref["spacing"]
    hit = float((ref["nn"] == case["planted"]).mean())
    scores = [ref["score_coarse"]] + [s for _, s in ref["path"]]
    Jc = ref["coarse"]
    print(f"[register yardstick] {name}: reflected {ref['reflected']} (planted {case['mirrored']}), angle "
          f"{ref['angle']:.4f}, rms {rms:.3f} spacings (bar 0.5), nn == planted on {hit:.4f} of rows, coarse best "
          f"{ref['score_coarse']:.4f} against median {np.median(Jc[np.isfinite(Jc)]):.3f}, start {ref['score_start']:.3f}, "
          f"final {ref['score']:.4f}, runner-up {ref['runner_up']}")
    assert ref["reflected"] == case["mirrored"]
    assert rms < 0.5
    if name in ru.PLANTED_TIGHT:
        assert hit >= 0.98
    assert all(b <= a for a, b in zip(scores, scores[1:])), scores
    assert ref["score"] == scores[-1] and ref["score"] < 0.2 * ref["score_start"]
    assert len(ref["path"]) == 6 and all(0 <= p < 75 for p, _ in ref["path"])
    # the runner-up is another pose, and a worse one
    assert ref["runner_up"] is not None and ref["runner_up"][2] >= ref["score_coarse"]


# ------------------------------------------------------------------------------------------------------------------------
# decisiveness: what lets the device tests ask for equal indices and equal choices
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ru.CONTRACT_SHAPES) + list(ru.CONTRACT_VARIANTS))
def test_every_contract_input_is_decisive(name):
    case = ru.contract_case(name)
    bad = ru.undecided_rows(case["ref"], case["max_d2"])
    assert bad.shape == case["ref"]["d2"].shape and int(bad.sum()) == 0


@pytest.mark.parametrize("name", sorted(ru.PLANTED))
def test_every_planted_input_is_decisive_at_every_level(name):
    ref = ru.planted_reference(name)
    assert len(ref["stages"]) == 7
    assert [st["undecided"] for st in ref["stages"]] == [0] * 7 and ref["final_undecided"] == 0
    assert not any(ru.undecided_stage(st) for st in ref["stages"])


def test_the_lattice_is_the_exception_its_moved_half_is_tied():
    case = ru.lattice_case()
    bad = ru.undecided_rows(case["ref"], case["max_d2"])
    assert bad[8:].sum() == 8 * (bad.shape[1] - 1) and not bad[:8].any()


# ------------------------------------------------------------------------------------------------------------------------
# the plumbing
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,res,n_args", [("gpsa_rigid_scores_workspace", "long long", 6),
                                             ("gpsa_rigid_scores_f64", "int", 19)])
def test_the_entry_is_in_the_header_in_signatures_and_in_the_library(name, res, n_args):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpsa_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/gpsa_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is (_lib._ll if res == "long long" else _lib._i)
    assert len(args) == n_args == len(argtypes)
    for a, t in zip(args, argtypes):
        want = _lib._vp if "*" in a else _lib._ll if a.startswith("long long") else _lib._d if a.startswith("double") \
            else _lib._i
        assert t is want, (name, a, t)
    assert hasattr(_lib.load(), name)
    src = open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "register.hip")).read()
    assert re.search(r"\b" + res + r"\s+" + name + r"\s*\(", src)


def test_the_workspace_query_and_the_refusals_before_any_launch():
    import ctypes as C

    lib = _lib.load()
    q = lib.gpsa_rigid_scores_workspace
    n, m, K, P = 1000, 5000, 20, 50
    G = -(-n // max(ru.RG_GROUP_MIN, -(-n // ru.RG_MAX_GROUPS)))
    assert q(n, m, K, P, 1, 1) == 24 * K * G
    assert q(n, m, K, P, 1, 0) == 24 * K * G + 12 * K * n
    assert q(n, m, K, P, 3, 0) == 24 * K * G + 12 * K * n + 3 * 12 * K * n
    assert q(n, m, K, P, 0, 1) >= q(n, m, K, P, 1, 1)
    assert q(0, m, K, P, 1, 1) == 0 and q(n, m, 70000, P, 1, 1) == 0
    # the dummy address 8 is never dereferenced: every refusal comes back before a launch
    p, call = C.c_void_p(8), lib.gpsa_rigid_scores_f64
    good = dict(XA=p, YA=p, m=m, XB=p, YB=p, n=n, P=P, T=p, K=K, max_d2=1.0, parts=1, sse=p, nm=p, ds=p, nn=p, d2=p, ws=p,
                wsb=1 << 40, st=None)
    for change, want in ((dict(XA=None), _lib.GPSA_EINVAL), (dict(nn=None), _lib.GPSA_EINVAL), (dict(n=0), _lib.GPSA_EINVAL),
                         (dict(max_d2=-1.0), _lib.GPSA_EINVAL), (dict(max_d2=float("nan")), _lib.GPSA_EINVAL),
                         (dict(max_d2=float("inf")), _lib.GPSA_EINVAL), (dict(parts=-1), _lib.GPSA_EINVAL),
                         (dict(K=65536), _lib.GPSA_EUNSUPPORTED), (dict(wsb=24 * K * G - 8), _lib.GPSA_EWORKSPACE),
                         (dict(ws=None), _lib.GPSA_EWORKSPACE)):
        assert call(*dict(good, **change).values()) == want, change


def test_the_custom_op_propagates_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers the op)

    with FakeTensorMode():
        e = lambda *sh, dt=f64: torch.empty(*sh, dtype=dt, device="cuda")
        args = (e(900, 2), e(900, 50, dt=torch.float32), e(700, 2), e(700, 50, dt=torch.float32), e(19, 6), 0.3)
        sse, nm, ds, nn, d2 = torch.ops.gpsa.rigid_scores(*args, 0, True)
        assert (sse.shape, nm.shape, ds.shape, nn.shape, d2.shape) == ((19,), (19,), (19,), (19, 700), (19, 700))
        assert (sse.dtype, nm.dtype, ds.dtype, nn.dtype, d2.dtype) == (f64, torch.int64, f64, torch.int32, f64)
        assert torch.ops.gpsa.rigid_scores(*args)[3].numel() == 0


def test_the_exports():
    for name in NAMES:
        assert name in pkg.__all__ and name in gpsa.__all__ and getattr(gpsa, name) is getattr(register, name)


def test_refusals_that_need_no_device():
    X, Y = torch.rand(40, 2), torch.rand(40, 3)
    T = torch.tensor([[1.0, 0, 0, 1, 0, 0]], dtype=f64)
    with pytest.raises(ValueError, match=r"D = 3.*slice by slice"):
        register.rigid_register(torch.rand(40, 3), Y, X, Y)
    with pytest.raises(ValueError, match=r"slice by slice"):
        register.prealign_slices(torch.rand(40, 3), Y, [20, 20])
    with pytest.raises(ValueError, match=r"P = 3 .* P = 5"):
        register.rigid_register(X, Y, X, torch.rand(40, 5))
    with pytest.raises(ValueError, match=r"YB has shape .*\[40, P >= 1\]"):
        register.rigid_scores(X, Y, X, torch.rand(39, 3), T, 1.0)
    with pytest.raises(ValueError, match=r"transforms has shape .*\(1, 5\)"):
        register.rigid_scores(X, Y, X, Y, T[:, :5], 1.0)
    with pytest.raises(ValueError, match="max_dist must be finite and >= 0, not -1.0"):
        register.rigid_scores(X, Y, X, Y, T, -1.0)
    with pytest.raises(ValueError, match="candidates_per_chunk must be an integer >= 1, not 0"):
        register.rigid_scores(X, Y, X, Y, T, 1.0, candidates_per_chunk=0)
    with pytest.raises(ValueError, match="n_angles must be an integer >= 1, not 0"):
        register.rigid_register(X, Y, X, Y, n_angles=0)
    with pytest.raises(ValueError, match=r"min_overlap must be in \(0, 1\], not 1.5"):
        register.rigid_register(X, Y, X, Y, min_overlap=1.5)
    with pytest.raises(ValueError, match=r"n_samples_list = \[20, 30\]"):
        register.prealign_slices(X, Y, [20, 30])
    with pytest.raises(ValueError, match=r"reference must be a view index in \[0, 2\), not 2"):
        register.prealign_slices(X, Y, [20, 20], reference=2)
    for call in (lambda: register.rigid_scores(X, Y, X, Y, T, 1.0), lambda: register.rigid_register(X, Y, X, Y),
                 lambda: register.prealign_slices(X, Y, [20, 20])):
        with pytest.raises(ValueError, match="device 'cpu'"):
            call()
