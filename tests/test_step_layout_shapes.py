"""Host side of tests/test_step_layout_gpu.py, without a GPU: every layout case still lands on the edge it is named
for (gpsa_step_describe builds the plan gpsa_step_create does), its inputs keep the fp64 reference's own error derivable
(the kappa condition of step_layout_util.py), and the reference is sound on its own - its KL terms add up to the
oracle's negative ELBO, its gradient agrees with central differences where the oracle has no KL (a free view without
rows)."""
import pytest
import torch

import step_layout_util as U
from oracle import gpsa_oracle as orc

CASE_NAMES = list(U.CASES)
# the run lengths the table names (free views in a row, at most 16 per batched launch)
RUNS = {"one_block_ragged": [3], "two_col_blocks": [3], "exact_blocks": [1, 1], "three_col_blocks": [2],
        "empty_in_one_modality": [3], "three_modalities": [2], "empty_everywhere": [3], "seventeen_free": [1, 16, 2],
        "four_dims": [1], "beyond_projection": [2]}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_lands_on_its_edge(name):
    case = U.Case(name)
    rc, got = case.describe()
    assert rc == 0
    want = case.expected()
    assert want["Cs"] == case.Cs                      # the table's column stride, restated from the rows ...
    assert got["Cs"] == case.Cs                       # ... and what the plan derives: Cs / 256 column blocks
    assert case.run_lengths() == RUNS[name]
    assert got["runs"] == len(RUNS[name])
    assert got["eps"] == want["eps"]                  # S D sum(rows of free views): an empty view draws nothing
    assert got["n_kl"] == want["n_kl"]                # V D + sum L: fixed and empty views keep their slots


def test_only_the_large_case_leaves_the_projection_kernel():
    """q = k^T alpha comes from coldot2_kernel exactly where the projection kernel has no workspace for M"""
    from spatial_alignment_amd import _lib

    lib = _lib.load()
    for name in CASE_NAMES:
        case = U.Case(name)
        assert (lib.gpsa_whiten_workspace(case.Mx) == 0) == (name == "beyond_projection"), name
        assert lib.gpsa_whiten_workspace(case.Mg) > 0, name


def test_cases_cover_the_column_block_counts():
    blocks = {n: -(-U.CASES[n]["Cs"] // 256) for n in CASE_NAMES}
    assert blocks["two_col_blocks"] == 2 and blocks["three_col_blocks"] == 3 and blocks["three_modalities"] == 3
    assert U.CASES["exact_blocks"]["Cs"] == 256 and blocks["one_block_ragged"] == 1


@pytest.mark.parametrize("name", CASE_NAMES)
def test_inputs_are_well_conditioned(name):
    case = U.Case(name)
    k = U.kappa(case, case.build())
    print(f"{name}: kappa = {k:.1f}")
    assert k <= U.KAPPA_MAX
    assert 8 * max(case.Mx, case.Mg) * k * 2.0 ** -53 < 3e-11


@pytest.mark.parametrize("name", ["one_block_ragged", "empty_in_one_modality"])
def test_kl_terms_add_up_to_the_oracles_elbo(name):
    """sum_t kl_t minus the log likelihood (the oracle's expression, vgpsa.py:532-538) is negative_elbo"""
    case = U.Case(name)
    inp = case.build()
    st = U._cast_state(inp, grads=False)
    out, h, kl = U.reference_forward(case, inp, st)
    Y = {m: inp["dd"][m]["outputs"].double() for m in case.mods}
    want = orc.negative_elbo(st, inp["cfg"], h, Y, out["F_obs"])
    ll = 0
    n_mod = len(case.mods)
    for i, m in enumerate(case.mods):
        scale = h["noise_variance_pos"][-n_mod + i]
        ll = ll + torch.distributions.Normal(out["F_obs"][m], scale).log_prob(Y[m]).sum() / case.S
    got = kl.sum() - ll
    assert abs(float(got - want)) <= 1e-12 * abs(float(want)), (float(got), float(want))
    fixed = [r for r in range(case.V * case.D) if case.is_fixed(r % case.V)]
    assert all(float(kl[r]) == 0.0 for r in fixed)


def test_reference_gradient_matches_central_differences():
    """empty_everywhere at a reduced size (the oracle alone has no KL for a free view without rows): the fp64 gradient
    of J against central differences, step 1e-6, three random directions per parameter, 1e-6 relative"""
    case = U.Case("small_empty", U.SMALL_EMPTY)
    assert case.nview[1] == 0 and not case.is_fixed(1)
    inp = case.build()
    ref = U.reference(case, inp)

    def J_at(over):
        st = U._cast_state(inp, overrides=over, grads=False)
        out, h, kl = U.reference_forward(case, inp, st)
        return float(U.scalar_J(case, inp, out, kl))

    gen = torch.Generator().manual_seed(5)
    h = 1e-6
    worst = {}
    for k, g in ref["grads"].items():
        if g is None:
            assert k.startswith(U.MUST_BE_ZERO), k
            continue
        base = inp["state"][k].double()
        done = 0
        while done < 3:
            d = torch.randn(base.shape, generator=gen, dtype=U.F64)
            d = d / d.norm()
            an = float((g * d).sum())
            # J is ~1e2, so its differences carry ~2^-53 1e2 / 1e-6 = 1e-8 of rounding: a unit direction that happens to
            # be nearly orthogonal to the gradient (a derivative that is itself a cancelled sum) cannot be resolved to
            # 1e-6 of its own size at this step - drawn again
            if abs(an) < 0.05 * float(g.norm()):
                continue
            done += 1
            fd = (J_at({k: base + h * d}) - J_at({k: base - h * d})) / (2 * h)
            worst[k] = max(worst.get(k, 0.0), abs(fd - an) / abs(an))
    print({k: f"{e:.1e}" for k, e in worst.items()})
    assert all(e <= 1e-6 for e in worst.values()), worst
    # the empty free view's parameters do receive the KL's gradient
    assert float(ref["grads"]["Xtilde"][1].abs().max()) > 0 and float(ref["grads"]["delta_G_list"][1].abs().max()) > 0
