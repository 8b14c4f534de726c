"""The opt-in bf16x3 contraction of the data GP's fused ELBO pass (panel_elbo_x3_kernel, gpsa_step_desc.contraction = 1):
the kernel family in the built library, the descriptor field, the model attribute / GPSA_CONTRACTION, and on the GPU the
kernel against an fp64 statement of its contract (next to the fp32 kernel on the same inputs) and the whole step against
the goldens and the fp64 oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from golden_io import CASES, Golden, rel
from model_util import build_model, compare, run_step

from spatial_alignment_amd import _lib
from spatial_alignment_amd import step_engine as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, F64 = 0, 1


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_x3_kernel_family_is_built_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta as km

    ks = km.library_kernels(os.path.join(ROOT, "spatial_alignment_amd", "libgpsa_hip.so"))
    names = km.demangle([k["name"] for k in ks])
    x3 = {n: k for n, k in zip(names, ks) if "panel_elbo_x3_kernel<" in n}
    assert len(x3) == 5, sorted(x3)
    for n, k in x3.items():
        assert k["max_wg"] == 256 and k["scratch"] == 0, (n, k)
    head = [k for n, k in x3.items() if "panel_elbo_x3_kernel<13, 1>" in n]
    assert len(head) == 1 and head[0]["vgpr"] > 256, head  # one wave per SIMD, the unified register file
    assert any("pack_x3_kernel<double>" in n for n in names)
    gx3 = {n: k for n, k in zip(names, ks) if "gram_x3_kernel<" in n}
    assert len(gx3) == 5, sorted(gx3)
    for n, k in gx3.items():
        assert k["max_wg"] == 256 and k["scratch"] == 0, (n, k)
    assert any("split_image_kernel" in n for n in names)


def test_x3_gram_entry_points_decline_what_they_do_not_cover():
    lib = _lib.load()
    assert lib.gpsa_quadform_bwd_omega_x3_workspace(200, 10000, 50) > 0
    assert lib.gpsa_quadform_bwd_omega_x3_workspace(257, 10000, 50) == 0  # M > 256: the big-M kernels stay fp32
    # (argument checks run before any launch: no device needed)
    assert lib.gpsa_quadform_bwd_omega_x3(F64, F64, 1, 1, 200, 100, 5, 1, None, 0, None) == -3  # fp32 operands only


def _describe(contraction):
    lib = _lib.load()
    d = _lib.StepDesc()
    d.n_views, d.n_dims, d.n_mods, d.n_samples = 2, 2, 1, 5
    d.m_x, d.m_g = 200, 200
    d.n_latent[0], d.n_out[0], d.has_lmc[0], d.n_rows[0] = 50, 50, 0, 20000
    d.want_kl = 1
    fx = (C.c_int * 2)(0, 0)
    rw = (C.c_longlong * 2)(10000, 10000)
    d.view_fixed, d.view_rows = fx, rw
    d.contraction = contraction
    out = (C.c_longlong * 7)()
    return lib.gpsa_step_describe(C.byref(d), out)


def test_descriptor_accepts_fp32_and_bf16x3_only():
    assert _describe(0) == 0
    assert _describe(1) == 0
    for bad in (2, -1, 7):
        assert _describe(bad) != 0


class _M:
    def __init__(self, contraction):
        self.contraction = contraction


def test_model_attribute_and_environment(monkeypatch):
    monkeypatch.delenv("GPSA_CONTRACTION", raising=False)
    assert SE.contraction_mode(_M(None)) == "fp32"
    assert SE.contraction_mode(_M("bf16x3")) == "bf16x3"
    assert SE.contraction_mode(_M("fp32")) == "fp32"
    monkeypatch.setenv("GPSA_CONTRACTION", "bf16x3")
    assert SE.contraction_mode(_M(None)) == "bf16x3"
    assert SE.contraction_mode(_M("fp32")) == "fp32"  # the attribute wins
    monkeypatch.setenv("GPSA_CONTRACTION", "bf16")
    with pytest.raises(ValueError):
        SE.contraction_mode(_M(None))
    with pytest.raises(ValueError):
        SE.contraction_mode(_M("tf32"))


def test_new_model_has_the_attribute_unset():
    g = Golden(CASES[0])
    model, _ = build_model(g)
    assert model.contraction is None


# ---- GPU: the kernel ------------------------------------------------------------------------------------------------

def _elbo_ref(Om, al, meanT, q, var_u, eps, Y, N, S, noise_u):
    """fp64 statement of gpsa_quadform_elbo_f32's contract (include/gpsa_hip.h)"""
    W = torch.einsum("lmk,kc->lmc", Om, al)                       # [L, M, C]
    v = (al.unsqueeze(0) * W).sum(1)                             # [L, C]
    var = (torch.exp(var_u) - q).unsqueeze(0) + v + 2e-5
    C_ = al.shape[1]
    e = eps.t()                                                  # [L, C]
    F = meanT + torch.sqrt(var) * e
    s = torch.exp(noise_u) + 1e-5
    Yc = Y[torch.arange(C_) % N].t()                             # [L, C]
    dF = -(Yc - F) / (s * s * S)
    g = dF * e / (2 * torch.sqrt(var))
    abar = 2 * (g.unsqueeze(1) * W).sum(0)                       # [M, C]
    z2 = (((Yc - F) / s) ** 2).sum()
    return g, dF, abar, z2


def _run_kernel(x3, delta_form, om_dtype, Om64, al, delta, meanT, q, var_u, eps, Y, N, S, noise_u):
    lib = _lib.load()
    M, C_ = al.shape
    L = Om64.shape[0]
    ws_fn = lib.gpsa_quadform_elbo_x3_f32_workspace if x3 else lib.gpsa_quadform_elbo_f32_workspace
    wsb = int(ws_fn(M, C_, L))
    assert wsb > 0
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)  # exactly the query's size, NaN throughout
    g = torch.empty(L, C_, device=DEV)
    dF = torch.empty(L, C_, device=DEV)
    abar = torch.empty(M, C_, device=DEV)
    part = torch.empty(int(lib.gpsa_quadform_elbo_parts()), dtype=torch.float64, device=DEV)
    Om = Om64 if om_dtype == F64 else Om64.float()
    args = [om_dtype, al.data_ptr(), Om.data_ptr(), M, C_, L]
    args += [delta.data_ptr() if delta_form else meanT.data_ptr()]
    args += [q.data_ptr(), var_u.data_ptr(), eps.data_ptr(), Y.data_ptr(), N, S, noise_u.data_ptr(), g.data_ptr(),
             dF.data_ptr(), abar.data_ptr(), part.data_ptr(), None, ws.data_ptr(), wsb,
             torch.cuda.current_stream().cuda_stream]
    if x3:
        fn = lib.gpsa_quadform_elbo_delta_x3_f32 if delta_form else lib.gpsa_quadform_elbo_x3_f32
    else:
        fn = lib.gpsa_quadform_elbo_delta_f32 if delta_form else lib.gpsa_quadform_elbo_f32
    rc = fn(*args)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return g.double().cpu(), dF.double().cpu(), abar.double().cpu(), part.sum().cpu()


# the edges of every row-tile class MB (tests/test_hip_kernels.py: TILE_EDGE_M), at a small shape: C = 260, L = 3
TILE_EDGE_M = [16 * (mb - 1) + d for mb in (2, 4, 7, 13, 16) for d in (1, 8, 9, 15, 16)]
LONG_M = [16, 25, 64, 100, 200, 208, 240]  # at C ~ 10 000, L = 5
SHAPE_IDS = [str(m) for m in LONG_M] + [f"{m}-edge" for m in TILE_EDGE_M]


@pytest.mark.gpu
@pytest.mark.parametrize("M,L,N", [(m, 5, 4999) for m in LONG_M] + [(m, 3, 130) for m in TILE_EDGE_M], ids=SHAPE_IDS)
def test_x3_kernel_matches_fp64_contract(M, L, N):
    """C = 9998 (not a multiple of 64) and L = 5: more items than workgroups, so column tiles are cut between them and
    their abar leaves through the slabs.  Both mean forms (the delta one where M allows it), fp64 and fp32 Omega.
    C = 260, L = 3: the edges of the row-tile classes."""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(M)
    S = 2
    C_ = N * S
    A = torch.randn(L, M, M, generator=gen, dtype=torch.float64)
    Om64 = 0.1 * A @ A.transpose(1, 2) / M
    al64 = 0.3 * torch.randn(M, C_, generator=gen, dtype=torch.float64)
    delta64 = torch.randn(M, L, generator=gen, dtype=torch.float64)
    eps64 = torch.randn(C_, L, generator=gen, dtype=torch.float64)
    Y64 = torch.randn(N, L, generator=gen, dtype=torch.float64)
    q64 = 0.5 * torch.rand(C_, generator=gen, dtype=torch.float64)
    # what the kernels see (fp32 operands) is what the reference is given
    al = al64.float()
    delta, eps, Y = delta64.float(), eps64.float(), Y64.float()
    meanT = (delta.double().t() @ al.double()).float()
    var_u = torch.tensor([0.1], dtype=torch.float32)
    noise_u = torch.tensor([-0.5], dtype=torch.float32)
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    ins = [dev(al), dev(delta), dev(meanT), dev(q64), dev(var_u), dev(eps), dev(Y), N, S, dev(noise_u)]
    forms = [False] + ([True] if lib.gpsa_quadform_elbo_takes_delta(M) else [])
    for delta_form in forms:
        for om_dtype in (F64, F32):
            Om = dev(Om64)
            ref = _elbo_ref(Om64 if om_dtype == F64 else Om64.float().double(), al.double(), meanT.double(), q64,
                            var_u.double(), eps.double(), Y.double(), N, S, noise_u.double())
            errs = {}
            for x3 in (False, True):
                out = _run_kernel(x3, delta_form, om_dtype, Om, *ins)
                errs[x3] = [rel(o.numpy(), r.numpy()) for o, r in zip(out, ref)]
            print(M, "delta" if delta_form else "meanT", "f64" if om_dtype == F64 else "f32",
                  "fp32:", ["%.1e" % e for e in errs[False]], "x3:", ["%.1e" % e for e in errs[True]])
            for e32, ex3 in zip(errs[False], errs[True]):
                # the bar: no worse than twice the fp32 instruction's error on the same inputs (a floor of 1e-7 for
                # quantities both get to the last bits)
                assert ex3 <= max(2 * e32, 1e-7), (errs[False], errs[True])


# ---- GPU: the step --------------------------------------------------------------------------------------------------

def _plans(model):
    return list(model.__dict__.get("_step_plans", {}).values())


def _contraction_seen(model):
    return [p.contraction for p in _plans(model)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_x3_step_matches_reference_fp64(name):
    g = Golden(name)
    model, dd = build_model(g, device=DEV)
    model.contraction = "bf16x3"
    res = run_step(model, dd, g, device=DEV)
    bad, errs = compare(res, g, tol_out=1e-4, tol_grad=1e-4)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert not bad, bad
    assert max(v for k, v in errs.items() if not k.startswith("grad/")) < 2e-6, errs
    assert _plans(model) and all(p.key[-1] == "bf16x3" for p in _plans(model))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c for c in CASES if "m200" in c] + ["c2_three_free_views"])
def test_x3_mode_really_runs(name):
    g = Golden(name)
    model, dd = build_model(g, device=DEV)
    model.contraction = "bf16x3"
    run_step(model, dd, g, device=DEV)
    assert model._cache.fuse is not None and "fused" in model._cache.fuse["state"]
    train = _plans(model)
    assert train
    for p in train:
        for i, m in enumerate(p.mods):
            if not p.lmc[i]:
                assert p.contraction[m] == 3, p.contraction
                assert int(p.lib.gpsa_step_contraction(p.handle, i)) == 3


@pytest.mark.gpu
def test_default_runs_fp32(monkeypatch):
    monkeypatch.delenv("GPSA_CONTRACTION", raising=False)
    g = Golden("c7_m200_conditioning")
    model, dd = build_model(g, device=DEV)
    run_step(model, dd, g, device=DEV)
    assert _plans(model)
    for p in _plans(model):
        assert all(v == 0 for v in p.contraction.values())
        for i in range(len(p.mods)):
            assert int(p.lib.gpsa_step_contraction(p.handle, i)) == 0


@pytest.mark.gpu
def test_x3_step_is_bitwise_repeatable_and_differs_from_fp32():
    g = Golden("c7_m200_conditioning")
    res = []
    for mode in ("bf16x3", "bf16x3", "fp32"):
        model, dd = build_model(g, device=DEV)
        model.contraction = mode
        res.append(run_step(model, dd, g, device=DEV))
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), k
    # (and the mode is not a no-op: the data GP's gradients see the other rounding)
    m = g.mods[0]
    assert not np.array_equal(res[0][f"grad/Omega_sqt_F_dict.{m}"], res[2][f"grad/Omega_sqt_F_dict.{m}"])


@pytest.mark.gpu
def test_x3_config2_full_size_matches_fp64_oracle():
    """the headline shape (2 views x 10 000 spots, L = 50, M = 200) at S = 5 through both x3 kernels, against the fp64
    oracle: every output, the ELBO and every gradient within 1e-4"""
    import psutil

    if psutil.virtual_memory().available < 80 * 2**30:
        pytest.skip("the fp64 oracle at S = 5 wants ~60 GB of host memory")
    _synthetic_vs_oracle(side=100, views=2, L=50, M=200, S=5, expect=3)


def _synthetic_vs_oracle(side, views, L, M, S, expect):
    from oracle import gpsa_oracle as orc
    from spatial_alignment_amd.synthetic import make_grid_problem, make_model

    MOD = "expression"
    dd = make_grid_problem(side=side, n_views=views, n_outputs=L, device="cpu")
    model = make_model(dd, m=M, device="cpu", seed=5)
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        model.delta_G_list.add_(0.15 * torch.randn(model.delta_G_list.shape, generator=gen))
        model.Xtilde.add_(0.03 * torch.randn(model.Xtilde.shape, generator=gen))
        model.Gtilde.add_(0.03 * torch.randn(model.Gtilde.shape, generator=gen))
        for p in (model.warp_kernel_variances, model.warp_kernel_lengthscales, model.data_kernel_lengthscale,
                  model.data_kernel_variance, model.noise_variance):
            p.add_(0.2 * torch.randn(p.shape, generator=gen))
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for name in ("mean_slopes", "mean_intercepts"):
        state.setdefault(name, getattr(model, name).detach().clone())
    model = model.to(DEV)
    model.fuse_elbo = True
    model.contraction = "bf16x3"
    n, N = side * side, side * side * views
    eps_G = [torch.randn(S, n, 2, generator=gen) for _ in range(views)]
    eps_F = {MOD: torch.randn(S, N, L, generator=gen)}
    ddd = {MOD: {"spatial_coords": dd[MOD]["spatial_coords"].to(DEV), "outputs": dd[MOD]["outputs"].to(DEV),
                 "n_samples_list": dd[MOD]["n_samples_list"]}}
    view_idx, Ns, _, _ = model.create_view_idx_dict(ddd)
    model.inject_noise(eps_G, eps_F, None)
    out = model.forward({MOD: ddd[MOD]["spatial_coords"]}, view_idx=view_idx, Ns=Ns, S=S)
    loss = model.loss_fn(ddd, out[3])
    loss.backward()
    assert model._cache.fuse["state"] == ["fused"]
    assert any(p.contraction == {MOD: expect} for p in _plans(model))
    cfg = dict(modality_names=[MOD], n_views=views, n_spatial_dims=2, kernel_warp="rbf", kernel_data="rbf",
               n_latent_gps={MOD: None}, fixed_view_idx=None)
    ref = orc.evaluate(state, cfg, {MOD: dd[MOD]["spatial_coords"]}, {MOD: dd[MOD]["outputs"]},
                       {MOD: dd[MOD]["n_samples_list"]}, S, eps_G, eps_F, dtype=torch.float64)
    errs = {"G_means": rel(out[0][MOD].detach().cpu().numpy(), ref["G_means"][MOD].numpy()),
            "F_samples": rel(out[3][MOD].detach().cpu().numpy(), ref["F_obs"][MOD].numpy()),
            "loss": rel(loss.detach().cpu().numpy(), ref["loss"].numpy())}
    gerr = {k: rel(p.grad.detach().cpu().numpy(), ref["grads"][k].numpy())
            for k, p in model.named_parameters() if k in ref["grads"] and float(ref["grads"][k].norm()) > 0}
    print(f"{views} x {side * side} spots, L = {L}, M = {M}, S = {S}, bf16x3, vs fp64 oracle:", {k: f"{v:.1e}" for k, v in errs.items()})
    print("   gradients:", {k: f"{v:.1e}" for k, v in gerr.items()})
    assert all(v < 1e-4 for v in errs.values()), errs
    for k, e in gerr.items():
        assert e < 1e-4, (k, e)


# ---- GPU: the Gram kernel ---------------------------------------------------------------------------------------------

def _gram(x3, delta_form, al, g, dmean, ddelta0):
    lib = _lib.load()
    M, C_ = al.shape
    L = g.shape[0]
    wsb = int(lib.gpsa_quadform_bwd_omega_x3_workspace(M, C_, L) if x3 else lib.gpsa_quadform_workspace(F32, M, C_, L))
    ws = torch.full((max(wsb, 1),), 0xFF, dtype=torch.uint8, device=DEV)  # exactly the query's size, NaN throughout
    out = torch.empty(L, M, M, dtype=torch.float64, device=DEV)
    dd = ddelta0.clone()
    st = torch.cuda.current_stream().cuda_stream
    if delta_form:
        fn = lib.gpsa_quadform_bwd_omega_delta_x3 if x3 else lib.gpsa_quadform_bwd_omega_delta_f32
        rc = fn(F64, al.data_ptr(), g.data_ptr(), dmean.data_ptr(), M, C_, L, out.data_ptr(), dd.data_ptr(), 1.0,
                ws.data_ptr(), wsb, st)
    else:
        fn = lib.gpsa_quadform_bwd_omega_x3 if x3 else lib.gpsa_quadform_bwd_omega
        rc = fn(F32, F64, al.data_ptr(), g.data_ptr(), M, C_, L, out.data_ptr(), ws.data_ptr(), wsb, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu(), dd.double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("M,L,C_", [(m, 5, 9996) for m in LONG_M] + [(m, 3, 260) for m in TILE_EDGE_M], ids=SHAPE_IDS)
def test_x3_gram_matches_fp64_contract(M, L, C_):
    """dOmega_l = sum_c g[l,c] alpha_c alpha_c^T (and d delta = beta d delta + alpha dmean^T in the delta form) against
    fp64, next to the fp32 kernel on the same inputs; C = 9996 (not a multiple of 32 or 64), L = 5, and the edges of the
    row-tile classes at C = 260, L = 3"""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(1000 + M)
    al = (0.3 * torch.randn(M, C_, generator=gen)).float()
    g = torch.randn(L, C_, generator=gen).float()
    dmean = torch.randn(L, C_, generator=gen).float()
    dd0 = torch.randn(M, L, generator=gen).float()
    ref = torch.einsum("lc,mc,kc->lmk", g.double(), al.double(), al.double())
    ref_dd = dd0.double() + al.double() @ dmean.double().t()
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    forms = [False] + ([True] if lib.gpsa_quadform_bwd_omega_takes_delta(M, C_) else [])
    for delta_form in forms:
        errs = {}
        for x3 in (False, True):
            out, dd = _gram(x3, delta_form, dev(al), dev(g), dev(dmean), dev(dd0))
            errs[x3] = [rel(out.numpy(), ref.numpy())] + ([rel(dd.numpy(), ref_dd.numpy())] if delta_form else [])
        print(M, "delta" if delta_form else "plain", "fp32:", ["%.1e" % e for e in errs[False]],
              "x3:", ["%.1e" % e for e in errs[True]])
        for e32, ex3 in zip(errs[False], errs[True]):
            assert ex3 <= max(2 * e32, 1e-7), (errs[False], errs[True])
    # bitwise repeatable
    a, _ = _gram(True, False, dev(al), dev(g), dev(dmean), dev(dd0))
    b, _ = _gram(True, False, dev(al), dev(g), dev(dmean), dev(dd0))
    assert torch.equal(a, b)


# ---- GPU: more of the step ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3_lmc_matern12_warp", "c5_two_modalities", "c11_lmc_gtest_unequal"])
def test_lmc_modalities_keep_the_fp32_elbo_pass(name):
    """an LMC modality's likelihood pass is lmc_mfma_kernel (fp32): only its Gram runs x3 (query 2); the others get 3"""
    g = Golden(name)
    model, dd = build_model(g, device=DEV)
    model.contraction = "bf16x3"
    res = run_step(model, dd, g, device=DEV)
    bad, _ = compare(res, g, tol_out=1e-4, tol_grad=1e-4)
    assert not bad, bad
    train = _plans(model)
    assert train
    for p in train:
        for i, m in enumerate(p.mods):
            assert p.contraction[m] == (2 if p.lmc[i] else 3), (m, p.contraction)


@pytest.mark.gpu
def test_x3_graphed_step_equals_eager_x3_step():
    """GraphedTrainStep captures the x3 sequence (pack, ELBO kernel, slab reduce, image split, Gram, reduce) with its own
    scratch sizes: one replay after the capture's warm-up steps equals the same number of eager steps"""
    from spatial_alignment_amd.train import GraphedTrainStep, train_step

    g = Golden("c7_m200_conditioning")
    res = []
    for mode in ("eager", "graph"):
        model, dd = build_model(g, device=DEV)
        model.contraction = "bf16x3"
        view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
        eps_G = [e.to(DEV) for e in g.eps_G]
        eps_F = {m: e.to(DEV) for m, e in g.eps_F.items()}
        orig = model.forward

        def fwd(*a, _orig=orig, _m=model, **k):
            _m.inject_noise(eps_G, eps_F)
            return _orig(*a, **k)

        model.forward = fwd
        if mode == "eager":
            for _ in range(4):
                loss = train_step(model, opt, dd, view_idx, Ns, S=g.S)
        else:
            gs = GraphedTrainStep(model, opt, dd, view_idx, Ns, S=g.S, warmup=3)
            loss = gs.step()
            gs.check()
        torch.cuda.synchronize()
        assert any(p.contraction.get(g.mods[0]) == 3 for p in _plans(model))
        res.append((float(loss), {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[0][0]), (res[0][0], res[1][0])
    for k in res[0][1]:
        a, b = res[0][1][k].double(), res[1][1][k].double()
        assert (a - b).norm() <= 1e-5 * max(a.norm().item(), 1e-6), k


@pytest.mark.gpu
def test_x3_step_m240_matches_fp64_oracle():
    """M = 240 (16 row tiles, the largest shape either x3 kernel covers) through the whole step against the fp64 oracle"""
    _synthetic_vs_oracle(side=30, views=2, L=8, M=240, S=2, expect=3)
