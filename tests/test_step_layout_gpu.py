"""GPU: the step engine's own kernels (csrc/step.hip: step_prep, warp_gather, warp_sample_views fwd / bwd with its
last-block reduce, flag_reduce, coldot2, step_finalize) element by element against an fp64 reference on the CPU, at the
smallest layouts that reach each indexing edge (step_layout_util.py: the scalar, the cases, the bounds); the same
per-element checks for the stand-alone sampler entries of csrc/elementwise.hip and for gpsa_adam_step.

No comparison here is norm-wise: one wrong row, view, modality or term fails its own element."""
import functools

import pytest
import torch

import step_layout_util as U
from fake_ops import FakeOps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FK = FakeOps()
F64 = torch.float64


@pytest.fixture(scope="module")
def hip():
    from spatial_alignment_amd.ops import HipOps

    return HipOps()


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs and the fp64 reference of a case: computed once, shared by its two runs, never written to"""
    case = U.Case(name)
    inp = case.build()
    return case, inp, U.reference(case, inp)


def _show(tag, ratios):
    print(tag, {k: f"{v:.3f}" for k, v in ratios.items()})


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_step_layout(name, fuse):
    """J = sum <A, G_means> + sum <B, G_samples> + sum c_t kl_t through the engine; every output and every parameter
    gradient is the fp64 answer rounded to fp32 once.  Worst error / bound per tensor is printed (docs/LAB_NOTES.md
    keeps one run's table)."""
    case, inp, ref = _case(name)
    model = case.model(inp, DEV)
    model.use_step_engine = True
    model.fuse_elbo = fuse
    model.fuse_min_flops = 0  # these layouts are tiny: the product itself would not fuse below ~5 GF per step
    dd = {m: {"spatial_coords": d["spatial_coords"].to(DEV), "outputs": d["outputs"].to(DEV),
              "n_samples_list": d["n_samples_list"]} for m, d in inp["dd"].items()}
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    model.inject_noise(inp["eps_G"], inp["eps_F"], None)
    Gm, Gs, Fl, _ = model.forward({m: dd[m]["spatial_coords"] for m in case.mods}, view_idx=view_idx, Ns=Ns, S=case.S)
    assert model._cache.kl is not None  # the engine ran
    plan = model._cache.plan
    assert (plan.n_kl, plan.eps_g_numel) == (case.expected()["n_kl"], case.expected()["eps"])
    if fuse:  # the draws are lazy handles that nobody touches; without: plain tensors whose gradient stays None
        from spatial_alignment_amd.lazy import LazyDraws

        lazy = [isinstance(Fl[m], LazyDraws) for m in case.mods]
        assert lazy == [not lmc for _, _, lmc in case.outs], lazy
    else:
        assert model._cache.fuse is None and all(torch.is_tensor(Fl[m]) for m in case.mods)
    kl = model._cache.kl  # the node's fp64 per-term output
    J = (inp["c"].to(DEV) * kl).sum()
    for m in case.mods:
        J = J + (inp["A"][m].to(DEV) * Gm[m]).sum() + (inp["B"][m].to(DEV) * Gs[m]).sum()
    J.backward()
    torch.cuda.synchronize()
    if fuse:
        assert all(s in (None, "lazy") for s in model._cache.fuse["state"])

    ratios = {}
    # ---- outputs
    for i, m in enumerate(case.mods):
        X = inp["X"][m]
        edge = 0
        for v in range(case.V):
            n = case.rows[i][v]
            if case.is_fixed(v) and n:  # a fixed view passes its coordinates through: bit for bit
                assert torch.equal(Gm[m][edge:edge + n].cpu(), X[edge:edge + n]), (m, v)
                for s in range(case.S):
                    assert torch.equal(Gs[m][s, edge:edge + n].cpu(), X[edge:edge + n]), (m, v, s)
            edge += n
        ratios[f"G_means/{m}"] = U.ratio32(Gm[m], ref["G_means"][m])
        ratios[f"G_samples/{m}"] = U.ratio32(Gs[m], ref["G_samples"][m])
    ratios["mu_z"] = U.ratio32(model.mu_z_G, ref["mu_z"], per_lead=True)
    # ---- the per-term KL (fp64): 1e-11 per term, a fixed view's terms exactly 0
    kl = kl.detach()
    assert kl.dtype == F64 and tuple(kl.shape) == tuple(ref["kl"].shape)
    for r in range(case.V * case.D):
        if case.is_fixed(r % case.V):
            assert float(kl[r]) == 0.0, r
    ratios["kl"] = U.ratio64(kl, ref["kl"])
    # ---- parameter gradients
    params = dict(model.named_parameters())
    assert set(params) == set(ref["grads"]), set(params) ^ set(ref["grads"])
    for k, want in ref["grads"].items():
        got = params[k].grad
        if k.startswith(U.MUST_BE_ZERO):  # nothing reaches the likelihood or the LMC weights
            assert want is None
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        assert want is not None and got is not None, k
        ratios[f"grad/{k}"] = U.ratio32(got, want, per_lead=k in U.PER_VIEW)
    for v in range(case.V):
        if case.is_fixed(v):
            assert float(params["Xtilde"].grad[v].abs().max()) == 0.0
            assert float(params["delta_G_list"].grad[v].abs().max()) == 0.0
    _show(f"[step_layout] {name} {'fused' if fuse else 'unfused'}", ratios)
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# the per-layer sampler entries (csrc/elementwise.hip), per element
# ---------------------------------------------------------------------------------------------------------
def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, dtype=F64) * scale).to(dtype)


FP64_ABS = 1e-13  # an fp64 output here is a sum of at most S + D + 2 terms no larger than ~max|ref|: (S + D + 2) 2^-53


def _warp_inputs(n, D, S):
    meanT, v = rnd(D, n, dtype=F64), rnd(D, n, dtype=F64, seed=1).abs()
    q, X = rnd(n, dtype=F64, seed=2).abs() * 0.1, rnd(n, D, seed=3, scale=4)
    A, b = torch.eye(D) + 0.1 * rnd(D, D, seed=7), rnd(D, seed=8)
    eps, var_u = rnd(S, n, D, seed=4), torch.tensor([0.2])
    return meanT, v, q, var_u, X, A, b, eps


@pytest.mark.parametrize("n,D,S", [(1, 1, 1), (255, 2, 3), (256, 4, 2), (257, 3, 1), (513, 2, 2)])
def test_warp_sample_per_element(hip, n, D, S):
    meanT, v, q, var_u, X, A, b, eps = _warp_inputs(n, D, S)
    dev = lambda *ts: [t.to(DEV) for t in ts]
    Gm, Gs, bad, Gs64 = hip.warp_sample_fwd(*dev(meanT, v, q, var_u, X, A, b, eps))
    Sigma = torch.exp(var_u.double()[0]) - q.unsqueeze(0) + v + 2e-5
    mu = X.double() @ A.double() + b.double() + meanT.t()
    _, _, _, rGs64 = FK.warp_sample_fwd(meanT, v, q, var_u, X, A, b, eps)
    assert torch.allclose(rGs64, mu.unsqueeze(0) + Sigma.t().unsqueeze(0) * eps.double(), rtol=0, atol=1e-12)
    ratios = {"Gm": U.ratio32(Gm, mu), "Gs": U.ratio32(Gs, rGs64),
              "Gs64": U.ratio64(Gs64, rGs64, abs_rel=FP64_ABS)}
    assert torch.equal(Gs64.float(), Gs)
    assert bad.numel() == (n + 255) // 256 and int(bad.abs().max()) == 0
    dGm, dGs = rnd(n, D, seed=5), rnd(S, n, D, seed=6)
    dGs64 = rnd(S, n, D, seed=9, dtype=F64)
    for tag, a32, a64 in (("f32", dGs, None), ("f64", None, dGs64), ("both", dGs, dGs64)):
        got = hip.warp_sample_bwd(dGm.to(DEV), None if a32 is None else a32.to(DEV), *dev(eps, var_u, X),
                                  None if a64 is None else a64.to(DEV))
        dmT, g, qbar = FK.warp_sample_bwd(dGm, a32, eps, var_u, X, a64)[:3]  # fp64
        dm = dmT.t()
        want32 = ((torch.exp(var_u.double()[0]) * g.sum()).reshape(1), X.double().t() @ dm, dm.sum(0))
        for nm, a, w in zip(("dmeanT", "g", "qbar"), got[:3], (dmT, g, qbar)):
            assert a.dtype == F64
            ratios[f"{tag}/{nm}"] = U.ratio64(a, w, abs_rel=FP64_ABS)
        for nm, a, w in zip(("dvar", "dslopes", "dintercept"), got[3:], want32):
            assert a.dtype == torch.float32
            ratios[f"{tag}/{nm}"] = U.ratio32(a, w)
    _show(f"[warp_sample] n={n} D={D} S={S}", ratios)
    bad_r = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad_r, bad_r


@pytest.mark.parametrize("n", [257, 513])
def test_warp_sample_flag_of_the_last_partial_block(hip, n):
    """a non-positive variance in the last, partial block only: that block's flag and no other"""
    D, S = 2, 1
    meanT, v, q, var_u, X, A, b, eps = _warp_inputs(n, D, S)
    v = v.clone()
    v[1, n - 1] = -100.0
    _, _, bad, _ = hip.warp_sample_fwd(*[t.to(DEV) for t in (meanT, v, q, var_u, X, A, b, eps)])
    nb = (n + 255) // 256
    assert bad.cpu().tolist() == [0] * (nb - 1) + [1]


@pytest.mark.parametrize("M,D,scale", [(1, 1, 1.0), (85, 3, 1.0), (128, 2, 100.0), (129, 2, 1.0), (257, 4, 1.0)])
def test_mean_resid_per_element(hip, M, D, scale):
    """M D = 1, 255, 256, 258, 1028 elements: the forward's 256-element blocks; the backward's one block strides"""
    Z, delta = rnd(M, D, seed=1, scale=5), rnd(M, D, seed=2, scale=5)
    A, b = torch.eye(D) + 0.1 * rnd(D, D, seed=3), rnd(D, seed=4)
    mu, r = hip.mean_resid_fwd(*[t.to(DEV) for t in (Z, A, b, delta)], scale)
    rmu = scale * (Z.double() @ A.double() + b.double())
    assert torch.allclose(FK.mean_resid_fwd(Z, A, b, delta, scale)[1], delta.double() - rmu, rtol=0, atol=1e-11)
    assert mu.dtype == torch.float32 and r.dtype == F64
    ratios = {"mu": U.ratio32(mu, rmu), "resid": U.ratio64(r, delta.double() - rmu, abs_rel=FP64_ABS)}
    dres = rnd(M, D, dtype=F64, seed=5)
    got = hip.mean_resid_bwd(dres.to(DEV), Z.to(DEV), A.to(DEV), scale)
    want = (dres, -scale * dres @ A.double().t(), -scale * Z.double().t() @ dres, -scale * dres.sum(0))
    for nm, a, w in zip(("ddelta", "dZ", "dslopes", "dintercept"), got, want):
        ratios[nm] = U.ratio32(a, w)
    _show(f"[mean_resid] M={M} D={D}", ratios)
    bad = {k: x for k, x in ratios.items() if not x <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("C,L", [(31, 1), (32, 32), (33, 33), (65, 31)])
def test_data_sample_per_element(hip, C, L):
    """the fp32 data sampler at the edges of its 32 x 32 transposes; bounds: rounding count x 2^-24 x magnitude
    (step_layout_util.data_sample_*_bounds derive them next to the formulas)"""
    meanT, v = rnd(L, C), rnd(L, C, seed=1).abs()
    q, eps = rnd(C, seed=2, dtype=F64).abs() * 0.1, rnd(C, L, seed=3)
    var_u = torch.tensor([0.5])
    F, Sig = hip.data_sample_fwd(meanT.to(DEV), v.to(DEV), q.to(DEV), var_u.to(DEV), eps.to(DEV))
    rF, rS, bF, bS = U.data_sample_fwd_bounds(meanT, v, q, var_u, eps)
    fF, fS = FK.data_sample_fwd(meanT.double(), v.double(), q, var_u.double(), eps.double())
    assert float((fF - rF).abs().max()) <= 1e-14 * float(rF.abs().max()) and float((fS - rS).abs().max()) <= 1e-14
    ratios = {"F": U.ratio_to(F, rF, bF), "Sigma": U.ratio_to(Sig, rS, bS)}
    dF = rnd(C, L, seed=4)
    g_ext, dmeanT, dvar = hip.data_sample_bwd(dF.to(DEV), eps.to(DEV), Sig, var_u.to(DEV))
    assert g_ext.shape == (L + 1, C)
    g, qbar, dv, bg, bq, bd = U.data_sample_bwd_bounds(dF, eps, Sig.cpu(), var_u)
    assert torch.equal(dmeanT.cpu(), dF.t())  # a transposed copy
    ratios.update(g=U.ratio_to(g_ext[:L], g, bg), qbar=U.ratio_to(g_ext[L], qbar, bq),
                  dvar=U.ratio_to(dvar.reshape(()), dv, bd))
    _show(f"[data_sample] C={C} L={L}", ratios)
    bad = {k: x for k, x in ratios.items() if not x <= 1.0}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# gpsa_adam_step
# ---------------------------------------------------------------------------------------------------------
def test_adam_step_per_element():
    """one step from a given fp32 state (p, m, v, t) loaded through the optimiser's state dict: 17 tensors (two
    launches of ADAM_MAXT = 16 and 1 tensors behind ONE tick of the step word) of 1, 1023, 1024, 1025 and 4097
    elements (the kernel's 1024-element blocks) against the update evaluated in fp64 from the same state"""
    from spatial_alignment_amd.optim import FusedAdam

    sizes = [1, 1023, 1024, 1025, 4097]
    sizes = [sizes[i % 5] for i in range(17)]
    t0, lr, (b1, b2), eps = 7, 1e-2, (0.9, 0.999), 1e-8
    P = [rnd(n, seed=10 + i) for i, n in enumerate(sizes)]
    G = [rnd(n, seed=40 + i, scale=0.3) for i, n in enumerate(sizes)]
    Mo = [rnd(n, seed=70 + i, scale=0.1) for i, n in enumerate(sizes)]
    Vo = [rnd(n, seed=100 + i, scale=0.2).square() for i, n in enumerate(sizes)]
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in P]
    opt = FusedAdam(params, lr=lr, betas=(b1, b2), eps=eps)
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(t0)), "exp_avg": Mo[i].clone(), "exp_avg_sq": Vo[i].clone()}
                   for i in range(len(sizes))}
    opt.load_state_dict(sd)
    for p, g in zip(params, G):
        p.grad = g.clone().to(DEV)
    opt.step()
    torch.cuda.synchronize()
    words = {id(opt.state[p]["step"]) for p in params}
    assert len(words) == 1 and float(opt.state[params[0]]["step"]) == t0 + 1  # one word, ticked once
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, p in enumerate(params):
        p1, m1, v1, bp, bm, bv = U.adam_bounds(P[i], G[i], Mo[i], Vo[i], t0, lr, b1, b2, eps)
        st = opt.state[p]
        worst["p"] = max(worst["p"], U.ratio_to(p.detach(), p1, bp))
        worst["m"] = max(worst["m"], U.ratio_to(st["exp_avg"], m1, bm))
        worst["v"] = max(worst["v"], U.ratio_to(st["exp_avg_sq"], v1, bv))
        assert torch.equal(p.grad.cpu(), G[i])  # the gradient is read, never written
    _show("[adam]", worst)
    assert all(r <= 1.0 for r in worst.values()), worst
