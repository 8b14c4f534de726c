"""Training on partly observed outputs (model.skip_missing): a NaN in the outputs is a missing observation and the loss
is the ELBO of the observed entries.  The kernels (gpsa_count_observed, gpsa_elbo_loss_skip_fwd / _bwd,
gpsa_quadform_elbo_skip_f32 / _delta_skip_f32, gpsa_lmc_loglik_fused_skip_f32) against fp64 torch at the bars their
unmasked counterparts are held to (tests/test_loss_ops_gpu.py, tests/test_fused_elbo.py), and whole steps against the
fp64 oracle with the sum restricted to the observed entries:
    negative_elbo(Y with the NaNs replaced by 0)  +  sum_missing log N(0; F, s) / S
(fp64 torch with autograd, so every parameter's gradient comes with it) at the project's hard 1e-4."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from golden_io import Golden, rel
from model_util import build_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
LOG2PI_2 = 0.9189385332046727
MASK_SEED = 20240917  # every random mask of this file


def _build():
    import __graft_entry__ as ge

    ge.build()
    import spatial_alignment_amd.torch_ops  # noqa: F401  (registers torch.ops.gpsa.*)
    from spatial_alignment_amd import _lib

    return _lib.load()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


# ---- 1. counts and the loss closings ---------------------------------------------------------------------------------
# the grid-edge shapes of tests/test_loss_ops_gpu.py (ONE_TERM): one element, one block, a full block, one past it, an
# odd size over several blocks, several grid strides
SHAPES = [(1, 1, 1), (2, 50, 4), (2, 512, 1), (1, 1025, 1), (3, 333, 7), (1, 4099, 1025)]
MASKS = ["none", "random", "column", "view", "term"]


def _views_of(N):
    """three views where the rows allow it (unequal, the middle one a single row)"""
    if N < 3:
        return [N]
    a = N // 3
    return [a, 1, N - a - 1]


def _mask(kind, N, P, views, gen):
    miss = torch.zeros(N, P, dtype=torch.bool)
    if kind == "random":
        miss = torch.rand(N, P, generator=gen) < 0.3
    elif kind == "column":
        miss[:, P // 2] = True
    elif kind == "view":
        lo = sum(views[:-1])
        miss[lo:] = True
    elif kind == "term":
        miss[:] = True
    return miss


def _ref_loss(F, Y, miss, noise_u, w_rows, kl, kl_scale, gloss):
    """fp64 torch: loss, ll, dF, dnoise of one term (w_rows: per-row weights [N])"""
    F = F.double().clone().requires_grad_(True)
    nu = noise_u.double().clone().requires_grad_(True)
    s = torch.exp(nu) + 1e-5
    Y0 = torch.where(miss, torch.zeros_like(Y), Y).double()
    lp = -0.5 * ((Y0 - F) / s) ** 2 - torch.log(s) - LOG2PI_2
    lp = lp * (~miss).double() * w_rows.double()[None, :, None]
    ll = lp.sum() / F.shape[0]
    loss = -ll + kl_scale * kl.sum()
    dF, dn = torch.autograd.grad(loss * gloss, [F, nu])
    return float(loss), float(ll), dF, float(dn)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_and_loss_closings(shape, mask):
    _build()
    S, N, P = shape
    gen = torch.Generator().manual_seed(MASK_SEED + S + N + P)
    views = _views_of(N)
    off = [0]
    for n in views:
        off.append(off[-1] + n)
    F = torch.randn(S, N, P, generator=gen)
    Y = torch.randn(N, P, generator=gen)
    miss = _mask(mask, N, P, views, gen)
    Ym = torch.where(miss, torch.full_like(Y, NAN), Y)
    noise = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float32)
    kl = torch.rand(5, generator=gen, dtype=torch.float64)
    ks, gl = 0.7, -0.75
    Fd, Yd, nd, kd = F.to(DEV), Ym.to(DEV), noise.to(DEV), kl.to(DEV)
    work = torch.empty(8 * 4100 + 64, dtype=torch.uint8, device=DEV)
    cws = torch.empty(8 * 64 * 64 + 64, dtype=torch.uint8, device=DEV)
    g = torch.tensor([gl], device=DEV)
    for weighted in (False, True):
        V = len(views) if weighted else 1
        w = (torch.rand(V, generator=gen, dtype=torch.float64) + 0.5) if weighted else torch.ones(1, dtype=torch.float64)
        nv, vo, wl = ([V], off, [w.to(DEV)]) if weighted else ([], [], [])
        nobs = [torch.full((V,), -1.0, dtype=torch.float64, device=DEV)]
        torch.ops.gpsa.count_observed([Yd], nv, vo, nobs, cws)
        bounds = off if weighted else [0, N]
        want_n = [float((~miss[bounds[v]:bounds[v + 1]]).sum()) for v in range(V)]
        assert nobs[0].cpu().tolist() == want_n  # exact
        w_rows = torch.cat([w[v].expand(bounds[v + 1] - bounds[v]) for v in range(V)])
        loss = torch.empty(1, device=DEV)
        ll = torch.empty(1, dtype=torch.float64, device=DEV)
        torch.ops.gpsa.elbo_loss_skip_fwd([Fd], [Yd], nd, [1], [], [], nv, vo, wl, nobs, kd, ks, loss, ll, work)
        dF = [torch.full_like(Fd, NAN)]
        dn = torch.full((3,), NAN, device=DEV)
        dkl = torch.empty(5, dtype=torch.float64, device=DEV)
        torch.ops.gpsa.elbo_loss_skip_bwd([Fd], [Yd], nd, [1], [], [], nv, vo, wl, nobs, g, 5, ks, dF, dn, dkl, work)
        torch.cuda.synchronize()
        r_loss, r_ll, r_dF, r_dn = _ref_loss(F, Y, miss, noise[1], w_rows, kl, ks, gl)
        print(f"[{shape} {mask} weighted={weighted}] loss {float(loss):.6g} / {r_loss:.6g}, ll {float(ll):.6g} / {r_ll:.6g}, "
              f"dnoise {float(dn[1]):.6g} / {r_dn:.6g}, dF rel {_rel(dF[0], r_dF):.2g}")
        # the bars of the unmasked kernels (tests/test_minibatch_gpu.py, tests/test_loss_ops_gpu.py): the log-likelihood to
        # fp32 products summed in fp64, the fp32 loss and gradients to fp32 rounding
        n_obs = sum(want_n) * S
        assert abs(float(ll) - r_ll) <= 2e-6 * (abs(r_ll) + 1.0)
        assert abs(float(loss) - r_loss) <= 1e-6 * (abs(r_loss) + 1.0)
        assert torch.isfinite(dF[0]).all() and torch.isfinite(dn).all()
        assert float(dn[0]) == 0.0 and float(dn[2]) == 0.0  # zero-filled entries no term names
        assert abs(float(dn[1]) - r_dn) <= 2e-6 * (abs(r_dn) + 1e-3 * max(n_obs, 1.0) ** 0.5)
        if float(r_dF.norm()) > 0:
            assert _rel(dF[0], r_dF) <= 1e-6
        assert (dF[0].cpu()[:, miss] == 0).all()  # exactly 0 at a missing entry
        assert torch.equal(dkl.cpu(), torch.full((5,), ks * gl, dtype=torch.float64))
        if mask == "term":
            assert float(ll) == 0.0 and float(dn[1]) == 0.0 and abs(float(loss) - ks * float(kl.sum())) <= 1e-6
        if mask == "none":  # the unmasked entries at their own bars (not bitwise: another instantiation)
            l2 = torch.empty(1, device=DEV)
            ll2 = torch.empty(1, dtype=torch.float64, device=DEV)
            dF2, dn2 = [torch.empty_like(Fd)], torch.empty(3, device=DEV)
            if weighted:
                torch.ops.gpsa.elbo_loss_weighted_fwd([Fd], [Yd], nd, [1], nv, vo, wl, kd, ks, l2, ll2, work)
                torch.ops.gpsa.elbo_loss_weighted_bwd([Fd], [Yd], nd, [1], nv, vo, wl, g, 5, ks, dF2, dn2, dkl, work)
            else:
                torch.ops.gpsa.elbo_loss_fwd([Fd], [Yd], nd, [1], kd, ks, l2, ll2, work)
                torch.ops.gpsa.elbo_loss_bwd([Fd], [Yd], nd, [1], g, 5, ks, dF2, dn2, dkl, work)
            assert abs(float(loss) - float(l2)) <= 1e-6 * (abs(float(l2)) + 1.0)
            assert abs(float(ll) - float(ll2)) <= 2e-6 * (abs(float(ll2)) + 1.0)  # (fp32 z * z: fused or not)
            assert _rel(dF[0], dF2[0]) <= 1e-6 and abs(float(dn[1]) - float(dn2[1])) <= 1e-6 * (abs(float(dn2[1])) + 1e-3)


def test_fused_term_takes_the_counts():
    """a fused term (partial sums of z^2) closes with nobs where S N P stands; an empty one gives exact zeros"""
    _build()
    S, N, P = 2, 50, 4
    gen = torch.Generator().manual_seed(MASK_SEED)
    zp = torch.rand(7, generator=gen, dtype=torch.float64)
    noise = torch.tensor([0.25], dtype=torch.float32)
    work = torch.empty(8 * 4100 + 64, dtype=torch.uint8, device=DEV)
    Y = torch.zeros(N, P, device=DEV)
    for n_obs, z in ((123.0, zp), (0.0, torch.zeros(7, dtype=torch.float64))):
        nobs = [torch.tensor([n_obs], dtype=torch.float64, device=DEV)]
        loss, ll = torch.empty(1, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
        torch.ops.gpsa.elbo_loss_skip_fwd([z.to(DEV)], [Y], noise.to(DEV), [0], [S, N, P], [1], [], [], [], nobs, None, 1.0,
                                          loss, ll, work)
        dn = torch.empty(1, device=DEV)
        g = torch.tensor([1.0], device=DEV)
        torch.ops.gpsa.elbo_loss_skip_bwd([z.to(DEV)], [Y], noise.to(DEV), [0], [S, N, P], [1], [], [], [], nobs, g, 0, 1.0,
                                          [g], dn, None, work)
        s = math.exp(0.25) + 1e-5
        want_ll = (-0.5 * float(z.sum()) + (-math.log(s) - LOG2PI_2) * n_obs * S) / S
        want_dn = -(float(z.sum()) - n_obs * S) / s / S * math.exp(0.25)
        assert abs(float(ll) - want_ll) <= 1e-12 * (abs(want_ll) + 1) and abs(float(dn) - want_dn) <= 1e-6 * (abs(want_dn) + 1e-3)
        if n_obs == 0:
            assert float(ll) == 0.0 and float(dn) == 0.0 and float(loss) == 0.0


# ---- 2. the fused ELBO pass ------------------------------------------------------------------------------------------
def _elbo_inputs(M, L, S, N, gen):
    Cn = S * N
    A = torch.randn(L, M, M, generator=gen, dtype=torch.float64) / math.sqrt(M)
    Om = A @ A.transpose(1, 2) * 0.2
    alpha = torch.randn(M, Cn, generator=gen) * 0.3
    delta = torch.randn(M, L, generator=gen)
    q = torch.rand(Cn, generator=gen, dtype=torch.float64) * 0.3
    eps = torch.randn(Cn, L, generator=gen)
    Y = torch.randn(N, L, generator=gen)
    return Om, alpha, delta, q, eps, Y


@pytest.mark.parametrize("M,delta_form", [(200, True), (64, False)])
def test_quadform_elbo_skip(M, delta_form):
    lib = _build()
    L, S, N = 3, 3, 77  # C = 231 ends inside a column tile
    Cn = S * N
    gen = torch.Generator().manual_seed(MASK_SEED + M)
    Om, alpha, delta, q, eps, Y = _elbo_inputs(M, L, S, N, gen)
    miss = torch.rand(N, L, generator=gen) < 0.3
    miss[:, 1] = True  # one fully missing output
    Ym = torch.where(miss, torch.full_like(Y, NAN), Y)
    var_u, noise_u = torch.tensor([0.3]), torch.tensor([-0.4])
    # fp64 reference with autograd: loss = -LL over the observed entries, at upstream gradient 1
    a64 = alpha.double().requires_grad_(True)
    mean64 = (delta.double().t() @ a64).detach().requires_grad_(True)  # [L, C]
    W = Om @ a64  # [L, M, C]
    v = (a64[None] * W).sum(1)
    var = (math.exp(0.3) - q)[None] + v + 2e-5
    sd = var.sqrt()
    Fd = mean64 + sd * eps.double().t()
    s = math.exp(-0.4) + 1e-5
    Yc = torch.where(miss, torch.zeros_like(Y), Y).double().t().repeat(1, S)  # [L, C], column c -> row c % N
    mc = miss.t().repeat(1, S)
    z = torch.where(mc, torch.zeros_like(Fd), (Yc - Fd) / s)
    loss = 0.5 * (z ** 2).sum() / S
    var.retain_grad()
    dmean_ref, = torch.autograd.grad(loss, [mean64], retain_graph=True)
    g_ref, = torch.autograd.grad(loss, [var], retain_graph=True)
    # abar = 2 sum_l g_l Omega_l alpha: the gradient through v only (the mean's share is not included)
    abar_ref = 2 * (g_ref[:, None, :] * W.detach()).sum(0)
    d = lambda t: t.to(DEV).contiguous()
    al, Omd, dl, qd, ed, Yd = d(alpha), d(Om), d(delta), d(q), d(eps), d(Ym)
    meanT = d((delta.double().t() @ alpha.double()).float())
    nparts = lib.gpsa_quadform_elbo_parts()
    g = torch.full((L, Cn), NAN, device=DEV)
    dm = torch.full((L, Cn), NAN, device=DEV)
    abar = torch.full((M, Cn), NAN, device=DEV)
    FT = torch.full((L, Cn), NAN, device=DEV)
    part = torch.full((nparts,), NAN, dtype=torch.float64, device=DEV)
    wsb = lib.gpsa_quadform_elbo_f32_workspace(M, Cn, L)
    assert wsb > 0
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=DEV)
    vu, nu = d(var_u), d(noise_u)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    if delta_form:
        assert lib.gpsa_quadform_elbo_takes_delta(M) == 1
        rc = lib.gpsa_quadform_elbo_delta_skip_f32(1, p(al), p(Omd), M, Cn, L, p(dl), p(qd), p(vu), p(ed), p(Yd), N, S, p(nu),
                                                   p(g), p(dm), p(abar), p(part), p(FT), p(ws), wsb, C.c_void_p(st))
    else:
        rc = lib.gpsa_quadform_elbo_skip_f32(1, p(al), p(Omd), M, Cn, L, p(meanT), p(qd), p(vu), p(ed), p(Yd), N, S, p(nu),
                                             p(g), p(dm), p(abar), p(part), p(FT), p(ws), wsb, C.c_void_p(st))
    assert rc == 0
    torch.cuda.synchronize()
    mcd = mc.to(DEV)
    assert (g[mcd] == 0).all() and (dm[mcd] == 0).all()  # exactly 0 at the missing entries
    errs = dict(g=_rel(g, g_ref), dmeanT=_rel(dm, dmean_ref), abar=_rel(abar, abar_ref), F=_rel(FT, Fd),
                z2=abs(float(part.sum()) - float((z ** 2).sum())) / float((z ** 2).sum()))
    print(f"[quadform_elbo_skip M={M}]", {k: f"{e:.2e}" for k, e in errs.items()})
    # tests/test_fused_elbo.py's bars for the unmasked kernels against fp64: 3e-5 on gradients, 2e-6 on the loss
    assert errs["g"] <= 3e-5 and errs["dmeanT"] <= 3e-5 and errs["abar"] <= 3e-5 and errs["F"] <= 3e-5
    assert errs["z2"] <= 2e-6


# ---- 3. the fused LMC likelihood -------------------------------------------------------------------------------------
def test_lmc_loglik_fused_skip():
    lib = _build()
    L, P, N, S = 3, 5, 77, 2
    gen = torch.Generator().manual_seed(MASK_SEED + 3)
    F = torch.randn(S, N, L, generator=gen)
    W = torch.randn(L, P, generator=gen)
    Y = torch.randn(N, P, generator=gen)
    miss = torch.rand(N, P, generator=gen) < 0.3
    miss[:, 2] = True
    Ym = torch.where(miss, torch.full_like(Y, NAN), Y)
    noise = torch.tensor([0.1, -0.3])
    F64, W64 = F.double().requires_grad_(True), W.double().requires_grad_(True)
    s = math.exp(-0.3) + 1e-5
    z = torch.where(miss[None], torch.zeros(S, N, P, dtype=torch.float64), (torch.where(miss, torch.zeros_like(Y), Y).double()
                                                                          - F64 @ W64) / s)
    loss = 0.5 * (z ** 2).sum() / S
    dF_ref, dW_ref = torch.autograd.grad(loss, [F64, W64])
    nparts = lib.gpsa_quadform_elbo_parts()
    zpart = torch.full((nparts,), NAN, dtype=torch.float64, device=DEV)
    dF, dW = torch.full((S, N, L), NAN, device=DEV), torch.full((L, P), NAN, device=DEV)
    ws = torch.empty(lib.gpsa_lmc_loglik_workspace(S * N, L, P, nparts) + 64, dtype=torch.uint8, device=DEV)
    torch.ops.gpsa.lmc_loglik_fused_skip(F.to(DEV), W.to(DEV), Ym.to(DEV), noise.to(DEV), 1, zpart, dF, dW, ws)
    torch.cuda.synchronize()
    errs = dict(dF=_rel(dF, dF_ref), dW=_rel(dW, dW_ref),
                z2=abs(float(zpart.sum()) - float((z ** 2).sum())) / float((z ** 2).sum()))
    print("[lmc_loglik_fused_skip]", {k: f"{e:.2e}" for k, e in errs.items()})
    assert errs["dF"] <= 3e-5 and errs["dW"] <= 3e-5 and errs["z2"] <= 2e-6


# ---- 4. whole steps against the masked fp64 oracle -------------------------------------------------------------------
STEP_CASES = ["c1_example_fixed0", "c2_three_free_views", "c5_two_modalities", "c7_m200_conditioning",
              "c10_unequal_two_fixed", "c3_lmc_matern12_warp", "c11_lmc_gtest_unequal"]
_REFS = {}


def _step_mask(g, kind):
    """{modality: missing [N, P]}; "random": 30 % (seed MASK_SEED), redrawn until every (modality, view) keeps an
    observed entry; "panels": the last view measures the first half of the outputs only"""
    gen = torch.Generator().manual_seed(MASK_SEED)
    out = {}
    for m in g.mods:
        N, P = g.Y[m].shape
        sizes = [int(n) for n in g.cfg["n_samples"][m]]
        lo = sum(sizes[:-1])
        if kind == "panels":
            miss = torch.zeros(N, P, dtype=torch.bool)
            miss[lo:, (P + 1) // 2:] = True
            if P == 1:  # nothing to drop from a single output: its last view loses every other row instead
                miss[lo::2, 0] = True
        else:
            while True:
                miss = torch.rand(N, P, generator=gen) < 0.3
                at, ok = 0, True
                for n in sizes:
                    ok = ok and (n == 0 or bool((~miss[at:at + n]).any()))
                    at += n
                if ok:
                    break
        out[m] = miss
    return out


def _masked_reference(name, kind):
    """the fp64 reference of the module docstring, once per (case, mask)"""
    key = (name, kind)
    if key in _REFS:
        return _REFS[key]
    from oracle import gpsa_oracle as orc

    g = Golden(name)
    miss = _step_mask(g, kind)
    st = {}
    for k, v in g.full_state().items():
        t = v.detach().double().clone()
        if k.startswith(orc.TRAINABLE_PREFIXES):
            t.requires_grad_(True)
        st[k] = t
    cfg = g.oracle_cfg()
    view_idx, Ns = orc.make_view_index(g.cfg["n_samples"])
    Gt = {m: t.double() for m, t in g.G_test.items()} if g.G_test is not None else None
    eFt = {m: t.double() for m, t in g.eps_F_test.items()} if g.eps_F_test is not None else None
    out, h = orc.forward_pass(st, cfg, {m: g.X[m].double() for m in g.mods}, view_idx, Ns, g.S,
                              [e.double() for e in g.eps_G], {m: e.double() for m, e in g.eps_F.items()}, Gt, eFt)
    Y0 = {m: torch.where(miss[m], torch.zeros_like(g.Y[m]), g.Y[m]).double() for m in g.mods}
    loss = orc.negative_elbo(st, cfg, h, Y0, out["F_obs"])
    n_mod = len(g.mods)
    for i, m in enumerate(g.mods):
        scale = h["noise_variance_pos"][-n_mod + i]
        lp0 = torch.distributions.Normal(out["F_obs"][m], scale).log_prob(torch.zeros_like(Y0[m]))
        loss = loss + (lp0 * miss[m][None].double()).sum() / out["F_obs"][m].shape[0]
    leaves = {k: t for k, t in st.items() if t.requires_grad}
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    ref = {"loss": loss.detach().numpy()}
    for (k, t), gr in zip(leaves.items(), gs):
        ref[f"grad/{k}"] = (gr if gr is not None else torch.zeros_like(t)).numpy()
    for nm, o in out.items():  # every output of the forward (the masks touch none of them: they are the unmasked step's)
        for m in g.mods:
            ref[f"{nm}/{m}"] = o[m].detach().numpy()
    _REFS[key] = (g, miss, ref)
    return _REFS[key]


OUT_NAMES = ["G_means", "G_samples", "F_latent", "F_obs", "F_latent_test", "F_obs_test"]


def _run_step(model, dd, g):
    """forward, loss_fn, backward as the reference's loop writes them, with the golden's recorded noise -> (the loss,
    every output and every parameter's gradient as numpy; the forward's outputs themselves)"""
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    Gt = {m: g.G_test[m].to(DEV) for m in g.mods} if g.G_test is not None else None
    model.inject_noise(g.eps_G, g.eps_F, g.eps_F_test)
    model.zero_grad()
    out = model.forward({m: dd[m]["spatial_coords"] for m in g.mods}, view_idx=view_idx, Ns=Ns, S=g.S, G_test=Gt)
    loss = model.loss_fn(dd, out[3])
    loss.backward()
    return loss, out


def _collect(model, loss, out, g):
    res = {"loss": loss.detach().cpu().numpy()}
    for nm, o in zip(OUT_NAMES, out):  # (after the step: a lazy handle shows the draws the fused pass wrote)
        for m in g.mods:
            res[f"{nm}/{m}"] = o[m].detach().cpu().numpy()
    for k, p in model.named_parameters():
        res[f"grad/{k}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy()
    return res


def _against(res, ref):
    """every key of the reference - outputs, loss, every gradient - at the hard bar of tests/model_util.compare"""
    errs, bad = {}, {}
    for k, want in ref.items():
        assert k in res, k
        got = res[k]
        assert np.isfinite(got).all(), k
        if np.linalg.norm(want) == 0:
            e = float(np.abs(got).max())
            tol = 0.0
        else:
            e, tol = rel(got, want), 1e-4
        errs[k] = e
        if not e <= tol:
            bad[k] = (e, tol)
    return errs, bad


def _masked_dd(dd, g, miss):
    for m in g.mods:
        dd[m]["outputs"] = torch.where(miss[m].to(DEV), torch.full_like(dd[m]["outputs"], NAN), dd[m]["outputs"])
    return dd


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("kind", ["random", "panels"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_step_matches_masked_fp64_reference(name, kind, fuse):
    from spatial_alignment_amd.lazy import LazyProduct

    _build()
    g, miss, ref = _masked_reference(name, kind)
    model, dd = build_model(g, device=DEV)
    dd = _masked_dd(dd, g, miss)
    model.skip_missing = True
    model.fuse_elbo = fuse
    model.fuse_min_flops = 0  # (the golden cases are tiny: the fused pass would be declined at this size)
    loss, out = _run_step(model, dd, g)
    rec = model._cache.fuse
    lmc = [m for m in g.mods if model.n_latent_gps[m] is not None]
    if not fuse:
        assert rec is None
    elif not lmc:  # the fused pass really ran (gpsa_step_io.skip_missing -> panel_elbo_skip_kernel)
        assert rec is not None and "fused" in rec["state"], "the fused ELBO path did not run"
    for m in lmc:  # a lazy LMC product was never formed: gpsa_lmc_loglik_fused_skip_f32 ran in its place
        if isinstance(out[3][m], LazyProduct):
            assert not out[3][m].is_materialized
    res = _collect(model, loss, out, g)
    assert any(k.startswith("F_obs/") for k in ref) and any(k.startswith("grad/") for k in ref)
    errs, bad = _against(res, ref)
    print(name, kind, "fused" if fuse else "separate", {k: f"{v:.1e}" for k, v in errs.items()})
    assert not bad, bad


# ---- 4b. the loss node's closings, bit for bit -------------------------------------------------------------------------
# tests/golden/loss_node_closings.npz: the loss and every parameter's gradient of one step per closing of the loss node
# (plain, fused, per-view weighted, and each of them over partly observed outputs), through the step engine and - where
# the per-layer path has a closing of its own - through the layers, recorded on one MI355X at a77545a, when the node
# existed as ElboLossFn, WeightedElboLossFn and SkipElboLossFn.  The one node that replaced them runs the same ops on the
# same tables: the comparison is byte for byte.  c10 is the smallest case of STEP_CASES (4 unequal views, 211 x 5); c3
# adds the node's LMC pre-pass (gpsa_lmc_loglik_fused_f32 / _skip_f32).
NODE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_node_closings.npz")
NODE_CLOSINGS = [("c10_unequal_two_fixed", c, e) for e in ("engine", "layers")
                 for c in ("plain", "fused", "weighted", "skip_plain", "skip_fused", "skip_weighted")
                 if e == "engine" or c in ("weighted", "skip_plain", "skip_weighted")]
NODE_CLOSINGS += [("c3_lmc_matern12_warp", c, "engine") for c in ("fused", "skip_fused")]


def _closing_step(name, closing, path):
    """one step of golden case ``name`` through the named closing -> {"loss", "grad/<parameter>": numpy}"""
    _build()
    g = Golden(name)
    model, dd = build_model(g, device=DEV)
    kind = closing.split("_")[-1]
    if closing.startswith("skip"):
        dd = _masked_dd(dd, g, _step_mask(g, "random"))
        model.skip_missing = True
    model.use_step_engine = path == "engine"
    model.fuse_elbo = kind == "fused"
    model.fuse_min_flops = 0
    if kind == "weighted":
        for m in g.mods:  # fp64 weights that no fp32 holds, one per view
            nv = len(g.cfg["n_samples"][m])
            dd[m]["view_weights"] = torch.tensor([(3 + 2 * v) / 7 for v in range(nv)], dtype=torch.float64)
    loss, out = _run_step(model, dd, g)
    if kind == "fused" and model.n_latent_gps[g.mods[0]] is None:
        assert model._cache.fuse is not None and "fused" in model._cache.fuse["state"], "the fused ELBO path did not run"
    res = _collect(model, loss, out, g)
    return {k: v for k, v in res.items() if k == "loss" or k.startswith("grad/")}


@pytest.mark.parametrize("name,closing,path", NODE_CLOSINGS, ids=["-".join((n.split("_")[0], c, p)) for n, c, p in NODE_CLOSINGS])
def test_loss_node_closings_are_the_recorded_bits(name, closing, path):
    rec = np.load(NODE_GOLDEN)
    got = _closing_step(name, closing, path)
    pre = f"{name}/{closing}/{path}/"
    keys = sorted(k[len(pre):] for k in rec.files if k.startswith(pre))
    assert keys == sorted(got) and "loss" in keys and len(keys) > 5, (keys, sorted(got))
    for k in keys:
        want = rec[pre + k]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert np.isfinite(want).all(), k
        assert got[k].tobytes() == want.tobytes(), (k, float(np.abs(got[k].astype(np.float64) - want).max()))


def test_bf16x3_plan_takes_the_fp32_skip_kernel_and_goes_back():
    """contraction = "bf16x3" with skip_missing: the fused ELBO pass runs the fp32 skip kernel inside the x3 plan (its
    scratch holds the larger of the two workspaces), the Gram stays on x3, and plan.contraction / gpsa_step_contraction
    say 2; with the flag off again the same plan runs x3 and both say 3.  Both steps at the hard 1e-4: the masked one
    against the masked fp64 reference, the plain one against the golden's own."""
    from model_util import compare

    _build()
    name = "c7_m200_conditioning"
    g, miss, ref = _masked_reference(name, "random")
    model, dd = build_model(g, device=DEV)
    plain = {m: dd[m]["outputs"].clone() for m in g.mods}
    dd = _masked_dd(dd, g, miss)
    model.contraction = "bf16x3"
    model.fuse_min_flops = 0

    def seen(expect):
        plans = list(model.__dict__.get("_step_plans", {}).values())
        assert plans
        for p in plans:
            assert p.key[-1] == "bf16x3"
            for i, m in enumerate(p.mods):
                assert p.contraction[m] == expect, p.contraction
                assert int(p.lib.gpsa_step_contraction(p.handle, i)) == expect

    model.skip_missing = True
    loss, out = _run_step(model, dd, g)
    assert model._cache.fuse is not None and "fused" in model._cache.fuse["state"]
    errs, bad = _against(_collect(model, loss, out, g), ref)
    print(name, "bf16x3 + skip_missing", {k: f"{v:.1e}" for k, v in errs.items()})
    assert not bad, bad
    seen(2)
    model.skip_missing = False
    for m in g.mods:
        dd[m]["outputs"] = plain[m]
    loss, out = _run_step(model, dd, g)
    assert model._cache.fuse is not None and "fused" in model._cache.fuse["state"]
    bad, errs = compare(_collect(model, loss, out, g), g, tol_out=1e-4, tol_grad=1e-4)
    print(name, "bf16x3, flag off again", {k: f"{v:.1e}" for k, v in errs.items()})
    assert not bad, bad
    seen(3)


def test_counts_of_more_than_64_views():
    """the counting launch takes 64 (term, view) pairs; a call with more loops over them (70 one-row views here)"""
    _build()
    N, P = 70, 3
    gen = torch.Generator().manual_seed(MASK_SEED + 70)
    miss = torch.rand(N, P, generator=gen) < 0.5
    Y = torch.where(miss, torch.full((N, P), NAN), torch.randn(N, P, generator=gen)).to(DEV)
    cws = torch.empty(8 * 64 * 64 + 64, dtype=torch.uint8, device=DEV)
    a = torch.full((40,), -1.0, dtype=torch.float64, device=DEV)
    b = torch.full((30,), -1.0, dtype=torch.float64, device=DEV)
    torch.ops.gpsa.count_observed([Y[:40].contiguous(), Y[40:].contiguous()], [40, 30], list(range(41)) + list(range(31)),
                                  [a, b], cws)
    want = (~miss).sum(1).double()
    assert torch.equal(torch.cat([a, b]).cpu(), want)


def test_counts_are_cached_for_the_very_tensor_only():
    """observed_counts keeps the counts of the caller's own contiguous fp32 outputs, and only for that tensor: another
    tensor with the same key (address, version, shape) is counted again, and a converted copy is never cached"""
    _build()
    from spatial_alignment_amd import step_engine as SE

    class Holder:
        pass

    h = Holder()
    Y = torch.randn(9, 4, device=DEV)
    Y[0, 0] = NAN
    first = SE.observed_counts(h, [Y], None, cacheable=True)
    assert SE.observed_counts(h, [Y], None, cacheable=True) is first and float(first[0]) == 35.0
    # a stand-in that answers with Y's key but is another tensor (what a freed Y's successor at its address looks like)
    Z = torch.randn(9, 4, device=DEV)
    Z[:3] = NAN
    (key, entry), = h._nobs_cache.items()
    h._nobs_cache = {((Z.data_ptr(), Z._version, tuple(Z.shape)),) + key[1:]: entry}
    again = SE.observed_counts(h, [Z], None, cacheable=True)
    assert again is not first and float(again[0]) == 24.0
    # outputs that need a conversion: loss_fn's copy is counted at every step and leaves no cache entry
    g = Golden("c2_three_free_views")
    model, dd = build_model(g, device=DEV)
    m = g.mods[0]
    Y64 = dd[m]["outputs"].double()
    Y64[0, 0] = NAN
    dd[m]["outputs"] = Y64
    model.skip_missing = True
    loss, _ = _run_step(model, dd, g)
    assert math.isfinite(float(loss)) and not model.__dict__.get("_nobs_cache")


def test_flag_off_propagates_nan():
    """off by default: a NaN in the outputs makes the loss NaN, as before"""
    _build()
    g = Golden("c2_three_free_views")
    model, dd = build_model(g, device=DEV)
    assert model.skip_missing is False
    dd[g.mods[0]]["outputs"][0, 0] = NAN
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    model.inject_noise(g.eps_G, g.eps_F, None)
    out = model.forward({m: dd[m]["spatial_coords"] for m in g.mods}, view_idx=view_idx, Ns=Ns, S=g.S)
    assert torch.isnan(model.loss_fn(dd, out[3]))


# ---- 5. minibatch: the mean over a cover of batches is the full masked step ---------------------------------------
@pytest.mark.parametrize("engine", [True, False], ids=["engine", "layers"])
def test_cover_of_masked_batches_is_unbiased(engine):
    import test_minibatch_gpu as T

    MB = T._lib()
    model, dd, eG, eF = T._two_modality_problem()
    gen = torch.Generator().manual_seed(MASK_SEED)
    for m in T.MODS:
        Y = dd[m]["outputs"]
        miss = (torch.rand(Y.shape, generator=gen) < 0.3).to(DEV)
        miss[T.VIEWS[0]:, -1] = True  # view 1 does not measure the last output
        dd[m]["outputs"] = torch.where(miss, torch.full_like(Y, NAN), Y)
    model.skip_missing = True
    model.use_step_engine = engine
    vi, Ns, _, _ = model.create_view_idx_dict(dd)
    full_loss, full_g = T._step(model, dd, vi, Ns, [torch.cat([eG[m] for m in T.MODS], 1)], eF)
    assert math.isfinite(full_loss)
    sampler = MB.RowSampler(model, dd, T.BATCH, seed=17)
    steps = 6
    tot_loss, tot_g = 0.0, {n: torch.zeros_like(x) for n, x in full_g.items()}
    for t in range(steps):
        b = sampler.next()
        rows = {m: b.rows[m] for m in T.MODS}
        free = [torch.cat([eG[m][:, rows[m][200:] - T.VIEWS[0]] for m in T.MODS], 1)]
        l, gr = T._step(model, b.data_dict, b.view_idx, b.Ns, free, {m: eF[m][:, rows[m]] for m in T.MODS})
        tot_loss += l
        for n in tot_g:
            tot_g[n] += gr[n]
    mean_loss = tot_loss / steps
    assert abs(mean_loss - full_loss) <= 1e-5 * abs(full_loss), (mean_loss, full_loss)
    bad = {}
    for n, x in full_g.items():
        e = T._rel(tot_g[n] / steps, x) if float(x.abs().max()) > 0 else float(tot_g[n].abs().max())
        if e > 1e-5:
            bad[n] = e
    assert not bad, bad


# ---- 6. capture: the graphed minibatch step counts the batch it is replayed on --------------------------------------
def test_graphed_masked_svi_step_equals_eager():
    import test_minibatch_gpu as T

    MB = T._lib()
    from spatial_alignment_amd.optim import FusedAdam
    from spatial_alignment_amd.train import GraphedTrainStep, train_step

    B, S = 100, T.S
    gen = torch.Generator().manual_seed(8)
    noise = ([torch.randn(S, B, 2, generator=gen).to(DEV) for _ in range(2)],
             {"expression": torch.randn(S, 2 * B, 6, generator=gen).to(DEV)})
    res, counts = [], []
    for mode in ("eager", "graph"):
        model, dd = T._grid()
        Y = dd["expression"]["outputs"]
        mg = torch.Generator().manual_seed(MASK_SEED)
        miss = (torch.rand(Y.shape, generator=mg) < 0.3).to(DEV)
        dd["expression"]["outputs"] = torch.where(miss, torch.full_like(Y, NAN), Y)
        model.skip_missing = True
        opt = FusedAdam(list(model.parameters()), lr=1e-2)
        sampler = MB.RowSampler(model, dd, B, seed=21)
        vi, Ns, _, _ = model.create_view_idx_dict(dd)
        if mode == "eager":
            for t in range(4):
                host = sampler.host_rows(t)["expression"]
                counts.append(int((~miss.cpu()[host]).sum()))
                loss = train_step(model, opt, dd, vi, Ns, S, sampler=sampler, noise=noise)
        else:
            gs = GraphedTrainStep(model, opt, dd, vi, Ns, S=S, warmup=3, sampler=sampler, noise=noise)
            loss = gs.step()
            gs.check()
        torch.cuda.synchronize()
        assert math.isfinite(float(loss))
        res.append((float(loss), [p.detach().clone() for p in model.parameters()]))
    assert len(set(counts)) > 1, counts  # the observed counts change from step to step
    (l0, p0), (l1, p1) = res
    assert abs(l0 - l1) <= 1e-5 * abs(l0), (l0, l1)
    for a, b in zip(p0, p1):
        assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1.0)


# ---- 7. sharding: the row shares of an emulated world sum to the full masked step ---------------------------------
@pytest.mark.parametrize("fuse", [False, True], ids=["separate", "fused"])
def test_row_shares_sum_to_the_full_masked_step(fuse):
    import test_parallel_gpu as T
    from spatial_alignment_amd.parallel import shard_data_dict, shard_rows

    _build()
    world, n = 4, T.SIDE * T.SIDE
    eG, eF = T._noise()
    mg = torch.Generator().manual_seed(MASK_SEED)
    miss = (torch.rand(2 * n, 6, generator=mg) < 0.3).to(DEV)
    miss[n:, 3:] = True  # the second view measures half of the outputs

    def problem():
        dd, model = T._problem(DEV)
        Y = dd["expression"]["outputs"]
        dd["expression"]["outputs"] = torch.where(miss, torch.full_like(Y, NAN), Y)
        model.skip_missing = True
        model.fuse_min_flops = 0
        return dd, model

    dd, model = problem()
    loss1 = T._grads(model, dd, eG, eF, 1.0)
    assert math.isfinite(float(loss1))
    want = {k: p.grad.detach().double().clone() for k, p in model.named_parameters()}
    tot, acc = 0.0, {k: torch.zeros_like(v) for k, v in want.items()}
    for r in range(world):
        dd_r, model_r = problem()
        sdd = shard_data_dict(dd_r, r, world)
        lo, hi = shard_rows(n, r, world)
        rows = torch.cat([torch.arange(lo, hi), n + torch.arange(lo, hi)])
        tot += float(T._grads(model_r, sdd, [e[:, lo:hi] for e in eG], eF[:, rows], 1.0, fuse=fuse, owner=(r, world)))
        for k, p in model_r.named_parameters():
            acc[k] += p.grad.detach().double()
    assert abs(tot - float(loss1)) <= 1e-5 * abs(float(loss1)), (tot, float(loss1))
    for k in want:
        e = float((acc[k] - want[k]).norm()) / max(float(want[k].norm()), 1e-6)
        assert e <= 1e-4, (k, e)
