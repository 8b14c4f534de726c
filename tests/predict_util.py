"""Expected values for predict(): the mixture moments in plain fp64 torch, fed from the oracle's restatement of the
reference's forward (never from the code under test).  Shared by tests/test_predict.py (CPU) and
tests/test_predict_gpu.py."""
import math

import torch

from oracle import gpsa_oracle as orc

f64 = torch.float64


def moments_from_samples(mu, sig2, W=None, tau=None, include_noise=False, Y=None):
    """mu, sig2 [S, N, L] fp64 (per-sample conditional mean / variance of the data GP) -> dict of the moments of the
    mixture over S: F_mean, F_var [N, P], F_latent_mean, F_latent_var [N, L], lpd [N] (with Y), by the issue's formulas"""
    mu, sig2 = mu.to(f64), sig2.to(f64)
    S = mu.shape[0]
    if W is not None:
        W = W.to(f64)
        m, u = mu @ W, sig2 @ (W * W)
    else:
        m, u = mu, sig2
    out = dict(F_latent_mean=mu.mean(0), F_latent_var=sig2.mean(0) + ((mu - mu.mean(0)) ** 2).mean(0))
    Fm = m.mean(0)
    out["F_mean"] = Fm
    out["F_var"] = u.mean(0) + ((m - Fm) ** 2).mean(0) + (float(tau) ** 2 if include_noise else 0.0)
    if Y is not None:
        w = u + float(tau) ** 2
        Y = Y.to(f64)
        logp = -0.5 * (math.log(2 * math.pi) + torch.log(w) + (Y.unsqueeze(0) - m) ** 2 / w)  # [S, N, P]
        mix = torch.logsumexp(logp, 0) - math.log(S)
        mix = torch.where(torch.isnan(Y), torch.zeros_like(mix), mix)  # NaN observations contribute 0
        out["lpd"] = mix.sum(1)
        out["lpd_sum"] = out["lpd"].sum()
    return out


def _forward(g, state, S, eps_G, c_F, G_test=None):
    """the oracle's forward in fp64 with eps_F = c_F everywhere"""
    st = {k: v.double() for k, v in state.items()}
    vi, Ns = orc.make_view_index(g.cfg["n_samples"])
    X = {m: g.X[m].double() for m in g.mods}
    L = {m: st[f"delta_F_dict.{m}"].shape[1] for m in g.mods}
    eF = {m: torch.full((S, Ns[m], L[m]), c_F, dtype=f64) for m in g.mods}
    Gt = eFt = None
    if G_test is not None:
        Gt = {m: G_test[m].double() for m in g.mods}
        eFt = {m: torch.full(tuple(Gt[m].shape[:2]) + (L[m],), c_F, dtype=f64) for m in g.mods}
    out, _ = orc.forward_pass(st, g.oracle_cfg(), X, vi, Ns, S, [e.double() for e in eps_G], eF, Gt, eFt)
    return out


def fresh_eps_G(g, S, seed=1):
    """standard-normal warp draws in the fixture's layout (one [S, n_v, D] per non-fixed, non-empty view)"""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn((S,) + tuple(e.shape[1:]), generator=gen, dtype=torch.float32) for e in g.eps_G]


def oracle_prediction(g, S, eps_G, state=None, Y=None, include_noise=False, G_test=None):
    """{mod: dict} of every field predict() returns, from two oracle forwards (eps_F = 0: F_latent is mu_s; eps_F = 1:
    F_latent - mu_s is sqrt(sigma2_s)) and two more for the warp's scale (eps_G = 0 / 1).  ``eps_G`` None: warp="mean"
    (one sample with eps = 0).  ``G_test`` {mod: [S_t, n, D]}: the data-GP fields at those points."""
    state = g.full_state() if state is None else state
    if eps_G is None:
        S, eps_G = 1, [torch.zeros((1,) + tuple(e.shape[1:])) for e in g.eps_G]
    o0, o1 = _forward(g, state, S, eps_G, 0.0, G_test), _forward(g, state, S, eps_G, 1.0, G_test)
    zeros = [torch.zeros((1,) + tuple(e.shape[1:])) for e in g.eps_G]
    ones = [torch.ones((1,) + tuple(e.shape[1:])) for e in g.eps_G]
    w0, w1 = _forward(g, state, 1, zeros, 0.0), _forward(g, state, 1, ones, 0.0)
    key = "F_latent_test" if G_test is not None else "F_latent"
    nm = len(g.mods)
    res = {}
    for i, m in enumerate(g.mods):
        mu = o0[key][m]
        sig2 = (o1[key][m] - mu) ** 2
        W = state[f"W_dict.{m}"].double() if g.cfg["n_latent_gps"].get(m) is not None else None
        nz = state["noise_variance"].double()
        tau = torch.exp(nz[nz.numel() - nm + i]) + orc.JITTER
        r = moments_from_samples(mu, sig2, W, tau, include_noise, None if Y is None else Y[m])
        r["G_mean"] = o0["G_means"][m]
        r["G_scale"] = w1["G_samples"][m][0] - w0["G_samples"][m][0]
        res[m] = r
    return res


def compare_prediction(got, want, fields=None, bar=1e-4, tag=""):
    """norm-wise relative error of every field against the oracle-derived value; prints what is measured, returns the
    violations of ``bar`` (the project's output contract against the reference's fp64 arithmetic)"""
    from golden_io import rel

    bad = {}
    for m, w in want.items():
        for k, ref in w.items():
            if fields is not None and k not in fields:
                continue
            val = got[m][k]
            assert val is not None, (m, k)
            e = rel(val.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy())
            print(f"[predict parity] {tag} {m}/{k}: {e:.2e} (bar {bar:.0e})")
            if not e <= bar:
                bad[f"{m}/{k}"] = e
    return bad
