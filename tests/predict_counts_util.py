"""Expected values for predict(scale="response"): the lognormal closed forms and a BRUTE-FORCE Poisson-lognormal integral
in fp64 numpy, fed from the oracle's restatement of the reference's forward (never from the node rule or the code under
test).  Shared by tests/test_predict_counts.py (CPU) and tests/test_predict_counts_gpu.py."""
import math

import numpy as np
import torch

from predict_util import _forward

f64 = torch.float64
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def pln_logpdf_brute(y, mu, u, n=2001, block=4096):
    """log Int Poisson(y; e^eta) Normal(eta; mu, u) d eta, entry-wise over arrays of one shape, by a dense trapezoid sum.
    h(eta) = y eta - e^eta - (eta - mu)^2 / (2u) is concave with h'' <= -1/u everywhere and h'' <= -1/s^2 right of its
    mode (s^2 = 1 / (e^mode + 1/u)): the mode comes from 60 Newton iterations, the grid runs from where h has dropped
    45 nats on the left (found by widening; 9.5 sqrt(u) always suffices) to 9.5 s on the right (h has dropped >= 45
    there), and n points keep the step below s/2 (asserted) - the trapezoid sum of a bump this smooth is then exact to
    rounding: its error falls like exp(-2 pi^2 s^2 / step^2) (n = 2001 and n = 8001 agree to 2e-12 on the CPU test's grid)."""
    y, mu, u = (np.ascontiguousarray(np.broadcast_arrays(y, mu, u)[i], dtype=np.float64) for i in range(3))
    shape = y.shape
    y, mu, u = y.ravel(), mu.ravel(), u.ravel()
    out = np.empty_like(y)
    wts = np.ones(n)
    wts[0] = wts[-1] = 0.5
    tt = np.linspace(0.0, 1.0, n)
    for a in range(0, y.size, block):
        yb, mb, ub = y[a: a + block], mu[a: a + block], u[a: a + block]
        with np.errstate(divide="ignore"):
            e = np.minimum(mb + ub * yb, np.maximum(mb, np.log(yb)))
        for _ in range(60):
            E = np.exp(e)
            e = e + (ub * (yb - E) - (e - mb)) / (ub * E + 1.0)
        s = np.sqrt(ub / (ub * np.exp(e) + 1.0))
        h = lambda z: yb * z - np.exp(z) - (z - mb) ** 2 / (2 * ub)
        h0 = h(e)
        aR = 9.5 * s
        aL = 9.5 * s
        for _ in range(40):
            aL = np.where(h0 - h(e - aL) < 45.0, aL * 1.5, aL)
        aL = np.minimum(aL, 9.5 * np.sqrt(ub))
        assert ((aL + aR) / (n - 1) <= 0.5 * s).all(), "the grid is too coarse for this entry"
        z = (e - aL)[:, None] + (aL + aR)[:, None] * tt
        hz = yb[:, None] * z - np.exp(z) - (z - mb[:, None]) ** 2 / (2 * ub[:, None])
        integral = (np.exp(hz - h0[:, None]) * wts).sum(1) * (aL + aR) / (n - 1)
        out[a: a + block] = h0 + np.log(integral) - 0.5 * np.log(2 * math.pi * ub) - _lgamma(yb + 1.0)
    return out.reshape(shape)


def counts_from_samples(mu, sig2, W=None, offset=None, Y=None):
    """mu, sig2 [S, N, L] fp64 (the data GP's per-sample conditional mean / variance) -> the fields of a Poisson modality
    (formulas: spatial_alignment_amd/predict.py's docstring): Y_mean, Y_var [N, P]; with Y lpd [N], lpd_sum; also max_u / max_eta of the inputs"""
    mu, sig2 = mu.to(f64), sig2.to(f64)
    S = mu.shape[0]
    if W is not None:
        W = W.to(f64)
        m, u = mu @ W, sig2 @ (W * W)
    else:
        m, u = mu, sig2
    if offset is not None:
        m = m + offset.to(f64)[None, :, None]
    lam = torch.exp(m + 0.5 * u)
    Ym = lam.mean(0)
    out = dict(Y_mean=Ym, Y_var=Ym + (lam * lam * torch.expm1(u)).mean(0) + ((lam - Ym) ** 2).mean(0),
               max_u=float(u.max()), max_eta=float((m + 3 * torch.sqrt(u)).max()))
    if Y is not None:
        Yd = Y.to(f64)
        y0 = torch.where(torch.isnan(Yd), torch.zeros_like(Yd), Yd)
        logp = torch.from_numpy(pln_logpdf_brute(y0.unsqueeze(0).expand_as(m).numpy(), m.numpy(), u.numpy()))
        mix = torch.logsumexp(logp, 0) - math.log(S)
        mix = torch.where(torch.isnan(Yd), torch.zeros_like(mix), mix)  # NaN observations contribute 0
        out["lpd"] = mix.sum(1)
        out["lpd_sum"] = out["lpd"].sum()
    return out


def counts_and_offsets(g, pois_mods):
    """counts and offsets as tests/test_poisson_gpu.py makes them from a fixture: y = floor(exp(clamp(Y, max=3))),
    o[n] = 0.25 sin n (Gaussian modalities keep their Y and get no offsets)"""
    Y = {m: torch.floor(torch.exp(torch.clamp(g.Y[m], max=3.0))) if m in pois_mods else g.Y[m].clone() for m in g.mods}
    off = {m: 0.25 * torch.sin(torch.arange(g.Y[m].shape[0], dtype=torch.float32)) for m in pois_mods}
    return Y, off


def oracle_counts(g, S, eps_G, pois_mods, Y=None, offset=None, G_test=None, state=None):
    """{mod: counts_from_samples(...)} for the Poisson modalities, from two oracle forwards (eps_F = 0: mu_s; eps_F = 1:
    mu_s + sqrt(sigma2_s)) as predict_util.oracle_prediction gets them.  ``eps_G`` None: warp="mean"."""
    state = g.full_state() if state is None else state
    if eps_G is None:
        S, eps_G = 1, [torch.zeros((1,) + tuple(e.shape[1:])) for e in g.eps_G]
    o0, o1 = _forward(g, state, S, eps_G, 0.0, G_test), _forward(g, state, S, eps_G, 1.0, G_test)
    key = "F_latent_test" if G_test is not None else "F_latent"
    res = {}
    for m in pois_mods:
        mu = o0[key][m]
        sig2 = (o1[key][m] - mu) ** 2
        W = state[f"W_dict.{m}"].double() if g.cfg["n_latent_gps"].get(m) is not None else None
        res[m] = counts_from_samples(mu, sig2, W, None if offset is None else offset.get(m), None if Y is None else Y[m])
    return res


def relmax(got, want):
    """entry-wise relative error, worst entry"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def lpd_err(got, want):
    """|error| / max(1, |reference|), worst entry"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
