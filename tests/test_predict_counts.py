"""predict(scale="response") on the CPU: the quadrature rule itself, the arguments, the C signature and the whole call
on the TEST-ONLY fake backend.

The Poisson-lognormal log density has no closed form.  The reference everywhere is a dense trapezoid integral in fp64
(tests/predict_counts_util.py), fed with the oracle's per-sample moments; the rule under test is Gauss-Hermite with
``predict.GH_NODES`` centred on the integrand's mode after ``predict.NEWTON_ITERATIONS`` Newton iterations.  Measured,
rule against brute force on the grid y in {0, 1, 2, 5, 10, 30, 100, 300, 1000}, mu in {-6 .. 7}, u in {1e-6 .. 4}, worst
|error| / max(1, |lpd|): 1.9e-10 (u <= 0.5), 2.0e-8 (u <= 1), 1.8e-6 (u <= 2), 4.6e-5 (u <= 4); the test holds the rule to
3x these, which pins the table of constants.  The kernel gpsa_predict_counts_f32 is exercised by
tests/test_predict_counts_gpu.py."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from golden_io import Golden
from model_util import build_model
from predict_counts_util import counts_and_offsets, oracle_counts, pln_logpdf_brute
from predict_util import compare_prediction, fresh_eps_G, oracle_prediction
from spatial_alignment_amd import _lib
from spatial_alignment_amd import ops as ops_mod
from test_predict import PredictFakeOps

P = importlib.import_module("spatial_alignment_amd.predict")  # (the package's ``predict`` is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
# the rule (Q = 20, K = 8) against brute force per range of u, as measured (module docstring)
MEASURED = ((0.5, 1.9e-10), (1.0, 2.0e-8), (2.0, 1.8e-6), (4.0, 4.6e-5))
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def rule_logpdf(y, mu, u):
    """the rule of csrc/predict_counts.hip restated in fp64 numpy from predict.GH_NODES: log Int Poisson(y; e^eta)
    Normal(eta; mu, u) d eta"""
    x = np.array([n[0] for n in P.GH_NODES])
    lw = np.array([n[1] for n in P.GH_NODES])
    with np.errstate(divide="ignore"):
        e = np.minimum(mu + u * y, np.maximum(mu, np.log(y)))
    for _ in range(P.NEWTON_ITERATIONS):
        E = np.exp(e)
        e = e + (u * (y - E) - (e - mu)) / (u * E + 1.0)
    s2 = 1.0 / (np.exp(e) + 1.0 / u)
    eta = e[..., None] + np.sqrt(2.0 * s2)[..., None] * x
    terms = y[..., None] * eta - np.exp(eta) - (eta - mu[..., None]) ** 2 / (2.0 * u[..., None]) + lw
    top = terms.max(-1)
    lse = top + np.log(np.exp(terms - top[..., None]).sum(-1))
    return lse + 0.5 * np.log(2.0 * s2) - 0.5 * np.log(2.0 * math.pi * u) - _lgamma(y + 1.0)


def test_rule_against_brute_force_on_the_grid():
    ys = np.array([0, 1, 2, 5, 10, 30, 100, 300, 1000.0])
    mus = np.arange(-6.0, 8.0)
    us = np.array([1e-6, 2e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.25, 0.5, 1.0, 2.0, 4.0])
    y, mu, u = np.meshgrid(ys, mus, us, indexing="ij")
    want = pln_logpdf_brute(y, mu, u)
    err = np.abs(rule_logpdf(y, mu, u) - want) / np.maximum(1.0, np.abs(want))
    lo = 0.0
    for hi, measured in MEASURED:
        worst = float(err[(u > lo) & (u <= hi)].max())
        print(f"[counts rule] {lo} < u <= {hi}: {worst:.2e} (measured {measured:.1e}, bar 3x)")
        assert worst <= 3 * measured, (hi, worst)
        lo = hi


def test_the_table_is_the_gauss_hermite_rule_and_the_kernel_carries_it():
    assert len(P.GH_NODES) == 20 and P.NEWTON_ITERATIONS == 8
    x, w = np.polynomial.hermite.hermgauss(20)
    got = np.array(P.GH_NODES)
    assert np.abs(got[:, 0] - x).max() <= 1e-14 and np.abs(got[:, 1] - (np.log(w) + x * x)).max() <= 1e-13
    src = open(os.path.join(ROOT, "spatial_alignment_amd", "csrc", "predict_counts.hip")).read()
    body = src[src.index("PCNT_GH[PCNT_HALF_Q][2] = {"):]
    body = body[:body.index("};")]
    pairs = [(float(a), float(b)) for a, b in re.findall(r"\{\s*([-0-9.e]+),\s*([-0-9.e]+)\s*\}", body)]
    assert pairs == [tuple(n) for n in P.GH_NODES[10:]]  # the positive half; the kernel mirrors it
    assert [(-a, b) for a, b in reversed(pairs)] == [tuple(n) for n in P.GH_NODES[:10]]
    assert re.search(r"PCNT_NEWTON = 8;", src) and re.search(r"PCNT_HALF_Q = 10;", src)


def test_ctypes_signature_matches_the_header():
    src = open(os.path.join(ROOT, "include", "gpsa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+gpsa_predict_counts_f32\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "gpsa_predict_counts_f32 is not declared in include/gpsa_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["meanT", "v", "q", "var_u", "c", "S", "L", "P", "W", "log_offset", "Y", "Y_mean", "Y_var", "lpd",
                     "stream"]
    import ctypes as C

    def ctype(a):
        if "*" in a:
            return C.c_void_p
        return {"long long": C.c_longlong, "int": C.c_int, "double": C.c_double}[" ".join(a.split()[:-1])]

    res, argtypes = _lib.SIGNATURES["gpsa_predict_counts_f32"]
    assert res is C.c_int and argtypes == [ctype(a) for a in args]


# ---- the whole call on the fake backend -----------------------------------------------------------------------------------
class CountsFakeOps(PredictFakeOps):
    """PredictFakeOps + the contract of gpsa_predict_counts_f32: the lognormal moments in fp64 torch and the node rule
    above for lpd"""

    def predict_counts(self, meanT, v, q, var_u, S, W=None, log_offset=None, Y=None, out=None):
        L, SC = meanT.shape
        c = SC // S
        resid = torch.exp(var_u.reshape(-1)[0].double()) - q.double()
        mu = meanT.double().reshape(L, S, c).permute(1, 2, 0)
        sg = (resid.unsqueeze(0) + v.double() + 2e-5).reshape(L, S, c).permute(1, 2, 0)
        Wd = None if W is None else W.double()
        m, u = (mu, sg) if Wd is None else (mu @ Wd, sg @ (Wd * Wd))
        if log_offset is not None:
            m = m + log_offset.double()[None, :, None]
        lam = torch.exp(m + 0.5 * u)
        d = lam - lam[0]
        mean_d = d.mean(0)
        Ym = lam[0] + mean_d
        Yv = Ym + (lam * lam * torch.expm1(u)).mean(0) + ((d * d).mean(0) - mean_d * mean_d).clamp_min(0)
        lpd = None
        if Y is not None:
            Yd = Y.double()
            y0 = torch.where(torch.isnan(Yd), torch.zeros_like(Yd), Yd)
            logp = torch.from_numpy(rule_logpdf(y0.unsqueeze(0).expand_as(m).numpy(), m.numpy(), u.numpy()))
            mix = torch.logsumexp(logp, 0) - math.log(S)
            lpd = torch.where(torch.isnan(Yd), torch.zeros_like(mix), mix).sum(1)
        res = (Ym.float(), Yv.float(), lpd)
        if out is None:
            return res
        for dst, src in zip(out, res):
            assert (dst is None) == (src is None)
            if dst is not None:
                dst.copy_(src)
        return out


@pytest.fixture(autouse=True)
def fake_backend():
    ops_mod.set_ops(CountsFakeOps())
    yield
    ops_mod.set_ops(None)


def _setup(name, pois):
    g = Golden(name)
    model, dd = build_model(g)
    model.likelihood = "poisson" if len(pois) == len(g.mods) else {m: "poisson" for m in pois}
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    return g, model, X, view_idx, Ns


def _compare_counts(got, want, tag):
    bad = {}
    from golden_io import rel

    for m, w in want.items():
        assert w["max_u"] <= 4.0, (m, w["max_u"])  # the rule's measured domain: a condition on the reference's inputs
        for k in ("Y_mean", "Y_var", "lpd", "lpd_sum"):
            if k not in w:
                continue
            e = rel(got[m][k].detach().cpu().double().numpy(), w[k].numpy())
            print(f"[predict counts] {tag} {m}/{k}: {e:.2e} (bar {BAR:.0e}; max u {w['max_u']:.2f})")
            if not e <= BAR:
                bad[f"{m}/{k}"] = e
    return bad


def test_mixed_modalities_in_one_call():
    g, model, X, view_idx, Ns = _setup("c5_two_modalities", ["rna"])
    S = 3
    eps = fresh_eps_G(g, S)
    Y, off = counts_and_offsets(g, ["rna"])
    Y["rna"][1::7, 0] = float("nan")
    Y["rna"][3] = float("nan")
    got = model.predict(X, view_idx, Ns, S=S, eps_G=eps, Y=Y, scale="response", log_offset=off)
    want = oracle_counts(g, S, eps, ["rna"], Y=Y, offset=off)
    assert not _compare_counts(got, want, "c5")
    assert float(got["rna"].lpd[3]) == 0.0 and got["rna"].lpd.dtype == torch.float64
    assert torch.equal(got["rna"].lpd_sum, got["rna"].lpd.sum())
    # the log-rate fields are what the default call returns, and the Gaussian modality is the default call's
    link = model.predict(X, view_idx, Ns, S=S, eps_G=eps)
    assert "Y_mean" not in link["rna"] and "Y_var" not in link["protein"]
    for m in g.mods:
        for k in ("G_mean", "G_scale", "F_mean", "F_var"):
            assert torch.equal(link[m][k], got[m][k]), (m, k)
    model.likelihood = "gaussian"  # the Gaussian modality against the link call WITH Y (refused while rna is Poisson)
    ref = model.predict(X, view_idx, Ns, S=S, eps_G=eps, Y={"rna": g.Y["rna"], "protein": Y["protein"]})
    model.likelihood = {"rna": "poisson"}
    assert torch.equal(got["protein"].Y_mean, ref["protein"].F_mean) and torch.equal(got["protein"].lpd, ref["protein"].lpd)
    want_g = oracle_prediction(g, S, eps, Y=Y, include_noise=True)
    e = float((got["protein"].Y_var.double() - want_g["protein"]["F_var"]).norm() / want_g["protein"]["F_var"].norm())
    assert e <= BAR, e
    # include_noise changes F_var and leaves Y_var of either modality alone
    noisy = model.predict(X, view_idx, Ns, S=S, eps_G=eps, Y=Y, scale="response", log_offset=off, include_noise=True)
    for m in g.mods:
        torch.testing.assert_close(noisy[m].Y_var, got[m].Y_var, rtol=1e-6, atol=0)
    assert not torch.equal(noisy["protein"].F_var, got["protein"].F_var)
    # without offsets, without Y
    got0 = model.predict(X, view_idx, Ns, S=S, eps_G=eps, scale="response")
    assert got0["rna"].lpd is None and got0["protein"].lpd is None
    assert not _compare_counts(got0, oracle_counts(g, S, eps, ["rna"]), "c5 no offsets, no Y")


def test_lmc_at_g_test_and_chunks():
    g, model, X, view_idx, Ns = _setup("c11_lmc_gtest_unequal", ["expression"])
    m = g.mods[0]
    nt = g.G_test[m].shape[1]
    Yall, _ = counts_and_offsets(g, [m])
    Yt = {m: Yall[m][:nt].clone()}
    Yt[m][2, 1] = float("nan")
    off = {m: 0.25 * torch.sin(torch.arange(nt, dtype=torch.float32))}
    want = oracle_counts(g, g.S, g.eps_G, [m], Y=Yt, offset=off, G_test=g.G_test)
    runs = [model.predict(G_test=g.G_test, Y=Yt, scale="response", log_offset=off, rows_per_chunk=c) for c in (10**6, 4)]
    for r in runs:
        assert not _compare_counts(r, want, "c11 G_test")
    for k in ("Y_mean", "Y_var", "lpd"):  # (to rounding here: torch's CPU matmul blocks by shape; bitwise on the device)
        torch.testing.assert_close(runs[0][m][k], runs[1][m][k], rtol=1e-5, atol=1e-6)
    # the rows' own samples, warp="mean"
    Y, off = counts_and_offsets(g, [m])
    got = model.predict(X, view_idx, Ns, warp="mean", Y=Y, scale="response", log_offset=off)
    assert not _compare_counts(got, oracle_counts(g, 1, None, [m], Y=Y, offset=off), "c11 warp=mean")


def test_scale_and_log_offset_are_validated():
    g, model, X, view_idx, Ns = _setup("c5_two_modalities", ["rna"])
    Y, off = counts_and_offsets(g, ["rna"])
    with pytest.raises(ValueError, match="scale must be"):
        model.predict(X, view_idx, Ns, scale="counts")
    with pytest.raises(ValueError, match=r"(?s)Poisson.*scale=\"response\""):  # the default call still refuses
        model.predict(X, view_idx, Ns, Y=Y)
    with pytest.raises(ValueError, match="Poisson"):
        model.predict(X, view_idx, Ns, Y=Y, scale="link")
    with pytest.raises(ValueError, match="log_offset was given with scale='link'"):
        model.predict(X, view_idx, Ns, log_offset=off)
    with pytest.raises(ValueError, match=r"log_offset\['protein'\].*Gaussian likelihood.*model.likelihood"):
        model.predict(X, view_idx, Ns, scale="response", log_offset={"protein": torch.zeros(int(Ns["protein"]))})
    with pytest.raises(ValueError, match=r"log_offset\['rna'\] has shape"):
        model.predict(X, view_idx, Ns, scale="response", log_offset={"rna": off["rna"][:-1]})
    with pytest.raises(ValueError, match="log_offset names the modality"):
        model.predict(X, view_idx, Ns, scale="response", log_offset={"atac": off["rna"]})
    with pytest.raises(ValueError, match=r"Y\['rna'\] has shape"):
        model.predict(X, view_idx, Ns, scale="response", Y={**Y, "rna": Y["rna"][:, :-1]})
    # the default results are exactly as before: no new keys
    out = model.predict(X, view_idx, Ns, S=2)
    assert all(set(out[m]) == {"G_mean", "G_scale", "F_mean", "F_var", "F_latent_mean", "F_latent_var", "lpd", "lpd_sum"}
               for m in g.mods)
    import gpsa

    assert not compare_prediction(gpsa.predict(model, X, view_idx, Ns, S=2, eps_G=fresh_eps_G(g, 2)),
                                  oracle_prediction(g, 2, fresh_eps_G(g, 2)), fields=("G_mean", "G_scale", "F_mean", "F_var"),
                                  bar=BAR, tag="default call")
