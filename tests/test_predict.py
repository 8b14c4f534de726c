"""predict() on the CPU: the driver (argument checks, M x M stage, warp stage, row chunks, G_test, no side effects) on the
TEST-ONLY fake backend, every returned field against values derived from the oracle's restatement of the reference's
forward in fp64 (tests/predict_util.py).  Bar: the project's output contract, 1e-4 norm-wise.  The HIP kernel
gpsa_predict_moments_f32 is exercised by tests/test_predict_gpu.py."""
import math

import pytest
import torch

from fake_ops import FakeOps
from golden_io import Golden
from model_util import build_model
from predict_util import compare_prediction, fresh_eps_G, oracle_prediction
from spatial_alignment_amd import ops as ops_mod

CASES = ["c1_example_fixed0", "c3_lmc_matern12_warp", "c5_two_modalities", "c10_unequal_two_fixed",
         "c11_lmc_gtest_unequal"]
BAR = 1e-4


class PredictFakeOps(FakeOps):
    """FakeOps + the contract of gpsa_predict_moments_f32, restated with running sums over the samples in fp64 torch"""

    def predict_moments(self, meanT, v, q, var_u, S, W=None, noise_u=None, include_noise=False, Y=None, latent=False,
                        out=None):
        f64 = torch.float64
        L, SC = meanT.shape
        c = SC // S
        resid = torch.exp(var_u.reshape(-1)[0].double()) - q.double()
        mu = meanT.double().reshape(L, S, c).permute(1, 2, 0)                          # [S, c, L]
        sg = (resid.unsqueeze(0) + v.double() + 2e-5).reshape(L, S, c).permute(1, 2, 0)
        tau2 = 0.0 if noise_u is None else float(torch.exp(noise_u.reshape(-1)[0].double()) + 1e-5) ** 2

        def close(m, u, noise, Yc):
            m0 = m[0]
            sd, sdd, su = torch.zeros_like(m0), torch.zeros_like(m0), torch.zeros_like(m0)
            mx = torch.full_like(m0, -math.inf)
            acc = torch.zeros_like(m0)
            for s in range(S):
                d = m[s] - m0
                sd, sdd, su = sd + d, sdd + d * d, su + u[s]
                if Yc is not None:
                    w = u[s] + tau2
                    t = -0.5 * (math.log(2 * math.pi) + torch.log(w) + (Yc - m[s]) ** 2 / w)
                    new = torch.maximum(mx, t)
                    acc = acc * torch.exp(mx - new) + torch.exp(t - new)
                    mx = new
            mean_d = sd / S
            var = su / S + (sdd / S - mean_d * mean_d).clamp_min(0) + (tau2 if noise else 0.0)
            lpd = None
            if Yc is not None:
                lp = mx + torch.log(acc) - math.log(S)
                lpd = torch.where(torch.isnan(Yc), torch.zeros_like(lp), lp).sum(1)
            return m0 + mean_d, var, lpd

        Wd = None if W is None else W.double()
        m, u = (mu, sg) if Wd is None else (mu @ Wd, sg @ (Wd * Wd))
        Fm, Fv, lpd = close(m, u, include_noise, None if Y is None else Y.double())
        Lm = Lv = None
        if latent:
            Lm, Lv, _ = close(mu, sg, False, None)
        res = (Fm.float(), Fv.float(), None if Lm is None else Lm.float(), None if Lv is None else Lv.float(), lpd)
        if out is None:
            return res
        for dst, src in zip(out, res):
            assert (dst is None) == (src is None)
            if dst is not None:
                dst.copy_(src)
        return out


@pytest.fixture(autouse=True)
def fake_backend():
    ops_mod.set_ops(PredictFakeOps())
    yield
    ops_mod.set_ops(None)


def _setup(name):
    g = Golden(name)
    model, dd = build_model(g)
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    return g, model, X, view_idx, Ns


def _y_with_nans(g):
    Y = {m: g.Y[m].clone() for m in g.mods}
    for m in g.mods:
        Y[m][1::7, 0] = float("nan")
        Y[m][3] = float("nan")  # a row without any observation scores 0
    return Y


@pytest.mark.parametrize("name", CASES)
def test_every_field_matches_the_oracle(name):
    g, model, X, view_idx, Ns = _setup(name)
    S = 4
    eps = fresh_eps_G(g, S)
    Y = _y_with_nans(g)
    for include_noise in (False, True):
        want = oracle_prediction(g, S, eps, Y=Y, include_noise=include_noise)
        got = model.predict(X, view_idx, Ns, S=S, eps_G=eps, Y=Y, include_noise=include_noise, latent=True)
        assert not compare_prediction(got, want, bar=BAR, tag=f"{name} S=4 noise={include_noise}")
    for m in g.mods:
        assert got[m].lpd.dtype == torch.float64 and tuple(got[m].lpd.shape) == (int(Ns[m]),)
        assert float(got[m].lpd[3]) == 0.0
        assert torch.isfinite(got[m].lpd).all()
    # the plug-in variant: one sample with eps = 0
    want = oracle_prediction(g, 1, None, Y=Y)
    got = model.predict(X, view_idx, Ns, S=7, warp="mean", Y=Y, latent=True)
    assert not compare_prediction(got, want, bar=BAR, tag=f"{name} warp=mean")


@pytest.mark.parametrize("name", CASES)
def test_result_does_not_depend_on_the_chunking(name):
    g, model, X, view_idx, Ns = _setup(name)
    eps = fresh_eps_G(g, 4)
    Y = {m: g.Y[m] for m in g.mods}
    runs = [model.predict(X, view_idx, Ns, S=4, eps_G=eps, Y=Y, latent=True, rows_per_chunk=c)
            for c in (10**6, 37, 1)]
    want = oracle_prediction(g, 4, eps, Y=Y)
    for r in runs[1:]:
        for m in g.mods:
            for k, t in runs[0][m].items():
                # a row's arithmetic does not depend on its neighbours; torch's CPU matmul picks its blocking by shape,
                # so equality is held to rounding here (bitwise on the device: tests/test_predict_gpu.py)
                torch.testing.assert_close(r[m][k], t, rtol=1e-5, atol=1e-6, equal_nan=True)
        assert not compare_prediction(r, want, bar=BAR, tag=f"{name} chunked")


def test_g_test_moments_without_the_training_rows():
    g, model, X, view_idx, Ns = _setup("c11_lmc_gtest_unequal")
    m = g.mods[0]
    want = oracle_prediction(g, g.S, g.eps_G, G_test=g.G_test)
    # the data GP must not run on the training rows: count the columns its covariance is asked for
    seen = []
    inner = ops_mod.get_ops()
    kmat = inner.kmat
    inner.kmat = lambda kind, Z, Xc, *a, **k: (seen.append(Xc.shape[0]), kmat(kind, Z, Xc, *a, **k))[1]
    got = model.predict(G_test=g.G_test, latent=True)
    St, nt = g.G_test[m].shape[:2]
    assert max(seen) <= max(St * nt, model.Gtilde.shape[0]) and got[m].G_mean is None
    data_fields = ("F_mean", "F_var", "F_latent_mean", "F_latent_var")
    assert not compare_prediction(got, want, fields=data_fields, bar=BAR, tag="c11 G_test 3-D")
    # a 2-D G_test is one sample of the locations; with X_spatial the warp fields come along
    want1 = oracle_prediction(g, g.S, g.eps_G, G_test={m: g.G_test[m][:1]})
    Yt = {m: torch.randn(nt, g.Y[m].shape[1])}
    want1[m].update({k: v for k, v in oracle_prediction(g, g.S, g.eps_G, G_test={m: g.G_test[m][:1]}, Y=Yt)[m].items()
                     if k.startswith("lpd")})
    got1 = model.predict(X, view_idx, Ns, G_test={m: g.G_test[m][0]}, Y=Yt, latent=True)
    assert not compare_prediction(got1, want1, bar=BAR, tag="c11 G_test 2-D")


def test_value_errors():
    g, model, X, view_idx, Ns = _setup("c5_two_modalities")
    m0 = g.mods[0]
    eps = fresh_eps_G(g, 4)
    with pytest.raises(ValueError, match="X_spatial.*or G_test"):
        model.predict()
    with pytest.raises(ValueError, match="warp must be"):
        model.predict(X, view_idx, Ns, warp="median")
    for S in (0, -1, 2.5):
        with pytest.raises(ValueError, match="S must be"):
            model.predict(X, view_idx, Ns, S=S)
    with pytest.raises(ValueError, match=r"X_spatial\['rna'\] has shape"):
        model.predict({**X, m0: X[m0][:-1]}, view_idx, Ns)
    with pytest.raises(ValueError, match=r"Y\['rna'\] has shape"):
        model.predict(X, view_idx, Ns, Y={**g.Y, m0: g.Y[m0][:, :-1]})
    with pytest.raises(ValueError, match="G_test"):
        model.predict(G_test={m: torch.zeros(5, 3) for m in g.mods})
    with pytest.raises(ValueError, match="eps_G of view 0 has shape"):
        model.predict(X, view_idx, Ns, S=4, eps_G=[eps[0][:, :-1]] + eps[1:])
    with pytest.raises(ValueError, match="eps_G has 1 entries"):
        model.predict(X, view_idx, Ns, S=4, eps_G=eps[:1])
    with pytest.raises(ValueError, match="warp='mean'"):
        model.predict(X, view_idx, Ns, warp="mean", eps_G=eps)


def test_bad_numerics_raise_like_forward():
    g, model, X, view_idx, Ns = _setup("c2_three_free_views")
    with torch.no_grad():
        model.data_kernel_lengthscale.fill_(float("nan"))  # K_uu of the data GP is NaN: its factorisation flags it
    with pytest.raises(torch.linalg.LinAlgError):
        model.predict(X, view_idx, Ns, S=2)
    model.check_numerics = False
    model.predict(X, view_idx, Ns, S=2)  # no check, no raise


def test_predict_leaves_the_model_and_the_rng_alone():
    g, model, X, view_idx, Ns = _setup("c3_lmc_matern12_warp")
    model.train()
    model.inject_noise(g.eps_G, g.eps_F, None)
    noise = model._noise
    model._cache = cache = object()
    model.noise_generators = gens = {"G": torch.Generator().manual_seed(3), "F": torch.Generator().manual_seed(4)}
    gen_states = {k: v.get_state().clone() for k, v in gens.items()}
    state = torch.get_rng_state().clone()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.predict(X, view_idx, Ns, S=4, eps_G=fresh_eps_G(g, 4), Y={m: g.Y[m] for m in g.mods})
    model.predict(X, view_idx, Ns, warp="mean")
    model.predict(X, view_idx, Ns, S=2, generator=torch.Generator().manual_seed(9))  # its own generator only
    assert model.training and model._cache is cache and model._noise is noise
    assert torch.equal(torch.get_rng_state(), state)
    assert all(torch.equal(gens[k].get_state(), gen_states[k]) for k in gens)
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert all(p.grad is None for p in model.parameters())


def test_exports():
    import gpsa
    import spatial_alignment_amd as pkg
    from spatial_alignment_amd.predict import DEFAULT_WORKSPACE_GB, Prediction, rows_for_budget

    assert gpsa.predict is pkg.predict and "predict" in pkg.__all__ and "predict" in gpsa.__all__
    assert DEFAULT_WORKSPACE_GB > 0
    # BASELINE config 5's row count in 2000-row minibatch terms: the budget bounds the chunk, whatever N is
    c = rows_for_budget(0.25, 10, 200, 50, 2)
    assert c % 32 == 0 and 10 * c * (4 * 200 + 8 * 50) <= 0.25 * 2**30
    p = Prediction(F_mean=1)
    assert p.F_mean == 1 and not hasattr(p, "nope")
