"""predict() on the device: the closing kernel gpsa_predict_moments_f32 through the C ABI alone, then the whole call on
every golden fixture, a trained state and the generic tiled paths against values derived from the oracle's fp64
restatement of the reference's forward (tests/predict_util.py).  Bar: the project's output contract, 1e-4 norm-wise
against the reference's fp64 arithmetic; what is measured is printed next to it."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

import spatial_alignment_amd as gp
from golden_io import CASES, Golden, rel
from model_util import build_model
from predict_util import compare_prediction, fresh_eps_G, moments_from_samples, oracle_prediction

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-4
f64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------------
# the kernel's contract, through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def _call(meanT, v, q, var_u, S, W=None, noise_u=None, include_noise=False, Y=None, latent=False):
    """ctypes call on device copies of host tensors -> host results (F_mean, F_var, Fl_mean, Fl_var, lpd), rc"""
    from spatial_alignment_amd import _lib

    lib = _lib.load()
    d = lambda t, dt=torch.float32: None if t is None else t.to(device=DEV, dtype=dt).contiguous()
    p = lambda t: 0 if t is None else t.data_ptr()
    L, SC = meanT.shape
    c = SC // S
    P = L if W is None else W.shape[1]
    mT, vv, qq, vu, Wd, nu, Yd = d(meanT), d(v), d(q, f64), d(var_u), d(W), d(noise_u), d(Y)
    new = lambda *sh, dt=torch.float32: torch.full(sh, float("nan"), dtype=dt, device=DEV)
    Fm, Fv = new(c, P), new(c, P)
    Lm, Lv = (new(c, L), new(c, L)) if latent else (None, None)
    lpd = new(c, dt=f64) if Y is not None else None
    rc = lib.gpsa_predict_moments_f32(p(mT), p(vv), p(qq), p(vu), c, S, L, P, p(Wd), p(nu), int(include_noise), p(Yd),
                                      p(Fm), p(Fv), p(Lm), p(Lv), p(lpd), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu()
    return (host(Fm), host(Fv), host(Lm), host(Lv), host(lpd)), rc


def _expected(meanT, v, q, var_u, S, W, noise_u, include_noise, Y):
    L, SC = meanT.shape
    c = SC // S
    resid = torch.exp(var_u[0].double()) - q.double()
    mu = meanT.double().reshape(L, S, c).permute(1, 2, 0)
    sig2 = (resid.unsqueeze(0) + v.double() + 2e-5).reshape(L, S, c).permute(1, 2, 0)
    tau = None if noise_u is None else torch.exp(noise_u[0].double()) + 1e-5
    return moments_from_samples(mu, sig2, W, tau, include_noise, Y)


def _check(got, want, tag, latent):
    Fm, Fv, Lm, Lv, lpd = got
    pairs = [("F_mean", Fm), ("F_var", Fv)]
    if latent:
        pairs += [("F_latent_mean", Lm), ("F_latent_var", Lv)]
    if lpd is not None:
        pairs.append(("lpd", lpd))  # (relative to its norm over the rows)
    for k, t in pairs:
        assert torch.isfinite(t).all(), (tag, k)
        e = rel(t.double().numpy(), want[k].numpy())
        print(f"[predict kernel] {tag} {k}: {e:.2e} (bar {BAR:.0e})")
        assert e <= BAR, (tag, k, e)


def _inputs(gen, c, S, L, P, lmc, with_y):
    r = lambda *sh: torch.randn(*sh, generator=gen)
    meanT = r(L, S * c)
    v = torch.rand(L, S * c, generator=gen) * 0.5
    q = (torch.rand(S * c, generator=gen, dtype=f64) * 0.5)
    var_u = torch.tensor([math.log(1.3)])
    W = r(L, P) if lmc else None
    noise_u = torch.tensor([math.log(0.3)])
    Y = None
    if with_y:
        Y = 2.0 * r(c, P)
        Y[torch.rand(c, P, generator=gen) < 0.1] = float("nan")
    return meanT, v, q, var_u, W, noise_u, Y


def _kernel_cases():
    cs, Ss, Ls, Ps = (1, 17, 4096 + 5), (1, 3, 10), (1, 10, 50, 64), (1, 50, 500)
    cases = []
    for i, (L, P) in enumerate(itertools.product(Ls, Ps)):          # LMC: every (L, P), c and S cycling through twice
        for shift in (0, 1):
            cases.append((cs[(i + shift) % 3], Ss[(i // 3 + 2 * shift) % 3], L, P, True, (i + shift) % 2 == 0,
                          (i // 2) % 2 == 0))
    for i, L in enumerate(Ls + (500,)):                             # no LMC: P == L (500 outputs: 16 passes)
        for j, c in enumerate(cs):
            cases.append((c, Ss[(i + j) % 3], L, L, False, (i + j) % 2 == 0, j % 2 == 0))
    return cases


@pytest.mark.parametrize("c,S,L,P,lmc,with_y,noise", _kernel_cases())
def test_kernel_contract(c, S, L, P, lmc, with_y, noise):
    gen = torch.Generator().manual_seed(1000 * L + P + c + S)
    meanT, v, q, var_u, W, noise_u, Y = _inputs(gen, c, S, L, P, lmc, with_y)
    latent = (c + S) % 2 == 0
    got, rc = _call(meanT, v, q, var_u, S, W, noise_u, noise, Y, latent)
    assert rc == 0
    want = _expected(meanT, v, q, var_u, S, W, noise_u, noise, Y)
    _check(got, want, f"c={c} S={S} L={L} P={P} lmc={lmc} Y={with_y} noise={noise}", latent)
    if with_y:  # NaN observations contribute 0: a row of NaNs scores exactly 0
        Y2 = Y.clone()
        Y2[0] = float("nan")
        got2, _ = _call(meanT, v, q, var_u, S, W, noise_u, noise, Y2, False)
        assert float(got2[4][0]) == 0.0


def test_kernel_centred_sums_and_far_apart_components():
    """what breaks a naive closing and the fp64 formula handles: samples at 1000 +- 1e-2 (E[m^2] - E[m]^2 in fp32 is
    noise of 6e-2 on a variance of 1e-4) and observations 40 and 100 standard deviations from the two components
    (every density underflows; the log of their mean does not)"""
    gen = torch.Generator().manual_seed(3)
    c, S, L = 50, 10, 8
    meanT = 1000.0 + 1e-2 * torch.randn(L, S * c, generator=gen)
    v = torch.full((L, S * c), 1e-6)
    q = torch.full((S * c,), 1.0 - 1e-5, dtype=f64)
    var_u, noise_u = torch.tensor([0.0]), torch.tensor([math.log(1e-3)])
    got, rc = _call(meanT, v, q, var_u, S, None, noise_u, False, None, True)
    assert rc == 0
    want = _expected(meanT, v, q, var_u, S, None, noise_u, False, None)
    assert float(want["F_var"].mean()) < 2e-4  # the between-sample term is what is measured
    _check(got, want, "centred", True)

    S, sd = 2, 0.5
    meanT = torch.tensor([0.0, 60 * sd]).repeat_interleave(c).reshape(1, S * c).repeat(L, 1)  # column s*c + r
    v = torch.full((L, S * c), sd * sd - 2e-5 - 1e-6)
    q = torch.full((S * c,), 1.0, dtype=f64)
    Y = torch.full((c, L), 100 * sd)
    got, rc = _call(meanT, v, q, var_u, S, None, noise_u, False, Y, False)
    assert rc == 0
    want = _expected(meanT, v, q, var_u, S, None, noise_u, False, Y)
    assert torch.isfinite(want["lpd"]).all() and float(want["lpd"].max()) < -700 * L
    _check(got, want, "far apart", False)


def test_kernel_refuses_what_it_cannot_take():
    gen = torch.Generator().manual_seed(5)
    meanT, v, q, var_u, W, noise_u, Y = _inputs(gen, 9, 2, 4, 6, True, True)
    EINVAL, EUNSUPPORTED = -1, -3
    assert _call(meanT, v, q, var_u, 2, None, noise_u, False, None)[1] == 0
    assert _call(meanT, v, q, var_u, 2, W, None, True, None)[1] == EINVAL          # noise asked for, none given
    assert _call(meanT, v, q, var_u, 2, W, None, False, Y)[1] == EINVAL            # observations need the noise
    W65 = torch.randn(65, 6, generator=gen)
    big = torch.randn(65, 18, generator=gen)
    assert _call(big, big.abs(), q, var_u, 2, W65, noise_u, False, None)[1] == EUNSUPPORTED
    from spatial_alignment_amd import _lib

    lib = _lib.load()
    z = torch.zeros(64, device=DEV)
    zd = torch.zeros(64, device=DEV, dtype=f64)
    st = torch.cuda.current_stream().cuda_stream
    for c_, S_, L_, P_ in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 2, 3)):  # (2, 3: no W, P != L)
        rc = lib.gpsa_predict_moments_f32(z.data_ptr(), z.data_ptr(), zd.data_ptr(), z.data_ptr(), c_, S_, L_, P_, 0, 0, 0,
                                          0, z.data_ptr(), z.data_ptr(), 0, 0, 0, st)
        assert rc == EINVAL, (c_, S_, L_, P_, rc)
    torch.cuda.synchronize()


def test_new_kernels_have_no_scratch_and_no_spills():
    """register allocation of the closing kernels, read from the code objects inside the built library"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from kernel_meta import demangle, library_kernels

    from spatial_alignment_amd import _lib

    ks = library_kernels(_lib.LIB_PATH)
    mine = [(n, k) for n, k in zip(demangle([k["name"] for k in ks]), ks) if "predict_moments_kernel<" in n]
    assert len(mine) == 2, [n for n, _ in mine]
    for n, k in mine:
        assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)


# ------------------------------------------------------------------------------------------------------------------------
# the whole call
# ------------------------------------------------------------------------------------------------------------------------
def _setup(name):
    g = Golden(name)
    model, dd = build_model(g, device=DEV)
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    return g, model, X, view_idx, Ns


def _same(a, b):
    return all((a[m][k] is None and b[m][k] is None) or torch.equal(a[m][k].nan_to_num(12345.0), b[m][k].nan_to_num(12345.0))
               for m in a for k in a[m])


@pytest.mark.parametrize("name", CASES)
def test_goldens_match_the_oracle(name):
    g, model, X, view_idx, Ns = _setup(name)
    S = 4
    eps = fresh_eps_G(g, S)
    Y = {m: g.Y[m].clone() for m in g.mods}
    for m in g.mods:
        Y[m][2::9, -1] = float("nan")
    want = oracle_prediction(g, S, eps, Y=Y)
    kw = dict(S=S, eps_G=eps, Y=Y, latent=True)
    whole = model.predict(X, view_idx, Ns, **kw)
    assert not compare_prediction(whole, want, bar=BAR, tag=f"{name} S=4")
    chunked = model.predict(X, view_idx, Ns, rows_per_chunk=61, **kw)
    assert not compare_prediction(chunked, want, bar=BAR, tag=f"{name} S=4 chunks of 61")
    # a column's arithmetic does not depend on its neighbours: the chunked call is the unchunked one, bit for bit
    assert _same(whole, chunked), {f"{m}/{k}": float((whole[m][k].double() - chunked[m][k].double()).abs().max())
                                   for m in whole for k in whole[m] if whole[m][k] is not None}
    want = oracle_prediction(g, 1, None, Y=Y, include_noise=True)
    got = model.predict(X, view_idx, Ns, warp="mean", Y=Y, include_noise=True, latent=True)
    assert not compare_prediction(got, want, bar=BAR, tag=f"{name} warp=mean")
    assert _same(got, model.predict(X, view_idx, Ns, warp="mean", Y=Y, include_noise=True, latent=True,
                                    rows_per_chunk=61))
    if g.G_test is not None:
        want = oracle_prediction(g, g.S, g.eps_G, G_test=g.G_test)
        got = model.predict(G_test={m: t.to(DEV) for m, t in g.G_test.items()}, latent=True)
        fields = ("F_mean", "F_var", "F_latent_mean", "F_latent_var")
        assert not compare_prediction(got, want, fields=fields, bar=BAR, tag=f"{name} G_test")


class _Problem:
    """what predict_util needs of a fixture, for problems built here"""

    def __init__(self, dd, model, cfg):
        self.mods = list(dd)
        self.X = {m: dd[m]["spatial_coords"].cpu() for m in dd}
        self.Y = {m: dd[m]["outputs"].cpu() for m in dd}
        self.cfg = dict(n_samples={m: dd[m]["n_samples_list"] for m in dd}, n_latent_gps=cfg["n_latent_gps"])
        self._cfg = cfg
        D = model.n_spatial_dims
        self.eps_G = [torch.zeros(1, sum(dd[m]["n_samples_list"][v] for m in dd), D) for v in range(model.n_views)
                      if not model._is_fixed(v)]

    def oracle_cfg(self):
        return self._cfg

    @staticmethod
    def state_of(model):
        st = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        for name in ("mean_slopes", "mean_intercepts"):
            st.setdefault(name, getattr(model, name).detach().cpu().clone())
        return st


def _grid_model(M, mG, seed=5):
    from spatial_alignment_amd.synthetic import make_grid_problem

    dd = make_grid_problem(side=20, n_views=2, n_outputs=6, device="cpu")
    m = "expression"
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = gp.VariationalGPSA(dd, m_X_per_view=M, m_G=mG, data_init=False, n_latent_gps={m: None},
                               kernel_func_warp=gp.rbf_kernel, kernel_func_data=gp.rbf_kernel, fixed_view_idx=None)
    model = model.to(DEV)
    ddd = {m: {"spatial_coords": dd[m]["spatial_coords"].to(DEV), "outputs": dd[m]["outputs"].to(DEV),
               "n_samples_list": dd[m]["n_samples_list"]}}
    cfg = dict(modality_names=[m], n_views=2, n_spatial_dims=2, kernel_warp="rbf", kernel_data="rbf",
               n_latent_gps={m: None}, fixed_view_idx=None)
    return model, ddd, _Problem(dd, model, cfg)


def test_trained_state_matches_the_oracle():
    """after training the posterior variance is small and the between-sample term matters: same bar on every field"""
    from spatial_alignment_amd import train

    model, ddd, prob = _grid_model(64, 64)
    torch.manual_seed(11)
    trace = train.fit(model, ddd, 300, lr=1e-2, S=3)
    assert trace[-1] < trace[0]
    S = 8
    eps = fresh_eps_G(prob, S, seed=2)
    Y = prob.Y
    want = oracle_prediction(prob, S, eps, state=prob.state_of(model), Y=Y, include_noise=True)
    got = model.predict({m: ddd[m]["spatial_coords"] for m in ddd}, S=S, eps_G=eps, Y=Y, include_noise=True, latent=True)
    m = prob.mods[0]
    print("[predict trained] F_var mean %.3e, min %.3e; loss %.1f -> %.1f" % (
        float(want[m]["F_latent_var"].mean()), float(want[m]["F_latent_var"].min()), trace[0], trace[-1]))
    assert not compare_prediction(got, want, bar=BAR, tag="trained M=64")


@pytest.mark.parametrize("M,mG", [(288, 288), (300, 96)])
def test_generic_tiled_paths_match_the_oracle(M, mG):
    model, ddd, prob = _grid_model(M, mG)
    S = 2
    eps = fresh_eps_G(prob, S, seed=9)
    want = oracle_prediction(prob, S, eps, state=prob.state_of(model), Y=prob.Y)
    got = model.predict({m: ddd[m]["spatial_coords"] for m in ddd}, S=S, eps_G=eps, Y=prob.Y, latent=True)
    assert not compare_prediction(got, want, bar=BAR, tag=f"M={M} m_G={mG}")


@pytest.mark.parametrize("name", ["c2_three_free_views", "c3_lmc_matern12_warp", "c5_two_modalities"])
def test_agrees_with_the_average_of_noise_free_forward_draws(name):
    """the route users have: forward(prediction_mode=True) with the same warp draws and eps_F = 0 gives mu_s; its mean
    over S in fp64 is F_latent_mean, and through W, F_mean"""
    g, model, X, view_idx, Ns = _setup(name)
    S = 4
    eps = fresh_eps_G(g, S)
    got = model.predict(X, view_idx, Ns, S=S, eps_G=eps, latent=True)
    model2, dd2 = build_model(g, device=DEV)
    model2.inject_noise(eps, {m: torch.zeros(S, int(Ns[m]), model2.n_latent_outputs[m]) for m in g.mods}, None)
    with torch.no_grad():
        out = model2.forward(X, view_idx=view_idx, Ns=Ns, S=S, prediction_mode=True)
    for m in g.mods:
        for k, t in (("G_mean", out[0][m].double()), ("F_latent_mean", out[2][m].double().mean(0)),
                     ("F_mean", out[3][m].double().mean(0))):
            e = rel(got[m][k].double().cpu().numpy(), t.cpu().numpy())
            print(f"[predict vs forward] {name} {m}/{k}: {e:.2e} (bar {BAR:.0e})")
            assert e <= BAR, (m, k, e)


def test_training_is_bit_identical_with_predict_in_the_loop():
    from spatial_alignment_amd import train

    runs = []
    for with_predict in (False, True):
        g = Golden("c5_two_modalities")
        model, dd = build_model(g, device=DEV)
        X = {m: dd[m]["spatial_coords"] for m in g.mods}
        Y = {m: dd[m]["outputs"] for m in g.mods}
        gen = torch.Generator(device=DEV).manual_seed(77)
        calls = []

        def cb(step, mdl, trace):
            if with_predict:
                calls.append(mdl.predict(X, S=3, generator=gen, Y=Y, latent=True))
                mdl.predict(X, warp="mean")

        torch.manual_seed(21)
        trace = train.fit(model, dd, 20, lr=1e-2, S=3, sync_every=5, callback=cb)
        assert len(calls) == (4 if with_predict else 0) and model.training
        runs.append((trace, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_peak_memory_is_bounded_by_the_chunk():
    """N = 2 x 20 000, L = 50, M = 200, S = 10 in chunks of 2000 rows: the call's peak over the resident model and data
    stays below the 400 MB the issue sets (by shapes: the chunk's panels, the M x M stage and the results, expected well
    under 150 MB) - independent of N, where the draw-and-average route holds two [S, N, L] tensors.
    Measured on an MI355X: 97.5 MiB (16 MiB of it the fp64 variational covariances, 16 MiB the results, the rest the
    chunk's panels and the kernels' scratch buffer).  The issue calls its 400 MB "the size of ONE [S, N, L] fp32
    tensor"; at THESE shapes one such tensor is 76 MiB, which the call does not stay under - it does from about
    N = 2 x 27 000 rows up, since its peak does not grow with N beyond the results (8 N L bytes)."""
    n, Lp, M, S = 20000, 50, 200, 10
    gen = torch.Generator().manual_seed(0)
    m = "expression"
    dd = {m: {"spatial_coords": torch.rand(2 * n, 2, generator=gen) * 10, "outputs": torch.randn(2 * n, Lp, generator=gen),
              "n_samples_list": [n, n]}}
    torch.manual_seed(0)
    np.random.seed(0)
    model = gp.VariationalGPSA(dd, m_X_per_view=M, m_G=M, data_init=False, n_latent_gps={m: None}, fixed_view_idx=None)
    with torch.no_grad():  # inducing points inside the data's box (well-conditioned covariances)
        model.Xtilde.copy_(torch.rand(model.Xtilde.shape, generator=gen) * 10)
        model.delta_G_list.copy_(model.Xtilde)
        model.Gtilde.copy_(torch.rand(model.Gtilde.shape, generator=gen) * 10)
    model = model.to(DEV)
    X = {m: dd[m]["spatial_coords"].to(DEV)}
    Y = {m: dd[m]["outputs"].to(DEV)}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = model.predict(X, S=S, Y=Y, rows_per_chunk=2000, generator=torch.Generator(device=DEV).manual_seed(1))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    one = S * 2 * n * Lp * 4
    print(f"[predict memory] peak rise {rise / 2**20:.1f} MiB (bound 400 MB); one [S, N, L] fp32 tensor at these shapes "
          f"{one / 2**20:.1f} MiB")
    assert torch.isfinite(out[m].F_mean).all() and torch.isfinite(out[m].lpd).all()
    assert rise < 400e6, rise
