"""predict(scale="response") on the device: the closing kernel gpsa_predict_counts_f32 through the C ABI alone at the
smallest shapes that can still break it, then the whole call on the golden fixtures.

References (tests/predict_counts_util.py): fp64 numpy / torch on the CPU - the lognormal closed forms for Y_mean / Y_var
and a dense trapezoid integral for the Poisson-lognormal log density - fed with the kernel's own fp32 inputs, or with the
oracle's per-sample moments for whole calls; never the node rule, never the code under test.  Every case first asserts
on the REFERENCE's inputs that it lies where the rule is measured: max u <= 4, max (mu + 3 sqrt(u)) <= 20.

Bars: the whole call is held to the project's hard 1e-4, norm-wise.  The kernel's measured worst values are far below
it, so its bars are 3x the measurement (KERNEL_BARS; never above 1e-4), with a floor of 1e-11 under the lpd bars: the
reference integral itself is good to 2e-12 and a term y eta of 2000 carries 2e-13 of fp64 rounding.  Measured on an
MI355X (printed next to the bar on every run), Y_mean / Y_var entry-wise relative, lpd as |error| / max(1, |ref|) per
entry where P = 1 and norm-wise over rows otherwise:

    case               c     S  L   P   Y_mean    Y_var     lpd
    one                1     1  1   1   4.47e-08  2.62e-08  5.96e-15
    tails_two_passes   33    3  33  33  5.78e-08  5.86e-08  2.41e-08
    tails_no_offsets   33    3  33  33  5.62e-08  5.78e-08  2.42e-08
    lmc                31    2  3   33  6.43e-08  1.41e-07  5.52e-09
    lmc_no_y           31    2  3   33  6.43e-08  1.41e-07  -
    lmc_at_the_limit   64    1  64  1   5.57e-08  5.27e-08  6.38e-09
    many_workgroups    4101  2  2   2   5.88e-08  5.88e-08  3.76e-08
    far apart          50    2  8   8   7.82e-09  1.75e-08  1.05e-15
    nearly equal rates 40    10 4   4   2.52e-08  2.61e-08  -
    ... mixed, W = 1e-3 40   10 1   1   2.80e-08  2.84e-08  -

Y_mean / Y_var sit at the rounding of an fp64 value to fp32 (2^-24 = 6e-8; an LMC entry's u carries a little more).
Whole calls against the oracle (S = 3, seed 1), worst field over c1, c2, c10, c5 / rna, c3, c11 with own rows,
warp="mean" and G_test: Y_mean 1.5e-7, Y_var 4.0e-7, lpd 2.7e-7, lpd_sum 2.4e-7.
"""
import functools
import math
import os
import sys

import pytest
import torch

from golden_io import Golden, rel
from model_util import build_model
from predict_counts_util import (counts_and_offsets, counts_from_samples, lpd_err, oracle_counts, relmax)
from predict_util import fresh_eps_G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-4
f64 = torch.float64
EINVAL, EUNSUPPORTED = -1, -3

# (c, S, L, P, lmc, offsets, with_y) -> bars of (Y_mean, Y_var, lpd): 3x the measured worst value, never above BAR
KERNEL_CASES = {
    "one": (1, 1, 1, 1, False, True, True),
    "tails_two_passes": (33, 3, 33, 33, False, True, True),      # row-tile tail, output-pass tail, two passes
    "tails_no_offsets": (33, 3, 33, 33, False, False, True),
    "lmc": (31, 2, 3, 33, True, True, True),
    "lmc_no_y": (31, 2, 3, 33, True, True, False),
    "lmc_at_the_limit": (64, 1, 64, 1, True, True, True),
    "many_workgroups": (4101, 2, 2, 2, False, True, True),
}
KERNEL_BARS = {
    "one": (1.4e-7, 7.9e-8, 1e-11),
    "tails_two_passes": (1.8e-7, 1.8e-7, 7.3e-8),
    "tails_no_offsets": (1.7e-7, 1.8e-7, 7.3e-8),
    "lmc": (2.0e-7, 4.3e-7, 1.7e-8),
    "lmc_no_y": (2.0e-7, 4.3e-7),
    "lmc_at_the_limit": (1.7e-7, 1.6e-7, 2.0e-8),
    "many_workgroups": (1.8e-7, 1.8e-7, 1.2e-7),
}
FAR_APART_BARS = (2.4e-8, 5.3e-8, 1e-11)


# ------------------------------------------------------------------------------------------------------------------------
# the kernel's contract, through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def _call(meanT, v, q, var_u, S, W=None, off=None, Y=None):
    """ctypes call on device copies of host tensors -> host results (Y_mean, Y_var, lpd), rc"""
    from spatial_alignment_amd import _lib

    lib = _lib.load()
    d = lambda t, dt=torch.float32: None if t is None else t.to(device=DEV, dtype=dt).contiguous()
    p = lambda t: 0 if t is None else t.data_ptr()
    L, SC = meanT.shape
    c = SC // S
    P = L if W is None else W.shape[1]
    mT, vv, qq, vu, Wd, od, Yd = d(meanT), d(v), d(q, f64), d(var_u), d(W), d(off), d(Y)
    new = lambda *sh, dt=torch.float32: torch.full(sh, float("nan"), dtype=dt, device=DEV)
    Ym, Yv = new(c, P), new(c, P)
    lpd = new(c, dt=f64) if Y is not None else None
    rc = lib.gpsa_predict_counts_f32(p(mT), p(vv), p(qq), p(vu), c, S, L, P, p(Wd), p(od), p(Yd), p(Ym), p(Yv), p(lpd),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (Ym.cpu(), Yv.cpu(), None if lpd is None else lpd.cpu()), rc


def _expected(meanT, v, q, var_u, S, W, off, Y):
    L, SC = meanT.shape
    c = SC // S
    resid = torch.exp(var_u[0].double()) - q.double()
    mu = meanT.double().reshape(L, S, c).permute(1, 2, 0)
    sig2 = (resid.unsqueeze(0) + v.double() + 2e-5).reshape(L, S, c).permute(1, 2, 0)
    want = counts_from_samples(mu, sig2, W, off, Y)
    # a condition on the reference's inputs, not a measurement: the case lies where the rule is measured
    assert want["max_u"] <= 4.0 and want["max_eta"] <= 20.0, (want["max_u"], want["max_eta"])
    return want


@functools.lru_cache(maxsize=None)
def _case(name):
    """host inputs of a kernel case and their reference, computed once: log-rate means about 1 + 1.5 randn, u from the
    exact jitter floor 2e-5 (v = 0, q = exp(var_u) = 1 in the first column) up to about 2, offsets 0.25 sin n,
    y = floor(exp(1.5 randn)) with 10 % NaN and planted y = 0 and y = 300"""
    c, S, L, P, lmc, offsets, with_y = KERNEL_CASES[name]
    gen = torch.Generator().manual_seed(20251018 + 1000 * L + 10 * P + c + S)
    meanT = 1.0 + 1.5 * torch.randn(L, S * c, generator=gen)
    v = torch.rand(L, S * c, generator=gen)
    q = torch.rand(S * c, generator=gen, dtype=f64)
    v[:, 0], q[0] = 0.0, 1.0
    var_u = torch.tensor([0.0])
    W = torch.randn(L, P, generator=gen) * (0.6 / math.sqrt(L)) if lmc else None
    off = 0.25 * torch.sin(torch.arange(c, dtype=torch.float32)) if offsets else None
    Y = None
    if with_y:
        Y = torch.floor(torch.exp(1.5 * torch.randn(c, P, generator=gen)))
        Y[torch.rand(c, P, generator=gen) < 0.1] = float("nan")
        if c * P >= 4:
            Y.view(-1)[1], Y.view(-1)[c * P // 2] = 0.0, 300.0
            Y[0, 0] = 300.0  # a large count where u sits on the jitter floor
        else:
            Y[0, 0] = 2.0
    return (meanT, v, q, var_u, S, W, off, Y), _expected(meanT, v, q, var_u, S, W, off, Y)


def _check(got, want, tag, bars, single_output):
    Ym, Yv, lpd = got
    errs = {"Y_mean": relmax(Ym, want["Y_mean"]), "Y_var": relmax(Yv, want["Y_var"])}
    assert torch.isfinite(Ym).all() and torch.isfinite(Yv).all(), tag
    if lpd is not None:
        assert torch.isfinite(lpd).all(), tag
        # entry-wise on a single output; over rows the sum of P entries is held norm-wise
        errs["lpd"] = lpd_err(lpd, want["lpd"]) if single_output else rel(lpd.numpy(), want["lpd"].numpy())
    for (k, e), bar in zip(errs.items(), bars):
        print(f"[counts kernel] {tag} {k}: {e:.2e} (bar {bar:.1e}; max u {want['max_u']:.2f}, max eta {want['max_eta']:.1f})")
    for (k, e), bar in zip(errs.items(), bars):
        assert e <= bar <= BAR, (tag, k, e, bar)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_contract(name):
    args, want = _case(name)
    got, rc = _call(*args)
    assert rc == 0
    _check(got, want, name, KERNEL_BARS[name], single_output=KERNEL_CASES[name][3] == 1)


def test_missing_entries_and_the_launch_without_observations():
    """a row of NaNs scores exactly 0, and the moments do not depend on whether Y was given: bit for bit"""
    for name in ("tails_two_passes", "lmc"):
        (meanT, v, q, var_u, S, W, off, Y), _ = _case(name)
        Y2 = Y.clone()
        Y2[0] = float("nan")
        with_y, rc = _call(meanT, v, q, var_u, S, W, off, Y2)
        assert rc == 0 and float(with_y[2][0]) == 0.0 and torch.isfinite(with_y[2]).all()
        without, rc = _call(meanT, v, q, var_u, S, W, off, None)
        assert rc == 0 and without[2] is None
        assert torch.equal(with_y[0], without[0]) and torch.equal(with_y[1], without[1])


def test_far_apart_components():
    """S = 2 components 60 standard deviations apart (log rates -4 and 2, sd 0.1) and y = 1000: each component's density
    underflows in fp64 (log densities -5106 and -1082, below log(DBL_MIN) = -745), the log of their mean does not"""
    c, S, L, sd = 50, 2, 8, 0.1
    meanT = torch.tensor([-4.0, -4.0 + 60 * sd]).repeat_interleave(c).reshape(1, S * c).repeat(L, 1)  # column s*c + r
    v = torch.full((L, S * c), sd * sd - 2e-5)
    q = torch.full((S * c,), 1.0, dtype=f64)
    var_u = torch.tensor([0.0])
    Y = torch.full((c, L), 1000.0)
    want = _expected(meanT, v, q, var_u, S, None, None, Y)
    assert torch.isfinite(want["lpd"]).all() and float(want["lpd"].max()) < -745 * L
    got, rc = _call(meanT, v, q, var_u, S, None, None, Y)
    assert rc == 0
    _check(got, want, "far apart", FAR_APART_BARS, single_output=False)
    e = lpd_err(got[2] / L, want["lpd"] / L)  # (every output of a row is the same entry: the row sum / L is one entry)
    print(f"[counts kernel] far apart, per entry: {e:.2e}")
    assert e <= FAR_APART_BARS[2]


def test_between_sample_term_of_nearly_equal_rates():
    """samples at 1000 (1 +- 1e-5) in the rate, u on the jitter floor: Y_var = Y_mean + lam^2 expm1(u) + var_s(lam) is
    1000 + 20 + 1e-4.  The between-sample term is formed from sums centred on the first sample in fp64; E[lam^2] - E[lam]^2
    of raw values would carry 1e6 * 2^-53 * S in fp64 and 6e-2 in fp32.  (Next to 1020 the term itself is below the
    fp32 resolution of the result, 6e-5: what the output can show is that nothing of that size went wrong; the next test
    puts the term where fp32 resolves it.)"""
    c, S, L = 40, 10, 4
    gen = torch.Generator().manual_seed(7)
    sign = torch.where(torch.rand(L, S * c, generator=gen) < 0.5, -1.0, 1.0).double()
    meanT = torch.log(1000.0 * (1.0 + 1e-5 * sign)).float()
    v = torch.zeros(L, S * c)
    q = torch.full((S * c,), 1.0, dtype=f64)
    var_u = torch.tensor([0.0])
    want = _expected(meanT, v, q, var_u, S, None, None, None)
    got, rc = _call(meanT, v, q, var_u, S, None, None, None)
    assert rc == 0
    _check(got, want, "nearly equal rates", (BAR, BAR), single_output=False)
    assert relmax(got[1], want["Y_var"]) <= 3 * 2.0**-24  # fp64 arithmetic, one rounding to fp32 (and slack for exp)


def test_between_sample_term_where_the_output_resolves_it():
    """the same near-equal samples where fp32 can show the term: one latent output mixed with W = 1e-3 puts u at
    2e-5 * 1e-6 = 2e-11, far below the jitter floor of an unmixed output, and rates of 1e6 (1 +- 1e-5) (eta = 13.8) give
    Y_var = 1e6 + 20 + 100: the between-sample term is 1e-4 of the result, 1600 fp32 steps.  Leaving it out, or forming
    it as E[lam^2] - E[lam]^2 in fp32 (noise of 1e12 * 6e-8), misses the bar by orders of magnitude; the same raw form in
    fp64 (1e12 * 2^-53 * S = 1e-3 next to 1e6) would not show in an fp32 result at any rate - that form is excluded by
    the kernel's source, not by a measurement.  Bar: fp64 arithmetic and one rounding to fp32, 3 * 2^-24."""
    c, S, w = 40, 10, 1e-3
    gen = torch.Generator().manual_seed(8)
    sign = torch.where(torch.rand(1, S * c, generator=gen) < 0.5, -1.0, 1.0).double()
    meanT = (torch.log(1e6 * (1.0 + 1e-5 * sign)) / w).float()
    v = torch.zeros(1, S * c)
    q = torch.full((S * c,), 1.0, dtype=f64)
    var_u = torch.tensor([0.0])
    W = torch.tensor([[w]])
    want = _expected(meanT, v, q, var_u, S, W, None, None)
    mu = meanT.double().reshape(S, c) * float(W[0, 0])  # the reference's own between-sample term and its share
    between = torch.exp(mu).var(0, unbiased=False)
    assert float((between / want["Y_var"][:, 0]).min()) >= 2e-5  # a condition on the reference: the term is visible
    got, rc = _call(meanT, v, q, var_u, S, W, None, None)
    assert rc == 0
    _check(got, want, "nearly equal rates, mixed", (3 * 2.0**-24, 3 * 2.0**-24), single_output=True)


def test_kernel_refuses_what_it_cannot_take():
    (meanT, v, q, var_u, S, W, off, Y), _ = _case("lmc")
    assert _call(meanT, v, q, var_u, S, None, off, None)[1] == 0            # no W: P == L
    gen = torch.Generator().manual_seed(5)
    W65, big = torch.randn(65, 6, generator=gen) * 0.1, torch.randn(65, S * 31, generator=gen)
    assert _call(big, big.abs(), q, var_u, S, W65, off, None)[1] == EUNSUPPORTED
    from spatial_alignment_amd import _lib

    lib = _lib.load()
    z = torch.zeros(64, device=DEV)
    zd = torch.zeros(64, device=DEV, dtype=f64)
    st = torch.cuda.current_stream().cuda_stream
    zp, dp = z.data_ptr(), zd.data_ptr()
    ok = dict(meanT=zp, v=zp, q=dp, var_u=zp, c=1, S=1, L=1, P=1, W=0, log_offset=0, Y=0, Y_mean=zp, Y_var=zp, lpd=0)
    call = lambda **kw: lib.gpsa_predict_counts_f32(*{**ok, **kw}.values(), st)
    assert call() == 0
    for bad in (dict(c=0), dict(S=0), dict(L=0), dict(P=0), dict(L=2, P=3),    # (2, 3: no W, P != L)
                dict(meanT=0), dict(v=0), dict(q=0), dict(var_u=0), dict(Y_mean=0), dict(Y_var=0),
                dict(Y=zp), dict(lpd=dp)):                                     # lpd is given exactly when Y is
        assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()


def test_new_kernels_have_no_scratch_and_no_spills():
    """register allocation of the counts kernels, read from the code objects inside the built library"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from kernel_meta import demangle, library_kernels

    from spatial_alignment_amd import _lib

    ks = library_kernels(_lib.LIB_PATH)
    mine = [(n, k) for n, k in zip(demangle([k["name"] for k in ks]), ks) if "predict_counts_kernel<" in n]
    assert len(mine) == 4, [n for n, _ in mine]  # LMC or not, with Y or without
    for n, k in mine:
        assert "predict_moments_kernel<" not in n
        assert k["max_wg"] == 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)


# ------------------------------------------------------------------------------------------------------------------------
# the whole call
# ------------------------------------------------------------------------------------------------------------------------
# fixture -> its Poisson modalities (c7 is left out: its log rates reach +-249; c5's Gaussian protein reaches u = 7.6
# and does not use the rule)
WHOLE = {"c1_example_fixed0": None, "c2_three_free_views": None, "c10_unequal_two_fixed": None,
         "c5_two_modalities": ["rna"], "c3_lmc_matern12_warp": None, "c11_lmc_gtest_unequal": None}


def _setup(name):
    g = Golden(name)
    pois = WHOLE[name] or list(g.mods)
    model, dd = build_model(g, device=DEV)
    model.likelihood = "poisson" if len(pois) == len(g.mods) else {m: "poisson" for m in pois}
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    return g, pois, model, X, view_idx, Ns


def _compare(got, want, tag):
    bad = {}
    for m, w in want.items():
        assert w["max_u"] <= 4.0, (tag, m, w["max_u"])  # the domain condition, on the oracle's values
        for k in ("Y_mean", "Y_var", "lpd", "lpd_sum"):
            if k in w:
                e = rel(got[m][k].detach().cpu().double().numpy(), w[k].numpy())
                print(f"[predict counts] {tag} {m}/{k}: {e:.2e} (bar {BAR:.0e}; max u {w['max_u']:.2f})")
                if not e <= BAR:
                    bad[f"{m}/{k}"] = e
    return bad


def _same(a, b):
    return all((a[m][k] is None and b[m][k] is None) or torch.equal(a[m][k].nan_to_num(12345.0), b[m][k].nan_to_num(12345.0))
               for m in a for k in a[m])


@pytest.mark.parametrize("name", list(WHOLE))
def test_goldens_match_the_oracle(name):
    g, pois, model, X, view_idx, Ns = _setup(name)
    S = 3
    eps = fresh_eps_G(g, S)  # three fresh warp draws, seed 1
    Y, off = counts_and_offsets(g, pois)
    for m in pois:
        Y[m][2::9, -1] = float("nan")
    offd = {m: t.to(DEV) for m, t in off.items()}
    gens = model.noise_generators if hasattr(model, "noise_generators") else None
    before = {k: v.clone() for k, v in model.state_dict().items()}
    rng = torch.cuda.get_rng_state(0).clone()
    kw = dict(S=S, eps_G=eps, Y=Y, scale="response", log_offset=offd)
    whole = model.predict(X, view_idx, Ns, **kw)
    assert not _compare(whole, oracle_counts(g, S, eps, pois, Y=Y, offset=off), f"{name} S=3")
    for m in pois:
        assert torch.equal(whole[m].lpd_sum, whole[m].lpd.sum())
    # a row's value does not depend on its chunk: bit for bit
    chunked = model.predict(X, view_idx, Ns, rows_per_chunk=32, **kw)
    assert _same(whole, chunked), {f"{m}/{k}": float((whole[m][k].double() - chunked[m][k].double()).abs().max())
                                   for m in whole for k in whole[m] if whole[m][k] is not None}
    # the log-rate fields stay what the default call returns
    link = model.predict(X, view_idx, Ns, S=S, eps_G=eps)
    for m in g.mods:
        assert "Y_mean" not in link[m]
        for k in ("G_mean", "G_scale", "F_mean", "F_var"):
            assert torch.equal(link[m][k], whole[m][k]), (m, k)
    got = model.predict(X, view_idx, Ns, warp="mean", Y=Y, scale="response", log_offset=offd)
    assert not _compare(got, oracle_counts(g, 1, None, pois, Y=Y, offset=off), f"{name} warp=mean")
    if g.G_test is not None:
        m = g.mods[0]
        nt = g.G_test[m].shape[1]
        Yt, offt = {m: Y[m][:nt]}, {m: off[m][:nt]}
        want = oracle_counts(g, g.S, g.eps_G, pois, Y=Yt, offset=offt, G_test=g.G_test)
        got = model.predict(G_test={k: t.to(DEV) for k, t in g.G_test.items()}, Y=Yt, scale="response",
                            log_offset={m: offt[m].to(DEV)})
        assert not _compare(got, want, f"{name} G_test")
    if len(pois) < len(g.mods):  # the Gaussian modality is the link call's, bit for bit
        model.likelihood = "gaussian"
        ref = model.predict(X, view_idx, Ns, S=S, eps_G=eps, Y={m: (g.Y[m] if m in pois else Y[m]) for m in g.mods},
                            include_noise=True)
        model.likelihood = {m: "poisson" for m in pois}
        for m in g.mods:
            if m not in pois:
                assert torch.equal(whole[m].Y_mean, ref[m].F_mean) and torch.equal(whole[m].lpd, ref[m].lpd)
                assert rel(whole[m].Y_var.cpu().double().numpy(), ref[m].F_var.cpu().double().numpy()) <= 1e-6
    # the model's state and the generators are untouched
    assert torch.equal(torch.cuda.get_rng_state(0), rng)
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert gens is None or model.noise_generators is gens
    assert all(p.grad is None for p in model.parameters())


def test_dispatcher_op_and_its_fake():
    (meanT, v, q, var_u, S, W, off, Y), want = _case("lmc")
    d = lambda t, dt=torch.float32: t.to(device=DEV, dtype=dt)
    Ym, Yv, lpd = torch.ops.gpsa.predict_counts(d(meanT), d(v), d(q, f64), d(var_u), S, d(W), d(off), d(Y))
    direct, _ = _call(meanT, v, q, var_u, S, W, off, Y)
    assert torch.equal(Ym.cpu(), direct[0]) and torch.equal(Yv.cpu(), direct[1]) and torch.equal(lpd.cpu(), direct[2])
    assert torch.ops.gpsa.predict_counts(d(meanT), d(v), d(q, f64), d(var_u), S, d(W))[2].numel() == 0
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        L, SC = meanT.shape
        f = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device="cuda")
        a, b, c_ = torch.ops.gpsa.predict_counts(f(L, SC), f(L, SC), f(SC, dt=f64), f(1), S, f(L, 33), None, f(31, 33))
        assert tuple(a.shape) == tuple(b.shape) == (31, 33) and tuple(c_.shape) == (31,) and c_.dtype == f64
