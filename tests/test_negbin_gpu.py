"""Count outputs (model.likelihood = "negative_binomial") on the device.  For such a modality the draws are log means,
    a[s,n,p] = F_obs[s,n,p] + o[n] - rho_p,  r_p = exp(rho_p),
    LL = sum (y a - (y + r) softplus(a)) / S + sum (lgamma(y + r) - lgamma(r) - lgamma(y + 1)),
with rho a trainable vector per modality.  The kernels (gpsa_nb_const, gpsa_elbo_loss_nb_fwd / _bwd,
gpsa_quadform_elbo_nb_f32 / _delta_nb_f32, gpsa_lmc_loglik_fused_nb_f32) against fp64 torch with autograd, written here, at the bars the Poisson counterparts carry (tests/test_poisson_gpu.py); a sum of terms is
measured against the sum of the MAGNITUDES of the terms that enter it (the net sum cancels): |y a| + (y + r) softplus(a)
for t, r softplus(a) + (y + r) sigma(a) + y for u.  Whole steps against the fp64 oracle: orc.forward_pass, then
negative_elbo with its Gaussian log density taken back out for the NB modality and the NB log density put in, rho included
in autograd; every output, the loss and every gradient, log_dispersion's included, at the project's hard 1e-4.
c7_m200_conditioning, whose draws reach |F| = 136 and which the Poisson steps leave out, is covered: the softplus form has
no exp(eta)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import test_missing_gpu as TM
import test_poisson_gpu as TP
from golden_io import Golden
from model_util import build_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
SEED = 20241019  # every random draw of this file

_build = TM._build
_rel = TM._rel
_counts = TP._counts
SHAPES = TM.SHAPES  # (1,1,1), (2,50,4), (2,512,1), (1,1025,1), (3,333,7), (1,4099,1025)
MASKS = ["none", "random", "view", "term"]


def _offsets(views):
    off = [0]
    for n in views:
        off.append(off[-1] + n)
    return off


def _ws(nbytes):
    return torch.empty(int(nbytes) + 64, dtype=torch.uint8, device=DEV)


def _const_ws(lib, N, P, V):
    return _ws(lib.gpsa_nb_const_workspace(N, P, V))


def _loss_ws(shapes, n_views, kinds=None):
    from spatial_alignment_amd import torch_ops as TO

    return _ws(TO.nb_loss_workspace_bytes(shapes, n_views, kinds or [2] * (len(shapes) // 3)))


# ---- 1. the draw-independent pieces --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nb_const(shape, mask):
    """csum[v] = sum of lgamma(y + r) - lgamma(r) per view, dconst[p] = the view-weighted sum of r (psi(y + r) - psi(r)),
    rho uniform in [-3, 6]: within 1e-11 of (sum of magnitudes + 1)"""
    lib = _build()
    _, N, P = shape
    gen = torch.Generator().manual_seed(SEED + N + P)
    views = TM._views_of(N)
    off = _offsets(views)
    Y = _counts(gen, N, P)
    miss = TM._mask(mask, N, P, views, gen)
    Yd = torch.where(miss, torch.full_like(Y, NAN), Y).to(DEV)
    skip = int(mask != "none")
    rho = (9.0 * torch.rand(P, generator=gen) - 3.0)
    r = torch.exp(rho.double())
    Y0 = torch.where(miss, torch.zeros_like(Y), Y).double()
    obs = (~miss).double()
    c_terms = (torch.lgamma(Y0 + r) - torch.lgamma(r)) * obs
    d_terms = r * (torch.digamma(Y0 + r) - torch.digamma(r)) * obs
    for weighted in (False, True):
        V = len(views) if weighted else 1
        w = (torch.rand(V, generator=gen, dtype=torch.float64) + 0.5) if weighted else torch.ones(1, dtype=torch.float64)
        nv, vo, wl = ([V], off, [w.to(DEV)]) if weighted else ([], [], [])
        bounds = off if weighted else [0, N]
        csum = [torch.full((V,), NAN, dtype=torch.float64, device=DEV)]
        dconst = [torch.full((P,), NAN, dtype=torch.float64, device=DEV)]
        torch.ops.gpsa.nb_const([Yd], [rho.to(DEV)], nv, vo, wl, skip, csum, dconst, _const_ws(lib, N, P, V))
        torch.cuda.synchronize()
        want_c = torch.stack([c_terms[bounds[v]:bounds[v + 1]].sum() for v in range(V)])
        mag_c = torch.stack([c_terms[bounds[v]:bounds[v + 1]].abs().sum() for v in range(V)]) + 1.0
        want_d = sum(w[v] * d_terms[bounds[v]:bounds[v + 1]].sum(0) for v in range(V))
        mag_d = sum(w[v] * d_terms[bounds[v]:bounds[v + 1]].abs().sum(0) for v in range(V)) + 1.0
        ec = float(((csum[0].cpu() - want_c).abs() / mag_c).max())
        ed = float(((dconst[0].cpu() - want_d).abs() / mag_d).max())
        print(f"[{shape} {mask} weighted={weighted}] csum {ec:.2g}, dconst {ed:.2g} of the magnitudes")
        assert ec <= 1e-11 and ed <= 1e-11
        if mask == "term":
            assert (csum[0] == 0).all() and (dconst[0] == 0).all()


# ---- 2. the closing pair -------------------------------------------------------------------------------------------------
def _ref_nb(F, Y, miss, off, rho, w_rows, S, kl, kl_scale, gloss):
    """fp64 torch: loss, ll, dF, drho, the magnitudes of ll and (per output) of drho, for one NB term"""
    F = F.double().clone().requires_grad_(True)
    rho = rho.double().clone().requires_grad_(True)
    Y0 = torch.where(miss, torch.zeros_like(Y), Y).double()
    a = F + off.double()[None, :, None] - rho
    r = torch.exp(rho)
    obs = (~miss).double() * w_rows.double()[:, None]
    c = torch.lgamma(Y0 + r) - torch.lgamma(r) - torch.lgamma(Y0 + 1)
    ll = ((Y0 * a - (Y0 + r) * Fn.softplus(a)) * obs).sum() / S + (c * obs).sum()
    loss = -ll + kl_scale * kl.sum()
    dF, drho = torch.autograd.grad(loss * gloss, [F, rho])
    with torch.no_grad():
        sp, sg = Fn.softplus(a), torch.sigmoid(a)
        mag = ((((Y0 * a).abs() + (Y0 + r) * sp) * obs).sum() / S
               + (((torch.lgamma(Y0 + r) - torch.lgamma(r)).abs() + torch.lgamma(Y0 + 1)) * obs).sum() + 1.0)
        mag_rho = abs(gloss) * (((r * sp + (Y0 + r) * sg + Y0) * obs).sum((0, 1)) / S
                                + ((r * (torch.digamma(Y0 + r) - torch.digamma(r))).abs() * obs).sum(0))
    return float(loss.detach()), float(ll.detach()), dF, drho, float(mag), mag_rho


def _nb_tables(Yd, rho_d, nv, vo, wl, skip, V, lib):
    """(lgam, csum, dconst) of one NB term on the device"""
    N, P = Yd.shape
    lgam = [torch.full((V,), NAN, dtype=torch.float64, device=DEV)]
    torch.ops.gpsa.lgamma_sum([Yd], nv, vo, skip, lgam, _ws(8 * 64 * 64))
    csum = [torch.full((V,), NAN, dtype=torch.float64, device=DEV)]
    dconst = [torch.full((P,), NAN, dtype=torch.float64, device=DEV)]
    torch.ops.gpsa.nb_const([Yd], [rho_d], nv, vo, wl, skip, csum, dconst, _const_ws(lib, N, P, V))
    return lgam, csum, dconst


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_closing_pair(shape, mask):
    lib = _build()
    S, N, P = shape
    gen = torch.Generator().manual_seed(SEED + S + N + P)
    views = TM._views_of(N)
    off = _offsets(views)
    F = torch.randn(S, N, P, generator=gen)
    Y = _counts(gen, N, P)
    miss = TM._mask(mask, N, P, views, gen)
    Ym = torch.where(miss, torch.full_like(Y, NAN), Y)
    skip = int(mask != "none")
    offs = 0.5 * torch.randn(N, generator=gen)
    rho = torch.randn(P, generator=gen)
    noise = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float32)
    kl = torch.rand(5, generator=gen, dtype=torch.float64)
    ks, gl = 0.7, -0.75
    Fd, Yd, nd, kd, od, rd = F.to(DEV), Ym.to(DEV), noise.to(DEV), kl.to(DEV), offs.to(DEV), rho.to(DEV)
    g = torch.tensor([gl], device=DEV)
    for weighted in (False, True):
        for with_off in (False, True):
            V = len(views) if weighted else 1
            w = (torch.rand(V, generator=gen, dtype=torch.float64) + 0.5) if weighted else torch.ones(1, dtype=torch.float64)
            nv, vo, wl = ([V], off, [w.to(DEV)]) if weighted else ([], [], [])
            bounds = off if weighted else [0, N]
            lgam, csum, dconst = _nb_tables(Yd, rd, nv, vo, wl, skip, V, lib)
            work = _loss_ws([S, N, P], nv)
            work.fill_(0xFF)  # (NaN patterns: nothing reads what it has not written)
            w_rows = torch.cat([w[v].expand(bounds[v + 1] - bounds[v]) for v in range(V)])
            o_ref = offs if with_off else torch.zeros(N)
            loss = torch.empty(1, device=DEV)
            ll = torch.empty(1, dtype=torch.float64, device=DEV)
            tabs = ([], [], nv, vo, wl, [], [2], lgam, [od if with_off else None], [rd])
            torch.ops.gpsa.elbo_loss_nb_fwd([Fd], [Yd], nd, [1], *tabs, csum, skip, kd, ks, loss, ll, work)
            dF = [torch.full_like(Fd, NAN)]
            dn = torch.full((3,), NAN, device=DEV)
            dkl = torch.empty(5, dtype=torch.float64, device=DEV)
            dd = [torch.full((P,), NAN, device=DEV)]
            torch.ops.gpsa.elbo_loss_nb_bwd([Fd], [Yd], nd, [1], *tabs, dconst, [None], skip, g, 5, ks, dF, dn, dkl, dd, work)
            torch.cuda.synchronize()
            r_loss, r_ll, r_dF, r_dd, mag, mag_rho = _ref_nb(F, Y, miss, o_ref, rho, w_rows, S, kl, ks, gl)
            e_dd = float(((dd[0].cpu().double() - r_dd).abs() / (mag_rho + 1e-300)).max()) if mask != "term" else 0.0
            print(f"[{shape} {mask} weighted={weighted} offsets={with_off}] loss {float(loss):.6g} / {r_loss:.6g}, ll "
                  f"{float(ll):.6g} / {r_ll:.6g} (magnitudes {mag:.3g}), dF rel {_rel(dF[0], r_dF):.2g}, ddisp {e_dd:.2g} "
                  "of its magnitudes")
            assert abs(float(ll) - r_ll) <= 2e-6 * mag
            assert abs(float(loss) - r_loss) <= 2e-6 * mag
            assert torch.isfinite(dF[0]).all() and torch.isfinite(dd[0]).all()
            assert (dn.cpu() == 0).all()  # the NB term's noise gradient and the entries no term names: exactly 0
            if float(r_dF.norm()) > 0:
                assert _rel(dF[0], r_dF) <= 1e-6
            assert e_dd <= 2e-6
            assert (dF[0].cpu()[:, miss] == 0).all()  # exactly 0 at a missing entry
            assert (dd[0].cpu()[miss.all(0)] == 0).all()  # ... and for an output without an observed entry
            assert torch.equal(dkl.cpu(), torch.full((5,), ks * gl, dtype=torch.float64))
            if mask == "term":  # everything missing: exact zeros
                assert float(ll) == 0.0 and (dF[0] == 0).all() and (dd[0] == 0).all()
                assert abs(float(loss) - ks * float(kl.sum())) <= 1e-6


def test_large_log_means_stay_finite():
    """eta = 136 (beyond fp32 exp): t = -136 and dF = 1 for y = 0, r = 1, as the header states"""
    lib = _build()
    F = torch.full((1, 1, 1), 136.0, device=DEV)
    Y = torch.zeros(1, 1, device=DEV)
    rho = torch.zeros(1, device=DEV)
    lgam, csum, dconst = _nb_tables(Y, rho, [], [], [], 0, 1, lib)
    work = _loss_ws([1, 1, 1], [])
    loss, ll = torch.empty(1, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
    tabs = ([], [], [], [], [], [], [2], lgam, [None], [rho])
    torch.ops.gpsa.elbo_loss_nb_fwd([F], [Y], rho, [0], *tabs, csum, 0, None, 1.0, loss, ll, work)
    dF, dn, dd = [torch.empty_like(F)], torch.empty(1, device=DEV), [torch.empty(1, device=DEV)]
    g = torch.ones(1, device=DEV)
    torch.ops.gpsa.elbo_loss_nb_bwd([F], [Y], rho, [0], *tabs, dconst, [None], 0, g, 0, 1.0, dF, dn, None, dd, work)
    assert abs(float(ll) + 136.0) <= 1e-12 and float(loss) == 136.0 and float(dF[0]) == 1.0
    assert float(dd[0]) == -(-136.0 + 1.0)  # u = -r softplus(a) + (y + r) sigma(a) - y = -135, ddisp = -gloss u


def test_flag_off_nan_reaches_the_loss_of_the_closing():
    lib = _build()
    gen = torch.Generator().manual_seed(SEED)
    F, Y = torch.randn(2, 50, 4, generator=gen).to(DEV), _counts(gen, 50, 4).to(DEV)
    Y[3, 1] = NAN
    rho = torch.zeros(4, device=DEV)
    lgam, csum, dconst = _nb_tables(Y, rho, [], [], [], 0, 1, lib)
    loss, ll = torch.empty(1, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
    torch.ops.gpsa.elbo_loss_nb_fwd([F], [Y], torch.zeros(1, device=DEV), [0], [], [], [], [], [], [], [2], lgam, [None], [rho],
                                    csum, 0, None, 1.0, loss, ll, _loss_ws([2, 50, 4], []))
    assert torch.isnan(loss).all() and torch.isnan(ll).all() and torch.isnan(csum[0]).all()
    assert torch.isnan(dconst[0][1]) and torch.isfinite(dconst[0][[0, 2, 3]]).all()


@pytest.mark.parametrize("masked", [False, True], ids=["weighted", "skip"])
def test_mixed_call_closes_gaussian_and_poisson_terms_as_the_poisson_pair_does(masked):
    """one call with a Gaussian, a Poisson and an NB term: the first two come out as elbo_loss_pois_* gives them on the
    same inputs (bitwise: the same launches), the NB term against fp64, the loss as the sum of the three"""
    lib = _build()
    gen = torch.Generator().manual_seed(SEED + 1)
    S, N, P = 3, 333, 7
    views = TM._views_of(N)
    off = _offsets(views)
    Fg, Yg = torch.randn(S, N, P, generator=gen), torch.randn(N, P, generator=gen)
    Sp, Np, Pp = 2, 50, 4
    Fp, Yp = torch.randn(Sp, Np, Pp, generator=gen), _counts(gen, Np, Pp)
    Sn, Nn, Pn = 2, 77, 5
    Fn_, Yn = torch.randn(Sn, Nn, Pn, generator=gen), _counts(gen, Nn, Pn)
    op, on = 0.5 * torch.randn(Np, generator=gen), 0.5 * torch.randn(Nn, generator=gen)
    rho = torch.randn(Pn, generator=gen)
    mk = lambda n, p: (torch.rand(n, p, generator=gen) < 0.3) if masked else torch.zeros(n, p, dtype=torch.bool)
    missg, missp, missn = mk(N, P), mk(Np, Pp), mk(Nn, Pn)
    nanify = lambda Y, m: torch.where(m, torch.full_like(Y, NAN), Y)
    wg = torch.rand(3, generator=gen, dtype=torch.float64) + 0.5
    wp = torch.rand(1, generator=gen, dtype=torch.float64) + 0.5
    wn = torch.rand(1, generator=gen, dtype=torch.float64) + 0.5
    d = lambda t: t.to(DEV)
    noise = d(torch.tensor([0.3, -0.2, 0.4], dtype=torch.float32))
    kl = d(torch.rand(5, generator=gen, dtype=torch.float64))
    ks, gl = 0.7, -0.75
    g = torch.tensor([gl], device=DEV)
    skip = int(masked)
    Fs, Ys = [d(Fg), d(Fp), d(Fn_)], [d(nanify(Yg, missg)), d(nanify(Yp, missp)), d(nanify(Yn, missn))]
    nv, vo, wl = [3, 1, 1], off + [0, Np] + [0, Nn], [d(wg), d(wp), d(wn)]
    cws = _ws(8 * 64 * 64)
    lgp = torch.empty(1, dtype=torch.float64, device=DEV)
    torch.ops.gpsa.lgamma_sum([Ys[1]], [1], [0, Np], skip, [lgp], cws)
    lgn, csum, dconst = _nb_tables(Ys[2], d(rho), [1], [0, Nn], [d(wn)], skip, 1, lib)
    nobs = []
    if masked:
        cnt = torch.empty(3, dtype=torch.float64, device=DEV)
        torch.ops.gpsa.count_observed([Ys[0]], [3], off, [cnt], cws)
        nobs = [cnt, None, None]
    shapes = [S, N, P, Sp, Np, Pp, Sn, Nn, Pn]
    work = _loss_ws(shapes, nv, [0, 1, 2])  # (only the NB term has column partials)
    tabs = ([], [], nv, vo, wl, nobs, [0, 1, 2], [None, lgp, lgn[0]], [None, d(op), d(on)], [None, None, d(rho)])
    loss, ll = torch.empty(1, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV)
    torch.ops.gpsa.elbo_loss_nb_fwd(Fs, Ys, noise, [0, 1, 2], *tabs, [None, None, csum[0]], skip, kl, ks, loss, ll, work)
    dF = [torch.full_like(f, NAN) for f in Fs]
    dn, dkl = torch.full((3,), NAN, device=DEV), torch.empty(5, dtype=torch.float64, device=DEV)
    dd = [g, g, torch.full((Pn,), NAN, device=DEV)]
    torch.ops.gpsa.elbo_loss_nb_bwd(Fs, Ys, noise, [0, 1, 2], *tabs, [None, None, dconst[0]], [None] * 3, skip, g, 5, ks, dF,
                                    dn, dkl, dd, work)
    # the first two terms through the Poisson pair
    ptabs = ([], [], nv[:2], vo[:6], wl[:2], nobs[:2], [0, 1], [None, lgp], [None, d(op)], skip)
    l2, ll2 = torch.empty(1, device=DEV), torch.empty(2, dtype=torch.float64, device=DEV)
    torch.ops.gpsa.elbo_loss_pois_fwd(Fs[:2], Ys[:2], noise, [0, 1], *ptabs, kl, ks, l2, ll2, work)
    dF2 = [torch.full_like(f, NAN) for f in Fs[:2]]
    dn2, dkl2 = torch.full((3,), NAN, device=DEV), torch.empty(5, dtype=torch.float64, device=DEV)
    torch.ops.gpsa.elbo_loss_pois_bwd(Fs[:2], Ys[:2], noise, [0, 1], *ptabs, g, 5, ks, dF2, dn2, dkl2, work)
    torch.cuda.synchronize()
    assert torch.equal(ll[:2], ll2) and torch.equal(dF[0], dF2[0]) and torch.equal(dF[1], dF2[1])
    assert torch.equal(dn[:2], dn2[:2]) and float(dn[2]) == 0.0 and torch.equal(dkl, dkl2)
    r_loss, r_ll, r_dF, r_dd, mag, mag_rho = _ref_nb(Fn_, Yn, missn, on, rho, wn.expand(Nn), Sn,
                                                     torch.zeros(1, dtype=torch.float64), 0.0, gl)
    assert abs(float(ll[2]) - r_ll) <= 2e-6 * mag and _rel(dF[2], r_dF) <= 1e-6
    assert float(((dd[2].cpu().double() - r_dd).abs() / mag_rho).max()) <= 2e-6
    want = ks * float(kl.sum()) - float(ll2.sum()) - r_ll
    assert abs(float(loss) - want) <= 2e-6 * (mag + float(ll2.abs().sum()))


def test_an_nb_term_closes_from_partial_sums_and_its_sums_of_u():
    """an NB term that arrives as nparts partial sums of t with its [P] sums of u: the closing adds the constants and
    turns the sums into the gradient of rho"""
    _build()
    gen = torch.Generator().manual_seed(SEED + 2)
    S, N, P = 2, 50, 4
    tp = torch.randn(7, generator=gen, dtype=torch.float64) * 10
    us = torch.randn(P, generator=gen, dtype=torch.float64) * 5
    dc = torch.randn(P, generator=gen, dtype=torch.float64)
    Y = torch.zeros(N, P, device=DEV)
    rho = torch.zeros(P, device=DEV)
    one = torch.ones(1, dtype=torch.float64, device=DEV)
    lgam, csum = torch.tensor([12.5], dtype=torch.float64, device=DEV), torch.tensor([3.25], dtype=torch.float64, device=DEV)
    tabs = ([S, N, P], [1], [1], [0, N], [one], [], [2], [lgam], [None], [rho])
    work = _loss_ws([S, N, P], [1])
    loss, ll = torch.empty(1, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
    torch.ops.gpsa.elbo_loss_nb_fwd([tp.to(DEV)], [Y], rho, [0], *tabs, [csum], 0, None, 1.0, loss, ll, work)
    g = torch.tensor([-0.5], device=DEV)
    dn, dd = torch.full((P,), NAN, device=DEV), [torch.full((P,), NAN, device=DEV)]
    torch.ops.gpsa.elbo_loss_nb_bwd([tp.to(DEV)], [Y], rho, [0], *tabs, [dc.to(DEV)], [us.to(DEV)], 0, g, 0, 1.0, [g], dn,
                                    None, dd, work)
    want = float(tp.sum()) / S + 3.25 - 12.5
    assert abs(float(ll) - want) <= 1e-12 * (abs(want) + 1) and abs(float(loss) + want) <= 1e-6 * (abs(want) + 1)
    assert (dn == 0).all()
    want_dd = 0.5 * (us / S + dc)
    assert float((dd[0].cpu().double() - want_dd).abs().max()) <= 1e-6 * float(want_dd.abs().max())


# ---- 3a. the fused ELBO pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("M,delta_form", [(200, True), (64, False)])
def test_quadform_elbo_nb(M, delta_form, masked):
    """the fp64 chain of tests/test_poisson_gpu.py::test_quadform_elbo_pois with the NB term in the closing: g, dmeanT, abar,
    F, the partial sums of t, u per element (exact 0 at a missing entry) and its per-output sums; workspace at exactly the
    queried size, pre-filled with NaN patterns; one output fully missing in the masked cases"""
    lib = _build()
    L, S, N = 3, 3, 77  # C = 231 ends inside a column tile
    Cn = S * N
    gen = torch.Generator().manual_seed(SEED + M)
    Om, alpha, delta, q, eps, _ = TM._elbo_inputs(M, L, S, N, gen)
    delta = delta * (1.0 / math.sqrt(M))
    Y = _counts(gen, N, L)
    offs = 0.5 * torch.randn(N, generator=gen)
    rho = torch.randn(L, generator=gen)
    miss = torch.zeros(N, L, dtype=torch.bool)
    if masked:
        miss = torch.rand(N, L, generator=gen) < 0.3
        miss[:, 1] = True  # one fully missing output
    Ym = torch.where(miss, torch.full_like(Y, NAN), Y)
    var_u = torch.tensor([0.3])
    a64 = alpha.double().requires_grad_(True)
    mean64 = (delta.double().t() @ a64).detach().requires_grad_(True)  # [L, C]
    W = Om @ a64  # [L, M, C]
    v = (a64[None] * W).sum(1)
    var = (math.exp(0.3) - q)[None] + v + 2e-5
    Fd = mean64 + var.sqrt() * eps.double().t()
    aa = Fd + offs.double().repeat(S)[None] - rho.double()[:, None]  # column c -> row c % N
    r = torch.exp(rho.double())[:, None]
    Yc = torch.where(miss, torch.zeros_like(Y), Y).double().t().repeat(1, S)  # [L, C]
    mc = miss.t().repeat(1, S)
    obs = (~mc).double()
    sp, sg = Fn.softplus(aa), torch.sigmoid(aa)
    terms = (Yc * aa - (Yc + r) * sp) * obs
    loss = -terms.sum() / S
    var.retain_grad()
    dmean_ref, = torch.autograd.grad(loss, [mean64], retain_graph=True)
    g_ref, = torch.autograd.grad(loss, [var], retain_graph=True)
    abar_ref = 2 * (g_ref[:, None, :] * W.detach()).sum(0)
    with torch.no_grad():
        mag = float((((Yc * aa).abs() + (Yc + r) * sp) * obs).sum())
        u_ref = (-r * sp + (Yc + r) * sg - Yc) * obs
        u_mag = ((r * sp + (Yc + r) * sg + Yc) * obs).sum(1)
    d = lambda t: t.to(DEV).contiguous()
    al, Omd, dl, qd, ed, Yd, od, rd = d(alpha), d(Om), d(delta), d(q), d(eps), d(Ym), d(offs), d(rho)
    meanT = d((delta.double().t() @ alpha.double()).float())
    nparts = lib.gpsa_quadform_elbo_parts()
    g, dm, FT, ue = (torch.full((L, Cn), NAN, device=DEV) for _ in range(4))
    abar = torch.full((M, Cn), NAN, device=DEV)
    part = torch.full((nparts,), NAN, dtype=torch.float64, device=DEV)
    usum = torch.full((L,), NAN, dtype=torch.float64, device=DEV)
    wsb = lib.gpsa_quadform_elbo_f32_workspace(M, Cn, L)
    assert wsb > 0
    ws = torch.full((wsb,), 255, dtype=torch.uint8, device=DEV)  # the queried size exactly, NaN bit patterns
    vu = d(var_u)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    skip = int(masked)
    if delta_form:
        assert lib.gpsa_quadform_elbo_takes_delta(M) == 1
        rc = lib.gpsa_quadform_elbo_delta_nb_f32(1, p(al), p(Omd), M, Cn, L, p(dl), p(qd), p(vu), p(ed), p(Yd), N, S, None,
                                                 p(g), p(dm), p(abar), p(part), p(FT), p(od), p(rd), p(ue), p(usum), skip,
                                                 p(ws), wsb, C.c_void_p(st))
    else:
        rc = lib.gpsa_quadform_elbo_nb_f32(1, p(al), p(Omd), M, Cn, L, p(meanT), p(qd), p(vu), p(ed), p(Yd), N, S, None, p(g),
                                           p(dm), p(abar), p(part), p(FT), p(od), p(rd), p(ue), p(usum), skip, p(ws), wsb,
                                           C.c_void_p(st))
    assert rc == 0
    torch.cuda.synchronize()
    mcd = mc.to(DEV)
    assert (g[mcd] == 0).all() and (dm[mcd] == 0).all() and (ue[mcd] == 0).all()  # exactly 0 at the missing entries
    assert torch.isfinite(ue).all() and torch.isfinite(usum).all()
    e_us = float(((usum.cpu() - u_ref.sum(1)).abs() / (u_mag + 1e-300))[u_mag > 0].max())
    errs = dict(g=_rel(g, g_ref), dmeanT=_rel(dm, dmean_ref), abar=_rel(abar, abar_ref), F=_rel(FT, Fd),
                part=abs(float(part.sum()) - float(terms.sum().detach())) / mag, u=_rel(ue, u_ref), usum=e_us)
    print(f"[quadform_elbo_nb M={M} masked={masked}]", {k: f"{e:.2e}" for k, e in errs.items()},
          f"max |a| {float(aa.abs().max()):.1f}")
    assert errs["g"] <= 3e-5 and errs["dmeanT"] <= 3e-5 and errs["abar"] <= 3e-5 and errs["F"] <= 3e-5
    assert errs["part"] <= 2e-6 and errs["usum"] <= 2e-6
    if masked:
        assert float(usum[1]) == 0.0  # the fully missing output


# ---- 3. the fused LMC likelihood -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,P", [(3, 5), (20, 70), (40, 9)], ids=["L3", "L20", "L40"])
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
def test_lmc_loglik_fused_nb(masked, L, P):
    """gpsa_lmc_loglik_fused_nb_f32 at exactly the queried workspace, pre-filled with NaN patterns: one case per
    instantiation (L <= 16, <= 32, <= 64).  Every case fits one chunk of outputs: the NB kernels walk 256, 128 and 64 of
    them at a time, so P = 70 at L = 20 is one chunk of 128 (more than one chunk: tests/test_lmc_lik_gpu.py)"""
    lib = _build()
    N, S = 77, 2
    gen = torch.Generator().manual_seed(SEED + 3 + L)
    F = torch.randn(S, N, L, generator=gen)
    W = 0.5 * torch.randn(L, P, generator=gen) / math.sqrt(L / 3.0)
    Y = _counts(gen, N, P)
    offs = 0.5 * torch.randn(N, generator=gen)
    rho = torch.randn(P, generator=gen)
    miss = torch.zeros(N, P, dtype=torch.bool)
    if masked:
        miss = torch.rand(N, P, generator=gen) < 0.3
        miss[:, 2] = True
    Ym = torch.where(miss, torch.full_like(Y, NAN), Y)
    F64, W64 = F.double().requires_grad_(True), W.double().requires_grad_(True)
    a = F64 @ W64 + offs.double()[None, :, None] - rho.double()
    r = torch.exp(rho.double())
    Y0 = torch.where(miss, torch.zeros_like(Y), Y).double()
    obs = (~miss).double()[None]
    sp, sg = Fn.softplus(a), torch.sigmoid(a)
    terms = (Y0 * a - (Y0 + r) * sp) * obs
    loss = -terms.sum() / S
    dF_ref, dW_ref = torch.autograd.grad(loss, [F64, W64])
    with torch.no_grad():
        mag = float((((Y0 * a).abs() + (Y0 + r) * sp) * obs).sum())
        u_ref = ((-r * sp + (Y0 + r) * sg - Y0) * obs).sum((0, 1))
        u_mag = ((r * sp + (Y0 + r) * sg + Y0) * obs).sum((0, 1))
    nparts = lib.gpsa_quadform_elbo_parts()
    zpart = torch.full((nparts,), NAN, dtype=torch.float64, device=DEV)
    dF, dW = torch.full((S, N, L), NAN, device=DEV), torch.full((L, P), NAN, device=DEV)
    usum = torch.full((P,), NAN, dtype=torch.float64, device=DEV)
    need = lib.gpsa_lmc_loglik_nb_workspace(S * N, L, P, nparts)
    assert need > lib.gpsa_lmc_loglik_workspace(S * N, L, P, nparts)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
    torch.ops.gpsa.lmc_loglik_fused_nb(F.to(DEV), W.to(DEV), Ym.to(DEV), offs.to(DEV), rho.to(DEV), int(masked), zpart, dF,
                                       dW, usum, ws)
    torch.cuda.synchronize()
    e_u = float(((usum.cpu() - u_ref).abs() / (u_mag + 1e-300))[u_mag > 0].max())
    errs = dict(dF=_rel(dF, dF_ref), dW=_rel(dW, dW_ref), part=abs(float(zpart.sum()) - float(terms.sum())) / mag, u=e_u)
    print(f"[lmc_loglik_fused_nb L={L} masked={masked}]", {k: f"{e:.2e}" for k, e in errs.items()})
    assert errs["dF"] <= 3e-5 and errs["dW"] <= 3e-5 and errs["part"] <= 2e-6 and errs["u"] <= 2e-6
    assert (usum.cpu()[miss.all(0)] == 0).all() and torch.isfinite(usum).all()


# ---- 4. whole steps against the fp64 oracle ------------------------------------------------------------------------------
STEP_CASES = ["c1_example_fixed0", "c2_three_free_views", "c3_lmc_matern12_warp", "c5_two_modalities",
              "c10_unequal_two_fixed", "c11_lmc_gtest_unequal", "c7_m200_conditioning"]
_REFS = {}
_nb_mods = TP._pois_mods  # c5 is the mixed model: rna NB, protein Gaussian; every other case is all NB
_count_data = TP._count_data


def _rhos(g):
    gen = torch.Generator().manual_seed(SEED + 3)
    return {m: torch.randn(g.Y[m].shape[1], generator=gen) for m in _nb_mods(g)}


def _nb_step_reference(name, mask_kind=None):
    """fp64: orc.forward_pass, negative_elbo, the Gaussian log density of every NB modality taken back out, its NB log
    density (over the observed entries under ``mask_kind``) put in, rho a leaf; once per (case, mask)"""
    key = (name, mask_kind)
    if key in _REFS:
        return _REFS[key]
    from oracle import gpsa_oracle as orc

    g = Golden(name)
    Yc, off = _count_data(g)
    nbm = _nb_mods(g)
    rho = {m: t.double().requires_grad_(True) for m, t in _rhos(g).items()}
    miss = TM._step_mask(g, mask_kind) if mask_kind else {m: torch.zeros_like(g.Y[m], dtype=torch.bool) for m in g.mods}
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
    Y64 = {m: Yc[m].double() for m in g.mods}
    loss = orc.negative_elbo(st, cfg, h, Y64, out["F_obs"])
    n_mod = len(g.mods)
    max_eta = 0.0
    for i, m in enumerate(g.mods):
        if m not in nbm:
            continue
        Fo = out["F_obs"][m]
        S = Fo.shape[0]
        scale = h["noise_variance_pos"][-n_mod + i]
        loss = loss + torch.distributions.Normal(Fo, scale).log_prob(Y64[m]).sum() / S  # the Gaussian term back out
        eta = Fo + off[m].double()[None, :, None]
        a, r = eta - rho[m], torch.exp(rho[m])
        obs = (~miss[m]).double()
        y = Y64[m]
        c = torch.lgamma(y + r) - torch.lgamma(r) - torch.lgamma(y + 1)
        loss = loss - (((y * a - (y + r) * Fn.softplus(a)) * obs).sum() / S + (c * obs).sum())
        max_eta = max(max_eta, float(eta.abs().max()))
    leaves = {k: t for k, t in st.items() if t.requires_grad}
    leaves.update({f"log_dispersion.{m}": t for m, t in rho.items()})
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    ref = {"loss": loss.detach().numpy()}
    for (k, t), gr in zip(leaves.items(), gs):
        ref[f"grad/{k}"] = (gr if gr is not None else torch.zeros_like(t)).detach().numpy().copy()
    # the NB modalities' noise entries: +g - g of the two Gaussian terms; exactly 0 is what the model must give
    nz = ref["grad/noise_variance"].reshape(-1)
    for i, m in enumerate(g.mods):
        if m in nbm:
            assert abs(nz[-n_mod + i]) <= 1e-9 * max(1.0, float(np.abs(nz).max())), nz
            nz[-n_mod + i] = 0.0
    for nm, o in out.items():
        for m in g.mods:
            ref[f"{nm}/{m}"] = o[m].detach().numpy()
    _REFS[key] = (g, Yc, off, miss, ref, max_eta)
    return _REFS[key]


def _nb_problem(g, Yc, off, miss=None, **attrs):
    """the golden's model on the device with the count data: likelihood, rho, offsets, and NaN at ``miss``"""
    model, dd = build_model(g, device=DEV)
    nbm = _nb_mods(g)
    model.likelihood = "negative_binomial" if len(nbm) == len(g.mods) else {m: "negative_binomial" for m in nbm}
    rho = _rhos(g)
    for m in g.mods:
        Y = Yc[m].to(DEV)
        if miss is not None:
            Y = torch.where(miss[m].to(DEV), torch.full_like(Y, NAN), Y)
        dd[m]["outputs"] = Y.contiguous()
        if m in nbm:
            dd[m]["log_offset"] = off[m].to(DEV)
            assert model.log_dispersion[m].device == model.Xtilde.device
            with torch.no_grad():
                model.log_dispersion[m].copy_(rho[m])
    model.fuse_min_flops = 0  # (the golden cases are tiny: the fused pass would be declined at this size)
    for k, v in attrs.items():
        setattr(model, k, v)
    return model, dd


def _check_step(model, dd, g, ref, label, lazy_lmc=False):
    from spatial_alignment_amd.lazy import LazyProduct

    loss, out = TM._run_step(model, dd, g)
    rec = model._cache.fuse
    if not lazy_lmc:
        assert rec is None or "fused" not in rec["state"]
    elif any(model.n_latent_gps[m] is None for m in g.mods):  # gpsa_step_dispersion -> panel_elbo_nb_kernel really ran
        assert rec is not None and "fused" in rec["state"], "the fused ELBO path did not run"
        for i, m in enumerate(g.mods):
            if m in _nb_mods(g) and model.n_latent_gps[m] is None:
                assert rec["state"][i] == "fused" and i in rec["nb_usum"]
    for m in g.mods:  # a lazy LMC product was never formed: the fused LMC kernel (lmc_mfma_nb_kernel) ran in its place
        if model.n_latent_gps[m] is not None:
            if lazy_lmc and g.G_test is None:
                assert isinstance(out[3][m], LazyProduct)
            if isinstance(out[3][m], LazyProduct):
                assert not out[3][m].is_materialized
    res = TM._collect(model, loss, out, g)
    errs, bad = TM._against(res, ref)
    print(label, {k: f"{v:.1e}" for k, v in errs.items()})
    assert not bad, bad
    n_mod = len(g.mods)
    for i, m in enumerate(g.mods):  # an NB modality's noise gradient: exactly 0
        if m in _nb_mods(g):
            assert float(model.noise_variance.grad.reshape(-1)[-n_mod + i]) == 0.0
            assert f"grad/log_dispersion.{m}" in ref and np.abs(ref[f"grad/log_dispersion.{m}"]).max() > 0
    return res


@pytest.mark.parametrize("fuse", [True, False], ids=["fuse_elbo", "separate"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_step_matches_negbin_fp64_reference(name, fuse):
    """fuse_elbo on: an NB modality without latent mixing takes the fused ELBO pass (gpsa_step_dispersion ->
    panel_elbo_nb_kernel; c5's Gaussian protein next to it takes its own), an NB LMC modality (c3, c11) takes
    gpsa_lmc_loglik_fused_nb_f32 without forming F W; off: the draws come from forward"""
    _build()
    g, Yc, off, _, ref, max_eta = _nb_step_reference(name)
    if name.startswith("c7"):
        assert max_eta > 88.0, max_eta  # beyond fp32 exp: the case the Poisson steps had to leave out
    model, dd = _nb_problem(g, Yc, off, fuse_elbo=fuse)
    _check_step(model, dd, g, ref, f"{name} {'fuse_elbo' if fuse else 'separate'}", lazy_lmc=fuse)


def test_per_layer_path_matches_negbin_fp64_reference():
    """use_step_engine = False: the layers' nodes and the one loss node on materialised draws"""
    _build()
    name = "c10_unequal_two_fixed"
    g, Yc, off, _, ref, _ = _nb_step_reference(name)
    model, dd = _nb_problem(g, Yc, off, use_step_engine=False)
    _check_step(model, dd, g, ref, f"{name} layers")


# ---- 5. compositions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c10_unequal_two_fixed", "c3_lmc_matern12_warp"])
def test_skip_missing_panels_against_the_reference_over_observed_entries(name):
    _build()
    g, Yc, off, miss, ref, _ = _nb_step_reference(name, "panels")
    model, dd = _nb_problem(g, Yc, off, miss, skip_missing=True)
    _check_step(model, dd, g, ref, f"{name} panels", lazy_lmc=True)


def test_flag_off_propagates_nan():
    _build()
    name = "c10_unequal_two_fixed"
    g, Yc, off, _, _, _ = _nb_step_reference(name)
    model, dd = _nb_problem(g, Yc, off)
    dd[g.mods[0]]["outputs"][0, 0] = NAN
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    model.inject_noise(g.eps_G, g.eps_F, None)
    out = model.forward({m: dd[m]["spatial_coords"] for m in g.mods}, view_idx=view_idx, Ns=Ns, S=g.S)
    assert torch.isnan(model.loss_fn(dd, out[3]))


def test_two_runs_of_the_same_step_are_bitwise_equal():
    _build()
    name = "c5_two_modalities"
    g, Yc, off, _, _, _ = _nb_step_reference(name)
    runs = []
    for _ in range(2):
        model, dd = _nb_problem(g, Yc, off)
        loss, out = TM._run_step(model, dd, g)
        runs.append(TM._collect(model, loss, out, g))
    assert any(k.startswith("grad/log_dispersion.") for k in runs[0])
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_cover_of_negbin_batches_is_unbiased():
    """minibatch: the mean over a cover of batches equals the full NB loss and gradient, rho's included (the offsets are
    gathered with the rows, both constant tables recomputed on every batch); tests/test_poisson_gpu.py's construction"""
    import test_minibatch_gpu as T

    MB = T._lib()
    model, dd, eG, eF = T._two_modality_problem()
    model.likelihood = "negative_binomial"
    gen = torch.Generator().manual_seed(SEED + 4)
    for m in T.MODS:
        Y = dd[m]["outputs"]
        dd[m]["outputs"] = torch.floor(torch.exp(torch.clamp(Y, max=3.0)))
        dd[m]["log_offset"] = (0.25 * torch.sin(torch.arange(Y.shape[0], dtype=torch.float32))).to(DEV)
        with torch.no_grad():
            model.log_dispersion[m].copy_(torch.randn(Y.shape[1], generator=gen))
    vi, Ns, _, _ = model.create_view_idx_dict(dd)
    full_loss, full_g = T._step(model, dd, vi, Ns, [torch.cat([eG[m] for m in T.MODS], 1)], eF)
    assert math.isfinite(full_loss) and any(n.startswith("log_dispersion.") for n in full_g)
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


def test_graphed_negbin_step_equals_eager():
    """tests/test_poisson_gpu.py::test_graphed_poisson_step_equals_eager with NB outputs: 3 eager + 1 replayed step land
    on the parameters of 4 eager steps, rho among them"""
    from spatial_alignment_amd.train import GraphedTrainStep, train_step

    _build()
    name = "c10_unequal_two_fixed"
    g, Yc, off, _, _, _ = _nb_step_reference(name)
    res = []
    for mode in ("eager", "graph"):
        model, dd = _nb_problem(g, Yc, off)
        view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
        eps_G = [e.to(DEV) for e in g.eps_G]
        eps_F = {m: e.to(DEV) for m, e in g.eps_F.items()}
        orig = model.forward

        def fwd(*a, _orig=orig, _m=model, **k):  # same injected noise on every call
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
        assert math.isfinite(float(loss))
        res.append((float(loss), {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    assert any(k.startswith("log_dispersion.") for k in res[0][1])
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    moved = res[0][1][f"log_dispersion.{g.mods[0]}"] - _rhos(g)[g.mods[0]]
    assert float(moved.abs().min()) > 0  # the optimizer stepped rho


def test_row_shares_and_output_shares_sum_to_the_full_negbin_step():
    """emulated two-way shardings: the row shares' losses and gradients sum to the full step's (rho is shared: its
    gradient sums over the ranks); an output share's rho gradient is the full one's slice (a rank owns its columns' rho)"""
    import test_parallel_gpu as T
    from spatial_alignment_amd.parallel import shard_data_dict, shard_outputs, shard_rows

    _build()
    world, n = 2, T.SIDE * T.SIDE
    eG, eF = T._noise()
    gen = torch.Generator().manual_seed(SEED + 5)
    P = T._problem(DEV)[0]["expression"]["outputs"].shape[1]
    rho = torch.randn(P, generator=gen)

    def problem():
        dd, model = T._problem(DEV)
        Y = dd["expression"]["outputs"]
        dd["expression"]["outputs"] = torch.floor(torch.exp(torch.clamp(Y, max=3.0)))
        dd["expression"]["log_offset"] = (0.25 * torch.sin(torch.arange(2 * n, dtype=torch.float32))).to(DEV)
        model.likelihood = "negative_binomial"
        with torch.no_grad():
            model.log_dispersion["expression"].copy_(rho)
        model.fuse_min_flops = 0
        return dd, model

    dd, model = problem()
    loss1 = T._grads(model, dd, eG, eF, 1.0, fuse=True)
    assert math.isfinite(float(loss1))
    want = {k: p.grad.detach().double().clone() for k, p in model.named_parameters()}
    assert float(want["log_dispersion.expression"].abs().min()) > 0
    tot, acc = 0.0, {k: torch.zeros_like(v) for k, v in want.items()}
    for r in range(world):
        dd_r, model_r = problem()
        sdd = shard_data_dict(dd_r, r, world)
        lo, hi = shard_rows(n, r, world)
        rows = torch.cat([torch.arange(lo, hi), n + torch.arange(lo, hi)])
        tot += float(T._grads(model_r, sdd, [e[:, lo:hi] for e in eG], eF[:, rows], 1.0, fuse=True, owner=(r, world)))
        for k, p in model_r.named_parameters():
            acc[k] += p.grad.detach().double()
    assert abs(tot - float(loss1)) <= 1e-5 * abs(float(loss1)), (tot, float(loss1))
    for k in want:
        e = float((acc[k] - want[k]).norm()) / max(float(want[k].norm()), 1e-6)
        assert e <= 1e-4, (k, e)
    # output shares: the loss node alone on a column slice of the same draws
    from spatial_alignment_amd import step_engine as SE

    F = torch.randn(2, 2 * n, P, generator=gen).to(DEV)
    Y, o = dd["expression"]["outputs"], dd["expression"]["log_offset"]
    one = torch.ones(1, dtype=torch.float64, device=DEV)

    def node(Fc, Yc, rh):
        aux = dict(Y=[Yc.contiguous()], noise_idx=[0], kl_scale=1.0, kinds=[2], log_offset=[o], skip=False, n_views=[1],
                   view_off=[0, 2 * n], weights=[one], nobs=None, disp={0: 0})
        aux["lgam"] = SE.lgamma_sums(model, aux["Y"], None, False, cacheable=False)
        rh = rh.clone().requires_grad_(True)
        loss = SE.ElboLossFn.apply(aux, torch.zeros(1, device=DEV), None, Fc.contiguous(), rh)
        loss.backward()
        return float(loss), rh.grad

    full_l, full_g = node(F, Y, rho.to(DEV))
    tot = 0.0
    for r in range(world):
        lo, hi = shard_rows(P, r, world)
        sy = shard_outputs({"expression": dict(dd["expression"])}, r, world)["expression"]["outputs"]
        l, gr = node(F[:, :, lo:hi], sy, rho[lo:hi].to(DEV))
        tot += l
        assert _rel(gr, full_g[lo:hi]) <= 1e-6
    assert abs(tot - full_l) <= 1e-5 * abs(full_l)


def test_bf16x3_plan_takes_the_fp32_negbin_kernel_and_goes_back():
    """contraction = "bf16x3": an NB modality's fused pass runs the fp32 NB kernel inside the x3 plan, the Gram stays on x3,
    and plan.contraction / gpsa_step_contraction say so; Gaussian again, the same plan runs x3"""
    from model_util import compare

    _build()
    name = "c10_unequal_two_fixed"
    g, Yc, off, _, ref, _ = _nb_step_reference(name)
    model, dd = _nb_problem(g, Yc, off, contraction="bf16x3")
    gauss = {m: build_model(g, device=DEV)[1][m]["outputs"] for m in g.mods}

    def seen():
        plans = list(model.__dict__.get("_step_plans", {}).values())
        assert plans
        vals = set()
        for p in plans:
            assert p.key[-1] == "bf16x3"
            for i, m in enumerate(p.mods):
                assert p.contraction[m] == int(p.lib.gpsa_step_contraction(p.handle, i))
                vals.add(p.contraction[m])
        assert len(vals) == 1, vals
        return vals.pop()

    _check_step(model, dd, g, ref, f"{name} bf16x3 + negbin", lazy_lmc=True)
    with_nb = seen()
    assert with_nb & 1 == 0
    model.likelihood = "gaussian"
    for m in g.mods:
        dd[m]["outputs"] = gauss[m]
        del dd[m]["log_offset"]
    loss, out = TM._run_step(model, dd, g)
    assert model._cache.fuse is not None and "fused" in model._cache.fuse["state"]
    bad, errs = compare(TM._collect(model, loss, out, g), g, tol_out=1e-4, tol_grad=1e-4)
    assert not bad, bad
    back = seen()
    assert back & 1 == 1 and back & ~1 == with_nb & ~1, (with_nb, back)  # the fused pass is on x3 again


def test_step_setters_refuse_kind_2_without_a_dispersion():
    """gpsa_step_likelihood takes kinds 0 and 1 only - the NB kind is reached through gpsa_step_dispersion, which refuses
    a missing rho, u array or sum table - and going back through gpsa_step_likelihood forgets the tensors"""
    _build()
    name = "c10_unequal_two_fixed"
    g, Yc, off, _, _, _ = _nb_step_reference(name)
    model, dd = _nb_problem(g, Yc, off)
    TM._run_step(model, dd, g)
    p = next(iter(model._step_plans.values()))
    rec = model._cache.fuse
    o = dd[g.mods[0]]["log_offset"]
    rho, u, us = rec["log_disp"][0], rec["nb_u"][0], rec["nb_usum"][0]
    lik, disp = p.lib.gpsa_step_likelihood, p.lib.gpsa_step_dispersion
    assert lik(p.handle, 0, 2, None) == -1 and lik(p.handle, 0, 2, o.data_ptr()) == -1  # kind 2 without a dispersion
    assert disp(None, 0, rho.data_ptr(), u.data_ptr(), us.data_ptr(), None) == -1
    assert disp(p.handle, 0, None, u.data_ptr(), us.data_ptr(), None) == -1
    assert disp(p.handle, 0, rho.data_ptr(), None, us.data_ptr(), None) == -1
    assert disp(p.handle, 0, rho.data_ptr(), u.data_ptr(), None, None) == -1
    assert disp(p.handle, len(g.mods), rho.data_ptr(), u.data_ptr(), us.data_ptr(), None) == -1
    assert disp(p.handle, -1, rho.data_ptr(), u.data_ptr(), us.data_ptr(), None) == -1
    assert disp(p.handle, 0, rho.data_ptr(), u.data_ptr(), us.data_ptr(), o.data_ptr()) == 0
    assert disp(p.handle, 0, rho.data_ptr(), u.data_ptr(), us.data_ptr(), None) == 0
    assert lik(p.handle, 0, 0, None) == 0  # Gaussian again


def test_loss_node_with_and_without_view_tables_agree():
    """ElboLossFn on an NB term alone: with one view of weight 1 (what loss_fn passes) and with no view table at all"""
    _build()
    from spatial_alignment_amd import step_engine as SE

    class Holder:
        pass

    gen = torch.Generator().manual_seed(SEED + 6)
    S, N, P = 2, 50, 4
    F, Y = torch.randn(S, N, P, generator=gen).to(DEV), _counts(gen, N, P).to(DEV)
    rho = torch.randn(P, generator=gen).to(DEV)
    one = torch.ones(1, dtype=torch.float64, device=DEV)
    res = []
    for views in (dict(n_views=[1], view_off=[0, N], weights=[one]), {}):
        aux = dict(Y=[Y], noise_idx=[0], kl_scale=1.0, kinds=[2], log_offset=[None], skip=False, nobs=None, disp={0: 0}, **views)
        aux["lgam"] = SE.lgamma_sums(Holder(), aux["Y"], None, False, cacheable=False)
        Fr, rh = F.clone().requires_grad_(True), rho.clone().requires_grad_(True)
        loss = SE.ElboLossFn.apply(aux, torch.zeros(1, device=DEV), None, Fr, rh)
        loss.backward()
        res.append((loss.detach(), Fr.grad, rh.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][2].abs().min()) > 0


def test_predict_gives_log_mean_moments_and_refuses_the_count_scale():
    _build()
    name = "c10_unequal_two_fixed"
    g, Yc, off, _, _, _ = _nb_step_reference(name)
    model, dd = _nb_problem(g, Yc, off)
    X = {m: dd[m]["spatial_coords"] for m in g.mods}
    eps = [e.to(DEV) for e in g.eps_G]
    with pytest.raises(ValueError, match="negative binomial"):
        model.predict(X, Y={m: dd[m]["outputs"] for m in g.mods}, S=g.S, eps_G=eps)
    with pytest.raises(ValueError, match="negative binomial"):
        model.predict(X, S=g.S, eps_G=eps, scale="response")
    got = model.predict(X, S=g.S, eps_G=eps)
    model.likelihood = "gaussian"
    want = model.predict(X, S=g.S, eps_G=eps)
    for m in g.mods:
        assert torch.equal(got[m].F_mean, want[m].F_mean) and torch.equal(got[m].F_var, want[m].F_var)
        assert got[m].lpd is None
