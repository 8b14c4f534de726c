"""GPU: the ELBO loss node's kernels, one by one, against an fp64 restatement on the CPU - the plain, fused (some terms
arrive as partial sums of z^2) and per-view weighted ops at the edges of their grids (one element, a partial group of
four, exactly one block, a nearly empty second block, a sample boundary inside a group, the 4096-block cap and the
second grid-stride sweep behind it, GPSA_MAX_MODS terms, the strided loops of the finishing kernels), and
gpsa_elbo_fused_post over both of its branches.

Every call gets a workspace of NaN bytes and NaN-prefilled outputs (a partial that is read but was not written, or an
output that was not stored, poisons the result), dF and the three arrays of fused_post sit between NaN guards, and
sentinel elements (each worth at least 1/64 of the term's sum of z^2) stand where an off-by-one would drop them.

The bounds follow from the kernels' arithmetic (fp32 r, inv, z, z*z, four fp32 adds, then fp64), not from what the
kernels returned:
    dF          |got - want| <= 4 * 2^-24 |want|, elementwise
    ll[i]       2^-20 * 0.5 * sum(z^2) / S
    loss        the sum of the ll bounds + 2^-24 |want| (fp32 store) + n_kl 2^-52 kl_scale sum|kl|
    dnoise[j]   2^-20 * sum(z^2 + 1) |gloss| e / (s S) + 2^-24 |want|,  e = exp(noise_u), s = e + 1e-5
    fused term  nparts * 2^-52 * (the magnitudes added), + the fp32 store where there is one
    weighted    the same per view, combined as sum_v |w_v| bound_v
    dkl         kl_scale * float64(float32(gloss)) exactly
The worst error-to-bound ratio of every check is printed when the module finishes (docs/LAB_NOTES.md keeps the figures
of the run that introduced this file)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
GUARD = 64
U20, U24, U52, U53 = 2.0 ** -20, 2.0 ** -24, 2.0 ** -52, 2.0 ** -53
KL_SCALE = 0.7
GLOSS = (1.0, -0.75)
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)
RATIOS = {}


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from spatial_alignment_amd import _lib as L
    from spatial_alignment_amd import torch_ops

    return L, torch_ops


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print(f"[loss ops] worst error / bound  {k:28s} {RATIOS[k]:.3g}")


def _within(name, got, want, bound):
    """|got - want| <= bound (elementwise); the worst ratio goes to RATIOS[name] before the assertion"""
    got = torch.as_tensor(got, dtype=torch.float64).cpu().reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1).expand_as(want)
    assert not torch.isnan(got).any(), f"{name}: {int(torch.isnan(got).sum())} of {got.numel()} not written"
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # (0 / 0: an exact result within a zero bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    at = int(ratio.argmax()) if ratio.numel() else 0
    assert worst <= 1.0, f"{name}: error / bound = {worst:.3g} at {at}: got {got[at]!r}, want {want[at]!r}"


def _guarded(n, dtype=torch.float32):
    """-> (buffer, its inner n elements): NaN everywhere, GUARD elements on each side of the view a kernel gets"""
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_nan(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


# ---- the terms ------------------------------------------------------------------------------------------------------
class Term:
    """one likelihood term on the host: plain (F [S, N, P], Y [N, P]), weighted (the same + views, w) or fused (zpart).
    For the skip op: miss [N, P] marks the missing entries of Y (the device gets NaN there); a fused term carries its
    observed count as nobs"""

    def __init__(self, shape, slot, F=None, Y=None, zpart=None, views=None, w=None, sentinels=(), miss=None, nobs=None):
        self.S, self.N, self.P = shape
        self.tot = self.S * self.N * self.P
        self.slot, self.F, self.Y, self.zpart, self.views, self.w = slot, F, Y, zpart, views, w
        self.fused = zpart is not None
        self.sentinels = list(sentinels)
        self.miss, self.nobs = miss, nobs

    def view_bounds(self):
        return [0, self.N] if self.views is None else [int(x) for x in np.cumsum([0] + list(self.views))]

    def counts(self):
        """the observed entries of Y per view (a fused term: its nobs; no mask: all of them)"""
        if self.fused:
            return [float(self.N * self.P if self.nobs is None else self.nobs)]
        off = self.view_bounds()
        if self.miss is None:
            return [float((b - a) * self.P) for a, b in zip(off, off[1:])]
        return [float((~self.miss[a:b]).sum()) for a, b in zip(off, off[1:])]


def _blocks(tot):  # the grid of the plain kernels as the sentinels assume it (the checks do not depend on it)
    return min(max(-(-tot // 1024), 1), 4096)


def _std(noise, slot):
    e = math.exp(float(noise[slot]))
    return e, e + 1e-5


def _plant(F, Y, flat, s, tot):
    """the k-th distinct position carries z = (1 + k/8) sqrt(tot / 64): alone at least 1/64 of the random part's z^2"""
    NP = Y.numel()
    pos = []
    for i in flat:
        if i % tot not in pos:
            pos.append(i % tot)
    for k, i in enumerate(pos):
        F.view(-1)[i] = Y.view(-1)[i % NP] + (1 + k / 8) * s * math.sqrt(tot / 64)
    return pos


def _plain_term(shape, slot, noise, seed):
    S, N, P = shape
    gen = torch.Generator().manual_seed(seed)
    _, s = _std(noise, slot)
    Y = torch.randn(N, P, generator=gen)
    F = (Y.unsqueeze(0) + s * torch.randn(S, N, P, generator=gen)).contiguous()  # z ~ N(0, 1)
    tot, nb = S * N * P, _blocks(S * N * P)
    pos = _plant(F, Y, [0, tot - 1, 1023, 1024, nb * 1024 - 1, nb * 1024, N * P - 1, N * P], s, tot)
    return Term(shape, slot, F=F, Y=Y, sentinels=pos)


def _weighted_term(S, P, views, slot, noise, seed):
    N = sum(views)
    gen = torch.Generator().manual_seed(seed)
    _, s = _std(noise, slot)
    Y = torch.randn(N, P, generator=gen)
    F = (Y.unsqueeze(0) + s * torch.randn(S, N, P, generator=gen)).contiguous()
    w = torch.rand(len(views), generator=gen, dtype=torch.float64) * 3 + 0.5  # fp64, not fp32-representable
    assert not torch.equal(w, w.float().double())
    off = np.cumsum([0] + list(views))
    pos = []
    for v, rows in enumerate(views):  # first and last element of every non-empty view in the first and last sample
        if rows:
            lo, hi, last = int(off[v]) * P, int(off[v + 1]) * P - 1, (S - 1) * N * P
            pos += _plant(F, Y, [lo, hi, last + lo, last + hi], s, S * N * P)
    return Term((S, N, P), slot, F=F, Y=Y, views=list(views), w=w, sentinels=pos)


def _fused_term(shape, slot, nparts, seed, nobs=None, w=None):
    gen = torch.Generator().manual_seed(seed)
    zpart = torch.exp(torch.rand(nparts, generator=gen, dtype=torch.float64) * 30 - 20)  # positive, a wide spread
    return Term(shape, slot, zpart=zpart, Y=torch.zeros(shape[1], shape[2]), nobs=nobs, w=w,
                views=None if w is None else [shape[1]])


def _masked(t, seed, dead_views=()):
    """t with 30 % of its entries missing - never a sentinel - and every entry of the ``dead_views``, sentinels included"""
    gen = torch.Generator().manual_seed(seed)
    NP = t.N * t.P
    miss = torch.rand(t.N, t.P, generator=gen) < 0.3
    miss.view(-1)[[i % NP for i in t.sentinels]] = False
    off = t.view_bounds()
    for v in dead_views:
        miss[off[v]:off[v + 1]] = True
    t.sentinels = [i for i in t.sentinels if not bool(miss.view(-1)[i % NP])]
    t.miss = miss
    return t


# ---- fp64 reference -------------------------------------------------------------------------------------------------
class Ref:
    pass


def _reference(terms, noise, kl, glosses=GLOSS):
    """plain fp64 restatement from the same fp32 inputs; gradients from autograd, one backward per upstream gradient.
    groups[i]: (|weight|, sum z^2, elements) per view of term i (one group for an unweighted term)"""
    r = Ref()
    nz = noise.double().requires_grad_()
    k64 = None if kl is None else kl.clone().requires_grad_()
    F64, lls, r.groups = [], [], []
    for t in terms:
        s = torch.exp(nz[t.slot]) + 1e-5
        cst = -torch.log(s) - HALF_LOG_2PI
        if t.fused:
            z2 = math.fsum(t.zpart.tolist())
            tot = t.S * t.counts()[0]  # (S N P, or S nobs under the skip op)
            w0 = 1.0 if t.w is None else float(t.w[0])
            # (sum z^2 = Q / s^2 with Q fixed: d ll / d s = (z2 - tot) / s / S)
            lls.append(w0 * (-0.5 * z2 * (s.detach() / s) ** 2 + cst * tot) / t.S)
            F64.append(None)
            r.groups.append([(w0, z2, tot)])
            continue
        F = t.F.double().requires_grad_()
        F64.append(F)
        if t.miss is None:
            z = (t.Y.double() - F) / s
            lp = -0.5 * z ** 2 + cst
        else:  # the observed entries only (the others' Y is NaN on the device: a zero stands in here)
            obs = (~t.miss).double()
            z = (torch.where(t.miss, torch.zeros_like(t.Y), t.Y).double() - F) / s * obs
            lp = (-0.5 * z ** 2 + cst) * obs
        z2_row = (z.detach() ** 2).sum((0, 2))
        if t.views is None:
            lls.append(lp.sum() / t.S)
            r.groups.append([(1.0, float(z2_row.sum()), t.S * t.counts()[0])])
        else:
            per_row = lp.sum((0, 2)) / t.S
            off, cnt = t.view_bounds(), t.counts()
            w = torch.ones(len(t.views), dtype=torch.float64) if t.w is None else t.w
            lls.append(sum(w[v] * per_row[off[v]:off[v + 1]].sum() for v in range(len(t.views))))
            r.groups.append([(float(w[v]), float(z2_row[off[v]:off[v + 1]].sum()), t.S * cnt[v])
                             for v in range(len(t.views))])
    loss = -sum(lls) if k64 is None else KL_SCALE * k64.sum() - sum(lls)
    r.loss, r.ll = float(loss.detach()), [float(x.detach()) for x in lls]
    r.kl_abs = 0.0 if kl is None else float(kl.abs().sum())
    r.n_kl = 0 if kl is None else kl.numel()
    r.dF, r.dnoise = {}, {}
    for g in glosses:
        for leaf in F64 + [nz]:
            if leaf is not None:
                leaf.grad = None
        loss.backward(torch.tensor(g, dtype=torch.float64), retain_graph=True)
        r.dF[g] = [None if f is None else f.grad.clone() for f in F64]
        r.dnoise[g] = nz.grad.clone()
    return r


def _ll_bound(t, groups, noise):
    if t.fused:
        _, s = _std(noise, t.slot)
        (w, z2, tot), = groups
        return abs(w) * t.zpart.numel() * U52 * (0.5 * z2 + abs(-math.log(s) - HALF_LOG_2PI) * tot) / t.S
    return sum(abs(w) * U20 * 0.5 * z2 / t.S for w, z2, _ in groups)


def _dnoise_bound(t, groups, noise, g, want):
    e, s = _std(noise, t.slot)
    unit = t.zpart.numel() * U52 if t.fused else U20
    return sum(abs(w) * unit * (z2 + tot) for w, z2, tot in groups) * abs(g) * e / (s * t.S) + U24 * abs(want)


def _sentinels_bite(t, groups, noise):
    """on the CPU, with the reference alone: what one sentinel adds to ll and to dnoise, over the bound of that check.
    -> the smallest ratio over the term's sentinels: against the term's whole bound, against its own view's share"""
    e, s = _std(noise, t.slot)
    z2 = ((t.Y.double().reshape(-1)[[i % (t.N * t.P) for i in t.sentinels]]
           - t.F.double().reshape(-1)[t.sentinels]) / s) ** 2
    whole = sum(abs(w) * U20 * 0.5 * q for w, q, _ in groups)
    whole_dn = sum(abs(w) * (U20 + U24) * (q + n) for w, q, n in groups)  # (|want| <= sum |w| (z2 + tot) ...)
    if t.views is None:
        return float((0.5 * z2 / whole).min()), float((z2 / whole_dn).min()), None
    off = np.cumsum([0] + t.views) * t.P
    worst_whole, worst_dn, worst_own = math.inf, math.inf, math.inf
    for i, q in zip(t.sentinels, z2.tolist()):
        v = int(np.searchsorted(off, i % (t.N * t.P), side="right")) - 1
        w, qv, _ = groups[v]
        worst_whole = min(worst_whole, abs(w) * 0.5 * q / whole)
        worst_dn = min(worst_dn, abs(w) * q / whole_dn)
        worst_own = min(worst_own, 0.5 * q / (U20 * 0.5 * qv))
    return worst_whole, worst_dn, worst_own


# ---- the device side ------------------------------------------------------------------------------------------------
class Out:
    pass


def _device(op, terms, noise, kl, gloss, with_dkl=True, n_kl=None):
    """forward and backward of one op ("plain", "fused", "weighted", "skip") with poisoned workspace and outputs -> Out
    (CPU).  "skip": NaN at the terms' missing entries, the counts as device doubles; the view and weight tables go along
    when the first term has them (then every term does), the fused tables when a term is fused"""
    _, T = _lib()
    n = len(terms)
    d = lambda t: t.to(DEV).contiguous()
    Fd = [d(t.zpart if t.fused else t.F) for t in terms]
    Yd = [d(t.Y if t.miss is None else torch.where(t.miss, torch.full_like(t.Y, NAN), t.Y)) for t in terms]
    nd = d(noise)
    kd = None if kl is None else d(kl)
    idx = [t.slot for t in terms]
    shapes = [x for t in terms for x in (t.S, t.N, t.P)]
    fused = [int(t.fused) for t in terms]
    ws = torch.full((T.loss_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), NAN, device=DEV)
    ll = torch.full((n,), NAN, dtype=torch.float64, device=DEV)
    bufs, dFs = [], []
    for t in terms:
        b, v = _guarded(8 if t.fused else t.tot)
        bufs.append(b)
        dFs.append(v if t.fused else v.view(t.S, t.N, t.P))
    dnoise = torch.full((noise.numel(),), NAN, device=DEV)
    n_kl = (0 if kl is None else kl.numel()) if n_kl is None else n_kl
    dkl = torch.full((n_kl,), NAN, dtype=torch.float64, device=DEV) if with_dkl else None
    gl = torch.tensor([gloss], dtype=torch.float32, device=DEV)
    o = Out()
    nv, off, wd = [], [], []
    if op == "weighted" or (op == "skip" and terms[0].views is not None):
        nv = [len(t.views) for t in terms]
        off = [x for t in terms for x in t.view_bounds()]
        wd = [d(t.w) for t in terms] if terms[0].w is not None else []
    if op == "skip":
        tabs = (shapes, fused) if any(fused) else ([], [])
        tabs += (nv, off, wd, [torch.tensor(t.counts(), dtype=torch.float64, device=DEV) for t in terms])
    if op == "plain":
        torch.ops.gpsa.elbo_loss_fwd(Fd, Yd, nd, idx, kd, KL_SCALE, loss, ll, ws)
    elif op == "fused":
        torch.ops.gpsa.elbo_loss_fused_fwd(Fd, Yd, nd, idx, shapes, fused, kd, KL_SCALE, loss, ll, ws)
    elif op == "weighted":
        torch.ops.gpsa.elbo_loss_weighted_fwd(Fd, Yd, nd, idx, nv, off, wd, kd, KL_SCALE, loss, ll, ws)
    else:
        torch.ops.gpsa.elbo_loss_skip_fwd(Fd, Yd, nd, idx, *tabs, kd, KL_SCALE, loss, ll, ws)
    ws.fill_(0xFF)
    if op == "plain":
        torch.ops.gpsa.elbo_loss_bwd(Fd, Yd, nd, idx, gl, n_kl, KL_SCALE, dFs, dnoise, dkl, ws)
    elif op == "fused":
        torch.ops.gpsa.elbo_loss_fused_bwd(Fd, Yd, nd, idx, shapes, fused, gl, n_kl, KL_SCALE, dFs, dnoise, dkl, ws)
    elif op == "weighted":
        torch.ops.gpsa.elbo_loss_weighted_bwd(Fd, Yd, nd, idx, nv, off, wd, gl, n_kl, KL_SCALE, dFs, dnoise, dkl, ws)
    else:
        torch.ops.gpsa.elbo_loss_skip_bwd(Fd, Yd, nd, idx, *tabs, gl, n_kl, KL_SCALE, dFs, dnoise, dkl, ws)
    torch.cuda.synchronize()
    o.loss, o.ll, o.dnoise = float(loss), ll.cpu(), dnoise.cpu()
    o.dkl = None if dkl is None else dkl.cpu()
    o.dF = [v.cpu() for v in dFs]
    o.guards = [_guards_nan(b) for b in bufs]
    return o


def _check(tag, terms, noise, kl, ref, out, g):
    """every output of one call against the reference, within the bounds of the module docstring"""
    bounds = [_ll_bound(t, gr, noise) for t, gr in zip(terms, ref.groups)]
    for i, t in enumerate(terms):
        _within(f"{tag} ll" + (" (fused term)" if t.fused else ""), out.ll[i], ref.ll[i], bounds[i])
    _within(f"{tag} loss", out.loss, ref.loss,
            sum(bounds) + U24 * abs(ref.loss) + ref.n_kl * U52 * KL_SCALE * ref.kl_abs)
    named = set()
    for i, t in enumerate(terms):
        assert out.guards[i], f"{tag}: term {i}: a guard element next to dF was written"
        if t.fused:
            assert bool(torch.isnan(out.dF[i]).all()), f"{tag}: dF of fused term {i} was touched"
        else:
            want = ref.dF[g][i]
            _within(f"{tag} dF", out.dF[i], want, 4 * U24 * want.abs())
            if t.miss is not None:  # exactly +-0 at a missing entry
                assert bool((out.dF[i][:, t.miss] == 0).all()), f"{tag}: term {i}: dF at a missing entry"
        want = float(ref.dnoise[g][t.slot])
        _within(f"{tag} dnoise" + (" (fused term)" if t.fused else ""), out.dnoise[t.slot], want,
                _dnoise_bound(t, ref.groups[i], noise, g, want))
        named.add(t.slot)
    for j in range(noise.numel()):
        if j not in named:  # (bit pattern of +0.0: not NaN, not -0.0)
            assert out.dnoise[j:j + 1].view(torch.int32).item() == 0, f"{tag}: dnoise[{j}] = {out.dnoise[j]!r}"
    if out.dkl is not None:
        want = KL_SCALE * float(np.float64(np.float32(g)))
        assert out.dkl.numel() == 0 or bool((out.dkl == want).all()), f"{tag}: dkl {out.dkl[:4]} != {want!r}"


def _noise(n_terms):  # two more entries than there are terms
    return torch.tensor([0.3, -0.2, 0.1, -0.4, 0.25, -0.15][: n_terms + 2])


def _kl(n, seed=11):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)  # mixed signs


# ---- plain op -------------------------------------------------------------------------------------------------------
ONE_TERM = [(1, 1, 1), (2, 50, 4), (2, 512, 1), (1, 1025, 1), (3, 333, 7), (1, 4099, 1025)]
FOUR_TERMS = [(2, 50, 4), (1, 1025, 1), (3, 333, 7), (2, 512, 1)]


@pytest.mark.parametrize("shape", ONE_TERM, ids=lambda s: "x".join(map(str, s)))
def test_one_term(shape):
    noise, kl = _noise(1), _kl(7)
    terms = [_plain_term(shape, 1, noise, seed=5)]
    ref = _reference(terms, noise, kl)
    bite_ll, bite_dn, _ = _sentinels_bite(terms[0], ref.groups[0], noise)
    assert bite_ll > 1000 and bite_dn > 1000, (bite_ll, bite_dn)
    for g in GLOSS:
        _check("plain", terms, noise, kl, ref, _device("plain", terms, noise, kl, g), g)


def test_four_terms():
    noise, kl = _noise(4), _kl(7)
    terms = [_plain_term(s, j, noise, seed=20 + j) for s, j in zip(FOUR_TERMS, [3, 0, 5, 2])]
    ref = _reference(terms, noise, kl)
    for t, gr in zip(terms, ref.groups):
        bite_ll, bite_dn, _ = _sentinels_bite(t, gr, noise)
        assert bite_ll > 1000 and bite_dn > 1000, (bite_ll, bite_dn)
    for g in GLOSS:
        _check("plain", terms, noise, kl, ref, _device("plain", terms, noise, kl, g), g)


@pytest.mark.parametrize("n_kl", [1, 256, 257, 1000])
def test_kl_sizes(n_kl):
    noise, kl = _noise(1), _kl(n_kl)
    terms = [_plain_term((2, 50, 4), 0, noise, seed=6)]
    ref = _reference(terms, noise, kl)
    for g in GLOSS:
        out = _device("plain", terms, noise, kl, g)
        assert out.dkl.numel() == n_kl
        _check("plain", terms, noise, kl, ref, out, g)


def test_without_kl():
    """kl = None: loss = -sum(ll);  dkl = None: the backward runs and everything else is what it was with a dkl"""
    noise = _noise(2)
    terms = [_plain_term((3, 333, 7), 2, noise, seed=7), _plain_term((2, 50, 4), 0, noise, seed=8)]
    ref = _reference(terms, noise, None)
    for g in GLOSS:
        out = _device("plain", terms, noise, None, g, with_dkl=False, n_kl=7)
        _check("plain", terms, noise, None, ref, out, g)
        assert out.loss == float(np.float32(-math.fsum(out.ll.tolist())))
        kept = _device("plain", terms, noise, _kl(7), g)
        assert torch.equal(out.dnoise, kept.dnoise) and all(torch.equal(a, b) for a, b in zip(out.dF, kept.dF))


def test_five_terms_are_refused():
    """one term more than GPSA_MAX_MODS: refused before any launch, forward and backward; every output keeps its NaN"""
    L, T = _lib()
    noise = torch.tensor([0.3, -0.2, 0.1, -0.4, 0.25, -0.15, 0.05])
    terms = [_plain_term((2, 50, 4), j, noise, seed=30 + j) for j in range(5)]
    d = lambda t: t.to(DEV).contiguous()
    Fd, Yd, nd, kd = [d(t.F) for t in terms], [d(t.Y) for t in terms], d(noise), d(_kl(7))
    idx = [t.slot for t in terms]
    ws = torch.full((T.loss_workspace_bytes(5),), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), NAN, device=DEV)
    ll = torch.full((5,), NAN, dtype=torch.float64, device=DEV)
    bufs = [_guarded(t.tot)[0] for t in terms]
    dFs = [b[GUARD:-GUARD].view(t.S, t.N, t.P) for b, t in zip(bufs, terms)]
    dnoise = torch.full((7,), NAN, device=DEV)
    dkl = torch.full((7,), NAN, dtype=torch.float64, device=DEV)
    with pytest.raises(L.GpsaHipError, match="invalid argument"):
        torch.ops.gpsa.elbo_loss_fwd(Fd, Yd, nd, idx, kd, KL_SCALE, loss, ll, ws)
    with pytest.raises(L.GpsaHipError, match="invalid argument"):
        torch.ops.gpsa.elbo_loss_bwd(Fd, Yd, nd, idx, torch.ones(1, device=DEV), 7, KL_SCALE, dFs, dnoise, dkl, ws)
    torch.cuda.synchronize()
    for x in [loss, ll, dnoise, dkl] + bufs:
        assert bool(torch.isnan(x).all())
    assert bool((ws == 0xFF).all())


# ---- fused and plain terms mixed ------------------------------------------------------------------------------------
MIXED = [(2, 50, 4), (1, 1025, 1), (3, 333, 7)]
MIXED_SLOTS = [3, 0, 2]


def _mixed_terms(pattern, nparts, noise):
    return [_fused_term(s, j, nparts, seed=40 + i) if z else _plain_term(s, j, noise, seed=40 + i)
            for i, (s, j, z) in enumerate(zip(MIXED, MIXED_SLOTS, pattern))]


def _nparts(which):
    L, _ = _lib()
    return int(L.load().gpsa_quadform_elbo_parts()) if which == "elbo_parts" else which


@pytest.fixture(scope="module")
def all_plain():
    """the three mixed-case terms, all plain, through the plain op: what a plain term gives whatever its neighbours"""
    noise, kl = _noise(3), _kl(7)
    terms = _mixed_terms([0, 0, 0], 1, noise)
    return {g: _device("plain", terms, noise, kl, g) for g in GLOSS}


@pytest.mark.parametrize("nparts", [1, 255, 257, "elbo_parts"])
@pytest.mark.parametrize("pattern", [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], ids=lambda p: "".join(map(str, p)))
def test_fused_and_plain_terms(pattern, nparts, all_plain):
    """in every pattern: the unnamed noise gradients are exactly zero, dkl is written, dF of a fused term is not
    touched, dF of a plain term is complete (_check); and a plain term's ll, dF and dnoise are bit-equal to what it gives
    between plain neighbours - its launch and its workspace slot do not depend on them"""
    noise, kl = _noise(3), _kl(7)
    terms = _mixed_terms(pattern, _nparts(nparts), noise)
    ref = _reference(terms, noise, kl)
    for g in GLOSS:
        out = _device("fused", terms, noise, kl, g)
        _check("fused op", terms, noise, kl, ref, out, g)
        assert out.dkl.numel() == 7
        base = all_plain[g]
        for i, t in enumerate(terms):
            if not t.fused:
                assert out.ll[i].view(torch.int64) == base.ll[i].view(torch.int64)
                assert torch.equal(out.dF[i], base.dF[i])
                assert torch.equal(out.dnoise[t.slot].view(torch.int32), base.dnoise[t.slot].view(torch.int32))


def test_fused_op_without_a_fused_term_is_the_plain_op(all_plain):
    noise, kl = _noise(3), _kl(7)
    terms = _mixed_terms([0, 0, 0], 1, noise)
    for g in GLOSS:
        out, base = _device("fused", terms, noise, kl, g), all_plain[g]
        assert out.loss == base.loss and torch.equal(out.ll, base.ll) and torch.equal(out.dnoise, base.dnoise)
        assert all(torch.equal(a, b) for a, b in zip(out.dF, base.dF)) and torch.equal(out.dkl, base.dkl)


# ---- weighted op ----------------------------------------------------------------------------------------------------
UNEQUAL = (2, 3, [1, 1500, 20])  # S, P, views: nb = 9, blocks 1 .. 8 of the two short views write zero partials
MANY = (3, 33, [0] + [i * 7 % 5 + 1 for i in range(30)] + [0] + [700] + [i * 3 % 5 + 1 for i in range(31)])
# (64 views, two of them empty; the 700-row view has 69 300 elements against 4096 / 64 = 64 blocks: a second sweep)
FEW_CAPPED = (1, 1025, [5, 1400, 7])  # 1 435 000 elements in one view against 4096 / 3 = 1365 blocks


def _check_weighted(terms, noise, kl):
    ref = _reference(terms, noise, kl)
    for t, gr in zip(terms, ref.groups):
        whole, whole_dn, own = _sentinels_bite(t, gr, noise)
        # a sentinel outweighs its own view's share of the bound by more than 1000, and the combined bound (the
        # other views' sentinels and weights up to 7 times its own are in there) by more than 100
        assert own > 1000 and whole > 100 and whole_dn > 100, (own, whole, whole_dn)
    for g in GLOSS:
        _check("weighted", terms, noise, kl, ref, _device("weighted", terms, noise, kl, g), g)


@pytest.mark.parametrize("case", [UNEQUAL, MANY, FEW_CAPPED], ids=["unequal", "many", "few_capped"])
def test_weighted_one_term(case):
    S, P, views = case
    assert len(MANY[2]) == 64 and MANY[2][0] == 0 and MANY[2][31] == 0
    noise = _noise(1)
    _check_weighted([_weighted_term(S, P, views, 1, noise, seed=50)], noise, _kl(7))


def test_weighted_two_terms():
    noise = _noise(2)
    terms = [_weighted_term(3, 4, [20, 30], 3, noise, seed=51), _weighted_term(*MANY, 0, noise, seed=52)]
    _check_weighted(terms, noise, _kl(7))


def _bad_second_term(kind, noise):
    t = _weighted_term(2, 3, [10, 25, 35], 0, noise, seed=54)
    t.off = [int(x) for x in np.cumsum([0] + t.views)]
    if kind == "no views":
        t.views, t.w, t.off = [], torch.ones(1, dtype=torch.float64), [0]
    elif kind == "65 views":
        t.views, t.w = [1] * 65, torch.ones(65, dtype=torch.float64)
        t.off = list(range(65)) + [t.N]
    elif kind == "off[0] != 0":
        t.off[0] = 1
    elif kind == "off[V] != N":
        t.off[-1] -= 1
    elif kind == "decreasing":
        t.off[1], t.off[2] = t.off[2], t.off[1]
    elif kind == "no weights":
        t.w = torch.empty(0, dtype=torch.float64)  # (its data pointer is NULL)
    return t


@pytest.mark.parametrize("kind", ["no views", "65 views", "off[0] != 0", "off[V] != N", "decreasing", "no weights"])
def test_weighted_refusals(kind):
    """a bad SECOND term is refused before the first term's kernels run: every output keeps its NaN, dF[0] included"""
    noise = _noise(2)
    good = _weighted_term(3, 4, [20, 30], 2, noise, seed=53)
    good.off = [0, 20, 50]
    bad = _bad_second_term(kind, noise)
    L, T = _lib()
    d = lambda t: t.to(DEV).contiguous()
    terms = [good, bad]
    Fd, Yd, nd, kd = [d(t.F) for t in terms], [d(t.Y) for t in terms], d(noise), d(_kl(7))
    wd = [d(t.w) for t in terms]
    if kind == "no weights":
        assert wd[1].data_ptr() == 0
    idx, nv, off = [t.slot for t in terms], [len(t.views) for t in terms], good.off + bad.off
    ws = torch.full((T.loss_workspace_bytes(2),), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), NAN, device=DEV)
    ll = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
    bufs = [_guarded(t.tot)[0] for t in terms]
    dFs = [b[GUARD:-GUARD].view(t.S, t.N, t.P) for b, t in zip(bufs, terms)]
    dnoise = torch.full((4,), NAN, device=DEV)
    dkl = torch.full((7,), NAN, dtype=torch.float64, device=DEV)
    with pytest.raises(L.GpsaHipError, match="invalid argument"):
        torch.ops.gpsa.elbo_loss_weighted_fwd(Fd, Yd, nd, idx, nv, off, wd, kd, KL_SCALE, loss, ll, ws)
    with pytest.raises(L.GpsaHipError, match="invalid argument"):
        torch.ops.gpsa.elbo_loss_weighted_bwd(Fd, Yd, nd, idx, nv, off, wd, torch.ones(1, device=DEV), 7, KL_SCALE, dFs,
                                              dnoise, dkl, ws)
    torch.cuda.synchronize()
    for name, x in [("loss", loss), ("ll", ll), ("dF[0]", bufs[0]), ("dF[1]", bufs[1]), ("dnoise", dnoise),
                    ("dkl", dkl)]:
        assert bool(torch.isnan(x).all()), f"{kind}: {name} was written by a refused call"
    assert bool((ws == 0xFF).all()), f"{kind}: the workspace was written by a refused call"


# ---- the view table's edges, for both per-view op pairs (weighted, skip) ---------------------------------------------
ONE_VIEW = (2, 3, [37])  # V = 1
EDGE_EMPTY = (3, 5, [0, 0] + [i * 5 % 4 + 1 for i in range(38)] + [0] + [i * 3 % 4 + 1 for i in range(22)] + [0])
# (64 views, four of them empty: the first two, one inside and the last)
CAP_BINDS = (2, 64, [i % 3 + 1 for i in range(20)] + [600] + [i % 3 + 1 for i in range(43)])
# (64 views of 1-3 rows and one of 600: 76 800 elements against 4096 / 64 = 64 blocks of 1024, a second sweep)
VIEW_EDGES = {"one_view": ONE_VIEW, "empty_views": EDGE_EMPTY, "cap_binds": CAP_BINDS}


def test_view_edge_cases_are_what_they_say():
    for S, P, views in (EDGE_EMPTY, CAP_BINDS):
        assert len(views) == 64
    v = EDGE_EMPTY[2]
    assert v[0] == 0 and v[1] == 0 and v[40] == 0 and v[63] == 0 and sum(x == 0 for x in v) == 4
    S, P, views = CAP_BINDS
    assert max(views) == 600 and S * P * 600 == 76800 > 64 * 1024 and sorted(set(views) - {600}) == [1, 2, 3]


@pytest.mark.parametrize("case", sorted(VIEW_EDGES))
@pytest.mark.parametrize("op", ["weighted", "skip"])
def test_view_table_edges(op, case):
    S, P, views = VIEW_EDGES[case]
    noise = _noise(1)
    t = _weighted_term(S, P, views, 1, noise, seed=60)
    if op == "skip":
        t = _masked(t, seed=61)
    ref = _reference([t], noise, _kl(7))
    whole, whole_dn, own = _sentinels_bite(t, ref.groups[0], noise)
    assert own > 1000 and whole > 100 and whole_dn > 100, (own, whole, whole_dn)  # (as _check_weighted)
    for g in GLOSS:
        _check(op, [t], noise, _kl(7), ref, _device(op, [t], noise, _kl(7), g), g)


def test_skip_one_view_without_tables():
    """the skip op without a view table and without weights: the term is one view of its N rows"""
    noise = _noise(1)
    t = _masked(_plain_term((3, 333, 7), 1, noise, seed=62), seed=63)
    ref = _reference([t], noise, _kl(7))
    bite_ll, bite_dn, _ = _sentinels_bite(t, ref.groups[0], noise)
    assert bite_ll > 1000 and bite_dn > 1000, (bite_ll, bite_dn)
    for g in GLOSS:
        _check("skip", [t], noise, _kl(7), ref, _device("skip", [t], noise, _kl(7), g), g)


@pytest.mark.parametrize("nparts", [1, 257])
def test_skip_fused_term_then_draws_term(nparts):
    """two terms in one skip call: term 0 arrives as partial sums (one view, its own weight and count), term 1 comes from
    its draws into the SECOND workspace slot, with one view that has no observed entry and one that is empty.  The
    zero-fill of the noise gradient and dkl ride on the first (fused) term's finishing launch: the unnamed noise
    gradients are +0.0, dkl is written, the fused term's dF is not touched (_check)"""
    noise = _noise(2)
    w0 = torch.tensor([1.7], dtype=torch.float64) / 3
    fused = _fused_term((2, 50, 4), 3, nparts, seed=64, nobs=271.0, w=w0)
    draws = _masked(_weighted_term(3, 7, [20, 1500, 0, 33], 0, noise, seed=65), seed=66, dead_views=[0])
    assert draws.counts()[0] == 0.0 and draws.counts()[2] == 0.0 and draws.counts()[1] > 0 and draws.counts()[3] > 0
    terms = [fused, draws]
    ref = _reference(terms, noise, _kl(7))
    whole, whole_dn, own = _sentinels_bite(draws, ref.groups[1], noise)
    assert own > 1000 and whole > 100 and whole_dn > 100, (own, whole, whole_dn)
    for g in GLOSS:
        out = _device("skip", terms, noise, _kl(7), g)
        _check("skip", terms, noise, _kl(7), ref, out, g)
        assert out.dkl.numel() == 7
        alone = _device("skip", [draws], noise, _kl(7), g)  # the draws term's launch and slot do not depend on slot 0
        assert out.ll[1].view(torch.int64) == alone.ll[0].view(torch.int64) and torch.equal(out.dF[1], alone.dF[0])
        assert torch.equal(out.dnoise[0].view(torch.int32), alone.dnoise[0].view(torch.int32))


# ---- gpsa_elbo_fused_post -------------------------------------------------------------------------------------------
F32, F64 = 0, 1 # GPSA_F32, GPSA_F64 (include/gpsa_hip.h)
EINVAL, EWORKSPACE = -1, -2
VAR_U = 0.3


class Post:
    """the arguments of one gpsa_elbo_fused_post call: g_ext [L + 1, C] (row L: qbar, NaN), dmeanT [L, C], abar [M, C]
    between NaN guards, dvar_u and the workspace poisoned"""

    def __init__(self, C_, L_, M, gl, dt, seed=0):
        gen = torch.Generator().manual_seed(seed)
        self.C, self.L, self.M, self.gl, self.dt = C_, L_, M, gl, dt
        self.g0 = torch.randn(L_, C_, generator=gen)
        self.dm0 = torch.randn(L_, C_, generator=gen)
        self.ab0 = torch.randn(M, C_, generator=gen)
        self.gbuf, self.g = _guarded((L_ + 1) * C_)
        self.dmbuf, self.dm = _guarded(L_ * C_)
        self.abbuf, self.ab = _guarded(M * C_)
        self.g[: L_ * C_] = self.g0.reshape(-1).to(DEV)
        self.dm[:] = self.dm0.reshape(-1).to(DEV)
        self.ab[:] = self.ab0.reshape(-1).to(DEV)
        self.gloss = torch.tensor([gl], dtype=torch.float32, device=DEV)
        self.var_u = torch.tensor([VAR_U], dtype=torch.float32, device=DEV)
        self.dvar = torch.full((1,), NAN, dtype=torch.float64 if dt == F64 else torch.float32, device=DEV)
        self.ws = torch.full((8 * -(-C_ // 256),), 0xFF, dtype=torch.uint8, device=DEV)

    def call(self, **over):
        L, _ = _lib()
        a = dict(g=self.g.data_ptr(), dm=self.dm.data_ptr(), ab=self.ab.data_ptr(), M=self.M, C=self.C, L=self.L,
                 gloss=self.gloss.data_ptr(), var_u=self.var_u.data_ptr(), dt=self.dt, dvar=self.dvar.data_ptr(),
                 ws=self.ws.data_ptr(), wsb=self.ws.numel())
        a.update(over)
        rc = L.load().gpsa_elbo_fused_post(a["g"], a["dm"], a["ab"], a["M"], a["C"], a["L"], a["gloss"], a["var_u"],
                                           a["dt"], a["dvar"], a["ws"], a["wsb"], None)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        n = self.L * self.C
        return (torch.equal(self.g[:n].cpu(), self.g0.reshape(-1)) and torch.equal(self.dm.cpu(), self.dm0.reshape(-1))
                and torch.equal(self.ab.cpu(), self.ab0.reshape(-1)) and bool(torch.isnan(self.g[n:]).all())
                and bool(torch.isnan(self.dvar).all()) and bool((self.ws == 0xFF).all()))

    def check(self):
        L_, C_ = self.L, self.C
        assert self.call() == 0
        assert _guards_nan(self.gbuf) and _guards_nan(self.dmbuf) and _guards_nan(self.abbuf), "a guard was written"
        g, dm, ab = self.g[: L_ * C_].cpu().view(L_, C_), self.dm.cpu().view(L_, C_), self.ab.cpu().view(self.M, C_)
        if self.gl == 1.0:  # rows 0 .. L - 1 of g_ext, dmeanT and abar are bit-unchanged
            want = (self.g0, self.dm0, self.ab0)
        else:  # ... or the fp32 product x * float32(gl), bit for bit
            f = torch.tensor(self.gl, dtype=torch.float32)
            want = (self.g0 * f, self.dm0 * f, self.ab0 * f)
        for name, a, b in zip(("g_ext", "dmeanT", "abar"), (g, dm, ab), want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, self.C, self.L, self.M, self.gl)
        v = want[0].double()
        mag = v.abs().sum(0)
        qbar = self.g[L_ * C_:].cpu()
        _within("fused_post qbar", qbar, -v.sum(0), (L_ + 1) * U24 * mag)
        e = math.exp(float(np.float32(VAR_U)))
        dvar = e * float(v.sum())
        _within("fused_post dvar_u", self.dvar, dvar,
                (L_ + 1) * U24 * e * float(mag.sum()) + (U53 if self.dt == F64 else U24) * abs(dvar))


@pytest.mark.parametrize("gl", [1.0, 0.37, -2.0])
@pytest.mark.parametrize("C_", [1, 255, 256, 257, 1000])
def test_fused_post(C_, gl):
    for L_ in (1, 9, 10, 11, 25):  # the gl == 1 branch unrolls by ten: no trip and a tail, one trip, trips and a tail
        for M in (1, 16):
            for dt in (F32, F64):
                Post(C_, L_, M, gl, dt, seed=L_).check()


@pytest.mark.parametrize("gl", [1.0, 0.37, -2.0])
def test_fused_post_many_blocks(gl):
    for dt in (F32, F64):  # 274 blocks: the finishing kernel's strided sum takes a second trip
        Post(70001, 11, 16, gl, dt).check()


def test_fused_post_refusals():
    """none of these launches: the arrays, qbar's row, dvar_u and the workspace are what they were"""
    for C_ in (256, 257, 1000):
        p = Post(C_, 11, 16, 0.37, F64)
        assert p.call(wsb=8 * -(-C_ // 256) - 8) == EWORKSPACE and p.untouched()
    p = Post(257, 11, 16, 0.37, F64)
    for over in [dict(M=0), dict(C=0), dict(L=0), dict(g=None), dict(dm=None), dict(ab=None), dict(gloss=None),
                 dict(var_u=None), dict(dvar=None), dict(dt=7)]:
        assert p.call(**over) == EINVAL and p.untouched(), over
