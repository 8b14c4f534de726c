"""Helpers shared by tests/test_fused_elbo_gpu.py, tests/test_lmc_lik_gpu.py and tests/test_fused_lik_shapes.py (DESIGN.md
section 2g): the fp64 references and derived bounds of the fused ELBO kernels (csrc/qf_elbo_body.hpp: panel_elbo_kernel,
_skip_, _pois_, _nb_) and of the fused LMC likelihood kernels (csrc/lmc_body.hpp: lmc_mfma_kernel, _skip_, _pois_, _nb_),
their input families with the named edge indices, and a Python restatement of the launch arithmetic for 256 compute units
(csrc/qf_common.hpp: GPSA_ELBO_SHAPES, elbo_wgs_per_cu; csrc/quadform.hip: elbo_ws, elbo_launch; csrc/lmc.hip: the
instantiations; csrc/elementwise.hip: lmc_blocks) - kept here so that the shape test without a GPU and the GPU tests cannot
drift apart.  Frame, poisoned, ratio, same_bits, mb_for, item_ranges, tile_order, range_kind, last_tile_rl and
has_padding_row are contraction_util's; its NCT, width and wgs_per_cu are the panel kernels', not these.

Roundings (derived, never measured).  u = 2^-24; an fp32 add, multiply or fma rounds once: u |result|; sqrtf and the fp32
division are taken within 1 ulp (2u relative), expf and log1pf within 2 ulp (4u relative) - section 2c's assumption, extended
to log1pf; bar(K, S) = 2 (K + 4) u S is section 2b's bound of a K-term fp32 sum of products with absolute sum S.  Every
closing below is written once, operation by operation as the kernels evaluate it, and carries an input error E_in of the
draw through: the fused ELBO tests apply it to the FT the device returned (E_in = 0: the closing alone is tested, a few
ulp), the LMC tests to the fp64 product F W with E_in = bar(L, |F| |W|) (no intermediate is returned there).

  Gaussian   r = y - F; d = coef r; z = r inv; term z^2        coef = fp32(-1 / (s^2 S)), inv = fp32(1 / s), s = exp(noise_u) + 1e-5
  Poisson    eta = F + off; ex = expf(eta); d = coef (ex - y); term = fma(y, eta, -ex)          coef = fp32(1 / S)
  NB         a = (F + off) - rho; r = expf(rho); e = expf(-|a|); sp = max(a, 0) + log1pf(e); sg = (a >= 0 ? 1 : e) / (1 + e)
             yr = y + r; dd = fma(yr, sg, -y); d = coef dd; term = fma(y, a, -(yr sp)); u = fma(-r, sp, dd)
"""
import functools
import math

import numpy as np
import torch

import contraction_util as cu
from contraction_util import (CUS, EUNSUPPORTED, EWORKSPACE, Frame, U32, bar, cdiv, f32, f64, has_padding_row,  # noqa: F401
                              item_ranges, last_tile_rl, mb_for, poisoned, range_kind, ratio, same_bits, tile_order, visible)

U = U32
U64 = 2.0 ** -53
NAN = float("nan")
SENTINEL = 1e30  # what surrounds Y where a NaN means "missing": an out-of-range load damages the result instead of vanishing
GAUSS, SKIP, POIS, NB = "gauss", "skip", "pois", "nb"
LIKS = (GAUSS, SKIP, POIS, NB)
ETA_MAX = 20.0  # every test asserts |eta|, |a| <= 20 from its reference


# ---- the launchers, restated ---------------------------------------------------------------------------------------------
ELBO_CLASSES = (2, 4, 7, 13, 16)
ELBO_NCT = {2: 4, 4: 4, 7: 4, 13: 2, 16: 2}  # GPSA_ELBO_SHAPES


def elbo_nct_for(MB):
    return ELBO_NCT[MB]


def elbo_width(MB):
    """columns of one workgroup's tile: four waves of NCT column tiles of 16"""
    return 64 * ELBO_NCT[MB]


def elbo_wgs_per_cu(MB):
    return 1 if MB * ELBO_NCT[MB] >= 14 else 2


def elbo_full_grid(MB):
    return CUS * elbo_wgs_per_cu(MB)


def elbo_parts():
    return 2 * CUS


def elbo_workspace(M, C, L):
    """gpsa_quadform_elbo_f32_workspace: the packed operand and slabs for two workgroups per CU whatever the grid"""
    MB = mb_for(M)
    if M < 1 or C < 1 or L < 1 or not MB or MB > 16:
        return 0
    MP = 16 * MB
    return L * MP * MP * 4 + 2 * CUS * 2 * MP * elbo_width(MB) * 4


def elbo_takes_delta(M):
    MB = mb_for(M)
    return M >= 1 and bool(MB) and MB <= 16 and has_padding_row(M, MB)


def elbo_kernel(M):
    """(MB, NCT, RL, headline instantiation <13, 2, RL, FULLT, PAIRB>?) that elbo_shape launches"""
    MB = mb_for(M)
    return MB, ELBO_NCT[MB], last_tile_rl(M, MB), MB == 13 and M > 16 * (MB - 1)


def elbo_ngather(MB):
    """(4-byte gather operations per wave and output, surplus lanes of the last one)"""
    n = 3 * ELBO_NCT[MB] * 16
    ops = cdiv(n, 64)
    return ops, ops * 64 - n


def elbo_plan(M, C, L):
    """(ntiles, T, G, the set of range kinds, two-step ranges whose steps are both partial: both ``which`` in one workgroup)"""
    MB = mb_for(M)
    ntiles = cdiv(C, elbo_width(MB))
    T = ntiles * L
    G = min(elbo_full_grid(MB), T)
    rng = item_ranges(T, G)
    kinds = {range_kind(a, b, L) for (a, b) in rng} - {None}
    both = sum(1 for (a, b) in rng if b > a and len(tile_order(a, b, L)) >= 2
               and sum(1 for (_, lo, hi) in tile_order(a, b, L) if (lo, hi) != (0, L - 1)) >= 2)
    return ntiles, T, G, kinds, both


def lmc_inst(L, nb=False):
    """(NLT, NPT) of lmc_mfma_launch / lmc_mfma_nb_launch; None beyond 64 latent outputs"""
    for lim, nlt, npt in ((16, 1, 8), (32, 2, 4), (64, 4, 2)):
        if L <= lim:
            return nlt, (npt // 2 if nb else npt)
    return None


def lmc_pc(L, nb=False):
    """outputs per chunk: 64 NPT"""
    return 64 * lmc_inst(L, nb)[1]


def lmc_blocks(C, nparts):
    return max(1, min(cdiv(C, 16), 2 * CUS, nparts))


def lmc_grid(S, N, nparts):
    """the min(cdiv(N, 16), G) of the four LMC entries"""
    return min(cdiv(N, 16), lmc_blocks(S * N, nparts))


def lmc_workspace(C, L, P, nparts):
    return lmc_blocks(C, nparts) * L * P * 4 + 256 if min(C, L, P, nparts) >= 1 else 0


def lmc_nb_workspace(C, L, P, nparts):
    old = lmc_workspace(C, L, P, nparts)
    return ((old + 7) & ~7) + 8 * lmc_blocks(C, nparts) * P if old else 0


# ---- shapes (issue "Pin the fused ELBO and LMC likelihood kernels ..."; claims held by tests/test_fused_lik_shapes.py) -----
ELBO_ROWS = [1] + cu.TILE_EDGE_M + [65, 113, 192]
ELBO_ROW_L = 3
DELTA_M = sorted(set(range(17, 32)) | {16 * (mb - 1) + d for mb in (4, 7, 13, 16) for d in (1, 8, 9, 15)})
DELTA_REFUSED = [16 * mb for mb in ELBO_CLASSES]  # d = 16: no padding row


def elbo_columns(MB):
    """one full tile and a 5-column tail, and a 4-column tail"""
    return [elbo_width(MB) + 5, elbo_width(MB) + 4]


def sample_split(C):
    """(S, N) with S N = C and S the smallest factor above 1 (S = 1 for a prime C)"""
    for s in range(2, int(C ** 0.5) + 1):
        if C % s == 0:
            return s, C // s
    return 1, C


def elbo_split_cases(MB):
    """(M, C, L, what): T = G exactly (L = 4, one item per workgroup), T = G + 1 or + 2 (L = 3: ranges of one and two
    items - but at G = 256 and 512 no two-item range crosses a tile edge, so every slab is the workgroup's first),
    the fewest tiles above that at which one workgroup ends one tile and begins the next (T = G + 5 or + 7: both ``which``),
    L = 1 (nothing is shared: soff stays empty), T = 2G at L = 2 (every workgroup owns one whole tile: the loop over a
    tile's outputs runs twice in one workgroup - at the row-class shapes, T = 6 items on 6 workgroups, it never does - and
    the tile is stored plainly) and, for the headline class, T = 5G + 1"""
    G, w = elbo_full_grid(MB), elbo_width(MB)
    Ms, Ml = 16 * (MB - 1) + 5, 16 * (MB - 1) + 13
    out = [(Ms, (G // 4) * w - 3, 4, "T=G"), (Ml, cdiv(G + 1, 3) * w - 3, 3, "T=G+"), (Ms if MB % 2 else Ml, 2 * w - 3, 1, "L=1")]
    nt = next(n for n in range(cdiv(G + 1, 3), G) if elbo_plan(Ms, n * w - 3, 3)[4] >= 1)
    out.append((Ms, nt * w - 3, 3, "T=G++"))
    out.append((Ml, G * w - 3, 2, "T=2G"))
    if MB == 13:
        out.append((Ml, cdiv(5 * G + 1, 3) * w - 3, 3, "T=5G+"))
    return out


LMC_L = [1, 16, 17, 32, 33, 64]
LMC_GRIDS = [(49, 3, 3), (1, 1, 1), (15, 3, 1), (16, 1, 2 * CUS), (17, 3, 2 * CUS), (49, 1, 1)]  # (N, S, nparts)
LMC_MASKS = ["random", "output", "spot", "block", "corners"]


def lmc_outputs(L, nb=False):
    pc = lmc_pc(L, nb)
    return [1, 5, pc - 1, pc, pc + 1, 2 * pc + 17]


# ---- named edge indices ----------------------------------------------------------------------------------------------------
def elbo_named_rows(M, extra=()):
    base = 16 * (mb_for(M) - 1)
    return sorted({r for r in (M - 1, base, base + 7, base + 8) + tuple(extra) if 0 <= r < M})


def elbo_named_cols(C, N):
    cols = {0, 63, 64, C - 4, C - 1}
    for s in range(1, min(C // N, 5)):  # both sides of (at most four) sample boundaries
        cols |= {s * N - 1, s * N}
    return sorted(c for c in cols if 0 <= c < C)


def lmc_named(S, N, L, P, PC):
    return {"outputs": sorted({p for p in (P - 1, PC - 1, PC) if 0 <= p < P}),
            "spots": sorted({N - 1, 16 * ((N - 1) // 16)}),
            "latents": sorted({l for l in (15, 16, L - 1) if 0 <= l < L})}


def pow2_sqrt(n):
    """the power of two s with s^2 >= n"""
    return 2.0 ** math.ceil(math.log2(n) / 2) if n > 1 else 1.0


# ---- the closings: values, derivatives' carriers and bounds, fp64 ---------------------------------------------------------
def gam(k):
    return k * U / (1 - k * U)


def _rnd(x, E=0.0):
    """one fp32 rounding of a computed quantity whose exact value is within E of x"""
    return U * (x.abs() + E)


def close(lik, F, y, obs, S, noise_u=None, off=None, rho=None, E_in=0.0):
    """-> dict d, E_d (dLoss/dF), t, E_t (the summed term), u, E_u (NB), eta (what must stay below ETA_MAX; Gaussian: None).
    F, y, off, rho: fp64 tensors that broadcast; obs: bool (False: a missing entry - exact zeros); y may hold NaN there."""
    F = F.double()
    y = torch.where(obs, y.double(), torch.zeros((), dtype=f64)) + torch.zeros_like(F)
    obs = obs.expand_as(y)
    E_in = E_in + torch.zeros_like(F)
    out = {"u": None, "E_u": None, "eta": None}
    if lik in (GAUSS, SKIP):
        sN = math.exp(float(noise_u)) + 1e-5
        coef, inv = -1.0 / (sN * sN * S), 1.0 / sN
        r = y - F
        E_r = E_in + _rnd(r, E_in)
        d = coef * r
        E_d = abs(coef) * E_r * (1 + 2 * U) + gam(2) * d.abs()  # coef's own rounding, the product
        z = r * inv
        E_z = abs(inv) * E_r * (1 + 2 * U) + gam(2) * z.abs()
        t = z * z
        E_t = 2 * z.abs() * E_z + E_z * E_z + U * (z.abs() + E_z) ** 2  # the square (inside the fma of the LMC kernel: counted once more)
    elif lik == POIS:
        coef = 1.0 / S
        eta = F + (0.0 if off is None else off.double())
        E_eta = E_in + (0.0 if off is None else _rnd(eta, E_in))
        ex = torch.exp(eta)
        E_ex = ex * (torch.expm1(E_eta) + 4 * U * torch.exp(E_eta))
        dif = ex - y
        d = coef * dif
        E_d = coef * (E_ex + _rnd(dif, E_ex)) * (1 + 2 * U) + gam(2) * d.abs()
        t = y * eta - ex
        E_t = y.abs() * E_eta + E_ex
        E_t = E_t + _rnd(t, E_t)
        out["eta"] = eta
    else:
        assert lik == NB, lik
        coef = 1.0 / S
        s = F + (0.0 if off is None else off.double())
        E_s = E_in + (0.0 if off is None else _rnd(s, E_in))
        rho = rho.double()
        a = s - rho
        E_a = E_s + _rnd(a, E_s)
        r = torch.exp(rho) + torch.zeros_like(F)
        E_r = 4 * U * r
        ee = torch.exp(-a.abs())
        E_ee = ee * (torch.expm1(E_a) + 4 * U * torch.exp(E_a))
        l1p = torch.log1p(ee)
        E_l1p = E_ee + 4 * U * (l1p + E_ee)  # log1p' <= 1 on [0, 1]
        sp = a.clamp_min(0) + l1p
        E_sp = E_a + E_l1p
        E_sp = E_sp + _rnd(sp, E_sp)
        sg = torch.sigmoid(a)
        # either branch is sigma(a) exactly: sigma'(a) exp(E_a) carries a's error (|d log sigma' / da| <= 1), |d sg / d e| <= 1
        # expf's; 1 + e and the division round
        E_sg = (sg * (1 - sg) * torch.exp(E_a) * E_a + 4 * U * ee) * (1 + gam(3)) + gam(3) * sg
        yr = y + r
        E_yr = E_r + _rnd(yr, E_r)
        dd = yr * sg - y
        E_dd = E_yr * (sg + E_sg) + yr.abs() * E_sg
        E_dd = E_dd + _rnd(dd, E_dd)
        d = coef * dd
        E_d = coef * E_dd * (1 + 2 * U) + gam(2) * d.abs()
        prod = yr * sp
        E_prod = E_yr * (sp + E_sp) + yr.abs() * E_sp
        E_prod = E_prod + _rnd(prod, E_prod)
        t = y * a - prod
        E_t = y.abs() * E_a + E_prod
        E_t = E_t + _rnd(t, E_t)
        u = -r * sp + dd
        E_u = E_r * (sp + E_sp) + r * E_sp + E_dd
        E_u = E_u + _rnd(u, E_u)
        zero = torch.zeros_like(F)
        out.update(u=torch.where(obs, u, zero), E_u=torch.where(obs, E_u, zero), eta=a)
    zero = torch.zeros_like(F)
    out.update(d=torch.where(obs, d, zero), E_d=torch.where(obs, E_d, zero), t=torch.where(obs, t, zero),
               E_t=torch.where(obs, E_t, zero))
    return out


def np_close(lik, F, y, obs, S, noise_u=None, off=None, rho=None, other=False):
    """the closings in plain fp32 NumPy: the kernels' formulation, or (other) a different one - sigma(a) = 1 / (1 + exp(-a))
    directly, softplus through logaddexp, the Gaussian term as r^2 / s^2.  -> (d, t, u)"""
    f = np.float32
    F, y = F.astype(f), np.where(obs, y, 0).astype(f)
    if lik in (GAUSS, SKIP):
        sN = math.exp(float(noise_u)) + 1e-5
        r = y - F
        if other:
            d, t = -(r / f(sN * sN)) / f(S), (r * r) / f(sN * sN)
        else:
            d, z = f(-1.0 / (sN * sN * S)) * r, r * f(1.0 / sN)
            t = z * z
        u = None
    elif lik == POIS:
        eta = F + (f(0) if off is None else off.astype(f))
        ex = np.exp(eta)
        d, t, u = ((ex - y) / f(S), y * eta - ex, None) if other else (f(1.0 / S) * (ex - y), y * eta - ex, None)
    else:
        a = (F + (f(0) if off is None else off.astype(f))) - rho.astype(f)
        r = np.exp(rho.astype(f))
        if other:
            sg, sp = f(1) / (f(1) + np.exp(-a)), np.logaddexp(f(0), a)
        else:
            e = np.exp(-np.abs(a))
            sp, sg = np.maximum(a, f(0)) + np.log1p(e), np.where(a >= 0, f(1), e) / (f(1) + e)
        yr = y + r
        dd = yr * sg - y
        d, t, u = (dd / f(S) if other else f(1.0 / S) * dd), y * a - yr * sp, np.where(obs, -r * sp + dd, 0)
    return np.where(obs, d, 0), np.where(obs, t, 0), u


# ---- fused ELBO: inputs -----------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=f64)


def col_maps(C, N):
    return torch.arange(C) % N


def _counts(g, eta):
    return torch.poisson(torch.exp(eta.clamp(max=6.0)), generator=g)


@functools.lru_cache(maxsize=2)
def _elbo_base(M, C, L, family, rows=None):
    """alpha, Omega (both precisions) of contraction_util's family, and the fp64 pieces every closing of the shape shares:
    v = alpha^T Omega alpha and its absolute sum, from the fp32 Omega"""
    inp = cu.make_inputs(M, C, L, family, rows=rows)
    a, Om = inp["al"].double(), inp["Om32"].double()
    v = torch.stack([((Om[l] @ a) * a).sum(0) for l in range(L)])
    return inp["al"], inp["Om32"], inp["Om64"], v


def elbo_inputs(M, C, L, lik, family, delta=False, offs=True, miss=None, seed=0, rows=None):
    """dict of CPU tensors as stored (fp32; q fp64) and the scalars S, N.  family "plain" / "edge": contraction_util's
    alpha and Omega (edge: the named rows of alpha, rows and columns of Omega scaled by row_scale), delta's named rows
    likewise; eps is drawn N(0, 1) / max(1, sd) so that the draw's random part stays of order one whatever the variance (a
    log rate must stay below ETA_MAX) and doubled at the named columns (edge).  q is chosen so that exp(var_u) - q lies in
    [0.3, 0.5]: Omega is positive semi-definite, so the variance is at least 0.3.  miss: None, or a fraction of Y set NaN.
    rows: the edge family's named rows (of alpha, Omega and delta) where another kernel names its own (default:
    contraction_util's for alpha and Omega, elbo_named_rows for delta)"""
    S, N = sample_split(C)
    al, Om32, Om64, v = _elbo_base(M, C, L, family, None if rows is None else tuple(rows))
    g = _gen(1009 * seed + 31 * M + C + 7 * L + LIKS.index(lik) + 5 * int(delta))
    var_u = torch.tensor([math.log(0.8)], dtype=f32)
    var0 = math.exp(float(var_u))
    resid = 0.3 + 0.2 * torch.rand(C, generator=g, dtype=f64)
    q = var0 - resid
    sd = torch.sqrt(resid[None, :] + v + 2e-5)
    eps = (_randn(g, C, L) / sd.t().clamp_min(1.0))
    named = elbo_named_cols(C, N)
    if family == "edge":
        eps[named] *= 2.0
    eps = eps.float()
    out = {"al": al, "Om32": Om32, "Om64": Om64, "q": q, "var_u": var_u, "eps": eps, "S": S, "N": N, "named_cols": named}
    if delta:
        d = 0.25 * _randn(g, M, L) / M ** 0.5
        if family == "edge":
            d[elbo_named_rows(M) if rows is None else list(rows)] *= cu.row_scale(M)
        out["delta"] = d.float()
        mean = out["delta"].double().t() @ al.double()
    else:
        out["meanT"] = (0.5 * _randn(g, L, C)).float()
        mean = out["meanT"].double()
    Fd = mean + sd * eps.double().t()  # [L, C], close to what the device draws
    if lik in (GAUSS, SKIP):
        out["noise_u"] = torch.tensor([math.log(0.7)], dtype=f32)
        Y = Fd[:, :N].t() + 0.7 * _randn(g, N, L)
    else:
        if offs:
            out["off"] = (0.5 * _randn(g, N)).float()
        if lik == NB:
            out["rho"] = (0.5 * _randn(g, L)).float()
        eta = Fd[:, :N].t() + (out["off"].double()[:, None] if offs else 0.0)
        Y = _counts(g, eta)
    Y = Y.float()
    if miss:
        Y[torch.rand(N, L, generator=g) < miss] = NAN
    out["Y"] = Y
    return out


# ---- fused ELBO: reference, stage by stage ----------------------------------------------------------------------------------
def elbo_reference(inp, M, C, L, lik, om="Om32", delta=False, skip=False, prod_bar=None):
    """stage 1 from the inputs alone: dict F, E_F, sd, E_sd, var (all [L, C] fp64), W, absW ([L, M, C]: Omega_l alpha and its
    absolute counterpart) and the per-(l, c) views of Y, the offsets and the observed mask.  prod_bar(K, S): the bound of
    one element of Omega_l alpha where the contraction is not the fp32 one (the closing's M-term dot product stays fp32)"""
    a, Om = inp["al"].double(), inp[om].double()
    N, cm = inp["N"], col_maps(C, inp["N"])
    W = torch.stack([Om[l] @ a for l in range(L)])
    absW = torch.stack([Om[l].abs() @ a.abs() for l in range(L)])
    v, absv = (W * a[None]).sum(1), (absW * a.abs()[None]).sum(1)
    E_v = bar(2 * M, absv, u=U) if prod_bar is None else prod_bar(M, absv) + bar(M, absv + prod_bar(M, absv), u=U)
    resid = (math.exp(float(inp["var_u"])) - inp["q"]).float().double()[None, :]  # formed in fp64, rounded once
    t1 = resid + v
    var = t1 + float(np.float32(2e-5))
    # resid: the device's fp64 exp may differ in the last place before the rounding to fp32; then the two fp32 adds
    E_var = E_v + U * resid.abs() + _rnd(t1, E_v)
    E_var = E_var + _rnd(var, E_var)
    sd = torch.sqrt(var)
    E_sd = E_var / (2 * torch.sqrt((var - E_var).clamp_min(1e-300)))
    E_sd = E_sd + 2 * U * (sd + E_sd)
    e = inp["eps"].double().t()
    if delta:
        dl = inp["delta"].double()
        mean, E_mean = dl.t() @ a, (prod_bar or (lambda K, S: bar(K, S, u=U)))(M, dl.abs().t() @ a.abs())
    else:
        mean, E_mean = inp["meanT"].double(), torch.zeros_like(var)
    se = sd * e
    E_se = E_sd * e.abs()
    E_se = E_se + _rnd(se, E_se)
    F = mean + se
    E_F = E_mean + E_se
    E_F = E_F + _rnd(F, E_F)
    y = inp["Y"].double().t()[:, cm]
    obs = ~torch.isnan(y) if skip else torch.ones_like(y, dtype=torch.bool)
    off = inp["off"].double()[cm][None, :] if "off" in inp else None
    rho = inp["rho"].double()[:, None] if "rho" in inp else None
    return {"F": F, "E_F": E_F, "sd": sd, "E_sd": E_sd, "var": var, "E_var": E_var, "W": W, "absW": absW, "e": e, "y": y,
            "obs": obs, "off": off, "rho": rho, "v": v, "E_v": E_v}


def elbo_closing(inp, ref, lik, F):
    """the closing of ``lik`` applied in fp64 to the draws F ([L, C]: the device's FT, or the reference's)"""
    return close(lik, F, ref["y"], ref["obs"], inp["S"], noise_u=inp.get("noise_u"), off=ref["off"], rho=ref["rho"])


def abar_bound(M, L, abs_ab, want_ab=None, prod_bar=None):
    """section 2e's ACCUM bound; prod_bar: M terms of another contraction per product, then the fp32 chain over the L
    outputs and at most L slab addends (2 L roundings, which bar(L, .) covers with its factor 2)"""
    if prod_bar is None:
        return bar(L * (M + 2), abs_ab, u=U, want32=want_ab)
    return prod_bar(M, abs_ab) + bar(L, abs_ab, u=U, want32=want_ab)


def elbo_stage_ratios(inp, ref, M, C, L, lik, got, prod_bar=None, nct=None):
    """error / bound of every stage against the one before it.  got: FT, dm, g, abar, part [, u, usum] on the CPU.
    prod_bar, nct: another contraction's element bound (elbo_reference) and column tiles per wave"""
    FT, dm, g = got["FT"].double(), got["dm"].double(), got["g"].double()
    NCT = ELBO_NCT[mb_for(M)] if nct is None else nct
    out = {"FT": ratio(FT, ref["F"], ref["E_F"])}
    cl = elbo_closing(inp, ref, lik, FT)
    if cl["eta"] is not None:
        assert float(cl["eta"].abs().max()) <= ETA_MAX, float(cl["eta"].abs().max())
    out["dmeanT"] = ratio(dm, cl["d"], cl["E_d"])
    want_g = dm * ref["e"] / (2 * ref["sd"])
    out["g"] = ratio(g, want_g, want_g.abs() * (ref["E_sd"] / ref["sd"] + 4 * U))
    want_ab = 2 * (g[:, None, :] * ref["W"]).sum(0)
    abs_ab = 2 * (g.abs()[:, None, :] * ref["absW"]).sum(0)
    out["abar"] = ratio(got["abar"].double(), want_ab, abar_bound(M, L, abs_ab, want_ab, prod_bar))
    tsum, tabs = float(cl["t"].sum()), float(cl["t"].abs().sum())
    b_part = float(cl["E_t"].sum()) + NCT * U * tabs + C * L * U64 * tabs
    err = abs(float(got["part"].double().sum()) - tsum)
    out["part"] = err / b_part if b_part > 0 else (0.0 if err == 0 else float("inf"))
    if lik == NB:
        uu = got["u"].double()
        out["u_elems"] = ratio(uu, cl["u"], cl["E_u"])
        out["usum"] = ratio(got["usum"].double(), uu.sum(1), C * U64 * uu.abs().sum(1))
    return out, cl


def elbo_np(inp, M, C, L, lik, om="Om32", delta=False, skip=False, other=False, matmul=None):
    """the whole pass in plain fp32 NumPy (other: rows visited backwards, outputs backwards, the other closing formulation)
    -> FT, dm, g, abar, part (fp64 sum of the fp32 terms), u.  matmul(A, B): the contraction Omega_l alpha (and delta^T
    alpha) as another kernel forms it (default: NumPy's fp32 product)"""
    f = np.float32
    mm = matmul or (lambda A, B: A @ B)
    al, Om = inp["al"].numpy(), inp[om].float().numpy()
    order = list(range(M))[::-1] if other else list(range(M))
    a_o, Om_o = al[order], Om[:, order][:, :, order]
    W = np.stack([mm(Om_o[l], a_o) for l in range(L)])  # rows in ``order``
    v = (W * a_o[None]).sum(1, dtype=f)
    resid = (math.exp(float(inp["var_u"])) - inp["q"].numpy()).astype(f)[None, :]
    sd = np.sqrt(resid + v + f(2e-5))
    e = inp["eps"].numpy().T
    mean = mm(np.ascontiguousarray(inp["delta"].numpy()[order].T), a_o) if delta else inp["meanT"].numpy()
    F = mean + sd * e
    cm = col_maps(C, inp["N"]).numpy()
    y = inp["Y"].numpy().T[:, cm]
    obs = ~np.isnan(y) if skip else np.ones_like(y, dtype=bool)
    off = inp["off"].numpy()[cm][None, :] if "off" in inp else None
    rho = inp["rho"].numpy()[:, None] if "rho" in inp else None
    d, t, u = np_close(lik, F, y, obs, inp["S"], noise_u=inp.get("noise_u"), off=off, rho=rho, other=other)
    g = d * e * f(0.5) / sd
    ab = np.zeros((M, C), f)
    for l in (range(L - 1, -1, -1) if other else range(L)):
        ab += g[l][None, :] * W[l]
    inv = np.argsort(order)
    return {"FT": F, "dm": d, "g": g, "abar": (f(2) * ab)[inv], "part": t.astype(np.float64).sum(), "u": u}


def drop_row_FT(inp, ref, om, r):
    """what the draws lose with the terms of v that contain row r of alpha (delta form: and the mean's term)"""
    dv = cu.drop_row_v(inp["al"], inp[om], r)
    F2 = torch.sqrt((ref["var"] - dv).clamp_min(0)) * ref["e"]
    d = ref["sd"] * ref["e"] - F2
    if "delta" in inp:
        d = d + inp["delta"].double()[r][:, None] * inp["al"].double()[r][None, :]
    return d


# ---- fused LMC: inputs, reference --------------------------------------------------------------------------------------------
def lmc_mask(kind, N, P, PC, g):
    m = torch.zeros(N, P, dtype=torch.bool)
    if kind == "random":
        m = torch.rand(N, P, generator=g) < 0.3
    elif kind == "output":
        m[:, min(2, P - 1)] = True
    elif kind == "spot":
        m[N // 2, :] = True
    elif kind == "block":
        m[max(N - 16, 0):, max(P - 16, 0):][:16, :16] = True
    elif kind == "corners":
        m[N - 1, P - 1] = True
        if PC < P:
            m[0, PC] = True
    else:
        assert kind is None, kind
    return m


def lmc_inputs(S, N, L, P, lik, family, mask=None, offs=True, seed=0):
    """F [S, N, L], W [L, P], Y [N, P] (+ off [N], rho [P], noise_u) as stored.  "edge": the named latent rows of F
    are scaled by the power of two s with s^2 >= L (the named term of F W then weighs what the random walk over the
    other L - 1 does, and a log rate stays below ETA_MAX); the named outputs' and spots' observations are scaled by the
    power of two with s^2 >= P, or >= S N (counts: (y + 1) s), so that their dfo carries the sums over p and over (s, n)"""
    nb = lik == NB
    PC = lmc_pc(L, nb)
    g = _gen(7919 * seed + 131 * L + P + 17 * N + S + LIKS.index(lik))
    F = _randn(g, S, N, L)
    W = 0.3 * _randn(g, L, P) / math.sqrt(max(L, 3) / 3.0)
    nm = lmc_named(S, N, L, P, PC)
    if family == "edge":  # (entries at a named index are first raised to half their scale: none may draw a weight near zero)
        wsc = float(W.abs().mean())
        Fm = F.view(S * N, L)
        cu._weigh(Fm, [s_ * N + n for s_ in range(S) for n in nm["spots"]], 1.0, dim=0)
        cu._weigh(Fm, nm["latents"], pow2_sqrt(L), dim=1)
        cu._weigh(W, nm["latents"], 1.0, dim=0, floor=0.5 * wsc)
        cu._weigh(W, nm["outputs"], 1.0, dim=1, floor=0.5 * wsc)
    F, W = F.float(), W.float()
    out = {"F": F, "W": W, "S": S, "N": N, "named": nm, "PC": PC}
    fo = F.double() @ W.double()
    if lik in (GAUSS, SKIP):
        out["noise_u"] = torch.tensor([math.log(0.7)], dtype=f32)
        Y = fo[0] + 0.7 * _randn(g, N, P)
    else:
        if offs:
            out["off"] = (0.5 * _randn(g, N)).float()
        if nb:
            out["rho"] = (0.5 * _randn(g, P)).float()
        Y = _counts(g, fo[0] + (out["off"].double()[:, None] if offs else 0.0))
    if family == "edge":
        for idx, s, dim in ((nm["outputs"], pow2_sqrt(P), 1), (nm["spots"], pow2_sqrt(S * N), 0)):
            sel = Y[:, idx] if dim == 1 else Y[idx]
            sel = sel * s if lik in (GAUSS, SKIP) else (sel + 1.0) * s
            if dim == 1:
                Y[:, idx] = sel
            else:
                Y[idx] = sel
    Y = Y.float()
    if mask is not None:
        Y[lmc_mask(mask, N, P, PC, g)] = NAN
    out["Y"] = Y
    return out


def lmc_reference(inp, L, P, lik, skip, G, drop_latent=None):
    """want and bound of dF [S, N, L], dW [L, P], the sum of zpart and (NB) usum [P], with the closing's pieces.
    drop_latent: the product F W without that latent row (the visibility condition), everything behind it unchanged"""
    S, N, PC = inp["S"], inp["N"], inp["PC"]
    NPT = PC // 64
    F, W = inp["F"].double(), inp["W"].double()
    Ff, Wf = F, W
    if drop_latent is not None:
        Ff = F.clone()
        Ff[:, :, drop_latent] = 0
    fo = Ff @ Wf
    E_fo = bar(L, F.abs() @ W.abs(), u=U)
    y = inp["Y"].double()[None]
    obs = ~torch.isnan(y) if skip else torch.ones_like(y, dtype=torch.bool)
    off = inp["off"].double()[None, :, None] if "off" in inp else None
    rho = inp["rho"].double()[None, None, :] if "rho" in inp else None
    cl = close(lik, fo, y, obs, S, noise_u=inp.get("noise_u"), off=off, rho=rho, E_in=E_fo)
    d, E_d = cl["d"], cl["E_d"]
    nch = cdiv(P, PC)
    dF = d @ W.t()
    b_dF = bar(P + nch, d.abs() @ W.abs().t(), u=U, want32=dF) + E_d @ W.abs().t()
    Fm, dm_ = F.reshape(S * N, L), d.reshape(S * N, P)
    dW = Fm.t() @ dm_
    b_dW = bar(S * N + G, Fm.abs().t() @ dm_.abs(), u=U, want32=dW) + Fm.abs().t() @ E_d.reshape(S * N, P)
    tabs = float(cl["t"].abs().sum())
    out = {"dF": dF, "b_dF": b_dF, "dW": dW, "b_dW": b_dW, "z": float(cl["t"].sum()),
           "b_z": float(cl["E_t"].sum()) + (4 * NPT + 1) * U * tabs + S * N * P * U64 * tabs, "cl": cl, "fo": fo, "obs": obs}
    if lik == NB:
        uu = cl["u"]
        out["usum"] = uu.sum((0, 1))
        out["b_usum"] = cl["E_u"].sum((0, 1)) + (4 + S * N * U64 / U) * U * uu.abs().sum((0, 1))
    return out


def lmc_np(inp, L, P, lik, skip, other=False):
    """the pass in plain fp32 NumPy (other: contracted indices backwards, the other closing formulation)"""
    S = inp["S"]
    F, W = inp["F"].numpy(), inp["W"].numpy()
    fo = (F[:, :, ::-1] @ W[::-1]) if other else F @ W
    y = inp["Y"].numpy()[None] + np.zeros_like(fo)
    obs = ~np.isnan(y) if skip else np.ones_like(y, dtype=bool)
    off = inp["off"].numpy()[None, :, None] if "off" in inp else None
    rho = inp["rho"].numpy()[None, None, :] if "rho" in inp else None
    d, t, u = np_close(lik, fo, y, obs, S, noise_u=inp.get("noise_u"), off=off, rho=rho, other=other)
    d = d.astype(np.float32)
    dF = (d[:, :, ::-1] @ W.T[::-1]) if other else d @ W.T
    Fm, dm_ = F.reshape(-1, L), d.reshape(-1, P)
    dW = (Fm[::-1].T @ dm_[::-1]) if other else Fm.T @ dm_
    return {"dF": dF, "dW": dW, "z": t.astype(np.float64).sum(), "usum": None if u is None else u.astype(np.float64).sum((0, 1))}


def sentinel_frame(src, dev, fill=SENTINEL):
    """an input frame whose surroundings hold ``fill`` instead of NaN (Y under skip != 0)"""
    fr = Frame(src.shape, src.dtype, dev)
    fr.buf.fill_(fill)
    fr.view.copy_(src.to(dev))
    return fr


# ---- the visibility condition of the edge-weighted family, from the reference alone -----------------------------------------
def elbo_visibility(inp, ref, cl, got, M, C, L, lik, om, prod_bar=None, nct=None, rows=None):
    """a lost named row moves half of the draws and half of its abar entries, a lost named column the sum of the terms, by
    more than 4 x their bound.  got: the g that abar is held to (the device's, or the fp32 NumPy one)"""
    g = got["g"].double()
    abs_ab = 2 * (g.abs()[:, None, :] * ref["absW"]).sum(0)
    b_ab = abar_bound(M, L, abs_ab, None, prod_bar)
    for r in (elbo_named_rows(M) if rows is None else rows):
        if M > 1:
            assert visible(drop_row_FT(inp, ref, om, r), ref["E_F"]), ("FT", M, r)
        assert visible(cu.drop_row_dalpha(inp["al"], inp[om], g, r), b_ab), ("abar", M, r)
    tabs = float(cl["t"].abs().sum())
    b_part = float(cl["E_t"].sum()) + (ELBO_NCT[mb_for(M)] if nct is None else nct) * U * tabs
    lost = cl["t"][:, inp["named_cols"]].sum(0).abs()
    assert float((lost > 4 * b_part).double().mean()) >= 0.5, ("part", M, C)


def lmc_visibility(inp, ref, L, P, lik, skip, G):
    """a lost named output moves dF, a lost named spot dW, a lost latent row of the product F W both, at half of the elements
    they feed by more than 4 x the bound"""
    d, F, W = ref["cl"]["d"], inp["F"].double(), inp["W"].double()
    for p_ in inp["named"]["outputs"]:
        assert visible(d[:, :, p_][:, :, None] * W[:, p_][None, None, :], ref["b_dF"]), ("output", p_)
    for n in inp["named"]["spots"]:
        assert visible(torch.einsum("sl,sp->lp", F[:, n, :], d[:, n, :]), ref["b_dW"]), ("spot", n)
    for l in inp["named"]["latents"]:
        if L > 1:
            other = lmc_reference(inp, L, P, lik, skip, G, drop_latent=l)
            assert visible(ref["dW"] - other["dW"], ref["b_dW"]) and visible(ref["dF"] - other["dF"], ref["b_dF"]), ("latent", l)
