"""Shared by tests/test_step_layout_shapes.py (CPU) and tests/test_step_layout_gpu.py: the layout cases of the step
engine's own kernels (csrc/step.hip), a scalar whose gradient never passes through an fp32 contraction, its fp64
reference on the CPU, and the per-element bounds.

The scalar.  The warp layer and the KL terms of the step run in fp64 (engine.py / step.hip headers); their outputs and
gradients are rounded to fp32 ONCE (the sampler's stores, step_finalize_kernel).  For

    J = sum_m <A_m, G_means[m]> + sum_m <B_m, G_samples[m]> + sum_t c_t kl_t

(A, B fixed fp32 tensors: the node hands dG_* to the engine as fp32; c_t distinct fp64 weights: a permuted term order
shows) nothing reaches F_latent, so the engine's outputs and parameter gradients are the fp64 answer rounded to fp32 -
checked element by element:

    |got - ref| <= 2^-23 |ref| + 2^-30 max|ref|

one fp32 rounding (2^-24 |ref|, doubled) plus an absolute term 64 times below the rounding at the largest entry.  The
max is over the tensor, or over ONE VIEW's slice for the per-view parameters (a long view cannot shield a short one).

The reference's own error.  The fp64 chain's error is about 8 M kappa 2^-53 of the quantities it combines, kappa the
largest condition number of K_uu + 1e-5 I or Omega = A A^T + 1e-5 I in the case.  Inducing points on a jittered grid
(spacing 1.5 lengthscales, jitter 0.15 of it), Omega_sqt = 0.3 I + 0.05 tril(randn), delta_G = Xtilde + 0.1 randn, data
inside the grid's range keep kappa small; test_step_layout_shapes.py asserts kappa <= 1e3 for every case - a condition
on the INPUTS - which makes 8 M kappa 2^-53 < 3e-11 at M <= 27, three orders below 2^-30 (the one M = 512 case: the same
figure is asserted with its own, measured kappa).
"""
import ctypes as C
import math
import zlib

import numpy as np
import torch

from oracle import gpsa_oracle as orc

F64 = torch.float64
U32 = 2.0 ** -23       # relative term: one fp32 rounding is 2^-24 |ref|
ABS32 = 2.0 ** -30     # absolute term, times max|ref|
KL_RTOL = 1e-11        # the suite's fp64 tolerance (TOL[torch.float64] in test_hip_kernels.py)
KAPPA_MAX = 1e3
MAX_RUN = 16           # KM_MAXB_STEP: views per batched launch

# name: rows per modality per view, fixed views, D, S, Mx, Mg, (L, P, lmc) per modality, warp kernel
CASES = {
    "one_block_ragged": dict(rows=[[37, 90, 5]], fixed=None, D=2, S=1, Mx=9, Mg=11, Cs=128),
    "two_col_blocks": dict(rows=[[257, 64, 1]], fixed=None, D=2, S=3, Mx=9, Mg=9, Cs=320),
    "exact_blocks": dict(rows=[[256, 256, 256]], fixed=[1], D=1, S=1, Mx=6, Mg=8, Cs=256),
    "three_col_blocks": dict(rows=[[513, 255]], fixed=None, D=3, S=2, Mx=12, Mg=10, Cs=576, warp="matern32"),
    "empty_in_one_modality": dict(rows=[[100, 0, 60], [30, 200, 0]], fixed=None, D=2, S=2, Mx=9, Mg=12, Cs=256,
                                  outs=[(3, 3, 0), (2, 5, 1)]),
    "three_modalities": dict(rows=[[200, 100], [100, 250], [7, 300]], fixed=None, D=2, S=1, Mx=9, Mg=9, Cs=704),
    "empty_everywhere": dict(rows=[[40, 0, 50, 30]], fixed=[0], D=2, S=2, Mx=6, Mg=8, Cs=64),
    "seventeen_free": dict(rows=[list(range(11, 31))], fixed=[1], D=2, S=1, Mx=6, Mg=7, Cs=64),
    # D = MAXD: the constructor takes the dimension from the coordinates and the engine is eligible up to 4
    "four_dims": dict(rows=[[70, 130]], fixed=[1], D=4, S=2, Mx=16, Mg=16, Cs=128),
    # coldot2_kernel runs only where the projection kernel declines (gpsa_whiten_workspace(M) == 0, from M = 512 on): up
    # to there q = k^T alpha comes out of the projection itself, so none of the small-M cases above launches it.  This
    # one does, over two column blocks and two problems of a batch (blockIdx.y); its K_uu is a 23 x 23 lattice's first 512
    "beyond_projection": dict(rows=[[300, 70]], fixed=None, D=2, S=1, Mx=512, Mg=8, Cs=320),
}
# empty_everywhere at a size where central differences over every parameter take a second
SMALL_EMPTY = dict(rows=[[8, 0, 10, 6]], fixed=[0], D=2, S=2, Mx=6, Mg=8, Cs=64)


class Case:
    def __init__(self, name, spec=None):
        spec = dict(CASES[name] if spec is None else spec)
        self.name = name
        self.rows = [list(r) for r in spec["rows"]]
        self.fixed = spec["fixed"]
        self.D, self.S, self.Mx, self.Mg, self.Cs = (spec[k] for k in ("D", "S", "Mx", "Mg", "Cs"))
        self.warp = spec.get("warp", "rbf")
        self.V = len(self.rows[0])
        self.mods = [f"mod{i}" for i in range(len(self.rows))]
        self.outs = spec.get("outs") or [(3, 3, 0)] * len(self.rows)  # (L, P, lmc)
        self.seed = zlib.crc32(name.encode()) % 100000  # a function of the name alone: adding a case moves no other

    def is_fixed(self, v):
        return self.fixed is not None and v in self.fixed

    # ---- what the plan must derive from the layout (restated here, independently of step.hip) -------------
    @property
    def nview(self):
        return [sum(r[v] for r in self.rows) for v in range(self.V)]

    @property
    def free(self):
        return [v for v in range(self.V) if not self.is_fixed(v)]

    def expected(self):
        free = self.free
        live = max([self.nview[v] for v in free] or [0])
        runs, i = 0, 0
        while i < len(free):
            e = i + 1
            while e < len(free) and free[e] == free[e - 1] + 1 and e - i < MAX_RUN:
                e += 1
            runs += 1
            i = e
        return dict(Cs=(live + 63) // 64 * 64, runs=runs, eps=self.S * self.D * sum(self.nview[v] for v in free),
                    n_kl=self.V * self.D + sum(L for L, _, _ in self.outs))

    def run_lengths(self):
        free, out, i = self.free, [], 0
        while i < len(free):
            e = i + 1
            while e < len(free) and free[e] == free[e - 1] + 1 and e - i < MAX_RUN:
                e += 1
            out.append(e - i)
            i = e
        return out

    def describe(self):
        """gpsa_step_describe on this layout -> (rc, dict(n_kl, eps, runs, Cs))"""
        from spatial_alignment_amd import _lib
        from spatial_alignment_amd.ops import KINDS

        lib = _lib.load()
        d = _lib.StepDesc()
        d.n_views, d.n_dims, d.n_mods, d.n_samples = self.V, self.D, len(self.rows), self.S
        d.m_x, d.m_g, d.kind_warp, d.kind_data = self.Mx, self.Mg, KINDS[self.warp], KINDS["rbf"]
        flat = []
        for i, ((L, P, lmc), r) in enumerate(zip(self.outs, self.rows)):
            d.n_latent[i], d.n_out[i], d.has_lmc[i], d.n_rows[i] = L, P, lmc, sum(r)
            flat += r
        d.want_kl = 1
        fx = (C.c_int * self.V)(*[1 if self.is_fixed(v) else 0 for v in range(self.V)])
        rw = (C.c_longlong * len(flat))(*flat)
        d.view_fixed, d.view_rows = fx, rw
        out = (C.c_longlong * 7)()
        rc = lib.gpsa_step_describe(C.byref(d), out)
        return rc, dict(n_kl=int(out[2]), eps=int(out[3]), runs=int(out[4]), Cs=int(out[5]))

    # ---- inputs -----------------------------------------------------------------------------------------
    def _grid(self, M, ell, gen):
        """the first M points of a lattice with spacing 1.5 ell, jittered by 0.15 of the spacing -> ([M, D], side)"""
        D = self.D
        side = max(2, math.ceil(M ** (1.0 / D) - 1e-9))
        ax = [torch.arange(side, dtype=F64)] * D
        pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, D)[:M]
        h = 1.5 * ell
        return h * (pts + 0.15 * (2 * torch.rand(M, D, generator=gen, dtype=F64) - 1)), side

    def build(self):
        """-> dict(dd, X, state (fp32 CPU tensors, state_dict names + the mean function), cfg (the oracle's), eps_G,
        eps_F, A, B, c); everything a function of the case's seed"""
        gen = torch.Generator().manual_seed(self.seed)
        V, D, S = self.V, self.D, self.S
        randn = lambda *sh: torch.randn(*sh, generator=gen, dtype=F64)
        ls_u = 0.1 * randn(V)                      # per-view lengthscales around 1: per-view strides show
        var_u = 0.1 * randn(V)
        dls_u, dvar_u = 0.1 * randn(1), 0.1 * randn(1)
        Xt, span = [], []
        for v in range(V):
            z, side = self._grid(self.Mx, float(torch.exp(ls_u[v])), gen)
            Xt.append(z)
            span.append(1.5 * float(torch.exp(ls_u[v])) * (side - 1))
        Xtilde = torch.stack(Xt)
        Gtilde, _ = self._grid(self.Mg, float(torch.exp(dls_u[0])), gen)

        def sqt(n, M):
            # (0.05 up to M = 27; beyond, scaled so that the triangle's norm ~ 0.05 sqrt(M) stays well below the 0.3 I)
            return 0.3 * torch.eye(M, dtype=F64) + 0.05 * min(1.0, 27.0 / M) * torch.tril(randn(n, M, M))

        st = {"Xtilde": Xtilde, "delta_G_list": Xtilde + 0.1 * randn(V, self.Mx, D),
              "Omega_sqt_G_list": sqt(V * D, self.Mx), "warp_kernel_lengthscales": ls_u,
              "warp_kernel_variances": var_u, "Gtilde": Gtilde, "data_kernel_lengthscale": dls_u,
              "data_kernel_variance": dvar_u, "noise_variance": randn(2) - 1,
              # non-trivial mean function: step_finalize_kernel applies the slopes transposed, the identity hides that
              "mean_slopes": torch.eye(D, dtype=F64) + 0.1 * randn(V, D, D), "mean_intercepts": randn(V, D)}
        dd, X = {}, {}
        for m, r, (L, P, lmc) in zip(self.mods, self.rows, self.outs):
            st[f"Omega_sqt_F_dict.{m}"] = sqt(L, self.Mg)
            st[f"delta_F_dict.{m}"] = randn(self.Mg, L)
            if lmc:
                st[f"W_dict.{m}"] = randn(L, P)
            # data inside the range of its view's grid
            X[m] = torch.cat([span[v] * torch.rand(r[v], D, generator=gen, dtype=F64) for v in range(V)]).float()
            dd[m] = {"spatial_coords": X[m], "outputs": randn(sum(r), P).float(), "n_samples_list": list(r)}
        st = {k: t.float() for k, t in st.items()}
        nview = self.nview
        eps_G = [randn(S, nview[v], D).float() for v in self.free if nview[v] > 0]
        eps_F = {m: randn(S, sum(r), L).float() for m, r, (L, _, _) in zip(self.mods, self.rows, self.outs)}
        A = {m: randn(sum(r), D).float() for m, r in zip(self.mods, self.rows)}
        B = {m: randn(S, sum(r), D).float() for m, r in zip(self.mods, self.rows)}
        T = V * D + sum(L for L, _, _ in self.outs)
        c = 0.5 + torch.rand(T, generator=gen, dtype=F64) + 0.01 * torch.arange(T, dtype=F64)  # distinct
        cfg = dict(modality_names=list(self.mods), n_views=V, n_spatial_dims=D, kernel_warp=self.warp,
                   kernel_data="rbf", fixed_view_idx=self.fixed,
                   n_latent_gps={m: (L if lmc else None) for m, (L, _, lmc) in zip(self.mods, self.outs)})
        return dict(dd=dd, X=X, state=st, cfg=cfg, eps_G=eps_G, eps_F=eps_F, A=A, B=B, c=c)

    def model(self, inp, device):
        """VariationalGPSA on ``device`` carrying ``inp["state"]`` (parameters and the mean function's buffers)"""
        import spatial_alignment_amd as gp

        kfn = {"rbf": gp.rbf_kernel, "matern12": gp.matern12_kernel, "matern32": gp.matern32_kernel}
        torch.manual_seed(0)
        np.random.seed(0)
        model = gp.VariationalGPSA(inp["dd"], m_X_per_view=self.Mx, m_G=self.Mg, data_init=False,
                                   n_latent_gps=inp["cfg"]["n_latent_gps"], kernel_func_warp=kfn[self.warp],
                                   kernel_func_data=gp.rbf_kernel, fixed_view_idx=self.fixed)
        st = inp["state"]
        missing = model.load_state_dict({k: t for k, t in st.items() if not k.startswith("mean_")}, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        with torch.no_grad():
            model.mean_slopes.copy_(st["mean_slopes"])
            model.mean_intercepts.copy_(st["mean_intercepts"])
        return model.to(device)


# ---------------------------------------------------------------------------------------------------------
# the fp64 reference
# ---------------------------------------------------------------------------------------------------------
TRAINABLE = orc.TRAINABLE_PREFIXES


def _mvn_kl(d, Om, Lk):
    """KL( N(mu_q, Om) || N(mu_p, Lk Lk^T) ) with d = mu_q - mu_p (torch.distributions.kl's formula, what
    negative_elbo evaluates): 0.5 (logdet K - logdet Om + tr K^-1 Om + d^T K^-1 d - M)"""
    M = d.shape[0]
    Lo = torch.linalg.cholesky(Om)
    half = lambda L: torch.log(torch.diagonal(L)).sum()
    tr = torch.linalg.solve_triangular(Lk, Lo, upper=False).square().sum()
    maha = torch.linalg.solve_triangular(Lk, d.unsqueeze(1), upper=False).square().sum()
    return half(Lk) - half(Lo) + 0.5 * (tr + maha - M)


def _prior_chol(st, cfg, v):
    k = orc.KERNELS[cfg["kernel_warp"]]
    Z = st["Xtilde"][v]
    K = k(Z, Z, lengthscale_unconstrained=st["warp_kernel_lengthscales"][v],
          output_variance_unconstrained=st["warp_kernel_variances"][v])
    return torch.linalg.cholesky(K + orc.JITTER * torch.eye(Z.shape[0], dtype=Z.dtype))


def kl_terms(st, cfg, h):
    """the per-term KL vector in the engine's order: Omega_G rows r = j*V + v (quirk 2: row r pairs with view r % V and
    coordinate r // V), then every modality's outputs.  A fixed view's terms are 0; a free view WITHOUT rows keeps its
    terms (test_empty_free_view_keeps_its_kl_terms): the oracle leaves its Kuu_chol_G as None, so its prior is
    factorised here."""
    V, D = cfg["n_views"], cfg["n_spatial_dims"]
    OmG = orc.omega_from_sqrt(st["Omega_sqt_G_list"])
    zero = torch.zeros((), dtype=OmG.dtype)
    chol = {}
    terms = []
    for r in range(V * D):
        j, v = divmod(r, V)
        if orc._is_fixed(cfg.get("fixed_view_idx"), v):
            terms.append(zero)
            continue
        if v not in chol:
            Lk = h["Kuu_chol_G"][v]
            chol[v] = Lk if Lk is not None else _prior_chol(st, cfg, v)
        terms.append(_mvn_kl(st["delta_G_list"][v, :, j] - h["mu_z_G"][v, :, j], OmG[r], chol[v]))
    Lf = h["Kuu_chol_F"]
    for m in cfg["modality_names"]:
        OmF = orc.omega_from_sqrt(st[f"Omega_sqt_F_dict.{m}"])
        dF = st[f"delta_F_dict.{m}"]
        for l in range(OmF.shape[0]):
            terms.append(_mvn_kl(dF[:, l], OmF[l], Lf))
    return torch.stack(terms)


def _cast_state(inp, overrides=None, grads=True):
    st = {}
    for k, t in inp["state"].items():
        t = t.double().clone()
        if overrides is not None and k in overrides:
            t = overrides[k].double().clone()
        if grads and k.startswith(TRAINABLE):
            t.requires_grad_(True)
        st[k] = t
    return st


def reference_forward(case, inp, st):
    """oracle forward on the fp32 inputs cast up -> (outputs, handoff, kl [T])"""
    view_idx, Ns = orc.make_view_index({m: d["n_samples_list"] for m, d in inp["dd"].items()})
    X = {m: x.double() for m, x in inp["X"].items()}
    out, h = orc.forward_pass(st, inp["cfg"], X, view_idx, Ns, case.S, [e.double() for e in inp["eps_G"]],
                              {m: e.double() for m, e in inp["eps_F"].items()})
    return out, h, kl_terms(st, inp["cfg"], h)


def scalar_J(case, inp, out, kl):
    J = (inp["c"] * kl).sum()
    for m in case.mods:
        J = J + (inp["A"][m].double() * out["G_means"][m]).sum() + (inp["B"][m].double() * out["G_samples"][m]).sum()
    return J


def reference(case, inp):
    """-> dict(G_means, G_samples {m: fp64}, mu_z [V, Mx, D], kl [T], grads {name: fp64 or None})"""
    st = _cast_state(inp)
    out, h, kl = reference_forward(case, inp, st)
    J = scalar_J(case, inp, out, kl)
    leaves = {k: t for k, t in st.items() if t.requires_grad}
    gs = torch.autograd.grad(J, list(leaves.values()), allow_unused=True)
    return dict(G_means={m: t.detach() for m, t in out["G_means"].items()},
                G_samples={m: t.detach() for m, t in out["G_samples"].items()},
                mu_z=h["mu_z_G"].detach(), kl=kl.detach(), J=J.detach(),
                grads={k: (None if g is None else g.detach()) for k, g in zip(leaves, gs)})


def kappa(case, inp):
    """the largest 2-norm condition number among K_uu + 1e-5 I (free views, data GP) and Omega = A A^T + 1e-5 I"""
    st = _cast_state(inp, grads=False)
    cfg = inp["cfg"]
    mats = []
    for v in case.free:
        Lk = _prior_chol(st, cfg, v)
        mats.append(Lk @ Lk.t())
    kd = orc.KERNELS[cfg["kernel_data"]]
    G = st["Gtilde"]
    mats.append(kd(G, G, lengthscale_unconstrained=st["data_kernel_lengthscale"],
                   output_variance_unconstrained=st["data_kernel_variance"]) + orc.JITTER * torch.eye(G.shape[0], dtype=F64))
    mats += list(orc.omega_from_sqrt(st["Omega_sqt_G_list"]))
    for m in case.mods:
        mats += list(orc.omega_from_sqrt(st[f"Omega_sqt_F_dict.{m}"]))
    def cond(A):  # symmetric positive definite: the 2-norm condition number is the eigenvalues' ratio
        w = torch.linalg.eigvalsh(A)
        return float(w[-1] / w[0])

    return max(cond(A) for A in mats)


# ---------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------
def ratio32(got, ref, per_lead=False):
    """worst |got - ref| / (2^-23 |ref| + 2^-30 max|ref|), the max over the tensor or (per_lead) over each slice of the
    leading dimension; a slice whose reference is all zero must be exactly zero (ratio 0, else inf)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    if per_lead:
        g2, r2 = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    else:
        g2, r2 = got.reshape(1, -1), ref.reshape(1, -1)
    top = r2.abs().amax(1, keepdim=True)
    bound = U32 * r2.abs() + ABS32 * top
    err = (g2 - r2).abs()
    if not bool(torch.isfinite(g2).all()):
        return float("inf")
    rat = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(rat.max())


def ratio64(got, ref, rtol=KL_RTOL, abs_rel=0.0):
    """worst per-element |got - ref| / (rtol |ref| + abs_rel max|ref|) of an fp64 output; where the bound is exactly 0
    so must the error be"""
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    bound = rtol * ref.abs() + abs_rel * ref.abs().max()
    rat = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(rat.max()) if rat.numel() else 0.0


def ratio_to(got, ref, bound):
    """worst per-element |got - ref| / bound for an element-wise bound tensor (or number)"""
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref, dtype=F64)
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    bound = torch.as_tensor(bound, dtype=F64).expand_as(ref)
    err = (got - ref).abs()
    rat = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(rat.max())


PER_VIEW = ("Xtilde", "delta_G_list", "Omega_sqt_G_list", "warp_kernel_lengthscales", "warp_kernel_variances")
MUST_BE_ZERO = ("noise_variance", "W_dict.")


# ---------------------------------------------------------------------------------------------------------
# the stand-alone fp32 kernels' bounds: rounding count x 2^-24 x the magnitude rounded, derived next to the formula
# ---------------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24


def gamma(k):
    """k roundings compounded: k u / (1 - k u) (Higham's gamma_k), u = 2^-24"""
    return k * U24 / (1.0 - k * U24)


SQRT_ULPS = 2  # sqrtf / the fp32 division: at most 1 ulp = 2 u (HIP's documented accuracy; correctly rounded: 1 u)


def data_sample_fwd_bounds(meanT, v, q, var_u, eps):
    """data_sample_fwd_kernel in fp64 with its rounding points (fp32 inputs cast up; q fp64):
        resid = fl(exp(var_u) - q)                       1 rounding of |resid|
        Sigma = fl(fl(resid + v) + fl(2e-5))             + 1 of |resid + v| + 1 of 2e-5 + 1 of |Sigma|
        F     = fl(mean + fl(fl(sqrt(Sigma)) eps))       sqrt: dSigma / (2 sqrt Sigma) + 2 u sqrt Sigma; product 1; sum 1
    -> (F [C, L], Sigma [L, C], bound_F, bound_Sigma)"""
    meanT, v, q, eps = meanT.double(), v.double(), q.double(), eps.double()
    resid = (torch.exp(var_u.double()[0]) - q).unsqueeze(0)
    Sigma = resid + v + orc.JITTER * 2
    bS = gamma(1) * resid.abs() + gamma(1) * (resid + v).abs() + gamma(1) * 2e-5 + gamma(1) * Sigma.abs()
    bS = bS * (1 + gamma(3))  # the later roundings act on already rounded values
    root = torch.sqrt(Sigma)
    F = meanT.t() + root.t() * eps
    b_root = bS / (2 * root) + gamma(SQRT_ULPS) * root
    bF = eps.abs() * (b_root.t() + gamma(1) * root.t()) * (1 + gamma(2)) + gamma(1) * F.abs()
    bF = bF + gamma(1) * bF  # the final sum rounds a value that already carries bF
    return F, Sigma, bF, bS


def data_sample_bwd_bounds(dF, eps, Sigma, var_u):
    """data_sample_bwd_kernel from the SAME fp32 Sigma the kernel reads:
        g     = fl(fl(fl(dF eps) 0.5) / fl(sqrt Sigma))   product 1, halving exact, sqrt 2, division 2: 5 u |g|
        dmean = dF                                        exact
        qbar  = -sum_l g   fp32, a thread's chain of ceil(L / 8) terms, then 8 threads: depth ceil(L/8) + 7
        dvar  = fl(exp(var_u) sum g)  the threads' fp32 chains (depth ceil(L/8)), then fp64 sums, one rounding
    -> (g [L, C], qbar [C], dvar, bound_g, bound_qbar, bound_dvar)"""
    dF, eps, Sigma = dF.double(), eps.double(), Sigma.double()
    L = Sigma.shape[0]
    g = (dF * eps).t() * 0.5 / torch.sqrt(Sigma)
    bg = gamma(1 + 2 * SQRT_ULPS) * g.abs()
    chain = (L + 7) // 8
    qbar = -g.sum(0)
    bq = (gamma(1 + 2 * SQRT_ULPS) + gamma(chain + 7)) * g.abs().sum(0) * (1 + gamma(chain + 7))
    ev = float(torch.exp(var_u.double()[0]))
    dvar = ev * g.sum()
    bd = ev * (gamma(1 + 2 * SQRT_ULPS) + gamma(chain)) * float(g.abs().sum()) * (1 + gamma(chain)) + gamma(1) * abs(float(dvar))
    bd = bd * (1 + gamma(1))
    return g, qbar, dvar, bg, bq, bd


def adam_bounds(p, g, m, v, t, lr, b1, b2, eps):
    """adam_kernel (torch.optim.Adam's single-tensor update in fp32) in fp64 from the same fp32 state, step t -> t + 1:
        m' = fl(m + fl(fl(1 - b1) fl(g - m)))              3 roundings of |(1 - b1)(g - m)|, 1 of |m'|
        v' = fl(fl(fl(b2) v) + fl(fl(fl(1 - b2) g) g))     2 of |b2 v|, 3 of |(1 - b2) g^2|, 1 of |v'|
        den = fl(fl(fl(sqrt v') / fl(rs2)) + fl(eps))      sqrt: dv' / (2 sqrt v') + 2 u; rs2 1, division 2; eps 1; sum 1
        p' = fl(p - fl(fl(step) fl(m' / den)))             division 2, step 1, product 1 (relative), sum 1 of |p'|
    (a fused multiply-add rounds less often, never more) -> (p', m', v', bound_p, bound_m, bound_v)"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    tt = float(t) + 1.0
    w1, w2 = 1.0 - b1, 1.0 - b2
    m1 = m + w1 * (g - m)
    bm = gamma(3) * (w1 * (g - m)).abs() + gamma(1) * m1.abs()
    bm = bm * (1 + gamma(1))
    v1 = b2 * v + w2 * g * g
    bv = gamma(2) * (b2 * v).abs() + gamma(3) * (w2 * g * g).abs() + gamma(1) * v1.abs()
    bv = bv * (1 + gamma(1))
    rs2 = math.sqrt(1.0 - b2 ** tt)
    step = lr / (1.0 - b1 ** tt)
    root = torch.sqrt(v1)
    den = root / rs2 + eps
    b_root = bv / (2 * root) + gamma(SQRT_ULPS) * root
    b_den = (b_root / rs2 + gamma(1 + SQRT_ULPS) * root / rs2) * (1 + gamma(3)) + gamma(1) * eps + gamma(1) * den
    b_den = b_den * (1 + gamma(1))
    upd = step * (m1 / den)
    # the quotient's inherited error (first order in bm and b_den, their second order through den - b_den below)
    b_upd = step * (bm / (den - b_den) + m1.abs() * b_den / (den * (den - b_den))) + gamma(SQRT_ULPS + 2) * upd.abs()
    b_upd = b_upd * (1 + gamma(SQRT_ULPS + 2))
    p1 = p - upd
    bp = (b_upd + gamma(1) * p1.abs()) * (1 + gamma(1))
    return p1, m1, v1, bp, bm, bv
