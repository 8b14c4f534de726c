"""``predict``: what a user does after training - closed-form posterior moments and the held-out log density.

The reference class offers one route to a prediction: ``forward(..., prediction_mode=True, S=10)`` and the average of
the draws (experiments/expression/slideseq/slideseq_prediction.py:360-368).  That answers with noisy draws of a quantity
known in closed form, holds ``[S, N, L]`` draws of every row at once and returns neither a variance nor a score.  This
module closes the same layers as MOMENTS, row chunk by row chunk:

* warp GP, closed form per row: ``G_mean`` (what ``forward`` returns as ``G_means``) and ``G_scale``, the factor
  ``forward`` multiplies its standard-normal draw with (the conditional's variance used as a scale, rows ``v*D + j`` of
  the variational covariances: SURVEY quirks 1 and 2 are kept - ``predict`` describes the model that was trained).
  Rows of fixed views: ``G_mean = X``, ``G_scale = 0``.
* warp samples ``G_s = G_mean + G_scale * eps_s``, s = 1..S (``warp="mean"``: one sample with eps = 0, nothing drawn).
* per sample the data GP's conditional ``mu_s``, ``sigma2_s`` (vgpsa.py:174-204 with its ``+2e-5``, quirk 3) and per
  observed output ``m_s = mu_s W``, ``u_s = sigma2_s (W o W)`` (no LMC: ``m_s = mu_s``, ``u_s = sigma2_s``); with
  ``include_noise`` ``u_s += tau^2``, ``tau = noise_variance_pos[-n_modalities + i]`` used as a standard deviation
  (quirk 5, as ``loss_fn`` does).
* the mixture's moments (law of total variance): ``F_mean = mean_s m_s``, ``F_var = mean_s u_s + mean_s (m_s - F_mean)^2``
  and, with observations ``Y``, ``lpd[n] = sum_p log mean_s Normal(Y[n,p]; m_s[n,p], u_s[n,p] + tau^2)`` (always with the
  noise; NaN entries of ``Y`` contribute 0).

Count outputs (``model.likelihood``: a Poisson modality's draws are log rates): the fields above stay on the log-rate
scale.  ``scale="response"`` adds the prediction on the scale of the observations, ``Y_mean`` / ``Y_var``, under each
modality's own likelihood, and makes ``lpd`` that likelihood's held-out log density:

* Gaussian modality: ``Y_mean = F_mean``, ``Y_var = F_var`` with the noise ``tau^2`` in it whatever ``include_noise``
  says, ``lpd`` the closed form above.
* Poisson modality, per sample ``eta ~ Normal(mu, u)`` with ``mu = m_s + log_offset[n]``, ``u = u_s`` (never ``tau``):
  ``lam_s = exp(mu + u/2)``, ``Y_mean = mean_s lam_s``, ``Y_var = Y_mean + mean_s[lam_s^2 expm1(u)] + var_s(lam_s)`` and
  ``lpd[n] = sum_p log mean_s Int Poisson(y; e^eta) Normal(eta; mu, u) d eta`` (``gpsa_predict_counts_f32``).  The integral
  has no closed form: it is taken by ``len(GH_NODES)``-node Gauss-Hermite quadrature centred on the integrand's mode
  (``NEWTON_ITERATIONS`` Newton iterations).  Against a brute-force integral its error, as ``|error| / max(1, |value|)``,
  is 1.9e-10 for u <= 0.5, 2.0e-8 for u <= 1, 1.8e-6 for u <= 2 and 4.6e-5 for u <= 4 (tests/test_predict_counts.py);
  BEYOND u = 4 NOTHING IS MEASURED.  ``y`` is not validated (the formula is taken as written for any real y > -1, as
  in training; y <= -1 gives NaN);
  ``include_noise`` has no meaning for the ``Y_*`` of a Poisson modality.

Memory: the data stage handles ``c`` rows at a time - sample locations, covariance panel, projection, the two
contractions and ``gpsa_predict_moments_f32`` straight into the rows' slice of the results - so the peak beyond the
results is about ``S c (4 M + 8 L + 8 D)`` bytes plus a fixed fp64 covariance block (PROJECT_BLOCK columns) and the
M x M matrices (the L variational covariances in fp64 dominate: 8 L M^2), independent of N.
"""
import torch

from . import engine as E
from .models.vgpsa import _as_index

# Chunk budget of the data stage when neither ``rows_per_chunk`` nor ``workspace_gb`` is given.  Chosen at BASELINE
# config 2's size (2 x 10 000 rows, 50 outputs, M = 200, S = 10: 12.3 KB per row, so both views in one chunk), where
# tools/predict_timing.py measured 5.47 ms per call in one chunk against 5.90 / 6.54 ms in chunks of 5000 / 2000 rows.
DEFAULT_WORKSPACE_GB = 0.5

TWO_JITTER = 2e-5  # diagonal_offset added twice by the reference's conditional (quirk 3)

# The Gauss-Hermite rule of the Poisson-lognormal integral (scale="response"): (x_k, log w_k + x_k^2), Q = 20 nodes, and the
# number of Newton iterations for the integrand's mode.  The kernel (csrc/predict_counts.hip) carries the same literals;
# tests/test_predict_counts.py restates the rule in numpy from THESE and holds it against a brute-force integral.
GH_NODES = (
    (-5.387480890011233, -0.10692622802020324),
    (-4.603682449550744, -0.35050407841539055),
    (-3.944764040115625, -0.4743672219775181),
    (-3.3478545673832163, -0.5529289199616052),
    (-2.7888060584281305, -0.6072415536850873),
    (-2.2549740020892757, -0.6461102649118216),
    (-1.7385377121165861, -0.6739741099862373),
    (-1.234076215395323, -0.6933054504113765),
    (-0.7374737285453944, -0.7055368459223146),
    (-0.24534070830090124, -0.7114710404116901),
    (0.24534070830090124, -0.7114710404116901),
    (0.7374737285453944, -0.7055368459223146),
    (1.234076215395323, -0.6933054504113765),
    (1.7385377121165861, -0.6739741099862373),
    (2.2549740020892757, -0.6461102649118216),
    (2.7888060584281305, -0.6072415536850873),
    (3.3478545673832163, -0.5529289199616052),
    (3.944764040115625, -0.4743672219775181),
    (4.603682449550744, -0.35050407841539055),
    (5.387480890011233, -0.10692622802020324),
)
NEWTON_ITERATIONS = 8


class Prediction(dict):
    """one modality's result: a dict whose entries also read as attributes (``G_mean``, ``G_scale``, ``F_mean``, ``F_var``,
    ``F_latent_mean``, ``F_latent_var``, ``lpd``, ``lpd_sum``; None where not asked for; with ``scale="response"`` also
    ``Y_mean``, ``Y_var``)"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def _fixed_splitk(k):
    """the split of a mean product's M-long reduction, from M alone: ops.gemm's own choice also looks at the number of
    columns, which would make a row's value depend on the chunk it was computed in"""
    return min(4, k // 48) if 128 <= k <= 1024 else 1


def rows_for_budget(workspace_gb, S, M, L, D):
    """rows per chunk that keep the data stage's panels inside ``workspace_gb``"""
    per_row = S * (4 * M + 8 * L + 8 * D + 16)
    c = int(workspace_gb * 2**30) // per_row
    return max(32, c // 32 * 32)


def _check_rows(name, m, t, want):
    if t.dim() != len(want) or tuple(t.shape) != tuple(want):
        raise ValueError(f"{name}[{m!r}] has shape {tuple(t.shape)}, the views' row counts give {tuple(want)}")


PROJECT_BLOCK = 8192  # columns of the fp64 covariance panel alive at a time inside a chunk


def _project_blocks(model, o, fac, Z, Gf, ls_u, var_u):
    """alpha = K_uu^-1 k(Z, Gf) [M, C] fp32 and q [C] fp64 of a chunk's C sample locations.  The fp64 covariance panel
    (8 M bytes per column, the largest thing a chunk needs) exists for PROJECT_BLOCK columns at a time; a column's
    arithmetic does not depend on the block it is in."""
    Cn = Gf.shape[0]
    if Cn <= PROJECT_BLOCK:
        return E._project(o, fac, model._kmat("data", Z, Gf, ls_u, var_u, 0.0, torch.float64, False), torch.float32)
    alpha = torch.empty(Z.shape[0], Cn, dtype=torch.float32, device=Gf.device)
    q = torch.empty(Cn, dtype=torch.float64, device=Gf.device)
    for a in range(0, Cn, PROJECT_BLOCK):
        Kuf = model._kmat("data", Z, Gf[a: a + PROJECT_BLOCK], ls_u, var_u, 0.0, torch.float64, False)
        al, qb = E._project(o, fac, Kuf, torch.float32)
        del Kuf
        alpha[:, a: a + PROJECT_BLOCK] = al
        q[a: a + PROJECT_BLOCK] = qb
    return alpha, q


@torch.no_grad()
def predict(model, X_spatial=None, view_idx=None, Ns=None, *, S=10, warp="sample", G_test=None, Y=None,
            include_noise=False, latent=False, eps_G=None, generator=None, rows_per_chunk=None, workspace_gb=None,
            scale="link", log_offset=None):
    """Posterior moments of ``model`` (a VariationalGPSA) at its own rows or at ``G_test``; see the module docstring.

    X_spatial {mod: [N, D]}, view_idx, Ns: as ``forward`` takes them (view_idx / Ns default to the model's own).
    G_test {mod: [n_test, D]} (or [S_t, n_test, D]: S_t samples of the locations): points already in the aligned system;
        the data GP is then evaluated THERE and not on the rows of ``X_spatial``, which may be omitted (given, it still
        yields ``G_mean`` / ``G_scale``).
    Y {mod: [N, P]} (at ``G_test``'s rows when that is given): adds ``lpd`` [N] fp64 and ``lpd_sum``.
        Refused (ValueError), like ``scale="response"``, when a modality has a negative binomial likelihood: it has no
        count-scale prediction yet (its ``F_mean`` / ``F_var``, the moments of the log mean, are there).
        With ``scale="link"`` refused (ValueError) when a modality has a Poisson likelihood (``model.likelihood``): its
        ``F_mean`` / ``F_var`` are the moments of the log rate, and the Gaussian closed form of ``lpd`` does not apply to
        counts; ``scale="response"`` scores them.
    scale: ``"link"`` (default): the fields above and nothing else.  ``"response"``: every Prediction also carries
        ``Y_mean`` / ``Y_var`` [N, P] fp32, the prediction on the scale of the observations under the modality's own
        likelihood, and ``lpd`` is that likelihood's (module docstring; a Poisson modality's integral is measured for
        u <= 4 only).  ``F_*`` and ``G_*`` do not change.
    log_offset {mod: [N] fp32} (at ``G_test``'s rows when that is given; only with ``scale="response"``): per-row offsets of
        a Poisson modality's log rate, as ``loss_fn`` takes them in ``data_dict[m]["log_offset"]``.  Absent: 0.
    eps_G: the warp draws, a list over the non-fixed, non-empty views in order, each [S, n_v, D] (``inject_noise``'s
        layout); otherwise they come from ``generator`` or the device's default generator.
    rows_per_chunk / workspace_gb: the data stage's chunk, directly or as a budget (default DEFAULT_WORKSPACE_GB).

    Returns {mod: Prediction}.  Runs without gradients and leaves the model as it found it: no ``eval()``, nothing of the
    forward -> loss_fn hand-off, no injected noise consumed, the training generators untouched.  ``model.contraction`` is
    ignored: the bf16x3 kernels are ELBO / Gram kernels, the no-keep product here is the fp32 one.
    """
    if warp not in ("sample", "mean"):
        raise ValueError(f"warp must be 'sample' or 'mean', not {warp!r}")
    if int(S) != S or S < 1:
        raise ValueError(f"S must be a positive integer, not {S!r}")
    if X_spatial is None and G_test is None:
        raise ValueError("predict needs X_spatial (rows to align and predict) or G_test (aligned locations)")
    if warp == "mean" and eps_G is not None:
        raise ValueError("eps_G was given with warp='mean', which draws nothing")
    if scale not in ("link", "response"):
        raise ValueError(f"scale must be 'link' or 'response', not {scale!r}")
    S = 1 if warp == "mean" else int(S)
    response = scale == "response"
    pois = {m: getattr(model, "likelihood_of", lambda _m: "gaussian")(m) == "poisson" for m in model.modality_names}
    for m in model.modality_names:
        # a negative binomial modality has no count-scale prediction yet (it would otherwise take the Gaussian branch)
        if getattr(model, "likelihood_of", lambda _m: "gaussian")(m) == "negative_binomial" and (response or Y is not None):
            raise ValueError(f"predict: modality {m!r} has a negative binomial likelihood, which has no count-scale "
                             "prediction yet: scale=\"response\" and Y (lpd) are not available for it; the link-scale "
                             "fields (F_mean / F_var: the moments of its log mean) are - call predict with "
                             "scale=\"link\" and without Y")
    if Y is not None and not response:
        for m in model.modality_names:
            if pois[m]:
                raise ValueError(f"predict: Y was given, but modality {m!r} has a Poisson likelihood: lpd is the Gaussian "
                                 "closed form and does not apply to counts (F_mean / F_var are the moments of its log "
                                 "rate; call predict without Y, or with scale=\"response\" for the counts' own moments "
                                 "and log density)")
    if log_offset is not None:
        if not response:
            raise ValueError("predict: log_offset was given with scale='link'; offsets act on the counts' scale only "
                             "(scale=\"response\")")
        for m in log_offset:
            if m not in pois:
                raise ValueError(f"predict: log_offset names the modality {m!r}; the model has {list(pois)}")
            if log_offset[m] is not None and not pois[m]:
                raise ValueError(f"predict: log_offset[{m!r}] was given, but modality {m!r} has a Gaussian likelihood "
                                 "(offsets belong to a Poisson modality: model.likelihood)")
    o = E.ops()
    dev = model.Xtilde.device
    mods = model.modality_names
    V, D = model.n_views, model.n_spatial_dims
    f64, f32 = torch.float64, torch.float32
    wide = lambda t: t.detach().double() if t.dtype == f32 else t.detach()
    nm = len(mods)

    # ---- arguments against the views' row counts ----------------------------------------------------------------------
    rows_of, N = None, {}
    if X_spatial is not None:
        view_idx = model.view_idx if view_idx is None else view_idx
        rows_of = {v: {m: _as_index(view_idx[m][v], dev) for m in mods} for v in range(V)}
        for m in mods:
            N[m] = int(Ns[m]) if Ns is not None else sum(rows_of[v][m][1] for v in range(V))
            _check_rows("X_spatial", m, X_spatial[m], (N[m], D))
    Gt = None
    if G_test is not None:
        Gt = {}
        for m in mods:
            g = G_test[m].to(device=dev, dtype=f64)
            if g.dim() == 2:
                g = g.unsqueeze(0)
            if g.dim() != 3 or g.shape[2] != D or g.shape[0] < 1:
                raise ValueError(f"G_test[{m!r}] has shape {tuple(G_test[m].shape)}: [n_test, {D}] or "
                                 f"[S_t, n_test, {D}] is needed")
            Gt[m] = g
    n_out = {m: (int(Gt[m].shape[1]) if Gt is not None else N[m]) for m in mods}
    P = {m: int(model.Ps[m]) for m in mods}
    Lm = {m: int(model.n_latent_outputs[m]) for m in mods}
    if Y is not None:
        for m in mods:
            _check_rows("Y", m, Y[m], (n_out[m], P[m]))
    if log_offset is not None:
        for m, t in log_offset.items():
            if t is not None:
                _check_rows("log_offset", m, t, (n_out[m],))
    free = [v for v in range(V) if not model._is_fixed(v)]
    nonempty = [v for v in free if rows_of is not None and sum(rows_of[v][m][1] for m in mods) > 0]
    sampled = warp == "sample" and Gt is None
    if eps_G is not None:
        if len(eps_G) != len(nonempty):
            raise ValueError(f"eps_G has {len(eps_G)} entries, the non-fixed views with rows are {len(nonempty)}")
        for e, v in zip(eps_G, nonempty):
            n_v = sum(rows_of[v][m][1] for m in mods)
            if tuple(e.shape) != (S, n_v, D):
                raise ValueError(f"eps_G of view {v} has shape {tuple(e.shape)}, the views' row counts give "
                                 f"({S}, {n_v}, {D})")

    # ---- everything M x M, once per call: prior factorisations and the variational covariances --------------------------
    Xt = wide(model.Xtilde)
    Gt64 = wide(model.Gtilde)
    dls, dvar = wide(model.data_kernel_lengthscale), wide(model.data_kernel_variance)
    jit = model.diagonal_offset
    Kuu = [model._kmat("warp", Xt[v], Xt[v], wide(model.warp_kernel_lengthscales[v]),
                       wide(model.warp_kernel_variances[v]), jit, f64, True) for v in nonempty]
    Kuu.append(model._kmat("data", Gt64, Gt64, dls, dvar, jit, f64, True))
    parts = E.factor_batch([k.unsqueeze(0) for k in Kuu])
    fac_w = {v: E.Factor(parts=parts[i]) for i, v in enumerate(nonempty)}
    fac_F = E.Factor(parts=parts[len(nonempty)])
    flags = [p[3].reshape(-1) for p in parts]
    Mx, Mg = int(Xt.shape[1]), int(Gt64.shape[0])

    # ---- warp stage: closed form per (view, modality) block, all fp64 -----------------------------------------------------
    G_mean64 = G_scale64 = None
    if rows_per_chunk is not None:  # the same number of columns per launch as the data stage
        cw = max(1, int(rows_per_chunk) * S // 2)  # (the warp panels are fp64: half the columns, about the same bytes)
    else:
        cw = rows_for_budget(DEFAULT_WORKSPACE_GB if workspace_gb is None else workspace_gb, 1, 4 * Mx, D, D)
    if X_spatial is not None:
        nan = float("nan")
        G_mean64 = {m: torch.full([N[m], D], nan, dtype=f64, device=dev) for m in mods}
        G_scale64 = {m: torch.full([N[m], D], nan, dtype=f64, device=dev) for m in mods}
        for v in range(V):
            if not model._is_fixed(v):
                continue
            for m in mods:  # vgpsa.py:262-273
                r, cnt = rows_of[v][m]
                if cnt:
                    G_mean64[m][r] = X_spatial[m][r].to(f64)
                    G_scale64[m][r] = 0.0
        for v in nonempty:
            Z = Xt[v]
            ls_u, var_u = wide(model.warp_kernel_lengthscales[v]), wide(model.warp_kernel_variances[v])
            slopes, icpt = model.mean_slopes[v].detach(), model.mean_intercepts[v].detach()
            _, dc = o.mean_resid_fwd(Z, slopes, icpt, model.delta_G_list[v].detach(), 1.0)
            Om = E.OmegaFn.apply(model.Omega_sqt_G_list[v * D: v * D + D].detach())  # quirk 2: rows v*D + j
            var0 = torch.exp(var_u.reshape(()))
            for m in mods:
                r, cnt = rows_of[v][m]
                if cnt == 0:
                    continue
                Xv = X_spatial[m][r].to(f64)
                for a in range(0, cnt, cw):
                    Xc = Xv[a: a + cw].contiguous()
                    Kuf = model._kmat("warp", Z, Xc, ls_u, var_u, 0.0, f64, False)
                    alpha, q = E._project(o, fac_w[v], Kuf, f64)
                    del Kuf
                    meanT = o.gemm(dc, alpha, transA=True, splitk=_fixed_splitk(Mx))  # [D, n]
                    vq = o.quadform_fwd(alpha, Om)
                    mean = Xc @ slopes.to(f64) + icpt.to(f64) + meanT.t()
                    scale = (var0 - q).unsqueeze(1) + vq.t() + TWO_JITTER  # the variance, used as a scale: quirk 1
                    flags.append((~(scale > 0)).any().to(torch.int32).reshape(1))
                    if isinstance(r, slice):
                        G_mean64[m][r.start + a: r.start + a + Xc.shape[0]] = mean
                        G_scale64[m][r.start + a: r.start + a + Xc.shape[0]] = scale
                    else:
                        G_mean64[m][r[a: a + cw]] = mean
                        G_scale64[m][r[a: a + cw]] = scale
    if model.check_numerics and int(torch.cat(flags).max()) != 0:
        raise torch.linalg.LinAlgError(
            "GPSA predict: an inducing-point covariance is not positive-definite or a warp scale is not positive "
            "(forward raises here too)")

    # ---- the warp draws, per modality [S, N, D] (the draw order of vgpsa.py:346-348) ---------------------------------------
    eps = None
    if sampled:
        eps = {m: torch.zeros(S, N[m], D, dtype=f32, device=dev) for m in mods}
        for i, v in enumerate(nonempty):
            n_v = sum(rows_of[v][m][1] for m in mods)
            if eps_G is not None:
                e = eps_G[i].to(device=dev, dtype=f32)
            else:
                e = torch.empty(S, n_v, D, dtype=f32, device=dev).normal_(generator=generator)
            a = 0
            for m in mods:
                r, cnt = rows_of[v][m]
                if cnt:
                    eps[m][:, r] = e[:, a: a + cnt]
                a += cnt

    # ---- data stage in row chunks ----------------------------------------------------------------------------------------
    res = {}
    var32 = model.data_kernel_variance.detach().float().reshape(1)
    nz = model.noise_variance.detach()
    for i, m in enumerate(mods):
        n, L = n_out[m], Lm[m]
        S_m = int(Gt[m].shape[0]) if Gt is not None else S
        if rows_per_chunk is not None:
            c = max(1, int(rows_per_chunk))
        else:
            c = rows_for_budget(DEFAULT_WORKSPACE_GB if workspace_gb is None else workspace_gb, S_m, Mg, L, D)
        lmc = model.n_latent_gps[m] is not None
        W = model.W_dict[m].detach() if lmc else None
        noise_u = nz[nz.numel() - nm + i]  # quirk 5: the LAST n_modalities entries
        dcT = model.delta_F_dict[m].detach().to(f32).contiguous()
        Om_F = E.OmegaFn.apply(model.Omega_sqt_F_dict[m].detach())  # [L, M, M] fp64, alive for this modality's chunks
        new = lambda *sh, dt=f32: torch.empty(*sh, dtype=dt, device=dev)
        Fm, Fv = new(n, P[m]), new(n, P[m])
        Flm, Flv = (new(n, L), new(n, L)) if latent else (None, None)
        lpd = new(n, dt=f64) if Y is not None else None
        Ym = None if Y is None else Y[m].to(device=dev, dtype=f32).contiguous()
        counts = response and pois[m]  # the Gaussian closing then leaves lpd alone: the counts' closing writes it
        Cm, Cv = (new(n, P[m]), new(n, P[m])) if counts else (None, None)
        off = None if not counts or log_offset is None or log_offset.get(m) is None else \
            log_offset[m].to(device=dev, dtype=f32).contiguous()
        for a in range(0, n, c):
            b = min(n, a + c)
            if Gt is not None:
                loc = Gt[m][:, a:b]
            elif sampled:
                loc = G_mean64[m][a:b].unsqueeze(0) + G_scale64[m][a:b].unsqueeze(0) * eps[m][:, a:b].to(f64)
            else:
                loc = G_mean64[m][a:b].unsqueeze(0)
            Gf = loc.reshape(S_m * (b - a), D).contiguous()  # column s*c + r
            alpha, q = _project_blocks(model, o, fac_F, Gt64, Gf, dls, dvar)
            meanT = o.gemm(dcT, alpha, transA=True, splitk=_fixed_splitk(Mg))
            vq = o.quadform_fwd(alpha, Om_F)
            cut = lambda t: None if t is None else t[a:b]
            o.predict_moments(meanT, vq, q, var32, S_m, W=W, noise_u=noise_u, include_noise=include_noise,
                              Y=None if counts else cut(Ym), latent=latent,
                              out=(Fm[a:b], Fv[a:b], cut(Flm), cut(Flv), None if counts else cut(lpd)))
            if counts:
                o.predict_counts(meanT, vq, q, var32, S_m, W=W, log_offset=cut(off), Y=cut(Ym),
                                 out=(Cm[a:b], Cv[a:b], cut(lpd)))
            del alpha, meanT, vq, q
        del Om_F
        if response and not counts:  # Gaussian: the observation's moments are the field's, with the noise
            tau = torch.exp(noise_u.double()) + 1e-5  # vgpsa.py:217; a standard deviation (quirk 5)
            Cm, Cv = Fm.clone(), Fv.clone() if include_noise else (Fv.double() + tau * tau).to(f32)  # (no aliases)
        res[m] = Prediction(
            G_mean=None if G_mean64 is None else G_mean64[m].to(f32),
            G_scale=None if G_scale64 is None else G_scale64[m].to(f32),
            F_mean=Fm, F_var=Fv, F_latent_mean=Flm, F_latent_var=Flv, lpd=lpd,
            lpd_sum=None if lpd is None else lpd.sum())
        if response:
            res[m]["Y_mean"], res[m]["Y_var"] = Cm, Cv
    return res
