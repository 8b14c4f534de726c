"""Rigid pre-registration of slices on the device: which rotation, reflection and shift puts slice B on slice A.

The warp's mean starts at the identity and its prior pulls towards it, so a slice that arrives turned by 83 degrees or
mirrored never aligns, and the reference's experiment scripts undo such poses by hand before they build ``data_dict``:
``angle = 1.45`` in experiments/expression/slideseq/slideseq_alignment.py:122-131 (and the three scripts beside it),
``rotate_90deg_counterclockwise`` three times "manually" in macosko_alignment/two_slice_alignment.py.  Here the pose is
searched: every candidate transform takes B's spots onto A, each spot is matched to its nearest spot of A within
``max_dist``, and the candidate's score is the mean squared expression difference over the matched pairs,

    J = sse / (n_matched P)   where n_matched >= min_overlap n,   +inf otherwise.

``rigid_scores`` is the raw table (one HIP entry, csrc/register.hip: ``gpsa_rigid_scores_f64`` scans 8 candidates per
pass over A's spots); ``rigid_register`` is a coarse grid over angle x reflection x shift followed by ``levels`` rounds
of halving refinement; ``prealign_slices`` registers every view of a stacked data set onto a reference view - the call
that replaces the hand rotation in front of ``data_dict``.

The candidate tables are built on the host from a handful of Python floats (a few hundred rows), the scores are read
back once per level, everything else stays on the device.  The neighbours are exact and ties go to the lower index, the
sums are fixed-order fp64: the result does not depend on ``candidates_per_chunk``, bit for bit.  Everything runs under
``torch.no_grad()``; D = 2 only (a 3-D stack is registered slice by slice in its plane); tensors on the CPU are refused.
"""
import math

import torch

from ._args import as_device, describe, on_device, require_finite, values, view_counts, view_offsets
from ._args import ops as _ops
from .predict import Prediction

f64, f32 = torch.float64, torch.float32
INF = float("inf")
NOT_FINITE = "{name} has {count} entries that are NaN or infinite; drop those spots first"
REFINE_ANGLE_OFFSETS = (-1, 0, 1)
REFINE_SHIFT_OFFSETS = (-2, -1, 0, 1, 2)


class RigidRegistration(Prediction):
    """The result of ``rigid_register``; entries also read as attributes.

    ``R`` [2, 2], ``t`` [2] fp64 on the device with ``aligned = XB @ R.T + t``; ``angle`` (radians, counter-clockwise),
    ``reflected`` (the rotation follows a flip of the second axis: ``R = rot(angle) @ diag(1, -1)``); ``score`` = J of
    the returned transform, ``score_start`` = J of the centroid match at angle 0, ``score_coarse`` = J of the coarse
    winner; ``n_matched``; ``coarse_scores`` [reflection, angle, shift, shift] fp64; ``path`` = [(chosen index, J)] per
    refinement level; ``runner_up`` = (angle, reflected, J) of the best coarse candidate more than two coarse angle
    steps away from the winner or with the other reflection (None where there is none) - a symmetric tissue shows here
    as a score close to the winner's; ``spacing`` (median nearest-neighbour distance inside A), ``max_dist``; ``nn``
    [n] int32 = the row of A nearest each row of B under the returned transform, ``matched`` [n] bool."""

    def apply(self, X):
        """``X @ R.T + t`` for any [*, 2] points on R's device"""
        if not torch.is_tensor(X) or X.dim() != 2 or X.shape[1] != 2:
            shape = tuple(X.shape) if torch.is_tensor(X) else type(X).__name__
            raise ValueError(f"RigidRegistration.apply: X has shape {shape}; [n, 2] is needed")
        return X.detach().to(device=self.R.device, dtype=f64) @ self.R.T + self.t


# ------------------------------------------------------------------------------------------------------------------------
# argument checks (all of them before any device work)
# ------------------------------------------------------------------------------------------------------------------------
def _slice_args(XA, YA, XB, YB, what):
    for name, t in (("XA", XA), ("XB", XB)):
        if not torch.is_tensor(t) or t.dim() != 2 or not t.is_floating_point() or t.shape[0] < 1:
            raise ValueError(f"{what}: {name} has shape {describe(t)}; a floating-point [n >= 1, 2] is needed")
        if t.shape[1] != 2:
            raise ValueError(f"{what}: {name} has D = {int(t.shape[1])} coordinates; the candidates are transforms of the "
                             "plane (D = 2) - a 3-D stack is registered slice by slice in its plane")
    values(YA, "YA", what, int(XA.shape[0]))
    values(YB, "YB", what, int(XB.shape[0]))
    if YA.shape[1] != YB.shape[1]:
        raise ValueError(f"{what}: YA has P = {int(YA.shape[1])} outputs and YB P = {int(YB.shape[1])}: the two slices "
                         "must carry the same outputs, in the same order")


def _positive_int(v, name, what, least=1):
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError(f"{what}: {name} must be an integer >= {least}, not {v!r}")
    return v


def _per_chunk(candidates_per_chunk, K, n, what):
    if candidates_per_chunk is None:
        c = 2**22 // max(n, 1)  # tables of at most 2^22 (candidate, row) pairs: 48 MB of scratch
        return max(1, min(K, c // 8 * 8 if c >= 8 else c))  # whole groups of the 8 candidates a thread carries
    return _positive_int(candidates_per_chunk, "candidates_per_chunk", what)


def _device_args(XA, YA, XB, YB):
    return as_device(XA, f64), as_device(YA, f32), as_device(XB, f64), as_device(YB, f32)


# ------------------------------------------------------------------------------------------------------------------------
# the raw table
# ------------------------------------------------------------------------------------------------------------------------
def _scores(o, XA, YA, XB, YB, T, max_d2, per_chunk, return_nn):
    """the entry over chunks of T's rows -> (sse [K], n_matched [K], d2_sum [K], nn [K, n] | None, d2 [K, n] | None)"""
    K = int(T.shape[0])
    if per_chunk >= K:
        return o.rigid_scores(XA, YA, XB, YB, T, max_d2, return_nn=return_nn)
    parts = [o.rigid_scores(XA, YA, XB, YB, T[a: a + per_chunk], max_d2, return_nn=return_nn)
             for a in range(0, K, per_chunk)]
    return tuple(torch.cat([p[q] for p in parts]) if parts[0][q] is not None else None for q in range(5))


@torch.no_grad()
def rigid_scores(XA, YA, XB, YB, transforms, max_dist, return_nn=False, candidates_per_chunk=None):
    """The score table of ``transforms`` [K, 6] (per row R row-major, then t): B's spots ``XB`` [n, 2] are taken to
    ``R x + t``, each is matched to its nearest spot of ``XA`` [m, 2] where that is within ``max_dist``, and the matched
    pairs are compared on ``YB`` [n, P] / ``YA`` [m, P].

    Returns a ``Prediction``: ``sse`` [K] fp64 (sum over matched pairs and outputs of the squared difference),
    ``n_matched`` [K] int64, ``d2_sum`` [K] fp64 (sum of the matched squared distances); with ``return_nn`` also ``nn``
    [K, n] int32 (the nearest row of A, by the key (squared distance, index)) and ``d2`` [K, n] fp64.  Coordinates are
    taken to fp64, outputs to fp32.  ``candidates_per_chunk``: rows of the table per launch (default: as many as keep
    the neighbour tables within 2^22 entries, 48 MB); the result does not depend on it, bit for bit."""
    what = "rigid_scores"
    _slice_args(XA, YA, XB, YB, what)
    if not torch.is_tensor(transforms) or transforms.dim() != 2 or transforms.shape[0] < 1 or transforms.shape[1] != 6 \
            or not transforms.is_floating_point():
        raise ValueError(f"{what}: transforms has shape {describe(transforms)}; a floating-point [K >= 1, 6] (R row-major, "
                         "then t) is needed")
    max_dist = float(max_dist)
    if not (0.0 <= max_dist < INF):
        raise ValueError(f"{what}: max_dist must be finite and >= 0, not {max_dist}")
    K, n = int(transforms.shape[0]), int(XB.shape[0])
    c = _per_chunk(candidates_per_chunk, K, n, what)
    # ("neighbour": the noun these calls' device refusal has carried since they shared neighbors' check; kept as it reads)
    on_device(what, "neighbour", XA=XA, YA=YA, XB=XB, YB=YB, transforms=transforms)
    XA, YA, XB, YB = _device_args(XA, YA, XB, YB)
    T = as_device(transforms, f64)
    sse, n_matched, d2_sum, nn, d2 = _scores(_ops(), XA, YA, XB, YB, T, max_dist * max_dist, c, return_nn)
    return Prediction(sse=sse, n_matched=n_matched, d2_sum=d2_sum, nn=nn, d2=d2)


# ------------------------------------------------------------------------------------------------------------------------
# the search
# ------------------------------------------------------------------------------------------------------------------------
def _row(theta, refl, sx, sy, cA, cB):
    """the row of T of: flip the second axis where ``refl``, turn by theta about B's centroid, move that centroid onto
    A's, shift by (sx, sy)"""
    c, s = math.cos(theta), math.sin(theta)
    sg = -1.0 if refl else 1.0
    r00, r01, r10, r11 = c, -s * sg, s, c * sg
    t0 = cA[0] + sx - (r00 * cB[0] + r01 * cB[1])
    t1 = cA[1] + sy - (r10 * cB[0] + r11 * cB[1])
    return [r00, r01, r10, r11, t0, t1]


def _shift_grid(n_shifts, half):
    """n_shifts values spanning [-half, half] (one value: 0)"""
    if n_shifts == 1:
        return [0.0]
    return [-half + 2.0 * half * q / (n_shifts - 1) for q in range(n_shifts)]


def _first_argmin(values):
    best = 0
    for q, v in enumerate(values):
        if v < values[best]:
            best = q
    return best


def _J(sse, n_matched, n, P, min_overlap):
    nm = n_matched.to(f64)
    return torch.where(nm >= min_overlap * n, sse / (nm * P), torch.full_like(sse, INF))


@torch.no_grad()
def rigid_register(XA, YA, XB, YB, *, n_angles=360, reflection=True, n_shifts=1, shift_extent=0.25, max_dist=None,
                   min_overlap=0.5, levels=6, candidates_per_chunk=None):
    """Register slice B (``XB`` [n, 2], ``YB`` [n, P]) onto slice A (``XA`` [m, 2], ``YA`` [m, P]) by a rotation, an
    optional reflection and a shift -> ``RigidRegistration``.

    spacing = the median nearest-neighbour distance inside A (the lower of the two middle values); ``max_dist`` defaults
    to 3 spacings.  Coarse stage: angles ``2 pi a / n_angles``, reflection off / on (``R diag(1, -1)``), shifts on an
    ``n_shifts x n_shifts`` grid spanning ``+- shift_extent`` times A's extent per axis (default: none), the rotation
    about B's centroid, which is moved onto A's centroid; candidate index = ((reflection, angle), shift x, shift y) in
    that nesting.  The winner is the smallest J, ties to the lowest index.  Refinement, levels l = 1 .. ``levels``: 75
    candidates - the current best first, then angle offsets {-1, 0, 1} x shift offsets {-2 .. 2}^2 (in that nesting,
    without the all-zero one) in steps of ``(2 pi / n_angles) / 2^l`` and ``spacing / 2^(l - 1)``; J never rises.

    Raises ValueError for D != 2, a P mismatch, non-finite input, and where no coarse candidate matches
    ``min_overlap`` of B's spots within ``max_dist``."""
    what = "rigid_register"
    _slice_args(XA, YA, XB, YB, what)
    _positive_int(n_angles, "n_angles", what)
    _positive_int(n_shifts, "n_shifts", what)
    _positive_int(levels, "levels", what, least=0)
    if not 0.0 < float(min_overlap) <= 1.0:
        raise ValueError(f"{what}: min_overlap must be in (0, 1], not {min_overlap!r}")
    if not 0.0 <= float(shift_extent) < INF:
        raise ValueError(f"{what}: shift_extent must be finite and >= 0, not {shift_extent!r}")
    if max_dist is not None and not 0.0 < float(max_dist) < INF:
        raise ValueError(f"{what}: max_dist must be finite and > 0, not {max_dist!r}")
    m, n, P = int(XA.shape[0]), int(XB.shape[0]), int(YA.shape[1])
    if m < 2:
        raise ValueError(f"{what}: XA has {m} row; the spacing of A needs two spots")
    refls = (False, True) if reflection else (False,)
    K = len(refls) * n_angles * n_shifts * n_shifts
    c = _per_chunk(candidates_per_chunk, K + 1, n, what)
    on_device(what, "neighbour", XA=XA, YA=YA, XB=XB, YB=YB)
    XA, YA, XB, YB = _device_args(XA, YA, XB, YB)
    require_finite(what, NOT_FINITE, XA=XA, YA=YA, XB=XB, YB=YB)
    o, dev = _ops(), XA.device

    # one host read: the spacing, the centroids, A's extent
    _, d2 = o.knn(XA, XA, 1, exclude_self=True)
    nearest = d2[:, 0].sqrt()
    stats = torch.cat([nearest.sort().values[(m - 1) // 2].reshape(1), XA.mean(0), XB.mean(0),
                       XA.amax(0) - XA.amin(0)]).tolist()
    spacing, cA, cB, ext = stats[0], stats[1:3], stats[3:5], stats[5:7]
    max_dist = 3.0 * spacing if max_dist is None else float(max_dist)
    if not 0.0 < max_dist < INF:
        raise ValueError(f"{what}: max_dist = {max_dist} (3 spacings of A, spacing = {spacing}); A's spots coincide - "
                         "pass max_dist")
    max_d2 = max_dist * max_dist
    table = lambda rows: torch.tensor(rows, dtype=f64, device=dev)

    def score(rows):
        sse, nm, _, _, _ = _scores(o, XA, YA, XB, YB, table(rows), max_d2, c, False)
        return _J(sse, nm, n, P, float(min_overlap))

    # the coarse stage (and, as the last row, the centroid match at angle 0: score_start)
    gx, gy = _shift_grid(n_shifts, shift_extent * ext[0]), _shift_grid(n_shifts, shift_extent * ext[1])
    step = 2.0 * math.pi / n_angles
    params = [(a * step, f, sx, sy) for f in refls for a in range(n_angles) for sx in gx for sy in gy]
    rows = [_row(th, f, sx, sy, cA, cB) for th, f, sx, sy in params] + [_row(0.0, False, 0.0, 0.0, cA, cB)]
    J = score(rows)
    Jh = J.tolist()  # host read
    score_start, Jh = Jh[K], Jh[:K]
    win = _first_argmin(Jh)
    if not Jh[win] < INF:
        raise ValueError(f"{what}: none of the {K} coarse candidates matches min_overlap = {min_overlap} of B's {n} spots "
                         f"within max_dist = {max_dist} of a spot of A (spacing {spacing}); raise max_dist, lower "
                         "min_overlap or add shifts (n_shifts)")
    theta, refl, sx, sy = params[win]
    best = Jh[win]
    # the runner-up: another reflection, or more than two coarse steps away on the circle
    a_win, per_angle = (win // (n_shifts * n_shifts)) % n_angles, n_shifts * n_shifts
    runner = None
    for q, v in enumerate(Jh):
        a_q, f_q = (q // per_angle) % n_angles, params[q][1]
        gap = min((a_q - a_win) % n_angles, (a_win - a_q) % n_angles)
        if (f_q != refl or gap > 2) and (runner is None or v < Jh[runner]):
            runner = q
    runner_up = None if runner is None else (params[runner][0], params[runner][1], Jh[runner])

    path = []
    for level in range(1, levels + 1):
        da, ds = step / 2.0**level, spacing / 2.0 ** (level - 1)
        cand = [(theta, sx, sy)] + [(theta + qa * da, sx + qx * ds, sy + qy * ds) for qa in REFINE_ANGLE_OFFSETS
                                    for qx in REFINE_SHIFT_OFFSETS for qy in REFINE_SHIFT_OFFSETS if (qa, qx, qy) != (0, 0, 0)]
        Jl = score([_row(th, refl, x, y, cA, cB) for th, x, y in cand]).tolist()  # host read
        pick = _first_argmin(Jl)
        theta, sx, sy = cand[pick]
        best = Jl[pick]
        path.append((pick, best))

    final = _row(theta, refl, sx, sy, cA, cB)
    sse, nm, _, nn, d2 = _scores(o, XA, YA, XB, YB, table([final]), max_d2, 1, True)
    Tf = table(final)
    return RigidRegistration(
        R=Tf[:4].reshape(2, 2).clone(), t=Tf[4:].clone(), angle=theta, reflected=bool(refl), score=best,
        score_start=score_start, score_coarse=Jh[win], n_matched=int(nm[0]),
        coarse_scores=J[:K].reshape(len(refls), n_angles, n_shifts, n_shifts), path=path, runner_up=runner_up,
        spacing=spacing, max_dist=max_dist, nn=nn[0], matched=d2[0] <= max_d2)


@torch.no_grad()
def prealign_slices(X, Y, n_samples_list, reference=0, chain=False, **kw):
    """Register every view of a stacked data set onto the reference view -> ``(X_aligned, registrations)``.

    ``X`` [N, 2] and ``Y`` [N, P] hold the views one after the other, ``n_samples_list`` their row counts (as
    ``data_dict`` takes them).  View ``reference`` stays where it is (its entry of the list is None); every other view v
    is registered onto it with ``rigid_register(**kw)`` and its rows of ``X_aligned`` (fp64) are ``apply``'d.  With
    ``chain=True`` a view is registered onto its neighbour on the reference's side (v - 1 after the reference, v + 1
    before it) and the transforms are composed towards the reference: the entry's ``R`` / ``t`` (``angle``,
    ``reflected``) are the composed transform, ``pair_R`` / ``pair_t`` the one onto the neighbour.  This is the call
    that replaces a hand-tuned rotation in front of ``data_dict``."""
    what = "prealign_slices"
    if not torch.is_tensor(X) or X.dim() != 2 or not torch.is_tensor(Y) or Y.dim() != 2 or X.shape[0] != Y.shape[0]:
        sh = lambda t: tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: X has shape {sh(X)} and Y {sh(Y)}; [N, 2] and [N, P] are needed")
    if X.shape[1] != 2:
        raise ValueError(f"{what}: X has D = {int(X.shape[1])} coordinates; the candidates are transforms of the plane "
                         "(D = 2) - a 3-D stack is registered slice by slice in its plane")
    counts, ok = view_counts(n_samples_list, int(X.shape[0]), least_views=2)
    V = len(counts)
    if not ok:
        raise ValueError(f"{what}: n_samples_list = {counts} must hold two or more positive row counts that add up to "
                         f"X's {int(X.shape[0])} rows")
    if isinstance(reference, bool) or not isinstance(reference, int) or not 0 <= reference < V:
        raise ValueError(f"{what}: reference must be a view index in [0, {V}), not {reference!r}")
    on_device(what, "neighbour", X=X, Y=Y)
    offs = view_offsets(counts)
    view = lambda t, v: t[offs[v]: offs[v + 1]]
    out = X.detach().to(f64).clone()
    regs = [None] * V
    order = list(range(reference + 1, V)) + list(range(reference - 1, -1, -1))
    for v in order:
        onto = reference if not chain else (v - 1 if v > reference else v + 1)
        reg = rigid_register(view(X, onto), view(Y, onto), view(X, v), view(Y, v), **kw)
        if chain and regs[onto] is not None:
            up = regs[onto]
            R = up.R @ reg.R
            t = up.R @ reg.t + up.t
            Rh = R.tolist()
            reg.update(pair_R=reg.R, pair_t=reg.t, R=R, t=t, reflected=Rh[0][0] * Rh[1][1] - Rh[0][1] * Rh[1][0] < 0,
                       angle=math.atan2(Rh[1][0], Rh[0][0]))
        else:
            reg.update(pair_R=reg.R, pair_t=reg.t)
        regs[v] = reg
        out[offs[v]: offs[v + 1]] = reg.apply(view(X, v))
    return out, regs
