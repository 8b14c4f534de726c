"""The yardstick of the rigid pre-registration (spatial_alignment_amd/register.py, csrc/register.hip): numpy fp64 on the
host, written from the feature's statement and never fed from the code under test.

* ``scores``: per candidate row of T [K, 6] (R row-major, then t) the transformed points q = R x + t, brute-force squared
  distances in difference form, the nearest row of A by the key (d2, index) - ``np.argmin`` keeps the first of equals -
  with a NaN distance counted as +inf, the matched rows d2 <= max_d2, and sse / d2_sum / n_matched; also every row's
  second-smallest distance, for the decisiveness checks.
* ``register``: the whole schedule of ``rigid_register`` (spacing, coarse grid, runner-up, halving refinement), with the
  score list and an assignment signature per candidate of every stage.
* the seeded inputs both test files use: ``contract_case`` (shapes around the kernels' constants), ``lattice_case``
  (exact arithmetic, every row tied) and ``planted_case`` (a jittered lattice with random-Fourier-feature expression, a
  subset of its rows turned, mirrored, shifted and perturbed).

Shared by tests/test_register.py (CPU: the yardstick held to facts, and every seeded input shown to be decisive) and
tests/test_register_gpu.py (the device against the yardstick); the references are computed once (``functools.lru_cache``)
and must not be modified by a test."""
import functools
import math

import numpy as np

# the constants the kernels of csrc/register.hip introduce (the GPU tests' shapes sit around each of them)
RG_ROWS = 256        # rows of B per scan workgroup
RG_TILE = 1024       # rows of A per LDS tile
RG_C = 8             # candidates a thread carries
RG_LANES = (16, 64)  # gene lanes of the closing kernel: P <= 16, otherwise
RG_MAX_GROUPS, RG_GROUP_MIN = 32, 32  # row groups of the sums: ceil(n / max(32, ceil(n / 32)))
DECISIVE_REL = 1e-9


# ------------------------------------------------------------------------------------------------------------------------
# the scoring entry
# ------------------------------------------------------------------------------------------------------------------------
def transform(T_row, X):
    """q [n, 2] = R x + t, the products added as the entry nests them: R_d0 x0 + (R_d1 x1 + t_d)"""
    X = np.asarray(X, np.float64)
    r00, r01, r10, r11, t0, t1 = (float(v) for v in T_row)
    return np.stack([r00 * X[:, 0] + (r01 * X[:, 1] + t0), r10 * X[:, 0] + (r11 * X[:, 1] + t1)], 1)


def scores(XA, YA, XB, YB, T, max_d2):
    """-> dict: sse, d2_sum [K] fp64, n_matched [K] int64, nn [K, n] int64, d2 [K, n] and d2_second [K, n] (the
    second-smallest distance; +inf where A has one row)"""
    XA, XB, T = np.asarray(XA, np.float64), np.asarray(XB, np.float64), np.asarray(T, np.float64)
    YA, YB = np.asarray(YA, np.float32).astype(np.float64), np.asarray(YB, np.float32).astype(np.float64)
    K, n, m = len(T), len(XB), len(XA)
    a0, a1 = XA[None, :, 0], XA[None, :, 1]
    rows = np.arange(n)
    out = dict(sse=np.zeros(K), d2_sum=np.zeros(K), n_matched=np.zeros(K, np.int64), nn=np.zeros((K, n), np.int64),
               d2=np.zeros((K, n)), d2_second=np.full((K, n), np.inf))
    for k in range(K):
        q = transform(T[k], XB)
        with np.errstate(invalid="ignore", over="ignore"):
            u0, u1 = q[:, 0, None] - a0, q[:, 1, None] - a1
            D2 = u0 * u0 + u1 * u1
        D2[np.isnan(D2)] = np.inf
        nn = np.argmin(D2, axis=1)  # the first of equal minima: the lower index
        d2 = D2[rows, nn]
        if m > 1:
            D2[rows, nn] = np.inf
            out["d2_second"][k] = D2.min(axis=1)
        hit = d2 <= max_d2
        diff = YB[hit] - YA[nn[hit]]
        out["sse"][k] = float((diff * diff).sum())
        out["d2_sum"][k] = float(d2[hit].sum())
        out["n_matched"][k] = int(hit.sum())
        out["nn"][k], out["d2"][k] = nn, d2
    return out


def undecided_rows(ref, max_d2):
    """[K, n] bool: rows whose nearest neighbour or whose matching could turn on a rounding - the second-smallest
    distance within DECISIVE_REL max(1, d2) of the smallest (or equal to it), or d2 that close to max_d2.  A row at
    +inf (a NaN coordinate) is unmatched whatever its index: decided."""
    d2, second = ref["d2"], ref["d2_second"]
    with np.errstate(invalid="ignore"):
        tol = DECISIVE_REL * np.maximum(1.0, d2)
        close = ~(second - d2 > tol) | (np.abs(d2 - max_d2) <= tol)
    return close & np.isfinite(d2)


def J_of(sse, n_matched, n, P, min_overlap):
    n_matched = np.asarray(n_matched, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n_matched >= min_overlap * n, np.asarray(sse) / (n_matched * P), np.inf)


# ------------------------------------------------------------------------------------------------------------------------
# the search
# ------------------------------------------------------------------------------------------------------------------------
def candidate_row(theta, refl, sx, sy, cA, cB):
    """flip the second axis where ``refl``, turn by theta about B's centroid, move it onto A's centroid, shift"""
    c, s = math.cos(theta), math.sin(theta)
    sg = -1.0 if refl else 1.0
    r00, r01, r10, r11 = c, -s * sg, s, c * sg
    return [r00, r01, r10, r11, cA[0] + sx - (r00 * cB[0] + r01 * cB[1]), cA[1] + sy - (r10 * cB[0] + r11 * cB[1])]


def spacing_of(XA):
    """the median (the lower of the two middle values) distance from a row of A to its nearest other row"""
    XA = np.asarray(XA, np.float64)
    u0, u1 = XA[:, 0, None] - XA[None, :, 0], XA[:, 1, None] - XA[None, :, 1]
    D2 = u0 * u0 + u1 * u1
    np.fill_diagonal(D2, np.inf)
    return float(np.sort(np.sqrt(D2.min(axis=1)))[(len(XA) - 1) // 2])


def _first_argmin(v):
    best = 0
    for q in range(len(v)):
        if v[q] < v[best]:
            best = q
    return best


def _stage(XA, YA, XB, YB, rows, max_d2, min_overlap):
    """one table scored: J per row, the first argmin, and what the decisiveness checks need"""
    ref = scores(XA, YA, XB, YB, rows, max_d2)
    n, P = len(XB), np.asarray(YA).shape[1]
    J = J_of(ref["sse"], ref["n_matched"], n, P, min_overlap)
    hit = ref["d2"] <= max_d2
    sig = [hash((ref["nn"][k][hit[k]].tobytes(), hit[k].tobytes())) for k in range(len(J))]  # the matched assignment
    return dict(J=J, pick=_first_argmin(J), sig=sig, undecided=int(undecided_rows(ref, max_d2).sum()))


def undecided_stage(stage):
    """True where the stage's choice could turn on a rounding: a candidate with ANOTHER assignment within DECISIVE_REL
    (relative) of the winner's J.  (Candidates with the winner's assignment have its J bit for bit: the first wins.)"""
    J, pick = stage["J"], stage["pick"]
    if not np.isfinite(J[pick]):
        return False
    others = [J[k] for k in range(len(J)) if stage["sig"][k] != stage["sig"][pick]]
    return bool(others) and min(others) - J[pick] <= DECISIVE_REL * abs(J[pick])


def register(XA, YA, XB, YB, n_angles=360, reflection=True, n_shifts=1, shift_extent=0.25, max_dist=None,
             min_overlap=0.5, levels=6):
    """the schedule of ``rigid_register`` -> dict (R [2, 2], t [2], angle, reflected, score, score_start, score_coarse,
    n_matched, coarse J [K], path [(index, J)], runner_up, spacing, max_dist, nn [n], stages: every scored table)"""
    XA, XB = np.asarray(XA, np.float64), np.asarray(XB, np.float64)
    n = len(XB)
    spacing = spacing_of(XA)
    max_dist = 3.0 * spacing if max_dist is None else float(max_dist)
    max_d2 = max_dist * max_dist
    cA, cB = XA.mean(0).tolist(), XB.mean(0).tolist()
    ext = (XA.max(0) - XA.min(0)).tolist()
    refls = (False, True) if reflection else (False,)

    def grid(half):
        return [0.0] if n_shifts == 1 else [-half + 2.0 * half * q / (n_shifts - 1) for q in range(n_shifts)]

    gx, gy = grid(shift_extent * ext[0]), grid(shift_extent * ext[1])
    step = 2.0 * math.pi / n_angles
    params = [(a * step, f, sx, sy) for f in refls for a in range(n_angles) for sx in gx for sy in gy]
    K = len(params)
    rows = [candidate_row(th, f, sx, sy, cA, cB) for th, f, sx, sy in params] + [candidate_row(0.0, False, 0.0, 0.0, cA, cB)]
    coarse = _stage(XA, YA, XB, YB, rows, max_d2, min_overlap)
    score_start = float(coarse["J"][K])
    # the start row is scored with the table but does not compete
    coarse["J"], coarse["sig"] = coarse["J"][:K], coarse["sig"][:K]
    coarse["pick"] = win = _first_argmin(coarse["J"])
    Jc = coarse["J"]
    if not Jc[win] < np.inf:
        raise ValueError("no coarse candidate reaches min_overlap")
    theta, refl, sx, sy = params[win]
    per_angle = n_shifts * n_shifts
    a_win = (win // per_angle) % n_angles
    runner = None
    for q in range(K):
        a_q = (q // per_angle) % n_angles
        gap = min((a_q - a_win) % n_angles, (a_win - a_q) % n_angles)
        if (params[q][1] != refl or gap > 2) and (runner is None or Jc[q] < Jc[runner]):
            runner = q
    runner_up = None if runner is None else (params[runner][0], params[runner][1], float(Jc[runner]))
    stages, path, best = [coarse], [], float(Jc[win])
    for level in range(1, levels + 1):
        da, ds = step / 2.0**level, spacing / 2.0 ** (level - 1)
        cand = [(theta, sx, sy)] + [(theta + qa * da, sx + qx * ds, sy + qy * ds) for qa in (-1, 0, 1)
                                    for qx in (-2, -1, 0, 1, 2) for qy in (-2, -1, 0, 1, 2) if (qa, qx, qy) != (0, 0, 0)]
        st = _stage(XA, YA, XB, YB, [candidate_row(th, refl, x, y, cA, cB) for th, x, y in cand], max_d2, min_overlap)
        theta, sx, sy = cand[st["pick"]]
        best = float(st["J"][st["pick"]])
        path.append((st["pick"], best))
        stages.append(st)
    final = candidate_row(theta, refl, sx, sy, cA, cB)
    last = scores(XA, YA, XB, YB, [final], max_d2)
    return dict(R=np.array(final[:4]).reshape(2, 2), t=np.array(final[4:]), angle=theta, reflected=bool(refl), score=best,
                score_start=score_start, score_coarse=float(Jc[win]), n_matched=int(last["n_matched"][0]), coarse=Jc,
                path=path, runner_up=runner_up, spacing=spacing, max_dist=max_dist, nn=last["nn"][0],
                matched=last["d2"][0] <= max_d2, stages=stages,
                final_undecided=int(undecided_rows(last, max_d2).sum()))


# ------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------------------------------------
def random_transforms(rng, K, XA, XB, spread):
    """K rows of T: a random angle and reflection about B's centroid onto A's, a shift of up to ``spread``"""
    cA, cB = XA.mean(0).tolist(), XB.mean(0).tolist()
    return np.array([candidate_row(rng.uniform(0, 2 * math.pi), bool(rng.integers(2)), rng.uniform(-spread, spread),
                                   rng.uniform(-spread, spread), cA, cB) for _ in range(K)])


# name -> (n, m, K, P): around the 256-row block, the 1024-row LDS tile, the 8 candidates of a thread, the 16 / 64 gene
# lanes, the row groups of the sums (n = 1024: 32 groups of 32; 1025: 32 of 33, the last one short), m = 1 and n = 1
CONTRACT_SHAPES = {
    "all-ones": (1, 1, 1, 1),
    "below-the-edges": (RG_ROWS - 1, RG_TILE - 1, RG_C - 1, 3),
    "on-the-edges": (RG_ROWS, RG_TILE, RG_C, 63),
    "past-the-edges": (RG_ROWS + 1, RG_TILE + 1, RG_C + 1, 64),
    "one-row-of-A": (300, 1, 2 * RG_C + 3, 65),
    "one-row-of-B": (1, 1500, 2 * RG_C + 3, 17),
    "many-groups": (1025, 2 * RG_TILE + 52, 3, 16),
    "groups-on-the-edge": (1024, 300, 2, 1),
    "typical": (700, 600, 2 * RG_C + 3, 50),
}
# variants of "typical": max_d2 that matches no row / every row, a NaN coordinate in B
CONTRACT_VARIANTS = ("typical/none-matched", "typical/all-matched", "typical/nan-in-B")


@functools.lru_cache(maxsize=None)
def contract_case(name):
    """-> dict XA, YA, XB, YB, T, max_d2 (numpy; Y fp32) and ``ref`` = scores(...) of it"""
    base, _, variant = name.partition("/")
    n, m, K, P = CONTRACT_SHAPES[base]
    rng = np.random.default_rng(sorted(CONTRACT_SHAPES).index(base) + 100)
    side = max(2.0, math.sqrt(m))  # about one spot of A per unit square
    XA = rng.uniform(0, side, (m, 2))
    XB = rng.uniform(0, side, (n, 2)) + rng.uniform(-50, 50, 2)
    YA = rng.normal(size=(m, P)).astype(np.float32)
    YB = rng.normal(size=(n, P)).astype(np.float32)
    T = random_transforms(rng, K, XA, XB, 0.2 * side)
    max_d2 = 0.3  # about 60 % of the rows that land inside A
    if variant == "none-matched":
        max_d2 = 0.0
    elif variant == "all-matched":
        max_d2 = 1e300
    elif variant == "nan-in-B":
        XB[5, 0] = np.nan
        XB[n - 1, 1] = np.nan
    else:
        assert variant == "", name
    case = dict(XA=XA, YA=YA, XB=XB, YB=YB, T=T, max_d2=max_d2)
    case["ref"] = scores(XA, YA, XB, YB, T, max_d2)
    return case


def quarter_turns(cA, cB, shift):
    """the four quarter turns x reflection about B's centroid onto A's (+ shift), R's entries exactly 0 / +-1"""
    rows = []
    for refl in (False, True):
        for c, s in ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)):
            sg = -1.0 if refl else 1.0
            r00, r01, r10, r11 = c, -s * sg, s, c * sg
            rows.append([r00, r01, r10, r11, cA[0] + shift - (r00 * cB[0] + r01 * cB[1]),
                         cA[1] + shift - (r10 * cB[0] + r11 * cB[1])])
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def lattice_case(nx=33, ny=33):
    """an integer lattice (nx * ny > one LDS tile) registered onto itself: the eight lattice symmetries, and the same
    moved by half a cell, where every row of B sits at the same distance from four rows of A.  Coordinates are multiples
    of 1/2, the expression small integers: every product, sum and comparison is exact, in any order."""
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    XA = np.stack([gx.ravel(), gy.ravel()], 1)
    rng = np.random.default_rng(7)
    YA = rng.integers(-4, 5, (len(XA), 3)).astype(np.float32)
    c = [(nx - 1) / 2.0, (ny - 1) / 2.0]
    T = np.concatenate([quarter_turns(c, c, 0.0), quarter_turns(c, c, 0.5)])
    case = dict(XA=XA, YA=YA, XB=XA.copy(), YB=YA.copy(), T=T, max_d2=2.0)
    case["ref"] = scores(XA, YA, XA, YA, T, 2.0)
    return case


# the planted cases: (P, fraction of A's rows kept, angle, mirrored, shift, position jitter / spacing, expression noise)
PLANTED = {
    "p3-80-1.45": (3, 0.8, 1.45, False, (0.0, 0.0), 0.1, 0.1),
    "p10-80-1.45-mirrored": (10, 0.8, 1.45, True, (0.0, 0.0), 0.1, 0.1),
    "p10-60-3.0-mirrored-shifted": (10, 0.6, 3.0, True, (7.3, -4.1), 0.1, 0.2),
    "p3-60-3.0-shifted": (3, 0.6, 3.0, False, (-11.0, 5.5), 0.1, 0.1),
    "p10-80-1.45-mirrored-noisy": (10, 0.8, 1.45, True, (0.0, 0.0), 0.2, 0.3),
}
PLANTED_TIGHT = tuple(k for k, v in PLANTED.items() if v[5] == 0.1)  # the jitter-0.1 cases: nn == planted on >= 0.98


@functools.lru_cache(maxsize=None)
def planted_case(name, side=25):
    """a jittered side x side lattice (spacing 1, uniform +-0.25) with random-Fourier-feature expression; B = a shuffled
    subset of A's rows, moved by Gaussian position jitter, mirrored, turned, shifted, its expression perturbed.
    -> dict XA, YA, XB, YB, planted [n] (B's row i is A's row planted[i]), origin [n, 2] = XA[planted], mirrored"""
    P, frac, angle, mirrored, shift, jitter, noise = PLANTED[name]
    rng = np.random.default_rng(sorted(PLANTED).index(name))
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
    XA = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.25, 0.25, (side * side, 2))
    F = 40
    W, b = rng.normal(size=(2, F)) / 4.0, rng.uniform(0, 2 * math.pi, F)  # length scale: 4 spacings
    Y = math.sqrt(2.0 / F) * np.cos(XA @ W + b) @ rng.normal(size=(F, P))
    Y = (Y - Y.mean(0)) / Y.std(0)
    m = len(XA)
    planted = rng.permutation(m)[: int(round(frac * m))]
    pos = XA[planted] + jitter * rng.normal(size=(len(planted), 2))
    if mirrored:
        pos = pos * np.array([1.0, -1.0])
    c, s = math.cos(angle), math.sin(angle)
    XB = pos @ np.array([[c, -s], [s, c]]).T + np.array(shift)
    YB = Y[planted] + noise * rng.normal(size=(len(planted), P))
    return dict(XA=XA, YA=Y.astype(np.float32), XB=XB, YB=YB.astype(np.float32), planted=planted, origin=XA[planted],
                mirrored=mirrored)


@functools.lru_cache(maxsize=None)
def planted_reference(name):
    case = planted_case(name)
    return register(case["XA"], case["YA"], case["XB"], case["YB"])
