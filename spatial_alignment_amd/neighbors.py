"""Neighbour statistics on the device: exact k nearest neighbours, kNN regression scores, Moran's I, the alignment score.

Almost every experiment of the reference steps outside GPSA to a CPU k-nearest-neighbour library around the fit; with the
coordinates and the expression matrix already in HBM these are thin Python over two HIP entries (csrc/neighbors.hip:
``gpsa_knn_f64``, ``gpsa_knn_average_*``):

* ``spatial_r2``: leave-one-out kNN self-regression R^2 per gene - the gene selection before the fit
  (experiments/expression/st/st_alignment.py:127-138, visium/visium_alignment.py:100-112);
* ``kth_neighbor_distance``: the outlier filter (slideseq/slideseq_alignment.py:108-118);
* ``alignment_score``: view b's expression predicted from view a's spots at the aligned coordinates, scored by R^2 - what
  the reference prints while it trains (visium/visium_alignment.py:284-293), before / after as moransi_post_alignment.py;
* ``knn_regress``: the prediction baselines, ``KNeighborsRegressor(n_neighbors=10, weights="distance")``
  (slideseq/slideseq_prediction.py:275-308, 400-402);
* ``moran_i``: Moran's I with its normal-approximation z score (visium/moransi_post_alignment.py:88-102).

The neighbours are exact: the k smallest keys (squared distance in fp64 in difference form, row index), so a tie goes to
the lower index and the result does not depend on how the work was cut - not on ``rows_per_chunk``, bit for bit.
Everything runs under ``torch.no_grad()`` and touches no model state.  Coordinates of any float dtype are taken to fp64,
``Y`` to fp32.  Tensors on the CPU are refused with a ``ValueError`` that names the device: there is no host path.
"""
import math

import torch

from ._args import as_device, chunk_rows, coords, on_device, ops as _ops, values
from .predict import Prediction

f64, f32 = torch.float64, torch.float32
MAX_K, MAX_D = 32, 4  # csrc/neighbors.hip: KNN_MAXK, MAXD
WEIGHTS = ("uniform", "distance")


# ------------------------------------------------------------------------------------------------------------------------
# argument checks (all of them before any device work)
# ------------------------------------------------------------------------------------------------------------------------
def _check_k(k, available, what, excluded=False):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k must be an integer in [1, {MAX_K}], not {k!r}")
    if k > available:
        raise ValueError(f"{what}: k = {k} neighbours asked of {available} reference rows"
                         + (" (the point itself is left out)" if excluded else ""))
    return k


def _check_weights(weights, what):
    if weights not in WEIGHTS:
        raise ValueError(f"{what}: weights must be 'uniform' or 'distance', not {weights!r}")
    return weights


def _chunk(rows_per_chunk, n, what):
    c = chunk_rows(rows_per_chunk, what)
    return max(n, 1) if c is None else c


# ------------------------------------------------------------------------------------------------------------------------
# the neighbours
# ------------------------------------------------------------------------------------------------------------------------
def _knn_chunks(Q, R, k, exclude_self, c):
    """(a, idx, d2) per chunk of c query rows; Q, R contiguous fp64 on the device, Q is R where exclude_self (a chunk
    is then a row slice of R's storage, which is how gpsa_knn_f64 knows each query's own row)"""
    o = _ops()
    for a in range(0, int(Q.shape[0]), c):
        idx, d2 = o.knn(Q[a: a + c], R, k, exclude_self=exclude_self)
        yield a, idx, d2


def _self_or_ref(query, ref, exclude_self, what):
    """-> (ref or query, exclude_self) with the defaults resolved; exclude_self only for the points' own neighbours"""
    own = ref is None or ref is query
    if exclude_self is None:
        exclude_self = ref is None
    if exclude_self and not own:
        raise ValueError(f"{what}: exclude_self=True is the points' own neighbours: leave the second set of points out "
                         "(None) or pass the same tensor twice")
    return (query if own else ref), bool(exclude_self)


@torch.no_grad()
def knn(query, ref=None, k=10, exclude_self=None, rows_per_chunk=None):
    """The ``k`` nearest rows of ``ref`` [nr, D] for every row of ``query`` [nq, D], exact.

    ``ref=None``: the points' own neighbours, each point left out of its own list (``exclude_self=True``; sklearn gets
    this by asking for k + 1 and dropping column 0).  Returns a ``Prediction``: ``idx`` [nq, k] int32 (rows of ``ref``),
    ``dist`` [nq, k] fp64 and ``d2`` [nq, k] fp64 (``dist = sqrt(d2)``), ascending in the key (d2, index): ties in the
    distance go to the lower index.  1 <= D <= 4, 1 <= k <= 32.  rows_per_chunk: query rows per launch (default: all;
    the result does not depend on it, bit for bit)."""
    what = "knn"
    coords(query, "query", what, MAX_D)
    if ref is not None:
        coords(ref, "ref", what, MAX_D)
        if ref.shape[1] != query.shape[1]:
            raise ValueError(f"{what}: query has shape {tuple(query.shape)} and ref {tuple(ref.shape)}: the same D is needed")
    ref_t, excl = _self_or_ref(query, ref, exclude_self, what)
    _check_k(k, int(ref_t.shape[0]) - excl, what, excl)
    c = _chunk(rows_per_chunk, int(query.shape[0]), what)
    on_device(what, "neighbour", query=query, ref=ref)
    R = as_device(ref_t, f64)
    Q = R if ref_t is query else as_device(query, f64)
    nq = int(Q.shape[0])
    idx = torch.empty(nq, k, dtype=torch.int32, device=Q.device)
    d2 = torch.empty(nq, k, dtype=f64, device=Q.device)
    o = _ops()
    for a in range(0, nq, c):
        o.knn(Q[a: a + c], R, k, exclude_self=excl, out=(idx[a: a + c], d2[a: a + c]))
    return Prediction(idx=idx, dist=d2.sqrt(), d2=d2)


@torch.no_grad()
def knn_regress(X_train, Y_train, X_test=None, k=10, weights="uniform", exclude_self=False, rows_per_chunk=None):
    """kNN regression: for every row of ``X_test`` [n_test, D] the (weighted) average of ``Y_train`` [n_train, P] over its
    ``k`` nearest rows of ``X_train`` [n_train, D] -> [n_test, P] fp32 (``KNeighborsRegressor(n_neighbors=k,
    weights=weights).fit(X_train, Y_train).predict(X_test)``).

    weights: "uniform", or "distance" (1 / distance; where some neighbours are at distance 0 exactly those are averaged -
    sklearn's rule).  A NaN in ``Y_train`` is left out of the averages it would enter; an entry whose neighbours are all
    NaN is NaN.  ``exclude_self=True`` (with ``X_test=None`` or ``X_train`` itself): leave-one-out, every training point
    predicted from the others.  The average is accumulated in fp64 in neighbour order and does not depend on
    ``rows_per_chunk``, bit for bit."""
    what = "knn_regress"
    coords(X_train, "X_train", what, MAX_D)
    values(Y_train, "Y_train", what, int(X_train.shape[0]))
    if X_test is None:
        X_test = X_train
    coords(X_test, "X_test", what, MAX_D)
    if X_test.shape[1] != X_train.shape[1]:
        raise ValueError(f"{what}: X_test has shape {tuple(X_test.shape)} and X_train {tuple(X_train.shape)}: the same D "
                         "is needed")
    _, excl = _self_or_ref(X_test, X_train, bool(exclude_self), what)
    _check_weights(weights, what)
    _check_k(k, int(X_train.shape[0]) - excl, what, excl)
    c = _chunk(rows_per_chunk, int(X_test.shape[0]), what)
    on_device(what, "neighbour", X_train=X_train, Y_train=Y_train, X_test=X_test)
    R = as_device(X_train, f64)
    Q = R if X_test is X_train else as_device(X_test, f64)
    Y = as_device(Y_train, f32)
    out = torch.empty(int(Q.shape[0]), int(Y.shape[1]), dtype=f32, device=Q.device)
    o = _ops()
    for a, idx, d2 in _knn_chunks(Q, R, k, excl, c):
        o.knn_average(idx, d2 if weights == "distance" else None, Y, weights, out=out[a: a + c])
    return out


def _masked(Y, pred, what):
    if not torch.is_tensor(Y) or not torch.is_tensor(pred) or Y.dim() != 2 or tuple(Y.shape) != tuple(pred.shape):
        sh = lambda t: tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: Y has shape {sh(Y)} and pred {sh(pred)}; two [n, P] tensors are needed")
    Y, pred = Y.detach().to(f64), pred.detach().to(device=Y.device, dtype=f64)
    use = ~(torch.isnan(Y) | torch.isnan(pred))
    zero = torch.zeros((), dtype=f64, device=Y.device)
    return torch.where(use, Y, zero), torch.where(use, pred, zero), use, use.sum(0).to(f64)


@torch.no_grad()
def r2_score(Y, pred):
    """Coefficient of determination per column, fp64 [P]: ``1 - SS_res / SS_tot`` with ``SS_tot`` around the column mean,
    over the rows where neither ``Y`` nor ``pred`` is NaN (``sklearn.metrics.r2_score(multioutput="raw_values")`` on
    complete data).  A column with ``SS_tot == 0`` (a constant column, or no row left) is NaN; sklearn returns 0 or 1 there."""
    y, p, use, n = _masked(Y, pred, "r2_score")
    mean = y.sum(0) / n
    zero = torch.zeros((), dtype=f64, device=y.device)
    ss_res = torch.where(use, y - p, zero).square().sum(0)
    ss_tot = torch.where(use, y - mean, zero).square().sum(0)
    return torch.where(ss_tot > 0, 1.0 - ss_res / ss_tot, torch.full_like(ss_tot, float("nan")))


@torch.no_grad()
def pearson(Y, pred):
    """Pearson correlation per column, fp64 [P], over the rows where neither ``Y`` nor ``pred`` is NaN; NaN where either
    side is constant there."""
    y, p, use, n = _masked(Y, pred, "pearson")
    zero = torch.zeros((), dtype=f64, device=y.device)
    yc = torch.where(use, y - y.sum(0) / n, zero)
    pc = torch.where(use, p - p.sum(0) / n, zero)
    den = (yc.square().sum(0) * pc.square().sum(0)).sqrt()
    return torch.where(den > 0, (yc * pc).sum(0) / den, torch.full_like(den, float("nan")))


@torch.no_grad()
def spatial_r2(X, Y, k=10, weights="uniform", rows_per_chunk=None):
    """Leave-one-out kNN self-regression R^2 per output, fp64 [P]: how well each column of ``Y`` [N, P] is predicted at a
    spot from its ``k`` nearest OTHER spots - the reference's gene-selection score (st_alignment.py:127-138)."""
    pred = knn_regress(X, Y, None, k=k, weights=weights, exclude_self=True, rows_per_chunk=rows_per_chunk)
    return r2_score(Y.to(f32), pred)


@torch.no_grad()
def kth_neighbor_distance(X, k=10, rows_per_chunk=None):
    """Distance from every point of ``X`` [N, D] to its ``k``-th nearest other point, fp64 [N] - the reference's outlier
    filter (slideseq_alignment.py:108-118)."""
    return knn(X, None, k=k, rows_per_chunk=rows_per_chunk).dist[:, k - 1].contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# Moran's I
# ------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def moran_i(X, Y, k=6, row_standardize=True, rows_per_chunk=None):
    """Moran's I of every column of ``Y`` [N, P] on the directed binary kNN graph of ``X`` [N, D] (no self edges):
    ``w_ij = 1`` where j is among i's ``k`` nearest, divided by ``k`` when ``row_standardize``.

    ``I_p = (n / S0) sum_i z_ip lag_ip / sum_i z_ip^2`` with z the centred column and ``lag = W z`` (the neighbours'
    average, in fp64).  Returns a ``Prediction``, all fp64: ``I`` [P], ``expected`` = -1 / (n - 1), ``variance`` under the
    normality assumption, ``(n^2 S1 - n S2 + 3 S0^2) / ((n^2 - 1) S0^2) - expected^2`` with ``S0 = sum w``, ``S1 = 1/2
    sum_ij (w_ij + w_ji)^2`` and ``S2 = sum_i (w_i. + w_.i)^2`` from the in-degrees and the count of mutual edges, ``z``
    [P] = (I - expected) / sqrt(variance) and ``p_norm`` [P] = 1/2 erfc(z / sqrt 2), the upper tail.  A constant column
    is NaN.  ``Y`` with a NaN is refused (ValueError).  No permutation p-values; the graph is not symmetrised."""
    what = "moran_i"
    coords(X, "X", what, MAX_D)
    n = int(X.shape[0])
    values(Y, "Y", what, n)
    _check_k(k, n - 1, what, True)
    c = _chunk(rows_per_chunk, n, what)
    if bool(torch.isnan(Y).any()):
        raise ValueError(f"{what}: Y has NaN entries; Moran's I is defined on complete columns (drop or fill them first)")
    on_device(what, "neighbour", X=X, Y=Y)
    R = as_device(X, f64)
    y = Y.detach().to(f32).to(f64)
    zc = (y - y.mean(0)).contiguous()
    idx = torch.empty(n, k, dtype=torch.int32, device=R.device)
    lag = torch.empty_like(zc)
    o = _ops()
    for a, ia, _ in _knn_chunks(R, R, k, True, c):
        idx[a: a + c] = ia
        o.knn_average(ia, None, zc, "uniform", out=lag[a: a + c])  # fp64 in, fp64 out
    wt = 1.0 / k if row_standardize else 1.0
    if not row_standardize:
        lag = lag * k
    # the graph's sums: E = n k directed edges, of which `mutual` have their reverse in the graph
    li = idx.long()
    rows = torch.arange(n, device=R.device).view(n, 1, 1)
    mutual = float((li[li] == rows).any(-1).sum())
    indeg = torch.bincount(li.reshape(-1), minlength=n).to(f64)
    E = float(n * k)
    S0 = wt * E
    S1 = wt * wt * (E + mutual)
    S2 = wt * wt * float((indeg + k).square().sum())
    den = zc.square().sum(0)
    nan = torch.full_like(den, float("nan"))
    const = y.amax(0) == y.amin(0)
    I = torch.where(const | (den <= 0), nan, (n / S0) * (zc * lag).sum(0) / den)
    EI = -1.0 / (n - 1)
    var = (n * n * S1 - n * S2 + 3.0 * S0 * S0) / ((n * n - 1.0) * S0 * S0) - EI * EI
    z = (I - EI) / math.sqrt(var) if var > 0 else nan
    full = lambda v: torch.full_like(den, v)
    return Prediction(I=I, expected=full(EI), variance=full(var), z=z, p_norm=0.5 * torch.erfc(z / math.sqrt(2.0)))


# ------------------------------------------------------------------------------------------------------------------------
# the alignment score
# ------------------------------------------------------------------------------------------------------------------------
def _pair_scores(coords, Ys, k, weights, c, V):
    """r2 / pearson [V, V, P] of predicting view b's outputs from view a's spots at ``coords`` (None: an empty view)"""
    P, dev = next(int(y.shape[1]) for y in Ys if y is not None), next(y.device for y in Ys if y is not None)
    r2 = torch.full((V, V, P), float("nan"), dtype=f64, device=dev)
    pr = torch.full((V, V, P), float("nan"), dtype=f64, device=dev)
    for a in range(V):
        for b in range(V):
            if a == b or coords[a] is None or coords[b] is None:
                continue
            pred = knn_regress(coords[a], Ys[a], coords[b], k=k, weights=weights, rows_per_chunk=c)
            r2[a, b] = r2_score(Ys[b], pred)
            pr[a, b] = pearson(Ys[b], pred)
    return r2, pr


def _nanmean(t):
    use = ~torch.isnan(t)
    cnt = use.sum(-1)
    s = torch.where(use, t, torch.zeros((), dtype=t.dtype, device=t.device)).sum(-1)
    return torch.where(cnt > 0, s / cnt, torch.full_like(s, float("nan")))


@torch.no_grad()
def alignment_score(model, X_spatial, Y, view_idx=None, *, k=10, weights="uniform", G=None, raw=True,
                    rows_per_chunk=None):
    """Did the alignment get better?  For every ordered pair of non-empty views a != b of a modality, view b's outputs are
    predicted from view a's spots by kNN regression AT THE ALIGNED COORDINATES and scored against view b's own - the
    score the reference prints while it trains (visium_alignment.py:284-293).

    X_spatial {mod: [N, D]}, Y {mod: [N, P]}, view_idx: as ``forward`` takes them (view_idx defaults to the model's own).
    The aligned coordinates of view v's rows are ``warp_field(X[rows_v], v, jacobian=False).G_mean`` (a fixed view is the
    identity), or the rows of ``G`` {mod: [N, D]} where that is given (any aligned coordinates, e.g. of a plug-in warp
    kernel, for which ``warp_field`` raises its ValueError).

    Returns {mod: ``Prediction``}: ``r2`` and ``pearson`` [V, V, P] fp64 (entry [a, b]: b predicted from a; NaN on the
    diagonal and for an empty view) and ``r2_mean`` [V, V], the plain mean over the outputs whose R^2 is not NaN; with
    ``raw=True`` also ``r2_raw`` / ``pearson_raw`` / ``r2_mean_raw``, the same from the native coordinates - the before /
    after comparison.  Raises ValueError for a shape that does not match the views' row counts, ``k`` larger than a source
    view's rows, or fewer than two non-empty views."""
    from .models.vgpsa import _as_index
    from .warp import _check_kind, warp_field

    what = "alignment_score"
    mods, V, D = model.modality_names, int(model.n_views), int(model.n_spatial_dims)
    view_idx = model.view_idx if view_idx is None else view_idx
    _check_weights(weights, what)
    dev = model.Xtilde.device
    rows_of, tensors = {}, {}
    for m in mods:
        rows_of[m] = [_as_index(view_idx[m][v], dev) for v in range(V)]
        N = sum(cnt for _, cnt in rows_of[m])
        for name, d, width in (("X_spatial", X_spatial, D), ("Y", Y, None), ("G", G, D)):
            if d is None:
                continue
            t = d[m]
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != N or (width is not None and t.shape[1] != width):
                shape = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"{what}: {name}[{m!r}] has shape {shape}, the views' row counts give "
                                 f"[{N}, {width if width is not None else 'P'}]")
            tensors[f"{name}[{m!r}]"] = t
        live = [cnt for _, cnt in rows_of[m] if cnt > 0]
        if len(live) < 2:
            raise ValueError(f"{what}: modality {m!r} has rows in {len(live)} view(s); a score needs two non-empty views")
        _check_k(k, min(live), f"{what} (modality {m!r}, its smallest view)")
    c = None if rows_per_chunk is None else _chunk(rows_per_chunk, 1, what)
    if G is None and any(not model._is_fixed(v) for v in range(V)):
        _check_kind(model, what)
    on_device(what, "neighbour", **tensors, model=model.Xtilde)

    out = {}
    for m in mods:
        X = X_spatial[m].detach().to(device=dev, dtype=f64)
        Ym = Y[m].detach().to(device=dev, dtype=f32)
        native, aligned, Ys = [], [], []
        for v, (rows, cnt) in enumerate(rows_of[m]):
            if cnt == 0:
                native.append(None), aligned.append(None), Ys.append(None)
                continue
            Xv = X[rows].contiguous()
            native.append(Xv)
            Ys.append(Ym[rows].contiguous())
            if G is not None:
                aligned.append(G[m].detach().to(device=dev, dtype=f64)[rows].contiguous())
            else:
                aligned.append(warp_field(model, Xv, v, jacobian=False, rows_per_chunk=c).G_mean)
        r2, pr = _pair_scores(aligned, Ys, k, weights, c, V)
        res = Prediction(r2=r2, pearson=pr, r2_mean=_nanmean(r2))
        if raw:
            r2n, prn = _pair_scores(native, Ys, k, weights, c, V)
            res.update(r2_raw=r2n, pearson_raw=prn, r2_mean_raw=_nanmean(r2n))
        out[m] = res
    return out
