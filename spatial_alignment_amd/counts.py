"""Count preprocessing on the device: from a raw count matrix in HBM to what ``fit()`` takes.

The reference ships these steps as numpy in gpsa/util/util.py:155-254 (``compute_size_factors``, ``poisson_deviance``,
``deviance_feature_selection``, ``deviance_residuals``, ``pearson_residuals``) and its experiments run them, or their
scanpy spellings (``normalize_total`` + ``log1p``, a z-score per view), right before they build ``data_dict``.  Here they
are thin Python over four HIP entries (csrc/counts.hip): ``gpsa_count_margins_f32`` (row / column sums, entries > 0, the
count of invalid entries in ONE read), ``gpsa_count_deviance_f32``, ``gpsa_count_transform_f32`` and
``gpsa_standardize_views_f32``.  ``Y`` is [N spots, P genes]; it is taken to contiguous fp32 (counts are exact in fp32 up
to 2^24), every sum is fp64 in a fixed order, and nothing of N * P elements is allocated beyond the result.

* ``count_stats``, ``size_factors``, ``poisson_deviance``, ``deviance_feature_selection``: the Poisson / NB route and the
  gene ranking;
* ``pearson_residuals``, ``deviance_residuals``, ``normalize_log1p``, ``standardize_views``: the Gaussian route;
* ``prepare_counts``: the one call, in the order the experiments use.

Deliberate departures from the reference: a gene with no counts has deviance exactly 0 (the reference drops it) and
residual 0 (the reference divides 0 by 0); a column that is constant within a view standardises to 0 and is counted (the
reference writes NaN); a spot with no counts is refused by name (the reference takes log 0); equal deviances rank by
the lower gene index.  Everything runs under ``torch.no_grad()``.  Tensors on the CPU are refused with a ``ValueError``
that names the device: there is no host path.
"""
import math

import torch

from .predict import Prediction

f64, f32 = torch.float64, torch.float32
# csrc/counts.hip: the rows of a group (at least / at most), the cap on the groups, the columns of a tile.  A matrix of
# more than ROWS_MIN * MAX_GROUPS rows has more row blocks than the cap, and its groups grow.
ROWS_MIN, ROWS_MAX, MAX_GROUPS, COL_TILE = 16, 512, 1024, 512
TRANSFORMS = ("pearson", "deviance", "log1p", "counts")


# ------------------------------------------------------------------------------------------------------------------------
# argument checks (all of them before any device work)
# ------------------------------------------------------------------------------------------------------------------------
def _matrix(Y, what):
    if not torch.is_tensor(Y) or Y.dim() != 2 or Y.shape[0] < 1 or Y.shape[1] < 1 or Y.dtype == torch.bool \
            or Y.is_complex():
        shape = f"{Y.dtype} {tuple(Y.shape)}" if torch.is_tensor(Y) else type(Y).__name__
        raise ValueError(f"{what}: Y has shape {shape}; a real [N >= 1, P >= 1] matrix of counts is needed")
    return Y


def _on_device(what, **tensors):
    devs = {name: t.device for name, t in tensors.items() if t is not None}
    for name, d in devs.items():
        if d.type != "cuda":
            raise ValueError(f"{what}: {name} is on device {str(d)!r}; the count kernels run on the GPU only and there is "
                             "no host path - move the tensors to the device first")
    if len(set(devs.values())) > 1:
        raise ValueError(f"{what}: the tensors are on different devices: " + ", ".join(f"{n} on {d}" for n, d in devs.items()))


def _check_theta(theta, what, allow_inf):
    ok = isinstance(theta, (int, float)) and not isinstance(theta, bool) and theta > 0 and not math.isnan(theta)
    if not ok or (math.isinf(theta) and not allow_inf):
        raise ValueError(f"{what}: theta must be a positive number" + (" (inf: Poisson)" if allow_inf else ", finite")
                         + f", not {theta!r}")
    return float(theta)


def _check_views(n_samples_list, N, what):
    try:
        ns = [int(n) for n in n_samples_list]
        ok = len(ns) >= 1 and all(n >= 1 and n == m for n, m in zip(ns, n_samples_list)) and sum(ns) == N
    except (TypeError, ValueError):
        ns, ok = None, False
    if not ok:
        raise ValueError(f"{what}: n_samples_list {n_samples_list!r} must be positive integers that sum to the {N} rows of Y")
    return ns


def _bound(v, name, what):
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or v < 0:
        raise ValueError(f"{what}: {name} must be None or a number >= 0, not {v!r}")
    return v


def _ops():
    from . import engine as E

    return E.ops()


def _f32c(Y):
    return Y.detach().to(f32).contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# the steps over an ops backend ``o`` (HipOps; the tests drive the same code through a fake of their own)
# ------------------------------------------------------------------------------------------------------------------------
def _stats(o, Y):
    rs, cs, rn, cn, bad = o.count_margins(Y)
    return Prediction(row_sum=rs, col_sum=cs, row_nnz=rn, col_nnz=cn, n_invalid=int(bad.item()), total=float(rs.sum()))


def _refuse_invalid(st, what):
    if st.n_invalid > 0:
        raise ValueError(f"{what}: Y holds {st.n_invalid} entries that are NaN, infinite or negative: not a count matrix")


def _log_size_factors(row_sum, what):
    empty = int((row_sum <= 0).sum())
    if empty:
        raise ValueError(f"{what}: {empty} of {row_sum.numel()} rows have no counts, and a size factor is the log of a "
                         "row sum; remove them first (prepare_counts(..., min_counts=1))")
    lrs = torch.log(row_sum)
    return lrs - lrs.mean()


def _deviance(o, Y, col_sum, log_sz):
    ll_sat, abs_sat = o.count_deviance(Y, log_sz)
    sum_sz = torch.exp(log_sz).sum()
    some = col_sum > 0
    ll_null = torch.where(some, col_sum * torch.log(torch.where(some, col_sum, torch.ones_like(col_sum)) / sum_sz),
                          torch.zeros_like(col_sum))
    dev = torch.where(some, 2.0 * (ll_sat - ll_null), torch.zeros_like(col_sum))
    return Prediction(deviance=dev, ll_sat=ll_sat, abs_sat=abs_sat, ll_null=ll_null)


def _order(dev, mask=None, n_top=None):
    """gene indices by descending deviance, equal values by the lower index, restricted to ``mask``"""
    order = torch.sort(dev, descending=True, stable=True).indices
    if mask is not None:
        order = order[mask[order]]
    return order if n_top is None else order[:n_top]


def _median(v):
    s = torch.sort(v).values
    n = s.numel()
    return float(s[n // 2]) if n % 2 else 0.5 * (float(s[n // 2 - 1]) + float(s[n // 2]))


def _residuals(o, Y, st, kind, theta, clip, out):
    if st.total <= 0:
        raise ValueError("the matrix holds no counts at all")
    if kind == "pearson":
        return o.count_transform(Y, "pearson", st.row_sum, st.col_sum, total=st.total, theta=theta, clip=clip, out=out)
    mode = "poisson_deviance" if math.isinf(theta) else "nb_deviance"
    return o.count_transform(Y, mode, st.row_sum, st.col_sum, total=st.total, theta=theta, out=out)


def _target(row_sum, target_sum, what):
    if target_sum is None:
        some = row_sum[row_sum > 0]
        if some.numel() == 0:
            raise ValueError(f"{what}: the matrix holds no counts at all")
        return _median(some)
    if isinstance(target_sum, bool) or not isinstance(target_sum, (int, float)) or not 0 < target_sum < math.inf:
        raise ValueError(f"{what}: target_sum must be None or a positive finite number, not {target_sum!r}")
    return float(target_sum)


def _offsets(ns):
    off = [0]
    for n in ns:
        off.append(off[-1] + n)
    return off


def _prepare(o, Y, ns, min_counts, max_counts, min_cells, n_top_genes, transform, theta, standardize):
    what = "prepare_counts"
    N, P = (int(s) for s in Y.shape)
    # 1. rows, on the row sums over all genes
    st = _stats(o, Y)
    _refuse_invalid(st, what)
    keep = torch.ones(N, dtype=torch.bool, device=Y.device)
    if min_counts is not None:
        keep &= st.row_sum >= min_counts
    if max_counts is not None:
        keep &= st.row_sum <= max_counts
    rows = torch.nonzero(keep).flatten()
    off = _offsets(ns)
    kept = torch.cat([keep.new_zeros(1, dtype=torch.int64), torch.cumsum(keep.to(torch.int64), 0)])[off].tolist()
    ns_kept = [b - a for a, b in zip(kept, kept[1:])]
    if min(ns_kept) < 1:
        raise ValueError(f"{what}: the row filter leaves {ns_kept} rows in the views: every view needs at least one")
    fresh = rows.numel() < N  # Yr is a copy of ours from here on
    Yr = Y[rows].contiguous() if fresh else Y
    # 2. genes, on the margins of the kept rows
    st_r = _stats(o, Yr) if fresh else st
    passed = None if min_cells is None else st_r.col_nnz >= min_cells
    # 3. ranking: the deviance over all genes of the kept rows (a row without counts is refused here)
    log_sz = _log_size_factors(st_r.row_sum, what)
    dev = _deviance(o, Yr, st_r.col_sum, log_sz).deviance
    if n_top_genes is None and passed is None:
        genes = torch.arange(P, device=Y.device)
    else:
        genes = torch.sort(_order(dev, passed, n_top_genes)).values
    if genes.numel() < 1:
        raise ValueError(f"{what}: no gene passes min_cells = {min_cells!r}")
    if genes.numel() < P:
        Ysel, fresh = Yr[:, genes].contiguous(), True
    else:
        Ysel = Yr
    # 4. the transform
    out_buf = Ysel if fresh else None  # in place on a copy of ours, never on the caller's matrix
    log_offset, n_constant = None, None
    if transform == "counts":
        outputs, log_offset = (Ysel if fresh else Ysel.clone()), log_sz.to(f32)  # never the caller's own tensor
    elif transform == "log1p":
        outputs = o.count_transform(Ysel, "log1p", st_r.row_sum, target=_target(st_r.row_sum, None, what), out=out_buf)
    else:
        st_s = _stats(o, Ysel) if genes.numel() < P else st_r
        clip = math.sqrt(Ysel.shape[0])
        try:
            outputs = _residuals(o, Ysel, st_s, transform, theta, clip, out_buf)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
    # 5. the z-score per view
    if transform != "counts" and standardize:
        outputs, n_constant = o.standardize_views(outputs, _offsets(ns_kept), out=outputs)
    return Prediction(outputs=outputs, log_offset=log_offset, rows=rows, genes=genes, n_samples_list=ns_kept,
                      deviance=dev, n_constant=n_constant)


# ------------------------------------------------------------------------------------------------------------------------
# the public calls
# ------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def count_stats(Y):
    """The margins of ``Y`` [N, P] in one read: a ``Prediction`` with ``row_sum`` [N] and ``col_sum`` [P] (fp64, exact
    for counts), ``row_nnz`` [N] and ``col_nnz`` [P] (int64: the entries > 0), ``total`` (float) and ``n_invalid`` (int:
    the entries that are NaN, infinite or negative - reported here, refused by every other call)."""
    what = "count_stats"
    _matrix(Y, what)
    _on_device(what, Y=Y)
    return _stats(_ops(), _f32c(Y))


@torch.no_grad()
def size_factors(Y, log=False):
    """Per-spot size factors with geometric mean 1: ``exp(log rs - mean(log rs))`` of the row sums ``rs`` (util.py:155-164),
    [N] fp64; ``log=True`` returns their logs (what ``log_offset`` takes).  A row without counts raises a ``ValueError``
    that states how many there are: remove them with ``prepare_counts(min_counts=1)``."""
    what = "size_factors"
    _matrix(Y, what)
    _on_device(what, Y=Y)
    st = _stats(_ops(), _f32c(Y))
    _refuse_invalid(st, what)
    lsz = _log_size_factors(st.row_sum, what)
    return lsz if log else torch.exp(lsz)


@torch.no_grad()
def poisson_deviance(Y, log_sz=None, return_parts=False):
    """The Poisson deviance per gene against the null of one rate per gene scaled by the size factors (util.py:167-178):
    ``2 (ll_sat - ll_null)`` with ``ll_sat[g] = sum_i y log(y / sz_i)`` over the entries > 0 and ``ll_null[g] = cs_g
    log(cs_g / sum_i sz_i)``, [P] fp64.  ``log_sz`` [N]: the log size factors (default: ``size_factors(Y, log=True)``).
    A gene without counts gives exactly 0.  ``return_parts``: a ``Prediction`` with ``deviance``, ``ll_sat``, ``ll_null``
    and ``abs_sat`` (the sum of the magnitudes of ll_sat's terms: the scale of its rounding error)."""
    res = _poisson_deviance("poisson_deviance", Y, log_sz)
    return res if return_parts else res.deviance


def _poisson_deviance(what, Y, log_sz=None):
    """the checks and the two reads behind poisson_deviance and deviance_feature_selection, refusing under ``what``"""
    _matrix(Y, what)
    if log_sz is not None and (not torch.is_tensor(log_sz) or tuple(log_sz.shape) != (Y.shape[0],)
                               or not log_sz.is_floating_point()):
        raise ValueError(f"{what}: log_sz must be a floating-point tensor of shape [{Y.shape[0]}]")
    _on_device(what, Y=Y, log_sz=log_sz)
    o, Y = _ops(), _f32c(Y)
    st = _stats(o, Y)
    _refuse_invalid(st, what)
    lsz = _log_size_factors(st.row_sum, what) if log_sz is None else log_sz.detach().to(f64).contiguous()
    return _deviance(o, Y, st.col_sum, lsz)


@torch.no_grad()
def deviance_feature_selection(Y, n_top=None):
    """Genes ranked by Poisson deviance (util.py:181-197): a ``Prediction`` with ``deviance`` [P] fp64 and ``order``
    (int64 gene indices by descending deviance, equal values by the lower index; the first ``n_top`` when given).  Genes
    without counts have deviance 0 and rank last (the reference drops them)."""
    what = "deviance_feature_selection"
    _matrix(Y, what)
    if n_top is not None and (isinstance(n_top, bool) or not isinstance(n_top, int) or not 1 <= n_top <= Y.shape[1]):
        raise ValueError(f"{what}: n_top must be None or an integer in [1, {Y.shape[1]}], not {n_top!r}")
    dev = _poisson_deviance(what, Y).deviance
    return Prediction(deviance=dev, order=_order(dev, None, n_top))


@torch.no_grad()
def pearson_residuals(Y, theta=100.0, clipping=True, inplace=False):
    """Analytic Pearson residuals of a negative binomial null with fixed ``theta`` (util.py:238-254): with ``mu = rs_i
    cs_g / total`` from the margins of ``Y`` itself, ``(y - mu) / sqrt(mu + mu^2 / theta)``, clipped to +-sqrt(N) when
    ``clipping``; [N, P] fp32 (fp64 arithmetic, rounded once).  ``inplace``: overwrite ``Y`` (contiguous fp32 only)."""
    return _residual_call("pearson_residuals", "pearson", Y, _check_theta(theta, "pearson_residuals", True),
                          bool(clipping), inplace)


@torch.no_grad()
def deviance_residuals(Y, theta, inplace=False):
    """Deviance residuals of a negative binomial null with fixed ``theta``, or of a Poisson null for ``theta=inf``
    (util.py:200-235), margins as in ``pearson_residuals``; a negative square-root term is set to 0."""
    return _residual_call("deviance_residuals", "deviance", Y, _check_theta(theta, "deviance_residuals", True), False,
                          inplace)


def _inplace_ok(Y, inplace, what):
    if inplace and (Y.dtype != f32 or not Y.is_contiguous()):
        raise ValueError(f"{what}: inplace=True needs a contiguous fp32 Y, not {Y.dtype}"
                         + ("" if Y.is_contiguous() else ", not contiguous"))
    return Y if inplace else None


def _residual_call(what, kind, Y, theta, clipping, inplace):
    _matrix(Y, what)
    out = _inplace_ok(Y, inplace, what)
    _on_device(what, Y=Y)
    o, Y = _ops(), _f32c(Y)
    st = _stats(o, Y)
    _refuse_invalid(st, what)
    try:
        return _residuals(o, Y, st, kind, theta, math.sqrt(Y.shape[0]) if clipping else 0.0, out)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None


@torch.no_grad()
def normalize_log1p(Y, target_sum=None, inplace=False):
    """``log1p(y * target_sum / rs_i)`` with ``rs_i`` the row sums: scanpy's ``normalize_total`` followed by ``log1p``, as
    a formula.  ``target_sum=None``: the median of the row sums of the rows that have counts (the mean of the two middle
    values for an even number of them).  A row without counts stays 0.  [N, P] fp32."""
    what = "normalize_log1p"
    _matrix(Y, what)
    if target_sum is not None:
        _target(None, target_sum, what)
    out = _inplace_ok(Y, inplace, what)
    _on_device(what, Y=Y)
    o, Y = _ops(), _f32c(Y)
    st = _stats(o, Y)
    _refuse_invalid(st, what)
    return o.count_transform(Y, "log1p", st.row_sum, target=_target(st.row_sum, target_sum, what), out=out)


@torch.no_grad()
def standardize_views(Y, n_samples_list, inplace=False):
    """The z-score per (view, column): ``(y - mean) / std`` over each view's consecutive rows (``n_samples_list``), ``std``
    the population value (``numpy.std``), moments in fp64 by Welford / Chan.  A ``Prediction`` with ``outputs`` [N, P] fp32
    and ``n_constant`` [V] int64: the columns that are constant within a view, which are written as 0 (the reference
    writes NaN there, which would poison the ELBO).  ``Y`` need not be counts (residuals are negative), so ``n_invalid``
    does not apply here; a NaN or an infinite entry is refused with a ``ValueError`` (one more read of ``Y``: the margins' row sums)."""
    what = "standardize_views"
    _matrix(Y, what)
    ns = _check_views(n_samples_list, int(Y.shape[0]), what)
    out = _inplace_ok(Y, inplace, what)
    _on_device(what, Y=Y)
    o, Y = _ops(), _f32c(Y)
    # the margins' fp64 row sums: a NaN or an infinite entry makes its row's sum non-finite, finite fp32 values cannot
    bad_rows = int((~torch.isfinite(o.count_margins(Y)[0])).sum())
    if bad_rows:
        raise ValueError(f"{what}: Y holds NaN or infinite entries (in {bad_rows} rows); their columns' moments would be NaN")
    outputs, n_constant = o.standardize_views(Y, _offsets(ns), out=out)
    return Prediction(outputs=outputs, n_constant=n_constant)


@torch.no_grad()
def prepare_counts(Y, n_samples_list, *, min_counts=None, max_counts=None, min_cells=None, n_top_genes=None,
                   transform="pearson", theta=100.0, standardize=True):
    """From raw counts ``Y`` [N, P] (the views' rows one after the other, ``n_samples_list``) to the outputs of a fit, in
    the order the reference's experiments use:

    1. rows with ``min_counts <= row sum <= max_counts`` are kept (``None``: no bound at that end).  A spot without counts
       is NOT dropped implicitly: it is refused at step 3, so remove such rows with ``min_counts >= 1``;
    2. genes seen (> 0) in at least ``min_cells`` of the kept rows pass;
    3. the Poisson deviance of all genes over the kept rows ranks them; the top ``n_top_genes`` of those that passed are
       selected (``None``: all that passed), kept in their original column order;
    4. ``transform``: "log1p" (row sums over ALL genes of the kept rows, target: their median), "pearson" /
       "deviance" (analytic residuals with ``theta``, margins of the SELECTED sub-matrix), or "counts": the selected
       counts untouched plus ``log_offset``, the log size factors in fp32 from all genes - the pair the Poisson /
       negative binomial likelihood takes;
    5. the z-score per view (``standardize``; never for "counts").

    Returns a ``Prediction``: ``outputs`` [N', P'] fp32, ``log_offset`` ([N'] fp32, None except for "counts"), ``rows`` and
    ``genes`` (the kept indices, int64, ascending), ``n_samples_list`` of the kept rows, ``deviance`` ([P] fp64, over the
    kept rows) and ``n_constant`` ([V] int64 or None).  ``Y`` itself is never modified, and ``outputs`` never shares its
    memory (a copy even where no row or gene is dropped)."""
    what = "prepare_counts"
    _matrix(Y, what)
    N, P = (int(s) for s in Y.shape)
    ns = _check_views(n_samples_list, N, what)
    if transform not in TRANSFORMS:
        raise ValueError(f"{what}: transform must be one of {TRANSFORMS}, not {transform!r}")
    min_counts, max_counts = _bound(min_counts, "min_counts", what), _bound(max_counts, "max_counts", what)
    min_cells = _bound(min_cells, "min_cells", what)
    if n_top_genes is not None and (isinstance(n_top_genes, bool) or not isinstance(n_top_genes, int) or n_top_genes < 1):
        raise ValueError(f"{what}: n_top_genes must be None or a positive integer, not {n_top_genes!r}")
    theta = _check_theta(theta, what, True)
    _on_device(what, Y=Y)
    return _prepare(_ops(), _f32c(Y), ns, min_counts, max_counts, min_cells, n_top_genes, transform, theta,
                    bool(standardize))
