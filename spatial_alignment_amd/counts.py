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
* ``column_moments``, ``highly_variable_genes``: mean and variance per (view, gene) in one read (csrc/moments.hip, dense
  and CSR) and scanpy's Seurat-flavoured dispersion ranking on them - the gene selection the experiments' real-data
  scripts use, and their per-slice variance filter;
* ``prepare_counts``: the one call, in the order the experiments use (``selection="deviance"`` or ``"seurat"``);
* ``csr_counts`` / ``CSRCounts`` / ``densify``: sparse input (csrc/counts_sparse.hip).  ``count_stats``, ``size_factors``,
  ``poisson_deviance``, ``deviance_feature_selection`` and ``prepare_counts`` take a ``CSRCounts`` or a ``torch.sparse_csr``
  tensor where they take ``Y``, with the same return fields, and never build the dense [N, P] matrix: the margins and
  the deviance are sums over the stored entries, the row filter is a mask, and only the selected block becomes dense.
  Integer counts give the dense path's sums bit for bit; non-integer values agree to rounding.  The four calls whose
  result is dense N x P refuse sparse input and point to ``prepare_counts`` / ``densify``.

Deliberate departures from the reference: a gene with no counts has deviance exactly 0 (the reference drops it) and
residual 0 (the reference divides 0 by 0); a column that is constant within a view standardises to 0 and is counted (the
reference writes NaN); a spot with no counts is refused by name (the reference takes log 0); equal deviances rank by
the lower gene index.  Everything runs under ``torch.no_grad()``.  Tensors on the CPU are refused with a ``ValueError``
that names the device: there is no host path.
"""
import math

import torch

from ._args import as_device, describe, on_device, ops as _ops, view_offsets
from .predict import Prediction

f64, f32 = torch.float64, torch.float32
# csrc/counts.hip: the rows of a group (at least / at most), the cap on the groups, the columns of a tile.  A matrix of
# more than ROWS_MIN * MAX_GROUPS rows has more row blocks than the cap, and its groups grow.
ROWS_MIN, ROWS_MAX, MAX_GROUPS, COL_TILE = 16, 512, 1024, 512
# csrc/counts_sparse.hip: the rows of a group (at least), the cap on the groups, the columns of a tile, the output columns
# the gather assembles at a time
CSR_ROWS_MIN, CSR_MAX_GROUPS, CSR_COL_TILE, CSR_GATHER_TILE = 16, 32, 512, 8192
TRANSFORMS = ("pearson", "deviance", "log1p", "counts")
# csrc/moments.hip: the rows of a group (at least), the caps on a view's groups (dense, CSR), the columns of a tile
MOM_ROWS_MIN, MOM_MAX_GROUPS, MOM_CSR_MAX_GROUPS, MOM_COL_TILE = 16, 512, 16, 512
MOMENT_TRANSFORMS = ("identity", "expm1", "normalize")
SELECTIONS = ("deviance", "seurat")
COMBINE = ("intersection", "union")
HVG_DEFAULTS = dict(min_mean=0.0125, max_mean=3, min_disp=0.5, max_disp=math.inf, n_bins=20)  # scanpy's


# ------------------------------------------------------------------------------------------------------------------------
# argument checks (all of them before any device work)
# ------------------------------------------------------------------------------------------------------------------------
def _matrix(Y, what):
    if not torch.is_tensor(Y) or Y.dim() != 2 or Y.shape[0] < 1 or Y.shape[1] < 1 or Y.dtype == torch.bool \
            or Y.is_complex():
        raise ValueError(f"{what}: Y has shape {describe(Y)}; a real [N >= 1, P >= 1] matrix of counts is needed")
    return Y


def _on_device(what, **tensors):
    """(a name of this module: the tests that drive it through a fake backend on the host replace it)"""
    on_device(what, "count", **tensors)


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


# ------------------------------------------------------------------------------------------------------------------------
# the steps over an ops backend ``o`` (HipOps; the tests drive the same code through a fake of their own)
# ------------------------------------------------------------------------------------------------------------------------
def _stats(o, src):
    """the margins of a source of counts (_DenseCounts / _SparseCounts below)"""
    rs, cs, rn, cn, bad = src.margins(o)
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


def _deviance(o, src, col_sum, log_sz):
    return _close_deviance(*src.deviance_sums(o, log_sz), col_sum, log_sz)


def _close_deviance(ll_sat, abs_sat, col_sum, log_sz):
    """2 (ll_sat - ll_null) from the entry's two sums; ``log_sz``: of the rows the sums ran over"""
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


def _transform_selected(o, Ysel, fresh, margins, row_sum, log_sz, ns_kept, transform, theta, standardize, what):
    """steps 4 and 5 of prepare_counts on the selected dense block ``Ysel`` (``fresh``: a copy of ours, transformed in
    place).  ``margins()``: the margins of Ysel itself; ``row_sum``: of the kept rows over ALL genes
    -> (outputs, log_offset, n_constant)"""
    out_buf = Ysel if fresh else None  # in place on a copy of ours, never on the caller's matrix
    log_offset, n_constant = None, None
    if transform == "counts":
        outputs, log_offset = (Ysel if fresh else Ysel.clone()), log_sz.to(f32)  # never the caller's own tensor
    elif transform == "log1p":
        outputs = o.count_transform(Ysel, "log1p", row_sum, target=_target(row_sum, None, what), out=out_buf)
    else:
        st_s = margins()
        clip = math.sqrt(Ysel.shape[0])
        try:
            outputs = _residuals(o, Ysel, st_s, transform, theta, clip, out_buf)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
    if transform != "counts" and standardize:
        outputs, n_constant = o.standardize_views(outputs, view_offsets(ns_kept), out=outputs)
    return outputs, log_offset, n_constant


def _view_counts(keep, ns, what):
    """the rows each view keeps under the mask ``keep``; every view needs one"""
    off = view_offsets(ns)
    kept = torch.cat([keep.new_zeros(1, dtype=torch.int64), torch.cumsum(keep.to(torch.int64), 0)])[off].tolist()
    ns_kept = [b - a for a, b in zip(kept, kept[1:])]
    if min(ns_kept) < 1:
        raise ValueError(f"{what}: the row filter leaves {ns_kept} rows in the views: every view needs at least one")
    return ns_kept


# ------------------------------------------------------------------------------------------------------------------------
# per-view column moments and the Seurat ranking on them (csrc/moments.hip; the ranking is fp64 torch on P-long vectors)
# ------------------------------------------------------------------------------------------------------------------------
def _scale(row_sum, target):
    """target / row sum per row, 0 for a row without counts: what mode "normalize" multiplies a row by"""
    some = row_sum > 0
    return torch.where(some, target / torch.where(some, row_sum, torch.ones_like(row_sum)), torch.zeros_like(row_sum))


def _close_moments(s1, s2, n):
    """mean and scanpy's variance (mean of squares - mean^2) n / (n - 1) from the sums; ``n``: rows per view, a list"""
    n = torch.tensor([float(v) for v in n], dtype=f64, device=s1.device).unsqueeze(1)
    mean = s1 / n
    var = (s2 / n - mean * mean) * (n / (n - 1.0))
    return mean, var


def _seurat_bins(means, sel, n_bins):
    """the bin of every gene: ``n_bins`` equal-width, right-closed bins over [min, max] of ``means[sel]`` with the lowest
    edge moved down by 0.1 % of the range, and both ends moved out by 0.1 % of their magnitude (0.001 at 0) where the range
    is zero - ``pandas.cut(x, bins=n)``; the edges are ``numpy.linspace``'s, start + i step with the last one set to the
    maximum -> (bin [P] int64 in [0, n_bins), edges [n_bins + 1])"""
    inf = torch.full_like(means, math.inf)
    mn, mx = torch.where(sel, means, inf).min(), torch.where(sel, means, -inf).max()
    same = mn == mx
    pad = lambda v: torch.where(v != 0, 0.001 * v.abs(), torch.full_like(v, 0.001))
    lo, hi = torch.where(same, mn - pad(mn), mn), torch.where(same, mx + pad(mx), mx)
    edges = torch.arange(n_bins + 1, dtype=f64, device=means.device) * ((hi - lo) / n_bins) + lo
    edges[-1] = hi
    edges[0] = torch.where(same, edges[0], edges[0] - (mx - mn) * 0.001)
    idx = torch.searchsorted(edges, means.contiguous()) - 1  # right-closed: a value on an edge belongs to the bin below
    return idx.clamp_(0, n_bins - 1), edges


def _seurat_rank(mean, var, sel, n_bins):
    """scanpy's ``highly_variable_genes(flavor="seurat")`` for one view, on ``mean`` / ``var`` [P] fp64 of the normalised
    counts, restricted to the genes ``sel`` [P] bool -> (means, dispersions, dispersions_norm, bin), NaN in
    dispersions_norm outside ``sel``.  Every sum is a masked ``sum`` over the genes in torch's fixed order; the largest
    temporary is [n_bins, P] doubles."""
    nan = torch.full_like(mean, math.nan)
    mean = torch.where(mean == 0, torch.full_like(mean, 1e-12), mean)
    disp = var / mean
    disp = torch.log(torch.where(disp == 0, nan, disp))
    means = torch.log1p(mean)
    idx, _ = _seurat_bins(means, sel, n_bins)
    valid = sel & ~torch.isnan(disp)
    d0 = torch.where(valid, disp, torch.zeros_like(disp))
    # mean and ddof = 1 standard deviation per bin, NaN skipped, two-pass: row b of ``member`` [n_bins, P] is bin b
    member = valid.unsqueeze(0) & (idx.unsqueeze(0) == torch.arange(n_bins, device=idx.device).unsqueeze(1))
    zero = torch.zeros((), dtype=f64, device=mean.device)
    cnt = member.sum(1).to(f64)
    bmean = torch.where(member, d0.unsqueeze(0), zero).sum(1) / cnt  # (an empty bin: 0 / 0)
    ss = torch.where(member, (d0.unsqueeze(0) - bmean.unsqueeze(1)) ** 2, zero).sum(1)
    bstd = torch.where(cnt >= 2, torch.sqrt(ss / (cnt - 1.0)), nan[0])
    one = torch.isnan(bstd)  # a bin of one gene: its normalised dispersion is 1
    bstd = torch.where(one, bmean, bstd)
    bmean = torch.where(one, torch.zeros_like(bmean), bmean)
    dnorm = torch.where(sel, (disp - bmean[idx]) / bstd[idx], nan)
    return means, disp, dnorm, idx


def _seurat_select(means, dnorm, sel, n_top_genes, min_mean, max_mean, min_disp, max_disp, what):
    """-> highly_variable [P] bool"""
    if n_top_genes is None:
        dn = torch.where(torch.isnan(dnorm), torch.zeros_like(dnorm), dnorm)
        return sel & (means > min_mean) & (means < max_mean) & (dn > min_disp) & (dn < max_disp)
    ranked = sel & ~torch.isnan(dnorm)
    n_ranked = int(ranked.sum())
    if n_ranked < 1:
        raise ValueError(f"{what}: no gene has a normalised dispersion (all NaN): nothing to rank")
    if n_top_genes > n_ranked:
        import warnings

        warnings.warn(f"{what}: n_top_genes = {n_top_genes} is more than the {n_ranked} genes with a normalised "
                      "dispersion; all of them are selected")
        n_top_genes = n_ranked
    top = torch.topk(torch.where(ranked, dnorm, torch.full_like(dnorm, -math.inf)), n_top_genes).values
    return sel & (torch.nan_to_num(dnorm) >= top[-1])  # ties at the cutoff are all kept


def _check_hvg(what, n_top_genes, min_mean, max_mean, min_disp, max_disp, n_bins, combine):
    if n_top_genes is not None and (isinstance(n_top_genes, bool) or not isinstance(n_top_genes, int) or n_top_genes < 1):
        raise ValueError(f"{what}: n_top_genes must be None or a positive integer, not {n_top_genes!r}")
    for name, v in (("min_mean", min_mean), ("max_mean", max_mean), ("min_disp", min_disp), ("max_disp", max_disp)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ValueError(f"{what}: {name} must be a number, not {v!r}")
    if isinstance(n_bins, bool) or not isinstance(n_bins, int) or n_bins < 1:
        raise ValueError(f"{what}: n_bins must be a positive integer, not {n_bins!r}")
    if combine not in COMBINE:
        raise ValueError(f"{what}: combine must be one of {COMBINE}, not {combine!r}")


def _check_moment_views(n_samples_list, N, what):
    ns = [N] if n_samples_list is None else _check_views(n_samples_list, N, what)
    if min(ns) < 2:
        raise ValueError(f"{what}: the views have {ns} rows; a variance needs at least 2 in every view")
    return ns


def _check_moment_transform(transform, target_sum, what):
    if transform not in MOMENT_TRANSFORMS:
        raise ValueError(f"{what}: transform must be one of {MOMENT_TRANSFORMS}, not {transform!r}")
    if target_sum is not None:
        _target(None, target_sum, what)
        if transform != "normalize":
            raise ValueError(f"{what}: target_sum goes with transform='normalize', not with {transform!r}")


def _moments(o, src, ns, transform, target_sum, what):
    """the sums of one read of the matrix (two for "normalize": the row sums first), closed -> Prediction"""
    scale = None
    if transform == "normalize":
        st = _stats(o, src)
        _refuse_invalid(st, what)
        scale = _scale(st.row_sum, _target(st.row_sum, target_sum, what))
    s1, s2, ab, bad = src.moments(o, transform, view_offsets(ns), scale)
    mean, var = _close_moments(s1, s2, ns)
    return Prediction(mean=mean, var=var, n_nonfinite=int(bad.item()), abs_sum=ab)


def _prepare_seurat(o, src, row_sum, passed, n_top_genes, what):
    """step 3 of prepare_counts with selection="seurat": pooled over the rows of ``src`` (the kept ones), from the raw
    counts (mode "normalize": the row sums over all genes, their median as the target) -> (genes, dispersions_norm)"""
    n_rows = src.shape[0]
    if n_rows < 2:
        raise ValueError(f"{what}: the row filter leaves {n_rows} rows; selection='seurat' needs a variance, so at least 2")
    s1, s2, _, _ = src.moments(o, "normalize", [0, n_rows], _scale(row_sum, _target(row_sum, None, what)))
    mean, var = _close_moments(s1, s2, [n_rows])
    sel = torch.ones_like(mean[0], dtype=torch.bool) if passed is None else passed
    means, _, dnorm, _ = _seurat_rank(mean[0], var[0], sel, HVG_DEFAULTS["n_bins"])
    hv = _seurat_select(means, dnorm, sel, n_top_genes, HVG_DEFAULTS["min_mean"], HVG_DEFAULTS["max_mean"],
                        HVG_DEFAULTS["min_disp"], HVG_DEFAULTS["max_disp"], what)
    return torch.nonzero(hv).flatten(), dnorm


# ------------------------------------------------------------------------------------------------------------------------
# sparse input: a CSR matrix on the device (csrc/counts_sparse.hip)
# ------------------------------------------------------------------------------------------------------------------------
class CSRCounts:
    """A checked count matrix in CSR on the device, what ``csr_counts`` returns: ``crow`` [N + 1] int64, ``col`` [nnz]
    int32 and ``values`` [nnz] fp32 (contiguous), ``shape`` (N, P), ``nnz`` and ``n_stored_zeros`` (the explicitly stored
    zeros: allowed, they count as absent).  Rows are sorted by column and hold no duplicates.  Build it with
    ``csr_counts``: the constructor itself checks nothing."""
    __slots__ = ("crow", "col", "values", "shape", "nnz", "n_stored_zeros")

    def __init__(self, crow, col, values, shape, n_stored_zeros=0):
        self.crow, self.col, self.values = crow, col, values
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz, self.n_stored_zeros = int(col.numel()), int(n_stored_zeros)

    @property
    def device(self):
        return self.values.device

    def __repr__(self):
        return f"CSRCounts(shape={self.shape}, nnz={self.nnz}, n_stored_zeros={self.n_stored_zeros}, device={self.device})"


def _is_scipy_sparse(m):
    return type(m).__module__.startswith("scipy.sparse") and hasattr(m, "tocsr")


def _is_sparse_tensor(Y):
    return torch.is_tensor(Y) and Y.layout != torch.strided


def _is_sparse(Y):
    return isinstance(Y, CSRCounts) or _is_sparse_tensor(Y) or _is_scipy_sparse(Y)


def _upload_device(device, what):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError(f"{what}: device {str(dev)!r}: the count kernels run on the GPU only and there is no host path")
    return dev


def _csr_parts(matrix, what):
    """(crow, col, values, shape) of a torch.sparse_csr tensor or a 4-tuple, checked on the host: shapes, dtypes, one
    device - before any device work"""
    if _is_sparse_tensor(matrix):
        if matrix.layout != torch.sparse_csr:
            raise ValueError(f"{what}: a sparse tensor must have layout torch.sparse_csr, not {matrix.layout}; convert it "
                             "with .to_sparse_csr()")
        if matrix.dim() != 2:
            raise ValueError(f"{what}: the sparse tensor has shape {tuple(matrix.shape)}; a [N, P] matrix is needed")
        parts = (matrix.crow_indices(), matrix.col_indices(), matrix.values(), tuple(matrix.shape))
    elif isinstance(matrix, (tuple, list)) and len(matrix) == 4:
        parts = tuple(matrix)
    else:
        raise ValueError(f"{what}: a scipy.sparse matrix, a torch.sparse_csr tensor, a (crow, col, values, shape) tuple of "
                         f"device tensors or a CSRCounts is needed, not {type(matrix).__name__}")
    crow, col, val, shape = parts
    try:
        N, P = (int(v) for v in shape)
        ok = len(tuple(shape)) == 2 and 1 <= N < 2**31 and 1 <= P < 2**31
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: shape {shape!r} must be (N, P) with 1 <= N, P < 2^31")
    for name, t in (("crow", crow), ("col", col), ("values", val)):
        if not torch.is_tensor(t) or t.dim() != 1 or t.layout != torch.strided:
            raise ValueError(f"{what}: {name} must be a 1-D tensor, not {describe(t)}")
    for name, t in (("crow", crow), ("col", col)):
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: {name} has dtype {t.dtype}; the index dtypes are int32 and int64")
    if val.dtype == torch.bool or val.is_complex():
        raise ValueError(f"{what}: values has dtype {val.dtype}; real counts are needed")
    if crow.numel() != N + 1:
        raise ValueError(f"{what}: crow has {crow.numel()} entries, shape {(N, P)} needs N + 1 = {N + 1}")
    if col.numel() != val.numel():
        raise ValueError(f"{what}: nnz differs: col has {col.numel()} entries, values has {val.numel()}")
    if col.numel() > N * P:
        raise ValueError(f"{what}: nnz = {col.numel()} is more than N * P = {N * P}")
    _on_device(what, crow=crow, col=col, values=val)
    return crow, col, val, (N, P)


def _checked(o, crow, col, val, shape, what):
    """the device check of arrays already in the kernels' types -> CSRCounts, or the ValueError that names the rule"""
    N, P = shape
    n_crow, n_range, n_order, n_zero = (int(v) for v in o.csr_check(crow, col, val, N, P).tolist())
    if n_crow:
        raise ValueError(f"{what}: crow is not a row pointer: {n_crow} violations (crow[0] must be 0, crow must not "
                         f"decrease, crow[N] must be nnz = {col.numel()})")
    if n_range:
        raise ValueError(f"{what}: {n_range} column indices are outside [0, {P})")
    if n_order:
        raise ValueError(f"{what}: rows are not sorted / hold duplicates: at {n_order} places a row's column index does not "
                         "strictly increase; use scipy's sum_duplicates / sort_indices or torch's coalesce first")
    return CSRCounts(crow, col, val, shape, n_zero)


def csr_counts(matrix, device=None, _what="csr_counts"):
    """A count matrix in sparse form -> ``CSRCounts`` on the device, checked.  ``matrix`` is one of

    * a scipy.sparse matrix of any format (scipy is imported only when one is passed): canonicalised on the host with
      ``tocsr``, ``sum_duplicates`` and ``sort_indices`` (on a copy: the caller's matrix is not modified), then uploaded to
      ``device`` (default: the current HIP device);
    * a ``torch.sparse_csr`` tensor on the device;
    * a tuple ``(crow, col, values, shape)`` of device tensors;
    * a ``CSRCounts``, returned as it is.

    Index dtypes int32 and int64 are accepted.  ``crow`` is taken to int64, ``col`` to int32 and the values to fp32:
    each conversion that changes a dtype (or makes a tensor contiguous) copies that one array, an array already in its
    type is shared with the caller, not copied.  Device-side input is never rewritten: it is checked by one kernel
    (``gpsa_csr_check``) and a ``ValueError`` names the violated rule with its count - a malformed row pointer, column
    indices outside [0, P), rows that are not sorted or hold duplicates.  Explicitly stored zeros are allowed and counted
    in ``n_stored_zeros``.  CPU tensors are refused: there is no host path."""
    what = _what
    if isinstance(matrix, CSRCounts):
        return matrix
    if _is_scipy_sparse(matrix):
        import numpy as np

        dev = _upload_device(device, what)
        m = matrix.tocsr(copy=True)
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1 or m.shape[1] >= 2**31 or m.dtype.kind not in "iuf":
            raise ValueError(f"{what}: the matrix has shape {m.shape} and dtype {m.dtype}; a real [N >= 1, P >= 1] matrix of "
                             "counts is needed")
        m.sum_duplicates()
        m.sort_indices()
        parts = (torch.from_numpy(m.indptr.astype(np.int64)).to(dev), torch.from_numpy(m.indices.astype(np.int32)).to(dev),
                 torch.from_numpy(m.data.astype(np.float32)).to(dev), tuple(int(v) for v in m.shape))
    else:
        if device is not None:
            raise ValueError(f"{what}: device is for scipy input; tensors stay where they are")
        parts = _csr_parts(matrix, what)
    crow, col, val, shape = parts
    crow, col, val = as_device(crow, torch.int64), as_device(col, torch.int32), as_device(val, f32)
    return _checked(_ops(), crow, col, val, shape, what)


def _sparse_arg(Y, what):
    """the CSRCounts behind a sparse ``Y`` (a torch.sparse_csr tensor is checked here, on entry), or None for a dense one"""
    if isinstance(Y, CSRCounts):
        return Y
    if _is_sparse_tensor(Y) or _is_scipy_sparse(Y):
        if _is_scipy_sparse(Y):
            raise ValueError(f"{what}: Y is a scipy.sparse matrix; upload it once with csr_counts(Y) and pass the result")
        return csr_counts(Y, _what=what)
    return None


def _refuse_sparse(Y, what):
    if _is_sparse(Y):
        raise ValueError(f"{what}: Y is sparse, and the result of {what} is a dense N x P matrix; use prepare_counts, which "
                         "makes only the selected block dense, or densify(csr, rows, genes) first")


def _index_list(idx, n, name, what, device, unique):
    """None (all) or indices into [0, n) -> int64 tensor on the device"""
    if idx is None:
        return torch.arange(n, device=device)
    t = torch.as_tensor(idx)
    if t.dim() != 1 or t.numel() < 1 or t.dtype in (torch.bool,) or t.is_floating_point() or t.is_complex():
        raise ValueError(f"{what}: {name} must be None or a non-empty 1-D integer index list")
    t = t.to(device=device, dtype=torch.int64).contiguous()
    if int(t.min()) < 0 or int(t.max()) >= n:
        raise ValueError(f"{what}: {name} holds indices outside [0, {n})")
    if unique and torch.unique(t).numel() != t.numel():
        raise ValueError(f"{what}: {name} holds an index twice")
    return t


def _gather(o, A, rows, genes):
    N, P = A.shape
    slot = torch.full((P,), -1, dtype=torch.int32, device=A.device)
    slot[genes] = torch.arange(genes.numel(), dtype=torch.int32, device=A.device)
    return o.csr_gather_dense(A.crow, A.col, A.values, N, P, rows, slot, int(genes.numel()))


@torch.no_grad()
def densify(csr, rows=None, genes=None):
    """The block ``[rows, genes]`` of a sparse count matrix as a dense fp32 ``[len(rows), len(genes)]`` tensor with zeros
    where nothing is stored (``None``: all rows / all genes).  ``csr``: a ``CSRCounts`` or anything ``csr_counts`` takes.
    ``genes`` must not repeat an index.  One kernel; each element is written once."""
    what = "densify"
    A = csr_counts(csr, _what=what)
    rows = _index_list(rows, A.shape[0], "rows", what, A.device, False)
    genes = _index_list(genes, A.shape[1], "genes", what, A.device, True)
    return _gather(_ops(), A, rows, genes)


# ------------------------------------------------------------------------------------------------------------------------
# one source of counts: what the pipeline asks of the matrix, answered by a dense fp32 matrix or by a CSRCounts.
# ``restrict(rows, keep)`` is the source of the kept rows (``rows`` = nonzero(``keep``), fewer than all); row vectors go in
# and come out by kept row.
# ------------------------------------------------------------------------------------------------------------------------
class _DenseCounts:
    """a contiguous fp32 [N, P] on the device; ``fresh``: a copy of ours, which a transform may overwrite.  The kept rows
    are a copy."""

    def __init__(self, Y, fresh=False):
        self.Y, self.fresh, self.shape, self.device = Y, fresh, (int(Y.shape[0]), int(Y.shape[1])), Y.device

    def restrict(self, rows, keep):
        return _DenseCounts(self.Y[rows].contiguous(), True)

    def margins(self, o):
        return o.count_margins(self.Y)

    def deviance_sums(self, o, log_sz):
        return o.count_deviance(self.Y, log_sz)

    def moments(self, o, mode, off, scale):
        return o.column_moments(self.Y, mode, off, scale)

    def block(self, o, genes):
        """-> (the columns ``genes`` as a dense matrix, whether it is a copy of ours)"""
        if genes.numel() < self.shape[1]:
            return self.Y[:, genes].contiguous(), True
        return self.Y, self.fresh


class _SparseCounts:
    """a CSRCounts.  The kept rows are the kernels' mask over the same matrix, not a copy: a row vector is scattered to
    the original rows on its way in (a masked row's entry is not read), row outputs are indexed by ``rows``, and only
    ``block`` makes anything dense - by one gather."""

    def __init__(self, A, rows=None, keep=None):
        self.A, self.rows, self.keep, self.device = A, rows, keep, A.device
        self.shape = (A.shape[0] if rows is None else int(rows.numel()), A.shape[1])
        self.csr = (A.crow, A.col, A.values, A.shape[0], A.shape[1])

    def restrict(self, rows, keep):
        return _SparseCounts(self.A, rows, keep)

    def _by_row(self, v):
        if self.keep is None or v is None:
            return v
        return torch.zeros(self.A.shape[0], dtype=f64, device=self.device).index_copy_(0, self.rows, v)

    def margins(self, o):
        rs, cs, rn, cn, bad = o.count_margins_csr(*self.csr, self.keep)
        return (rs, cs, rn, cn, bad) if self.keep is None else (rs[self.rows], cs, rn[self.rows], cn, bad)

    def deviance_sums(self, o, log_sz):
        return o.count_deviance_csr(*self.csr, self._by_row(log_sz), self.keep)

    def moments(self, o, mode, off, scale):
        if self.keep is not None:  # the views' bounds by original row: a kept row's own index, the ends 0 and N
            off = [0] + self.rows[off[1:-1]].tolist() + [self.A.shape[0]]
        return o.column_moments_csr(*self.csr, mode, off, self._by_row(scale), self.keep)

    def block(self, o, genes):
        rows = torch.arange(self.shape[0], device=self.device) if self.rows is None else self.rows
        return _gather(o, self.A, rows, genes), True


def _counts_source(Y, what, upload=False):
    """the source behind ``Y``: a CSRCounts or a torch.sparse_csr tensor (checked here, on entry), or a dense matrix on the
    device, taken to contiguous fp32; ``upload``: a scipy.sparse matrix is uploaded, not refused"""
    A = csr_counts(Y, _what=what) if upload and _is_scipy_sparse(Y) else _sparse_arg(Y, what)
    if A is not None:
        return _SparseCounts(A)
    _matrix(Y, what)
    _on_device(what, Y=Y)
    return _DenseCounts(as_device(Y, f32))


def _prepare(o, src, ns, min_counts, max_counts, min_cells, n_top_genes, transform, theta, standardize,
             selection="deviance"):
    """``src``: a source of counts, a contiguous fp32 matrix or a CSRCounts"""
    what = "prepare_counts"
    if not isinstance(src, (_DenseCounts, _SparseCounts)):
        src = _SparseCounts(src) if isinstance(src, CSRCounts) else _DenseCounts(src)
    N, P = src.shape
    # 1. rows, on the row sums over all genes
    st = _stats(o, src)
    _refuse_invalid(st, what)
    keep = torch.ones(N, dtype=torch.bool, device=src.device)
    if min_counts is not None:
        keep &= st.row_sum >= min_counts
    if max_counts is not None:
        keep &= st.row_sum <= max_counts
    rows = torch.nonzero(keep).flatten()
    ns_kept = _view_counts(keep, ns, what)
    # 2. genes, on the margins of the kept rows
    kept = src.restrict(rows, keep) if rows.numel() < N else src
    st_r = _stats(o, kept) if kept is not src else st
    passed = None if min_cells is None else st_r.col_nnz >= min_cells
    # 3. ranking: the deviance over all genes of the kept rows (a row without counts is refused here)
    log_sz = _log_size_factors(st_r.row_sum, what)
    dev, extra = None, {}
    if selection == "seurat":  # ... or the normalised dispersion, pooled over the kept rows
        genes, dnorm = _prepare_seurat(o, kept, st_r.row_sum, passed, n_top_genes, what)
        extra = dict(dispersions_norm=dnorm)
    else:
        dev = _deviance(o, kept, st_r.col_sum, log_sz).deviance
        if n_top_genes is None and passed is None:
            genes = torch.arange(P, device=src.device)
        else:
            genes = torch.sort(_order(dev, passed, n_top_genes)).values
    if genes.numel() < 1:
        raise ValueError(f"{what}: no gene passes min_cells = {min_cells!r}" if selection == "deviance" else
                         f"{what}: no gene is selected (min_cells = {min_cells!r}, n_top_genes = {n_top_genes!r})")
    Ysel, fresh = kept.block(o, genes)
    # 4. the transform, 5. the z-score per view: on the dense block
    margins = (lambda: _stats(o, _DenseCounts(Ysel))) if genes.numel() < P else (lambda: st_r)
    outputs, log_offset, n_constant = _transform_selected(o, Ysel, fresh, margins, st_r.row_sum, log_sz, ns_kept, transform,
                                                          theta, standardize, what)
    return Prediction(outputs=outputs, log_offset=log_offset, rows=rows, genes=genes, n_samples_list=ns_kept,
                      deviance=dev, n_constant=n_constant, **extra)


# ------------------------------------------------------------------------------------------------------------------------
# the public calls
# ------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def count_stats(Y):
    """The margins of ``Y`` [N, P] in one read: a ``Prediction`` with ``row_sum`` [N] and ``col_sum`` [P] (fp64, exact
    for counts), ``row_nnz`` [N] and ``col_nnz`` [P] (int64: the entries > 0), ``total`` (float) and ``n_invalid`` (int:
    the entries that are NaN, infinite or negative - reported here, refused by every other call)."""
    src = _counts_source(Y, "count_stats")
    return _stats(_ops(), src)


@torch.no_grad()
def size_factors(Y, log=False):
    """Per-spot size factors with geometric mean 1: ``exp(log rs - mean(log rs))`` of the row sums ``rs`` (util.py:155-164),
    [N] fp64; ``log=True`` returns their logs (what ``log_offset`` takes).  A row without counts raises a ``ValueError``
    that states how many there are: remove them with ``prepare_counts(min_counts=1)``."""
    what = "size_factors"
    src = _counts_source(Y, what)
    st = _stats(_ops(), src)
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
    sparse = _is_sparse(Y)
    if not sparse:
        _matrix(Y, what)
    if log_sz is not None and (not torch.is_tensor(log_sz) or tuple(log_sz.shape) != (Y.shape[0],)
                               or not log_sz.is_floating_point()):
        raise ValueError(f"{what}: log_sz must be a floating-point tensor of shape [{Y.shape[0]}]")
    if sparse:
        if log_sz is not None:
            _on_device(what, log_sz=log_sz)
        src = _counts_source(Y, what)
        if log_sz is not None and log_sz.device != src.device:
            raise ValueError(f"{what}: the tensors are on different devices: Y on {src.device}, log_sz on {log_sz.device}")
    else:
        _on_device(what, Y=Y, log_sz=log_sz)
        src = _DenseCounts(as_device(Y, f32))
    o = _ops()
    st = _stats(o, src)
    _refuse_invalid(st, what)
    lsz = _log_size_factors(st.row_sum, what) if log_sz is None else as_device(log_sz, f64)
    return _deviance(o, src, st.col_sum, lsz)


@torch.no_grad()
def deviance_feature_selection(Y, n_top=None):
    """Genes ranked by Poisson deviance (util.py:181-197): a ``Prediction`` with ``deviance`` [P] fp64 and ``order``
    (int64 gene indices by descending deviance, equal values by the lower index; the first ``n_top`` when given).  Genes
    without counts have deviance 0 and rank last (the reference drops them)."""
    what = "deviance_feature_selection"
    if not (isinstance(Y, CSRCounts) or _is_sparse_tensor(Y)):
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
    _refuse_sparse(Y, what)
    _matrix(Y, what)
    out = _inplace_ok(Y, inplace, what)
    _on_device(what, Y=Y)
    o, Y = _ops(), as_device(Y, f32)
    st = _stats(o, _DenseCounts(Y))
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
    _refuse_sparse(Y, what)
    _matrix(Y, what)
    if target_sum is not None:
        _target(None, target_sum, what)
    out = _inplace_ok(Y, inplace, what)
    _on_device(what, Y=Y)
    o, Y = _ops(), as_device(Y, f32)
    st = _stats(o, _DenseCounts(Y))
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
    _refuse_sparse(Y, what)
    _matrix(Y, what)
    ns = _check_views(n_samples_list, int(Y.shape[0]), what)
    out = _inplace_ok(Y, inplace, what)
    _on_device(what, Y=Y)
    o, Y = _ops(), as_device(Y, f32)
    # the margins' fp64 row sums: a NaN or an infinite entry makes its row's sum non-finite, finite fp32 values cannot
    bad_rows = int((~torch.isfinite(o.count_margins(Y)[0])).sum())
    if bad_rows:
        raise ValueError(f"{what}: Y holds NaN or infinite entries (in {bad_rows} rows); their columns' moments would be NaN")
    outputs, n_constant = o.standardize_views(Y, view_offsets(ns), out=out)
    return Prediction(outputs=outputs, n_constant=n_constant)


@torch.no_grad()
def column_moments(Y, n_samples_list=None, *, transform="identity", target_sum=None):
    """Mean and variance per (view, column) in one read of ``Y`` [N, P], without a second N x P matrix: a ``Prediction``
    with ``mean`` and ``var`` [V, P] fp64, ``n_nonfinite`` (int: the transformed values that are NaN or infinite - their
    columns' moments are then NaN) and ``abs_sum`` [V, P] (the sum of the magnitudes: the scale of the mean's rounding
    error).  ``Y``: dense, a ``CSRCounts``, a ``torch.sparse_csr`` tensor or a scipy.sparse matrix (uploaded); the views
    are the consecutive row ranges ``n_samples_list`` (``None``: one view), each of at least 2 rows.  ``transform``:

    * "identity": the values as they are (any sign) - the variance filter ``Y[a:b].var(0) > 0.1`` on transformed data;
    * "expm1": ``expm1(y)`` - ``Y`` is log1p of normalised counts, scanpy's convention;
    * "normalize": ``y target_sum / row_sum_i`` - ``Y`` holds raw counts (refused otherwise); ``target_sum=None``: the
      median of the positive row sums, as in ``normalize_log1p``.  One more read for the row sums.

    The variance is scanpy's: ``(mean of squares - mean^2) n / (n - 1)``, every value and square formed in fp64 and
    summed in fp64 in a fixed order (csrc/moments.hip).  In a sparse matrix the unstored entries count as zeros."""
    what = "column_moments"
    _check_moment_transform(transform, target_sum, what)
    if not _is_sparse(Y):
        _matrix(Y, what)
    ns = _check_moment_views(n_samples_list, int(Y.shape[0]), what)
    src = _counts_source(Y, what, upload=True)
    return _moments(_ops(), src, ns, transform, target_sum, what)


@torch.no_grad()
def highly_variable_genes(Y, n_samples_list=None, *, transform="expm1", target_sum=None, n_top_genes=None,
                          min_mean=HVG_DEFAULTS["min_mean"], max_mean=HVG_DEFAULTS["max_mean"],
                          min_disp=HVG_DEFAULTS["min_disp"], max_disp=HVG_DEFAULTS["max_disp"],
                          n_bins=HVG_DEFAULTS["n_bins"], gene_mask=None, combine="intersection"):
    """Dispersion-based gene selection per view, the Seurat flavour as scanpy's ``highly_variable_genes(flavor="seurat")``
    computes it, on the moments of ``column_moments(Y, n_samples_list, transform=..., target_sum=...)`` (default: ``Y`` is
    log1p of normalised counts).  Per view: a mean of 0 is set to 1e-12; ``dispersions = log(var / mean)`` with a ratio of
    0 made NaN; ``means = log1p(mean)``; the genes fall into ``n_bins`` equal-width right-closed bins of ``means``
    (``pandas.cut``: the lowest edge 0.1 % of the range lower); ``dispersions_norm = (dispersions - bin mean) / bin
    std`` with NaN skipped, ddof = 1, and 1 for the only gene of a bin.  With ``n_top_genes`` the genes at or above the
    ``n_top_genes``-th largest ``dispersions_norm`` are selected (ties at the cutoff are all kept; a warning where fewer
    genes have a value), without it the genes with ``min_mean < means < max_mean`` and ``min_disp < dispersions_norm <
    max_disp``, NaN counting as 0.  ``gene_mask`` [P] bool: only these genes are binned, ranked and selected, as if the
    others were absent (their ``dispersions_norm`` is NaN).

    Returns a ``Prediction``: ``means``, ``dispersions``, ``dispersions_norm`` [V, P] fp64, ``highly_variable`` [V, P] bool,
    ``genes`` (int64, ascending: selected in every view for ``combine="intersection"``, in any view for "union") and
    ``n_nonfinite``.  The reduction is the HIP kernel of ``column_moments``; binning and ranking are fp64 torch on P-long
    vectors on the device.  Not pinned to scanpy itself ("Highly variable genes")."""
    what = "highly_variable_genes"
    _check_moment_transform(transform, target_sum, what)
    _check_hvg(what, n_top_genes, min_mean, max_mean, min_disp, max_disp, n_bins, combine)
    if not _is_sparse(Y):
        _matrix(Y, what)
    N, P = (int(s) for s in Y.shape)
    ns = _check_moment_views(n_samples_list, N, what)
    if gene_mask is not None:
        gene_mask = torch.as_tensor(gene_mask)
        if gene_mask.dtype != torch.bool or tuple(gene_mask.shape) != (P,):
            raise ValueError(f"{what}: gene_mask must be a bool [{P}], not {gene_mask.dtype} {tuple(gene_mask.shape)}")
    src = _counts_source(Y, what, upload=True)
    mom = _moments(_ops(), src, ns, transform, target_sum, what)
    return _hvg_from_moments(mom, gene_mask, n_top_genes, min_mean, max_mean, min_disp, max_disp, n_bins, combine, what)


def _hvg_from_moments(mom, gene_mask, n_top_genes, min_mean, max_mean, min_disp, max_disp, n_bins, combine, what):
    dev = mom.mean.device
    sel = torch.ones(mom.mean.shape[1], dtype=torch.bool, device=dev) if gene_mask is None else gene_mask.to(dev)
    if not bool(sel.any()):
        raise ValueError(f"{what}: gene_mask selects no gene")
    per_view = []
    for v in range(mom.mean.shape[0]):
        means, disp, dnorm, _ = _seurat_rank(mom.mean[v], mom.var[v], sel, n_bins)
        hv = _seurat_select(means, dnorm, sel, n_top_genes, min_mean, max_mean, min_disp, max_disp, what)
        per_view.append((means, disp, dnorm, hv))
    means, disp, dnorm, hv = (torch.stack(t) for t in zip(*per_view))
    genes = torch.nonzero(hv.all(0) if combine == "intersection" else hv.any(0)).flatten()
    return Prediction(means=means, dispersions=disp, dispersions_norm=dnorm, highly_variable=hv, genes=genes,
                      n_nonfinite=mom.n_nonfinite)


@torch.no_grad()
def prepare_counts(Y, n_samples_list, *, min_counts=None, max_counts=None, min_cells=None, n_top_genes=None,
                   transform="pearson", theta=100.0, standardize=True, selection="deviance"):
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

    ``selection="seurat"`` replaces step 3's ranking by ``highly_variable_genes``: the normalised dispersion pooled over
    all kept rows, from the raw counts (``y target / row_sum_i`` with the row sums over ALL genes of the kept rows and
    their median as the target - the sums step 4's "log1p" uses), among the genes that passed ``min_cells``;
    ``n_top_genes=None`` then selects by scanpy's default bounds.  The result carries ``dispersions_norm`` [P] fp64 (NaN for
    a gene that did not pass or has no dispersion) and ``deviance`` is None.

    Returns a ``Prediction``: ``outputs`` [N', P'] fp32, ``log_offset`` ([N'] fp32, None except for "counts"), ``rows`` and
    ``genes`` (the kept indices, int64, ascending), ``n_samples_list`` of the kept rows, ``deviance`` ([P] fp64, over the
    kept rows) and ``n_constant`` ([V] int64 or None).  ``Y`` itself is never modified, and ``outputs`` never shares its
    memory (a copy even where no row or gene is dropped)."""
    what = "prepare_counts"
    if not _is_sparse(Y):
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
    if selection not in SELECTIONS:
        raise ValueError(f"{what}: selection must be one of {SELECTIONS}, not {selection!r}")
    src = _counts_source(Y, what)  # (a torch.sparse_csr tensor is checked here)
    return _prepare(_ops(), src, ns, min_counts, max_counts, min_cells, n_top_genes, transform, theta, bool(standardize),
                    selection)
