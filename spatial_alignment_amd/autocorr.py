"""Spatial autocorrelation on the device: the weight graph, Moran's I and Geary's C with permutation tests, BH-adjusted p.

What the reference's experiments compute with ``sq.gr.spatial_neighbors`` followed by ``sq.gr.spatial_autocorr``
(experiments/expression/visium/moransi_post_alignment.py:88-133, visium_morans_i.py, visium_prediction.py:91-97,
slideseq/slideseq_alignment.py:146, st/st_alignment_synthetic_warp*.py) and then threshold on ``pval_norm_fdr_bh``:

* ``spatial_graph``: the kNN graph of the spots in CSR - directed as ``moran_i`` uses it, or symmetrised by union or by
  mutual neighbours - with its sums S0, S1, S2;  ``SpatialGraph.from_csr`` takes a caller's own weights;
* ``spatial_autocorr``: the statistic per gene, its analytic moments under the normality assumption, ``n_perms``
  permuted statistics and the p-values and FDR columns derived from them;
* ``fdr_bh``: Benjamini-Hochberg adjusted p-values.

The per-row merge that builds the graph, the check of a caller's graph, the graph sums and the permuted statistic are
HIP (csrc/autocorr.hip); the neighbours are ``knn``'s (exact, ties to the lower index); sorting, the random permutations
and the closed-form columns are torch on the device.  The formulas are the textbook (Cliff and Ord) ones that esda and
squidpy implement; squidpy is not a dependency and nothing here is pinned to its output.  Everything runs under
``torch.no_grad()`` and touches no model state.  Tensors on the CPU are refused with a ``ValueError`` that names the
device: there is no host path.
"""
import math

import torch

from . import neighbors as _nb
from ._args import as_device, coords, describe, on_device, ops as _ops, values
from .predict import Prediction

f64, f32, i32, i64 = torch.float64, torch.float32, torch.int32, torch.int64
SYMMETRIC = ("none", "union", "mutual")
MODES = ("moran", "geary")
_RULES = ("crow is not 0 = crow[0] <= ... <= crow[n] = nnz", "col outside [0, n)", "col not ascending within a row",
          "self edge", "w not finite or < 0")


class SpatialGraph:
    """A spatial weight graph in CSR on the device: ``crow`` [n + 1] int64, ``col`` [nnz] int32 (ascending within a row, no
    self edge, no duplicate), ``w`` [nnz] fp64, ``n``; ``n_isolated`` (rows without an edge, a 0-dim int64 tensor) and the
    sums ``S0 = sum w``, ``S1 = 1/2 sum_ij (w_ij + w_ji)^2``, ``S2 = sum_i (w_i. + w_.i)^2`` (0-dim fp64 tensors, fixed-order
    sums), all on the device.  Made by ``spatial_graph`` or ``SpatialGraph.from_csr``."""

    def __init__(self, crow, col, w, n):
        self.crow, self.col, self.w, self.n = crow, col, w, int(n)
        # the transposed structure, for the column sums of S2: the entries' positions sorted by column (stable)
        scol, tperm = torch.sort(col, stable=True)
        tptr = torch.searchsorted(scol, torch.arange(self.n + 1, dtype=i32, device=col.device)).to(i64)
        self.sums = _ops().graph_sums(crow, col, w, self.n, tptr.contiguous(), tperm.contiguous())
        self.n_isolated = (crow[1:] == crow[:-1]).sum()

    S0 = property(lambda self: self.sums[0])
    S1 = property(lambda self: self.sums[1])
    S2 = property(lambda self: self.sums[2])
    nnz = property(lambda self: int(self.col.numel()))
    device = property(lambda self: self.crow.device)

    def __repr__(self):
        return f"SpatialGraph(n={self.n}, nnz={self.nnz}, device={str(self.device)!r})"

    @classmethod
    @torch.no_grad()
    def from_csr(cls, crow, col, w, n):
        """A caller's graph.  It is checked on the device - ``crow`` monotone from 0 to nnz, ``col`` in [0, n) and
        ascending within a row, no self edge, ``w`` finite and >= 0 - and a ``ValueError`` names every violated rule with
        its count."""
        what = "SpatialGraph.from_csr"
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"{what}: n must be a positive integer, not {n!r}")
        for name, t, ok in (("crow", crow, lambda t: not t.is_floating_point() and tuple(t.shape) == (n + 1,)),
                            ("col", col, lambda t: not t.is_floating_point() and t.dim() == 1),
                            ("w", w, lambda t: t.is_floating_point() and t.dim() == 1)):
            if not torch.is_tensor(t) or t.dtype == torch.bool or not ok(t):
                raise ValueError(f"{what}: {name} is {describe(t)}; crow integer [{n + 1}], col integer [nnz] and w "
                                 "floating-point [nnz] are needed")
        if col.shape != w.shape:
            raise ValueError(f"{what}: col has {col.numel()} entries and w {w.numel()}")
        on_device(what, "neighbour", crow=crow, col=col, w=w)
        crow, col, w = as_device(crow, i64), as_device(col, i32), as_device(w, f64)
        bad = _ops().graph_check(crow, col, w, n).tolist()
        if any(bad):
            raise ValueError(f"{what}: the graph is malformed: "
                             + "; ".join(f"{rule}: {cnt}" for rule, cnt in zip(_RULES, bad) if cnt))
        return cls(crow, col, w, n)


@torch.no_grad()
def spatial_graph(X, k=6, symmetric="none", row_standardize=True, rows_per_chunk=None):
    """The k-nearest-neighbour graph of the points ``X`` [n, D] as a ``SpatialGraph``.

    The neighbour lists are ``knn``'s own (exact, the point itself left out, ties to the lower index).  ``symmetric``:
    "none" - i -> j where j is among i's ``k`` nearest, ``moran_i``'s directed graph; "union" - an edge where either
    direction is a kNN edge; "mutual" - only where both are (a row may then be empty: it keeps weight sum 0 and is counted
    in ``n_isolated``).  Weights are 1, or 1 / (the row's degree) with ``row_standardize``.  Columns ascend within a
    row.  The in-neighbour lists come from a stable sort of the flattened lists; the per-row merge of the two sorted
    lists is HIP (count, scan, write), without atomics and without anything of n x n."""
    what = "spatial_graph"
    coords(X, "X", what, _nb.MAX_D)
    n = int(X.shape[0])
    _nb._check_k(k, n - 1, what, True)
    if symmetric not in SYMMETRIC:
        raise ValueError(f"{what}: symmetric must be 'none', 'union' or 'mutual', not {symmetric!r}")
    c = _nb._chunk(rows_per_chunk, n, what)
    on_device(what, "neighbour", X=X)
    R = as_device(X, f64)
    idx = torch.empty(n, k, dtype=i32, device=R.device)
    for a, ia, _ in _nb._knn_chunks(R, R, k, True, c):
        idx[a: a + c] = ia
    out_sorted = torch.sort(idx, dim=1).values.contiguous()
    in_ptr = in_src = None
    if symmetric != "none":
        tgt, order = torch.sort(out_sorted.reshape(-1), stable=True)  # by target; the sources ascend within a target
        in_src = torch.div(order, k, rounding_mode="floor").to(i32).contiguous()
        in_ptr = torch.searchsorted(tgt, torch.arange(n + 1, dtype=i32, device=R.device)).to(i64).contiguous()
    crow, col, w = _ops().graph_merge(out_sorted, in_ptr, in_src, symmetric, row_standardize)
    return SpatialGraph(crow, col, w, n)


@torch.no_grad()
def fdr_bh(p):
    """Benjamini-Hochberg adjusted p-values of ``p`` [m] over its finite entries (a NaN stays NaN and does not count):
    a sort, ``p_(i) m / i``, a reversed cumulative minimum, a clip at 1
    (``scipy.stats.false_discovery_control(p, method="bh")`` on complete input).  fp64, on ``p``'s device."""
    if not torch.is_tensor(p) or p.dim() != 1 or not p.is_floating_point():
        raise ValueError(f"fdr_bh: p must be a floating-point [m], not {describe(p)}")
    p = p.detach().to(f64)
    finite = torch.isfinite(p)
    m = finite.sum()
    q, order = torch.sort(torch.where(finite, p, torch.full_like(p, float("inf"))))
    rank = torch.arange(1, p.numel() + 1, dtype=f64, device=p.device)
    adj = torch.cummin((q * m / rank).flip(0), 0).values.flip(0).clamp(max=1.0)
    out = torch.empty_like(p)
    out[order] = adj
    return torch.where(finite, out, torch.full_like(p, float("nan")))


def _folded_tail(z, two_tailed):
    """sf(z) where z > 0, else cdf(z): 1/2 erfc(|z| / sqrt 2); doubled when two_tailed"""
    p = 0.5 * torch.erfc(z.abs() / math.sqrt(2.0))
    return 2.0 * p if two_tailed else p


def _check_perms(perms, n, what):
    if not torch.is_tensor(perms) or perms.dim() != 2 or perms.is_floating_point() or perms.dtype == torch.bool \
            or perms.shape[0] < 1 or perms.shape[1] != n:
        raise ValueError(f"{what}: perms is {describe(perms)}; an integer [R >= 1, {n}] is needed, every row a permutation "
                         f"of 0..{n - 1}")


@torch.no_grad()
def spatial_autocorr(X_or_graph, Y, mode="moran", n_perms=100, two_tailed=False, perms=None, generator=None,
                     perms_per_chunk=None, k=6, symmetric="none", row_standardize=True, rows_per_chunk=None):
    """Moran's I (``mode="moran"``) or Geary's C (``"geary"``) of every column of ``Y`` [n, P] on a spatial graph, with
    the analytic and the permutation p-values and their Benjamini-Hochberg columns - ``sq.gr.spatial_autocorr``'s table.

    ``X_or_graph``: a ``SpatialGraph``, or points [n, D] from which ``spatial_graph(X, k, symmetric, row_standardize,
    rows_per_chunk)`` is built.  ``Y`` is taken to fp32, widened and centred per column in fp64 (as ``moran_i`` does); a
    NaN in it is refused.  Returns a ``Prediction``, fp64 [P] unless noted:

    * ``I`` or ``C``: ``(n / S0) num / sum z^2`` with ``num = sum_i z_i sum_j w_ij z_j``, or ``(n - 1) num / (2 S0 sum z^2)``
      with ``num = sum_ij w_ij (z_i - z_j)^2``; NaN for a constant column;
    * ``expected``: ``-1 / (n - 1)``, or 1;
    * ``var_norm`` under the normality assumption: ``(n^2 S1 - n S2 + 3 S0^2) / ((n^2 - 1) S0^2) - expected^2``, or
      ``((2 S1 + S2)(n - 1) - 4 S0^2) / (2 (n + 1) S0^2)``;
    * ``pval_norm``: from ``z = (stat - expected) / sqrt(var_norm)`` the folded one-sided tail, ``sf(z)`` where z > 0 and
      ``cdf(z)`` otherwise (doubled with ``two_tailed``).  This is NOT ``moran_i``'s ``p_norm``, which is the upper tail
      ``sf(z)`` for every z: the two differ wherever z < 0;
    * ``sims`` [n_perms, P]: the statistic with the rows of ``Y`` permuted, ``n_perms`` times;
    * ``pval_sim``: with ``larger = #{r: sims_r >= stat}``, folded to ``n_perms - larger`` where that is smaller,
      ``(larger + 1) / (n_perms + 1)``;
    * ``var_sim`` (the population variance of ``sims``) and ``pval_z_sim`` (as ``pval_norm``, from ``z_sim = (stat - mean
      sims) / std sims``);
    * ``pval_norm_fdr_bh``, ``pval_sim_fdr_bh``, ``pval_z_sim_fdr_bh``: ``fdr_bh`` of the column over its finite entries;
    * ``n_isolated``, ``S0``, ``S1``, ``S2``: the graph's (0-dim tensors on the device).

    With ``n_perms=0`` (and no ``perms``) the simulation fields are None.  The permutations are
    ``torch.argsort(torch.rand(n_perms, n, generator=generator))`` on the device (the same generator state gives the same
    result bit for bit), or the caller's ``perms`` [R, n] (then ``n_perms = R``), checked to be permutations.  The
    observed statistic is not a separate code path: it is the same kernel on the identity, so a permutation that happens
    to be the identity ties with it exactly.  ``perms_per_chunk``: permutations per launch (default: all; it bounds
    the workspace, 8 * 32 * chunk * P bytes at most, and does not change a bit of the result).  The permuted matrix is
    never formed.  No gradients."""
    what = "spatial_autocorr"
    if mode not in MODES:
        raise ValueError(f"{what}: mode must be 'moran' or 'geary', not {mode!r}")
    graph = X_or_graph if isinstance(X_or_graph, SpatialGraph) else None
    if graph is None:
        coords(X_or_graph, "X", what, _nb.MAX_D)
        n = int(X_or_graph.shape[0])
        _nb._check_k(k, n - 1, what, True)
        if symmetric not in SYMMETRIC:
            raise ValueError(f"{what}: symmetric must be 'none', 'union' or 'mutual', not {symmetric!r}")
    else:
        n = graph.n
    if n < 3:
        raise ValueError(f"{what}: {n} points; the moments need at least 3")
    values(Y, "Y", what, n)
    if isinstance(n_perms, bool) or not isinstance(n_perms, int) or n_perms < 0:
        raise ValueError(f"{what}: n_perms must be a non-negative integer, not {n_perms!r}")
    if perms is not None:
        _check_perms(perms, n, what)
        n_perms = int(perms.shape[0])
    if perms_per_chunk is not None and (isinstance(perms_per_chunk, bool) or not isinstance(perms_per_chunk, int)
                                        or perms_per_chunk < 1):
        raise ValueError(f"{what}: perms_per_chunk must be a positive integer, not {perms_per_chunk!r}")
    if bool(torch.isnan(Y).any()):
        raise ValueError(f"{what}: Y has NaN entries; the statistic is defined on complete columns (drop or fill them first)")
    on_device(what, "neighbour", X=None if graph is not None else X_or_graph,
              graph=graph.crow if graph is not None else None, Y=Y, perms=perms)
    if graph is None:
        graph = spatial_graph(X_or_graph, k=k, symmetric=symmetric, row_standardize=row_standardize,
                              rows_per_chunk=rows_per_chunk)
    dev = Y.device
    if perms is not None:
        ref = torch.arange(n, device=dev, dtype=perms.dtype)
        if not bool((torch.sort(perms, dim=1).values == ref).all()):
            raise ValueError(f"{what}: perms holds a row that is not a permutation of 0..{n - 1}")
        perms = perms.detach().to(i32).contiguous()
    elif n_perms:
        perms = torch.argsort(torch.rand(n_perms, n, generator=generator, device=dev), dim=1).to(i32)

    # Z: the fp32 values widened and centred per column in fp64.  torch's reductions along dim 0 allocate several times the
    # matrix, so the column sums are the count kernels' (fp64, fixed order) and sum z^2 is the Moran numerator of the
    # identity graph under the identity permutation - the same kernel, nothing of [n, P] beside Z
    o = _ops()
    y = Y.detach().to(f32).contiguous()
    P = int(y.shape[1])
    mean = o.column_moments(y, "identity", [0, n])[0][0] / n
    Z = y.to(f64)
    del y
    Z.sub_(mean)
    ident = torch.arange(n, dtype=i32, device=dev).view(1, n)
    den, _ = o.autocorr_perm(Z, torch.arange(n + 1, dtype=i64, device=dev), ident.view(n),
                             torch.ones(n, dtype=f64, device=dev), ident, "moran")
    den = den[0]
    # (a constant fp32 column sums exactly in fp64, so its mean is the value itself, its z are 0 and so is sum z^2)
    const = den <= 0

    S0, S1, S2 = graph.S0, graph.S1, graph.S2
    stat_all = torch.empty(n_perms + 1, P, dtype=f64, device=dev)
    _, n_bad = o.autocorr_perm(Z, graph.crow, graph.col, graph.w, ident, mode, out=stat_all[:1])
    c = n_perms if perms_per_chunk is None else perms_per_chunk
    for a in range(0, n_perms, max(c, 1)):
        _, nb = o.autocorr_perm(Z, graph.crow, graph.col, graph.w, perms[a: a + c], mode, out=stat_all[1 + a: 1 + a + c])
        n_bad = n_bad + nb
    if int(n_bad):
        raise ValueError(f"{what}: {int(n_bad)} entries of the graph's columns or of the permutations lie outside "
                         f"[0, {n}); they were not followed")
    del Z
    # the numerators become the statistic in place, the observed row and every permuted row by the same operations
    scale = n / S0 if mode == "moran" else (n - 1) / (2.0 * S0)
    stat_all.div_(den).mul_(scale).masked_fill_(const.view(1, P), float("nan"))
    stat, sims = stat_all[0], stat_all[1:]

    if mode == "moran":
        E = -1.0 / (n - 1)
        var = (n * n * S1 - n * S2 + 3.0 * S0 * S0) / ((n * n - 1.0) * S0 * S0) - E * E
    else:
        E = 1.0
        var = ((2.0 * S1 + S2) * (n - 1) - 4.0 * S0 * S0) / (2.0 * (n + 1) * S0 * S0)
    pval_norm = _folded_tail((stat - E) / var.sqrt(), two_tailed)
    res = Prediction(expected=torch.full_like(den, E), var_norm=var.expand(P).clone(), pval_norm=pval_norm,
                     pval_norm_fdr_bh=fdr_bh(pval_norm), sims=None, pval_sim=None, var_sim=None, pval_z_sim=None,
                     pval_sim_fdr_bh=None, pval_z_sim_fdr_bh=None, n_isolated=graph.n_isolated, S0=S0, S1=S1, S2=S2)
    res["I" if mode == "moran" else "C"] = stat.clone() if n_perms else stat
    if n_perms:
        nan = torch.full_like(den, float("nan"))
        larger = (sims >= stat).sum(0)
        larger = torch.where(n_perms - larger < larger, n_perms - larger, larger)
        pval_sim = torch.where(torch.isnan(stat), nan, (larger + 1).to(f64) / (n_perms + 1))
        pval_z_sim = _folded_tail((stat - sims.mean(0)) / sims.std(0, unbiased=False), two_tailed)
        res.update(sims=sims, pval_sim=pval_sim, var_sim=sims.var(0, unbiased=False), pval_z_sim=pval_z_sim,
                   pval_sim_fdr_bh=fdr_bh(pval_sim), pval_z_sim_fdr_bh=fdr_bh(pval_z_sim))
    return res
