"""Optimal-transport slice alignment on the device: the reference's third outside baseline, next to kNN regression
(neighbors.py) and exact GP regression (gpr.py).

The reference's experiments hold GPSA against PASTE (``from src.paste import PASTE, visualization`` in 29 experiment
scripts, e.g. experiments/expression/st/st_alignment_synthetic_warp.py:121-125,
simulations/two_dimensional_time_complexity.py:25-26):

    pi12       = PASTE.pairwise_align(slice1, slice2, alpha=0.1)      ->  ot_align
    new_slices = visualization.stack_slices_pairwise(slices, [pi12])  ->  stack_slices        (both: paste_baseline)

The problem is PASTE's: couplings T of two slices with marginals a, b that minimise the fused Gromov-Wasserstein objective

    (1 - alpha) <M, T> + alpha sum_ijkl (C1_ik - C2_jl)^2 T_ij T_kl

with C1, C2 the Euclidean (not squared) distances inside each slice and M the expression cost between spots: with "kl",
0.01 is added to both expression matrices, every row is divided by its sum (P, Q) and
M_ij = sum_p P_ip log P_ip - sum_p P_ip log Q_jp; with "euclidean", the SQUARED Euclidean distance of expression rows.

THE SOLVER IS NOT PASTE'S.  PASTE runs conditional gradient with an exact network-simplex transport solve per step, which
has no sensible GPU form.  This is the entropic projected-gradient solver of Peyre, Cuturi and Solomon (2016), the algorithm
behind POT's ``entropic_fused_gromov_wasserstein``: starting from T_0 = a b^T (or ``T_init``), ``max_iter`` times

    cost_t  = (1 - alpha) M + 2 alpha (cA 1^T + 1 cB^T - 2 C1 T_t C2),     cA = (C1 o C1) a,  cB = (C2 o C2) b
    T_{t+1} = argmin <cost_t, T> + e KL(T || a x b)       by ``sinkhorn_iters`` log-domain Sinkhorn sweeps, the potentials
                                                          warm-started from the step before

with e = epsilon * mean |cost_0| (``relative_epsilon``, the default: costs scale with the coordinates' units to the fourth
power) or e = epsilon.  The returned coupling is a SMOOTHED one; it sharpens as ``epsilon`` falls, and the Sinkhorn sweeps
then take longer to converge - ``marginal_error`` and ``plan_change`` report how far they got.  Nothing here is pinned to
the ``paste`` or ``POT`` packages (neither is a dependency, neither was available to test against): the tests hold the
kernels to a numpy fp64 restatement of the algorithm above, and that restatement to exact transport results.

Everything is fp64 on tensors already on the device, under ``torch.no_grad()``.  The iteration counts are fixed by default:
the result is the same bits on every call and nothing is read back inside the loop.  ``tol`` ends the loop when
|T_{t+1} - T_t|_1 < tol, checked every ``sync_every`` outer steps with one host read (the pattern of ``fit``).
Memory: C1, C2, M, T, the cost and one n x m intermediate, 8 (n^2 + m^2 + 4 n m) bytes.
"""
from dataclasses import dataclass

import torch

from ._args import as_device, describe, on_device, ops as _ops

f64 = torch.float64
MAX_D = 4  # csrc/common.hpp: MAXD
DISSIMILARITIES = ("kl", "euclidean")
MARGINAL_SUM_TOL = 1e-9


@dataclass
class OTAlignment:
    """What ``ot_align`` returns.  ``objective`` = (1 - alpha) ``expression_cost`` + alpha ``gw_cost``, all three evaluated at
    the returned ``T`` with T's own marginals; ``marginal_error`` = |T 1 - a|_1 + |T^T 1 - b|_1 (the Sinkhorn sweeps of the
    last outer step did not converge when this is not small); ``plan_change`` the last |T_{t+1} - T_t|_1; ``n_iter`` the
    outer steps run; ``epsilon_used`` the regulariser e; ``f`` [n], ``g`` [m] the potentials."""
    T: torch.Tensor
    objective: float
    expression_cost: float
    gw_cost: float
    marginal_error: float
    plan_change: float
    n_iter: int
    epsilon_used: float
    f: torch.Tensor
    g: torch.Tensor


def _matrix(t, name, what):
    if not torch.is_tensor(t) or t.dim() != 2 or not t.is_floating_point() or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: {name} has shape {describe(t)}; a floating-point [n >= 1, >= 1] tensor is needed")
    return t


def _count(v, name, what, low):
    if isinstance(v, bool) or int(v) != v or v < low:
        raise ValueError(f"{what}: {name} must be an integer >= {low}, not {v!r}")
    return int(v)


def _marginal(w, name, what, n):
    """a strictly positive fp64 [n] that sums to 1 (one host read)"""
    if not torch.is_tensor(w) or w.dim() != 1 or w.shape[0] != n or not w.is_floating_point():
        raise ValueError(f"{what}: marginal {name} has shape {describe(w)}; a floating-point [{n}] is needed")
    w = as_device(w, f64)
    bad = int((~(w > 0)).sum())
    if bad:
        raise ValueError(f"{what}: marginal {name} must be strictly positive; {bad} of its {n} entries are not")
    total = float(w.sum())
    if abs(total - 1.0) > MARGINAL_SUM_TOL:
        raise ValueError(f"{what}: marginal {name} must sum to 1 (within {MARGINAL_SUM_TOL}); it sums to {total!r}")
    return w


def _check_args(what, XA, YA, XB, YB, alpha, dissimilarity, epsilon, a, b, T_init, max_iter, sinkhorn_iters, tol,
                sync_every):
    """every rule that needs no launch; -> (n, m, D, P)"""
    for t, name in ((XA, "XA"), (YA, "YA"), (XB, "XB"), (YB, "YB")):
        _matrix(t, name, what)
    n, m = int(XA.shape[0]), int(XB.shape[0])
    D, P = int(XA.shape[1]), int(YA.shape[1])
    if D > MAX_D or XB.shape[1] != D:
        raise ValueError(f"{what}: XA has D = {D} and XB has D = {XB.shape[1]} coordinates; one D of at most {MAX_D} is needed")
    if YA.shape[0] != n or YB.shape[0] != m:
        raise ValueError(f"{what}: YA has {YA.shape[0]} rows for {n} spots and YB has {YB.shape[0]} rows for {m} spots")
    if YB.shape[1] != P:
        raise ValueError(f"{what}: the slices must share their genes; YA has {P} columns and YB has {YB.shape[1]}")
    if dissimilarity not in DISSIMILARITIES:
        raise ValueError(f"{what}: dissimilarity must be one of {DISSIMILARITIES}, not {dissimilarity!r}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"{what}: alpha = {alpha!r} is outside [0, 1]")
    if not 0.0 < float(epsilon) < float("inf"):
        raise ValueError(f"{what}: epsilon = {epsilon!r} must be positive and finite")
    _count(max_iter, "max_iter", what, 1)
    _count(sinkhorn_iters, "sinkhorn_iters", what, 1)
    _count(sync_every, "sync_every", what, 1)
    if tol is not None and not float(tol) >= 0.0:
        raise ValueError(f"{what}: tol = {tol!r} must be None or >= 0")
    if T_init is not None and (not torch.is_tensor(T_init) or tuple(T_init.shape) != (n, m) or not T_init.is_floating_point()):
        raise ValueError(f"{what}: T_init has shape {describe(T_init)}; a floating-point [{n}, {m}] is needed")
    on_device(what, "optimal-transport", XA=XA, YA=YA, XB=XB, YB=YB, a=a if torch.is_tensor(a) else None,
              b=b if torch.is_tensor(b) else None, T_init=T_init)
    return n, m, D, P


def spatial_cost(X, norm=False):
    """C [n, n] = |x_i - x_k| (fp64, symmetric to the bit, zero diagonal); ``norm``: divided by its smallest positive entry"""
    C = _ops().ot_dist(as_device(X, f64))
    if norm:
        pos = C[C > 0]
        if pos.numel():
            C = C / pos.min()
    return C


def expression_cost(YA, YB, dissimilarity="kl"):
    """M [n, m] fp64 between the rows of YA [n, P] and YB [m, P] (read as fp32) as PASTE poses it (the head of the module);
    a ``ValueError`` names the count of entries "kl" cannot take (negative, NaN or infinite; "euclidean": NaN or infinite)"""
    what = "expression_cost"
    o = _ops()
    Pa, La, ta, bad_a = o.ot_expr_rows(as_device(YA, torch.float32), dissimilarity)
    Pb, Lb, tb, bad_b = o.ot_expr_rows(as_device(YB, torch.float32), dissimilarity)
    na, nb = (int(v) for v in torch.cat([bad_a, bad_b]).tolist())
    if na or nb:
        rule = "non-negative and finite" if dissimilarity == "kl" else "finite"
        raise ValueError(f"{what}: dissimilarity {dissimilarity!r} needs {rule} expression; {na} entries of YA and {nb} of YB "
                         "are not")
    M = o.gemm(Pa, Lb, transB=True)
    o.ot_expr_cost(M, ta, tb, dissimilarity)
    return M


@torch.no_grad()
def ot_align(XA, YA, XB, YB, alpha=0.1, dissimilarity="kl", epsilon=0.01, relative_epsilon=True, a=None, b=None,
             T_init=None, norm=False, max_iter=40, sinkhorn_iters=50, tol=None, sync_every=10):
    """Entropic fused Gromov-Wasserstein alignment of slice A (coordinates XA [n, D <= 4], expression YA [n, P]) and slice B
    (XB [m, D], YB [m, P]) -> ``OTAlignment``.  The problem is ``PASTE.pairwise_align``'s; the solver is not (the head of
    the module): the coupling is a smoothed one that sharpens as ``epsilon`` falls.

    ``a`` [n], ``b`` [m]: the marginals (uniform by default; strictly positive, summing to 1).  ``norm``: each distance matrix
    divided by its smallest positive entry.  With ``tol=None`` exactly ``max_iter`` outer steps of ``sinkhorn_iters`` sweeps
    run and nothing is read back before the end."""
    what = "ot_align"
    n, m, D, P = _check_args(what, XA, YA, XB, YB, alpha, dissimilarity, epsilon, a, b, T_init, max_iter, sinkhorn_iters,
                             tol, sync_every)
    alpha, epsilon = float(alpha), float(epsilon)
    dev = XA.device
    a = torch.full((n,), 1.0 / n, dtype=f64, device=dev) if a is None else _marginal(a, "a", what, n)
    b = torch.full((m,), 1.0 / m, dtype=f64, device=dev) if b is None else _marginal(b, "b", what, m)
    o = _ops()
    M = expression_cost(YA, YB, dissimilarity)  # (refuses what "kl" cannot take before anything of the solve runs)
    C1, C2 = spatial_cost(XA, norm), spatial_cost(XB, norm)
    cA, cB = o.ot_sqmatvec(C1, a), o.ot_sqmatvec(C2, b)
    loga, logb = a.log(), b.log()
    T = torch.outer(a, b) if T_init is None else as_device(T_init, f64).clone()
    f, g = torch.zeros(n, dtype=f64, device=dev), torch.zeros(m, dtype=f64, device=dev)
    tmp, G = torch.empty(n, m, dtype=f64, device=dev), torch.empty(n, m, dtype=f64, device=dev)
    sums = torch.empty(3, dtype=f64, device=dev)
    eps = torch.full((1,), epsilon, dtype=f64, device=dev)
    n_iter, rowsum, colsum, psums = 0, None, None, None
    for t in range(int(max_iter)):
        o.gemm(C1, T, out=tmp)
        o.gemm(tmp, C2, out=G)  # G = C1 T C2
        o.ot_cost(G, M, T, cA, cB, cA, cB, alpha, sums)
        if t == 0 and relative_epsilon:
            mean = sums[0:1] / float(n * m)
            eps = torch.where(mean > 0, epsilon * mean, eps)  # (a cost of all zeros: epsilon itself)
        o.ot_sinkhorn(G, loga, logb, eps, f, g, int(sinkhorn_iters))
        T, rowsum, colsum, psums = o.ot_plan(G, f, g, a, b, eps, T)
        n_iter = t + 1
        if tol is not None and n_iter % int(sync_every) == 0 and float(psums[2]) < float(tol):
            break
    # the objective at the returned T, with T's own marginals
    o.gemm(C1, T, out=tmp)
    o.gemm(tmp, C2, out=G)
    o.ot_cost(G, M, T, cA, cB, o.ot_sqmatvec(C1, rowsum), o.ot_sqmatvec(C2, colsum), alpha, sums)
    _, expr, gw, rerr, cerr, chg, e = torch.cat([sums, psums, eps]).tolist()
    return OTAlignment(T=T, objective=(1.0 - alpha) * expr + alpha * gw, expression_cost=expr, gw_cost=gw,
                       marginal_error=rerr + cerr, plan_change=chg, n_iter=n_iter, epsilon_used=e, f=f, g=g)


def _matmul(A, B, transA=False):
    if A.device.type == "cuda":
        return _ops().gemm(A, B, transA=transA)
    return (A.T if transA else A) @ B


@torch.no_grad()
def stack_slices(X_list, T_list, reflection=True):
    """PASTE's ``visualization.stack_slices_pairwise``: the chain of slices X_list[k] [n_k, D] put on top of each other by
    the couplings T_list[k] [n_k, n_{k+1}] through generalised Procrustes steps.  For each consecutive pair, X the
    previous slice's NEW coordinates and Y the next slice's own:

        X <- X - (T 1)^T X,   Y <- Y - (T^T 1)^T Y,   H = Y^T T^T X = U S V^T,   R = V U^T,   Y <- Y R^T

    (the recentred X is kept for the first pair only, as PASTE does).  ``reflection=True`` is PASTE's behaviour: no
    determinant guard, R may be a reflection.  ``reflection=False`` flips the last right singular vector when det R < 0.
    -> (aligned coordinates, rotations R_k [D, D], translations t_k [D]) with aligned_k = (X_k - t_k) R_k^T (fp64; the
    D x D SVD runs on the host)."""
    what = "stack_slices"
    if len(X_list) < 1 or len(T_list) != len(X_list) - 1:
        raise ValueError(f"{what}: {len(X_list)} slices need {max(len(X_list) - 1, 0)} couplings, not {len(T_list)}")
    Xs = [as_device(_matrix(X, f"X_list[{k}]", what), f64) for k, X in enumerate(X_list)]
    D = Xs[0].shape[1]
    eye = torch.eye(D, dtype=f64, device=Xs[0].device)
    out, rots, trans = [Xs[0]], [eye], [torch.zeros(D, dtype=f64, device=Xs[0].device)]
    for k, T in enumerate(T_list):
        X, Y = out[k], Xs[k + 1]
        if not torch.is_tensor(T) or tuple(T.shape) != (X.shape[0], Y.shape[0]) or Y.shape[1] != D:
            raise ValueError(f"{what}: T_list[{k}] has shape {describe(T)}; [{X.shape[0]}, {Y.shape[0]}] is needed, and "
                             f"D = {D} coordinates in every slice")
        T = as_device(T, f64)
        tx, ty = T.sum(1) @ X, T.sum(0) @ Y
        Xc, Yc = X - tx, Y - ty
        H = _matmul(Yc, _matmul(T, Xc, transA=True), transA=True)  # Y^T (T^T X)  [D, D]
        U, _, Vt = torch.linalg.svd(H.cpu())
        R = Vt.T @ U.T
        if not reflection and float(torch.linalg.det(R)) < 0:
            Vt = Vt.clone()
            Vt[-1] *= -1.0
            R = Vt.T @ U.T
        R = R.to(Y.device)
        if k == 0:
            out[0], trans[0] = Xc, tx
        out.append(Yc @ R.T)
        rots.append(R)
        trans.append(ty)
    return out, rots, trans


@torch.no_grad()
def paste_baseline(X, Y, n_samples_list, reflection=True, **ot_kwargs):
    """What the reference's scripts do with PASTE, in the ``data_dict`` row layout: X [N, D], Y [N, P] hold the views one
    after the other (``n_samples_list``); consecutive views are coupled by ``ot_align(**ot_kwargs)`` and stacked by
    ``stack_slices``.  -> coordinates [N, D] fp64 in the same row order, ready for ``alignment_score(..., G=coords)`` or the
    error against a simulation's truth, next to GPSA's aligned coordinates."""
    what = "paste_baseline"
    _matrix(X, "X", what), _matrix(Y, "Y", what)
    ns = [int(v) for v in n_samples_list]
    if len(ns) < 2 or any(v < 1 for v in ns) or sum(ns) != X.shape[0] or Y.shape[0] != X.shape[0]:
        raise ValueError(f"{what}: n_samples_list {ns} does not partition the {X.shape[0]} rows of X and {Y.shape[0]} of Y "
                         "into at least two views")
    off = [0]
    for v in ns:
        off.append(off[-1] + v)
    Xv = [X[off[k]:off[k + 1]] for k in range(len(ns))]
    Yv = [Y[off[k]:off[k + 1]] for k in range(len(ns))]
    Ts = [ot_align(Xv[k], Yv[k], Xv[k + 1], Yv[k + 1], **ot_kwargs).T for k in range(len(ns) - 1)]
    return torch.cat(stack_slices(Xv, Ts, reflection=reflection)[0])
