"""numpy fp64 yardstick for the optimal-transport alignment (spatial_alignment_amd/ot.py, csrc/ot.hip): the algorithm of the
module's head restated with its own log-sum-exp, no torch, no scipy.  tests/test_ot.py ties it to exact results (the
assignment optimum of a pure expression cost, a planted permutation); tests/test_ot_gpu.py holds the kernels to it."""
import numpy as np

SHIFT = 0.01


def lse(V, axis):
    """log sum exp along ``axis`` with the maximum subtracted"""
    top = np.max(V, axis=axis, keepdims=True)
    return np.squeeze(top, axis) + np.log(np.sum(np.exp(V - top), axis=axis))


def dist(X, norm=False):
    """|x_i - x_k|, difference form, summed over the coordinates in order"""
    X = np.asarray(X, np.float64)
    s = np.zeros((X.shape[0], X.shape[0]))
    for d in range(X.shape[1]):
        t = X[:, None, d] - X[None, :, d]
        s = s + t * t
    C = np.sqrt(s)
    if norm and np.any(C > 0):
        C = C / C[C > 0].min()
    return C


def expr_rows(Y, mode="kl"):
    """-> (Pm, Lg, term, n_invalid) of the rows of Y as stored in fp32"""
    Y = np.asarray(Y, np.float32).astype(np.float64)
    if mode == "kl":
        bad = int(np.sum(~(np.isfinite(Y) & (Y >= 0))))
        with np.errstate(invalid="ignore", divide="ignore"):  # (a row with an entry "kl" cannot take: NaN, and counted)
            Pm = (Y + SHIFT) / np.sum(Y + SHIFT, axis=1, keepdims=True)
            Lg = np.log(Pm)
            return Pm, Lg, np.sum(Pm * Lg, axis=1), bad
    return Y, Y, np.sum(Y * Y, axis=1), int(np.sum(~np.isfinite(Y)))


def expr_cost(YA, YB, mode="kl"):
    Pa, _, ta, _ = expr_rows(YA, mode)
    Pb, Lb, tb, _ = expr_rows(YB, mode)
    if mode == "kl":
        return ta[:, None] - Pa @ Lb.T
    return np.maximum(0.0, (ta[:, None] + tb[None, :]) - 2.0 * (Pa @ Pb.T))


def sqmatvec(C, v):
    return (C * C) @ v


def cost_pass(G, M, T, cA, cB, cAt, cBt, alpha):
    """-> (cost, [sum |cost|, <M, T>, <cAt 1^T + 1 cBt^T - 2 G, T>])"""
    cost = (1.0 - alpha) * M + 2.0 * alpha * ((cA[:, None] + cB[None, :]) - 2.0 * G)
    gw = np.sum(((cAt[:, None] + cBt[None, :]) - 2.0 * G) * T)
    return cost, np.array([np.sum(np.abs(cost)), np.sum(M * T), gw])


def sinkhorn(cost, loga, logb, eps, f, g, iters):
    f, g = f.copy(), g.copy()
    for _ in range(iters):
        f = -eps * lse((g[None, :] - cost) / eps + logb[None, :], axis=1)
        g = -eps * lse((f[:, None] - cost) / eps + loga[:, None], axis=0)
    return f, g


def plan(cost, f, g, a, b, eps, T_old):
    """-> (T, T 1, T^T 1, [|T 1 - a|_1, |T^T 1 - b|_1, |T - T_old|_1])"""
    T = a[:, None] * b[None, :] * np.exp(((f[:, None] + g[None, :]) - cost) / eps)
    r, c = T.sum(1), T.sum(0)
    return T, r, c, np.array([np.sum(np.abs(r - a)), np.sum(np.abs(c - b)), np.sum(np.abs(T - T_old))])


def solve(C1, C2, M, alpha=0.1, epsilon=0.01, relative_epsilon=True, a=None, b=None, T_init=None, max_iter=40,
          sinkhorn_iters=50):
    """the outer loop on given cost matrices -> dict with the fields of OTAlignment"""
    n, m = M.shape
    a = np.full(n, 1.0 / n) if a is None else np.asarray(a, np.float64)
    b = np.full(m, 1.0 / m) if b is None else np.asarray(b, np.float64)
    cA, cB = sqmatvec(C1, a), sqmatvec(C2, b)
    loga, logb = np.log(a), np.log(b)
    T = np.outer(a, b) if T_init is None else np.array(T_init, np.float64)
    f, g = np.zeros(n), np.zeros(m)
    eps = float(epsilon)
    for t in range(max_iter):
        cost, sums = cost_pass(C1 @ T @ C2, M, T, cA, cB, cA, cB, alpha)
        if t == 0 and relative_epsilon:
            mean = sums[0] / float(n * m)
            eps = epsilon * mean if mean > 0 else eps
        f, g = sinkhorn(cost, loga, logb, eps, f, g, sinkhorn_iters)
        T, r, c, ps = plan(cost, f, g, a, b, eps, T)
    _, sums = cost_pass(C1 @ T @ C2, M, T, cA, cB, sqmatvec(C1, r), sqmatvec(C2, c), alpha)
    return dict(T=T, expression_cost=sums[1], gw_cost=sums[2], objective=(1.0 - alpha) * sums[1] + alpha * sums[2],
                marginal_error=ps[0] + ps[1], plan_change=ps[2], n_iter=max_iter, epsilon_used=eps, f=f, g=g)


def ot_align(XA, YA, XB, YB, alpha=0.1, dissimilarity="kl", epsilon=0.01, relative_epsilon=True, a=None, b=None,
             T_init=None, norm=False, max_iter=40, sinkhorn_iters=50):
    return solve(dist(XA, norm), dist(XB, norm), expr_cost(YA, YB, dissimilarity), alpha, epsilon, relative_epsilon, a, b,
                 T_init, max_iter, sinkhorn_iters)


def gw_objective_direct(C1, C2, T):
    """sum_ijkl (C1_ik - C2_jl)^2 T_ij T_kl written out (small sizes only)"""
    p, q = T.sum(1), T.sum(0)
    return float(p @ (C1 * C1) @ p + q @ (C2 * C2) @ q - 2.0 * np.sum((C1 @ T @ C2) * T))


def stack_slices(X_list, T_list, reflection=True):
    """PASTE's stack_slices_pairwise -> (aligned, rotations, translations), aligned_k = (X_k - t_k) R_k^T"""
    Xs = [np.asarray(X, np.float64) for X in X_list]
    D = Xs[0].shape[1]
    out, rots, trans = [Xs[0]], [np.eye(D)], [np.zeros(D)]
    for k, T in enumerate(T_list):
        X, Y = out[k], Xs[k + 1]
        tx, ty = T.sum(1) @ X, T.sum(0) @ Y
        Xc, Yc = X - tx, Y - ty
        U, _, Vt = np.linalg.svd(Yc.T @ (T.T @ Xc))
        R = Vt.T @ U.T
        if not reflection and np.linalg.det(R) < 0:
            Vt = Vt.copy()
            Vt[-1] *= -1.0
            R = Vt.T @ U.T
        if k == 0:
            out[0], trans[0] = Xc, tx
        out.append(Yc @ R.T)
        rots.append(R)
        trans.append(ty)
    return out, rots, trans


# ------------------------------------------------------------------------------------------------------------------------
# the seeded cases of the anchors (tests/golden/make_ot_golden.py records their exact results)
# ------------------------------------------------------------------------------------------------------------------------
def assignment_case(seed=0, n=60, P=8):
    """anchor (a): two slices of Poisson(3) counts; only the expression cost matters at alpha = 0"""
    rs = np.random.RandomState(1000 + seed)
    YA, YB = rs.poisson(3.0, (n, P)).astype(np.float32), rs.poisson(3.0, (n, P)).astype(np.float32)
    XA, XB = rs.uniform(0.0, 10.0, (n, 2)), rs.uniform(0.0, 10.0, (n, 2))
    return XA, YA, XB, YB


def rotation(theta):
    return np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])


def permutation_case(seed, n, P, theta=0.7, shift=(3.0, -2.0)):
    """anchor (b): slice B is slice A rotated by ``theta``, shifted and row-permuted, with identical expression.  Points
    uniform in [0, 10]^2 (no lattice: its symmetries make the optimum non-unique), counts Poisson(Gamma(2, 2)).
    -> XA, YA, XB, YB, perm with XB[j] = image of XA[perm[j]]: row i's true partner is column inv[i]"""
    rs = np.random.RandomState(seed)
    XA = rs.uniform(0.0, 10.0, (n, 2))
    YA = rs.poisson(rs.gamma(2.0, 2.0, (n, P))).astype(np.float32)
    perm = rs.permutation(n)
    XB = (XA @ rotation(theta).T + np.asarray(shift))[perm]
    return XA, YA, XB, YA[perm], perm


def partner(perm):
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    return inv
