"""The fp64 numpy yardstick of expression PCA (spatial_alignment_amd/pca.py) and the seeded inputs its suites share.

The yardstick centres and scales, forms Z^T Z / (N - 1), decomposes it with numpy.linalg.eigh, applies sklearn's sign rule
and computes scores; ``subspace`` is the orthogonal iteration of pca.py restated in numpy with the same start, the same
check schedule and the same stopping rule.  tests/test_pca.py holds it against sklearn's own results recorded in
tests/golden/reference_pca.npz (written by tests/golden/make_pca_golden.py).
"""
import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
SEED = 1
OVERSAMPLE = 8
# (N, P, r, decay, noise), n_components: low-rank signal with singular values 10 decay^j, isotropic noise, a column offset
CASES = [((300, 129, 12, 0.8, 0.05), 10), ((257, 65, 8, 0.7, 0.1), 5), ((1025, 257, 20, 0.85, 0.05), 16),
         ((97, 45, 6, 0.75, 0.1), 4), ((64, 200, 10, 0.8, 0.05), 8)]
# name -> (index into CASES, the views' rows, center, scale, a column made constant or None)
VARIANTS = {
    "case0": (0, [300], "pooled", False, None), "case1": (1, [257], "pooled", False, None),
    "case2": (2, [1025], "pooled", False, None), "case3": (3, [97], "pooled", False, None),
    "case4": (4, [64], "pooled", False, None),
    "view2": (0, [130, 170], "view", False, None), "view3": (3, [40, 2, 55], "view", False, None),
    "scale_const": (1, [257], "pooled", True, 7), "view2_scale": (0, [130, 170], "view", True, None),
}
GAP_BAR = 1e-3  # the relative eigengap every case used on the device must have at each kept component
NOISE = dict(seed=7, shape=(400, 150), k=6)


def make_case(N, P, r, decay, noise, seed=SEED):
    g = np.random.default_rng(seed)
    U = g.standard_normal((N, r))
    V, _ = np.linalg.qr(g.standard_normal((P, r)))
    s = 10.0 * decay ** np.arange(r)
    Y = (U * s) @ V.T + noise * g.standard_normal((N, P)) + 3.0 * g.standard_normal(P)
    return Y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def variant(name):
    """-> (Y fp32 [N, P], ns, center, scale, k); computed once and shared: do not modify"""
    ci, ns, center, scale, const = VARIANTS[name]
    shape, k = CASES[ci]
    Y = make_case(*shape)
    if const is not None:
        Y[:, const] = np.float32(2.5)
    Y.setflags(write=False)
    return Y, list(ns), center, scale, k


@functools.lru_cache(maxsize=None)
def noise_matrix():
    Y = np.random.default_rng(NOISE["seed"]).standard_normal(NOISE["shape"]).astype(np.float32)
    Y.setflags(write=False)
    return Y


def offsets(ns):
    return [0] + [int(x) for x in np.cumsum(ns)]


def view_stats(Y, ns, center, scale):
    """(ns used, mean [V, P], inv_scale [V, P] or None): two-pass fp64 moments; ddof = 0; a column with
    var <= 4 n eps mean(y^2) inside a view is constant there: inv_scale 0 (pca.close_moments' rule)"""
    Y = np.asarray(Y, dtype=np.float64)
    if center == "pooled":
        ns = [Y.shape[0]]
    off = offsets(ns)
    mean = np.stack([Y[a:b].mean(0) for a, b in zip(off, off[1:])])
    if not scale:
        return ns, mean, None
    inv = np.zeros_like(mean)
    for v, (a, b) in enumerate(zip(off, off[1:])):
        var = ((Y[a:b] - mean[v]) ** 2).mean(0)
        msq = (Y[a:b] ** 2).mean(0)
        ok = var > 4.0 * (b - a) * EPS * msq
        inv[v, ok] = 1.0 / np.sqrt(var[ok])
    return ns, mean, inv


def zmatrix(Y, ns, mean, inv_scale):
    """the centred and scaled matrix in fp64, formed as the kernels form it: (y - mean) * inv_scale"""
    Z = np.asarray(Y, dtype=np.float64).copy()
    off = offsets(ns)
    for v, (a, b) in enumerate(zip(off, off[1:])):
        Z[a:b] -= mean[v]
        if inv_scale is not None:
            Z[a:b] *= inv_scale[v]
    return Z


def sign_rule(components):
    """sklearn >= 1.5: in each row the entry of largest magnitude is positive (numpy's argmax: ties to the lower index)"""
    idx = np.argmax(np.abs(components), axis=1)
    sgn = np.where(components[np.arange(components.shape[0]), idx] < 0, -1.0, 1.0)
    return components * sgn[:, None]


def eigh_pca(C, k):
    """-> (components [k, P] with the sign rule, variances [k] descending, all eigenvalues descending)"""
    w, U = np.linalg.eigh(C)
    w, U = w[::-1], U[:, ::-1]
    return sign_rule(U[:, :k].T.copy()), w[:k].copy(), w.copy()


def yardstick(Y, ns, center, scale, k):
    ns, mean, inv = view_stats(Y, ns, center, scale)
    Z = zmatrix(Y, ns, mean, inv)
    N = Z.shape[0]
    C = Z.T @ Z / (N - 1)
    comps, lam, allw = eigh_pca(C, k)
    return dict(ns=ns, mean=mean, inv_scale=inv, Z=Z, C=C, components=comps, explained_variance=lam, eigenvalues=allw,
                ratio=lam / np.trace(C), singular_values=np.sqrt(lam * (N - 1)), scores=Z @ comps.T)


def relative_gaps(eigenvalues, k):
    """(l_i - l_{i+1}) / l_1 for the kept components i < k"""
    return (eigenvalues[:k] - eigenvalues[1:k + 1]) / eigenvalues[0]


def residuals(C, components, lam):
    """|C v_i - l_i v_i|_2 / l_1"""
    R = C @ components.T - components.T * lam
    return np.sqrt((R * R).sum(0)) / lam[0]


def _cholqr2(Z):
    for _ in range(2):
        L = np.linalg.cholesky(Z.T @ Z)
        Z = Z @ np.linalg.inv(L).T
    return Z


def subspace(C, k, m, tol=1e-9, max_iter=300, check_every=10, seed=0):
    """pca._subspace in numpy -> (components [k, P] signed, variances [k], residual [k], n_iter, converged)"""
    P = C.shape[0]
    Q = np.random.default_rng(seed).standard_normal((P, m))
    it = 0
    while True:
        it += 1
        Q = _cholqr2(C @ Q)
        if it % check_every and it < max_iter:
            continue
        Z = C @ Q
        B = Q.T @ Z
        w, S = np.linalg.eigh(0.5 * (B + B.T))
        w, S = w[::-1], S[:, ::-1]
        Q, Z = Q @ S, Z @ S
        R = Z - Q * w
        res = np.sqrt((R * R).sum(0))[:k] / w[0]
        converged = bool(res.max() <= tol)
        if converged or it >= max_iter:
            return sign_rule(Q[:, :k].T.copy()), w[:k].copy(), res, it, converged
