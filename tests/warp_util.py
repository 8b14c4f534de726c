"""The yardstick for warp_field / unwarp: the warp's mean as a function of the point, restated in fp64 torch on the CPU
from the oracle's covariance functions and a state dict (never fed from the code under test), its Jacobian by autograd
and a reference Newton iteration.  Shared by tests/test_warp.py (CPU) and tests/test_warp_gpu.py."""
import torch

from oracle import gpsa_oracle as orc

f64 = torch.float64


class WarpRef:
    """g_v of one non-fixed view: g(x) = x A + b + k(x, Z) K_uu^-1 (delta - (Z A + b)), K_uu with the diagonal offset
    (oracle.forward_pass's warp stage, mean only, as a function of x)"""

    def __init__(self, state, kernel_warp, v):
        st = {k: t.detach().cpu().double() for k, t in state.items() if torch.is_tensor(t)}
        self.k = orc.KERNELS[kernel_warp]
        self.Z = st["Xtilde"][v]
        M, D = self.Z.shape
        self.D = D
        self.A = st["mean_slopes"][v] if "mean_slopes" in st else torch.eye(D, dtype=f64)
        self.b = st["mean_intercepts"][v] if "mean_intercepts" in st else torch.zeros(D, dtype=f64)
        self.ls, self.var = st["warp_kernel_lengthscales"][v], st["warp_kernel_variances"][v]
        Kuu = self.k(self.Z, self.Z, self.ls, self.var) + orc.JITTER * torch.eye(M, dtype=f64)
        self.L = torch.linalg.cholesky(Kuu)
        self.dc = st["delta_G_list"][v] - (self.Z @ self.A + self.b)
        self.beta = torch.cholesky_solve(self.dc, self.L)
        self.extent = float((self.Z.max(0).values - self.Z.min(0).values).max())

    @classmethod
    def from_parts(cls, kernel_warp, Z, beta, A, b, ls, var):
        """the same function from its pieces (the kernels' own arguments): no prior, no factorisation"""
        self = object.__new__(cls)
        d = lambda t: torch.as_tensor(t).detach().cpu().double()
        self.k = orc.KERNELS[kernel_warp]
        self.Z, self.beta, self.A, self.b, self.ls, self.var = d(Z), d(beta), d(A), d(b), d(ls), d(var)
        self.D = self.Z.shape[1]
        self.extent = float((self.Z.max(0).values - self.Z.min(0).values).max())
        return self

    def g(self, X):
        X = X.double()
        return X @ self.A + self.b + self.k(X, self.Z, self.ls, self.var) @ self.beta

    def g_like_forward(self, X):
        """the oracle's own association: (K_uu^-1 k(Z, X))^T (delta - mu_z)"""
        X = X.double()
        alpha = torch.cholesky_solve(self.k(self.Z, X, self.ls, self.var), self.L)
        return X @ self.A + self.b + alpha.t() @ self.dc

    def g_and_J(self, X):
        """g [n, D], J [n, D, D] with J[n, j, d] = d g_j / d x_d: one autograd call per output dimension"""
        X = X.detach().double().clone().requires_grad_(True)
        G = self.g(X)
        rows = [torch.autograd.grad(G[:, j].sum(), X, retain_graph=j + 1 < self.D)[0] for j in range(self.D)]
        return G.detach(), torch.stack(rows, 1)

    def x0(self, G):
        return (G.double() - self.b) @ torch.linalg.inv(self.A)

    def newton(self, G, x0, iters):
        """``iters`` undamped Newton updates from x0 -> the list of iterates [x_1 .. x_iters] (a row whose Jacobian is
        singular or whose iterate is not finite is NaN from there on)"""
        G, x = G.double(), x0.double().clone()
        out = []
        for _ in range(iters):
            g, J = self.g_and_J(torch.nan_to_num(x))
            dx = torch.full_like(x, float("nan"))
            ok = torch.isfinite(x).all(1) & torch.isfinite(J).all((1, 2)) & (torch.linalg.det(J) != 0)
            if ok.any():
                dx[ok] = torch.linalg.solve(J[ok], (g - G)[ok].unsqueeze(-1)).squeeze(-1)
            x = x - dx
            x[~torch.isfinite(x).all(1)] = float("nan")
            out.append(x.clone())
        return out

    def residual(self, X, G):
        return (self.g(torch.nan_to_num(X)) - G.double()).norm(dim=1)


def free_views(g):
    fixed = g.cfg["fixed_view_idx"]
    return [v for v in range(g.cfg["n_views"]) if not orc._is_fixed(fixed, v)]


def view_rows(g, v):
    """the fixture's own rows of view v, all modalities one after the other (the order of the oracle's warp stage)"""
    vi, _ = orc.make_view_index(g.cfg["n_samples"])
    return torch.cat([g.X[m][vi[m][v]] for m in g.mods], 0).double()


def forward_G_means(g, state=None):
    """view -> the oracle forward's G_means at view_rows(g, view), fp64"""
    from predict_util import _forward

    state = g.full_state() if state is None else state
    zeros = [torch.zeros((1,) + tuple(e.shape[1:])) for e in g.eps_G]
    out = _forward(g, state, 1, zeros, 0.0)["G_means"]
    vi, _ = orc.make_view_index(g.cfg["n_samples"])
    return {v: torch.cat([out[m][vi[m][v]] for m in g.mods], 0) for v in range(g.cfg["n_views"])}


def folded_state(g, v, factor=4.0):
    """the fixture's state with view v's warp exaggerated: delta_G[v] <- Z_v + factor (delta_G[v] - Z_v)"""
    st = {k: t.clone() for k, t in g.full_state().items()}
    Z = st["Xtilde"][v]
    st["delta_G_list"][v] = Z + factor * (st["delta_G_list"][v] - Z)
    return st


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))
