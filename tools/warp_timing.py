"""Time warp_field (with the Jacobian) and unwarp(max_iter=12) against the only route that existed before them.

Route A (what a user could do before): the built-in covariance functions of kernels.py on the device in fp64 plus
torch.autograd.grad, one call per output dimension, in row chunks that fit (--chunk); for the inverse the same evaluation
inside a hand-written Newton loop of 12 updates with the 2 x 2 solve in closed form.  Both routes form beta =
K_uu^-1 (delta - mu_z) once per call (warp._warp_model), so the difference is the per-point work alone.
Route B: model.warp_field(X, view) and model.unwarp(G, view, max_iter=12).

One process, device events around synchronised work, every shape warmed up first, the routes alternating in blocks
(median and min-max over the blocks are reported).  D = 2, RBF warp kernel, inducing points uniform in the data's box,
delta_G a smooth displacement of them (no fold), warp lengthscale 0.7.

  python tools/warp_timing.py                         # 2 x 10 000 points, M = 200
  python tools/warp_timing.py --side 316 --m 1000     # 2 x 99 856 points, M = 1000
Appends one JSON line per run to --out (default profiles/warp_timing.jsonl).
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_alignment_amd as gp  # noqa: E402
from spatial_alignment_amd import engine as E  # noqa: E402
from spatial_alignment_amd import warp as W  # noqa: E402

f64 = torch.float64


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def eval_autograd(mdl, X, chunk, jacobian=True):
    """route A: g (and J) of the rows of X by the covariance function and autograd, chunk by chunk"""
    _, Z, beta, A, b, ls_u, var_u = mdl
    n, D = X.shape
    G = torch.empty(n, D, dtype=f64, device=X.device)
    J = torch.empty(n, D, D, dtype=f64, device=X.device) if jacobian else None
    for a in range(0, n, chunk):
        with torch.enable_grad():
            Xc = X[a: a + chunk].detach().clone().requires_grad_(jacobian)
            Gc = Xc @ A + b + gp.rbf_kernel(Xc, Z, ls_u, var_u) @ beta
            if jacobian:
                for j in range(D):
                    J[a: a + chunk, j] = torch.autograd.grad(Gc[:, j].sum(), Xc, retain_graph=j + 1 < D)[0]
        G[a: a + chunk] = Gc.detach()
    return G, J


def route_a_field(model, X, view, chunk):
    mdl = W._warp_model(model, view, E.ops())
    G, J = eval_autograd(mdl, X, chunk)
    det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    return G, J, det


def route_a_unwarp(model, G, view, chunk, iters):
    mdl = W._warp_model(model, view, E.ops())
    A, b = mdl[3], mdl[4]
    x = (G - b) @ torch.linalg.inv(A.cpu()).to(G.device)
    for _ in range(iters):
        g, J = eval_autograd(mdl, x, chunk)
        r = g - G
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        dx0 = (J[:, 1, 1] * r[:, 0] - J[:, 0, 1] * r[:, 1]) / det
        dx1 = (J[:, 0, 0] * r[:, 1] - J[:, 1, 0] * r[:, 0]) / det
        x = x - torch.stack([dx0, dx1], 1)
    g, _ = eval_autograd(mdl, x, chunk, jacobian=False)
    return x, (g - G).norm(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100, help="points per view = side^2")
    ap.add_argument("--m", type=int, default=200)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per block")
    ap.add_argument("--chunk", type=int, default=20000, help="rows per chunk of the autograd route")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "warp_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    n, M = args.side * args.side, args.m
    gen = torch.Generator().manual_seed(0)
    mod = "expression"
    dd = {mod: {"spatial_coords": torch.rand(2 * n, 2, generator=gen) * 10, "outputs": torch.randn(2 * n, 2, generator=gen),
                "n_samples_list": [n, n]}}
    torch.manual_seed(0)
    np.random.seed(0)
    model = gp.VariationalGPSA(dd, m_X_per_view=M, m_G=16, data_init=False, n_latent_gps={mod: None}, fixed_view_idx=None)
    with torch.no_grad():
        Z = torch.rand(model.Xtilde.shape, generator=gen) * 10
        model.Xtilde.copy_(Z)
        model.delta_G_list.copy_(Z + 0.3 * torch.sin(0.6 * Z.flip(-1)))  # a smooth displacement: no fold
        model.warp_kernel_lengthscales.fill_(math.log(0.7))
    model = model.to(dev)
    X = [dd[mod]["spatial_coords"][:n].to(dev).double(), dd[mod]["spatial_coords"][n:].to(dev).double()]

    def b_field():
        return [model.warp_field(X[v], v) for v in (0, 1)]

    def a_field():
        return [route_a_field(model, X[v], v, args.chunk) for v in (0, 1)]

    Gs = [r.G_mean for r in b_field()]

    def b_unwarp():
        return [model.unwarp(Gs[v], v, max_iter=args.iters) for v in (0, 1)]

    def a_unwarp():
        return [route_a_unwarp(model, Gs[v], v, args.chunk, args.iters) for v in (0, 1)]

    # the routes agree (and the warp is not folded) before anything is timed
    fb, fa, ub, ua = b_field(), a_field(), b_unwarp(), a_unwarp()
    agree = dict(
        G=max(float((fb[v].G_mean - fa[v][0]).abs().max()) for v in (0, 1)),
        J=max(float((fb[v].jacobian - fa[v][1]).abs().max()) for v in (0, 1)),
        X=max(float((ub[v].X - ua[v][0]).abs().max()) for v in (0, 1)),
        n_folded=sum(int(fb[v].n_folded) for v in (0, 1)),
        converged=sum(int(ub[v].converged.sum()) for v in (0, 1)),
        worst_residual=max(float(ub[v].residual.max()) for v in (0, 1)),
        round_trip=max(float((ub[v].X - X[v]).abs().max()) for v in (0, 1)),
    )
    legs = {"warp_field": b_field, "autograd_field": a_field, "unwarp": b_unwarp, "autograd_newton": a_unwarp}
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.calls))
    line = dict(tool="warp_timing", points=[n, n], M=M, D=2, kind="rbf", iters=args.iters, chunk=args.chunk,
                blocks=args.blocks, calls=args.calls, device=torch.cuda.get_device_name(0), agree=agree,
                ms={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()})
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
