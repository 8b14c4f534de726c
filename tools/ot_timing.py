"""Time the optimal-transport alignment (spatial_alignment_amd/ot.py over csrc/ot.hip) against the same algorithm written in
fp64 torch on the same device (torch.matmul, torch.logsumexp, elementwise ops) at the same fixed iteration counts.

Two slices of n spots each (points uniform in [0, 10]^2, the second a rotated, shifted, row-permuted copy with the same
Poisson(Gamma(2, 2)) counts, P genes), default parameters of ``ot_align`` (alpha 0.1, "kl", relative epsilon 0.01,
40 outer steps of 50 sweeps).  Legs:
  ot_align / torch_align        the whole solve from coordinates and counts to the plan
  sweep / torch_sweep           ONE Sinkhorn sweep (row pass + column pass) on the final cost; the bytes it MUST move are the
                                cost matrix twice (16 n m), reported over the time as a share of the 8.0 TB/s HBM rate of
                                MI355X_MICROARCH.md
  products / torch_products     one outer step's two products C1 T C2 (gpsa_gemm / torch.matmul), 4 n^3 flops
One process, device events around synchronised work, every leg warmed up first (also where its peak memory is taken from
torch's allocator statistics), the legs alternating in blocks; median and min-max over the blocks.

  python tools/ot_timing.py                     # n = 2000 and n = 10 000, P = 50
  python tools/ot_timing.py --sizes 500 --blocks 3
Appends one JSON line per size to --out (default profiles/ot_timing.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_alignment_amd as pkg  # noqa: E402
from spatial_alignment_amd import engine as E  # noqa: E402
from spatial_alignment_amd import ot  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
f64 = torch.float64


def timed(fn, calls=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2**20


def make_slices(n, P, dev):
    rs = np.random.RandomState(0)
    XA = rs.uniform(0.0, 10.0, (n, 2))
    YA = rs.poisson(rs.gamma(2.0, 2.0, (n, P))).astype(np.float32)
    perm = rs.permutation(n)
    c, s = np.cos(0.7), np.sin(0.7)
    XB = (XA @ np.array([[c, -s], [s, c]]).T + np.array([3.0, -2.0]))[perm]
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    return t(XA, f64), t(YA, torch.float32), t(XB, f64), t(YA[perm], torch.float32), t(perm, torch.int64)


def t_sweep(cost, loga, logb, eps, f, g):
    f = -eps * torch.logsumexp((g[None, :] - cost) / eps + logb[None, :], dim=1)
    g = -eps * torch.logsumexp((f[:, None] - cost) / eps + loga[:, None], dim=0)
    return f, g


def t_align(XA, YA, XB, YB, alpha=0.1, epsilon=0.01, max_iter=40, sinkhorn_iters=50):
    """ot_align's algorithm at its defaults, in fp64 torch"""
    n, m = XA.shape[0], XB.shape[0]
    C1, C2 = torch.cdist(XA, XA), torch.cdist(XB, XB)
    Pa, Pb = YA.double() + 0.01, YB.double() + 0.01
    Pa, Pb = Pa / Pa.sum(1, keepdim=True), Pb / Pb.sum(1, keepdim=True)
    M = (Pa * Pa.log()).sum(1)[:, None] - Pa @ Pb.log().T
    a, b = torch.full((n,), 1.0 / n, dtype=f64, device=XA.device), torch.full((m,), 1.0 / m, dtype=f64, device=XA.device)
    cA, cB = (C1 * C1) @ a, (C2 * C2) @ b
    loga, logb = a.log(), b.log()
    T = torch.outer(a, b)
    f, g = torch.zeros_like(a), torch.zeros_like(b)
    eps = None
    for t in range(max_iter):
        cost = (1.0 - alpha) * M + 2.0 * alpha * (cA[:, None] + cB[None, :] - 2.0 * (C1 @ T @ C2))
        if eps is None:
            eps = epsilon * cost.abs().mean()
        for _ in range(sinkhorn_iters):
            f, g = t_sweep(cost, loga, logb, eps, f, g)
        T = a[:, None] * b[None, :] * torch.exp((f[:, None] + g[None, :] - cost) / eps)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[2000, 10000])
    ap.add_argument("--genes", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "ot_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    o = E.ops()
    for n in args.sizes:
        XA, YA, XB, YB, perm = make_slices(n, args.genes, dev)
        res = pkg.ot_align(XA, YA, XB, YB)
        Tt = t_align(XA, YA, XB, YB)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n, device=dev)
        agree = dict(max_abs_diff_vs_torch_over_max_T=float((res.T - Tt).abs().max() / Tt.max()),
                     rows_at_their_partner=float((res.T.argmax(1) == inv).double().mean()),
                     torch_rows_at_their_partner=float((Tt.argmax(1) == inv).double().mean()),
                     marginal_error=res.marginal_error, plan_change=res.plan_change, objective=res.objective,
                     epsilon_used=res.epsilon_used)
        del Tt
        # the pieces, on the solve's own matrices
        C1, C2 = ot.spatial_cost(XA), ot.spatial_cost(XB)
        a = torch.full((n,), 1.0 / n, dtype=f64, device=dev)
        cA, cB = o.ot_sqmatvec(C1, a), o.ot_sqmatvec(C2, a)
        cost = o.gemm(o.gemm(C1, res.T), C2)
        o.ot_cost(cost, ot.expression_cost(YA, YB), res.T, cA, cB, cA, cB, 0.1)  # the cost at the returned plan
        loga, eps = a.log(), torch.full((1,), res.epsilon_used, dtype=f64, device=dev)
        f, g = res.f.clone(), res.g.clone()
        tmp, G = torch.empty(n, n, dtype=f64, device=dev), torch.empty(n, n, dtype=f64, device=dev)
        e = float(eps)

        def products():
            o.gemm(C1, res.T, out=tmp)
            return o.gemm(tmp, C2, out=G)

        legs = {
            "ot_align": lambda: pkg.ot_align(XA, YA, XB, YB).T,
            "torch_align": lambda: t_align(XA, YA, XB, YB),
            "sweep": lambda: o.ot_sinkhorn(cost, loga, loga, eps, f, g, 1),
            "torch_sweep": lambda: t_sweep(cost, loga, loga, e, f, g),
            "products": products,
            "torch_products": lambda: C1 @ res.T @ C2,
        }
        peaks = {}
        for k, fn in legs.items():  # also the warm-up of every leg
            peaks[k] = peak_mib(fn)
            print(f"[ot_timing] n = {n}: warmed up {k}, peak {peaks[k]:.0f} MiB", flush=True)
        times = {k: [] for k in legs}
        for blk in range(args.blocks):
            for k, fn in legs.items():
                times[k].append(timed(fn, 1 if k.endswith("align") else 10))
            print(f"[ot_timing] n = {n}: block {blk + 1} of {args.blocks}", flush=True)
        ms = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}
        sweep_bytes = 16 * n * n
        line = dict(tool="ot_timing", n=n, m=n, P=args.genes, alpha=0.1, epsilon=0.01, max_iter=40, sinkhorn_iters=50,
                    blocks=args.blocks, device=torch.cuda.get_device_name(0), cost_matrix_mib=round(8 * n * n / 2**20, 1),
                    ms=ms, peak_mib={k: round(v, 1) for k, v in peaks.items()},
                    speedup_over_torch={k: ms["torch_" + k]["median"] / ms[k]["median"] for k in ("sweep", "products")}
                    | {"ot_align": ms["torch_align"]["median"] / ms["ot_align"]["median"]},
                    sweep_must_move_bytes=sweep_bytes,
                    sweep_share_of_8_tb_s=sweep_bytes / (ms["sweep"]["median"] * 1e-3) / HBM_BYTES_PER_S,
                    products_tflops=4.0 * n ** 3 / (ms["products"]["median"] * 1e-3) / 1e12, agree=agree,
                    package_scratch_mib=round(sum(b.numel() * b.element_size() for b in o._scratch.values()
                                                 if b is not None) / 2**20, 1))
        print(json.dumps(line))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        del XA, YA, XB, YB, res, C1, C2, cost, tmp, G, legs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
