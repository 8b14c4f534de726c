"""Time the permuted Moran / Geary statistic (gpsa_autocorr_perm_f64) against the same algorithm in fp64 torch on the device.

n uniform points in 2-D, k = 6, the "none" and the "union" graph (row-standardised), P centred fp64 columns, the identity
and 100 random permutations, both modes.
Route B (this package): ops.autocorr_perm on all 101 permutation rows in one call - the rows of Z gathered through the
  permutation inside the kernel; next to it the whole spatial_autocorr call on the prebuilt graph (permutations drawn,
  Z formed, p-values and FDR columns closed).
Route A (torch): per permutation Zp = Z[perm] (a permuted [n, P] copy), lag = torch.sparse.mm(W_csr, Zp), Moran
  sum(Zp * lag, 0); Geary from the same lag, sum((w_i. + w_.i) Zp^2, 0) - 2 sum(Zp * lag, 0).

One process, device events around synchronised work, every leg warmed up first, the legs alternating in blocks (median
and min-max over the blocks); peak memory per leg from torch's allocator (the package's workspace lives in a torch
tensor held by the ops object and is reported separately).  The entry's gather rate is (permutation rows) x (n + nnz)
gathered rows x 8 P bytes over its time, to be read next to the guide figures for indexed rows: 7.4-8.6 TB/s from the
Infinity Cache, 5.5-6.1 TB/s from HBM.

  python tools/autocorr_timing.py                       # n = 10 000, P = 50 and 2000
  python tools/autocorr_timing.py --side 316            # n = 99 856
Appends one JSON line per run to --out (default profiles/autocorr_timing.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_alignment_amd as gp  # noqa: E402
from spatial_alignment_amd import engine as E  # noqa: E402

K, R = 6, 100
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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2**20


def torch_route(Z, W, rc, perms, mode):
    out = torch.empty(perms.shape[0], Z.shape[1], dtype=f64, device=Z.device)
    for r in range(perms.shape[0]):
        Zp = Z[perms[r].long()]
        cross = (Zp * torch.sparse.mm(W, Zp)).sum(0)
        out[r] = cross if mode == "moran" else (rc * Zp.square()).sum(0) - 2.0 * cross
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100, help="points = side^2")
    ap.add_argument("--p", type=int, nargs="+", default=[50, 2000])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1, help="calls per block")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "autocorr_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    n = args.side * args.side
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(n, 2, generator=gen, dtype=f64, device=dev) * args.side
    perms = torch.cat([torch.arange(n, device=dev).view(1, n),
                       torch.argsort(torch.rand(R, n, generator=gen, device=dev), dim=1)]).to(torch.int32).contiguous()
    o = E.ops()
    results = []
    for kind in ("none", "union"):
        g = gp.spatial_graph(X, k=K, symmetric=kind)
        W = torch.sparse_csr_tensor(g.crow, g.col.long(), g.w, size=(n, n))
        rows = torch.repeat_interleave(torch.arange(n, device=dev), g.crow[1:] - g.crow[:-1])
        rc = (torch.zeros(n, dtype=f64, device=dev).index_add_(0, rows, g.w)
              + torch.zeros(n, dtype=f64, device=dev).index_add_(0, g.col.long(), g.w)).view(n, 1)
        for P in args.p:
            Y = torch.randn(n, P, generator=gen, device=dev)
            Z = Y.double()
            Z.sub_(Z.mean(0))
            for mode in ("moran", "geary"):
                legs = {"entry": lambda: o.autocorr_perm(Z, g.crow, g.col, g.w, perms, mode)[0],
                        "torch": lambda: torch_route(Z, W, rc, perms, mode),
                        "spatial_autocorr": lambda: gp.spatial_autocorr(g, Y, mode=mode, n_perms=R, generator=gen)}
                a, b = legs["entry"](), legs["torch"]()
                scale = (Z.square().sum(0) * (float(rc.sum()) if mode == "geary" else 1.0)).clamp_min(1e-300)
                diff = float(((a - b).abs() / scale).max())
                del a, b
                peaks = {name: peak_mb(fn) for name, fn in legs.items()}  # also the warm-up of every leg
                times = {name: [] for name in legs}
                for _ in range(args.blocks):
                    for name, fn in legs.items():
                        times[name].append(timed(fn, args.calls))
                ms = {name: dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in times.items()}
                gathered = (R + 1) * (n + g.nnz) * 8 * P
                results.append(dict(graph=kind, nnz=g.nnz, P=P, mode=mode, ms=ms,
                                    peak_mb={name: round(v, 1) for name, v in peaks.items()},
                                    entry_gather_tb_per_s=gathered / (ms["entry"]["median"] * 1e-3) / 1e12,
                                    gathered_gb=gathered / 1e9, z_mb=8 * n * P / 2**20,
                                    entry_vs_torch_max_diff_over_sum_z2=diff,
                                    workspace_mb=o._wsq("gpsa_autocorr_perm_workspace", n, P, R + 1) / 2**20))
                print(json.dumps(results[-1]), flush=True)
            del Y, Z
    line = dict(tool="autocorr_timing", n=n, k=K, permutations=R, blocks=args.blocks, calls=args.calls,
                device=torch.cuda.get_device_name(0), results=results,
                guide_indexed_rows_tb_per_s={"infinity_cache": [7.4, 8.6], "hbm": [5.5, 6.1]},
                not_measured=["real data", "squidpy itself", "kernel profiles"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
