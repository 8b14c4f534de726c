"""Time knn (k = 10, each point left out of its own list) and knn_regress against torch on the same device.

Two views of n points each, D = 2, uniform in [0, 10]^2.
  knn:          the k nearest OTHER points of every point, per view (the gene-selection / outlier-filter searches).
  knn_regress:  view 1's outputs predicted from view 0's spots and the other way round (the alignment score's pairs),
                uniform weights, P outputs.
Route B (this package): neighbors.knn / neighbors.knn_regress - gpsa_knn_f64 + gpsa_knn_average_f32.
Route A (torch): chunked torch.cdist (fp64, the default compute mode) + topk(largest=False) + Y[idx].mean(1); the chunk is
sized so that its distance block, topk's copy of it and the [chunk, k, P] gather stay under --budget-gb (8).  A second
torch leg runs the same in fp32, which is what a user in a hurry would do; its neighbours differ from the fp64 ones where
distances are close, so it is context, not the baseline.

One process, device events around synchronised work, every leg warmed up first, the legs alternating in blocks (median
and min-max over the blocks are reported); peak memory per leg from torch's allocator statistics (the package's scratch
lives in a torch tensor, so it is counted).  If sklearn is importable its CPU time (kd_tree, one call) is added as context.

  python tools/neighbors_timing.py                      # 2 x 10 000 points, P = 50 and P = 3000
  python tools/neighbors_timing.py --side 316 --p 50    # 2 x 99 856 points
Appends one JSON line per run to --out (default profiles/neighbors_timing.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_alignment_amd import engine as E  # noqa: E402
from spatial_alignment_amd import neighbors  # noqa: E402

K = 10


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


def torch_chunk(n_ref, P, elem, budget):
    """query rows per chunk: the distance block and topk's working copy (2 n_ref elem bytes a row) and the gather with
    its mean (about 2 K P 4 bytes a row) under the budget"""
    per_row = 2 * n_ref * elem + 2 * K * P * 4 + 64
    return max(1, int(budget // per_row))


def torch_knn(Q, R, k, exclude_self, chunk):
    idx = torch.empty(Q.shape[0], k, dtype=torch.long, device=Q.device)
    d = torch.empty(Q.shape[0], k, dtype=Q.dtype, device=Q.device)
    kk = k + 1 if exclude_self else k
    for a in range(0, Q.shape[0], chunk):
        dd, ii = torch.cdist(Q[a: a + chunk], R).topk(kk, dim=1, largest=False)
        idx[a: a + chunk], d[a: a + chunk] = ii[:, kk - k:], dd[:, kk - k:]  # sklearn's way: column 0 is the point itself
    return idx, d


def torch_regress(Xa, Ya, Xb, k, chunk):
    out = torch.empty(Xb.shape[0], Ya.shape[1], dtype=Ya.dtype, device=Ya.device)
    for a in range(0, Xb.shape[0], chunk):
        ii = torch.cdist(Xb[a: a + chunk], Xa).topk(k, dim=1, largest=False).indices
        out[a: a + chunk] = Ya[ii].mean(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100, help="points per view = side^2")
    ap.add_argument("--p", type=int, nargs="+", default=[50, 3000], help="outputs of the regression legs")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per block")
    ap.add_argument("--budget-gb", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "neighbors_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    n = args.side * args.side
    gen = torch.Generator().manual_seed(0)
    X = [(torch.rand(n, 2, generator=gen, dtype=torch.float64) * 10).to(dev) for _ in range(2)]
    X32 = [x.float() for x in X]
    budget = args.budget_gb * 1e9

    legs, agree = {}, {}
    c64, c32 = torch_chunk(n, 0, 8, budget), torch_chunk(n, 0, 4, budget)
    legs["knn"] = lambda: [neighbors.knn(x, k=K) for x in X]
    legs["torch_knn_f64"] = lambda: [torch_knn(x, x, K, True, c64) for x in X]
    legs["torch_knn_f32"] = lambda: [torch_knn(x, x, K, True, c32) for x in X32]
    mine, theirs = legs["knn"](), legs["torch_knn_f64"]()
    agree["knn_rows_equal_torch_f64"] = [float((m.idx.long() == t[0]).all(1).double().mean()) for m, t in zip(mine, theirs)]
    agree["knn_rows_equal_torch_f32"] = [float((m.idx.long() == t[0]).all(1).double().mean())
                                         for m, t in zip(mine, legs["torch_knn_f32"]())]
    del mine, theirs
    chunks = {"knn_f64": c64, "knn_f32": c32}
    Ys = {}
    for P in args.p:
        Ys[P] = [torch.randn(n, P, generator=gen).to(dev) for _ in range(2)]
        cp64, cp32 = torch_chunk(n, P, 8, budget), torch_chunk(n, P, 4, budget)
        chunks[f"regress_P{P}_f64"], chunks[f"regress_P{P}_f32"] = cp64, cp32
        legs[f"knn_regress_P{P}"] = lambda P=P: [neighbors.knn_regress(X[a], Ys[P][a], X[1 - a], k=K) for a in (0, 1)]
        legs[f"torch_regress_P{P}_f64"] = lambda P=P, c=cp64: [torch_regress(X[a], Ys[P][a], X[1 - a], K, c) for a in (0, 1)]
        legs[f"torch_regress_P{P}_f32"] = lambda P=P, c=cp32: [torch_regress(X32[a], Ys[P][a], X32[1 - a], K, c)
                                                               for a in (0, 1)]
        m, t = legs[f"knn_regress_P{P}"](), legs[f"torch_regress_P{P}_f64"]()
        agree[f"regress_P{P}_max_abs_diff"] = max(float((a - b).abs().max()) for a, b in zip(m, t))
        del m, t

    peaks = {k: peak_mb(fn) for k, fn in legs.items()}  # also the warm-up of every leg
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.calls))

    line = dict(tool="neighbors_timing", points=[n, n], D=2, k=K, P=args.p, blocks=args.blocks, calls=args.calls,
                budget_gb=args.budget_gb, torch_chunk_rows=chunks, device=torch.cuda.get_device_name(0), agree=agree,
                ms={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()},
                peak_mb={k: round(v, 1) for k, v in peaks.items()},
                # the slices' lists of gpsa_knn_f64 live in the ops object's scratch tensor, allocated by the first call
                # (before the peaks were taken): it is reported here and belongs on top of the package's peaks
                package_scratch_mb=round(sum(b.numel() for b in E.ops()._scratch.values() if b is not None) / 2**20, 1))
    try:
        from sklearn.neighbors import KNeighborsRegressor, NearestNeighbors

        Xh = [x.cpu().numpy() for x in X]
        t0 = time.perf_counter()
        for x in Xh:
            NearestNeighbors(n_neighbors=K + 1, algorithm="kd_tree").fit(x).kneighbors(x)
        t1 = time.perf_counter()
        P = args.p[0]
        Yh = [y.cpu().numpy() for y in Ys[P]]
        for a in (0, 1):
            KNeighborsRegressor(n_neighbors=K, algorithm="kd_tree").fit(Xh[a], Yh[a]).predict(Xh[1 - a])
        t2 = time.perf_counter()
        line["sklearn_cpu_ms"] = {"knn": 1e3 * (t1 - t0), f"knn_regress_P{P}": 1e3 * (t2 - t1),
                                  "threads": os.environ.get("OMP_NUM_THREADS")}
    except ImportError:
        pass
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
