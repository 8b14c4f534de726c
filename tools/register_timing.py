"""Time the rigid pre-registration: the score table of K candidate transforms, and the whole ``rigid_register`` call.

Two slices of n = side^2 spots each, D = 2, P outputs: A a jittered lattice with smooth random-Fourier-feature expression,
B the same spots moved by 0.1 spacings of Gaussian jitter, mirrored, turned by 1.45 rad and shifted, its expression
perturbed.  The table is ``rigid_register``'s own coarse grid: 360 angles x reflection off / on about the matched
centroids, K = 720.
  rigid_scores     route B (this package): the K candidates through gpsa_rigid_scores_f64 (8 candidates per pass over A,
                   then the gather of YA[nn] and the fixed-order sums), in chunks of ``candidates_per_chunk`` (default).
  knn_loop         route A (the pieces the package had before): per candidate the transformed spots in torch, ONE
                   ``ops.knn(k = 1)`` call (gpsa_knn_f64), then a gather of YA's rows and an fp64 sum in torch.
                   ``--baseline-candidates C`` times the first C candidates only and scales the time by K / C (recorded
                   as ``knn_loop_scaled``); the loop's cost is the same for every candidate.
  rigid_register   the whole call: spacing, the coarse table, 6 refinement levels of 75 candidates, the final pairing.

One process, device events around synchronised work, every leg warmed up first, the legs alternating in blocks (median
and min-max over the blocks are reported); peak memory per leg from torch's allocator statistics, the package's scratch
tensor reported beside it.

  python tools/register_timing.py                       # 2 x 10 000 spots, P = 50
  python tools/register_timing.py --side 316 --calls 1  # 2 x 99 856 spots
Appends one JSON line per run to --out (default profiles/register_timing.jsonl).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_alignment_amd import engine as E  # noqa: E402
from spatial_alignment_amd import register  # noqa: E402

f64, f32 = torch.float64, torch.float32


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


def slices(side, P, dev):
    gen = torch.Generator().manual_seed(0)
    g = torch.arange(side, dtype=f64)
    XA = torch.stack(torch.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) + (torch.rand(side * side, 2, generator=gen, dtype=f64) - 0.5) / 2
    F = 40
    W = torch.randn(2, F, generator=gen, dtype=f64) / (side / 6.0)
    b = torch.rand(F, generator=gen, dtype=f64) * 2 * math.pi
    Y = math.sqrt(2.0 / F) * torch.cos(XA @ W + b) @ torch.randn(F, P, generator=gen, dtype=f64)
    Y = (Y - Y.mean(0)) / Y.std(0)
    perm = torch.randperm(side * side, generator=gen)
    pos = (XA[perm] + 0.1 * torch.randn(side * side, 2, generator=gen, dtype=f64)) * torch.tensor([1.0, -1.0], dtype=f64)
    c, s = math.cos(1.45), math.sin(1.45)
    XB = pos @ torch.tensor([[c, -s], [s, c]], dtype=f64).T + torch.tensor([3.0, -2.0], dtype=f64)
    YB = Y[perm] + 0.1 * torch.randn(side * side, P, generator=gen, dtype=f64)
    return XA.to(dev), Y.to(dev, f32), XB.to(dev), YB.to(dev, f32), perm.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100, help="spots per slice = side^2")
    ap.add_argument("--p", type=int, default=50)
    ap.add_argument("--n-angles", type=int, default=360)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per block")
    ap.add_argument("--baseline-candidates", type=int, default=0, help="candidates the knn loop runs (0: all K)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "register_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    XA, YA, XB, YB, perm = slices(args.side, args.p, dev)
    n, P = int(XB.shape[0]), args.p
    o = E.ops()
    cA, cB = XA.mean(0).tolist(), XB.mean(0).tolist()
    step = 2 * math.pi / args.n_angles
    T = torch.tensor([register._row(a * step, f, 0.0, 0.0, cA, cB) for f in (False, True) for a in range(args.n_angles)],
                     dtype=f64, device=dev)
    K = int(T.shape[0])
    max_dist = 3.0  # spacings of the lattice
    max_d2 = max_dist * max_dist
    Kb = K if args.baseline_candidates <= 0 else min(K, args.baseline_candidates)
    YA64 = YA.double()  # the loop's gather source, made once outside the timed region
    YB64 = YB.double()

    def batched():
        return register.rigid_scores(XA, YA, XB, YB, T, max_dist)

    def knn_loop():
        sse = torch.empty(Kb, dtype=f64, device=dev)
        nm = torch.empty(Kb, dtype=torch.int64, device=dev)
        for k in range(Kb):
            q = XB @ T[k, :4].reshape(2, 2).T + T[k, 4:]
            idx, d2 = o.knn(q, XA, 1)
            hit = d2[:, 0] <= max_d2
            diff = (YB64 - YA64[idx[:, 0].long()]) * hit[:, None]
            sse[k] = diff.square().sum()
            nm[k] = hit.sum()
        return sse, nm

    def whole():
        return register.rigid_register(XA, YA, XB, YB, n_angles=args.n_angles)

    legs = {"rigid_scores": batched, "knn_loop": knn_loop, "rigid_register": whole}
    mine, theirs, reg = batched(), knn_loop(), whole()
    agree = dict(
        n_matched_equal=bool(torch.equal(mine.n_matched[:Kb], theirs[1])),
        sse_max_rel_diff=float(((mine.sse[:Kb] - theirs[0]).abs() / theirs[0].clamp_min(1e-300)).max()),
        register_reflected=bool(reg.reflected), register_angle=reg.angle, register_score=reg.score,
        register_score_start=reg.score_start, register_nn_equals_planted=float((reg.nn.long() == perm).double().mean()),
        register_rms_spacings=float((reg.apply(XB) - XA[perm]).square().sum(1).mean().sqrt()))
    del mine, theirs, reg
    print("[register_timing] agreement:", json.dumps(agree), flush=True)

    peaks = {}
    for k, fn in legs.items():  # also the warm-up of every leg
        peaks[k] = peak_mb(fn)
        print(f"[register_timing] {k}: peak {peaks[k]:.1f} MB", flush=True)
    times = {k: [] for k in legs}
    for blk in range(args.blocks):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.calls))
        print(f"[register_timing] block {blk}: " + ", ".join(f"{k} {v[-1]:.2f} ms" for k, v in times.items()), flush=True)

    ms = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}
    if Kb < K:
        ms["knn_loop_scaled"] = {q: v * K / Kb for q, v in ms["knn_loop"].items()}
    line = dict(tool="register_timing", spots=[int(XA.shape[0]), n], D=2, P=P, K=K, max_dist_spacings=max_dist,
                baseline_candidates=Kb, blocks=args.blocks, calls=args.calls, device=torch.cuda.get_device_name(0),
                candidates_per_chunk=register._per_chunk(None, K, n, "register_timing"), agree=agree, ms=ms,
                peak_mb={k: round(v, 1) for k, v in peaks.items()},
                # the entry's tables and the kNN slices' lists live in the ops object's scratch tensor, allocated by the
                # first call (before the peaks were taken): it belongs on top of the package's peaks
                package_scratch_mb=round(sum(b.numel() for b in o._scratch.values() if b is not None) / 2**20, 1),
                not_measured="real data; kernel profiles (counters, occupancy)")
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
