"""Time expression PCA (spatial_alignment_amd/pca.py over csrc/pca.hip) against the straightforward fp64 torch route on the
same device.

Y [N, P] fp32: a rank-64 signal plus noise plus a column offset, generated on the device in row chunks; two views of N / 2
rows, centred and scaled per view.  Legs:
  entry_gram / entry_project     the C entries alone (ops.pca_gram, ops.pca_project with k components, fp32 scores)
  torch_gram / torch_project     Z = (Y.double() - mean) * inv_scale per view (the centred fp64 copy), Z.T @ Z and
                                 Z @ comp.T through torch (the vendor's BLAS: a yardstick, not a path of the package)
  expression_pca                 the whole call, solver="subspace" (moments, Gram, iteration); sizes with --whole only
  transform                      ExpressionPCA.transform of the training matrix
  host_eigh                      numpy.linalg.eigh of the P x P covariance on the host (what solver="host" pays), once
The Gram's useful work, N P (P + 1) flops (the upper triangle, a multiply and an add each), over its time is reported as
a share of the 78.6 TF fp64-MFMA peak of MI355X_MICROARCH.md; the projection's N P 4 bytes over its time as a share of
the 8.0 TB/s HBM rate.

One process, device events around synchronised work, every leg warmed up first (where its peak memory is taken from
torch's allocator statistics), the legs alternating in blocks; median and min-max over the blocks.

  python tools/pca_timing.py                       # 20 000 x 2000, 100 000 x 2000 (whole call too), 100 000 x 20 000
  python tools/pca_timing.py --shapes 8000x1000 --whole 8000x1000
Appends one JSON line per shape to --out (default profiles/pca_timing.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_alignment_amd as gp  # noqa: E402
from spatial_alignment_amd import engine as E  # noqa: E402
from spatial_alignment_amd import pca  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
MFMA_F64_FLOPS = 78.6e12
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


def make_matrix(N, P, dev, rank=64, chunk=10000):
    gen = torch.Generator(device=dev).manual_seed(0)
    load = torch.randn(rank, P, device=dev, generator=gen) * torch.logspace(0, -1.5, rank, device=dev)[:, None]
    shift = 3.0 * torch.randn(P, device=dev, generator=gen)
    Y = torch.empty(N, P, device=dev)
    for a in range(0, N, chunk):
        n = min(chunk, N - a)
        Y[a:a + n] = torch.randn(n, rank, device=dev, generator=gen) @ load + shift \
            + 0.3 * torch.randn(n, P, device=dev, generator=gen)
    return Y


def torch_z(Y, off, mean, inv):
    return torch.cat([(Y[a:b].double() - mean[v]) * inv[v] for v, (a, b) in enumerate(zip(off, off[1:]))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20000x2000", "100000x2000", "100000x20000"])
    ap.add_argument("--whole", nargs="*", default=["20000x2000", "100000x2000"], help="shapes that also time the whole call")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per block (1 above 10^9 elements)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "pca_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    o = E.ops()
    for shape in args.shapes:
        N, P = (int(v) for v in shape.split("x"))
        k = args.k
        calls = 1 if N * P > 10**9 else args.calls
        Y = make_matrix(N, P, dev)
        ns = [N // 2, N - N // 2]
        off = [0, ns[0], N]
        s1, s2, _, _ = o.column_moments(Y, "identity", off)
        mean, inv = pca.close_moments(s1, s2, ns, True)
        comp = torch.linalg.qr(torch.randn(P, k, dtype=f64, device=dev,
                                           generator=torch.Generator(device=dev).manual_seed(1)))[0].t().contiguous()
        legs = {
            "entry_gram": lambda: o.pca_gram(Y, mean, off, inv),
            "entry_project": lambda: o.pca_project(Y, mean, off, comp, inv),
            "torch_gram": lambda: (lambda Z: Z.t() @ Z)(torch_z(Y, off, mean, inv)),
            "torch_project": lambda: (torch_z(Y, off, mean, inv) @ comp.t()).float(),
        }
        res = None
        if shape in args.whole:
            res = gp.expression_pca(Y, ns, n_components=k, center="view", scale=True)
            legs["expression_pca"] = lambda: gp.expression_pca(Y, ns, n_components=k, center="view", scale=True)
            legs["transform"] = lambda: res.transform(Y, ns)
        Gm, Gt = legs["entry_gram"](), legs["torch_gram"]()
        Sm, St = o.pca_project(Y, mean, off, comp, inv, f64), torch_z(Y, off, mean, inv) @ comp.t()
        agree = {
            "gram_max_diff_over_max_abs": float((Gm - Gt).abs().max() / Gt.abs().max()),
            "gram_symmetric": bool(torch.equal(Gm, Gm.t())),
            "project_max_diff_over_max_abs": float((Sm - St).abs().max() / St.abs().max()),
        }
        t0 = time.perf_counter()
        np.linalg.eigh((Gm / (N - 1)).cpu().numpy())
        host_eigh_s = time.perf_counter() - t0
        del Gm, Gt, Sm, St
        peaks = {name: peak_mib(fn) for name, fn in legs.items()}  # also the warm-up of every leg
        times = {name: [] for name in legs}
        for _ in range(args.blocks):
            for name, fn in legs.items():
                times[name].append(timed(fn, calls))
        ms = {name: dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in times.items()}
        line = dict(tool="pca_timing", N=N, P=P, k=k, views=2, scale=True, blocks=args.blocks, calls=calls,
                    device=torch.cuda.get_device_name(0), matrix_mib=round(N * P * 4 / 2**20, 1),
                    gram_groups=o.pca_gram_groups(N, P), gram_workspace_mib=round(o.pca_gram_workspace(N, P, 2) / 2**20, 1),
                    ms=ms, peak_mib={name: round(v, 1) for name, v in peaks.items()}, host_eigh_s=round(host_eigh_s, 3),
                    gram_share_of_78_6_tf=N * P * (P + 1) / (ms["entry_gram"]["median"] * 1e-3) / MFMA_F64_FLOPS,
                    project_share_of_8_tb_s=N * P * 4 / (ms["entry_project"]["median"] * 1e-3) / HBM_BYTES_PER_S,
                    speedup_over_torch={"gram": ms["torch_gram"]["median"] / ms["entry_gram"]["median"],
                                        "project": ms["torch_project"]["median"] / ms["entry_project"]["median"]},
                    agree=agree)
        if res is not None:
            line["whole_call"] = dict(n_iter=res.n_iter, converged=res.converged, max_residual=float(res.residual.max()),
                                      ratio_sum=float(res.explained_variance_ratio.sum()))
        print(json.dumps(line))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del Y, legs, res, comp, mean, inv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
