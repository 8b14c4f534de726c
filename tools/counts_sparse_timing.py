"""Time the count preprocessing on a sparse (CSR) count matrix (spatial_alignment_amd/counts.py over
csrc/counts_sparse.hip) against the dense path (csrc/counts.hip) on the same matrix already densified in HBM.

The matrix: N spots x P genes, a gene stored in a spot with probability density * exp(0.8 z_g - 0.32) (z_g standard
normal: genes differ, the mean stays near ``density``), stored values 1 + Poisson(1), column 0 stored everywhere (no spot
without counts); generated on the device in row chunks, as CSR and, from the same draws, dense.  Two views of N / 2 rows.

Legs, each on the CSR (``sparse_*``) and on the dense tensor (``dense_*``):
  count_stats, poisson_deviance, prepare_counts(n_top_genes=2000, transform="pearson")
then ``csr_counts`` alone (the conversions are no-ops here: what is timed is the check kernel and its readback) and the two
host-to-device copies: the three CSR arrays against the dense fp32 matrix, from pageable host memory with
``Tensor.to(device)``.  ``route_ms`` adds the copy to the call: what a user pays who starts from host memory.

One process, device events around synchronised work, every leg warmed up first (which is also where its peak allocation
above its inputs is taken from torch's allocator statistics; the kernels' workspace is allocated by the first call and
stays, so it is reported separately as package_scratch_mib), the legs alternating in blocks; median and min-max over the
blocks.  Not measured: pinned host memory, a copy overlapped with compute, scipy's own host-side canonicalisation.

  python tools/counts_sparse_timing.py                       # 20 000 x 20 000 and 100 000 x 20 000 at 5 % and 1 %
  python tools/counts_sparse_timing.py --shapes 8000x20000 --densities 0.02
Appends one JSON line per (shape, density) to --out (default profiles/counts_sparse_timing.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_alignment_amd import counts  # noqa: E402
from spatial_alignment_amd import engine as E  # noqa: E402


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


def make_counts(N, P, density, dev, chunk=2048):
    """-> (crow int64, col int32, val fp32, Y dense fp32) on the device"""
    gen = torch.Generator(device=dev).manual_seed(0)
    p_gene = (density * torch.exp(0.8 * torch.randn(P, generator=gen, device=dev) - 0.32)).clamp_(max=1.0)
    Y = torch.empty(N, P, device=dev)
    crow, cols, vals = [torch.zeros(1, dtype=torch.int64, device=dev)], [], []
    for a in range(0, N, chunk):
        n = min(chunk, N - a)
        blk = (torch.rand(n, P, generator=gen, device=dev) < p_gene[None, :]).float()
        blk[:, 0] = 1.0
        blk *= 1.0 + torch.poisson(torch.ones(n, P, device=dev), generator=gen)
        Y[a: a + n] = blk
        nz = blk.nonzero()  # row-major: by row, then by column
        crow.append(torch.cumsum(torch.bincount(nz[:, 0], minlength=n), 0) + crow[-1][-1])
        cols.append(nz[:, 1].to(torch.int32))
        vals.append(blk[nz[:, 0], nz[:, 1]])
        del blk, nz
    return torch.cat(crow), torch.cat(cols), torch.cat(vals), Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20000x20000", "100000x20000"])
    ap.add_argument("--densities", nargs="+", type=float, default=[0.05, 0.01])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per block")
    ap.add_argument("--top", type=int, default=2000, help="genes prepare_counts keeps")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "counts_sparse_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    o = E.ops()
    for shape in args.shapes:
        N, P = (int(v) for v in shape.split("x"))
        ns = [N // 2, N - N // 2]
        for density in args.densities:
            crow, col, val, Y = make_counts(N, P, density, dev)
            A = counts.csr_counts((crow, col, val, (N, P)))
            print(f"[counts_sparse_timing] {N} x {P} at {density:g}: nnz {A.nnz}", file=sys.stderr, flush=True)
            sp, de = counts.count_stats(A), counts.count_stats(Y)
            agree = {
                "margins_equal": bool(torch.equal(sp.row_sum, de.row_sum) and torch.equal(sp.col_sum, de.col_sum)
                                      and torch.equal(sp.row_nnz, de.row_nnz) and torch.equal(sp.col_nnz, de.col_nnz)),
                "deviance_max_rel_diff": float(((counts.poisson_deviance(A) - counts.poisson_deviance(Y)).abs()
                                                / counts.poisson_deviance(Y).abs().clamp_min(1.0)).max()),
            }
            prep = dict(n_top_genes=args.top, transform="pearson")
            ra, rd = counts.prepare_counts(A, ns, **prep), counts.prepare_counts(Y, ns, **prep)
            agree["prepare_genes_equal"] = bool(torch.equal(ra.genes, rd.genes))
            agree["prepare_outputs_equal"] = bool(ra.genes.shape == rd.genes.shape and torch.equal(ra.outputs, rd.outputs))
            del ra, rd
            host_csr = [t.cpu() for t in (crow, col, val)]
            host_dense = Y.cpu()
            legs = {
                "sparse_count_stats": lambda: counts.count_stats(A),
                "dense_count_stats": lambda: counts.count_stats(Y),
                "sparse_poisson_deviance": lambda: counts.poisson_deviance(A),
                "dense_poisson_deviance": lambda: counts.poisson_deviance(Y),
                "sparse_prepare_counts": lambda: counts.prepare_counts(A, ns, **prep),
                "dense_prepare_counts": lambda: counts.prepare_counts(Y, ns, **prep),
                "csr_counts_check": lambda: counts.csr_counts((crow, col, val, (N, P))),
                "h2d_csr": lambda: [t.to(dev) for t in host_csr],
                "h2d_dense": lambda: host_dense.to(dev),
            }
            peaks = {k: peak_mib(fn) for k, fn in legs.items()}  # also the warm-up of every leg
            print("[counts_sparse_timing] warmed up", file=sys.stderr, flush=True)
            times = {k: [] for k in legs}
            for _ in range(args.blocks):
                for k, fn in legs.items():
                    times[k].append(timed(fn, 1 if k.startswith("h2d") else args.calls))
            ms = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}
            route = {}
            for k in ("count_stats", "poisson_deviance", "prepare_counts"):
                route["sparse_" + k] = ms["h2d_csr"]["median"] + ms["csr_counts_check"]["median"] + ms["sparse_" + k]["median"]
                route["dense_" + k] = ms["h2d_dense"]["median"] + ms["dense_" + k]["median"]
            csr_bytes = sum(t.numel() * t.element_size() for t in (crow, col, val))
            line = dict(tool="counts_sparse_timing", N=N, P=P, density=density, nnz=int(col.numel()),
                        measured_density=round(col.numel() / (N * P), 5), views=2, top=args.top, blocks=args.blocks,
                        calls=args.calls, device=torch.cuda.get_device_name(0), csr_mib=round(csr_bytes / 2**20, 1),
                        dense_mib=round(N * P * 4 / 2**20, 1), ms=ms, route_ms=route,
                        peak_mib={k: round(v, 1) for k, v in peaks.items()}, agree=agree,
                        csr_workspace_mib=round(o.lib.gpsa_count_csr_workspace(N, P) / 2**20, 1),
                        dense_workspace_mib=round(o.lib.gpsa_count_workspace(N, P) / 2**20, 1),
                        package_scratch_mib=round(sum(b.numel() * b.element_size() for b in o._scratch.values()
                                                      if b is not None) / 2**20, 1))
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del crow, col, val, Y, A, host_csr, host_dense, legs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
