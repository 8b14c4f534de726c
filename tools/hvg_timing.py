"""Time the per-view column moments and the dispersion-based gene selection (spatial_alignment_amd/counts.py over
csrc/moments.hip) against the straightforward fp64 torch route on the same device.

X [N, P] fp32: log1p of normalised counts as scanpy holds them, a share ``density`` of the entries non-zero, generated on
the device in row chunks, as a dense matrix and as the same matrix in CSR; two views of N / 2 rows.  Legs:
  column_moments / column_moments_csr     the package's call, transform="expm1" (one read of X or of its stored entries)
  torch_moments                           per view: t = expm1(X.double()), t.mean(0), t.var(0) on the dense matrix
  highly_variable_genes / _csr            the moments plus the Seurat ranking, n_top_genes = 2000
  normalize_moments                       transform="normalize" on raw counts (the row sums, then one read)
  entry_dense / entry_csr                 the C entries alone (ops.column_moments / column_moments_csr, mode "expm1"), for
                                          which the bytes each MUST move (N P 4 for the dense matrix; 8 nnz + 8 N for the
                                          CSR arrays) over the time is reported as a share of the 8.0 TB/s HBM rate of
                                          MI355X_MICROARCH.md.  The expm1 of every element runs in fp64 on the vector
                                          units, so the dense entry is not expected to reach the copy rate.

One process, device events around synchronised work, every leg warmed up first (which is also where its peak memory is
taken from torch's allocator statistics; the package's workspace is a torch tensor, reported separately as
package_scratch_mib), the legs alternating in blocks; median and min-max over the blocks.

  python tools/hvg_timing.py                          # 20 000 x 20 000 and 100 000 x 20 000 at 5 % and 1 %
  python tools/hvg_timing.py --shapes 8000x20000 --densities 0.02
Appends one JSON line per (shape, density) to --out (default profiles/hvg_timing.jsonl).
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

HBM_BYTES_PER_S = 8.0e12
f64, i64, i32 = torch.float64, torch.int64, torch.int32


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


def make_matrix(N, P, density, dev, chunk=4000):
    """-> (counts Y [N, P] fp32, X = log1p(Y target / row sum) fp32, the CSR arrays of X); every row holds a count"""
    gen = torch.Generator(device=dev).manual_seed(0)
    Y = torch.empty(N, P, device=dev)
    for a in range(0, N, chunk):
        blk = (torch.rand(min(chunk, N - a), P, device=dev, generator=gen) < density).float()
        blk *= torch.randint(1, 9, blk.shape, device=dev, generator=gen)
        blk[:, 0] = 1.0
        Y[a: a + chunk] = blk
    X = counts.normalize_log1p(Y)
    crow, cols, vals = [torch.zeros(1, dtype=i64, device=dev)], [], []
    for a in range(0, N, chunk):
        blk = X[a: a + chunk]
        nz = blk.nonzero()  # row-major: sorted by row, then by column
        crow.append(torch.cumsum(torch.bincount(nz[:, 0], minlength=blk.shape[0]), 0) + crow[-1][-1])
        cols.append(nz[:, 1].to(i32))
        vals.append(blk[nz[:, 0], nz[:, 1]])
        del nz
    return Y, X, counts.csr_counts((torch.cat(crow), torch.cat(cols), torch.cat(vals), (N, P)))


def t_moments(X, ns):
    out, a = [], 0
    for n in ns:
        t = torch.expm1(X[a: a + n].double())
        out.append((t.mean(0), t.var(0)))
        a += n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20000x20000", "100000x20000"])
    ap.add_argument("--densities", nargs="+", type=float, default=[0.05, 0.01])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per block")
    ap.add_argument("--top", type=int, default=2000, help="n_top_genes of highly_variable_genes")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "hvg_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    o = E.ops()
    for shape in args.shapes:
        N, P = (int(v) for v in shape.split("x"))
        for density in args.densities:  # one matrix at a time: the largest is 8 GB dense, twice
            Y, X, A = make_matrix(N, P, density, dev)
            ns = [N // 2, N - N // 2]
            off = [0, ns[0], N]
            legs = {
                "column_moments": lambda: counts.column_moments(X, ns, transform="expm1"),
                "column_moments_csr": lambda: counts.column_moments(A, ns, transform="expm1"),
                "torch_moments": lambda: t_moments(X, ns),
                "highly_variable_genes": lambda: counts.highly_variable_genes(X, ns, n_top_genes=args.top),
                "highly_variable_genes_csr": lambda: counts.highly_variable_genes(A, ns, n_top_genes=args.top),
                "normalize_moments": lambda: counts.column_moments(Y, ns, transform="normalize"),
                "entry_dense": lambda: o.column_moments(X, "expm1", off),
                "entry_csr": lambda: o.column_moments_csr(A.crow, A.col, A.values, N, P, "expm1", off),
            }
            ours, theirs = counts.column_moments(X, ns, transform="expm1"), t_moments(X, ns)
            sparse = counts.column_moments(A, ns, transform="expm1")
            rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1.0)).max())
            agree = {
                "mean_max_rel_diff_vs_torch": max(rel(ours.mean[v], theirs[v][0]) for v in range(2)),
                "var_max_rel_diff_vs_torch": max(rel(ours.var[v], theirs[v][1]) for v in range(2)),
                "csr_vs_dense_mean_max_rel_diff": rel(sparse.mean, ours.mean),
                "csr_vs_dense_var_max_rel_diff": rel(sparse.var, ours.var),
                "normalize_vs_expm1_mean_max_rel_diff": rel(counts.column_moments(Y, ns, transform="normalize").mean, ours.mean),
            }
            del ours, theirs, sparse
            peaks = {k: peak_mib(fn) for k, fn in legs.items()}  # also the warm-up of every leg
            times = {k: [] for k in legs}
            for _ in range(args.blocks):
                for k, fn in legs.items():
                    times[k].append(timed(fn, args.calls))
            ms = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}
            mat = N * P * 4
            must_move = {"entry_dense": mat, "entry_csr": 8 * A.nnz + 8 * N}
            hbm_share = {k: b / (ms[k]["median"] * 1e-3) / HBM_BYTES_PER_S for k, b in must_move.items()}
            speedup = {k: ms["torch_moments"]["median"] / ms[k]["median"] for k in ("column_moments", "column_moments_csr")}
            line = dict(tool="hvg_timing", N=N, P=P, density=density, nnz=A.nnz, views=2, top=args.top, blocks=args.blocks,
                        calls=args.calls, device=torch.cuda.get_device_name(0), matrix_mib=round(mat / 2**20, 1), ms=ms,
                        speedup_over_torch=speedup, peak_mib={k: round(v, 1) for k, v in peaks.items()},
                        must_move_bytes=must_move, share_of_8_tb_s=hbm_share, agree=agree,
                        package_scratch_mib=round(sum(b.numel() * b.element_size() for b in o._scratch.values()
                                                     if b is not None) / 2**20, 1))
            print(json.dumps(line))
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del Y, X, A, legs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
