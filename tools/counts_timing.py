"""Time the count preprocessing (spatial_alignment_amd/counts.py over csrc/counts.hip) against the straightforward torch
route on the same device.

Y [N, P] fp32: negative binomial counts (size 3) with a per-spot depth and a per-gene level, generated on the device in
row chunks; two views of N / 2 rows.  Legs, each as the package's call and as torch ops:
  count_stats        Y.sum(dim, dtype=float64) on both axes, (Y > 0).sum on both axes, the count of invalid entries
  poisson_deviance   the margins, then sum_i xlogy(y, y) - y log_sz_i in fp64 and the closing per gene
  pearson_residuals  the margins, then the broadcast fp64 formula, clamped, cast back to fp32
  normalize_log1p    the row sums, their median, log1p(y target / rs) in fp64 cast back
  standardize_views  per view: fp64 mean / std (two-pass, torch.var_mean), (y - mean) / std cast back
  prepare_counts     2000 genes kept by deviance, "pearson", standardised (the torch leg strings the routes above together)
and the four C entries alone (ops.count_margins / count_deviance / count_transform / standardize_views), for which the bytes
each MUST move (from the shapes: N P 4 per read or write of the matrix) over the time is reported as a share of the
8.0 TB/s HBM rate of MI355X_MICROARCH.md (6.29 TB/s measured for a float4 copy there).

One process, device events around synchronised work, every leg warmed up first (which is also where its peak memory is
taken from torch's allocator statistics; the package's workspace is a torch tensor, reported separately as
package_scratch_mib; the *_mib fields are MiB, 2^20 bytes), the legs alternating in blocks; median and min-max over the blocks.

  python tools/counts_timing.py                          # 20 000 x 20 000 and 100 000 x 20 000
  python tools/counts_timing.py --shapes 8000x20000
Appends one JSON line per shape to --out (default profiles/counts_timing.jsonl).
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


def make_counts(N, P, dev, chunk=4096):
    gen = torch.Generator(device=dev).manual_seed(0)
    zi = torch.randn(N, generator=gen, device=dev)
    zg = torch.randn(P, generator=gen, device=dev)
    Y = torch.empty(N, P, device=dev)
    three = torch.full((1, 1), 3.0, device=dev)
    for a in range(0, N, chunk):
        mean = torch.exp(0.6 * zi[a: a + chunk, None] + 1.0) * torch.exp(1.2 * zg[None, :] - 0.5)
        lam = torch._standard_gamma(three.expand_as(mean).contiguous(), generator=gen) / 3.0
        Y[a: a + chunk] = torch.poisson(mean * lam, generator=gen)
    return Y


# ------------------------------------------------------------------------------------------------------------------------
# the torch route
# ------------------------------------------------------------------------------------------------------------------------
def t_stats(Y):
    pos = Y > 0
    bad = (~torch.isfinite(Y) | (Y < 0)).sum()
    return Y.sum(1, dtype=f64), Y.sum(0, dtype=f64), pos.sum(1), pos.sum(0), bad


def t_deviance(Y):
    rs, cs = Y.sum(1, dtype=f64), Y.sum(0, dtype=f64)
    lrs = torch.log(rs)
    lsz = lrs - lrs.mean()
    Yd = Y.double()
    ll_sat = (torch.xlogy(Yd, Yd) - Yd * lsz[:, None]).sum(0)
    ll_null = torch.where(cs > 0, cs * torch.log(cs.clamp_min(1.0) / torch.exp(lsz).sum()), torch.zeros_like(cs))
    return 2.0 * (ll_sat - ll_null)


def t_pearson(Y, theta=100.0):
    rs, cs = Y.sum(1, dtype=f64), Y.sum(0, dtype=f64)
    mu = rs[:, None] * cs[None, :] / rs.sum()
    z = (Y.double() - mu) / torch.sqrt(mu + mu * mu / theta)
    c = float(Y.shape[0]) ** 0.5
    return torch.nan_to_num(z).clamp_(-c, c).float()


def t_log1p(Y):
    rs = Y.sum(1, dtype=f64)
    return torch.log1p(Y.double() * (rs.median() / rs)[:, None]).float()


def t_standardize(Y, ns):
    out, a = torch.empty_like(Y), 0
    for n in ns:
        blk = Y[a: a + n].double()
        var, mean = torch.var_mean(blk, 0, unbiased=False)
        out[a: a + n] = torch.nan_to_num((blk - mean) / torch.sqrt(var), nan=0.0, posinf=0.0, neginf=0.0).float()
        a += n
    return out


def t_prepare(Y, ns, n_top):
    dev = t_deviance(Y)
    genes = torch.sort(torch.sort(dev, descending=True, stable=True).indices[:n_top]).values
    return t_standardize(t_pearson(Y[:, genes].contiguous()), ns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20000x20000", "100000x20000"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per block")
    ap.add_argument("--top", type=int, default=2000, help="genes prepare_counts keeps")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "counts_timing.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    o = E.ops()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    data = {}
    for N, P in shapes:  # every shape generated and warmed up before any is timed
        Y = make_counts(N, P, dev)
        ns = [N // 2, N - N // 2]
        st = counts.count_stats(Y)
        assert st.n_invalid == 0 and int((st.row_sum == 0).sum()) == 0
        lsz = counts.size_factors(Y, log=True)
        legs = {
            "count_stats": lambda Y=Y: counts.count_stats(Y),
            "torch_count_stats": lambda Y=Y: t_stats(Y),
            "poisson_deviance": lambda Y=Y: counts.poisson_deviance(Y),
            "torch_poisson_deviance": lambda Y=Y: t_deviance(Y),
            "pearson_residuals": lambda Y=Y: counts.pearson_residuals(Y),
            "torch_pearson_residuals": lambda Y=Y: t_pearson(Y),
            "normalize_log1p": lambda Y=Y: counts.normalize_log1p(Y),
            "torch_normalize_log1p": lambda Y=Y: t_log1p(Y),
            "standardize_views": lambda Y=Y, ns=ns: counts.standardize_views(Y, ns),
            "torch_standardize_views": lambda Y=Y, ns=ns: t_standardize(Y, ns),
            "prepare_counts": lambda Y=Y, ns=ns: counts.prepare_counts(Y, ns, n_top_genes=args.top, transform="pearson"),
            "torch_prepare_counts": lambda Y=Y, ns=ns: t_prepare(Y, ns, args.top),
            # the entries alone
            "entry_margins": lambda Y=Y: o.count_margins(Y),
            "entry_deviance": lambda Y=Y, lsz=lsz: o.count_deviance(Y, lsz),
            "entry_transform_pearson": lambda Y=Y, st=st: o.count_transform(Y, "pearson", st.row_sum, st.col_sum,
                                                                            total=st.total, theta=100.0, clip=100.0),
            "entry_standardize": lambda Y=Y, ns=ns: o.standardize_views(Y, [0, ns[0], ns[0] + ns[1]]),
        }
        agree = {
            "deviance_max_rel_diff": float(((counts.poisson_deviance(Y) - t_deviance(Y)).abs()
                                            / t_deviance(Y).abs().clamp_min(1.0)).max()),
            "pearson_max_abs_diff": float((counts.pearson_residuals(Y) - t_pearson(Y)).abs().max()),
            "standardize_max_abs_diff": float((counts.standardize_views(Y, ns).outputs - t_standardize(Y, ns)).abs().max()),
        }
        peaks = {k: peak_mib(fn) for k, fn in legs.items()}  # also the warm-up of every leg
        data[(N, P)] = (legs, peaks, agree)

    for N, P in shapes:
        legs, peaks, agree = data[(N, P)]
        times = {k: [] for k in legs}
        for _ in range(args.blocks):
            for k, fn in legs.items():
                times[k].append(timed(fn, args.calls))
        ms = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}
        mat = N * P * 4
        must_move = {"entry_margins": mat, "entry_deviance": mat + 8 * N, "entry_transform_pearson": 2 * mat + 8 * (N + P),
                     "entry_standardize": 3 * mat}
        hbm_share = {k: b / (ms[k]["median"] * 1e-3) / HBM_BYTES_PER_S for k, b in must_move.items()}
        speedup = {k: ms["torch_" + k]["median"] / ms[k]["median"] for k in legs if "torch_" + k in legs}
        line = dict(tool="counts_timing", N=N, P=P, views=2, top=args.top, blocks=args.blocks, calls=args.calls,
                    device=torch.cuda.get_device_name(0), matrix_mib=round(mat / 2**20, 1), ms=ms,
                    speedup_over_torch=speedup, peak_mib={k: round(v, 1) for k, v in peaks.items()},
                    must_move_bytes=must_move, share_of_8_tb_s=hbm_share, agree=agree,
                    package_scratch_mib=round(sum(b.numel() * b.element_size() for b in o._scratch.values()
                                                 if b is not None) / 2**20, 1))
        print(json.dumps(line))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
