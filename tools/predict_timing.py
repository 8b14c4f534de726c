"""Time predict() against the draw-and-average route it replaces.

Route A (what the reference class allows): forward(prediction_mode=True, S) + mean(0) and var(0) of the draws.
Route B: predict(..., Y=...) at the default chunking and at the chunk sizes given with --chunks.
One process, device events around synchronised work, every shape warmed up first, the routes alternating in blocks
(median and min-max over the blocks are reported).  Also: peak allocated bytes of each route and the Monte-Carlo error
route A's S-draw average carries against F_mean with the same warp draws (RMS over entries).

  python tools/predict_timing.py                      # BASELINE config 2's size: 2 x 10 000 spots, 50 outputs, M = 200
  python tools/predict_timing.py --side 316           # config 5's row count (2 x 99 856), 50 outputs
  python tools/predict_timing.py --once               # one predict() call, for rocprofv3 --kernel-trace --stats
  python tools/predict_timing.py --counts             # the counts leg: scale="response" on a Poisson model, see below
--counts times three calls in alternating blocks: the Gaussian call with Y (route B), predict(scale="response",
log_offset=...) of the same model with likelihood "poisson" with Y (counts/Y: B + the quadrature of
gpsa_predict_counts_f32), and the same without Y (counts: B + the counts' moments alone).  Like the other legs it only
appends its line to --out; the README row and docs/LAB_NOTES.md are brought up to date from that line by hand.
Appends one JSON line per run to --out (default profiles/predict_timing.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_alignment_amd as gp  # noqa: E402
from spatial_alignment_amd.predict import DEFAULT_WORKSPACE_GB, rows_for_budget  # noqa: E402
from spatial_alignment_amd.synthetic import make_grid_problem  # noqa: E402


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--outputs", type=int, default=50)
    ap.add_argument("--m", type=int, default=200)
    ap.add_argument("--S", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per block")
    ap.add_argument("--chunks", default="2000,5000", help="rows_per_chunk values next to the default")
    ap.add_argument("--skip-a", action="store_true", help="do not run route A (its two [S, N, L] tensors do not fit)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--counts", action="store_true", help="time the counts leg (scale='response') next to route B")
    ap.add_argument("--out", default=os.path.join("profiles", "predict_timing.jsonl"))
    args = ap.parse_args()

    dev = "cuda:0"
    mod = "expression"
    dd = make_grid_problem(side=args.side, n_views=2, n_outputs=args.outputs, device=dev, compute_device=dev)
    torch.manual_seed(0)
    model = gp.VariationalGPSA(dd, m_X_per_view=args.m, m_G=args.m, data_init=True, n_latent_gps={mod: None},
                               fixed_view_idx=None).to(dev)
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    X, Y = {mod: dd[mod]["spatial_coords"]}, {mod: dd[mod]["outputs"]}
    N, S, L = int(Ns[mod]), args.S, args.outputs
    gen = torch.Generator(device=dev).manual_seed(1)
    eps_G = [torch.randn(S, N // 2, 2, device=dev, generator=gen) for _ in range(2)]

    def route_b(c=None):
        return model.predict(X, view_idx, Ns, S=S, eps_G=eps_G, Y=Y, rows_per_chunk=c)

    if args.counts:
        Yc = {mod: torch.floor(torch.exp(torch.clamp(Y[mod], max=3.0)))}
        off = {mod: 0.25 * torch.sin(torch.arange(N, dtype=torch.float32, device=dev))}

        def counts(with_y):
            model.likelihood = "poisson"
            try:
                return model.predict(X, view_idx, Ns, S=S, eps_G=eps_G, Y=Yc if with_y else None, scale="response",
                                     log_offset=off)
            finally:
                model.likelihood = "gaussian"

        routes = {"B": route_b, "counts/Y": lambda: counts(True), "counts": lambda: counts(False)}
        for fn in routes.values():
            fn()
            fn()
        times = {k: [] for k in routes}
        for _ in range(args.blocks):
            for k, fn in routes.items():
                times[k].append(timed(fn, args.calls))
        rec = dict(tool="predict_timing", leg="counts", side=args.side, N=N, outputs=L, M=args.m, S=S, blocks=args.blocks,
                   calls_per_block=args.calls, exponentials_per_call=(9 + 40 + 3) * S * N * L,
                   ms={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()})
        line = json.dumps(rec)
        print(line)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        return

    if args.once:
        route_b()
        route_b()
        torch.cuda.synchronize()
        return

    def route_a():
        model.inject_noise(eps_G, None, None)
        with torch.no_grad():
            F = model.forward(X, view_idx=view_idx, Ns=Ns, S=S, prediction_mode=True)[3][mod]
        return F.mean(0), F.var(0)

    chunks = [None] + [int(c) for c in args.chunks.split(",") if c]
    routes = {} if args.skip_a else {"A": route_a}
    for c in chunks:
        routes["B" if c is None else f"B/{c}"] = (lambda c=c: route_b(c))
    for fn in routes.values():  # warm-up of every shape
        fn()
        fn()
    times = {k: [] for k in routes}
    for _ in range(args.blocks):  # alternating blocks
        for k, fn in routes.items():
            times[k].append(timed(fn, args.calls))
    peaks = {k: peak_of(fn) for k, fn in routes.items()}
    rec = dict(tool="predict_timing", side=args.side, N=N, outputs=L, M=args.m, S=S, blocks=args.blocks,
               calls_per_block=args.calls, default_workspace_gb=DEFAULT_WORKSPACE_GB,
               default_rows_per_chunk=rows_for_budget(DEFAULT_WORKSPACE_GB, S, args.m, L, 2),
               one_SNL_tensor_bytes=S * N * L * 4,
               closing_kernel_bytes=2 * L * S * N * 4 + 2 * N * L * 4,
               ms={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()},
               peak_bytes=peaks)
    if not args.skip_a:
        Fa = route_a()[0].double()
        Fb = route_b()[mod].F_mean.double()
        rec["mc_rms_error_of_A"] = float((Fa - Fb).pow(2).mean().sqrt())
        rec["rms_of_F_mean"] = float(Fb.pow(2).mean().sqrt())
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
