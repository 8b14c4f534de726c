"""Minibatch (stochastic variational) training step time on a simulated Slide-seq-scale problem: BASELINE config 5's
size (2 views x 99 856 spots, 1000 outputs, M = 1000, S = 1), B rows per view drawn on the device at every step
(minibatch.RowSampler), train.train_step on the batch.  One JSON line per batch size; --graphed also times the step
captured with its draw (train.GraphedTrainStep(..., sampler=...)).
usage: python tools/minibatch_timing.py [--batch 2000 5000 10000] [--steps 20] [--warmup 3] [--graphed] [--out F]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=316)
ap.add_argument("--outputs", type=int, default=1000)
ap.add_argument("--M", type=int, default=1000)
ap.add_argument("--S", type=int, default=1)
ap.add_argument("--batch", type=int, nargs="+", default=[2000, 5000, 10000])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--graphed", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

ge.build()
from spatial_alignment_amd.minibatch import RowSampler  # noqa: E402
from spatial_alignment_amd.optim import FusedAdam  # noqa: E402
from spatial_alignment_amd.synthetic import make_grid_problem, make_model  # noqa: E402
from spatial_alignment_amd.train import GraphedTrainStep, train_step  # noqa: E402

dev = torch.device("cuda:0")
dd_cpu = make_grid_problem(side=args.side, n_views=2, n_outputs=args.outputs, device="cpu", compute_device=dev)
model = make_model(dd_cpu, m=args.M, device=dev)
dd = {m: {"spatial_coords": d["spatial_coords"].to(dev), "outputs": d["outputs"].to(dev),
          "n_samples_list": d["n_samples_list"]} for m, d in dd_cpu.items()}
opt = FusedAdam(list(model.parameters()), lr=1e-2)
vi, Ns, _, _ = model.create_view_idx_dict(dd)
lines = []


def timed(step):
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(args.steps):
        loss = step()
    ev1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    return ev0.elapsed_time(ev1) / args.steps, wall, float(loss)


for B in args.batch:
    sampler = RowSampler(model, dd, B, seed=0)
    gpu_ms, wall_ms, loss = timed(lambda: train_step(model, opt, dd, vi, Ns, S=args.S, sampler=sampler))
    rec = dict(mode="eager", views=2, spots_per_view=args.side ** 2, outputs=args.outputs, M=args.M, S=args.S,
               batch_per_view=B, steps=args.steps, ms_per_step=round(wall_ms, 3), gpu_ms_per_step=round(gpu_ms, 3),
               last_loss=loss)
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if args.graphed:
        g = GraphedTrainStep(model, opt, dd, vi, Ns, S=args.S, sampler=sampler)
        gpu_ms, wall_ms, loss = timed(g.step)
        g.check()
        rec = dict(rec, mode="graphed", ms_per_step=round(wall_ms, 3), gpu_ms_per_step=round(gpu_ms, 3), last_loss=loss)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del g
    model.release_arenas()
    torch.cuda.empty_cache()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
