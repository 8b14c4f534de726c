"""Step time of the negative binomial likelihood next to the Poisson and the Gaussian one at the headline size: 2 views x
10 000 spots, 50 outputs, M = 200, S = 5, outputs from simulate.generate_twod_data (the Gaussian blocks train on them as
they are, the Poisson and NB blocks on counts drawn from exp of them, with per-spot log offsets; the NB counts carry a
Gamma multiplier of size 2).  Gaussian, Poisson and NB blocks ALTERNATE in one process (the boxes drift by several per
cent between processes); per block: ms/step (wall and device).  Every step takes its likelihood's fused ELBO pass (the
NB one: panel_elbo_nb_kernel, then gpsa_nb_const and gpsa_elbo_loss_nb_fwd / _bwd).  One JSON line per likelihood, medians
over the blocks.  It does not compare against another build of the library.
usage: python tools/negbin_timing.py [--blocks 5] [--steps 20] [--warmup 3] [--out profiles/negbin_timing.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=100)
ap.add_argument("--outputs", type=int, default=50)
ap.add_argument("--M", type=int, default=200)
ap.add_argument("--S", type=int, default=5)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import simulate  # noqa: E402
from spatial_alignment_amd.optim import FusedAdam  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import train_step  # noqa: E402

dev = torch.device("cuda:0")
X, F, nsl, _ = simulate.generate_twod_data(2, args.outputs, args.side, noise_variance=0.01, seed=0, device=dev)
n = int(nsl[0])
gen = torch.Generator(device=dev).manual_seed(1)
off = 0.3 * torch.randn(2 * n, device=dev, generator=gen)
mu = torch.exp(F + off[:, None])
counts = torch.poisson(mu, generator=gen)
torch.manual_seed(2)  # (the Gamma sampler takes no generator argument: the device's default generator, seeded here)
lam = torch._standard_gamma(torch.full_like(mu, 2.0)) / 2.0
nb_counts = torch.poisson(mu * lam, generator=gen)
mod = "expression"
problems = {"gaussian": {mod: {"spatial_coords": X, "outputs": F.contiguous(), "n_samples_list": [n, n]}},
            "poisson": {mod: {"spatial_coords": X, "outputs": counts.contiguous(), "n_samples_list": [n, n],
                              "log_offset": off}},
            "negative_binomial": {mod: {"spatial_coords": X, "outputs": nb_counts.contiguous(), "n_samples_list": [n, n],
                             "log_offset": off}}}
state = {}
for kind, dd in problems.items():
    model = make_model(dd, m=args.M, device=dev)
    if kind != "gaussian":
        model.likelihood = kind  # (before the optimizer: an NB model's log_dispersion is a parameter)
    opt = FusedAdam(list(model.parameters()), lr=1e-3)
    vi, Ns, _, _ = model.create_view_idx_dict(dd)
    state[kind] = (model, opt, dd, vi, Ns)


def block(kind):
    model, opt, dd, vi, Ns = state[kind]
    step = lambda: train_step(model, opt, dd, vi, Ns, S=args.S)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.steps):
        loss = step()
    ev1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    assert model._cache.fuse is not None and "fused" in model._cache.fuse["state"], "the fused ELBO pass did not run"
    return wall, ev0.elapsed_time(ev1) / args.steps, float(loss)


res = {k: [] for k in state}
for _ in range(args.blocks):
    for kind in state:
        res[kind].append(block(kind))
lines = []
for kind, rows in res.items():
    med = lambda j: round(statistics.median(r[j] for r in rows), 4)
    rec = dict(likelihood=kind, views=2, spots_per_view=n, outputs=args.outputs, M=args.M, S=args.S, blocks=args.blocks, steps=args.steps,
               ms_per_step=med(0), gpu_ms_per_step=med(1), last_loss=rows[-1][2],
               ms_per_step_blocks=[round(r[0], 4) for r in rows])
    print(json.dumps(rec), flush=True)
    lines.append(rec)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
