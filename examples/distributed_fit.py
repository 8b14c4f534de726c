"""Data-parallel training in one call per rank: spatial_alignment_amd.fit (parallel.fit) under torchrun.

    torchrun --nproc_per_node N examples/distributed_fit.py [--side 60] [--epochs 200] [--kl owner|replicated]
    torchrun --nproc_per_node 2 examples/distributed_fit.py --one-device    # every rank on cuda:0 over gloo

Every rank builds the same problem and model from the FULL data (a simulated lattice of ``side`` x ``side`` spots per
view) and calls ``fit``: it broadcasts rank 0's parameters, keeps this rank's rows of every view, draws this rank's noise
from generators seeded by (seed, rank), and sums every step's loss with the gradients in one all-reduce - every rank
prints the same trace.  RCCL (backend nccl) with one GPU per rank; ``--one-device`` puts every rank on cuda:0 and the
collectives on gloo (RCCL refuses two ranks on one device), for a box with one GPU.
Needs the HIP library (python -c "import __graft_entry__ as g; g.build()") and an MI355X."""
import argparse
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spatial_alignment_amd as gp  # noqa: E402
from spatial_alignment_amd.synthetic import make_grid_problem, make_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=60, help="spots per view: side x side")
    ap.add_argument("--outputs", type=int, default=20)
    ap.add_argument("--inducing", type=int, default=49)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--kl", default="owner", choices=["owner", "replicated"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--one-device", action="store_true", help="every rank on cuda:0, collectives over gloo")
    args = ap.parse_args()

    local = 0 if args.one_device else int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    if args.one_device:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=dev)
    rank, world = dist.get_rank(), dist.get_world_size()

    data = make_grid_problem(side=args.side, n_views=2, n_outputs=args.outputs)
    model = make_model(data, m=args.inducing, device=dev)
    data = {m: {"spatial_coords": d["spatial_coords"].to(dev), "outputs": d["outputs"].to(dev),
                "n_samples_list": d["n_samples_list"]} for m, d in data.items()}
    checker = gp.LossNotDecreasingChecker(max_epochs=args.epochs, atol=1e-4)
    t0 = time.perf_counter()
    trace = gp.fit(model, data, args.epochs, shard="rows", kl=args.kl, seed=args.seed, lr=1e-2, S=3,
                   sync_every=10, checker=checker)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"rank {rank}/{world}: {len(trace)} steps in {dt:.2f} s, loss {trace[0]:.1f} -> {trace[-1]:.1f}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
