"""Dispatches of a short world-1 data-parallel loop with and without the loss slot (GradAllReducer(with_loss=True)).

Run each variant under ``rocprofv3 --kernel-trace --stats`` and compare the summed kernel calls:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o plain -- python tools/loss_slot_probe.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o loss -- python tools/loss_slot_probe.py --with-loss
    python tools/loss_slot_probe.py --summarize OUT/.../plain_kernel_stats.csv OUT/.../loss_kernel_stats.csv

One process, RCCL at world 1 with ``always=True`` (the all-reduce runs as it would with more ranks).  The loss enters
the bucket inside the backward's closing kernel (gpsa_step_io.loss_dst); what the loss slot may add per step is the one
scalar copy out of the bucket (``reducer.loss``)."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(paths, steps):
    tot = []
    for path in paths:
        calls = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
        tot.append(calls)
    for name, calls in zip(paths, tot):
        print(f"{os.path.basename(name)}: {sum(calls.values())} kernel dispatches in {steps} timed + warm-up steps")
    a, b = tot
    d = sum(b.values()) - sum(a.values())
    print(f"difference: {d} dispatches over {steps} steps = {d / steps:.2f} per step")
    for k in sorted(set(a) | set(b)):
        if a.get(k, 0) != b.get(k, 0):
            print(f"  {a.get(k, 0):6d} -> {b.get(k, 0):6d}  {k[:140]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--with-loss", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--summarize", nargs=2)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.steps)
    import torch
    import torch.distributed as dist

    import __graft_entry__ as ge

    ge.build()
    from spatial_alignment_amd.optim import FusedAdam
    from spatial_alignment_amd.parallel import GradAllReducer
    from spatial_alignment_amd.synthetic import make_grid_problem, make_model
    from spatial_alignment_amd.train import train_step

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(47500 + os.getpid() % 2000))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    dd = make_grid_problem(side=20, n_views=2, n_outputs=6)
    model = make_model(dd, m=25, device=dev)
    dd = {m: {"spatial_coords": d["spatial_coords"].to(dev), "outputs": d["outputs"].to(dev),
              "n_samples_list": d["n_samples_list"]} for m, d in dd.items()}
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    opt = FusedAdam(model.parameters(), lr=1e-2)
    r = GradAllReducer(model.parameters(), always=True, with_loss=a.with_loss)
    torch.manual_seed(0)
    trace = []
    for _ in range(a.steps):
        train_step(model, opt, dd, view_idx, Ns, S=3, reducer=r)
        if a.with_loss:
            trace.append(r.loss)
    torch.cuda.synchronize()
    print("with_loss" if a.with_loss else "plain", a.steps, "steps",
          f"last loss {float(trace[-1]):.6f}" if trace else "")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
