"""A/B of the data GP's contraction modes at the headline size (2 views x 10 000 spots, L = 50, M = 200, S = 5): one
model, built once, stepped (forward + loss_fn + backward + Adam) in alternating blocks of fp32 and bf16x3 in ONE
process, so that clocks and thermals drift over both alike.  Prints one JSON line: per mode the median and the spread
of the blocks' ms per step, the graphics clock read after each block, and which kernels each mode's plan really ran
(plan.contraction: 1 = the fused ELBO pass, 2 = the Gram).  The bf16x3 mode's outputs and gradients against the fp64
oracle at this size and S = 5 are tests/test_contraction_x3.py::test_x3_config2_full_size_matches_fp64_oracle (the
oracle wants ~60 GB of host memory and minutes: not a timing tool's job).
    python tools/contraction_ab.py [--blocks 8] [--steps 100] [--warmup 10] [--out path]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sclk_mhz():
    """the current graphics clock of GPU 0 (rocm-smi, read only, from a child process), or None"""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: *\d+: *\((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)  # ~0.6 s per block: long against clock and scheduler noise
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from spatial_alignment_amd.optim import FusedAdam
    from spatial_alignment_amd.synthetic import make_grid_problem, make_model

    dev = "cuda:0"
    S = 5
    dd = make_grid_problem(side=100, n_views=2, n_outputs=50, device=dev)
    model = make_model(dd, m=200, device=dev, seed=0)
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    Xs = {m: dd[m]["spatial_coords"] for m in dd}
    opt = FusedAdam(model.parameters(), lr=1e-2)

    def step():
        out = model.forward(X_spatial=Xs, view_idx=view_idx, Ns=Ns, S=S)
        loss = model.loss_fn(dd, out[3])
        opt.zero_grad()
        loss.backward()
        opt.step()

    modes = ("fp32", "bf16x3")
    for mode in modes:
        model.contraction = mode
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    clk = {m: [] for m in modes}
    for b in range(args.blocks):
        for mode in (modes if b % 2 == 0 else modes[::-1]):
            model.contraction = mode
            step()  # (the first step after a switch: the other mode's plan is cached, nothing is built)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            e1.synchronize()
            ms[mode].append(e0.elapsed_time(e1) / args.steps)
            clk[mode].append(sclk_mhz())
    ran = {}
    for p in model.__dict__.get("_step_plans", {}).values():
        ran.setdefault(p.key[-1], []).append(p.contraction)
    res = {"shape": "2 views x 10000 spots, L=50, M=200, S=5", "blocks": args.blocks, "steps_per_block": args.steps}
    for m in modes:
        v = sorted(ms[m])
        res[m] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
                  "blocks_ms": [round(x, 4) for x in ms[m]], "sclk_mhz_after_blocks": clk[m], "plans": ran.get(m)}
    res["bf16x3_over_fp32"] = round(res["bf16x3"]["median_ms"] / res["fp32"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
