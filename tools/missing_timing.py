"""What model.skip_missing costs at the headline size (2 views x 10 000 spots, L = 50, M = 200, S = 5): one model, built
once, stepped (forward + loss_fn + backward + Adam) in alternating blocks with the flag off (complete outputs) and on (30 %
of the outputs NaN) in ONE process, as tools/contraction_ab.py does, so that clocks and thermals drift over both alike;
then the two fused kernels alone (gpsa_quadform_elbo_delta_f32 against gpsa_quadform_elbo_delta_skip_f32 on the same
operands, alternating).  Appends one JSON line to --out (default profiles/missing_timing.jsonl).
    python tools/missing_timing.py [--blocks 8] [--steps 100] [--warmup 10] [--out path]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "missing_timing.jsonl"))
    args = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build()
    from spatial_alignment_amd import _lib
    from spatial_alignment_amd.optim import FusedAdam
    from spatial_alignment_amd.synthetic import make_grid_problem, make_model

    dev = "cuda:0"
    S = 5
    dd = make_grid_problem(side=100, n_views=2, n_outputs=50, device=dev)
    model = make_model(dd, m=200, device=dev, seed=0)
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    Xs = {m: dd[m]["spatial_coords"] for m in dd}
    opt = FusedAdam(model.parameters(), lr=1e-2)
    mod = next(iter(dd))
    Y = dd[mod]["outputs"]
    miss = torch.rand(Y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.3
    data = {"off": dd, "on": {mod: dict(dd[mod], outputs=torch.where(miss, torch.full_like(Y, float("nan")), Y))}}

    def step(mode):
        model.skip_missing = mode == "on"
        out = model.forward(X_spatial=Xs, view_idx=view_idx, Ns=Ns, S=S)
        loss = model.loss_fn(data[mode], out[3])
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    modes = ("off", "on")
    for mode in modes:
        for _ in range(args.warmup):
            last = step(mode)
        assert bool(torch.isfinite(last)), mode
    ms = {m: [] for m in modes}
    for b in range(args.blocks):
        for mode in (modes if b % 2 == 0 else modes[::-1]):
            step(mode)
            ms[mode].append(timed(lambda: step(mode), args.steps))
    res = {"shape": "2 views x 10000 spots, L=50, M=200, S=5, 30 % missing with the flag on", "blocks": args.blocks,
           "steps_per_block": args.steps}
    for m in modes:
        v = sorted(ms[m])
        res[f"step_{m}"] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4),
                            "max_ms": round(v[-1], 4), "blocks_ms": [round(x, 4) for x in ms[m]]}
    res["step_on_over_off"] = round(res["step_on"]["median_ms"] / res["step_off"]["median_ms"], 4)

    # the two fused kernels alone, on the same operands
    lib = _lib.load()
    M, L, N = 200, 50, int(Y.shape[0])
    Cn = S * N
    g = torch.Generator(device=dev).manual_seed(2)
    A = torch.randn(L, M, M, device=dev, dtype=torch.float64, generator=g) / M ** 0.5
    Om = (A @ A.transpose(1, 2) * 0.2).contiguous()
    alpha = torch.randn(M, Cn, device=dev, generator=g) * 0.3
    delta = torch.randn(M, L, device=dev, generator=g)
    q = torch.rand(Cn, device=dev, dtype=torch.float64, generator=g) * 0.3
    eps = torch.randn(Cn, L, device=dev, generator=g)
    var_u, noise_u = torch.tensor([0.3], device=dev), torch.tensor([-0.4], device=dev)
    gg, dm = torch.empty(L, Cn, device=dev), torch.empty(L, Cn, device=dev)
    abar = torch.empty(M, Cn, device=dev)
    part = torch.empty(lib.gpsa_quadform_elbo_parts(), dtype=torch.float64, device=dev)
    wsb = lib.gpsa_quadform_elbo_f32_workspace(M, Cn, L)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    Ys = {"plain": Y.contiguous(), "skip": data["on"][mod]["outputs"].contiguous()}
    fns = {"plain": lib.gpsa_quadform_elbo_delta_f32, "skip": lib.gpsa_quadform_elbo_delta_skip_f32}

    def kernel(which):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = fns[which](1, p(alpha), p(Om), M, Cn, L, p(delta), p(q), p(var_u), p(eps), p(Ys[which]), N, S, p(noise_u),
                        p(gg), p(dm), p(abar), p(part), None, p(ws), wsb, st)
        assert rc == 0, rc

    kms = {k: [] for k in fns}
    for k in fns:
        for _ in range(3):
            kernel(k)
    for b in range(args.blocks):
        for k in (("plain", "skip") if b % 2 == 0 else ("skip", "plain")):
            kms[k].append(timed(lambda: kernel(k), 20))
    for k in fns:
        v = sorted(kms[k])
        res[f"kernel_{k}"] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    res["kernel_skip_over_plain"] = round(res["kernel_skip"]["median_ms"] / res["kernel_plain"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
