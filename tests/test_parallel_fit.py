"""parallel.fit - the one-call data-parallel training loop - and what it rests on: the loss riding the gradient
all-reduce (GradAllReducer(with_loss=True)) and train.fit(reducer=...).  World 2 over gloo on the CPU (fake backend);
tests/test_parallel_fit_gpu.py runs the same worker through the real HIP path."""
import os
import queue
import sys
import time
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _problem(dev):
    from spatial_alignment_amd.synthetic import make_grid_problem, make_model

    if dev.type == "cpu":
        dd = make_grid_problem(side=8, n_views=2, n_outputs=3)
        return dd, make_model(dd, m=9)
    dd = make_grid_problem(side=20, n_views=2, n_outputs=6)
    model = make_model(dd, m=25, device=dev)
    dd = {m: {"spatial_coords": d["spatial_coords"].to(dev), "outputs": d["outputs"].to(dev),
              "n_samples_list": d["n_samples_list"]} for m, d in dd.items()}
    return dd, model


def _problem_outputs(dev, rank=None, world=None):
    """the full problem (rank None) or rank's output slice, its model carrying the full model's parameters (shared
    ones on rank 0 only - parallel.fit broadcasts them - and the rank's own rows / columns of the per-output ones)"""
    from spatial_alignment_amd.parallel import shard_outputs, shard_rows
    from spatial_alignment_amd.synthetic import make_grid_problem, make_model

    side, m = (8, 9) if dev.type == "cpu" else (20, 25)
    dd = make_grid_problem(side=side, n_views=2, n_outputs=4)
    full = make_model(dd, m=m)
    if rank is None:
        model, sdd = full, dd
    else:
        sdd = shard_outputs(dd, rank, world)
        model = make_model(sdd, m=m, seed=100 + rank)  # deliberately different construction RNG per rank
        lo, hi = shard_rows(4, rank, world)
        with torch.no_grad():
            for (n, p), (_, pf) in zip(model.named_parameters(), full.named_parameters()):
                if n.startswith("Omega_sqt_F_dict."):
                    p.copy_(pf[lo:hi])
                elif n.startswith("delta_F_dict."):
                    p.copy_(pf[:, lo:hi])
                elif rank == 0:
                    p.copy_(pf)
    model = model.to(dev)
    sdd = {k: {"spatial_coords": d["spatial_coords"].to(dev), "outputs": d["outputs"].to(dev),
               "n_samples_list": d["n_samples_list"]} for k, d in sdd.items()}
    return sdd, model


def _noise(n, L, S):
    gen = torch.Generator().manual_seed(11)
    return [torch.randn(S, n, 2, generator=gen) for _ in range(2)], torch.randn(S, 2 * n, L, generator=gen)


def _fit_worker(rank, world, port, q, cfg):
    """rank ``rank`` of a parallel.fit run; puts (rank, result) - or (rank, ("raised", message)) on ValueError"""
    sys.path.insert(0, HERE)
    from spatial_alignment_amd import parallel
    from spatial_alignment_amd import train as T
    from spatial_alignment_amd.util import LossNotDecreasingChecker

    dev = torch.device(cfg["device"])
    if dev.type == "cpu":
        from fake_ops import FakeOps
        from spatial_alignment_amd import ops as ops_mod

        ops_mod.set_ops(FakeOps())
    else:
        import __graft_entry__ as ge

        ge.build()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {"traces": [], "params": [], "first_eps_F": [], "partials": []}
    try:
        for run in range(cfg.get("runs", 1)):
            if cfg.get("shard") == "outputs":
                dd, model = _problem_outputs(dev, rank, world)
            else:
                dd, model = _problem(dev)
            model.fuse_elbo = cfg.get("fuse", True)
            S = cfg.get("S", 2) + (cfg.get("S_delta", 0) if rank == 1 else 0)
            n_epochs = cfg.get("n_epochs", 30) + (cfg.get("epochs_delta", 0) if rank == 1 else 0)
            draws = []
            orig_draw = model._draw

            def draw(shape, device, which="G", _orig=orig_draw, _d=draws):  # the rank's first eps_F
                e = _orig(shape, device, which)
                if which == "F" and not _d:
                    _d.append(e.detach().cpu().numpy())
                return e

            model._draw = draw
            if cfg.get("inject"):  # the full problem's draws, this rank's slice of them, at every step
                d = dd["expression"]  # (rows: the full problem - parallel.fit shards it; outputs: every row)
                n = int(d["n_samples_list"][0])
                eG, eF = _noise(n, 4 if cfg.get("shard") == "outputs" else int(d["outputs"].shape[1]), S)
                if cfg.get("shard") == "outputs":
                    lo, hi = parallel.shard_rows(4, rank, world)
                    mine = (eG, {"expression": eF[:, :, lo:hi]})
                else:
                    lo, hi = parallel.shard_rows(n, rank, world)
                    rows = torch.cat([torch.arange(lo, hi), n + torch.arange(lo, hi)])
                    mine = ([e[:, lo:hi] for e in eG], {"expression": eF[:, rows]})
                orig_fwd = model.forward

                def fwd(*a, _orig=orig_fwd, _m=model, **k):
                    _m.inject_noise(*mine)
                    return _orig(*a, **k)

                model.forward = fwd
            partials = []
            orig_step = T.train_step

            def step(*a, _orig=orig_step, _p=partials, **k):  # the rank's own (partial) loss of every step
                loss = _orig(*a, **k)
                _p.append(float(loss.detach()))
                return loss

            T.train_step = step
            ck = cfg.get("checker")
            checker = LossNotDecreasingChecker(max_epochs=n_epochs, atol=ck[0], window_size=ck[1]) if ck else None
            try:
                trace = parallel.fit(model, dd, n_epochs, shard=cfg.get("shard", "rows"), kl=cfg.get("kl", "owner"),
                                     seed=cfg.get("seed", 0), S=S, sync_every=cfg.get("sync_every", 10),
                                     checker=checker)
            finally:
                T.train_step = orig_step
            res["traces"].append(trace)
            res["partials"].append(partials)
            res["first_eps_F"].append(draws[0] if draws else None)
            res["params"].append({k: p.detach().cpu().numpy() for k, p in model.named_parameters()})
            if cfg.get("grads"):
                res["grads"] = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
        q.put((rank, res))
    except ValueError as e:
        q.put((rank, ("raised", str(e))))
    except BaseException:
        q.put((rank, ("error", traceback.format_exc())))
        raise
    finally:
        dist.destroy_process_group()


def collect(q, procs, n, timeout):
    """the workers' ``n`` results ({rank: result}); fails at once when a worker reports an error or dies without a
    result, and kills whatever is still running - a rank left waiting in a collective must not outlive the test"""
    out, deadline = {}, time.monotonic() + timeout
    try:
        while len(out) < n:
            try:
                r, res = q.get(timeout=1.0)
            except queue.Empty:
                codes = [p.exitcode for p in procs]
                assert all(c in (None, 0) for c in codes), f"a worker died without a result: exit codes {codes}"
                assert time.monotonic() < deadline, f"no result from the workers within {timeout} s"
                continue
            assert not (isinstance(res, tuple) and res[0] == "error"), f"rank {r}:\n{res[1]}"
            out[r] = res
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    assert [p.exitcode for p in procs] == [0] * len(procs)
    return out


def run_world2(cfg, port, timeout=300):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fit_worker, args=(r, 2, port, q, cfg), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    return collect(q, procs, 2, timeout)


def check_rank_consistency(out, n_epochs):
    a, b = out[0], out[1]
    assert len(a["traces"][0]) == n_epochs
    assert a["traces"][0] == b["traces"][0]  # bit-identical floats
    for k in a["params"][0]:
        assert np.array_equal(a["params"][0][k], b["params"][0][k]), k
    # every entry is the sum of the two ranks' partial losses (the all-reduce of the loss slot)
    for t, pa, pb in zip(a["traces"][0], a["partials"][0], b["partials"][0]):
        assert t == float(np.float32(pa) + np.float32(pb)), (t, pa, pb)
    assert a["partials"][0] != b["partials"][0]


def _port(base):
    return base + (os.getpid() % 2000)


@pytest.mark.parametrize("kl", ["owner", "replicated"])
def test_parallel_fit_ranks_agree(kl):
    out = run_world2(dict(device="cpu", kl=kl, n_epochs=30, sync_every=10), _port(41500) + (0 if kl == "owner" else 3))
    check_rank_consistency(out, 30)


def test_parallel_fit_output_sharded_ranks_agree():
    out = run_world2(dict(device="cpu", shard="outputs", n_epochs=12, sync_every=5), _port(41500) + 5)
    a, b = out[0], out[1]
    assert len(a["traces"][0]) == 12 and a["traces"][0] == b["traces"][0]
    for k in a["params"][0]:
        if not k.startswith(("Omega_sqt_F_dict.", "delta_F_dict.")):  # (the per-output ones are the rank's own)
            assert np.array_equal(a["params"][0][k], b["params"][0][k]), k
    for t, pa, pb in zip(a["traces"][0], a["partials"][0], b["partials"][0]):
        assert t == float(np.float32(pa) + np.float32(pb)), (t, pa, pb)


def test_parallel_fit_early_stop_is_the_same_step_everywhere():
    # atol 1e9: the checker fires as soon as it has a window (step 3), at the first sync (10 steps)
    out = run_world2(dict(device="cpu", n_epochs=30, sync_every=10, checker=(1e9, 3)), _port(41500) + 7)
    assert len(out[0]["traces"][0]) == len(out[1]["traces"][0]) == 10
    assert out[0]["traces"][0] == out[1]["traces"][0]


@pytest.mark.parametrize("what", ["epochs", "S"])
def test_parallel_fit_argument_mismatch_raises_on_every_rank(what):
    cfg = dict(device="cpu", n_epochs=3, epochs_delta=1 if what == "epochs" else 0, S_delta=1 if what == "S" else 0)
    out = run_world2(cfg, _port(41500) + (11 if what == "epochs" else 13), timeout=120)
    key = "n_epochs" if what == "epochs" else "'S'"
    for r in (0, 1):
        assert isinstance(out[r], tuple) and out[r][0] == "raised", out[r]
        assert key in out[r][1], out[r][1]


def test_parallel_fit_row_shards_draw_independent_repeatable_noise():
    out = run_world2(dict(device="cpu", n_epochs=1, runs=2, seed=4), _port(41500) + 17)
    e0, e1 = out[0]["first_eps_F"], out[1]["first_eps_F"]
    assert e0[0].shape == e1[0].shape
    assert not np.array_equal(e0[0], e1[0])  # the two shards draw different noise ...
    assert np.array_equal(e0[0], e0[1]) and np.array_equal(e1[0], e1[1])  # ... and the same again with the same seed


def test_parallel_fit_without_process_group_is_fit():
    from fake_ops import FakeOps
    from spatial_alignment_amd import ops as ops_mod
    from spatial_alignment_amd import parallel
    from spatial_alignment_amd.train import fit

    assert not dist.is_initialized()
    ops_mod.set_ops(FakeOps())
    try:
        traces = []
        for f in (fit, parallel.fit):
            dd, model = _problem(torch.device("cpu"))
            torch.manual_seed(5)
            traces.append(f(model, dd, 6, S=2, sync_every=4))
        assert traces[0] == traces[1]
    finally:
        ops_mod.set_ops(None)


def test_fit_refuses_a_reducer_it_cannot_use():
    from spatial_alignment_amd import parallel
    from spatial_alignment_amd.parallel import GradAllReducer
    from spatial_alignment_amd.train import fit

    dd, model = _problem(torch.device("cpu"))
    with pytest.raises(ValueError, match="graphed"):
        fit(model, dd, 1, graphed=True, reducer=GradAllReducer(model.parameters(), with_loss=True))
    with pytest.raises(ValueError, match="with_loss"):
        fit(model, dd, 1, reducer=GradAllReducer(model.parameters()))
    with pytest.raises(ValueError):
        parallel.fit(model, dd, 1, shard="columns")
    with pytest.raises(ValueError):
        parallel.fit(model, dd, 1, kl="half")
    r = GradAllReducer(model.parameters(), with_loss=True)
    with pytest.raises(ValueError):
        r()  # a loss-carrying reducer needs the loss
    with pytest.raises(ValueError):
        GradAllReducer(model.parameters())(torch.ones(()))


def _reducer_worker(rank, world, port, q):
    from spatial_alignment_amd.parallel import GradAllReducer

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    for i, p in enumerate(ps):
        p.grad = torch.full_like(p, float(rank + 1) * (i + 1))
    try:
        r = GradAllReducer(ps, with_loss=True)
        r(torch.tensor(0.25 + rank))
        q.put((rank, (float(r.loss), [p.grad.numpy() for p in ps], tuple(r.loss.shape))))
    except BaseException:
        q.put((rank, ("error", traceback.format_exc())))
        raise
    finally:
        dist.destroy_process_group()


def test_reducer_sums_the_loss_with_the_gradients():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port(41500) + 19
    procs = [ctx.Process(target=_reducer_worker, args=(r, 2, port, q), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    got = collect(q, procs, 2, 120)
    for r in (0, 1):
        loss, grads, shape = got[r]
        assert loss == 0.25 + 1.25 and shape == (1,)
        assert (grads[0] == 3.0).all() and grads[0].shape == (3,) and (grads[1] == 6.0).all() and grads[1].shape == (2, 2)
