"""GPU: parallel.fit through the real HIP path - two ranks sharing cuda:0 over gloo (RCCL refuses two ranks on one
device) - and the step engine's loss slot (gpsa_step_io.loss_src / loss_dst) with RCCL itself at world 1."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_parallel_fit import _noise, _problem, _problem_outputs, check_rank_consistency, collect, run_world2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _port(base):
    return base + (os.getpid() % 2000)


@pytest.mark.parametrize("fuse,kl", [(False, "owner"), (True, "owner"), (False, "replicated"), (True, "replicated")])
def test_parallel_fit_ranks_agree_hip(fuse, kl):
    import __graft_entry__ as ge

    ge.build()
    port = _port(43500) + (1 if fuse else 0) + (2 if kl == "owner" else 0)
    out = run_world2(dict(device=DEV, fuse=fuse, kl=kl, n_epochs=30, sync_every=10), port, timeout=600)
    check_rank_consistency(out, 30)


def test_parallel_fit_early_stop_hip():
    import __graft_entry__ as ge

    ge.build()
    out = run_world2(dict(device=DEV, n_epochs=30, sync_every=10, checker=(1e9, 3)), _port(43500) + 5, timeout=600)
    assert len(out[0]["traces"][0]) == len(out[1]["traces"][0]) == 10
    assert out[0]["traces"][0] == out[1]["traces"][0]


def _full_step(dev, shard, S):
    """the single-process step on the full problem with the draws the ranks slice: (loss, {name: grad})"""
    if shard == "outputs":
        dd, model = _problem_outputs(dev)
        L = 4
    else:
        dd, model = _problem(dev)
        L = int(dd["expression"]["outputs"].shape[1])
    n = int(dd["expression"]["n_samples_list"][0])
    eG, eF = _noise(n, L, S)
    model.fuse_elbo = False  # (the separate kernels: the ranks take the fused ELBO pass)
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    model.inject_noise(eG, {"expression": eF})
    out = model.forward({"expression": dd["expression"]["spatial_coords"]}, view_idx, Ns, S=S)
    loss = model.loss_fn(dd, out[3])
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}


@pytest.mark.parametrize("shard,kl", [("rows", "owner"), ("rows", "replicated"), ("outputs", "owner")])
def test_parallel_fit_first_step_is_the_full_step(shard, kl):
    """the ranks' slices of one full step's draws: trace[0] is the full loss, the reduced .grad the full gradient"""
    import __graft_entry__ as ge

    ge.build()
    port = _port(43500) + 7 + {"owner": 0, "replicated": 1}[kl] + (2 if shard == "outputs" else 0)
    cfg = dict(device=DEV, shard=shard, kl=kl, n_epochs=1, S=3, inject=True, grads=True)
    out = run_world2(cfg, port, timeout=600)
    loss1, want = _full_step(torch.device(DEV), shard, 3)
    for r in (0, 1):
        t = out[r]["traces"][0]
        assert len(t) == 1 and abs(t[0] - loss1) <= 1e-5 * abs(loss1), (t, loss1)
    for k, a in want.items():
        if shard == "outputs" and k.startswith("Omega_sqt_F_dict."):
            b = np.concatenate([out[r]["grads"][k] for r in range(2)], 0)
        elif shard == "outputs" and k.startswith("delta_F_dict."):
            b = np.concatenate([out[r]["grads"][k] for r in range(2)], 1)
        else:
            b = out[0]["grads"][k]
            assert np.array_equal(b, out[1]["grads"][k]), k
        assert np.linalg.norm(a - b) <= 1e-3 * max(np.linalg.norm(a), 1e-6), (k, np.linalg.norm(a - b), np.linalg.norm(a))


def _rccl_one_rank_worker(port, q):
    """RCCL at world 1 (always=True: the reduce runs): the loss slot the engine's closing kernel fills"""
    import __graft_entry__ as ge

    ge.build()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = torch.device(DEV)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        _rccl_one_rank(dev, q)
    except BaseException:
        import traceback

        q.put((0, ("error", traceback.format_exc())))
        raise
    finally:
        dist.destroy_process_group()


def _rccl_one_rank(dev, q):
    from spatial_alignment_amd import step_engine as SE
    from spatial_alignment_amd.optim import FusedAdam
    from spatial_alignment_amd.parallel import GradAllReducer
    from spatial_alignment_amd.train import fit, train_step

    res = {}
    dd, model = _problem(dev)
    view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
    opt = FusedAdam(model.parameters(), lr=1e-2)
    r = GradAllReducer(model.parameters(), always=True, with_loss=True)
    same, written = [], []
    for _ in range(3):
        loss = train_step(model, opt, dd, view_idx, Ns, S=3, reducer=r)
        ll = SE.LAST_LOSS.get(dev.index)
        written.append(ll is not None and ll.data_ptr() == loss.data_ptr())
        same.append(loss.detach().reshape(1).cpu().numpy().tobytes() == r.loss.cpu().numpy().tobytes())
    res["same"], res["written"] = same, written
    traces = []
    for with_r in (False, True):
        dd, model = _problem(dev)
        torch.manual_seed(3)
        red = GradAllReducer(model.parameters(), always=True, with_loss=True) if with_r else None
        traces.append(fit(model, dd, 12, S=3, sync_every=5, reducer=red))
    res["traces"] = traces
    q.put((0, res))


def test_loss_slot_on_rccl_one_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_one_rank_worker, args=(_port(45500), q), daemon=True)
    p.start()
    res = collect(q, [p], 1, 600)[0]
    assert res["written"] == [True] * 3  # the engine's closing kernel filled the slot (no copy by the reducer)
    assert res["same"] == [True] * 3     # reducer.loss is the step's loss, bit for bit
    assert len(res["traces"][0]) == 12 and res["traces"][0] == res["traces"][1]


@pytest.mark.parametrize("hand_loss", [False, True])
def test_closing_kernel_writes_the_loss_slot_only_when_asked(monkeypatch, hand_loss):
    """the C ABI: with gpsa_step_io.loss_src / loss_dst set the backward's closing kernel copies the loss into the
    bucket's last float; NULL - every backward that has no reducer carrying the loss - leaves the spare room behind
    the gradients untouched.  The gradients are the same bits either way."""
    import __graft_entry__ as ge
    from spatial_alignment_amd import step_engine as SE
    from spatial_alignment_amd import torch_ops as TO

    ge.build()
    dev = torch.device(DEV)
    sentinel = -12345.5
    monkeypatch.setattr(SE, "_grad_bucket", lambda n, d: torch.full((n,), sentinel, dtype=torch.float32, device=d))
    seen = []
    stash = TO.stash

    def spy(d):
        if "og" in d:  # a backward call: what it hands the C entry point
            seen.append((d["io"].loss_src, d["io"].loss_dst))
        return stash(d)

    monkeypatch.setattr(TO, "stash", spy)
    grads = []
    for hand in (False, hand_loss):
        dd, model = _problem(dev)
        view_idx, Ns, _, _ = model.create_view_idx_dict(dd)
        n = int(dd["expression"]["n_samples_list"][0])
        eG, eF = _noise(n, 6, 3)
        model.inject_noise(eG, {"expression": eF})
        out = model.forward({"expression": dd["expression"]["spatial_coords"]}, view_idx, Ns, S=3)
        loss = model.loss_fn(dd, out[3])
        if hand:
            model.__dict__["_loss_slot"] = loss
        try:
            loss.backward()
        finally:
            model.__dict__.pop("_loss_slot", None)
        torch.cuda.synchronize()
        flat, used = SE.LAST_FLAT[dev.index], SE.LAST_USED[dev.index]
        spare = flat[used:].cpu().numpy()
        assert spare.size == 64
        if hand:
            src, dst = seen[-1]
            assert src == loss.data_ptr() and dst == flat.data_ptr() + 4 * (flat.numel() - 1)
            assert (spare[:-1] == sentinel).all()
            assert spare[-1:].tobytes() == loss.detach().reshape(1).cpu().numpy().tobytes()
        else:
            assert seen[-1] == (None, None)
            assert (spare == sentinel).all()
        grads.append(flat[:used].cpu().numpy())
    assert np.array_equal(grads[0], grads[1])
