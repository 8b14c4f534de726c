"""GPU: minibatch (stochastic variational) training - the device sampler against its host restatement, eager and
captured; the per-view weighted likelihood kernels against an fp64 restatement; the exact unbiasedness of a cover of
batches; a graphed SVI step against the eager one; fit(batch_size=...) end to end."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _lib():
    import __graft_entry__ as ge

    ge.build()
    from spatial_alignment_amd import minibatch as MB
    from spatial_alignment_amd import torch_ops  # noqa: F401  (registers torch.ops.gpsa.*)

    return MB


def _gather_case(n_views, Ns, Bs, P=(5,), D=2, seed=0):
    """inputs / outputs of torch.ops.gpsa.row_sample_gather for modalities of n_views[m] views"""
    gen = torch.Generator().manual_seed(1)
    Xs, Ys, rows, Xb, Yb, at = [], [], [], [], [], 0
    for m, nv in enumerate(n_views):
        n, b = sum(Ns[at:at + nv]), sum(Bs[at:at + nv])
        Xs.append(torch.randn(n, D, generator=gen).to(DEV))
        Ys.append(torch.randn(n, P[m], generator=gen).to(DEV))
        rows.append(torch.full((b,), -1, dtype=torch.int64, device=DEV))
        Xb.append(torch.full((b, D), float("nan"), device=DEV))
        Yb.append(torch.full((b, P[m]), float("nan"), device=DEV))
        at += nv
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    return Xs, Ys, rows, Xb, Yb, counter


def _host(MB, n_views, Ns, Bs, seed, t):
    out, at = [], 0
    for m, nv in enumerate(n_views):
        parts, off = [], 0
        for v in range(nv):
            parts.append(off + MB.batch_indices(Ns[at + v], Bs[at + v], seed, m, v, t))
            off += Ns[at + v]
        out.append(np.concatenate(parts))
        at += nv
    return out


CASES = [  # (views per modality, N per (m, v), B per (m, v), P per modality, D): B does not divide N, B = N, N = 1, two
    # modalities; rows wider than a wave (the lanes' p += 64 / d += 64 loops take a second and a third trip)
    ([5], [1, 7, 600, 1000, 37], [1, 3, 200, 1000, 5], (5,), 2),
    ([2, 3], [64, 129, 10, 11, 4099], [16, 128, 10, 2, 700], (5, 3), 2),
    ([2, 3], [64, 129, 10, 11, 300], [16, 128, 10, 2, 70], (130, 65), 3),
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("seed", [0, 2**62 + 7])
def test_sampler_matches_host_mirror(case, seed):
    MB = _lib()
    n_views, Ns, Bs, P, D = CASES[case]
    Xs, Ys, rows, Xb, Yb, counter = _gather_case(n_views, Ns, Bs, P=P, D=D)
    starts = list(range(16)) + [10**9 + 5]  # several epochs of every view, and a far step
    for t in starts:
        counter.fill_(t)
        torch.ops.gpsa.row_sample_gather(Xs, Ys, n_views, Ns, Bs, seed, counter, rows, Xb, Yb)
        want = _host(MB, n_views, Ns, Bs, seed, t)
        assert int(counter.item()) == t + 1
        for m in range(len(n_views)):
            got = rows[m].cpu().numpy()
            assert np.array_equal(got, want[m]), (t, m)
            idx = rows[m]
            assert torch.equal(Xb[m], Xs[m][idx]) and torch.equal(Yb[m], Ys[m][idx])  # bitwise copies


def test_sampler_under_graph_capture():
    MB = _lib()
    n_views, Ns, Bs, P, D = CASES[1]
    seed, t0, R = 99, 5, 7
    Xs, Ys, rows, Xb, Yb, counter = _gather_case(n_views, Ns, Bs, P=P, D=D)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.gpsa.row_sample_gather(Xs, Ys, n_views, Ns, Bs, seed, counter, rows, Xb, Yb)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        torch.ops.gpsa.row_sample_gather(Xs, Ys, n_views, Ns, Bs, seed, counter, rows, Xb, Yb)
    counter.fill_(t0)
    for r in range(R):
        g.replay()
        torch.cuda.synchronize()
        want = _host(MB, n_views, Ns, Bs, seed, t0 + r)
        for m in range(2):
            assert np.array_equal(rows[m].cpu().numpy(), want[m]), (r, m)
            assert torch.equal(Yb[m], Ys[m][rows[m]])
    assert int(counter.item()) == t0 + R


def _segment_case(n_views):
    """small views, N = 1 and N = 2 among them, 1 <= B <= N"""
    n = sum(n_views)
    Ns = [1, 2] + [3 + (5 * i) % 11 for i in range(n - 2)]
    Bs = [1, 1] + [1 + (3 * i) % N for i, N in enumerate(Ns[2:])]
    assert all(1 <= b <= N for b, N in zip(Bs, Ns)) and any(b == N for b, N in zip(Bs[2:], Ns[2:]))
    return Ns, Bs


def test_sampler_with_a_full_segment_table():
    """64 (modality, view) segments, all the table holds"""
    MB = _lib()
    n_views, seed = [33, 31], 12345
    Ns, Bs = _segment_case(n_views)
    Xs, Ys, rows, Xb, Yb, counter = _gather_case(n_views, Ns, Bs, P=(5, 3))
    for t in (0, 1, 17):
        counter.fill_(t)
        torch.ops.gpsa.row_sample_gather(Xs, Ys, n_views, Ns, Bs, seed, counter, rows, Xb, Yb)
        want = _host(MB, n_views, Ns, Bs, seed, t)
        assert int(counter.item()) == t + 1
        for m in range(2):
            assert np.array_equal(rows[m].cpu().numpy(), want[m]), (t, m)
            assert torch.equal(Xb[m], Xs[m][rows[m]]) and torch.equal(Yb[m], Ys[m][rows[m]])


def test_sampler_refuses_a_65th_segment():
    """... and one more is refused before anything is launched: rows / Xb / Yb keep their fill, the counter its step"""
    _lib()
    from spatial_alignment_amd._lib import GpsaHipError

    n_views = [33, 32]
    Ns, Bs = _segment_case(n_views)
    Xs, Ys, rows, Xb, Yb, counter = _gather_case(n_views, Ns, Bs, P=(5, 3))
    counter.fill_(17)
    with pytest.raises(GpsaHipError, match="unsupported size"):
        torch.ops.gpsa.row_sample_gather(Xs, Ys, n_views, Ns, Bs, 12345, counter, rows, Xb, Yb)
    torch.cuda.synchronize()
    assert int(counter.item()) == 17
    for m in range(2):
        assert bool((rows[m] == -1).all()) and bool(torch.isnan(Xb[m]).all()) and bool(torch.isnan(Yb[m]).all())


def _weighted_inputs():
    gen = torch.Generator().manual_seed(4)
    shapes = [(3, 50, 4), (2, 70, 6)]
    views = [[20, 30], [10, 25, 35]]
    Fs = [torch.randn(*s, generator=gen) for s in shapes]
    Ys = [torch.randn(s[1], s[2], generator=gen) for s in shapes]
    noise = torch.tensor([0.3, -0.2, 0.1, -0.4])
    ws = [torch.rand(len(v), generator=gen, dtype=torch.float64) * 3 + 0.5 for v in views]
    kl = torch.rand(7, generator=gen, dtype=torch.float64)
    return Fs, Ys, noise, views, ws, kl


def _weighted_reference(Fs, Ys, noise, views, ws, kl, kl_scale, gloss, idx):
    """fp64 torch restatement on the CPU: (loss, ll, dF, dnoise, dkl)"""
    F64 = [f.double().requires_grad_() for f in Fs]
    nz = noise.double().requires_grad_()
    k64 = kl.clone().requires_grad_()
    lls = []
    for F, Y, vs, w, j in zip(F64, Ys, views, ws, idx):
        s = torch.exp(nz[j]) + 1e-5
        lp = -0.5 * ((Y.double() - F) / s) ** 2 - torch.log(s) - 0.5 * math.log(2 * math.pi)  # [S, N, P]
        per_row = lp.sum((0, 2)) / F.shape[0]
        bounds = np.cumsum([0] + vs)
        lls.append(sum(w[v] * per_row[bounds[v]:bounds[v + 1]].sum() for v in range(len(vs))))
    loss = kl_scale * k64.sum() - sum(lls)
    loss.backward(torch.tensor(gloss, dtype=torch.float64))
    return (float(loss.detach()), [float(x) for x in lls], [f.grad for f in F64], nz.grad, k64.grad)


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64).cpu(), torch.as_tensor(b, dtype=torch.float64).cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _run_weighted(Fs, Ys, noise, views, ws, kl, kl_scale, gloss, idx):
    d = lambda t: t.to(DEV).contiguous()
    Fd, Yd, nd, wd, kd = [d(f) for f in Fs], [d(y) for y in Ys], d(noise), [d(w) for w in ws], d(kl)
    off = [int(x) for v in views for x in np.cumsum([0] + v)]
    loss = torch.empty(1, device=DEV)
    ll = torch.empty(len(Fs), dtype=torch.float64, device=DEV)
    work = torch.empty(8 * 4100 * len(Fs) + 64, dtype=torch.uint8, device=DEV)
    torch.ops.gpsa.elbo_loss_weighted_fwd(Fd, Yd, nd, idx, [len(v) for v in views], off, wd, kd, kl_scale, loss, ll,
                                          work)
    g = torch.tensor([gloss], device=DEV)
    dF = [torch.full_like(f, float("nan")) for f in Fd]
    dnoise = torch.full((4,), float("nan"), device=DEV)
    dkl = torch.empty(kl.numel(), dtype=torch.float64, device=DEV)
    torch.ops.gpsa.elbo_loss_weighted_bwd(Fd, Yd, nd, idx, [len(v) for v in views], off, wd, g, kl.numel(), kl_scale,
                                          dF, dnoise, dkl, work)
    torch.cuda.synchronize()
    return float(loss), ll.cpu().tolist(), [t.cpu() for t in dF], dnoise.cpu(), dkl.cpu()


def test_weighted_likelihood_kernels():
    _lib()
    Fs, Ys, noise, views, ws, kl = _weighted_inputs()
    idx, ks, gl = [2, 3], 0.7, 1.25  # (an upstream gradient fp32 holds exactly)
    loss, ll, dF, dn, dkl = _run_weighted(Fs, Ys, noise, views, ws, kl, ks, gl, idx)
    rl, rll, rdF, rdn, rdkl = _weighted_reference(Fs, Ys, noise, views, ws, kl, ks, gl, idx)
    assert abs(loss - rl) <= 1e-6 * abs(rl), (loss, rl)
    assert _rel(ll, rll) <= 1e-6
    for a, b in zip(dF, rdF):
        assert _rel(a, b) <= 1e-5
    assert _rel(dn, rdn) <= 1e-5 and float(dn[0]) == 0.0 and float(dn[1]) == 0.0
    assert _rel(dkl, rdkl) <= 1e-12


# one term each: views of very unequal length (9 blocks per view, all but one of them past the end of the two short
# views); 64 views, two of them empty, one that takes a second grid-stride sweep behind the 4096 / 64 block cap
UNEQUAL_VIEWS = (2, 3, [1, 1500, 20])  # S, P, rows per view
MANY_VIEWS = (3, 33, [0] + [i * 7 % 5 + 1 for i in range(30)] + [0] + [700] + [i * 3 % 5 + 1 for i in range(31)])


def _one_term_inputs(S, P, views):
    gen = torch.Generator().manual_seed(6)
    N = sum(views)
    Fs, Ys = [torch.randn(S, N, P, generator=gen)], [torch.randn(N, P, generator=gen)]
    ws = [torch.rand(len(views), generator=gen, dtype=torch.float64) * 3 + 0.5]
    _, _, noise, _, _, kl = _weighted_inputs()
    return Fs, Ys, noise, [views], ws, kl


def test_unit_weights_equal_the_unweighted_kernels():
    _lib()
    assert len(MANY_VIEWS[2]) == 64
    for inputs, idx in [(_weighted_inputs(), [2, 3]), (_one_term_inputs(*UNEQUAL_VIEWS), [2]),
                        (_one_term_inputs(*MANY_VIEWS), [3])]:
        Fs, Ys, noise, views, ws, kl = inputs
        ones = [torch.ones_like(w) for w in ws]
        ks, gl = 0.7, 1.3
        loss, ll, dF, dn, dkl = _run_weighted(Fs, Ys, noise, views, ones, kl, ks, gl, idx)
        d = lambda t: t.to(DEV).contiguous()
        Fd, Yd, nd, kd = [d(f) for f in Fs], [d(y) for y in Ys], d(noise), d(kl)
        l2 = torch.empty(1, device=DEV)
        ll2 = torch.empty(len(Fs), dtype=torch.float64, device=DEV)
        work = torch.empty(8 * 4100 * 2 + 64, dtype=torch.uint8, device=DEV)
        torch.ops.gpsa.elbo_loss_fwd(Fd, Yd, nd, idx, kd, ks, l2, ll2, work)
        dF2 = [torch.empty_like(f) for f in Fd]
        dn2 = torch.empty(4, device=DEV)
        dkl2 = torch.empty(7, dtype=torch.float64, device=DEV)
        torch.ops.gpsa.elbo_loss_bwd(Fd, Yd, nd, idx, torch.tensor([gl], device=DEV), 7, ks, dF2, dn2, dkl2, work)
        print(f"[unit weights] {len(views[0])} views: ll rel {_rel(ll, ll2):.3g}, dnoise rel {_rel(dn, dn2):.3g}")
        assert abs(loss - float(l2)) <= 1e-6 * abs(float(l2))
        assert _rel(ll, ll2) <= 1e-9
        for a, b in zip(dF, dF2):
            assert torch.equal(a, b.cpu())  # same per-element arithmetic
        assert _rel(dn, dn2) <= 1e-6 and torch.equal(dkl, dkl2.cpu())


# ---- the model ----------------------------------------------------------------------------------------------------
MODS = ("expr", "prot")
VIEWS = [600, 900]
BATCH = {"expr": [200, 150], "prot": [200, 150]}  # K = 3 and 6: a cover is lcm = 6 steps
S = 2


def _two_modality_problem():
    from spatial_alignment_amd.synthetic import make_model

    gen = torch.Generator().manual_seed(3)
    dd = {}
    for m, P in zip(MODS, (4, 5)):
        X = torch.rand(sum(VIEWS), 2, generator=gen) * 10
        dd[m] = {"spatial_coords": X, "outputs": torch.randn(sum(VIEWS), P, generator=gen),
                 "n_samples_list": list(VIEWS)}
    model = make_model(dd, m=16, n_latent_gps={"expr": None, "prot": 3}, fixed_view_idx=0, device=DEV)
    with torch.no_grad():  # away from the identity: the warp and the data GP carry gradient
        for p in model.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=gen).to(DEV))
    dd = {m: {"spatial_coords": d["spatial_coords"].to(DEV), "outputs": d["outputs"].to(DEV),
              "n_samples_list": d["n_samples_list"]} for m, d in dd.items()}
    L = {"expr": 4, "prot": 3}
    eG = {m: torch.randn(S, VIEWS[1], 2, generator=gen).to(DEV) for m in MODS}  # the free view (1), per modality
    eF = {m: torch.randn(S, sum(VIEWS), L[m], generator=gen).to(DEV) for m in MODS}
    return model, dd, eG, eF


def _step(model, dd, view_idx, Ns, eps_G, eps_F):
    model.zero_grad(set_to_none=True)
    model.inject_noise(eps_G, eps_F)
    out = model.forward({m: dd[m]["spatial_coords"] for m in MODS}, view_idx=view_idx, Ns=Ns, S=S)
    loss = model.loss_fn(dd, out[3])
    loss.backward()
    grads = {n: (p.grad.detach().double().clone() if p.grad is not None else torch.zeros_like(p, dtype=torch.float64))
             for n, p in model.named_parameters()}
    return float(loss.detach()), grads


@pytest.mark.parametrize("engine", [True, False])
def test_cover_of_batches_is_unbiased(engine):
    """the mean over a cover of batches (every row of every view equally often) of the weighted batch losses and of
    every gradient IS the full-batch step's, the per-row noise being the same draws"""
    MB = _lib()
    model, dd, eG, eF = _two_modality_problem()
    model.use_step_engine = engine
    vi, Ns, _, _ = model.create_view_idx_dict(dd)
    full_loss, full_g = _step(model, dd, vi, Ns, [torch.cat([eG[m] for m in MODS], 1)], eF)
    sampler = MB.RowSampler(model, dd, BATCH, seed=17)
    T = 6
    tot_loss, tot_g = 0.0, {n: torch.zeros_like(g) for n, g in full_g.items()}
    seen = {m: np.zeros(sum(VIEWS), dtype=int) for m in MODS}
    for t in range(T):
        b = sampler.next()
        rows = {m: b.rows[m] for m in MODS}
        host = sampler.host_rows(t)
        for m in MODS:
            assert np.array_equal(rows[m].cpu().numpy(), host[m])
            np.add.at(seen[m], host[m], 1)
        free = [torch.cat([eG[m][:, rows[m][200:] - VIEWS[0]] for m in MODS], 1)]
        l, g = _step(model, b.data_dict, b.view_idx, b.Ns, free, {m: eF[m][:, rows[m]] for m in MODS})
        tot_loss += l
        for n in tot_g:
            tot_g[n] += g[n]
    for m in MODS:  # the cover: view 0 twice, view 1 once
        assert (seen[m][:600] == 2).all() and (seen[m][600:] == 1).all()
    mean_loss = tot_loss / T
    assert abs(mean_loss - full_loss) <= 1e-5 * abs(full_loss), (mean_loss, full_loss)
    bad = {}
    for n, g in full_g.items():
        e = _rel(tot_g[n] / T, g) if float(g.abs().max()) > 0 else float((tot_g[n]).abs().max())
        if e > 1e-5:
            bad[n] = e
    assert not bad, bad


def _grid(dev=DEV, side=20, n_out=6):
    from spatial_alignment_amd.synthetic import make_grid_problem, make_model

    dd = make_grid_problem(side=side, n_views=2, n_outputs=n_out)
    model = make_model(dd, m=25, device=dev)
    dd = {m: {"spatial_coords": d["spatial_coords"].to(dev), "outputs": d["outputs"].to(dev),
              "n_samples_list": d["n_samples_list"]} for m, d in dd.items()}
    return model, dd


def test_graphed_svi_step_equals_eager():
    """the captured SVI step (draw included) does the work of the eager one: 3 warm-up steps + 1 replay land on the
    parameters of 4 eager steps over the same batches (same seed, counter 0 .. 3) and the same injected noise"""
    MB = _lib()
    from spatial_alignment_amd.optim import FusedAdam
    from spatial_alignment_amd.train import GraphedTrainStep, train_step

    B = 100
    gen = torch.Generator().manual_seed(8)
    noise = ([torch.randn(S, B, 2, generator=gen).to(DEV) for _ in range(2)],
             {"expression": torch.randn(S, 2 * B, 6, generator=gen).to(DEV)})
    res = []
    for mode in ("eager", "graph"):
        model, dd = _grid()
        opt = FusedAdam(list(model.parameters()), lr=1e-2)
        sampler = MB.RowSampler(model, dd, B, seed=21)
        vi, Ns, _, _ = model.create_view_idx_dict(dd)
        if mode == "eager":
            for _ in range(4):
                loss = train_step(model, opt, dd, vi, Ns, S, sampler=sampler, noise=noise)
        else:
            gs = GraphedTrainStep(model, opt, dd, vi, Ns, S=S, warmup=3, sampler=sampler, noise=noise)
            loss = gs.step()
            gs.check()
        torch.cuda.synchronize()
        assert int(sampler.counter.item()) == 4
        assert np.array_equal(sampler.batch.rows["expression"].cpu().numpy(), sampler.host_rows(3)["expression"])
        res.append((float(loss.detach()), {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[0][0]), (res[0][0], res[1][0])
    for k in res[0][1]:
        a, b = res[0][1][k].double(), res[1][1][k].double()
        assert (a - b).norm() <= 1e-5 * max(a.norm().item(), 1e-6), k


def _full_loss_and_distance(model, dd, eps):
    vi, Ns, _, _ = model.create_view_idx_dict(dd)
    X = {"expression": dd["expression"]["spatial_coords"]}
    with torch.no_grad():
        model.inject_noise(*eps)
        out = model.forward(X, view_idx=vi, Ns=Ns, S=S)
        loss = float(model.loss_fn(dd, out[3]))
        G = model.forward(X, view_idx=vi, Ns=Ns, S=1, prediction_mode=True)[0]["expression"]
    n = int(dd["expression"]["n_samples_list"][0])
    model.train()
    return loss, float((G[:n] - G[n:]).norm())


@pytest.mark.parametrize("graphed", [False, True])
def test_fit_minibatch_end_to_end(graphed):
    """fit(batch_size=...) on a simulate.generate_twod_data lattice lowers the full-batch loss and brings the two
    views' aligned coordinates together (tools/soak.py's measure)"""
    _lib()
    from spatial_alignment_amd import simulate
    from spatial_alignment_amd.synthetic import make_model
    from spatial_alignment_amd.train import fit

    X, Y, nsl, _ = simulate.generate_twod_data(2, 8, 20, seed=2)
    dd = simulate.as_data_dict(X, Y, nsl)
    model = make_model(dd, m=25, device=DEV)
    dd = {m: {"spatial_coords": d["spatial_coords"].to(DEV), "outputs": d["outputs"].to(DEV),
              "n_samples_list": d["n_samples_list"]} for m, d in dd.items()}
    gen = torch.Generator().manual_seed(5)
    n = int(nsl[0])
    eps = ([torch.randn(S, n, 2, generator=gen).to(DEV) for _ in range(2)],
           {"expression": torch.randn(S, 2 * n, 8, generator=gen).to(DEV)})
    l0, d0 = _full_loss_and_distance(model, dd, eps)
    x0 = float((dd["expression"]["spatial_coords"][:n] - dd["expression"]["spatial_coords"][n:]).norm())
    trace = fit(model, dd, 400, lr=1e-2, S=S, batch_size=100, sample_seed=3, graphed=graphed, sync_every=50)
    assert len(trace) == 400 and all(np.isfinite(trace))
    l1, d1 = _full_loss_and_distance(model, dd, eps)
    print(f"[minibatch fit graphed={graphed}] full loss {l0:.1f} -> {l1:.1f}; |view0 - view1| {x0:.3f} (data), "
          f"{d0:.3f} -> {d1:.3f} (aligned)")
    assert l1 < l0
    assert d1 < min(d0, x0)
