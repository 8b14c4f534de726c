"""Full-batch against minibatch (stochastic variational) training on a simulated lattice.

Two warped views of a 40 x 40 lattice (simulate.generate_twod_data); the same model trained with the full negative ELBO
and with 200 rows per view per step (train.fit(batch_size=...)); both are then scored on the FULL data with the same
draws, and by how close the two views' aligned coordinates come (tools/soak.py's measure).
usage: python examples/minibatch_fit.py [steps]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda:0")
X, Y, nsl, _ = simulate.generate_twod_data(2, 10, 40, seed=0)
n, S = int(nsl[0]), 3
gen = torch.Generator().manual_seed(1)
eps = ([torch.randn(S, n, 2, generator=gen).to(dev) for _ in range(2)],
       {"expression": torch.randn(S, 2 * n, 10, generator=gen).to(dev)})


def score(model, dd):
    """(full negative ELBO with fixed draws, |view 0 - view 1| of the aligned coordinates)"""
    vi, Ns, _, _ = model.create_view_idx_dict(dd)
    X = {"expression": dd["expression"]["spatial_coords"]}
    with torch.no_grad():
        model.inject_noise(*eps)
        loss = float(model.loss_fn(dd, model.forward(X, view_idx=vi, Ns=Ns, S=S)[3]))
        G = model.forward(X, view_idx=vi, Ns=Ns, S=1, prediction_mode=True)[0]["expression"]
    model.train()
    return loss, float((G[:n] - G[n:]).norm())


for batch in (None, 200):
    dd = simulate.as_data_dict(X, Y, nsl)
    model = make_model(dd, m=25, device=dev)
    dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}
    l0, d0 = score(model, dd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit(model, dd, steps, lr=1e-2, S=S, batch_size=batch, graphed=True, sync_every=100)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3 / steps
    l1, d1 = score(model, dd)
    what = "full batch" if batch is None else f"{batch} rows per view"
    print(f"{what:>18}: {dt:.2f} ms/step; full negative ELBO {l0:.4g} -> {l1:.4g}; |view0 - view1| {d0:.3f} -> {d1:.3f}")
