"""Hold out a tenth of one view's spots, fit, predict them, and impute on a grid in the common coordinate system.

Two warped views of a 30 x 30 lattice (simulate.generate_twod_data).  A tenth of the second view's spots is left out of
training; after ``fit`` their expression is predicted in closed form (``predict``: posterior mean and variance over S
warp samples, held-out log predictive density) and the expression is imputed on a regular grid through ``G_test``.
usage: python examples/predict_heldout.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import predict, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda:0")
mod = "expression"
X, Y, nsl, _ = simulate.generate_twod_data(2, 10, 30, noise_variance=0.01, seed=0)
n = int(nsl[0])
held = torch.randperm(n, generator=torch.Generator().manual_seed(1))[: n // 10] + n  # rows of view 1
keep = torch.ones(2 * n, dtype=torch.bool)
keep[held] = False

# train on what is left: view 0 in full, nine tenths of view 1
dd = simulate.as_data_dict(X[keep], Y[keep], [n, n - len(held)])
model = make_model(dd, m=25, device=dev)
dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}
fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)

# the held-out spots belong to view 1: align and predict them as rows of that view (view 0 gets no rows here)
view_idx = {mod: [torch.arange(0), torch.arange(len(held))]}
out = predict(model, {mod: X[held].to(dev)}, view_idx, {mod: len(held)}, S=10, Y={mod: Y[held].to(dev)},
              include_noise=True, generator=torch.Generator(device=dev).manual_seed(2))[mod]
mse = float((out.F_mean.cpu() - Y[held]).pow(2).mean())
print(f"held-out spots: {len(held)}; MSE of F_mean {mse:.4f} (outputs have unit scale); "
      f"mean predictive variance {float(out.F_var.mean()):.4f}; mean lpd per spot {float(out.lpd.mean()):.3f}")

# imputation on a grid of the aligned coordinate system: no training row is evaluated
grid = simulate.lattice_2d(50, device=dev)
imp = predict(model, G_test={mod: grid})[mod]
print(f"imputed {tuple(imp.F_mean.shape)} on a 50 x 50 grid; predictive sd between "
      f"{float(imp.F_var.min().sqrt()):.3f} and {float(imp.F_var.max().sqrt()):.3f}")
