"""Fit the grid example, then look at the alignment itself: deformation map, folding check, the way back, transfer.

Two warped views of a 20 x 20 lattice (simulate.generate_twod_data), view 0 fixed as in the reference's grid example.
After ``fit``: the warp of view 1 on a 40 x 40 lattice with its Jacobian determinant (the local area change; ``det <= 0``
would be a fold) - what plot_slideseq_deformation_field.py draws from finite differences of scattered points, here exact
and at any points; the lattice of the common coordinate system put back on view 1 (``unwarp``); and view 1's spots in
view 0's coordinates (``transfer``), which the two views' shared lattice lets us score.
usage: python examples/warp_field.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import simulate, transfer, unwarp, warp_field  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda:0")
X, Y, nsl, _ = simulate.generate_twod_data(2, 10, 20, noise_variance=0.01, fixed_view_idx=0, seed=0)
n = int(nsl[0])
dd = simulate.as_data_dict(X, Y, nsl)
model = make_model(dd, m=25, fixed_view_idx=0, device=dev)
dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}
fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)

# the deformation map of view 1 on a lattice (no training row is evaluated) and the folding check
grid = simulate.lattice_2d(40, device=dev)
w = warp_field(model, grid, 1)
disp = (w.G_mean - grid.double()).norm(dim=1)
print(f"view 1 on a 40 x 40 lattice: displacement up to {float(disp.max()):.3f}; det J between {float(w.det.min()):.3f} "
      f"and {float(w.det.max()):.3f}; folded points: {int(w.n_folded)}")

# the way back: where the lattice of the COMMON coordinate system lies on view 1's own slice
u = unwarp(model, grid, 1)
print(f"unwarp of the lattice into view 1: {int(u.converged.sum())} of {len(grid)} points converged (tol {u.tol:.1e}); "
      f"worst residual {float(u.residual[u.converged].max()):.1e}")

# view 1's spots in view 0's coordinates; both views observe the same lattice, so spot i of view 1 should land on
# spot i of view 0 (view 0 is fixed: its coordinates ARE the common system)
X1, X0 = X[n:].to(dev), X[:n].to(dev)
t = transfer(model, X1, 1, 0)
before = float((X1 - X0).norm(dim=1).mean())
after = float((t.X - X0.double()).norm(dim=1).mean())
print(f"view 1's spots against view 0's: mean distance {before:.3f} before, {after:.3f} after transfer")
