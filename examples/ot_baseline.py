"""GPSA next to the optimal-transport baseline, on the device.

The simulated lattice of examples/alignment_score.py: two views of a 20 x 20 lattice observing the same 10 outputs, view 1
warped.  Three sets of coordinates are scored by the same number - each view's outputs predicted from the OTHER view's
spots by 10-nearest-neighbour regression (``alignment_score``):

* the raw coordinates;
* the coordinates of ``paste_baseline``: consecutive views coupled by ``ot_align`` (entropic fused Gromov-Wasserstein, the
  problem PASTE poses; NOT PASTE's solver - see spatial_alignment_amd/ot.py) and stacked by ``stack_slices`` (PASTE's
  rigid Procrustes step).  The outputs here are Gaussian, not counts, so the expression cost is "euclidean";
* GPSA's aligned coordinates after ``fit``.

A rigid stacking cannot undo a nonlinear warp; GPSA can.  That is the comparison the reference's experiments print
(experiments/expression/st/st_alignment_synthetic_warp.py:121-125).
usage: python examples/ot_baseline.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import alignment_score, ot_align, paste_baseline, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
dev = torch.device("cuda:0")
X, Y, nsl, _ = simulate.generate_twod_data(2, 10, 20, noise_variance=0.01, fixed_view_idx=0, seed=0)
n = int(nsl[0])
dd = simulate.as_data_dict(X, Y, nsl)
model = make_model(dd, m=25, fixed_view_idx=0, device=dev)
dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}
mod = model.modality_names[0]
Xd, Yd = dd[mod]["spatial_coords"], dd[mod]["outputs"]

res = ot_align(Xd[:n], Yd[:n], Xd[n:], Yd[n:], alpha=0.1, dissimilarity="euclidean")
print(f"ot_align: objective {res.objective:.4g} (expression {res.expression_cost:.4g}, GW {res.gw_cost:.4g}), "
      f"epsilon used {res.epsilon_used:.3g}, marginal error {res.marginal_error:.1e}, last plan change {res.plan_change:.1e}")
stacked = paste_baseline(Xd, Yd, nsl, alpha=0.1, dissimilarity="euclidean")

fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)
s_gpsa = model.alignment_score({mod: Xd}, {mod: Yd}, k=10)[mod]
s_ot = alignment_score(model, {mod: Xd}, {mod: Yd}, k=10, G={mod: stacked.to(Xd.dtype)})[mod]
for a, b in ((0, 1), (1, 0)):
    print(f"view {b} predicted from view {a}: mean R^2 {float(s_gpsa.r2_mean_raw[a, b]):.4f} at the raw coordinates, "
          f"{float(s_ot.r2_mean[a, b]):.4f} at the OT-stacked ones, {float(s_gpsa.r2_mean[a, b]):.4f} at GPSA's aligned ones")
