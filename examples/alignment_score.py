"""Did the alignment get better?  Fit the grid example for a few hundred steps and score it.

Two views of a 20 x 20 lattice observing the same 10 outputs (simulate.generate_twod_data), view 1 warped, view 0 fixed
as in the reference's grid example.  After ``fit``:

* ``alignment_score``: each view's outputs predicted from the OTHER view's spots by 10-nearest-neighbour regression, at
  the native coordinates (``r2_mean_raw``) and at the aligned ones (``r2_mean``) - the number the reference prints while
  it trains (visium_alignment.py:284-293), here on the device, without sklearn;
* Moran's I of one output on the two views' pooled spots, before and after: with the views on top of each other a spot's
  neighbours from the other view carry the same signal, so the spatial autocorrelation rises;
* ``spatial_r2``: the leave-one-out self-regression R^2 per output the reference selects genes by.
usage: python examples/alignment_score.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import moran_i, simulate, spatial_r2  # noqa: E402
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

sel = spatial_r2(Xd[:n], Yd[:n], k=10)
print(f"spatial R^2 of view 0's {Yd.shape[1]} outputs (leave-one-out, k = 10): {float(sel.min()):.3f} .. {float(sel.max()):.3f}")

fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)

s = model.alignment_score({mod: Xd}, {mod: Yd}, k=10)[mod]
for a, b in ((0, 1), (1, 0)):
    print(f"view {b} predicted from view {a}: mean R^2 {float(s.r2_mean_raw[a, b]):.4f} at the native coordinates, "
          f"{float(s.r2_mean[a, b]):.4f} at the aligned ones")

aligned = torch.cat([model.warp_field(Xd[:n], 0, jacobian=False).G_mean, model.warp_field(Xd[n:], 1, jacobian=False).G_mean])
before, after = moran_i(Xd, Yd[:, :1], k=6), moran_i(aligned, Yd[:, :1], k=6)
print(f"Moran's I of output 0 on the pooled spots (k = 6): {float(before.I[0]):.4f} (z = {float(before.z[0]):.1f}) before, "
      f"{float(after.I[0]):.4f} (z = {float(after.z[0]):.1f}) after")
