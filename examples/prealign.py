"""A slice that arrives turned and mirrored: fit with and without the rigid pre-registration.

Two views of a 20 x 20 lattice observing the same 10 outputs (simulate.generate_twod_data), view 1 warped, view 0 fixed
as in the reference's grid example - and then view 1 mirrored and turned by 1.45 rad about the lattice's centre, the pose
the reference's Slide-seq scripts undo by hand (``angle = 1.45``, slideseq_alignment.py:121-131).  The warp's mean starts at
the identity and its prior pulls towards it, so the fit cannot undo such a pose on its own.

* ``prealign_slices`` searches the rotation, reflection and shift that put view 1 on view 0 and reports what it found
  (angle, reflection, the score before and after, the runner-up pose);
* the model is fitted twice, on the coordinates as they arrived and on the pre-registered ones, and each fit is scored by
  ``alignment_score``: each view's outputs predicted from the OTHER view's spots by 10-nearest-neighbour regression at the
  aligned coordinates, mean R^2 over the outputs.  The numbers are printed, not asserted.
usage: python examples/prealign.py [steps]"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import prealign_slices, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
dev = torch.device("cuda:0")
X, Y, nsl, _ = simulate.generate_twod_data(2, 10, 20, noise_variance=0.01, fixed_view_idx=0, seed=0)
n = int(nsl[0])
centre = torch.tensor([5.0, 5.0], dtype=X.dtype)
c, s = math.cos(1.45), math.sin(1.45)
turned = ((X[n:] - centre) * torch.tensor([1.0, -1.0], dtype=X.dtype)) @ torch.tensor([[c, -s], [s, c]], dtype=X.dtype).T + centre
X_arrived = torch.cat([X[:n], turned])

X_pre, regs = prealign_slices(X_arrived.to(dev), Y.to(dev), nsl)
r = regs[1]
print(f"pre-registration of view 1 onto view 0: angle {r.angle:.4f} rad, reflected {r.reflected}, J {r.score_start:.4f} at the "
      f"centroid match -> {r.score_coarse:.4f} after the coarse grid -> {r.score:.4f} after {len(r.path)} refinement levels; "
      f"{r.n_matched} of {n} spots matched within {r.max_dist:.3f}; runner-up pose (angle, reflected, J): {r.runner_up}")
print(f"  RMS distance of view 1's spots from their own coordinates before the mirror and turn (those differ from view 0's "
      f"by the simulated warp, which no rigid motion removes): "
      f"{float((X_pre[n:].cpu() - X[n:].double()).square().sum(1).mean().sqrt()):.4f} (lattice spacing {10 / 19:.4f})")

for label, coords in (("as it arrived", X_arrived), ("pre-registered", X_pre.to(X.dtype).cpu())):
    dd = simulate.as_data_dict(coords, Y, nsl)
    model = make_model(dd, m=25, fixed_view_idx=0, device=dev)
    dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}
    mod = model.modality_names[0]
    fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)
    sc = model.alignment_score({mod: dd[mod]["spatial_coords"]}, {mod: dd[mod]["outputs"]}, k=10)[mod]
    print(f"{label}: after {steps} steps, cross-view kNN R^2 (mean over outputs) view 1 from view 0 "
          f"{float(sc.r2_mean[0, 1]):.4f}, view 0 from view 1 {float(sc.r2_mean[1, 0]):.4f} "
          f"(at the coordinates given to the fit: {float(sc.r2_mean_raw[0, 1]):.4f}, {float(sc.r2_mean_raw[1, 0]):.4f})")
