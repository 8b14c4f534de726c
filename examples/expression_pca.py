"""Align on a few principal components instead of on every gene.

Two views of a 20 x 20 lattice (400 spots each) observing 200 genes that are mixtures of 10 planted spatial factors
(simulate.generate_twod_data with n_latent_gps=10), view 1 warped, view 0 fixed as in the reference's grid example.

* ``expression_pca`` reduces the 200 genes to 10 components on the device (each view centred on its own means) and
  reports how much of the variance they carry;
* the model is fitted twice, on the 10 scores and on all 200 genes, with the same settings; the time per training step is
  measured over the run, and each fit is scored by ``alignment_score`` ON THE 200 GENES: each view's genes predicted from
  the other view's spots by 10-nearest-neighbour regression at the aligned coordinates, mean R^2 over the genes;
* the 10-component fit's scores are mapped back to genes with ``inverse_transform`` and compared with the data.
The numbers are printed, not asserted.
usage: python examples/expression_pca.py [steps]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import expression_pca, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
dev = torch.device("cuda:0")
X, Y, nsl, _ = simulate.generate_twod_data(2, 200, 20, n_latent_gps=10, noise_variance=0.01, fixed_view_idx=0, seed=0)
ns = [int(n) for n in nsl]
Yd = Y.to(dev, torch.float32).contiguous()

res = expression_pca(Yd, ns, n_components=10, center="view")
scores = res.transform(Yd, ns)
back = res.inverse_transform(scores, ns)
print(f"expression_pca: {Yd.shape[1]} genes -> {scores.shape[1]} components carrying "
      f"{float(res.explained_variance_ratio.sum()):.4f} of the variance (converged {res.converged} after {res.n_iter} "
      f"iterations, largest residual {float(res.residual.max()):.2e}); genes rebuilt from the scores: RMS error "
      f"{float((back - Yd).square().mean().sqrt()):.4f} against a gene RMS of {float(Yd.square().mean().sqrt()):.4f}")

for label, outputs in (("10 components", scores.cpu()), ("200 genes", Y)):
    dd = simulate.as_data_dict(X, outputs.to(X.dtype), nsl)
    model = make_model(dd, m=25, fixed_view_idx=0, device=dev)
    dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}
    mod = model.modality_names[0]
    fit(model, dd, 5, lr=1e-2, S=3, sync_every=100)  # plans, workspaces, the first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    sc = model.alignment_score({mod: dd[mod]["spatial_coords"]}, {mod: Yd}, k=10)[mod]
    print(f"fit on {label}: {ms:.2f} ms per step over {steps} steps; cross-view kNN R^2 on the 200 genes, view 1 from "
          f"view 0 {float(sc.r2_mean[0, 1]):.4f}, view 0 from view 1 {float(sc.r2_mean[1, 0]):.4f} (before the fit: "
          f"{float(sc.r2_mean_raw[0, 1]):.4f}, {float(sc.r2_mean_raw[1, 0]):.4f})")
