"""Spatial autocorrelation before and after the alignment: what moransi_post_alignment.py does with squidpy, on the device.

Two views of a 20 x 20 lattice observing the same 10 outputs plus 10 columns of pure noise
(simulate.generate_twod_data), view 1 warped, view 0 fixed.  The two slices are pooled at their native coordinates and,
after a short fit, at their aligned ones; on each pooled set ``spatial_autocorr`` gives Moran's I per gene on the
symmetrised 6-nearest-neighbour graph with its analytic p-value, 100 permutations and the Benjamini-Hochberg columns.  The
figure the reference reports is the number of genes with ``pval_norm_fdr_bh < 0.01`` before and after
(visium/moransi_post_alignment.py:88-133): with the views on top of each other a spot's neighbours from the other view
carry the same signal, so I rises on the genes that have spatial structure and stays at its expectation on the noise.
usage: python examples/spatial_autocorr.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import simulate, spatial_autocorr, spatial_graph  # noqa: E402
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
genes = torch.cat([Yd, torch.randn(Yd.shape[0], 10, device=dev, generator=torch.Generator(device=dev).manual_seed(1))], 1)

fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)
aligned = torch.cat([model.warp_field(Xd[:n], 0, jacobian=False).G_mean, model.warp_field(Xd[n:], 1, jacobian=False).G_mean])

for name, coords in (("native", Xd), ("aligned", aligned)):
    g = spatial_graph(coords, k=6, symmetric="union")
    res = spatial_autocorr(g, genes, mode="moran", n_perms=100, generator=torch.Generator(device=dev).manual_seed(0))
    hits = int((res.pval_norm_fdr_bh < 0.01).sum())
    hits_sim = int((res.pval_sim_fdr_bh < 0.05).sum())
    print(f"{name:8s} coordinates: {g.nnz} edges, {int(g.n_isolated)} isolated spots; Moran's I of the 10 outputs "
          f"{float(res.I[:10].mean()):.4f} (mean), of the 10 noise columns {float(res.I[10:].mean()):+.4f}; "
          f"{hits} of {genes.shape[1]} genes with pval_norm_fdr_bh < 0.01, {hits_sim} with pval_sim_fdr_bh < 0.05 "
          f"(100 permutations: the smallest possible p is {1 / 101:.4f})")
