"""Highly variable genes the way the reference's real-data scripts select them, on the device.

Two warped views of a 30 x 30 lattice (simulate.generate_twod_data).  10 of 400 genes carry the spatial signal (their log
means are draws of the simulator's GP); the other 390 are flat noise genes.  The raw counts go through

    prepare_counts(selection="seurat", transform="log1p")   filter_cells / filter_genes / normalize_total / log1p /
                                                            highly_variable_genes(flavor="seurat", subset=True)
    column_moments(outputs, n_samples_list)                 the per-slice "remove genes with low variance" filter
    fit                                                     a short Gaussian fit on what is left

``prepare_counts`` ranks the genes by normalised dispersion, pooled over the kept spots and computed straight from the raw
counts (no normalised N x P matrix exists); ``column_moments`` gives the variance of every kept gene inside each view in
one read.  It prints which genes were selected at each stage and the loss at the start and at the end of the fit.
usage: python examples/variable_genes.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
import spatial_alignment_amd as gp  # noqa: E402
from spatial_alignment_amd import simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda:0")
mod = "expression"
P_signal, P, n_top = 10, 400, 20
X, Fl, nsl, _ = simulate.generate_twod_data(2, P_signal, 30, noise_variance=0.0, seed=0)
n = int(nsl[0])
N = 2 * n
gen = torch.Generator().manual_seed(1)
depth = 0.5 * torch.randn(N, generator=gen) + 1.0
signal_genes = torch.sort(torch.randperm(P, generator=gen)[:P_signal]).values
level = torch.randn(P, generator=gen) - 0.5
Y = torch.poisson(torch.exp(level[None, :] + depth[:, None]), generator=gen)  # flat genes: Poisson noise around a level
Y[:, signal_genes] = torch.poisson(torch.exp(1.5 * Fl + depth[:, None]), generator=gen)
Y = Y.to(dev)

# steps 1-5 of the scripts' process_data in one call: the selection is scanpy's Seurat flavour
res = gp.prepare_counts(Y, [n, n], min_counts=1, min_cells=10, n_top_genes=n_top, transform="log1p", standardize=False,
                        selection="seurat")
found = sorted(set(res.genes.tolist()) & set(signal_genes.tolist()))
print(f"kept {res.outputs.shape[0]} of {N} spots and {res.genes.numel()} genes by normalised dispersion: "
      f"{len(found)} of the {P_signal} signal genes among them")

# the per-slice variance filter: a gene stays if its variance exceeds 0.1 in BOTH views
mom = gp.column_moments(res.outputs, res.n_samples_list)
varying = (mom.var > 0.1).all(0)
genes = res.genes[varying]
found = sorted(set(genes.tolist()) & set(signal_genes.tolist()))
print(f"variance > 0.1 in both views: {int(varying.sum())} genes left, {len(found)} of the {P_signal} signal genes")

outputs = gp.standardize_views(res.outputs[:, varying].contiguous(), res.n_samples_list).outputs
rows = res.rows.cpu()
dd = simulate.as_data_dict(X[rows], outputs.cpu(), res.n_samples_list)
dd = {m: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for m, d in dd.items()}
model = make_model(dd, m=25, device=dev)
trace = fit(model, dd, steps, lr=1e-2, S=3, sync_every=50)
print(f"negative ELBO: {trace[0]:.1f} -> {trace[-1]:.1f} over {len(trace)} steps")
