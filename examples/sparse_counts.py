"""From a sparse count matrix to a negative binomial fit without ever building the dense matrix.

Two warped views of a 30 x 30 lattice (simulate.generate_twod_data).  10 of 400 genes carry the spatial signal (their log
means are draws of the simulator's GP); the other 390 are sparse noise genes, stored in 3 % of the spots.  The matrix is
assembled as CSR - the way Slide-seq or Visium counts arrive from ``scipy.sparse.load_npz`` - and goes through

    csr_counts  ->  prepare_counts(transform="counts")  ->  fit with model.likelihood = "negative_binomial"

``prepare_counts`` ranks the genes by Poisson deviance on the CSR arrays, keeps the top 10 and returns them as a dense
[N, 10] block together with the log size factors (``log_offset``).  It prints which genes were selected and the loss at
the start and at the end of a short fit.
usage: python examples/sparse_counts.py [steps]"""
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
P_signal, P = 10, 400
X, Fl, nsl, _ = simulate.generate_twod_data(2, P_signal, 30, noise_variance=0.0, seed=0)
n = int(nsl[0])
N = 2 * n
gen = torch.Generator().manual_seed(1)
depth = 0.5 * torch.randn(N, generator=gen) + 1.0
signal_genes = torch.sort(torch.randperm(P, generator=gen)[:P_signal]).values
Y = (torch.rand(N, P, generator=gen) < 0.03).float() * (1.0 + torch.poisson(torch.ones(N, P), generator=gen))
Y[:, signal_genes] = torch.poisson(torch.exp(1.5 * Fl + depth[:, None]), generator=gen)

# the CSR arrays, as a file of counts would hold them
nz = Y.nonzero()
crow = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(nz[:, 0], minlength=N), 0)])
csr = gp.csr_counts((crow.to(dev), nz[:, 1].to(torch.int32).to(dev), Y[nz[:, 0], nz[:, 1]].to(dev), (N, P)))
print(f"{csr}: {csr.nnz / (N * P) * 100:.1f} % of {N} x {P} stored")

res = gp.prepare_counts(csr, [n, n], min_counts=1, n_top_genes=P_signal, transform="counts")
found = sorted(set(res.genes.tolist()) & set(signal_genes.tolist()))
print(f"kept {res.outputs.shape[0]} of {N} spots and genes {res.genes.tolist()}: {len(found)} of the {P_signal} signal genes")

rows = res.rows.cpu()
dd = simulate.as_data_dict(X[rows], res.outputs, res.n_samples_list)
dd[mod]["log_offset"] = res.log_offset
dd = {m: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for m, d in dd.items()}
model = make_model(dd, m=25, device=dev)
model.likelihood = "negative_binomial"  # before fit builds its optimizer
trace = fit(model, dd, steps, lr=1e-2, S=3, sync_every=50)
print(f"negative ELBO: {trace[0]:.1f} -> {trace[-1]:.1f} over {len(trace)} steps")
print("dispersion r per kept gene:", [round(float(v), 2) for v in torch.exp(model.log_dispersion[mod].detach().cpu())])
