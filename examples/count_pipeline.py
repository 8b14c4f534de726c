"""From a raw count matrix to a fit, both ways: ``prepare_counts`` into a negative binomial fit and into a Gaussian fit.

Two warped views of a 24 x 24 lattice (simulate.generate_twod_data) whose outputs are read as log means of 30 genes; spot n
has a depth exp(o[n]) and y[n, p] ~ NB(mean exp(f[n, p] + o[n]), size 3).  Ten further genes are pure noise at a low
level, and a few spots are emptied.  Then, on the device:

* ``prepare_counts(transform="counts")``: empty spots out, the 20 genes with the largest Poisson deviance, the counts
  untouched plus ``log_offset`` (log size factors) - the pair ``model.likelihood = "negative_binomial"`` takes;
* ``prepare_counts(transform="pearson")``: the same rows and genes as analytic Pearson residuals, z-scored per view - the
  outputs of a Gaussian fit.

For each fit it prints the cross-view kNN R^2 (``alignment_score``) of the standardised residuals at the native coordinates
(before) and at the aligned ones (after).
usage: python examples/count_pipeline.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import prepare_counts, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
dev = torch.device("cuda:0")
mod = "expression"
X, Fl, nsl, _ = simulate.generate_twod_data(2, 30, 24, noise_variance=0.0, fixed_view_idx=0, seed=0)
n = int(nsl[0])
gen = torch.Generator().manual_seed(1)
o = 0.5 * torch.randn(2 * n, generator=gen) + 1.0                     # log depth per spot
mu = torch.cat([torch.exp(Fl + o[:, None]), 0.3 * torch.exp(o)[:, None].expand(2 * n, 10)], 1)
lam = torch._standard_gamma(torch.full_like(mu, 3.0), generator=gen) / 3.0
Y = torch.poisson(mu * lam, generator=gen)
Y[torch.randperm(2 * n, generator=gen)[:7]] = 0.0                     # a few spots without counts
print(f"{tuple(Y.shape)} counts, mean {float(Y.mean()):.2f}, {float((Y == 0).float().mean()) * 100:.0f} % zeros, "
      f"{int((Y.sum(1) == 0).sum())} empty spots")

Yd = Y.to(dev)
kw = dict(min_counts=1, min_cells=10, n_top_genes=20)
raw = prepare_counts(Yd, [n, n], transform="counts", **kw)
res = prepare_counts(Yd, [n, n], transform="pearson", theta=3.0, **kw)
assert torch.equal(raw.rows, res.rows) and torch.equal(raw.genes, res.genes)
print(f"kept {raw.rows.numel()} spots {raw.n_samples_list} and {raw.genes.numel()} genes, "
      f"{int((raw.genes < 30).sum())} of them among the 30 with signal; constant columns per view {res.n_constant.tolist()}")
Xk = X[raw.rows.cpu()].to(dev)


def run(outputs, likelihood, log_offset=None):
    dd = simulate.as_data_dict(Xk, outputs, raw.n_samples_list)
    if log_offset is not None:
        dd[mod]["log_offset"] = log_offset
    model = make_model(dd, m=25, fixed_view_idx=0, device=dev)
    if likelihood is not None:
        model.likelihood = likelihood  # before fit builds its optimizer
    fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)
    s = model.alignment_score({mod: Xk}, {mod: res.outputs}, k=10)[mod]
    return float(s.r2_mean_raw[0, 1]), float(s.r2_mean[0, 1])


before, after = run(raw.outputs, "negative_binomial", raw.log_offset)
print(f"negative binomial fit on the counts + log_offset: view 1 from view 0, mean R^2 {before:.4f} before, {after:.4f} after")
before, after = run(res.outputs, None)
print(f"Gaussian fit on the Pearson residuals:           view 1 from view 0, mean R^2 {before:.4f} before, {after:.4f} after")
