"""Overdispersed count outputs: two warped views of a lattice whose outputs are negative binomial counts with a known
dispersion per output.

Two warped views of a 30 x 30 lattice (simulate.generate_twod_data).  The simulator's outputs are draws of a GP; here they
are log means: spot n has a size factor exp(o[n]) and output p a size r_p, and y[n, p] ~ NB(mean exp(f[n, p] + o[n]),
size r_p), drawn as a Poisson with a Gamma(r_p, r_p)-distributed multiplier on its rate (variance mu + mu^2 / r_p).
``model.likelihood = "negative_binomial"`` creates ``model.log_dispersion[m]`` (rho, r = exp(rho), zeros at the start) -
set it BEFORE the optimizer is built, as ``fit`` does here after the assignment - and the fit runs on the counts themselves.  It prints
the recovered r next to the true one, and the RMSE of the log mean for the NB fit and for a Poisson fit of the same counts
(which has nowhere to put the excess variance).
usage: python examples/negbin_counts.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import predict, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 600
dev = torch.device("cuda:0")
mod = "expression"
P = 10
X, Fl, nsl, _ = simulate.generate_twod_data(2, P, 30, noise_variance=0.0, seed=0)  # Fl [2 n, P]: the log means
n = int(nsl[0])
gen = torch.Generator().manual_seed(1)
o = 0.5 * torch.randn(2 * n, generator=gen) + 1.5  # log size factors (mean counts of a few)
r_true = torch.exp(torch.linspace(-1.0, 2.0, P))   # sizes from 0.37 (heavy overdispersion) to 7.4 (nearly Poisson)
mu = torch.exp(Fl + o[:, None])
lam = torch._standard_gamma(r_true.expand_as(mu).contiguous(), generator=gen) / r_true
Y = torch.poisson(mu * lam, generator=gen)
print(f"{Y.numel()} counts, mean {float(Y.mean()):.2f}, {float((Y == 0).float().mean()) * 100:.0f} % zeros, max {int(Y.max())}")


def on_device(dd):
    return {m: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for m, d in dd.items()}


def log_mean_rmse(model):
    view_idx = {mod: [torch.arange(n), torch.arange(n, 2 * n)]}
    out = predict(model, {mod: X.to(dev)}, view_idx, {mod: 2 * n}, S=10,
                  generator=torch.Generator(device=dev).manual_seed(2))[mod]
    return float((out.F_mean.cpu() - Fl).pow(2).mean().sqrt())


dd = simulate.as_data_dict(X, Y, [n, n])
dd[mod]["log_offset"] = o
model = make_model(dd, m=25, device=dev)
model.likelihood = "negative_binomial"  # before fit builds its optimizer: log_dispersion is a parameter from here on
fit(model, on_device(dd), steps, lr=1e-2, S=3, sync_every=100)
r_fit = torch.exp(model.log_dispersion[mod].detach().cpu())
print("negative binomial likelihood on the counts: size r per output, recovered / true")
for p in range(P):
    print(f"  output {p}: {float(r_fit[p]):7.3f} / {float(r_true[p]):7.3f}")
print(f"  RMSE of the log mean {log_mean_rmse(model):.4f} (the log means have unit scale)")

model_p = make_model(dd, m=25, device=dev)
model_p.likelihood = "poisson"
fit(model_p, on_device(dd), steps, lr=1e-2, S=3, sync_every=100)
print(f"Poisson likelihood on the same counts: RMSE of the log rate {log_mean_rmse(model_p):.4f}")
