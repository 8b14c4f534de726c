"""Count outputs: two warped views of a lattice whose outputs are Poisson counts with per-spot size factors.

Two warped views of a 30 x 30 lattice (simulate.generate_twod_data).  The simulator's outputs are draws of a GP; here they
are log rates: every spot n gets a size factor exp(o[n]) and its counts are y[n, p] ~ Poisson(exp(f[n, p] + o[n])).
With ``model.likelihood = "poisson"`` and ``data_dict[m]["log_offset"] = o`` the fit runs on the counts themselves - no
log transform, no Gaussian noise model - and ``predict`` returns the moments of the log rate, printed as an RMSE against
the simulated f.  Next to it, the usual route: the same model with the Gaussian likelihood on log1p of the
size-normalised counts.  It ends with the held-out score: a second draw of counts at the same spots, scored by
``predict(..., Y=counts, scale="response", log_offset=o)`` - the Poisson-lognormal log predictive density ``lpd_sum`` and
the expected counts ``Y_mean``.
usage: python examples/poisson_counts.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import predict, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
dev = torch.device("cuda:0")
mod = "expression"
P = 10
X, Fl, nsl, _ = simulate.generate_twod_data(2, P, 30, noise_variance=0.0, seed=0)  # Fl [2 n, P]: the log rates
n = int(nsl[0])
gen = torch.Generator().manual_seed(1)
o = 0.5 * torch.randn(2 * n, generator=gen)  # log size factors
Y = torch.poisson(torch.exp(Fl + o[:, None]), generator=gen)
print(f"{Y.numel()} counts, mean {float(Y.mean()):.2f}, {float((Y == 0).float().mean()) * 100:.0f} % zeros, max {int(Y.max())}")


def on_device(dd):
    return {m: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for m, d in dd.items()}


def log_rate_rmse(model):
    view_idx = {mod: [torch.arange(n), torch.arange(n, 2 * n)]}
    out = predict(model, {mod: X.to(dev)}, view_idx, {mod: 2 * n}, S=10,
                  generator=torch.Generator(device=dev).manual_seed(2))[mod]
    return float((out.F_mean.cpu() - Fl).pow(2).mean().sqrt())


# the counts themselves, with the size factors as offsets
dd = simulate.as_data_dict(X, Y, [n, n])
dd[mod]["log_offset"] = o
model = make_model(dd, m=25, device=dev)
model.likelihood = "poisson"
fit(model, on_device(dd), steps, lr=1e-2, S=3, sync_every=100)
print(f"Poisson likelihood on the counts: RMSE of the log rate {log_rate_rmse(model):.4f} (the log rates have unit scale)")

# the work-around: normalise by the size factors, log1p, fit the Gaussian model
dd_g = simulate.as_data_dict(X, torch.log1p(Y / torch.exp(o)[:, None]), [n, n])
model_g = make_model(dd_g, m=25, device=dev)
fit(model_g, on_device(dd_g), steps, lr=1e-2, S=3, sync_every=100)
print(f"Gaussian likelihood on log1p(counts / size factor): RMSE against the log rate {log_rate_rmse(model_g):.4f}")

# held-out counts at the same spots: the score of the Poisson fit on the scale of the observations
Y_new = torch.poisson(torch.exp(Fl + o[:, None]), generator=gen)
view_idx = {mod: [torch.arange(n), torch.arange(n, 2 * n)]}
out = predict(model, {mod: X.to(dev)}, view_idx, {mod: 2 * n}, S=10, Y={mod: Y_new}, scale="response",
              log_offset={mod: o.to(dev)}, generator=torch.Generator(device=dev).manual_seed(3))[mod]
rmse = float((out.Y_mean.cpu() - Y_new).pow(2).mean().sqrt())
print(f"held-out counts: lpd_sum {float(out.lpd_sum):.1f} ({float(out.lpd_sum) / Y_new.numel():.4f} per count), "
      f"RMSE of Y_mean {rmse:.3f} (the counts' own sd {float(Y_new.std()):.3f})")
