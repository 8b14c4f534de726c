"""Two views profiled with different panels: view 1 measures half of the outputs.  Fit on all of it, impute the rest.

Two warped views of a 30 x 30 lattice (simulate.generate_twod_data).  View 0 measures all 10 outputs, view 1 the first 5:
its other entries are NaN.  With ``model.skip_missing = True`` the fit uses every observed entry - the loss is the ELBO
of the observed data - and ``predict`` then imputes view 1's unmeasured outputs, printed as an RMSE against the
simulated truth.  The only route without the flag is to cut both views to the shared 5 outputs: that model has no
output 5 .. 9 at all, so the same figure is printed for its best guess, the per-output mean of view 0.
usage: python examples/missing_panels.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import predict, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda:0")
mod = "expression"
P, shared = 10, 5
X, Y, nsl, _ = simulate.generate_twod_data(2, P, 30, noise_variance=0.01, seed=0)
n = int(nsl[0])
view1 = torch.arange(n, 2 * n)
truth = Y[view1][:, shared:]  # what view 1 did not measure


def on_device(dd):
    return {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}


# all outputs, view 1's unmeasured ones marked missing
Ym = Y.clone()
Ym[n:, shared:] = float("nan")
dd = simulate.as_data_dict(X, Ym, [n, n])
model = make_model(dd, m=25, device=dev)
model.skip_missing = True
fit(model, on_device(dd), steps, lr=1e-2, S=3, sync_every=100)
view_idx = {mod: [torch.arange(0), torch.arange(n)]}  # predict rows of view 1 (view 0 gets none here)
out = predict(model, {mod: X[view1].to(dev)}, view_idx, {mod: n}, S=10,
              generator=torch.Generator(device=dev).manual_seed(2))[mod]
rmse = float((out.F_mean.cpu()[:, shared:] - truth).pow(2).mean().sqrt())
print(f"skip_missing fit on {int((~torch.isnan(Ym)).sum())} of {Ym.numel()} entries: "
      f"RMSE of view 1's {P - shared} unmeasured outputs {rmse:.4f} (outputs have unit scale)")

# the shared half only: this model cannot predict outputs 5 .. 9 - the per-output mean of view 0 stands in
dd_s = simulate.as_data_dict(X, Y[:, :shared].contiguous(), [n, n])
model_s = make_model(dd_s, m=25, device=dev)
fit(model_s, on_device(dd_s), steps, lr=1e-2, S=3, sync_every=100)
out_s = predict(model_s, {mod: X[view1].to(dev)}, view_idx, {mod: n}, S=10,
                generator=torch.Generator(device=dev).manual_seed(2))[mod]
rmse_shared = float((out_s.F_mean.cpu() - Y[view1][:, :shared]).pow(2).mean().sqrt())
guess = Y[:n, shared:].mean(0, keepdim=True).expand_as(truth)
rmse_guess = float((guess - truth).pow(2).mean().sqrt())
print(f"shared-half fit ({shared} outputs): its own outputs at RMSE {rmse_shared:.4f}; outputs {shared} .. {P - 1} are not "
      f"in the model - view 0's per-output mean gives RMSE {rmse_guess:.4f}")
