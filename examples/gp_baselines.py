"""The prediction baselines of the reference's simulations, on the device: exact GP regression next to kNN.

Two views of a 15 x 15 lattice observing the same 5 outputs (simulate.generate_twod_data), view 1 warped, view 0 fixed.
A fifth of every view's spots is held out.

* The data kernel's starting length scale is estimated by an exact GP on view 0 alone, ``RBF() + WhiteKernel()``, and fed
  to the model before the fit (experiments/simulations/two_dimensional.py:84-91).
* ``prediction_baselines``: the "union" GP on all training spots at their unaligned coordinates and the "separate" GP per
  view (two_dimensional_prediction.py:126-155) - mean over spots of the summed squared error.
* The GP on the ALIGNED coordinates (``G_means``, :238), before and after a short ``fit``, with ``knn_regress`` (k = 10,
  inverse-distance weights: slideseq_prediction.py:275-308) at the same coordinates next to it.
usage: python examples/gp_baselines.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from spatial_alignment_amd import gp_regress, knn_regress, prediction_baselines, simulate  # noqa: E402
from spatial_alignment_amd.synthetic import make_model  # noqa: E402
from spatial_alignment_amd.train import fit  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
dev = torch.device("cuda:0")
X, Y, nsl, _ = simulate.generate_twod_data(2, 5, 15, noise_variance=0.01, fixed_view_idx=0, seed=0)
X, Y = torch.as_tensor(X, dtype=torch.float32), torch.as_tensor(Y, dtype=torch.float32)
n = int(nsl[0])

# hold out every fifth spot of each view
test = torch.zeros(2 * n, dtype=torch.bool)
test[torch.randperm(n, generator=torch.Generator().manual_seed(1))[: n // 5]] = True
test[n + torch.randperm(n, generator=torch.Generator().manual_seed(2))[: n // 5]] = True
Xtr, Ytr, Xte, Yte = X[~test].to(dev), Y[~test].to(dev), X[test].to(dev), Y[test].to(dev)
ns_tr = [int((~test[:n]).sum()), int((~test[n:]).sum())]
ns_te = [int(test[:n].sum()), int(test[n:].sum())]


def mse(pred, truth):
    return float((pred.double() - truth.double()).square().sum(1).mean())


base = prediction_baselines(Xtr, Ytr, Xte, Yte, ns_tr, ns_te, kernel="rbf")
print(f"GP, union of the views at their own coordinates: {base.error_union:.4f}   "
      f"(length scale {base.fit_union.length_scale:.3f}, noise {base.fit_union.noise_level:.4f}, "
      f"{base.fit_union.n_eval} evaluations)")
print(f"GP, every view on its own:                        {base.error_separate:.4f}")

# the data kernel's starting length scale from view 0 (the reference's gpr.kernel_.k1.theta[0], a log value)
view0 = gp_regress(Xtr[: ns_tr[0]], Ytr[: ns_tr[0]], kernel="rbf")
print(f"view 0 alone: length scale {view0.length_scale:.3f}, noise {view0.noise_level:.4f}, LML {view0.lml:.2f}, "
      f"{view0.n_iter} iterations, {view0.n_eval} evaluations")

dd = simulate.as_data_dict(Xtr.cpu(), Ytr.cpu(), ns_tr)
model = make_model(dd, m=25, fixed_view_idx=0, device=dev)
with torch.no_grad():
    model.data_kernel_lengthscale.fill_(float(view0.theta[1]))
dd = {m: dict(d, spatial_coords=d["spatial_coords"].to(dev), outputs=d["outputs"].to(dev)) for m, d in dd.items()}


def aligned(points, counts):
    a = counts[0]
    return torch.cat([model.warp_field(points[:a], 0, jacobian=False).G_mean,
                      model.warp_field(points[a:], 1, jacobian=False).G_mean])


def report(when):
    Gtr, Gte = aligned(Xtr, ns_tr), aligned(Xte, ns_te)
    gp = gp_regress(Gtr, Ytr, kernel="rbf")
    knn = knn_regress(Gtr, Ytr, Gte, k=10, weights="distance")
    print(f"{when}: GP on the aligned coordinates {mse(gp.predict(Gte), Yte):.4f} (length scale {gp.length_scale:.3f}), "
          f"kNN (k = 10, 1 / distance) {mse(knn, Yte):.4f}")


report("before the fit")
fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)
report(f"after {steps} steps")
