"""Two slices with an H&E-like image each: build the expression and the histology modality, fit, lay slice 2's image
over slice 1.

Simulated data only.  A smooth field (random Fourier features of an RBF kernel, simulate.gp_draws' "rff" construction)
is seen on two slices: slice 1 shows it as it is; slice 2 shows it deformed - the point q of slice 2 shows what lies at
h(q) = q + 0.35 (sin, cos) of the field.  Each slice has 20 x 20 spots with 6 expression features and a 96 x 96 RGB
image of the field's first three features whose border, outside the tissue, is the 0.7 gray of a Visium "hires" image.

``histology_modality`` turns the two images into ``data_dict["histology"]`` (background and pixels outside the spots
dropped, 1500 pixels per slice, coordinates scaled to [0, 10], values z-scored per slice: the reference's
visium_multimodal_alignment.py lines 70-127, 191-213, 243-266).  After the fit, ``warp_image`` resamples slice 2's image
in the common coordinate system - slice 1 is fixed, so that is slice 1's frame - and the mean squared difference to slice
1's image over the tissue both slices show is printed before and after.
usage: python examples/histology_modality.py [steps]"""
import math
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

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
P, R, SIDE, PIX = 6, 64, 20, 96

# the field and slice 2's deformation
om = torch.randn(2, R, dtype=torch.float64, device=dev, generator=gen) / 2.5  # lengthscale 2.5
ph = torch.rand(R, dtype=torch.float64, device=dev, generator=gen) * (2.0 * math.pi)
amp = torch.randn(R, P, dtype=torch.float64, device=dev, generator=gen) * math.sqrt(2.0 / R)


def field(x):
    return torch.cos(x.double() @ om + ph) @ amp


def h(q):
    q = q.double()
    return q + 0.35 * torch.stack([torch.sin(2 * math.pi * q[:, 1] / 10 + 1), torch.cos(2 * math.pi * q[:, 0] / 10 + 1)], 1)


# spots and expression: the same lattice of positions on both slices, different tissue under them on slice 2
lat = simulate.lattice_2d(SIDE, device=dev)
n = lat.shape[0]
noise = lambda: 0.1 * torch.randn(n, P, dtype=torch.float64, device=dev, generator=gen)
Y = torch.cat([field(lat) + noise(), field(h(lat)) + noise()]).float()
expression = {"spatial_coords": torch.cat([lat, lat]), "n_samples_list": [n, n],
              "outputs": gp.standardize_views(Y, [n, n]).outputs}

# the images: pixel (c, r) lies at -1 + 12 c / (PIX - 1) of the slice's coordinates; outside [0, 10]^2 there is no tissue
native = gp.Frame(origin=(-1.0, -1.0), step=(12.0 / (PIX - 1), 12.0 / (PIX - 1)))
rr, cc = torch.meshgrid(torch.arange(PIX, device=dev), torch.arange(PIX, device=dev), indexing="ij")
at = native(torch.stack([cc.reshape(-1), rr.reshape(-1)], 1))
tissue = ((at >= 0) & (at <= 10)).all(1)


def render(points):
    rgb = (0.5 + 0.4 * torch.tanh(field(points)[:, :3])).float()
    rgb[~tissue] = 0.7
    return rgb.view(PIX, PIX, 3)


images = [render(at), render(h(at))]
spots_px = native.inverse(lat)  # the spots in the images' pixel coordinates
hist = gp.histology_modality(images, [spots_px, spots_px], n_samples=1500, generator=gen)
for v in (0, 1):
    print(f"slice {v + 1}: {hist['n_pixels'][v]} tissue pixels under the spots ({hist['n_background'][v]} background, "
          f"{hist['n_outside'][v]} outside), {hist['n_samples_list'][v]} drawn; {hist['frames'][v]}")

dd = {"expression": expression,
      "histology": {k: hist[k] for k in ("spatial_coords", "outputs", "n_samples_list")}}
model = make_model(dd, m=25, fixed_view_idx=0, device=dev)
fit(model, dd, steps, lr=1e-2, S=3, sync_every=100)
learned = model.warp_field(lat, 1, jacobian=False).G_mean  # the simulation knows the answer: g(q) = h(q)
print(f"slice 2's spots: mean distance to where they belong {float((lat.double() - h(lat)).norm(dim=1).mean()):.3f} as "
      f"they are, {float((learned - h(lat)).norm(dim=1).mean()):.3f} through the learned warp")

# slice 2's image in the common coordinate system, on slice 1's pixel grid
res = model.warp_image(images[1], 1, img_frame=hist["frames"][1], out_frame=hist["frames"][0])
# compare where both slices show tissue: slice 2's tissue mask goes through the same warp (nearest pixel)
mask = model.warp_image(tissue.view(PIX, PIX).float(), 1, img_frame=hist["frames"][1], out_frame=hist["frames"][0], order=0)
inside = res.valid & tissue.view(PIX, PIX) & (mask.image[:, :, 0] > 0.5)
mse = lambda a: float(((a - images[0]) ** 2).sum(-1)[inside].mean())
print(f"warp_image: {int(res.valid.sum())} of {PIX * PIX} pixels valid, {int(res.n_unconverged)} not converged, "
      f"{int(res.n_outside)} outside slice 2's image")
print(f"image MSE against slice 1 over the {int(inside.sum())} pixels of common tissue: {mse(images[1]):.5f} before, "
      f"{mse(res.image):.5f} after {steps} steps")
