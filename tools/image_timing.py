"""Time image_pixels, image_sample and warp_image against what torch offers for the same work on the same device.

image_pixels (csrc/image.hip: count pass, scan, stable compaction) against the torch route: the fp32 values, the
background mask by torch.round, the bounding-box mask from two aranges, ``nonzero`` and a gather.  image_sample (bilinear,
fp64 arithmetic) against ``torch.nn.functional.grid_sample(align_corners=True)`` on an fp32 NCHW copy of the image (fp32
arithmetic; the copy is made outside the timed window), both at the same --points random coordinates.  warp_image at
2000 x 2000 with M = 200 inducing points per view (the size of config 2) has no torch counterpart: its time is reported
with the share of its unwarp stage.

One process, device events around synchronised work, every shape warmed up first, the routes alternating in blocks
(median and min-max over the blocks); peak allocations above the inputs per route.  The image is uint8 [side, side, 3]:
about 90 % gray background (178), the rest random; the bounding box keeps the middle 80 % of both axes.

  python tools/image_timing.py                    # 2000 x 2000 x 3, with warp_image
  python tools/image_timing.py --side 20000       # 20 000 x 20 000 x 3 (1.2 GB), without warp_image
Appends one JSON line per run to --out (default profiles/image_timing.jsonl).
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spatial_alignment_amd as gp  # noqa: E402
from spatial_alignment_amd import engine as E  # noqa: E402

MIB = float(1 << 20)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return round(peak / MIB, 1)


def make_image(side, dev, gen):
    """uint8 [side, side, 3] built in row bands (no side^2 fp32 temporary)"""
    img = torch.empty(side, side, 3, dtype=torch.uint8, device=dev)
    band = max(1, (1 << 24) // side)
    for r in range(0, side, band):
        rows = min(band, side - r)
        part = torch.randint(0, 150, (rows, side, 3), dtype=torch.uint8, device=dev, generator=gen)
        part[torch.rand(rows, side, device=dev, generator=gen) > 0.1] = 178
        img[r: r + rows] = part
    return img


def torch_pixels(img, bbox):
    """the torch route: mask, nonzero, gather -> (coords [n, 2] fp32, pixels [n, 3] fp32)"""
    H, W, _ = img.shape
    v = img.float() / 255.0
    bg = (torch.round(v * 10.0) == 7.0).all(-1)
    x = torch.arange(W, device=img.device, dtype=torch.float64)
    y = torch.arange(H, device=img.device, dtype=torch.float64)
    inside = ((x > bbox[0]) & (x < bbox[1]))[None, :] & ((y > bbox[2]) & (y < bbox[3]))[:, None]
    keep = ~bg & inside
    idx = keep.nonzero()
    return idx.flip(1).float(), v[idx[:, 0], idx[:, 1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=2000)
    ap.add_argument("--points", type=int, default=4_000_000, help="coordinates of the sampling comparison")
    ap.add_argument("--m", type=int, default=200, help="inducing points per view of the warp_image model")
    ap.add_argument("--no-warp", action="store_true", help="skip warp_image (it is skipped above side 4000 anyway)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per block")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "image_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    side, n = args.side, args.points
    img = make_image(side, dev, gen)
    bbox = (0.1 * side, 0.9 * side, 0.1 * side, 0.9 * side)
    o = E.ops()

    # ---- image_pixels against mask / nonzero / gather
    ours = lambda: gp.image_pixels(img, bbox=bbox)
    theirs = lambda: torch_pixels(img, bbox)
    a, b = ours(), theirs()
    # (torch divides by a scalar through its reciprocal, so its u / 255 can differ from the one fp32 division in an ulp)
    same_rows = tuple(a.coords.shape) == tuple(b[0].shape)
    agree = dict(pixels_rows=int(a.coords.shape[0]), torch_rows=int(b[0].shape[0]),
                 coords_equal=bool(same_rows and torch.equal(a.coords, b[0])),
                 pixels_max_abs_diff=float((a.pixels - b[1]).abs().max()) if same_rows and a.coords.shape[0] else None)
    del a, b

    # ---- image_sample against grid_sample(align_corners=True) on an fp32 copy
    xy = torch.rand(n, 2, dtype=torch.float64, device=dev, generator=gen) * (side - 1)
    nchw = (img.float() / 255.0).permute(2, 0, 1).unsqueeze(0).contiguous()
    grid = (xy / (side - 1) * 2.0 - 1.0).float().view(1, 1, n, 2)
    sample = lambda: o.image_sample(img, xy, order=1)
    gsample = lambda: torch.nn.functional.grid_sample(nchw, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    s, g = sample()[0], gsample()[0, :, 0].t()
    agree["sample_max_abs_diff_vs_grid_sample"] = float((s - g).abs().max())  # grid_sample: fp32 coordinates and arithmetic
    del s, g

    legs = {"image_pixels": ours, "torch_mask_nonzero_gather": theirs, "image_sample": sample, "grid_sample": gsample}

    # ---- warp_image: no torch counterpart
    if not args.no_warp and side <= 4000:
        M, mod = args.m, "expression"
        hg = torch.Generator().manual_seed(0)
        dd = {mod: {"spatial_coords": torch.rand(2000, 2, generator=hg) * 10, "outputs": torch.randn(2000, 2, generator=hg),
                    "n_samples_list": [1000, 1000]}}
        torch.manual_seed(0)
        np.random.seed(0)
        model = gp.VariationalGPSA(dd, m_X_per_view=M, m_G=16, data_init=False, n_latent_gps={mod: None}, fixed_view_idx=0)
        with torch.no_grad():
            Z = torch.rand(model.Xtilde.shape, generator=hg) * 10
            model.Xtilde.copy_(Z)
            model.delta_G_list.copy_(Z + 0.3 * torch.sin(0.6 * Z.flip(-1)))  # a smooth displacement: no fold
            model.warp_kernel_lengthscales.fill_(math.log(0.7))
        model = model.to(dev)
        frame = gp.Frame((0.0, 0.0), (10.0 / (side - 1), 10.0 / (side - 1)))
        legs["warp_image"] = lambda: model.warp_image(img, 1, img_frame=frame)
        legs["warp_image_fixed_view"] = lambda: model.warp_image(img, 0, img_frame=frame)
        r = legs["warp_image"]()
        agree.update(warp_valid=int(r.valid.sum()), warp_unconverged=int(r.n_unconverged), warp_outside=int(r.n_outside))
        del r

    for fn in legs.values():  # every shape warmed up
        fn()
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.calls))
    peaks = {k: peak_of(fn) for k, fn in legs.items()}
    line = dict(tool="image_timing", H=side, W=side, C=3, dtype="uint8", points=n, blocks=args.blocks, calls=args.calls,
                device=torch.cuda.get_device_name(0), image_mib=round(img.numel() / MIB, 1),
                select_workspace_mib=round(o.lib.gpsa_image_select_workspace(side, side, 1) / MIB, 3), agree=agree,
                ms={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()},
                peak_mib=peaks)
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
