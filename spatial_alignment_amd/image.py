"""Histology images: a pixel modality in, the aligned image out.

The reference's second modality is the H&E image (experiments/expression/visium/visium_multimodal_alignment.py):
``process_image`` (lines 70-117) lists the value at every (column, row) of the image with a Python loop, drops the gray
background (every channel rounds to 0.7 at one decimal), drops the pixels outside the spots' bounding box, and the
script then draws a random subset, rescales the coordinates (``scale_spatial_coords``) and z-scores the values per
slice (lines 191-213, 243-266).  Here that is

* ``image_pixels``: the selection on the device in two passes over the image (csrc/image.hip: count, then a stable
  compaction), optionally on ``bin`` x ``bin`` block means - no [H W, 2] coordinate array, nothing of H W elements;
* ``histology_modality``: the whole of ``data_dict["histology"]`` for several slices, with the frames that map a pixel
  to its model coordinate;
* ``warp_image``: what a fitted warp is for - slice ``view``'s image resampled in the common coordinate system, every
  output pixel sent back through ``unwarp`` and read by bilinear interpolation;
* ``Frame`` / ``scale_spatial_coords``: the affine map between pixel indices and coordinates that ties these together.

Coordinates are (x, y) = (column, row), as the reference's ``X_img``.  Everything runs without gradients.  Not offered:
reading image files or AnnData, volumes, bicubic or antialiased resampling, sampled warps.
"""
import math
import operator
from typing import NamedTuple

import numpy as np
import torch

from ._args import ops as _ops

f32, f64 = torch.float32, torch.float64
GRAY_PIXEL_VAL = 0.7  # the reference's background: visium_multimodal_alignment.py:27
DEFAULT_CHUNK_PIXELS = 1 << 20  # warp_image: output pixels per chunk of rows by default


class Frame:
    """The affine map ``coord = origin + step * pixel`` on the two axes (x, y), and its inverse.  ``origin`` and ``step``
    are pairs of finite numbers, no ``step`` zero.  Calling the frame maps pixel coordinates [..., 2] to coordinates,
    ``inverse`` maps back; both work in fp64 and return fp64 (a tensor for a tensor, an array for anything else)."""

    __slots__ = ("origin", "step")

    def __init__(self, origin=(0.0, 0.0), step=(1.0, 1.0)):
        try:
            o, s = tuple(float(v) for v in origin), tuple(float(v) for v in step)
        except (TypeError, ValueError):
            o = s = ()
        if len(o) != 2 or len(s) != 2 or not all(math.isfinite(v) for v in o + s) or 0.0 in s:
            raise ValueError(f"Frame: origin and step must be two finite numbers each and no step 0, not {origin!r}, "
                             f"{step!r}")
        self.origin, self.step = o, s

    def _pair(self, like, vals):
        if torch.is_tensor(like):
            return torch.tensor(vals, dtype=f64, device=like.device)
        return np.asarray(vals, dtype=np.float64)

    @staticmethod
    def _points(P, what):
        P = P.detach().to(f64) if torch.is_tensor(P) else np.asarray(P, dtype=np.float64)
        if P.ndim < 1 or P.shape[-1] != 2:
            raise ValueError(f"Frame.{what}: the last axis must hold (x, y), not shape {tuple(P.shape)}")
        return P

    def __call__(self, pixel):
        P = self._points(pixel, "__call__")
        return self._pair(P, self.origin) + self._pair(P, self.step) * P

    def inverse(self, coord):
        X = self._points(coord, "inverse")
        return (X - self._pair(X, self.origin)) / self._pair(X, self.step)

    def __eq__(self, other):
        return isinstance(other, Frame) and self.origin == other.origin and self.step == other.step

    def __hash__(self):
        return hash((self.origin, self.step))

    def __repr__(self):
        return f"Frame(origin={self.origin}, step={self.step})"


def _check_frame(frame, name, what):
    if not isinstance(frame, Frame):
        raise ValueError(f"{what}: {name} must be a Frame, not {type(frame).__name__}")
    return frame


def scale_spatial_coords(X, max_val=10.0, frame=None):
    """The helper every script of the reference defines: subtract the column minimum, divide by the maximum of what is
    left, multiply by ``max_val`` - per column of ``X`` [n, 2].  Returns ``(X_scaled, frame)``: the ``Frame`` that was
    applied (``X_scaled = frame(X)``, formed in fp64 and returned in ``X``'s floating dtype; fp64 for integers), so that
    other points - an image's pixels next to its spots - can be given the same scaling with ``frame=``.
    Raises ValueError for an ``X`` that is not [n >= 1, 2], NaN or infinite values, or a column without any extent."""
    what = "scale_spatial_coords"
    is_t = torch.is_tensor(X)
    A = X.detach() if is_t else np.asarray(X)
    if A.ndim != 2 or A.shape[1] != 2 or A.shape[0] < 1:
        raise ValueError(f"{what}: X has shape {tuple(A.shape)}, [n >= 1, 2] is needed")
    if frame is None:
        if not float(max_val) > 0.0 or not math.isfinite(float(max_val)):
            raise ValueError(f"{what}: max_val must be a positive finite number, not {max_val!r}")
        A64 = A.to(f64) if is_t else A.astype(np.float64)
        lo = [float(A64[:, d].min()) for d in range(2)]
        rng = [float(A64[:, d].max()) - lo[d] for d in range(2)]
        if not all(math.isfinite(v) for v in lo + rng) or min(rng) <= 0.0:
            raise ValueError(f"{what}: X must be finite and have an extent in both columns (minima {lo}, ranges {rng})")
        step = [float(max_val) / r for r in rng]
        frame = Frame(origin=[-l * s for l, s in zip(lo, step)], step=step)
    else:
        _check_frame(frame, "frame", what)
    out = frame(A)
    if is_t:
        return (out.to(X.dtype) if X.dtype.is_floating_point else out), frame
    return (out.astype(A.dtype) if np.issubdtype(A.dtype, np.floating) else out), frame


class ImagePixels(NamedTuple):
    """``image_pixels``' result: ``coords`` [n, 2] fp32 = (x, y) in pixel coordinates of the image, ``pixels`` [n, C] fp32,
    the counts of the dropped ``n_background`` and ``n_outside`` pixels, and ``shape`` = (H', W') of the (binned) grid the
    pixels come from: ``n + n_background + n_outside == H' W'``."""
    coords: torch.Tensor
    pixels: torch.Tensor
    n_background: int
    n_outside: int
    shape: tuple


def _check_image(img, what):
    """[H, W] or [H, W, C] tensor / array, uint8 or floating -> the tensor [H, W, C], where it is"""
    if not torch.is_tensor(img):
        if not isinstance(img, np.ndarray):
            raise ValueError(f"{what}: img must be a tensor or a numpy array, not {type(img).__name__}")
        img = torch.from_numpy(np.ascontiguousarray(img))
    img = img.detach()
    if img.dim() == 2:
        img = img.unsqueeze(-1)
    if img.dim() != 3 or min(img.shape) < 1 or img.shape[2] > 4:
        raise ValueError(f"{what}: img has shape {tuple(img.shape)}; [H, W] or [H, W, C] with C in 1..4 is needed")
    if img.dtype != torch.uint8 and not img.dtype.is_floating_point:
        raise ValueError(f"{what}: img is {img.dtype}; uint8 (read as u / 255) or a floating dtype is needed")
    return img


def _as_image(img, device, what):
    """... -> contiguous uint8 or fp32 [H, W, C] on ``device``"""
    img = _check_image(img, what)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"{what}: device {str(dev)!r}: the image kernels run on the GPU only and there is no host path")
    img = img.to(dev)
    return (img if img.dtype == torch.uint8 else img.to(f32)).contiguous()


def _bbox_of(spots, bbox, what):
    if spots is not None and bbox is not None:
        raise ValueError(f"{what}: give spots or bbox, not both")
    if spots is not None:
        S = spots.detach().to("cpu", f64).numpy() if torch.is_tensor(spots) else np.asarray(spots, dtype=np.float64)
        if S.ndim != 2 or S.shape[1] != 2 or S.shape[0] < 1:
            raise ValueError(f"{what}: spots has shape {tuple(S.shape)}, [m >= 1, 2] is needed")
        bbox = (S[:, 0].min(), S[:, 0].max(), S[:, 1].min(), S[:, 1].max())  # the reference's lines 103-104
    if bbox is None:
        return None
    try:
        vals = tuple(float(v) for v in bbox)
    except (TypeError, ValueError):
        vals = ()
    if len(vals) != 4 or any(v != v for v in vals):
        raise ValueError(f"{what}: the bounding box must be four numbers (xmin, xmax, ymin, ymax) without a NaN, "
                         f"not {bbox!r}")
    return vals


@torch.no_grad()
def image_pixels(img, *, spots=None, bbox=None, background=GRAY_PIXEL_VAL, bin=1, device=None):
    """The pixels of ``img`` that belong to the tissue under the spots: the reference's ``process_image`` on the device.

    img: [H, W] or [H, W, C] (C in 1..4), a tensor or a numpy array, uint8 (a value is u / 255) or floating (taken to
      fp32); moved to ``device`` (default: where it is when on a GPU, else the current GPU).
    bin: b in 1..64 - work on the [H div b, W div b] grid of the means of the full b x b blocks (fp64 sums, rounded once);
      a block's coordinate is its centre, ``x = c b + (b - 1) / 2``, so ``bin=1`` is the pixel's own (column, row).
    background: a pixel whose every channel rounds to it at one decimal (``numpy.round(v, 1) == 0.7`` in fp32) is
      dropped; ``None`` keeps such pixels.  A pixel with a NaN channel is never background.
    spots [m, 2] / bbox=(xmin, xmax, ymin, ymax): drop the pixels that are not strictly inside the spots' column minima
      and maxima, or inside the box given directly (in the image's pixel coordinates; give one of the two or neither).

    Returns ``ImagePixels(coords, pixels, n_background, n_outside, shape)`` in the row-major order of the image;
    ``n = 0`` is a valid result (empty tensors).  One small host read (the three counts) sizes the outputs exactly."""
    what = "image_pixels"
    box = _bbox_of(spots, bbox, what)
    if device is None:
        device = img.device if torch.is_tensor(img) and img.is_cuda else "cuda"
    img = _check_image(img, what)
    if isinstance(bin, bool) or not isinstance(bin, (int, np.integer)) or not 1 <= bin <= 64:
        raise ValueError(f"{what}: bin must be an integer in 1..64, not {bin!r}")
    if bin > min(img.shape[:2]):
        raise ValueError(f"{what}: bin = {bin} is larger than the image {tuple(img.shape[:2])}")
    if background is not None and not math.isfinite(float(background)):
        raise ValueError(f"{what}: background must be a finite number or None, not {background!r}")
    img = _as_image(img, device, what)
    coords, pixels, counts = _ops().image_select(img, bin=int(bin), background=background, bbox=box)
    H, W = int(img.shape[0]), int(img.shape[1])
    return ImagePixels(coords, pixels, int(counts[1]), int(counts[2]), (H // int(bin), W // int(bin)))


@torch.no_grad()
def histology_modality(images, spots_list=None, *, n_samples=None, generator=None, max_val=10.0, standardize=True,
                       **image_pixels_kw):
    """``data_dict["histology"]`` from one image per view: per view ``image_pixels`` (with ``spots=spots_list[v]`` when
    given), then an optional subset of ``n_samples`` rows without replacement (``torch.randperm`` from ``generator``,
    applied sorted: the rows stay in image order), then ``scale_spatial_coords``; over all views the per-view z-score of
    ``standardize_views`` (``standardize=False``: the raw values).

    Returns a dict: ``spatial_coords`` [N, 2] fp32, ``outputs`` [N, C] fp32, ``n_samples_list`` - what the model's
    ``data_dict`` takes - and ``outputs_rgb`` [N, C] (unstandardised, for ``callback_twod_multimodal(rgb=True)``),
    ``frames`` (a ``Frame`` per view: image pixel -> model coordinate), ``pixel_coords`` [N, 2] fp32 (the rows' pixel
    coordinates in their images), and per view ``n_pixels`` (kept before the subset), ``n_background``, ``n_outside``
    and ``shapes``.  Raises ValueError when a view keeps no pixel."""
    what = "histology_modality"
    images = list(images)
    V = len(images)
    if V < 1:
        raise ValueError(f"{what}: no image")
    spots_list = [None] * V if spots_list is None else list(spots_list)
    if len(spots_list) != V:
        raise ValueError(f"{what}: {V} images and {len(spots_list)} entries of spots_list")
    if n_samples is not None and (isinstance(n_samples, bool) or operator.index(n_samples) < 1):
        raise ValueError(f"{what}: n_samples must be a positive integer or None, not {n_samples!r}")
    from .counts import standardize_views

    coords, raw, px, frames, ns, n_pix, n_bg, n_out, shapes = [], [], [], [], [], [], [], [], []
    for v, (img, spots) in enumerate(zip(images, spots_list)):
        ip = image_pixels(img, spots=spots, **image_pixels_kw)
        n = int(ip.coords.shape[0])
        if n == 0:
            raise ValueError(f"{what}: view {v} keeps no pixel ({ip.n_background} background, {ip.n_outside} outside "
                             f"of {ip.shape[0]} x {ip.shape[1]})")
        C, P = ip.coords, ip.pixels
        if n_samples is not None and n_samples < n:  # the reference's lines 191-198, the rows kept in image order
            dev = C.device
            gdev = dev if generator is None else generator.device
            keep = torch.randperm(n, device=gdev, generator=generator)[: int(n_samples)].to(dev).sort().values
            C, P = C[keep].contiguous(), P[keep].contiguous()
        Xs, frame = scale_spatial_coords(C, max_val)
        coords.append(Xs), raw.append(P), px.append(C), frames.append(frame), ns.append(int(C.shape[0]))
        n_pix.append(n), n_bg.append(ip.n_background), n_out.append(ip.n_outside), shapes.append(ip.shape)
    if len({int(p.shape[1]) for p in raw}) != 1:
        raise ValueError(f"{what}: the images have different numbers of channels: {[int(p.shape[1]) for p in raw]}")
    rgb = torch.cat(raw).contiguous()
    outputs = standardize_views(rgb, ns).outputs if standardize else rgb.clone()
    return dict(spatial_coords=torch.cat(coords).contiguous(), outputs=outputs, n_samples_list=ns, outputs_rgb=rgb,
                frames=frames, pixel_coords=torch.cat(px), n_pixels=n_pix, n_background=n_bg, n_outside=n_out,
                shapes=shapes)


@torch.no_grad()
def warp_image(model, img, view, *, img_frame, out_shape=None, out_frame=None, order=1, fill=float("nan"),
               max_iter=None, rows_per_chunk=None):
    """Slice ``view``'s image in the common coordinate system, to lay over the template.

    Output pixel (r, c) has the common coordinate ``out_frame((c, r))``; ``unwarp(model, ., view)`` gives where that lies in
    the slice's native coordinates, ``img_frame.inverse`` gives the image's pixel coordinate, and the image is read there
    (``order=1``: bilinear in fp64, ``order=0``: nearest; csrc/image.hip).  ``img_frame`` maps a pixel of ``img`` to the
    coordinates the model was fitted in (``histology_modality``'s ``frames[view]``, or the spots' scaling);
    ``out_frame`` defaults to it and ``out_shape`` to the image's (H, W).

    Returns a ``Prediction``: ``image`` [Ho, Wo, C] fp32 (``fill`` where the pixel falls outside the image or the
    iteration failed), ``valid`` [Ho, Wo] bool (converged and inside the image), ``residual`` [Ho, Wo] fp64 (``unwarp``'s),
    ``n_unconverged`` and ``n_outside`` (0-dim int64: rows that did not converge; converged rows outside the image).
    The work goes in chunks of ``rows_per_chunk`` output rows (default: about a million pixels), so only a chunk's
    coordinate arrays exist besides the result; the result does not depend on the chunking.  A fixed view is the identity:
    no Newton stage, the two frames are composed in closed form.  ``max_iter``: ``unwarp``'s (default: its default).
    Raises ValueError for a model that is not two-dimensional, a bad ``view``, a warp kernel that is not a built-in, a
    frame that is not a ``Frame``, a bad ``out_shape``, ``order``, ``max_iter`` or ``rows_per_chunk``."""
    from . import warp as Wp
    from .predict import Prediction

    what = "warp_image"
    if int(model.n_spatial_dims) != 2:
        raise ValueError(f"{what}: the model has n_spatial_dims = {int(model.n_spatial_dims)}; an image needs 2")
    view = Wp._check_view(model, view, what)
    img_frame = _check_frame(img_frame, "img_frame", what)
    out_frame = img_frame if out_frame is None else _check_frame(out_frame, "out_frame", what)
    max_iter = Wp.DEFAULT_MAX_ITER if max_iter is None else max_iter
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 0:
        raise ValueError(f"{what}: max_iter must be an integer >= 0, not {max_iter!r}")
    if order not in (0, 1) or isinstance(order, bool):
        raise ValueError(f"{what}: order must be 0 (nearest) or 1 (bilinear), not {order!r}")
    fixed = bool(model._is_fixed(view))
    if not fixed:
        Wp._check_kind(model, what)
    img = _check_image(img, what)
    H, W, C = (int(s) for s in img.shape)
    if out_shape is None:
        out_shape = (H, W)
    try:
        Ho, Wo = (operator.index(s) for s in out_shape)
    except (TypeError, ValueError):
        Ho = Wo = 0
    if Ho < 1 or Wo < 1:
        raise ValueError(f"{what}: out_shape must be two positive integers (rows, columns), not {out_shape!r}")
    rows = Wp._chunk(max(1, DEFAULT_CHUNK_PIXELS // Wo) if rows_per_chunk is None else rows_per_chunk, Ho)
    dev = model.Xtilde.device
    img = _as_image(img, dev, what)

    o = _ops()
    image = torch.empty(Ho, Wo, C, dtype=f32, device=dev)
    inside = torch.empty(Ho * Wo, dtype=torch.uint8, device=dev)
    if fixed:
        residual = torch.zeros(Ho * Wo, dtype=f64, device=dev)
        # img_frame^-1 o out_frame in closed form: with equal frames the pixel's own indices, exactly
        step = [so / si for so, si in zip(out_frame.step, img_frame.step)]
        through = Frame([(oo - oi) / si for oo, oi, si in zip(out_frame.origin, img_frame.origin, img_frame.step)],
                        step) if out_frame != img_frame else Frame()
    else:
        residual = torch.empty(Ho * Wo, dtype=f64, device=dev)
        mdl = Wp._warp_model(model, view, o)
        A, b = mdl[3], mdl[4]
        Ainv = torch.linalg.inv(A.cpu()).to(dev)
    tol = Wp.REL_TOL * Wp._extent(model, view)
    cols = torch.arange(Wo, dtype=f64, device=dev)
    flat = image.view(Ho * Wo, C)
    for r0 in range(0, Ho, rows):
        r1 = min(Ho, r0 + rows)
        a, e = r0 * Wo, r1 * Wo
        P = torch.empty(e - a, 2, dtype=f64, device=dev)
        P[:, 0] = cols.repeat(r1 - r0)
        P[:, 1] = torch.arange(r0, r1, dtype=f64, device=dev).repeat_interleave(Wo)
        if fixed:
            xy = through(P) if through != Frame() else P
        else:
            G = out_frame(P)
            X = torch.empty_like(G)
            x0 = ((G - b) @ Ainv).contiguous()  # unwarp's default start: the affine part alone
            o.warp_invert(*mdl, G, x0, int(max_iter), out=(X, residual[a:e]))
            xy = img_frame.inverse(X)
        o.image_sample(img, xy, order=order, fill=fill, out=(flat[a:e], inside[a:e]))
    converged = residual <= tol
    inside = inside.bool()
    return Prediction(image=image, valid=(converged & inside).view(Ho, Wo), residual=residual.view(Ho, Wo),
                      n_unconverged=(~converged).sum(), n_outside=(converged & ~inside).sum(), tol=tol)
