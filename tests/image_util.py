"""The numpy yardstick of the image entries (csrc/image.hip), written from the rules of include/gpsa_hip.h with fp32
where a rule says fp32, plus the inputs the CPU and the GPU tests share."""
import functools
import os

import numpy as np

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_image.npz")


def as_values(img):
    """[H, W] / [H, W, C] uint8 or floating -> fp32 [H, W, C]: u / 255 as one fp32 division, a float as is"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    if img.dtype == np.uint8:
        return (img.astype(f32) / f32(255.0)).astype(f32)
    return img.astype(f32)


def block_mean(img, b):
    """[H div b, W div b, C] fp32: per channel the fp64 sum of the full b x b block in row-major order, / b^2 in fp64,
    rounded to fp32 once; the partial blocks at the right and bottom edges are dropped"""
    v = as_values(img)
    if b == 1:
        return v
    Ho, Wo = v.shape[0] // b, v.shape[1] // b
    acc = np.zeros((Ho, Wo, v.shape[2]), f64)
    for i in range(b):
        for j in range(b):  # row-major within the block: the order of the additions
            acc += v[i: Ho * b: b, j: Wo * b: b].astype(f64)
    return (acc / f64(b * b)).astype(f32)


def is_background(v, bg):
    """every channel has rint(v * 10) == rint(bg * 10), the products rounded in fp32, half to even; NaN: never"""
    with np.errstate(invalid="ignore"):
        q = np.rint((v * f32(10.0)).astype(f32))
        return np.all(q == np.rint(f32(bg) * f32(10.0)), axis=-1)


def select(img, bin=1, background=0.7, bbox=None):
    """-> coords [n, 2] fp32 = (x, y), pixels [n, C] fp32, (kept, background, outside), in row-major order"""
    v = block_mean(img, bin)
    Ho, Wo, C = v.shape
    half = (bin - 1) / 2.0
    x = (np.arange(Wo, dtype=f64) * bin + half)[None, :].repeat(Ho, 0)
    y = (np.arange(Ho, dtype=f64) * bin + half)[:, None].repeat(Wo, 1)
    bgm = is_background(v, background) if background is not None else np.zeros((Ho, Wo), bool)
    if bbox is not None:
        xmin, xmax, ymin, ymax = (f64(t) for t in bbox)
        inside = (xmin < x) & (x < xmax) & (ymin < y) & (y < ymax)
    else:
        inside = np.ones((Ho, Wo), bool)
    keep = ~bgm & inside
    coords = np.stack([x[keep], y[keep]], 1).astype(f32)
    return coords, v[keep], (int(keep.sum()), int(bgm.sum()), int((~bgm & ~inside).sum()))


def bbox_of(spots):
    s = np.asarray(spots, f64)
    return s[:, 0].min(), s[:, 0].max(), s[:, 1].min(), s[:, 1].max()


def sample(img, xy, order=1, fill=np.nan):
    """-> out [n, C] fp32, valid [n] bool; bilinear in fp64 rounded to fp32 once (order 1), nearest (order 0)"""
    v, (val, ok) = as_values(img), sample64(as_values(img), xy, order)
    out = np.full((len(ok), v.shape[2]), fill, f32)
    out[ok] = val[ok].astype(f32)
    return out, ok


def sample64(v, xy, order=1):
    """the fp64 value before the rounding: (val [n, C] fp64 - rows that are not valid hold 0 -, valid [n])"""
    v = np.asarray(v)
    if v.ndim == 2:
        v = v[:, :, None]
    H, W, C = v.shape
    xy = np.asarray(xy, f64)
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore"):
        ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    I = v.astype(f64)
    if order == 0:
        xi = np.clip(np.floor(xs + 0.5).astype(np.int64), 0, W - 1)
        yi = np.clip(np.floor(ys + 0.5).astype(np.int64), 0, H - 1)
        val = I[yi, xi]
    else:
        x0 = np.minimum(np.floor(xs).astype(np.int64), W - 2) if W > 1 else np.zeros(len(xs), np.int64)
        y0 = np.minimum(np.floor(ys).astype(np.int64), H - 2) if H > 1 else np.zeros(len(ys), np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        fx, fy = (xs - x0)[:, None], (ys - y0)[:, None]
        top = I[y0, x0] * (1.0 - fx) + I[y0, x1] * fx
        bot = I[y1, x0] * (1.0 - fx) + I[y1, x1] * fx
        val = top * (1.0 - fy) + bot * fy
    val = np.where(ok[:, None], val, 0.0)
    return val, ok


# ------------------------------------------------------------------------------------------------------------------------
# shared inputs
# ------------------------------------------------------------------------------------------------------------------------
def tissue_image(H, W, C, seed, dtype="f32", border=2, ties=True, nan_at=None):
    """a seeded image with a gray border of exactly 0.7 (uint8: 178 and 179, which both round to 0.7), values elsewhere
    spread over [0, 1], the ties 0.65 / 0.75 and a few interior gray pixels"""
    rng = np.random.default_rng(seed)
    if dtype == "u8":
        img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        gray = np.array([178, 179, 178, 179][:C], np.uint8)
    else:
        img = rng.random((H, W, C)).astype(f32)
        gray = np.full(C, 0.7, f32)
    if border:
        b = min(border, H, W)
        img[:b], img[H - b:], img[:, :b], img[:, W - b:] = gray, gray, gray, gray
    flat = img.reshape(-1, C)
    n = flat.shape[0]
    if n > 8:
        pick = rng.choice(n, size=max(1, n // 11), replace=False)
        flat[pick] = gray  # gray pixels inside
        if ties and dtype != "u8":
            t = rng.choice(n, size=min(n, 6), replace=False)
            flat[t[0::3]] = f32(0.65)
            flat[t[1::3]] = f32(0.75)
            flat[t[2::3], 0] = f32(0.65)  # one channel on a tie, the others random
    if nan_at is not None and dtype != "u8":
        img[nan_at] = np.nan
    return img


@functools.lru_cache(maxsize=None)
def golden():
    """the recorded runs of the reference's process_image (tests/golden/make_image_golden.py), or None"""
    if not os.path.exists(GOLDEN):
        return None
    z = np.load(GOLDEN)
    n = int(z["n_cases"])
    return [dict(img=z[f"img_{k}"], spots=z[f"spots_{k}"], img_spatial=z[f"img_spatial_{k}"],
                 img_pixels=z[f"img_pixels_{k}"]) for k in range(n)]
