"""Histology images on the device (csrc/image.hip, image.py) against the numpy yardstick of tests/image_util.py.

Bars:
* select: none - coords, pixels and the three counts are the yardstick's, bit for bit (the rule fixes every rounding);
* sample: 1e-6 max(1, |value|), the project's bar for one fp32 rounding (the yardstick's fp64 value and the kernel's can
  differ in the last fp64 bits only, which moves the fp32 rounding by at most one ulp = 1.2e-7 relative);
* warp_image: bit equality with the same steps done by hand; the linear image within the sample bar.
"""
import numpy as np
import pytest
import torch

import spatial_alignment_amd as gp
import image_util as U
from golden_io import Golden
from model_util import build_model
from warp_util import free_views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = torch.float64
TILE, THREADS, WAVE = 2048, 256, 64  # IMG_SELECT_TILE, IMG_SELECT_THREADS, the wave (csrc/image.hip)
SAMPLE_BAR = 1e-6


def _ops():
    from spatial_alignment_amd import engine as E

    return E.ops()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(t, a):
    """a device tensor against a numpy array: shape, dtype and every bit (a NaN against a NaN)"""
    h = t.cpu().numpy()
    if h.shape != a.shape or h.dtype != a.dtype:
        return False
    nan = np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    same_nan = np.array_equal(np.isnan(h), nan) if a.dtype.kind == "f" else True
    return same_nan and np.array_equal(h[~nan].view(np.uint8), a[~nan].view(np.uint8))


def _check_select(img, bin=1, background=0.7, bbox=None, tag=""):
    """image_pixels on the device == the yardstick, and the same bits on a second call; -> the kept count"""
    coords, pixels, (n, n_bg, n_out) = U.select(img, bin, background, bbox)
    d = _dev(img)
    res = gp.image_pixels(d, bbox=bbox, background=background, bin=bin)
    what = (tag, img.shape, str(img.dtype), bin, background, bbox)
    assert (res.coords.shape[0], res.n_background, res.n_outside) == (n, n_bg, n_out), what
    Cn = 1 if img.ndim == 2 else img.shape[2]
    assert res.shape == (img.shape[0] // bin, img.shape[1] // bin) and tuple(res.pixels.shape) == (n, Cn), what
    assert _same_bits(res.coords, coords), what
    assert _same_bits(res.pixels, pixels), what
    again = gp.image_pixels(d, bbox=bbox, background=background, bin=bin)
    assert torch.equal(again.coords, res.coords) and _same_bits(again.pixels, pixels), what
    assert _same_bits(d, img)  # the image is read, never written
    return n


# the issue's shapes, and one on each side of the wave, the workgroup and the tile in output pixels
SHAPES = [(1, 1), (1, 257), (3, 5), (16, 16), (31, 33), (255, 257),
          (1, WAVE - 1), (1, WAVE), (1, WAVE + 1), (1, THREADS - 1), (1, THREADS), (1, THREADS + 1),
          (1, TILE - 1), (1, TILE), (1, TILE + 1), (2, TILE), (TILE + 1, 1)]


# ------------------------------------------------------------------------------------------------------------------------
# select
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3, 4])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_select_equals_the_yardstick_on_every_shape(dtype, Cn):
    total = 0
    for k, (H, W) in enumerate(SHAPES):
        img = U.tissue_image(H, W, Cn, seed=100 * k + Cn, dtype=dtype, border=1 if min(H, W) > 2 else 0)
        for b in (1, 2, 3):
            if b > min(H, W):
                continue
            bbox = (0.2 * W, 0.9 * W, -1.0, 0.8 * H) if k % 2 else None
            total += _check_select(img, b, 0.7, bbox, "shapes")
    assert total > 1000


def test_select_partial_blocks_at_the_right_and_bottom_edges():
    for dtype in ("u8", "f32"):
        for (H, W, b) in ((7, 9, 2), (8, 10, 3), (130, 67, 3), (65, 129, 64), (6, 7, 5), (11, 6, 4)):
            img = U.tissue_image(H, W, 3, seed=H + W, dtype=dtype, border=0)
            assert H % b or W % b
            n = _check_select(img, b, None, None, "partial blocks")
            assert n == (H // b) * (W // b)
            _check_select(img, b, 0.7, (b - 0.5, W - b, 0.0, H), "partial blocks, rules on")


def test_select_contents():
    H, W = 37, 61
    gray = np.full((H, W, 3), 0.7, np.float32)
    assert _check_select(gray, 1, 0.7, None, "all background") == 0  # n = 0: empty tensors, no write pass
    assert _check_select(gray, 1, None, None, "the rule off") == H * W
    assert _check_select((gray * 255).astype(np.uint8), 2, 0.7, None, "all background u8") == 0
    rnd = np.random.default_rng(0).random((H, W, 3)).astype(np.float32) * 0.6  # below 0.65: no background anywhere
    assert _check_select(rnd, 1, 0.7, None, "no background") == H * W
    assert _check_select(rnd, 1, 0.7, (10.0, 11.0, 0.0, 30.0), "a bbox that keeps nothing") == 0
    assert _check_select(rnd, 1, 0.7, (50.0, 40.0, 0.0, 30.0), "an empty bbox") == 0
    assert _check_select(rnd, 1, 0.7, (np.inf, np.inf, 0.0, 1.0), "an infinite bbox") == 0
    # exactly on pixel coordinates: the comparison is strict, columns 4 and 20, rows 3 and 9 are outside
    assert _check_select(rnd, 1, 0.7, (4.0, 20.0, 3.0, 9.0), "bbox on pixel coordinates") == 15 * 5
    assert _check_select(rnd, 2, 0.7, (0.5, 8.5, 0.5, 4.5), "bbox on block centres") == 3 * 1
    ties = U.tissue_image(H, W, 3, seed=9, dtype="f32", ties=True, nan_at=(5, 7, 1))
    ties[6, 8] = np.nan  # a pixel that is NaN in every channel: kept
    ties[0, 0] = [0.7, np.nan, 0.7]  # on the gray border, one NaN channel: never background
    n = _check_select(ties, 1, 0.7, None, "ties and NaN")
    res = gp.image_pixels(_dev(ties))
    rows = {(int(x), int(y)) for x, y in res.coords.cpu().numpy()}
    assert {(7, 5), (8, 6), (0, 0)} <= rows and n == len(rows)
    _check_select(ties, 3, 0.7, (2.0, 50.0, 2.0, 30.0), "ties and NaN, binned")
    for v in (0.65, 0.75, 0.6500001, 0.7499999, 0.64, 0.76):  # the ties round half to even, after the fp32 product
        one = np.full((2, 2, 1), v, np.float32)
        want = bool(np.round(np.float32(v), 1) == np.float32(0.7))
        assert (_check_select(one, 1, 0.7, None, f"tie {v}") == 0) == want


def test_select_first_and_last_pixel_of_a_tile_and_empty_tiles_between():
    for dtype in ("u8", "f32"):
        W = 5 * TILE + 3
        img = np.full((1, W, 3), 178 if dtype == "u8" else 0.7, np.uint8 if dtype == "u8" else np.float32)
        # tile 0: only its first pixel; tile 1: only its last; tiles 2 and 3: empty; tile 4: first, a wave boundary and
        # last; the short tile 5: its last pixel
        keep = [0, 2 * TILE - 1, 4 * TILE, 4 * TILE + WAVE - 1, 4 * TILE + WAVE, 4 * TILE + THREADS, 5 * TILE - 1, W - 1]
        for j, p in enumerate(keep):
            img[0, p] = (10 + j) if dtype == "u8" else 0.1 + 0.01 * j
        assert _check_select(img, 1, 0.7, None, "sparse tiles") == len(keep)
        res = gp.image_pixels(_dev(img))
        assert res.coords[:, 0].cpu().tolist() == [float(p) for p in keep] and res.n_background == W - len(keep)
        assert _check_select(img.reshape(W, 1, 3), 1, 0.7, None, "sparse tiles, one column") == len(keep)


def test_select_equals_the_reference_fixture():
    cases = U.golden()
    assert cases is not None
    for c in cases:
        res = gp.image_pixels(c["img"], spots=c["spots"])  # a numpy image: uploaded
        assert res.coords.is_cuda and _same_bits(res.coords, c["img_spatial"].astype(np.float32))
        assert _same_bits(res.pixels, c["img_pixels"])
        assert res.coords.shape[0] + res.n_background + res.n_outside == c["img"].shape[0] * c["img"].shape[1]
        two = gp.image_pixels(torch.from_numpy(c["img"][:, :, 0].copy()), spots=torch.from_numpy(c["spots"]))  # [H, W]
        want = U.select(c["img"][:, :, 0], 1, 0.7, U.bbox_of(c["spots"]))
        assert _same_bits(two.coords, want[0]) and _same_bits(two.pixels, want[1])
        dbl = gp.image_pixels(c["img"].astype(np.float64), spots=c["spots"])  # a floating image is taken to fp32
        assert torch.equal(dbl.pixels, res.pixels)


def test_write_with_too_small_a_capacity_writes_nothing():
    """through the C ABI: the write pass reads the kept total back from the workspace of the count pass"""
    import ctypes as C

    from spatial_alignment_amd import _lib as L

    lib = L.load()
    H, W = 40, 53
    img = U.tissue_image(H, W, 3, seed=8, dtype="f32")
    want = U.select(img, 1, 0.7, None)
    n = want[2][0]
    d = _dev(img)
    nbytes = lib.gpsa_image_select_workspace(H, W, 1)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    head = (d.data_ptr(), H, W, 3, 1, 1, 0.7, 0, None, ws.data_ptr(), nbytes)
    assert lib.gpsa_image_select_count_f32(*head, st) == 0
    torch.cuda.synchronize()
    assert ws[:24].view(torch.int64).tolist() == list(want[2])
    coords = torch.full((n + 3, 2), -1.0, device=DEV)
    pixels = torch.full((n + 3, 3), -1.0, device=DEV)
    for cap in (n - 1, 1):
        assert lib.gpsa_image_select_write_f32(*head, coords.data_ptr(), pixels.data_ptr(), cap, st) == L.GPSA_EINVAL
        torch.cuda.synchronize()
        assert bool((coords == -1).all()) and bool((pixels == -1).all())
    assert lib.gpsa_image_select_write_f32(*head, coords.data_ptr(), pixels.data_ptr(), n + 3, st) == 0  # room to spare
    torch.cuda.synchronize()
    assert _same_bits(coords[:n], want[0]) and _same_bits(pixels[:n], want[1])
    assert bool((coords[n:] == -1).all()) and bool((pixels[n:] == -1).all())  # nothing beyond the kept rows


def test_select_memory_is_the_result_and_the_workspace():
    H = W = 2048
    gen = torch.Generator(device=DEV).manual_seed(1)
    img = torch.randint(0, 150, (H, W, 3), dtype=torch.uint8, device=DEV, generator=gen)
    drop = torch.rand(H, W, device=DEV, generator=gen) > 0.1
    img[drop] = 178  # about 90 % gray
    del drop
    from spatial_alignment_amd import _lib as L

    ws = L.load().gpsa_image_select_workspace(H, W, 1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = gp.image_pixels(img)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    n = int(res.coords.shape[0])
    result = res.coords.numel() * 4 + res.pixels.numel() * 4
    print(f"[image] 2048 x 2048 x 3 uint8: kept {n} ({n / (H * W):.1%}), peak {peak} bytes above the inputs; result "
          f"{result}, workspace {ws}")
    assert 0.08 * H * W < n < 0.12 * H * W
    assert peak <= result + ws + (1 << 20)
    host = img.cpu().numpy()
    want = U.select(host, 1, 0.7, None)
    assert _same_bits(res.coords, want[0]) and _same_bits(res.pixels, want[1])


# ------------------------------------------------------------------------------------------------------------------------
# sample
# ------------------------------------------------------------------------------------------------------------------------
def _check_sample(img, xy, order, fill=float("nan")):
    want, ok = U.sample(img, xy, order=order, fill=fill)
    out, valid = _ops().image_sample(_dev(img if img.ndim == 3 else img[:, :, None]), _dev(np.asarray(xy, np.float64)),
                                     order=order, fill=fill)
    assert out.dtype == torch.float32 and valid.dtype == torch.uint8
    assert np.array_equal(valid.cpu().numpy().astype(bool), ok)
    got = out.cpu().numpy()
    assert _same_bits(out[~valid.bool()], want[~ok])  # `fill`, bit for bit
    err = np.abs(got[ok].astype(np.float64) - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    return out, valid, float(err.max()) if ok.any() else 0.0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_sample_equals_the_yardstick(dtype, order):
    rng = np.random.default_rng(7)
    worst = 0.0
    for (H, W, Cn) in ((37, 53, 3), (1, 1, 2), (1, 9, 1), (9, 1, 4), (2, 2, 3)):
        img = U.tissue_image(H, W, Cn, seed=H * W + Cn, dtype=dtype, border=0)
        for n in (1, WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1, 1000):
            xy = np.stack([rng.random(n) * (W + 1) - 0.5, rng.random(n) * (H + 1) - 0.5], 1)  # some rows outside
            worst = max(worst, _check_sample(img, xy, order, fill=-7.5)[2])
    print(f"[image] sample {dtype} order {order} vs the yardstick: {worst:.2e} (bar {SAMPLE_BAR:.0e} of max(1, |value|))")
    assert worst <= SAMPLE_BAR


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_sample_integer_coordinates_edges_and_suffix(dtype):
    H, W, Cn = 23, 31, 3
    img = U.tissue_image(H, W, Cn, seed=4, dtype=dtype, border=0)
    vals = torch.from_numpy(U.as_values(img)).to(DEV)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xy = np.stack([cc.ravel(), rr.ravel()], 1).astype(np.float64)
    for order in (0, 1):  # integer coordinates: the pixels themselves
        out, valid, _ = _check_sample(img, xy, order)
        assert valid.all() and torch.equal(out.view(H, W, Cn), vals)
    up, down = (lambda t: np.nextafter(t, np.inf)), (lambda t: np.nextafter(t, -np.inf))
    edge = np.array([[W - 1.0, H - 1.0], [W - 1.0, 0.0], [0.0, H - 1.0], [-0.0, -0.0], [W - 1.0, 3.25], [4.5, H - 1.0],
                     [up(W - 1.0), 1.0], [1.0, up(H - 1.0)], [down(0.0), 1.0], [1.0, down(0.0)], [np.nan, 1.0],
                     [1.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [-np.inf, np.inf], [down(W - 1.0), down(H - 1.0)]])
    for order in (0, 1):
        for fill in (float("nan"), -0.0, 3.5):
            out, valid, err = _check_sample(img, edge, order, fill)
            assert valid.cpu().tolist() == [1] * 6 + [0] * 9 + [1] and err <= SAMPLE_BAR
            assert torch.equal(out[0], vals[H - 1, W - 1]) and torch.equal(out[3], vals[0, 0])
            bad = out[6:15].cpu().numpy()
            assert np.array_equal(bad.view(np.uint32), np.full(bad.shape, fill, np.float32).view(np.uint32))
    one = U.tissue_image(1, 1, 2, seed=1, dtype=dtype, border=0)  # a 1 x 1 image
    out, valid, _ = _check_sample(one, np.array([[0.0, 0.0], [-0.0, 0.0], [0.5, 0.0], [0.0, up(0.0)]]), 1)
    assert valid.cpu().tolist() == [1, 1, 0, 0] and torch.equal(out[0].cpu(), torch.from_numpy(U.as_values(one))[0, 0])
    # a row's result depends on neither the other rows nor n: a suffix gives the same bits
    rng = np.random.default_rng(1)
    xy = np.stack([rng.random(777) * (W + 1) - 1, rng.random(777) * (H + 1) - 1], 1)
    full, vfull, _ = _check_sample(img, xy, 1)
    for start in (1, 64, 300, 776):
        part, vpart, _ = _check_sample(img, xy[start:], 1)
        assert _same_bits(part, full[start:].cpu().numpy()) and torch.equal(vpart, vfull[start:])


# ------------------------------------------------------------------------------------------------------------------------
# warp_image
# ------------------------------------------------------------------------------------------------------------------------
def _model_and_frame(case, H, W):
    g = Golden(case)
    model, dd = build_model(g, device=DEV)
    X = dd[g.mods[0]]["spatial_coords"].double()
    lo, hi = X.min(0).values.cpu(), X.max(0).values.cpu()
    frame = gp.Frame(origin=lo.tolist(), step=[float(hi[0] - lo[0]) / (W - 1), float(hi[1] - lo[1]) / (H - 1)])
    return g, model, frame


def _grid(Ho, Wo):
    rr, cc = torch.meshgrid(torch.arange(Ho, dtype=f64, device=DEV), torch.arange(Wo, dtype=f64, device=DEV), indexing="ij")
    return torch.stack([cc.reshape(-1), rr.reshape(-1)], 1)


def _linear_image(H, W):
    """[H, W, 3], linear in the pixel coordinates with small integer coefficients: bilinear interpolation is exact on it"""
    coef = np.array([[3.0, 2.0, -1.0], [-5.0, 1.0, 4.0], [7.0, -3.0, 2.0]])  # per channel: a + b x + d y
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    img = np.stack([a + b * cc + d * rr for a, b, d in coef], 2).astype(np.float32)
    return img, coef


def test_warp_image_of_a_fixed_view_is_the_image():
    H, W = 13, 17
    g, model, frame = _model_and_frame("c1_example_fixed0", H, W)
    assert 0 not in free_views(g)
    img = U.tissue_image(H, W, 3, seed=2, dtype="f32", border=0)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    res = model.warp_image(img, 0, img_frame=frame)
    assert tuple(res.image.shape) == (H, W, 3) and res.image.dtype == torch.float32 and res.valid.dtype == torch.bool
    assert res.residual.dtype == f64 and tuple(res.residual.shape) == (H, W) and tuple(res.valid.shape) == (H, W)
    err = float(((res.image.cpu().double() - torch.from_numpy(img).double()).abs()
                 / torch.from_numpy(img).double().abs().clamp_min(1.0)).max())
    print(f"[image] warp_image of a fixed view vs the image: {err:.2e} (bar {SAMPLE_BAR:.0e})")
    assert err <= SAMPLE_BAR and bool(res.valid.all()) and int(res.n_unconverged) == 0 and int(res.n_outside) == 0
    assert float(res.residual.abs().max()) == 0.0
    u8 = model.warp_image((img * 255).astype(np.uint8), 0, img_frame=frame, order=0, rows_per_chunk=2)
    assert torch.equal(u8.image.cpu(), torch.from_numpy(U.as_values((img * 255).astype(np.uint8))))
    # another output frame: twice the resolution, shifted by a pixel
    out_frame = gp.Frame([frame.origin[0] + frame.step[0], frame.origin[1]], [frame.step[0] / 2, frame.step[1] / 2])
    res2 = gp.warp_image(model, img, 0, img_frame=frame, out_frame=out_frame, out_shape=(9, 40))
    xy = (_grid(9, 40) * 0.5 + torch.tensor([1.0, 0.0], dtype=f64, device=DEV)).cpu().numpy()
    want, ok = U.sample(img, xy, order=1)
    got = res2.image.view(-1, 3).cpu().numpy()
    assert np.array_equal(res2.valid.view(-1).cpu().numpy(), ok) and int(res2.n_outside) == int((~ok).sum()) > 0
    assert np.isnan(got[~ok]).all()
    assert float((np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max()) <= SAMPLE_BAR
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in state.items())


@pytest.mark.parametrize("case", ["c1_example_fixed0", "c2_three_free_views"])
def test_warp_image_of_a_free_view_is_unwarp_then_sample(case):
    H, W = 12, 15
    g, model, frame = _model_and_frame(case, H, W)
    img = U.tissue_image(H, W, 3, seed=5, dtype="f32", border=0)
    lin, coef = _linear_image(H, W)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    # the default frames, and an output grid that reaches beyond the slice on every side
    wide = gp.Frame([frame.origin[0] - 2 * frame.step[0], frame.origin[1] - 2 * frame.step[1]],
                    [frame.step[0] * 1.5, frame.step[1] * 1.5])
    for view in free_views(g):
        for out_frame, out_shape in ((None, None), (wide, (11, 14))):
            Ho, Wo = out_shape or (H, W)
            res = model.warp_image(img, view, img_frame=frame, out_frame=out_frame, out_shape=out_shape)
            # by hand
            G = (out_frame or frame)(_grid(Ho, Wo))
            uw = model.unwarp(G, view)
            xy = frame.inverse(uw.X)
            vals, inside = _ops().image_sample(_dev(img), xy.contiguous(), order=1, fill=float("nan"))
            what = (case, view, out_shape)
            assert _same_bits(res.image.view(-1, 3), vals.cpu().numpy()), what
            assert torch.equal(res.valid.view(-1), uw.converged & inside.bool()), what
            assert torch.equal(res.residual.view(-1), uw.residual), what
            assert int(res.n_unconverged) == int((~uw.converged).sum()), what
            assert int(res.n_outside) == int((uw.converged & ~inside.bool()).sum()), what
            assert int(res.valid.sum()) > 0.3 * Ho * Wo, what  # (the comparison is about something)
            for rows in (1, 5, Ho):  # the chunking changes no bit
                part = model.warp_image(img, view, img_frame=frame, out_frame=out_frame, out_shape=out_shape,
                                        rows_per_chunk=rows)
                assert _same_bits(part.image, res.image.cpu().numpy()) and torch.equal(part.valid, res.valid), (what, rows)
                assert torch.equal(part.residual, res.residual), (what, rows)
            # the linear image: exact under bilinear interpolation, so every valid pixel is the linear form at xy
            rl = model.warp_image(lin, view, img_frame=frame, out_frame=out_frame, out_shape=out_shape)
            ok = rl.valid.view(-1).cpu().numpy()
            p = xy.cpu().numpy()[ok]
            want = coef[:, 0][None, :] + p[:, :1] * coef[:, 1][None, :] + p[:, 1:] * coef[:, 2][None, :]
            got = rl.image.view(-1, 3).cpu().numpy()[ok].astype(np.float64)
            err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
            print(f"[image] {case} view {view} {out_shape}: linear image {err:.2e} (bar {SAMPLE_BAR:.0e}), "
                  f"{int(ok.sum())} of {Ho * Wo} valid")
            assert err <= SAMPLE_BAR, what
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in state.items())


# ------------------------------------------------------------------------------------------------------------------------
# histology_modality
# ------------------------------------------------------------------------------------------------------------------------
def test_histology_modality_on_two_simulated_images():
    H, W = 40, 48
    imgs = [U.tissue_image(H, W, 3, seed=s, dtype="f32", border=3) for s in (21, 22)]
    rng = np.random.default_rng(3)
    spots = [np.stack([rng.random(60) * (W - 8) + 4, rng.random(60) * (H - 8) + 4], 1) for _ in imgs]
    want = [U.select(im, 1, 0.7, U.bbox_of(sp)) for im, sp in zip(imgs, spots)]
    full = gp.histology_modality(imgs, spots)
    assert full["n_samples_list"] == [w[2][0] for w in want] == full["n_pixels"]
    assert full["n_background"] == [w[2][1] for w in want] and full["n_outside"] == [w[2][2] for w in want]
    assert full["shapes"] == [(H, W), (H, W)]
    assert _same_bits(full["pixel_coords"], np.concatenate([w[0] for w in want]))
    assert _same_bits(full["outputs_rgb"], np.concatenate([w[1] for w in want]))
    n_samples = 300
    assert min(full["n_samples_list"]) > n_samples
    gen = lambda: torch.Generator(device=DEV).manual_seed(17)
    res = gp.histology_modality(imgs, spots, n_samples=n_samples, generator=gen())
    assert res["n_samples_list"] == [n_samples, n_samples] and res["n_pixels"] == full["n_pixels"]
    assert tuple(res["spatial_coords"].shape) == (2 * n_samples, 2) and tuple(res["outputs"].shape) == (2 * n_samples, 3)
    assert res["spatial_coords"].dtype == torch.float32 and res["outputs"].dtype == torch.float32
    again = gp.histology_modality(imgs, spots, n_samples=n_samples, generator=gen())
    for k in ("spatial_coords", "outputs", "outputs_rgb", "pixel_coords"):
        assert torch.equal(res[k], again[k]), k
    other = gp.histology_modality(imgs, spots, n_samples=n_samples, generator=torch.Generator(device=DEV).manual_seed(18))
    assert not torch.equal(res["pixel_coords"], other["pixel_coords"])
    a = 0
    for v, (im, w) in enumerate(zip(imgs, want)):
        rows = slice(a, a + n_samples)
        a += n_samples
        px = res["pixel_coords"][rows].cpu().numpy()
        flat = px[:, 1].astype(np.int64) * W + px[:, 0].astype(np.int64)
        assert np.all(np.diff(flat) > 0)  # a subset without replacement, in image order
        ref_flat = w[0][:, 1].astype(np.int64) * W + w[0][:, 0].astype(np.int64)
        at = np.searchsorted(ref_flat, flat)
        assert np.array_equal(ref_flat[at], flat)  # ... of the yardstick's rows
        assert _same_bits(res["outputs_rgb"][rows], w[1][at])  # ... with their values
        # the frame maps the model coordinates back to the pixel indices
        back = res["frames"][v].inverse(res["spatial_coords"][rows])
        assert torch.equal(torch.round(back).cpu(), torch.from_numpy(px).double())
        assert float((back.cpu() - torch.from_numpy(px).double()).abs().max()) < 1e-4
        sc = res["spatial_coords"][rows].double()
        assert float(sc.min()) == 0.0 and abs(float(sc.max()) - 10.0) < 1e-6
        z = res["outputs"][rows].double()
        mean, std = z.mean(0).abs().max(), (z.std(0, unbiased=False) - 1).abs().max()
        print(f"[image] view {v}: |mean| {float(mean):.1e}, |std - 1| {float(std):.1e} (bar 1e-6)")
        assert float(mean) <= 1e-6 and float(std) <= 1e-6
    raw = gp.histology_modality(imgs, spots, n_samples=n_samples, generator=gen(), standardize=False)
    assert torch.equal(raw["outputs"], res["outputs_rgb"]) and torch.equal(raw["outputs_rgb"], res["outputs_rgb"])
    # the dict is what the model's data_dict takes
    dd = {"histology": {k: res[k] for k in ("spatial_coords", "outputs", "n_samples_list")}}
    model = gp.VariationalGPSA(dd, m_X_per_view=9, m_G=9, data_init=True, n_latent_gps={"histology": None},
                               fixed_view_idx=0).to(DEV)
    assert model.n_views == 2
    with pytest.raises(ValueError, match="keeps no pixel"):
        gp.histology_modality([np.full((6, 6, 3), 0.7, np.float32)], None)
