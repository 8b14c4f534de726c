"""Histology images without a device: the numpy yardstick of tests/image_util.py against the recorded runs of the
reference's process_image and against scipy, the C entries' refusals (csrc/image.hip: every one before a launch), the
Python wrappers' ValueErrors, the exports and Frame."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpsa
import spatial_alignment_amd as gp
import image_util as U
from spatial_alignment_amd import image as IM


def _lib():
    from spatial_alignment_amd import _lib as L

    return L


# ------------------------------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------------------------------
def test_yardstick_equals_the_reference_fixture():
    cases = U.golden()
    assert cases is not None and len(cases) == 3
    kept = []
    for c in cases:
        coords, pixels, (n, n_bg, n_out) = U.select(c["img"], 1, 0.7, U.bbox_of(c["spots"]))
        assert coords.dtype == np.float32 and pixels.dtype == np.float32
        assert np.array_equal(coords.astype(np.float64), c["img_spatial"])
        assert np.array_equal(pixels, c["img_pixels"])
        assert n + n_bg + n_out == c["img"].shape[0] * c["img"].shape[1]
        kept.append(n)
    assert kept[0] > 100 and kept[1] > 100 and kept[2] == 0  # the last image: nothing survives


def test_background_rule_is_numpy_round_on_fp32():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.random(200000).astype(np.float32), (np.arange(256) / 255.0).astype(np.float32),
                        np.arange(256, dtype=np.float32) / np.float32(255.0),
                        np.array([0.65, 0.75, 0.7, 0.6500001, 0.7499999, np.nan, np.inf], np.float32)])
    with np.errstate(invalid="ignore"):
        want = np.round(v, 1) == 0.7
    assert np.array_equal(U.is_background(v[:, None], 0.7), want)
    assert want.sum() > 1000 and not U.is_background(np.array([[np.nan]], np.float32), 0.7)[0]
    assert not U.is_background(np.array([[0.7, np.nan, 0.7]], np.float32), 0.7)[0]  # one NaN channel: never background


def test_block_mean_is_the_fp64_mean_rounded_once():
    for (H, W, Cn, b, dt) in ((12, 15, 3, 3, "f32"), (9, 8, 1, 2, "u8"), (7, 11, 4, 3, "f32"), (8, 8, 3, 4, "u8")):
        img = U.tissue_image(H, W, Cn, seed=H * W, dtype=dt)
        v = U.as_values(img).astype(np.float64)
        Ho, Wo = H // b, W // b
        want = v[: Ho * b, : Wo * b].reshape(Ho, b, Wo, b, Cn).mean(axis=(1, 3))
        got = U.block_mean(img, b)
        assert got.shape == (Ho, Wo, Cn) and got.dtype == np.float32
        # numpy's mean adds pairwise, the rule adds in row-major order: both are within b^2 fp64 roundings of the exact
        # mean, far below half an fp32 ulp except on a tie: equal up to one fp32 ulp, and equal nearly everywhere
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - want) <= ulp)
        assert np.mean(got == want.astype(np.float32)) > 0.99
    img = np.arange(16, dtype=np.float32).reshape(4, 4)  # exact sums: the partial blocks are dropped, the centres
    coords, pixels, counts = U.select(np.pad(img, ((0, 1), (0, 1))), 2, None, None)
    assert np.array_equal(pixels[:, 0], [2.5, 4.5, 10.5, 12.5]) and counts == (4, 0, 0)
    assert np.array_equal(coords, [[0.5, 0.5], [2.5, 0.5], [0.5, 2.5], [2.5, 2.5]])


def test_bilinear_equals_scipy_map_coordinates():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    img = rng.random((37, 53, 3))
    xy = np.stack([rng.random(20000) * 52, rng.random(20000) * 36], 1)
    xy[:4] = [[0, 0], [52, 36], [52, 0], [13, 36]]
    val, ok = U.sample64(img, xy, order=1)
    assert ok.all()
    want = np.stack([ndi.map_coordinates(img[:, :, c], [xy[:, 1], xy[:, 0]], order=1) for c in range(3)], 1)
    err = float(np.abs(val - want).max())
    print(f"[image] bilinear yardstick vs scipy.ndimage.map_coordinates: {err:.2e} (bar 1e-13)")
    assert err <= 1e-13
    ints = np.stack([rng.integers(0, 53, 500), rng.integers(0, 37, 500)], 1).astype(np.float64)
    val, ok = U.sample64(img, ints, order=1)
    assert ok.all() and np.array_equal(val, img[ints[:, 1].astype(int), ints[:, 0].astype(int)])
    near, ok = U.sample64(img, np.clip(ints + 0.25, 0, [52, 36]), order=0)  # (beyond the last pixel centre: not valid)
    assert ok.all() and np.array_equal(near, val)


def test_sample_yardstick_edges():
    img = U.tissue_image(5, 7, 2, seed=3, border=0)
    up = lambda t: np.nextafter(t, np.inf)
    xy = np.array([[6.0, 4.0], [-0.0, -0.0], [up(6.0), 1.0], [1.0, up(4.0)], [np.nextafter(0.0, -1.0), 1.0],
                   [np.nan, 1.0], [1.0, np.inf], [-np.inf, 1.0], [2.5, 1.5]])
    out, ok = U.sample(img, xy, order=1, fill=-3.0)
    assert ok.tolist() == [True, True, False, False, False, False, False, False, True]
    assert np.array_equal(out[0], img[4, 6]) and np.array_equal(out[1], img[0, 0]) and np.all(out[2:8] == -3.0)
    one = np.array([[[0.25, 0.5]]], np.float32)  # a 1 x 1 image: the only valid point is (0, 0)
    out, ok = U.sample(one, np.array([[0.0, 0.0], [0.5, 0.0]]), order=1)
    assert ok.tolist() == [True, False] and np.array_equal(out[0], one[0, 0]) and np.isnan(out[1]).all()


# ------------------------------------------------------------------------------------------------------------------------
# the C entries: refusals before any launch, a pure workspace query
# ------------------------------------------------------------------------------------------------------------------------
def test_workspace_query_is_pure():
    lib = _lib().load()
    q = lib.gpsa_image_select_workspace
    T = lambda H, W, b: -(-((H // b) * (W // b)) // 2048)
    for H, W, b in ((1, 1, 1), (2048, 2048, 1), (2000, 2000, 3), (20000, 20000, 1), (64, 4097, 64)):
        need = q(H, W, b)
        assert need == q(H, W, b) and need >= 32 + 20 * T(H, W, b) and need % 8 == 0
        assert need <= 64 + 20 * T(H, W, b)  # nothing of H W elements: 20 bytes per tile of 2048 output pixels
    for H, W, b in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 65), (5, 5, 6), (4, 9, 5), (-1, 5, 1), (65536, 32768, 1)):
        assert q(H, W, b) == 0, (H, W, b)
    assert q(65536, 32767, 1) > 0  # H' W' = 2^31 - 65536


def test_refusals_before_any_launch():
    """argument checks of the image entries run on the host (no device needed)"""
    L = _lib()
    lib = L.load()
    v = C.c_void_p(8)
    box = (C.c_double * 4)(1.0, 5.0, 1.0, 5.0)
    nanbox = (C.c_double * 4)(1.0, float("nan"), 1.0, 5.0)
    need = lib.gpsa_image_select_workspace(16, 24, 2)
    assert need > 0
    for sfx in ("u8", "f32"):
        count, write = getattr(lib, f"gpsa_image_select_count_{sfx}"), getattr(lib, f"gpsa_image_select_write_{sfx}")
        sample = getattr(lib, f"gpsa_image_sample_{sfx}")

        def sel(**kw):
            return (kw.get("img", v), kw.get("H", 16), kw.get("W", 24), kw.get("C", 3), kw.get("bin", 2), 1, 0.7,
                    kw.get("has_bbox", 1), kw.get("bbox", box), kw.get("ws", v), kw.get("bytes", need))

        bad = (dict(img=None), dict(H=0), dict(W=0), dict(H=-3), dict(C=0), dict(C=5), dict(bin=0), dict(bin=65),
               dict(bin=17), dict(H=40, W=3, bin=4), dict(bbox=None), dict(bbox=nanbox),
               dict(H=65536, W=32768, bin=1, bytes=1 << 40))
        for kw in bad:
            assert count(*sel(**kw), None) == L.GPSA_EINVAL, (sfx, kw)
            assert write(*sel(**kw), v, v, 10, None) == L.GPSA_EINVAL, (sfx, kw)
        for kw in (dict(ws=None), dict(bytes=need - 1), dict(bytes=0)):
            assert count(*sel(**kw), None) == L.GPSA_EWORKSPACE, (sfx, kw)
            assert write(*sel(**kw), v, v, 10, None) == L.GPSA_EWORKSPACE, (sfx, kw)
        for coords, pixels, cap in ((None, v, 10), (v, None, 10), (v, v, 0), (v, v, -1)):
            assert write(*sel(), coords, pixels, cap, None) == L.GPSA_EINVAL, (sfx, cap)

        def smp(**kw):
            return (kw.get("img", v), kw.get("H", 5), kw.get("W", 7), kw.get("C", 3), kw.get("xy", v), kw.get("n", 9),
                    kw.get("order", 1), 0.0, kw.get("out", v), kw.get("valid", v), None)

        for kw in (dict(img=None), dict(xy=None), dict(out=None), dict(valid=None), dict(H=0), dict(W=0), dict(C=0),
                   dict(C=5), dict(n=0), dict(n=-1), dict(n=1 << 31), dict(order=2), dict(order=-1)):
            assert sample(*smp(**kw)) == L.GPSA_EINVAL, (sfx, kw)


# ------------------------------------------------------------------------------------------------------------------------
# the Python side
# ------------------------------------------------------------------------------------------------------------------------
def test_exports():
    names = ("Frame", "scale_spatial_coords", "image_pixels", "ImagePixels", "histology_modality", "warp_image")
    for n in names:
        assert n in gp.__all__ and n in gpsa.__all__ and getattr(gpsa, n) is getattr(IM, n)
    from spatial_alignment_amd.util import scale_spatial_coords

    assert scale_spatial_coords is IM.scale_spatial_coords
    assert callable(gp.VariationalGPSA.warp_image)
    for name in ("gpsa_image_select_workspace", "gpsa_image_select_count_u8", "gpsa_image_select_count_f32",
                 "gpsa_image_select_write_u8", "gpsa_image_select_write_f32", "gpsa_image_sample_u8",
                 "gpsa_image_sample_f32"):
        assert name in _lib().SIGNATURES


def test_frame_round_trips():
    fr = gp.Frame(origin=(-3.25, 7.5), step=(0.125, -2.0))
    rng = np.random.default_rng(0)
    P = rng.integers(-50, 5000, (200, 2)).astype(np.float64)
    assert np.array_equal(fr.inverse(fr(P)), P)  # dyadic steps: exact
    fr2 = gp.Frame((1.0 / 3.0, -0.7), (10.0 / 47.0, 10.0 / 39.0))
    Pt = torch.from_numpy(P)
    back = fr2.inverse(fr2(Pt))
    assert torch.is_tensor(back) and back.dtype == torch.float64 and float((back - Pt).abs().max()) < 1e-9
    assert np.allclose(fr2(P), fr2(Pt).numpy(), rtol=0, atol=0)
    assert fr2(torch.tensor([[[2.0, 3.0]]])).shape == (1, 1, 2)
    assert fr == gp.Frame((-3.25, 7.5), (0.125, -2.0)) and fr != fr2 and "Frame(" in repr(fr)
    for kw in (dict(step=(0.0, 1.0)), dict(origin=(float("nan"), 0.0)), dict(step=(1.0, float("inf"))),
               dict(origin=(1.0, 2.0, 3.0)), dict(origin=None)):
        with pytest.raises(ValueError, match="Frame"):
            gp.Frame(**kw)
    with pytest.raises(ValueError, match="last axis"):
        fr(np.zeros((4, 3)))


def test_scale_spatial_coords_is_the_reference_helper():
    rng = np.random.default_rng(2)
    X = rng.random((50, 2)) * [300.0, 170.0] + [12.0, -4.0]
    ref = X - X.min(0)
    ref = ref / ref.max(0) * 10.0  # the reference's three lines
    Xs, fr = gp.scale_spatial_coords(X)
    assert isinstance(fr, gp.Frame) and Xs.dtype == np.float64 and np.abs(Xs - ref).max() < 1e-12
    assert abs(Xs.min()) < 1e-12 and abs(Xs.max() - 10.0) < 1e-12
    Xt, frt = gp.scale_spatial_coords(torch.from_numpy(X).float(), max_val=4.0)
    assert Xt.dtype == torch.float32 and float((Xt.double() - torch.from_numpy(ref) * 0.4).abs().max()) < 1e-5
    other, fr_same = gp.scale_spatial_coords(X[:7] + 1.0, frame=fr)  # someone else's scaling
    assert fr_same is fr and np.abs(other - fr(X[:7] + 1.0)).max() == 0.0
    assert np.abs(fr.inverse(Xs) - X).max() < 1e-9
    for bad in (np.zeros((5, 3)), np.zeros((0, 2)), np.ones((4, 2)), np.array([[0.0, 1.0], [np.nan, 2.0]])):
        with pytest.raises(ValueError, match="scale_spatial_coords"):
            gp.scale_spatial_coords(bad)
    with pytest.raises(ValueError, match="must be a Frame"):
        gp.scale_spatial_coords(X, frame=(0.0, 1.0))


def test_wrappers_raise_value_errors_without_a_device():
    img = np.zeros((6, 8, 3), np.float32)
    spots = np.array([[1.0, 1.0], [5.0, 4.0]])
    with pytest.raises(ValueError, match="spots or bbox, not both"):
        gp.image_pixels(img, spots=spots, bbox=(0, 1, 0, 1))
    for bad, pat in ((np.zeros((6, 8, 5), np.float32), "C in 1..4"), (np.zeros((6,), np.float32), "C in 1..4"),
                     (np.zeros((6, 8, 3), np.int32), "uint8"), ([[0.0]], "tensor or a numpy array")):
        with pytest.raises(ValueError, match=pat):
            gp.image_pixels(bad)
    for kw, pat in ((dict(bin=0), "bin"), (dict(bin=65), "bin"), (dict(bin=1.5), "bin"), (dict(bin=7), "larger than"),
                    (dict(background=float("nan")), "background"), (dict(bbox=(0, 1, 2)), "four numbers"),
                    (dict(bbox=(0, float("nan"), 0, 1)), "four numbers"), (dict(spots=np.zeros((3, 3))), "spots"),
                    (dict(device="cpu"), "GPU only")):
        with pytest.raises(ValueError, match=pat):
            gp.image_pixels(img, **kw)
    with pytest.raises(ValueError, match="entries of spots_list"):
        gp.histology_modality([img, img], [spots])
    with pytest.raises(ValueError, match="n_samples"):
        gp.histology_modality([img], [spots], n_samples=0)
    # the tensor-level wrappers: shape, dtype and device
    from spatial_alignment_amd.ops import HipOps

    o = object.__new__(HipOps)
    t = torch.zeros(6, 8, 3)
    for bad in (t[:, :, :2], t.double(), torch.zeros(6, 8), torch.zeros(6, 8, 5), None):
        with pytest.raises(ValueError, match="contiguous uint8 or fp32"):
            o.image_select(bad)
    with pytest.raises(ValueError, match="run on the device"):
        o.image_select(t)
    with pytest.raises(ValueError, match="run on the device"):
        o.image_sample(t, torch.zeros(4, 2, dtype=torch.float64))


def test_warp_image_refusals_without_a_device():
    from golden_io import Golden
    from model_util import build_model

    model, _ = build_model(Golden("c1_example_fixed0"))
    img = np.zeros((6, 8, 3), np.float32)
    fr = gp.Frame()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    for kw, pat in ((dict(view=2), "view"), (dict(view=-1), "view"), (dict(view=True), "view"),
                    (dict(img_frame=(0, 1)), "img_frame must be a Frame"), (dict(out_frame="x"), "out_frame must be a Frame"),
                    (dict(order=2), "order"), (dict(max_iter=-1), "max_iter"), (dict(max_iter=1.5), "max_iter"),
                    (dict(out_shape=(0, 4)), "out_shape"), (dict(out_shape=5), "out_shape"),
                    (dict(rows_per_chunk=0), "rows_per_chunk")):
        args = dict(view=1, img_frame=fr)
        args.update(kw)
        with pytest.raises(ValueError, match=pat):
            model.warp_image(img, **args)
    with pytest.raises(ValueError, match="GPU only"):  # a model on the host: there is no host path for the image
        model.warp_image(img, 0, img_frame=fr)
    model.kernel_func_warp = lambda *a, **k: None
    with pytest.raises(ValueError, match="built-ins"):
        model.warp_image(img, 1, img_frame=fr)
    one_d, _ = build_model(Golden("c6_one_dim"))
    with pytest.raises(ValueError, match="n_spatial_dims"):
        one_d.warp_image(img, 0, img_frame=fr)
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in state.items())
