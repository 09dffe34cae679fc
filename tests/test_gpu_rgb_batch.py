"""GPU tests of the batched chain of multi-plane (RGB) models: w2xc_convert_planes_batch_device, the RGB image batches, TTA passes and the RGB route of the
RGBA batch -- one launch per layer for a sub-batch of images (conv3x3_first_batch, conv3x3_wino_batch, conv3x3_wino4_batch[_l], conv3x3_last_batch).

No tolerance anywhere: an image of a batch has the bits of the single-image call (which tests/test_gpu_rgb.py gates against the oracle), so every
comparison is equality against that call.  The single-image results are computed once per (model, size, nn2x) and shared.  Every case asserts through
w2xc_batch_plan that it ran the batched way (or, where it is meant to, the fallback)."""
import functools

import numpy as np
import pytest

from tools import gen_model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f
TOPO = {"m7": ([3, 32, 32, 64, 64, 128, 128, 3], 501), "m4": ([3, 32, 64, 64, 3], 502), "m3": ([3, 32, 64, 3], 503), "p64": ([3, 64, 64, 3], 504),
        "p128": ([3, 128, 128, 3], 505), "m5": ([3, 32, 64, 32, 64, 3], 506)}
FIRST_TPW = LAST_TPW = 4       # tiles a workgroup of conv3x3_first / conv3x3_last walks (w2xc_kernels.hip)
GRID = 256                     # w2xc_persistent_grid: workgroups of conv3x3_wino / conv3x3_wino4 at most
# (h, w, n): one pixel; one pixel in the second tile column; odd sizes with more than one tile row
SIZES = [(1, 1, 3), (9, 33, 3), (37, 53, 2)]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@pytest.fixture(scope="module")
def models(gpu):
    return {k: gpu._ModelSet.from_layers(gen_model.synth_layers(*v)) for k, v in TOPO.items()}


def stream():
    return torch.cuda.current_stream()


@functools.lru_cache(maxsize=None)
def planes(h, w, n, seed=0):
    x = np.random.default_rng(1000 + seed + 7 * h + w).random((n, 3, h, w), dtype=np.float32)
    x.setflags(write=False)
    return x


_single = {}


def singles(gpu, models, name, h, w, n, nn2x, **opt):
    """n calls of convert_planes[_nn2x]_device, one per image, on contiguous planes (computed once, shared)"""
    key = (name, h, w, n, nn2x, tuple(sorted(opt.items())))
    if key not in _single:
        ms, x = models[name], planes(h, w, n)
        H, W = h << nn2x, w << nn2x
        out = []
        for i in range(n):
            d_in = torch.from_numpy(np.array(x[i])).cuda()
            d_out = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
            f = ms.convert_planes_nn2x_device if nn2x else ms.convert_planes_device
            f(3, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), H * W * 4, W * 4, stream=stream().cuda_stream, opts=gpu.make_opts(device=0, **opt))
            stream().synchronize()
            out.append(d_out.cpu())
        _single[key] = torch.stack(out)
        assert not torch.isnan(_single[key]).any()
    return _single[key]


def batch(gpu, ms, x, nn2x, pad=(0, 0, 0), **opt):
    """convert_planes_batch_device on x (n, 3, h, w); pad = (floats behind a row, rows behind a plane, floats behind an image) in and out alike.  Returns the
    (n, 3, H, W) results after checking that every guard float around them kept its bits and that the input was not written."""
    n, _, h, w = x.shape
    H, W = h << nn2x, w << nn2x
    pr, pp, pi = pad
    GUARD = -12345.0

    def buf(hh, ww):
        plane = (hh + pp) * (ww + pr)
        return torch.full((n, 3 * plane + pi), GUARD, dtype=torch.float32, device="cuda"), plane

    def view(t, plane, hh, ww):
        return t[:, :3 * plane].view(n, 3, hh + pp, ww + pr)[:, :, :hh, :ww]
    d_in, iplane = buf(h, w)
    view(d_in, iplane, h, w).copy_(torch.from_numpy(np.array(x)))
    before = d_in.clone()
    d_out, oplane = buf(H, W)
    ms.convert_planes_batch_device(n, 3, d_in.data_ptr(), d_in.stride(0) * 4, iplane * 4, (w + pr) * 4, w, h, d_out.data_ptr(), d_out.stride(0) * 4, oplane * 4,
                                   (W + pr) * 4, nn2x=bool(nn2x), stream=stream().cuda_stream, opts=gpu.make_opts(device=0, **opt))
    stream().synchronize()
    assert torch.equal(d_in, before), "the input was written"
    res = view(d_out, oplane, H, W).cpu()
    mask = torch.ones_like(d_out, dtype=torch.bool)
    view(mask, oplane, H, W).fill_(False)
    assert (d_out[mask] == GUARD).all(), "floats outside the output planes were written"
    return res


def tiles8(h, w):
    return ((w + 31) // 32) * ((h + 7) // 8)


# ---- 1. the plane call: bit-identity with the single calls ----
@pytest.mark.parametrize("name", sorted(TOPO))
@pytest.mark.parametrize("nn2x", [0, 1])
def test_planes_batch_equals_single_calls(gpu, models, name, nn2x):
    ms = models[name]
    for (h, w, n), pad in zip(SIZES, [(1, 2, 8), (0, 0, 0), (3, 1, 4)]):   # odd row strides, padded plane / image strides; and the packed layout
        assert ms.batch_plan(3, w, h, bool(nn2x))[0] == 1, (name, h, w)
        want = singles(gpu, models, name, h, w, n, nn2x)
        got = batch(gpu, ms, planes(h, w, n), nn2x, pad)
        assert torch.equal(got, want), (name, h, w, nn2x, float((got - want).abs().max()))


def test_consecutive_tiles_of_a_workgroup_straddle_two_images():
    """every model has a case above whose first layer, and one whose last layer, has a tile count per image that is no multiple of the tiles a workgroup
    walks: with n = 2 or 3 images a workgroup's consecutive tiles then belong to two images.  Layer k of L computes (W + 2 (L - k)) x (H + 2 (L - k))."""
    assert tiles8(18, 66) == 9 and 9 % LAST_TPW != 0            # 9 x 33 at nn2x: 3 x 3 tiles in the last layer
    for name, (topo, _) in TOPO.items():
        L = len(topo) - 1
        first = [tiles8((h << u) + 2 * (L - 1), (w << u) + 2 * (L - 1)) % FIRST_TPW for h, w, n in SIZES for u in (0, 1)]
        last = [tiles8(h << u, w << u) % LAST_TPW for h, w, n in SIZES for u in (0, 1)]
        assert any(first) and any(last), (name, first, last)


def test_workgroups_take_a_second_item_in_another_image(gpu, models):
    """more items than w2xc_persistent_grid gives workgroups: a workgroup of conv3x3_wino / conv3x3_wino4 walks on to an item of another image.  Items of a
    layer: 16 x 32 pixel tiles of its region x 32- (wino) / 64-plane (wino4) blocks; at least ceil(w / 32) ceil(h / 16) of them per image."""
    h, w = 37, 53
    per_image = ((w + 31) // 32) * ((h + 15) // 16)             # (the smallest layer: the last mid layer's region is two pixels larger a side)
    n = GRID // per_image + 1
    assert n * per_image > GRID and per_image < GRID // 8, (n, per_image)   # (an XCD's 32 workgroups step 32 items: past the image they started in)
    for name in ("m7", "m5"):
        assert models[name].batch_plan(3, w, h)[0] == 1
        want = singles(gpu, models, name, h, w, n, 0)
        got = batch(gpu, models[name], planes(h, w, n), 0)
        assert torch.equal(got, want), name


# ---- 2. launch counts ----
def launches(ms):
    return ms.profile_read(0)[1]


def profiled_batch(gpu, ms, n, h, w, nn2x, **opt):
    ms.profile_reset(0)
    batch(gpu, ms, planes(h, w, n), nn2x, profile=1, **opt)
    return launches(ms)


def test_one_launch_per_layer(gpu, models):
    ms, L = models["m7"], 7
    assert ms.batch_plan(3, 64, 64, True)[0] == 1
    assert profiled_batch(gpu, ms, 5, 64, 64, 1) == [1] * L
    assert profiled_batch(gpu, ms, 1, 64, 64, 1) == [1] * L
    # a workspace that holds fewer than five images, but one whole: ceil(5 / sub) launches
    for mb in range(8, 256, 4):
        batched, sub = ms.batch_plan(3, 64, 64, True, gpu.make_opts(workspace_mb=mb))
        if batched and 2 <= sub <= 4:
            break
    else:
        pytest.fail("no workspace_mb with 2 <= sub <= 4")
    print("workspace_mb %d: sub-batches of %d" % (mb, sub))
    assert profiled_batch(gpu, ms, 5, 64, 64, 1, workspace_mb=mb) == [-(-5 // sub)] * L


def u8_images(n, h, w, c=3, seed=0):
    return np.random.default_rng(2000 + seed + 3 * h + w).integers(0, 256, (n, h, w, c)).astype(np.uint8)


def image_batch_device(gpu, imgs, noise, scale, it, shrink=0.0, tta=False, roi=False, **opt):
    """process_image_rgb_u8_batch_device; roi: the images are ROIs of larger byte arrays (odd offsets and strides), guard bytes checked"""
    n, h, w, _ = imgs.shape
    H, W = h << it, w << it
    if shrink:
        W, H = int(float(W * shrink)), int(float(H * shrink))
    il, ir, ol, orr, tail = (7, 4, 5, 6, 11) if roi else (0, 0, 0, 0, 0)
    irs, ors = il + w * 3 + ir, ol + W * 3 + orr
    host = np.full((n, h * irs + tail), 0x5A, np.uint8)
    host[:, :h * irs].reshape(n, h, irs)[:, :, il:il + w * 3] = imgs.reshape(n, h, w * 3)
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((n, H * ors + tail), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.process_image_rgb_u8_batch_device(n, d_in.data_ptr() + il, d_in.stride(0), irs, w, h, d_out.data_ptr() + ol, d_out.stride(0), ors, noise, scale, it, shrink,
                                          stream=stream().cuda_stream, opts=gpu.make_opts(device=0, **opt), tta=tta)
    stream().synchronize()
    b = d_out.cpu().numpy()
    rows = b[:, :H * ors].reshape(n, H, ors)
    guard = np.ones(b.shape, bool)
    guard[:, :H * ors].reshape(n, H, ors)[:, :, ol:ol + W * 3] = False
    assert (b[guard] == 0xAB).all(), "bytes outside the output ROIs were written"
    assert np.array_equal(d_in.cpu().numpy(), host), "the input was written"
    return rows[:, :, ol:ol + W * 3].reshape(n, H, W, 3).copy()


def test_image_batch_launch_counts(gpu, models):
    noise, scale = models["m7"], models["m4"]
    imgs = u8_images(5, 64, 64)
    for m in (noise, scale):
        m.profile_reset(0)
    image_batch_device(gpu, imgs, noise, scale, 2, profile=1)
    assert launches(noise) == [1] * 7 and launches(scale) == [2] * 4      # one launch per layer and pass


@pytest.mark.parametrize("hw", [(64, 64), (48, 64)])
def test_tta_launch_counts(gpu, models, hw):
    h, w = hw
    ms, L = models["m4"], 4
    want = profiled_batch(gpu, ms, 8, h, w, 1) if h == w else [a + b for a, b in zip(profiled_batch(gpu, ms, 4, h, w, 1), profiled_batch(gpu, ms, 4, w, h, 1))]
    assert want == ([1] * L if h == w else [2] * L)
    ms.profile_reset(0)
    gpu.process_image_rgb_u8(u8_images(1, h, w)[0], None, ms, 1, gpu.make_opts(device=0, profile=1), tta=True)
    assert launches(ms) == want


# ---- 3. the image calls ----
IMAGE_CASES = [("scale", None, "m7", 1, 0.0), ("noise_scale", "m7", "m4", 1, 0.0), ("scale2", None, "m4", 2, 0.0), ("ratio1.5", None, "m4", 1, 0.75)]


_single_img = {}


def single_images(gpu, models, case, n, tta=False, **opt):
    name, noise, scale, it, shrink = case
    key = (name, n, tta, tuple(sorted(opt.items())))
    if key not in _single_img:
        imgs = u8_images(5, 37, 53)[:n]
        _single_img[key] = np.stack([gpu.process_image_rgb_u8(imgs[i], models[noise] if noise else None, models[scale] if scale else None, it,
                                                              gpu.make_opts(device=0, **opt), shrink, tta=tta) for i in range(n)])
    return _single_img[key]


@pytest.mark.parametrize("case", IMAGE_CASES, ids=[c[0] for c in IMAGE_CASES])
@pytest.mark.parametrize("n", [2, 5])
def test_image_batch_equals_single_calls(gpu, models, case, n):
    name, noise, scale, it, shrink = case
    imgs = u8_images(5, 37, 53)[:n]
    mn, msc = (models[noise] if noise else None), (models[scale] if scale else None)
    for m, up in ((mn, 0), (msc, it)):
        if m is not None:
            assert m.batch_plan(3, 53 << max(up - 1, 0), 37 << max(up - 1, 0), up > 0)[0] == 1
    for fusion in (gpu.FUSION_AUTO, gpu.FUSION_OFF):   # the uint8-fused first and last layers inside the batch, and the colour kernels around float planes
        want = single_images(gpu, models, case, n, fusion=fusion)
        for roi in (False, True):
            assert np.array_equal(image_batch_device(gpu, imgs, mn, msc, it, shrink, roi=roi, fusion=fusion), want), (name, n, fusion, roi)
    got = gpu.process_image_rgb_u8_batch(imgs, mn, msc, it, gpu.make_opts(device=0), shrink)    # the host form
    assert np.array_equal(got, single_images(gpu, models, case, n, fusion=gpu.FUSION_AUTO)), (name, n)


@pytest.mark.parametrize("n", [2, 5])
def test_image_batch_tta_equals_single_calls(gpu, models, n):
    case = IMAGE_CASES[1]
    name, noise, scale, it, shrink = case
    imgs = u8_images(5, 37, 53)[:n]
    want = single_images(gpu, models, case, n, tta=True)
    assert np.array_equal(image_batch_device(gpu, imgs, models[noise], models[scale], it, shrink, tta=True, roi=True), want)


@pytest.mark.parametrize("n", [2, 5])
def test_rgba_batch_on_rgb_models_equals_single_calls(gpu, models, n):
    h, w, it = 24, 36, 1
    imgs = u8_images(n, h, w, 4, seed=9)
    imgs[:, 3:11, 5:20, 3] = 0                                   # a transparent block: the bleed has work
    imgs[:, 15:, :9, 3] = 0
    noise, scale = models["m4"], models["m7"]
    want = np.stack([gpu.process_image_rgba_u8(imgs[i], noise, scale, it, gpu.make_opts(device=0)) for i in range(n)])
    d_in = torch.from_numpy(imgs).cuda()
    d_out = torch.full((n, 2 * h, 2 * w, 4), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.process_image_rgba_u8_batch_device(n, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), 16 * h * w, 8 * w, noise, scale, it, 0.0, -1,
                                           stream=stream().cuda_stream, opts=gpu.make_opts(device=0))
    stream().synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)


# ---- 4. nothing is read that the call did not write ----
def test_scratch_independence(gpu, models):
    h, w, n = 37, 53, 3
    case = IMAGE_CASES[1]
    name, noise, scale, it, shrink = case
    imgs = u8_images(5, h, w)[:n]
    ref_planes = singles(gpu, models, "m7", h, w, 2, 1)
    ref_img = single_images(gpu, models, case, n, fusion=gpu.FUSION_AUTO)
    ref_tta = single_images(gpu, models, case, 2, tta=True)
    for word in WORDS:
        for m in (models["m7"], models["m4"]):
            assert m.fill_scratch(word, 0) > 0
        assert torch.equal(batch(gpu, models["m7"], planes(h, w, 2), 1), ref_planes), hex(word)
        for m in (models["m7"], models["m4"]):
            m.fill_scratch(word, 0)
        assert np.array_equal(image_batch_device(gpu, imgs, models[noise], models[scale], it, shrink), ref_img), hex(word)
        for m in (models["m7"], models["m4"]):
            m.fill_scratch(word, 0)
        assert np.array_equal(image_batch_device(gpu, imgs[:2], models[noise], models[scale], it, shrink, tta=True), ref_tta), hex(word)


# ---- 5. bands: the batch falls back, with the same bits ----
def test_banded_image_falls_back(gpu, models):
    ms, h, w, n = models["m4"], 37, 53, 3
    o = dict(band_rows=16)
    assert ms.batch_plan(3, w, h, True, gpu.make_opts(**o)) == (0, 1)
    want = singles(gpu, models, "m4", h, w, n, 1)               # (banding-invariant: the banded single call has the bits of the whole one)
    assert torch.equal(singles(gpu, models, "m4", h, w, n, 1, **o), want)
    assert torch.equal(batch(gpu, ms, planes(h, w, n), 1, (1, 0, 4), **o), want)
    assert profiled_batch(gpu, ms, n, h, w, 1, **o)[0] > n      # (more than one launch per image and layer: the bands)
    for mb in (1, 2):
        om = gpu.make_opts(workspace_mb=mb)
        if ms.batch_plan(3, w, h, True, om)[0] == 0:
            assert torch.equal(batch(gpu, ms, planes(h, w, n), 1, workspace_mb=mb), want)
            break
    else:
        pytest.fail("no small workspace_mb bands a 74 x 106 image")
