"""GPU tests of the batch and TTA forms of upconv head models (revision 0.4.1.6.1): w2xc_convert_planes_up2x_batch_device and
w2xc_process_image_rgb_u8_up2x_batch[_device].  Every comparison is EQUALITY, to the bit or byte, against the single-image calls
(w2xc_convert_planes_up2x_device, w2xc_process_image_rgb_u8_ex_device) -- those are gated against float64 in tests/test_gpu_upconv.py -- and, for TTA,
against the route composed from the public building blocks.  Single-image results are computed once per (model, size, options) and shared."""
import functools

import numpy as np
import pytest

from tools import gen_model
import upconv_ref as ur

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f
GUARD = -7.25
# name -> (3x3 planes, head planes out, seed): the published topology, the shortest three-plane head model, a one-plane head model (no batched chain)
TOPO = {"pub": (ur.PUBLISHED, 3, gen_model.SEEDS["upconv7"]), "c32": ([3, 32], 3, 401), "c64y": ([1, 32, 64], 1, 402), "noise": ([3, 32, 32, 3], None, 403)}
# (model, h, w, n): one pixel, odd sizes below a tile, 5 x 3 head tiles with interior ones
PLANES = [(m, h, w, n) for m in ("pub", "c32", "c64y") for h, w, n in ((1, 1, 3), (17, 33, 2), (40, 70, 3))]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@functools.lru_cache(maxsize=None)
def arrays(name):
    planes, nout, seed = TOPO[name]
    if nout is None:
        return gen_model.synth_layers(planes, seed), None
    return ur.head_model(planes, nout, seed)


@pytest.fixture(scope="module")
def models(gpu):
    return {k: gpu._ModelSet.from_layers(arrays(k)[0], head=arrays(k)[1]) for k in TOPO}


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def sources(name, h, w, n):
    """n images of the model's input planes on the device, [n, nin, h, w]"""
    nin = arrays(name)[0][0][0]
    return torch.from_numpy(np.random.default_rng(7 * h + 1000 * w + n).random((n, nin, h, w), dtype=np.float32)).cuda()


def nout_of(ms):
    return ms.planes(ms.n_layers - 1)[1]


def single_planes(gpu, ms, xs, **opt):
    """w2xc_convert_planes_up2x_device on each image of xs [n, nin, h, w] -> [n, nout, 2h, 2w]"""
    n, nin, h, w = xs.shape
    out = torch.empty((n, nout_of(ms), 2 * h, 2 * w), dtype=torch.float32, device="cuda")
    for i in range(n):
        ms.convert_planes_up2x_device(nin, xs[i].data_ptr(), h * w * 4, w * 4, w, h, out[i].data_ptr(), 4 * h * w * 4, 2 * w * 4, stream=stream(),
                                      opts=gpu.make_opts(device=0, **opt))
    torch.cuda.synchronize()
    return out


_single_cache = {}


def single_planes_once(gpu, models, name, h, w, n):
    key = (name, h, w, n)
    if key not in _single_cache:
        _single_cache[key] = single_planes(gpu, models[name], sources(name, h, w, n))
    return _single_cache[key]


def batch_planes(gpu, ms, xs, padded=False, **opt):
    """w2xc_convert_planes_up2x_batch_device on xs [n, nin, h, w] -> [n, nout, 2h, 2w].  padded: rows, planes and images lie farther apart than they need
    to (odd row strides, a guard row per plane, a guard plane per image), the output pre-filled with a guard value that must survive everywhere outside
    the planes; the input must come back as it was either way."""
    n, nin, h, w = xs.shape
    nout = nout_of(ms)
    ip, ir, ic = (1, 2, 3) if padded else (0, 0, 0)
    op, orr, oc = (1, 3, 5) if padded else (0, 0, 0)
    d_in = torch.full((n, nin + ip, h + ir, w + ic), 0.5, dtype=torch.float32, device="cuda")
    d_in[:, :nin, :h, :w] = xs
    before = d_in.clone()
    d_out = torch.full((n, nout + op, 2 * h + orr, 2 * w + oc), GUARD, dtype=torch.float32, device="cuda")
    ms.convert_planes_up2x_batch_device(n, nin, d_in.data_ptr(), d_in.stride(0) * 4, d_in.stride(1) * 4, d_in.stride(2) * 4, w, h, d_out.data_ptr(),
                                        d_out.stride(0) * 4, d_out.stride(1) * 4, d_out.stride(2) * 4, stream=stream(), opts=gpu.make_opts(device=0, **opt))
    torch.cuda.synchronize()
    assert torch.equal(d_in, before), "the input planes were written"
    got = d_out[:, :nout, :2 * h, :2 * w].clone()
    d_out[:, :nout, :2 * h, :2 * w] = GUARD
    assert bool((d_out == GUARD).all()), "floats outside the output planes were written"
    return got


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. the plane batch equals the single calls ----
@pytest.mark.parametrize("name,h,w,n", PLANES, ids=["%s-%dx%d-n%d" % c for c in PLANES])
def test_plane_batch_equals_single_calls(gpu, models, name, h, w, n):
    ms = models[name]
    assert ms.batch_plan(arrays(name)[0][0][0], w, h, up2x=True)[0] == (0 if name == "c64y" else 1)
    want = single_planes_once(gpu, models, name, h, w, n)
    assert bool(torch.isfinite(want).all())
    for padded in (True, False):
        assert same_bits(batch_planes(gpu, ms, sources(name, h, w, n), padded), want), ("padded" if padded else "packed")


# ---- 2. a workgroup's run of head tiles straddles two images ----
def test_head_tile_run_straddles_two_images(gpu, models):
    h, w, n = 65, 600, 3
    tiles = -(-h // 8) * -(-w // 32)             # upconv4x4_head: tiles of 8 x 32 source pixels
    assert (-(-h // 8), -(-w // 32), tiles) == (9, 19, 171)
    total = n * tiles
    grid = min(total, 512)                       # w2xc_upconv_grid
    per = -(-total // grid)
    assert total == 513 and grid == 512 and per == 2
    # runs are [2 r, 2 r + 2): 171 is odd, so run 85 = tiles 170, 171 = the last tile of image 0 and the first of image 1 (the prefetch changes image there),
    # and run 171 = tiles 342, 343 does the same between images 1 and 2
    assert (170 // per == 171 // per) and 170 // tiles == 0 and 171 // tiles == 1
    assert (342 // per == 343 // per) and 341 // tiles == 1 and 342 // tiles == 2
    xs = sources("c32", h, w, n)
    assert same_bits(batch_planes(gpu, models["c32"], xs), single_planes(gpu, models["c32"], xs))


# ---- 3. the 128 -> 256 layer takes a second item in another image ----
def test_wide_layer_walks_items_of_another_image(gpu, models):
    h, w, n, layers = 40, 70, 8, 7
    k = layers - 1                                # the 128 -> 256 layer is layer 6 of 7
    out_w = w + 2 * (layers - k)
    top, bottom = max(-(layers - k), 0 - 4 * (layers - k)), min(h + (layers - k), ((h + 3) & ~3) + 4 * (layers - k))   # RowPlan::region, HL = 4
    out_h, py = bottom - top, top & 3
    tiles_x, tiles_y = -(-out_w // 32), (out_h + py + 15) // 16
    items = tiles_x * tiles_y * (256 // 64)
    assert (tiles_x, tiles_y, items) == (3, 3, 36)
    total = n * items
    grid = min(256, (total + 7) & ~7)             # w2xc_persistent_grid(items, per_cu = 1)
    assert total == 288 and grid == 256 and total > grid
    xs = sources("pub", h, w, n)
    assert same_bits(batch_planes(gpu, models["pub"], xs), single_planes(gpu, models["pub"], xs))


# ---- 4. launch counts ----
def launches(ms):
    return ms.profile_read(0)[1]


def profiled(gpu, ms, name, n, h, w, **opt):
    ms.profile_reset(0)
    batch_planes(gpu, ms, sources(name, h, w, n), profile=1, **opt)
    return launches(ms)


def test_one_launch_per_layer(gpu, models):
    ms, L = models["pub"], 7
    assert profiled(gpu, ms, "pub", 5, 64, 64) == [1] * L
    assert profiled(gpu, ms, "pub", 1, 64, 64) == [1] * L
    assert profiled(gpu, models["c32"], "c32", 5, 17, 33) == [1] * 2
    # a workspace that holds fewer than five images, but one whole: ceil(5 / sub) launches per layer
    for mb in range(8, 256, 4):
        batched, sub = ms.batch_plan(3, 64, 64, up2x=True, opts=gpu.make_opts(workspace_mb=mb))
        if batched and 2 <= sub <= 4:
            break
    else:
        pytest.fail("no workspace_mb with 2 <= sub <= 4")
    print("workspace_mb %d: sub-batches of %d" % (mb, sub))
    assert profiled(gpu, ms, "pub", 5, 64, 64, workspace_mb=mb) == [-(-5 // sub)] * L
    assert same_bits(batch_planes(gpu, ms, sources("pub", 64, 64, 5), workspace_mb=mb), batch_planes(gpu, ms, sources("pub", 64, 64, 5)))


def test_fallback_model_launches_per_image(gpu, models):
    assert profiled(gpu, models["c64y"], "c64y", 3, 17, 33) == [3] * 3
    assert profiled(gpu, models["pub"], "pub", 3, 17, 33, kernel=1) == [3] * 7   # W2XC_KERNEL_DIRECT: no batched chain


# ---- 5. the image call ----
def u8_images(n, h, w, seed=0):
    return np.random.default_rng(3000 + seed + 3 * h + w).integers(0, 256, (n, h, w, 3)).astype(np.uint8)


def final_size(h, w, it, shrink):
    H, W = h << it, w << it
    if shrink:
        W, H = int(float(W * shrink)), int(float(H * shrink))
    return H, W


def image_single(gpu, img, noise, scale, it, shrink=0.0, **opt):
    h, w, _ = img.shape
    H, W = final_size(h, w, it, shrink)
    d_in = torch.from_numpy(img).cuda()
    d_out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    gpu.process_image_rgb_u8_device(d_in.data_ptr(), w * 3, w, h, d_out.data_ptr(), W * 3, noise, scale, it, shrink, stream=stream(),
                                    opts=gpu.make_opts(device=0, **opt))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def image_batch(gpu, imgs, noise, scale, it, shrink=0.0, tta=False, **opt):
    """w2xc_process_image_rgb_u8_up2x_batch_device on ROIs of larger byte arrays (odd offsets and strides); the bytes around the output images must stay"""
    n, h, w, _ = imgs.shape
    H, W = final_size(h, w, it, shrink)
    il, ir, ol, orr, tail = 7, 4, 5, 6, 11
    irs, ors = il + w * 3 + ir, ol + W * 3 + orr
    host = np.full((n, h * irs + tail), 0x5A, np.uint8)
    for i in range(n):
        host[i, :h * irs].reshape(h, irs)[:, il:il + w * 3] = imgs[i].reshape(h, w * 3)
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((n, H * ors + tail), 0xA5, dtype=torch.uint8, device="cuda")
    gpu.process_image_rgb_u8_up2x_batch_device(n, d_in.data_ptr() + il, d_in.stride(0), irs, w, h, d_out.data_ptr() + ol, d_out.stride(0), ors, noise, scale,
                                               it, shrink, stream=stream(), opts=gpu.make_opts(device=0, **opt), tta=tta)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), host), "the input images were written"
    out = d_out.cpu().numpy()
    rows = out[:, :H * ors].reshape(n, H, ors)
    assert (rows[:, :, :ol] == 0xA5).all() and (rows[:, :, ol + W * 3:] == 0xA5).all() and (out[:, H * ors:] == 0xA5).all(), "bytes outside the output images were written"
    return np.ascontiguousarray(rows[:, :, ol:ol + W * 3]).reshape(n, H, W, 3)


# (noise model, iterations, shrink, options)
IMAGE_CASES = {
    "scale": (None, 1, 0.0, {}),
    "noise-scale": ("noise", 1, 0.0, {}),
    "x4": (None, 2, 0.0, {}),
    "ratio1.5": (None, 1, 0.75, {}),
    "fusion-off": ("noise", 1, 0.0, {"fusion": 1}),
    "banded": (None, 1, 0.0, {"band_rows": 4}),
}


@pytest.mark.parametrize("h,w", [(13, 21), (17, 33)])
@pytest.mark.parametrize("case", list(IMAGE_CASES))
def test_image_batch_equals_single_calls(gpu, models, case, h, w):
    noise, it, shrink, opt = IMAGE_CASES[case]
    nm, sc = (models[noise] if noise else None), models["pub"]
    if case == "banded":
        assert sc.plan_rows(w, h, opts=gpu.make_opts(**opt)).n_bands > 1 and sc.batch_plan(3, w, h, up2x=True, opts=gpu.make_opts(**opt))[0] == 0
    imgs = u8_images(5, h, w)
    want = np.stack([image_single(gpu, imgs[i], nm, sc, it, shrink, **opt) for i in range(5)])
    assert 0.2 < ((want > 0) & (want < 255)).mean()   # (not saturated images)
    for n in (1, 2, 5):
        assert np.array_equal(image_batch(gpu, imgs[:n], nm, sc, it, shrink, **opt), want[:n]), n
    if case in ("scale", "noise-scale"):   # the host form
        for n in (1, 2, 5):
            got = gpu.process_image_rgb_u8_up2x_batch(list(imgs[:n]), nm, sc, it, gpu.make_opts(**opt), shrink)
            assert np.array_equal(got, want[:n]), ("host", n)


def test_image_batch_launch_counts(gpu, models):
    noise, scale = models["noise"], models["pub"]
    for m in (noise, scale):
        m.profile_reset(0)
    image_batch(gpu, u8_images(5, 17, 33), noise, scale, 2, profile=1)
    assert launches(noise) == [1] * 3 and launches(scale) == [2] * 7      # one launch per layer and pass


# ---- 6. TTA ----
def tta_composed(gpu, ms, img):
    """u8 -> planes -> spread -> the head model on each of the 8 variants -> gather -> u8, from the public building blocks"""
    h, w, _ = img.shape
    ps, PS = h * w, 4 * h * w
    st = stream()
    d_img = torch.from_numpy(img).cuda()
    d_x = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    v_in = torch.empty((2, 4 * 3 * ps), dtype=torch.float32, device="cuda")     # the upright group, the transposed group
    v_out = torch.empty((2, 4 * 3 * PS), dtype=torch.float32, device="cuda")
    d_y = torch.empty((3, 2 * h, 2 * w), dtype=torch.float32, device="cuda")
    d_o = torch.empty((2 * h, 2 * w, 3), dtype=torch.uint8, device="cuda")
    gpu.u8_to_rgb_device(d_img.data_ptr(), w * 3, w, h, d_x.data_ptr(), st)
    gpu.tta_spread_device(d_x.data_ptr(), 3, ps * 4, w * 4, w, h, v_in[0].data_ptr(), v_in[1].data_ptr(), ps * 4, st)
    opts = gpu.make_opts(device=0)
    for k in range(8):
        g, vw, vh = k >> 2, (h if k & 4 else w), (w if k & 4 else h)   # variant k: planes (k & 3) * 3 .. + 2 of its group, vw x vh
        ms.convert_planes_up2x_device(3, v_in[g].data_ptr() + (k & 3) * 3 * ps * 4, ps * 4, vw * 4, vw, vh, v_out[g].data_ptr() + (k & 3) * 3 * PS * 4, PS * 4,
                                      2 * vw * 4, stream=st, opts=opts)
    gpu.tta_gather_device(v_out[0].data_ptr(), v_out[1].data_ptr(), PS * 4, 3, 2 * w, 2 * h, d_y.data_ptr(), PS * 4, 2 * w * 4, st)
    gpu.rgb_to_u8_device(d_y.data_ptr(), 2 * w, 2 * h, d_o.data_ptr(), 2 * w * 3, st)
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


@pytest.mark.parametrize("h,w", [(24, 24), (17, 33)], ids=["square-8", "4+4"])
def test_tta_equals_the_composed_route(gpu, models, h, w):
    ms = models["pub"]
    imgs = u8_images(2, h, w, seed=1)
    want = np.stack([tta_composed(gpu, ms, imgs[i]) for i in range(2)])
    assert 0.2 < ((want > 0) & (want < 255)).mean()
    assert not np.array_equal(want[0], image_single(gpu, imgs[0], None, ms, 1))   # (TTA changes bytes: the comparison below is not the plain call's)
    for n in (1, 2):
        assert np.array_equal(image_batch(gpu, imgs[:n], None, ms, 1, tta=True), want[:n]), n
    assert np.array_equal(gpu.process_image_rgb_u8_up2x_batch(list(imgs[:1]), None, ms, 1, None, 0.0, tta=True), want[:1])   # host, n = 1
    # the variants are the images of a head batch: one launch per layer for the group of 8, two for 4 + 4
    ms.profile_reset(0)
    image_batch(gpu, imgs[:1], None, ms, 1, tta=True, profile=1)
    assert launches(ms) == [1 if h == w else 2] * 7


# ---- 7. poisoned scratch ----
def test_poisoned_scratch_changes_nothing(gpu, models):
    ms, noise = models["pub"], models["noise"]
    xs, imgs = sources("pub", 17, 33, 2), u8_images(2, 17, 33, seed=2)
    planes = batch_planes(gpu, ms, xs)
    picture = image_batch(gpu, imgs, noise, ms, 1, 0.75)
    tta = image_batch(gpu, imgs, None, ms, 1, tta=True)
    for word in WORDS:
        assert ms.fill_scratch(word) > 0
        assert same_bits(batch_planes(gpu, ms, xs), planes), hex(word)
        assert ms.fill_scratch(word) > 0 and noise.fill_scratch(word) > 0
        assert np.array_equal(image_batch(gpu, imgs, noise, ms, 1, 0.75), picture), hex(word)
        assert ms.fill_scratch(word) > 0
        assert np.array_equal(image_batch(gpu, imgs, None, ms, 1, tta=True), tta), hex(word)


# ---- 8. the CLI: a size group is ONE call of the head batch function, --tta 1 goes there too ----
def test_cli_routes_groups_and_tta_to_the_head_batch_call(gpu, models, tmp_path, monkeypatch):
    from PIL import Image
    from tools import w2xc_cli
    gen_model.write_json(arrays("c32")[0], str(tmp_path / "scale2.0x_model.json"), head=arrays("c32")[1])
    rng = np.random.default_rng(21)
    pics = {"a.png": (12, 20), "b.png": (12, 20), "c.png": (9, 9)}
    imgs = {f: rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for f, (h, w) in pics.items()}
    for f, im in imgs.items():
        Image.fromarray(im).save(tmp_path / f)
    calls = []
    real = gpu.process_image_rgb_u8_up2x_batch
    monkeypatch.setattr(gpu, "process_image_rgb_u8_up2x_batch", lambda batch, *a, **k: calls.append((len(batch), k.get("tta", False))) or real(batch, *a, **k))
    args = ["-i"] + [str(tmp_path / f) for f in pics] + ["-m", "scale", "--model_dir", str(tmp_path)]
    for tta, want_calls in ((0, [(2, False)]), (1, [(2, True), (1, True)])):
        del calls[:]
        assert w2xc_cli.main(args + ["--tta", str(tta)]) == 0
        assert calls == want_calls
        for f, im in imgs.items():
            got = np.asarray(Image.open(tmp_path / (f[:-4] + "(scale)(x2.000000).png")))
            want = real([im], None, models["c32"], 1, None, 0.0, tta=True)[0] if tta else gpu.process_image_rgb_u8(im, None, models["c32"], 1)
            assert np.array_equal(got, want), (f, tta)
