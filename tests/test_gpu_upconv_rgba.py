"""GPU tests of the RGBA call for upconv head models (revision 0.4.1.6.2: w2xc_process_image_rgba_u8_up2x_batch[_device]).  Every comparison is EQUALITY of
bytes: n = 1 against the route composed from the existing public calls (include/w2xc_hip.h, "upconv head models", RGBA) -- w2xc_bleed_rgba_u8_device, then
w2xc_process_image_rgb_u8_ex_device on the bled image for the colour, and channel 1 of the scale-only w2xc_process_image_rgb_u8_ex_device on (A, A, A) for
alpha --, everything else against the n = 1 call.  References are computed once per (model, size, options) and shared."""
import functools

import numpy as np
import pytest

from tools import gen_model
import upconv_ref as ur

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f: the words of tests/test_gpu_scratch_poison.py
GUARD = 0xA5
KERNEL_DIRECT = 1
FUSION_OFF = 1
# name -> (3x3 planes, head planes out, seed): the published topology, the shortest three-plane head model, an ordinary RGB noise model
TOPO = {"pub": (ur.PUBLISHED, 3, gen_model.SEEDS["upconv7"]), "c32": ([3, 32], 3, 401), "noise": ([3, 32, 32, 3], None, 403)}
SIZES = ((1, 1), (17, 33), (40, 70))            # one pixel (P = 0); below one 8 x 32 head tile one way, over it the other; 5 x 3 head tiles with interior ones


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    assert (w2xc.KERNEL_DIRECT, w2xc.FUSION_OFF) == (KERNEL_DIRECT, FUSION_OFF)
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
def images(h, w, n=3):
    """n RGBA images [n, h, w, 4]: random colour, random alpha with a fully transparent block, an opaque block and partial values elsewhere"""
    rng = np.random.default_rng(91 * h + 7 * w + n)
    img = rng.integers(0, 256, (n, h, w, 4)).astype(np.uint8)
    for i in range(n):
        a = img[i, :, :, 3]
        a[(h // 5 + i) % h:(h // 5 + i) % h + max(1, h // 3), (w // 7 + 2 * i) % w:(w // 7 + 2 * i) % w + max(1, w // 3)] = 0
        a[h - max(1, h // 4):, : max(1, w // 4 + i)] = 255
        if h * w == 1:
            a[0, 0] = (0, 255, 77)[i]
    img.setflags(write=False)
    return img


def opts_of(gpu, kw):
    return gpu.make_opts(device=0, **dict(kw))


def composed(gpu, models, name, img, noise, it, shrink, passes, kw):
    """the route of "Definition" on ONE image [h, w, 4] from the existing public calls"""
    h, w, _ = img.shape
    ms, mn = models[name], (models["noise"] if noise else None)
    W, H = gpu._final_size(w, h, it, shrink)
    P = passes if passes >= 0 else ms.n_layers + (mn.n_layers if mn else 0)
    d_in = torch.from_numpy(np.array(img)).cuda()
    bled = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    gpu.bleed_rgba_u8_device(d_in.data_ptr(), 4 * w, w, h, P, bled.data_ptr(), 3 * w, stream=stream())
    colour = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    gpu.process_image_rgb_u8_device(bled.data_ptr(), 3 * w, w, h, colour.data_ptr(), 3 * W, noise=mn, scale=ms, iterations=it, shrink_ratio=shrink,
                                    stream=stream(), opts=opts_of(gpu, kw))
    grey = d_in[:, :, 3:4].expand(h, w, 3).contiguous()
    ares = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    gpu.process_image_rgb_u8_device(grey.data_ptr(), 3 * w, w, h, ares.data_ptr(), 3 * W, noise=None, scale=ms, iterations=it, shrink_ratio=shrink,
                                    stream=stream(), opts=opts_of(gpu, kw))
    torch.cuda.synchronize()
    return torch.cat([colour, ares[:, :, 1:2]], dim=2).cpu().numpy()


def call_device(gpu, models, name, imgs, noise=False, it=1, shrink=0.0, passes=-1, kw=(), padded=False):
    """the new device call on imgs [n, h, w, 4] -> [n, H, W, 4].  padded: odd row strides and image strides larger than needed, the output pre-filled with
    a guard pattern of which every byte outside the 4 W pixel bytes of each row must survive; the input must come back unchanged either way."""
    n, h, w, _ = imgs.shape
    W, H = gpu._final_size(w, h, it, shrink)
    irs, ors = (4 * w + 5, 4 * W + 3) if padded else (4 * w, 4 * W)
    iis, ois = (irs * h + 17, ors * H + 29) if padded else (irs * h, ors * H)
    src = np.full((n, iis), 0x3C, np.uint8)
    for i in range(n):
        rows = np.lib.stride_tricks.as_strided(src[i], (h, 4 * w), (irs, 1))
        rows[...] = imgs[i].reshape(h, 4 * w)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((n, ois), GUARD, dtype=torch.uint8, device="cuda")
    gpu.process_image_rgba_u8_up2x_batch_device(n, d_in.data_ptr(), iis, irs, w, h, d_out.data_ptr(), ois, ors, noise=models["noise"] if noise else None,
                                                scale=models[name], iterations=it, shrink_ratio=shrink, bleed_passes=passes, stream=stream(),
                                                opts=opts_of(gpu, kw))
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), src), "the input images were written"
    out = d_out.cpu().numpy()
    got = np.empty((n, H, W, 4), np.uint8)
    for i in range(n):
        rows = np.lib.stride_tricks.as_strided(out[i], (H, 4 * W), (ors, 1))
        got[i] = rows.reshape(H, W, 4)
        rows[...] = GUARD
    assert (out == GUARD).all(), "bytes outside the output pixels were written"
    return got


_single = {}


def single(gpu, models, name, h, w, i=0, n=3, **args):
    """the n = 1 call on image i of images(h, w, n), once per argument set"""
    key = (name, h, w, i, n, tuple(sorted(args.items())))
    if key not in _single:
        _single[key] = call_device(gpu, models, name, images(h, w, n)[i:i + 1], **args)[0]
    return _single[key]


# ---- 1. n = 1 equals the composed route ----
def option_sets():
    cases = []
    for name in ("pub", "c32"):
        for h, w in SIZES:
            cases.append((name, h, w, dict()))
            cases.append((name, h, w, dict(kw=(("fusion", FUSION_OFF),))))
            cases.append((name, h, w, dict(kw=(("kernel", KERNEL_DIRECT),))))
            cases.append((name, h, w, dict(shrink=0.75)))
            cases.append((name, h, w, dict(noise=True)))
            for p in (0, 3, 20):                  # (-1 is the default of every other case; 20 takes the pass chain, not the tiled bleed)
                cases.append((name, h, w, dict(passes=p)))
        cases.append((name, 40, 70, dict(kw=(("band_rows", 8),))))
        cases.append((name, 17, 33, dict(it=2)))
    return cases


def case_id(c):
    name, h, w, args = c
    return "%s-%dx%d-%s" % (name, h, w, "-".join("%s=%s" % (k, dict(v) if k == "kw" else v) for k, v in sorted(args.items())) or "default")


@pytest.mark.parametrize("case", option_sets(), ids=case_id)
def test_single_image_equals_composed_route(gpu, models, case):
    name, h, w, args = case
    a = dict(noise=False, it=1, shrink=0.0, passes=-1, kw=())
    a.update(args)
    got = single(gpu, models, name, h, w, **args)
    want = composed(gpu, models, name, images(h, w)[0], a["noise"], a["it"], a["shrink"], a["passes"], a["kw"])
    assert got.shape == want.shape
    assert np.array_equal(got[:, :, :3], want[:, :, :3]), "colour"
    assert np.array_equal(got[:, :, 3], want[:, :, 3]), "alpha"


def test_banded_run_equals_unbanded(gpu, models):
    for name in ("pub", "c32"):
        assert np.array_equal(single(gpu, models, name, 40, 70, kw=(("band_rows", 8),)), single(gpu, models, name, 40, 70))


# ---- 2. batch, n = 3: image i equals the n = 1 call ----
@pytest.mark.parametrize("name", ["pub", "c32"])
@pytest.mark.parametrize("h,w", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_batch_equals_single_calls(gpu, models, name, h, w):
    imgs = images(h, w)
    want = np.stack([single(gpu, models, name, h, w, i) for i in range(3)])
    assert np.array_equal(call_device(gpu, models, name, imgs), want), "packed"
    assert np.array_equal(call_device(gpu, models, name, imgs, padded=True), want), "padded"


def test_batch_with_noise_shrink_and_two_iterations(gpu, models):
    h, w = 17, 33
    for args in (dict(noise=True), dict(shrink=0.75), dict(it=2), dict(kw=(("fusion", FUSION_OFF),))):
        want = np.stack([single(gpu, models, "c32", h, w, i, **args) for i in range(3)])
        assert np.array_equal(call_device(gpu, models, "c32", images(h, w), padded=True, **args), want), args


def test_one_launch_per_layer_and_pass_and_no_noise_pass_for_alpha(gpu, models):
    """n = 3 under default options is one sub-batch: every layer of the scale model is launched twice, once for the colour pass and once for the alpha pass
    (its head the second time as the alpha head), the noise model once -- alpha never sees it"""
    h, w = 40, 70
    assert models["pub"].batch_plan(3, w, h, up2x=True)[0] == 1
    for m in ("pub", "noise"):
        models[m].profile_reset(0)
    got = call_device(gpu, models, "pub", images(h, w), noise=True, kw=(("profile", 1),))
    counts = [models[m].profile_read(0)[1] for m in ("noise", "pub")]
    assert counts == [[1] * models["noise"].n_layers, [2] * models["pub"].n_layers], counts
    assert np.array_equal(got, np.stack([single(gpu, models, "pub", h, w, i, noise=True) for i in range(3)]))


# ---- 3. sub-batching ----
def test_sub_batches_give_the_same_bytes(gpu, models):
    h, w, n = 40, 70, 3
    ms = models["pub"]
    for mb in (16, 12, 8, 6, 4, 2, 1):   # the published topology at 40 x 70 takes a few MiB of workspace per image: the largest budget that cuts the batch
        batched, sub = ms.batch_plan(3, w, h, up2x=True, opts=gpu.make_opts(workspace_mb=mb))
        if sub < n:
            break
    assert sub < n, "no workspace_mb found at which the plan's sub-batch is below n"
    want = np.stack([single(gpu, models, "pub", h, w, i) for i in range(n)])
    assert np.array_equal(call_device(gpu, models, "pub", images(h, w), kw=(("workspace_mb", mb),)), want)


# ---- 4. host form = device form ----
@pytest.mark.parametrize("n", [1, 3])
def test_host_form_equals_device_form(gpu, models, n):
    h, w = 17, 33
    imgs = np.array(images(h, w)[:n])            # pageable numpy memory
    for name, args in (("pub", dict()), ("c32", dict(noise=True))):
        want = np.stack([single(gpu, models, name, h, w, i, **args) for i in range(n)])
        got = gpu.process_image_rgba_u8_up2x_batch(imgs, models["noise"] if args else None, models[name], 1, gpu.make_opts(device=0), 0.0)
        assert np.array_equal(got, want), (name, n)
        assert np.array_equal(imgs, images(h, w)[:n])


# ---- 5. a workgroup's run of tiles straddles two images in the alpha head ----
def test_alpha_head_tile_run_straddles_two_images(gpu, models):
    h, w, n = 65, 600, 3
    tiles = -(-h // 8) * -(-w // 32)             # upconv4x4_head: tiles of 8 x 32 source pixels
    total = n * tiles
    grid = min(total, 512)                       # w2xc_upconv_grid
    per = -(-total // grid)
    assert (tiles, total, grid, per) == (171, 513, 512, 2)
    assert (170 // per == 171 // per) and 170 // tiles == 0 and 171 // tiles == 1       # run 85 holds the last tile of image 0 and the first of image 1
    assert (342 // per == 343 // per) and 341 // tiles == 1 and 342 // tiles == 2       # run 171 does the same between images 1 and 2
    assert models["c32"].batch_plan(3, w, h, up2x=True)[0] == 1
    imgs = images(h, w)
    want = np.stack([call_device(gpu, models, "c32", imgs[i:i + 1])[0] for i in range(n)])
    assert np.array_equal(call_device(gpu, models, "c32", imgs), want)


# ---- 6. scratch independence ----
def test_result_does_not_depend_on_scratch_content(gpu, models):
    h, w = 40, 70
    for name, args in (("pub", dict()), ("c32", dict(noise=True)), ("c32", dict(shrink=0.75))):
        want = np.stack([single(gpu, models, name, h, w, i, **args) for i in range(3)])
        for word in WORDS:
            filled = sum(models[k].fill_scratch(word, 0) for k in (name, "noise"))
            assert filled > 0
            assert np.array_equal(call_device(gpu, models, name, images(h, w), **args), want), (name, args, hex(word))
            models[name].fill_scratch(word, 0)
            assert np.array_equal(call_device(gpu, models, name, images(h, w)[:1], **args)[0], want[0]), (name, args, hex(word), "n = 1")


# ---- 7. the CLI: transparent inputs of a head model go to the new call, one call per size group ----
def test_cli_sends_transparent_inputs_to_the_rgba_head_call(gpu, models, tmp_path, monkeypatch):
    from PIL import Image
    from tools import w2xc_cli
    gen_model.write_json(arrays("c32")[0], str(tmp_path / "scale2.0x_model.json"), head=arrays("c32")[1])
    rng = np.random.default_rng(22)
    pics = {"a.png": (12, 20, 4), "b.png": (12, 20, 4), "c.png": (9, 9, 4), "d.png": (12, 20, 3)}
    imgs = {f: rng.integers(0, 256, s).astype(np.uint8) for f, s in pics.items()}
    for f, im in imgs.items():
        Image.fromarray(im).save(tmp_path / f)
    calls = []
    real = gpu.process_image_rgba_u8_up2x_batch
    monkeypatch.setattr(gpu, "process_image_rgba_u8_up2x_batch", lambda batch, *a, **k: calls.append(len(batch)) or real(batch, *a, **k))
    args = ["-i"] + [str(tmp_path / f) for f in pics] + ["-m", "scale", "--model_dir", str(tmp_path)]
    assert w2xc_cli.main(args) == 0
    assert calls == [2, 1]                        # a.png + b.png, c.png alone as a batch of one; d.png is opaque: the 3-channel call
    for f, im in imgs.items():
        got = np.asarray(Image.open(tmp_path / (f[:-4] + "(scale)(x2.000000).png")))
        want = real([im], None, models["c32"], 1)[0] if im.shape[2] == 4 else gpu.process_image_rgb_u8(im, None, models["c32"], 1)
        assert np.array_equal(got, want), f
    with pytest.raises(SystemExit):               # --tta 1 with transparency stays check_tta's refusal
        w2xc_cli.main(args + ["--tta", "1"])
