"""GPU tests of TTA for the RGBA image calls (revision 0.4.1.6.3: w2xc_process_image_rgba_u8_batch_tta[_device] for Y and RGB models,
w2xc_process_image_rgba_u8_up2x_batch_tta[_device] for upconv head models).  Every comparison is EQUALITY of bytes: n = 1 against the route composed from
calls that existed before (include/w2xc_hip.h, the RGBA TTA calls) -- w2xc_bleed_rgba_u8_device, the 3-channel TTA call of the route on the bled image for
the colour, and for alpha the scale model's TTA pass(es) on u8 / 255 (Y route) or channel 1 of the scale-only 3-channel TTA call on (A, A, A) (RGB and head
routes), with torch for the grey image, the rounding and the merge --, everything else against the n = 1 call.  References are computed once and shared."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from tools import gen_model
import upconv_ref as ur
from fp32_matrix import kernel_names   # (the device kernels a call launches, by torch's profiler)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f: the words of tests/test_gpu_scratch_poison.py
GUARD = 0xA5
Y_PLANES = [1, 32, 32, 64, 64, 128, 128, 1]     # (tests/test_gpu_rgba.py: the Y chain that has batch kernels)
# name -> (planes, head planes out or None, seed)
TOPO = {"ys": (Y_PLANES, None, gen_model.SEEDS["scale2.0x"]), "yn": (Y_PLANES, None, gen_model.SEEDS["noise1"]),
        "m4": ([3, 32, 64, 64, 3], None, 302), "n3": ([3, 32, 32, 3], None, 403),
        "c32": ([3, 32], 3, 401), "pub": (ur.PUBLISHED, 3, gen_model.SEEDS["upconv7"])}
# route -> (scale model, noise model, the head family?)
ROUTES = {"y": ("ys", "yn", False), "rgb": ("m4", "n3", False), "head": ("c32", "n3", True), "pub": ("pub", "n3", True)}
# one pixel; a tile edge + 1 in both orientations (variant groups of 4 + 4); one tile, square (one group of 8); several tiles on both axes
SIZES = ((1, 1), (17, 33), (33, 17), (32, 32), (40, 70))


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


def fresh(gpu, name):
    return gpu._ModelSet.from_layers(arrays(name)[0], head=arrays(name)[1])


@pytest.fixture(scope="module")
def models(gpu):
    return {k: fresh(gpu, k) for k in TOPO}


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def images(h, w, n=3):
    """n RGBA images [n, h, w, 4] from a fixed seed: random colour; alpha random with a run of zeros (a block), a run of 255 and partial values elsewhere"""
    rng = np.random.default_rng(131 * h + 17 * w + n)
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


def route_models(models, route, noise):
    s, n, head = ROUTES[route]
    return models[s], (models[n] if noise else None), head


def colour_call(gpu, route, head):
    """the 3-channel TTA device call of the route on ONE image"""
    if head:
        return lambda d_in, irs, w, h, d_out, ors, **kw: gpu.process_image_rgb_u8_up2x_batch_device(1, d_in, 0, irs, w, h, d_out, 0, ors, tta=True, **kw)
    f = gpu.process_image_u8_device if route == "y" else gpu.process_image_rgb_u8_device
    return lambda d_in, irs, w, h, d_out, ors, **kw: f(d_in, irs, w, h, d_out, ors, tta=True, **kw)


def composed(gpu, models, route, img, noise, it, shrink, passes, kw):
    """the definition on ONE image [h, w, 4], from calls that existed before this revision and torch"""
    h, w, _ = img.shape
    ms, mn, head = route_models(models, route, noise)
    msc = ms if it or head else None           # (the Y / RGB calls take no scale model they do not run; the head family asks for its head model always)
    W, H = gpu._final_size(w, h, it, shrink)
    P = passes if passes >= 0 else (msc.n_layers if msc else 0) + (mn.n_layers if mn else 0)
    o = opts_of(gpu, kw)
    d_in = torch.from_numpy(np.array(img)).cuda()
    bled = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    gpu.bleed_rgba_u8_device(d_in.data_ptr(), 4 * w, w, h, P, bled.data_ptr(), 3 * w, stream=stream())
    colour = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    call3 = colour_call(gpu, route, head)
    call3(bled.data_ptr(), 3 * w, w, h, colour.data_ptr(), 3 * W, noise=mn, scale=msc, iterations=it, shrink_ratio=shrink, stream=stream(), opts=o)
    if it == 0:
        # exactly what the call without TTA does with alpha: the bytes, or their linear shrink
        plain = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        f = gpu.process_image_rgba_u8_up2x_batch_device if head else gpu.process_image_rgba_u8_batch_device
        f(1, d_in.data_ptr(), 0, 4 * w, w, h, plain.data_ptr(), 0, 4 * W, noise=mn, scale=msc, iterations=0, shrink_ratio=shrink, bleed_passes=passes,
          stream=stream(), opts=o)
        alpha = plain[:, :, 3:4]
    elif route == "y":
        a = d_in[:, :, 3].to(torch.float32) * np.float32(1.0 / 255.0)
        cw, ch = w, h
        for _ in range(it):
            a = a.contiguous()
            b = torch.empty((2 * ch, 2 * cw), dtype=torch.float32, device="cuda")
            ms.convert_batch_tta_device(1, a.data_ptr(), cw * ch * 4, cw * 4, cw, ch, b.data_ptr(), 4 * cw * ch * 4, 2 * cw * 4, nn2x=True, stream=stream(), opts=o)
            a, cw, ch = b, 2 * cw, 2 * ch
        if shrink:
            b = torch.empty((H, W), dtype=torch.float32, device="cuda")
            gpu.resize_linear_device(a.data_ptr(), cw, ch, b.data_ptr(), W, H, stream=stream())
            a = b
        alpha = torch.clamp(torch.round(a * np.float32(255.0)), 0, 255).to(torch.uint8)[:, :, None]     # saturate(rint(255 a)), half to even
    else:
        grey = d_in[:, :, 3:4].expand(h, w, 3).contiguous()
        ares = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        call3(grey.data_ptr(), 3 * w, w, h, ares.data_ptr(), 3 * W, noise=None, scale=ms, iterations=it, shrink_ratio=shrink, stream=stream(), opts=o)
        alpha = ares[:, :, 1:2]
    torch.cuda.synchronize()
    return torch.cat([colour, alpha], dim=2).cpu().numpy()


def call_device(gpu, models, route, imgs, noise=False, it=1, shrink=0.0, passes=-1, kw=(), padded=False, tta=True, sibling=False):
    """the new device call on imgs [n, h, w, 4] -> [n, H, W, 4] (sibling: the call without the tta argument).  padded: odd row strides and image strides
    larger than needed; the output is pre-filled with a guard pattern of which every byte outside the 4 W pixel bytes of each row must survive, and the input
    must come back unchanged"""
    n, h, w, _ = imgs.shape
    ms, mn, head = route_models(models, route, noise)
    W, H = gpu._final_size(w, h, it, shrink)
    irs, ors = (4 * w + 5, 4 * W + 3) if padded else (4 * w, 4 * W)
    iis, ois = (irs * h + 17, ors * H + 29) if padded else (irs * h, ors * H)
    src = np.full((n, iis), 0x3C, np.uint8)
    for i in range(n):
        np.lib.stride_tricks.as_strided(src[i], (h, 4 * w), (irs, 1))[...] = imgs[i].reshape(h, 4 * w)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((n, ois), GUARD, dtype=torch.uint8, device="cuda")
    f = gpu.process_image_rgba_u8_up2x_batch_device if head else gpu.process_image_rgba_u8_batch_device
    more = {} if sibling else dict(tta=tta)
    f(n, d_in.data_ptr(), iis, irs, w, h, d_out.data_ptr(), ois, ors, noise=mn, scale=ms if it or head else None, iterations=it, shrink_ratio=shrink,
      bleed_passes=passes, stream=stream(), opts=opts_of(gpu, kw), **more)
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


def single(gpu, models, route, h, w, i=0, n=3, **args):
    """the n = 1 TTA call on image i of images(h, w, n), once per argument set"""
    key = (route, h, w, i, n, tuple(sorted(args.items())))
    if key not in _single:
        _single[key] = call_device(gpu, models, route, images(h, w, n)[i:i + 1], **args)[0]
    return _single[key]


# ---- 1. n = 1 equals the composed route ----
OPTION_SETS = (dict(), dict(noise=True), dict(noise=True, it=0), dict(it=2), dict(shrink=0.75), dict(noise=True, shrink=0.75), dict(passes=0),
               dict(noise=True, it=0, shrink=0.75))


def cases():
    out = []
    for route in ("y", "rgb", "head"):
        for h, w in SIZES:
            out.append((route, h, w, dict()))                    # scale only, the automatic bleed
        for h, w in ((17, 33), (32, 32)):
            out += [(route, h, w, a) for a in OPTION_SETS[1:]]
        out.append((route, 1, 1, dict(noise=True, it=0)))
    out.append(("pub", 17, 33, dict()))                          # the published upconv_7 topology, once
    return out


def case_id(c):
    route, h, w, args = c
    return "%s-%dx%d-%s" % (route, h, w, "-".join("%s=%s" % kv for kv in sorted(args.items())) or "scale")


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_single_image_equals_composed_route(gpu, models, case):
    route, h, w, args = case
    a = dict(noise=False, it=1, shrink=0.0, passes=-1, kw=())
    a.update(args)
    got = single(gpu, models, route, h, w, **args)
    want = composed(gpu, models, route, images(h, w)[0], a["noise"], a["it"], a["shrink"], a["passes"], a["kw"])
    assert got.shape == want.shape
    assert np.array_equal(got[:, :, :3], want[:, :, :3]), "colour"
    assert np.array_equal(got[:, :, 3], want[:, :, 3]), "alpha"
    if a["it"] and h * w > 1:
        plain = call_device(gpu, models, route, images(h, w)[:1], tta=False, **args)[0]
        assert not np.array_equal(got[:, :, :3], plain[:, :, :3]) and not np.array_equal(got[:, :, 3], plain[:, :, 3]), "TTA changes colour and alpha"


# ---- 2. W2XC_FUSION_OFF: the stages around float planes give the bytes of the fused ends ----
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_fusion_off_gives_the_bytes_of_the_default(gpu, models, route):
    off = (("fusion", gpu.FUSION_OFF),)
    for h, w in ((17, 33), (32, 32)):
        for args in OPTION_SETS[:6]:
            assert np.array_equal(single(gpu, models, route, h, w, kw=off, **args), single(gpu, models, route, h, w, **args)), (h, w, args)


# ---- 3. bands ----
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_banded_run_equals_unbanded(gpu, models, route):
    for args in (dict(), dict(noise=True, it=0)):
        assert np.array_equal(single(gpu, models, route, 40, 70, kw=(("band_rows", 8),), **args), single(gpu, models, route, 40, 70, **args)), args


# ---- 4. batches ----
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
@pytest.mark.parametrize("h,w", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_batch_equals_single_calls(gpu, models, route, h, w):
    want = np.stack([single(gpu, models, route, h, w, i) for i in range(3)])
    assert np.array_equal(call_device(gpu, models, route, images(h, w)), want), "packed"
    assert np.array_equal(call_device(gpu, models, route, images(h, w), padded=True), want), "padded"


@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_batch_with_every_option(gpu, models, route):
    h, w = 17, 33
    for args in OPTION_SETS[1:] + (dict(kw=(("fusion", gpu.FUSION_OFF),)), dict(noise=True, kw=(("kernel", gpu.KERNEL_DIRECT),))):
        want = np.stack([single(gpu, models, route, h, w, i, **args) for i in range(3)])
        assert np.array_equal(call_device(gpu, models, route, images(h, w), padded=True, **args), want), args


def scratch_after(gpu, route, n, mb, h, w):
    """bytes of scratch a batch of n leaves in fresh contexts (they hold this call's sizes alone)"""
    s, _, _ = ROUTES[route]
    mods = {s: fresh(gpu, s)}
    call_device(gpu, mods, route, images(h, w)[:n], kw=(("workspace_mb", mb),))
    return mods[s].fill_scratch(0, 0)


@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_sub_batches_of_two_and_one(gpu, models, route):
    """workspace_mb at which a sub-batch holds two images: the call's memory grows from n = 1 to n = 2 and no further"""
    h, w, n = 40, 70, 3
    for mb in range(1, 65):
        used = [scratch_after(gpu, route, k, mb, h, w) for k in (1, 2)]
        if used[0] < used[1]:
            break
    else:
        pytest.fail("no workspace_mb up to 64 at which two images share a sub-batch")
    assert scratch_after(gpu, route, 3, mb, h, w) == used[1], "workspace_mb = %d: a sub-batch of three" % mb
    want = np.stack([single(gpu, models, route, h, w, i) for i in range(n)])
    assert np.array_equal(call_device(gpu, models, route, images(h, w), kw=(("workspace_mb", mb),)), want), mb
    assert np.array_equal(call_device(gpu, models, route, images(h, w), noise=True, shrink=0.75, kw=(("workspace_mb", mb),)),
                          np.stack([single(gpu, models, route, h, w, i, noise=True, shrink=0.75) for i in range(n)])), mb


# ---- 5. host form = device form ----
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_host_form_equals_device_form(gpu, models, route, n):
    h, w = 17, 33
    imgs = np.array(images(h, w)[:n])            # pageable numpy memory
    f = gpu.process_image_rgba_u8_up2x_batch if ROUTES[route][2] else gpu.process_image_rgba_u8_batch
    for args in (dict(), dict(noise=True, shrink=0.75)):
        ms, mn, _ = route_models(models, route, args.get("noise", False))
        want = np.stack([single(gpu, models, route, h, w, i, **args) for i in range(n)])
        got = f(imgs, mn, ms, 1, gpu.make_opts(device=0), args.get("shrink", 0.0), tta=True)
        assert np.array_equal(got, want), (route, n, args)
        assert np.array_equal(imgs, images(h, w)[:n])
    if n == 1 and not ROUTES[route][2]:          # the single-image Python forms take the keyword too
        ms, _, _ = route_models(models, route, False)
        assert np.array_equal(gpu.process_image_rgba_u8(imgs[0], None, ms, 1, gpu.make_opts(device=0), tta=True), single(gpu, models, route, h, w, 0))


# ---- 6. tta = 0 / tta=False: the calls that existed ----
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_tta_false_equals_the_existing_calls(gpu, models, route):
    h, w = 17, 33
    for args in (dict(), dict(noise=True, shrink=0.75), dict(noise=True, it=0)):
        want = call_device(gpu, models, route, images(h, w), sibling=True, **args)
        assert np.array_equal(call_device(gpu, models, route, images(h, w), tta=False, **args), want), args
        assert np.array_equal(call_device(gpu, models, route, images(h, w), tta=0, **args), want), args


# ---- 7. launch lists ----
def launch_counts(gpu, models, names, run):
    for m in names:
        models[m].profile_reset(0)
    run()
    return [models[m].profile_read(0)[1] for m in names]


@pytest.mark.parametrize("h,w", [(40, 70), (32, 32)], ids=["40x70", "32x32"])
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_launches_per_layer(gpu, models, route, h, w):
    """Per layer and size group (two groups of 4 S variants; one of 8 S where w == h) ONE launch for the sub-batch: the launches of the opaque TTA batch of
    the route on 3-channel images of that size -- once for the noise model, which alpha never sees; for the scale model once on the Y route, where alpha
    rides in Y's launches, and twice on the RGB and head routes, colour and alpha.  A sub-batch of three launches what one image does."""
    s, nz, head = ROUTES[route]
    prof = (("profile", 1),)
    o = opts_of(gpu, prof)
    d3 = torch.from_numpy(np.ascontiguousarray(images(h, w)[:, :, :, :3])).cuda()
    d6 = torch.empty((3, 2 * h, 2 * w, 3), dtype=torch.uint8, device="cuda")
    opaque = (gpu.process_image_rgb_u8_up2x_batch_device if head else
              gpu.process_image_u8_batch_device if route == "y" else gpu.process_image_rgb_u8_batch_device)

    def opaque_batch():
        opaque(3, d3.data_ptr(), 3 * w * h, 3 * w, w, h, d6.data_ptr(), 12 * w * h, 6 * w, noise=models[nz], scale=models[s], iterations=1, stream=stream(),
               opts=o, tta=True)
        torch.cuda.synchronize()
    want_n, want_s = launch_counts(gpu, models, (nz, s), opaque_batch)
    assert sum(want_n) > 0 and sum(want_s) > 0
    twice = 1 if route == "y" else 2
    for n in (3, 1):
        got_n, got_s = launch_counts(gpu, models, (nz, s), lambda: call_device(gpu, models, route, images(h, w)[:n], noise=True, kw=prof))
        assert got_n == want_n, ("the noise model runs for the colour alone", n, got_n, want_n)
        assert got_s == [twice * c for c in want_s], (n, got_s, want_s)
    if route != "y":
        groups = 1 if h == w else 2
        assert want_s == [groups] * models[s].n_layers and want_n == [groups] * models[nz].n_layers, (want_s, want_n)


STAGES_AWAY = ("U8ToRgb", "RgbToU8", "AlphaToGrey", "MergeRgba")


@pytest.mark.parametrize("route", ["rgb", "head"])
def test_fused_ends_launch_no_colour_stage(gpu, models, route):
    """default options, a scale pass last, no shrink: both sequences spread from uint8 and gather into the caller's pixels -- no U8ToRgb, RgbToU8, AlphaToGrey
    or merge launch; on the head route the alpha sequence's head launches are the one-plane form with the float sink"""
    h, w, n = 40, 70, 3
    names = kernel_names(lambda: call_device(gpu, models, route, images(h, w)[:n], noise=True))
    if not any("k_ttau8" in k for k in names):
        pytest.fail("the profiler recorded no kernel of the library: %r" % names[:8])
    assert not [k for k in names if any(s in k for s in STAGES_AWAY)], names
    assert sum("k_ttau8_spread" in k for k in names) == 2 and sum("k_ttau8_gather" in k for k in names) == 2, names
    assert sum("k_tta_spread" in k for k in names) == 1 and sum("k_tta_gather" in k for k in names) == 1, "the level between the noise pass and the scale pass"
    if route == "head":
        heads = [k for k in names if "upconv4x4_head" in k]
        assert len(heads) == 4 and all("_batch" in k for k in heads), heads          # colour and alpha, two size groups each
        assert sum("Li3ELb0" in k or ", 3, false" in k for k in heads) == 2 and sum("Li1ELb0" in k or ", 1, false" in k for k in heads) == 2, heads
    # ... and with W2XC_FUSION_OFF or a shrink the stages are back
    off = kernel_names(lambda: call_device(gpu, models, route, images(h, w)[:n], noise=True, kw=(("fusion", gpu.FUSION_OFF),)))
    assert not any("k_ttau8" in k for k in off) and all(any(s in k for k in off) for s in STAGES_AWAY), off
    shr = kernel_names(lambda: call_device(gpu, models, route, images(h, w)[:n], shrink=0.75))
    assert sum("k_ttau8_spread" in k for k in shr) == 2 and not any("k_ttau8_gather" in k for k in shr) and any("MergeRgba" in k for k in shr), shr
    assert not any("U8ToRgb" in k or "AlphaToGrey" in k for k in shr), shr


# ---- 8. scratch independence ----
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_result_does_not_depend_on_scratch_content(gpu, models, route):
    h, w = 40, 70
    s, nz, _ = ROUTES[route]
    for args in (dict(noise=True), dict(shrink=0.75)):
        want = np.stack([single(gpu, models, route, h, w, i, **args) for i in range(3)])
        for word in WORDS:
            assert sum(models[k].fill_scratch(word, 0) for k in (s, nz)) > 0
            assert np.array_equal(call_device(gpu, models, route, images(h, w), **args), want), (args, hex(word))
            for k in (s, nz):
                models[k].fill_scratch(word, 0)
            assert np.array_equal(call_device(gpu, models, route, images(h, w)[:1], **args)[0], want[0]), (args, hex(word), "n = 1")


# ---- 9. the CLI under --tta 1 --tta_alpha 1 ----
@pytest.mark.parametrize("route", ["y", "rgb", "head"])
def test_cli_sends_transparent_inputs_to_the_tta_calls(gpu, models, route, tmp_path, monkeypatch):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    s, _, head = ROUTES[route]
    gen_model.write_json(arrays(s)[0], str(tmp_path / "scale2.0x_model.json"), **(dict(head=arrays(s)[1]) if head else {}))
    rng = np.random.default_rng(23)
    pics = {"a.png": (12, 20, 4), "b.png": (12, 20, 4), "c.png": (9, 9, 4), "d.png": (12, 20, 3)}
    imgs = {f: rng.integers(0, 256, shape).astype(np.uint8) for f, shape in pics.items()}
    for f, im in imgs.items():
        Image.fromarray(im).save(tmp_path / f)
    name = "process_image_rgba_u8_up2x_batch" if head else "process_image_rgba_u8_batch"
    real = getattr(gpu, name)
    calls = []
    monkeypatch.setattr(gpu, name, lambda batch, *a, **k: calls.append((len(batch), k.get("tta"))) or real(batch, *a, **k))
    args = ["-i"] + [str(tmp_path / f) for f in pics] + ["-m", "scale", "--model_dir", str(tmp_path), "--tta", "1"]
    with pytest.raises(SystemExit):               # without the opt-in: check_tta's refusal, nothing converted
        cli.main(args)
    assert calls == []
    assert cli.main(args + ["--tta_alpha", "1"]) == 0
    assert calls == [(2, True), (1, True)]        # a.png + b.png, c.png alone as a batch of one; d.png is opaque: the 3-channel TTA call
    order = [0, 1, 2, 3] if route != "y" else [2, 1, 0, 3]      # (the Y route takes cv::imread's BGR order)
    for f, im in imgs.items():
        got = np.asarray(Image.open(tmp_path / (f[:-4] + "(scale)(x2.000000).png")))
        if im.shape[2] == 4:
            want = real([np.ascontiguousarray(im[:, :, order])], None, models[s], 1, tta=True)[0][:, :, order]
        elif head:
            want = gpu.process_image_rgb_u8_up2x_batch([im], None, models[s], 1, tta=True)[0]
        elif route == "y":
            want = gpu.process_image_u8(np.ascontiguousarray(im[:, :, ::-1]), None, models[s], 1, tta=True)[:, :, ::-1]
        else:
            want = gpu.process_image_rgb_u8(im, None, models[s], 1, tta=True)
        assert np.array_equal(got, want), f
