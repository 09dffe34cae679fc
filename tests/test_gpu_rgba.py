"""GPU tests of the RGBA surface: w2xc_bleed_rgba_u8_device and w2xc_process_image_rgba_u8_ex[_device] on both routes (Y models, RGB models), and the
CLI's alpha route.  The expectations: bleed_ref (tests/test_rgba_api.py: the bleed of include/w2xc_hip.h restated in numpy), the existing 3-channel calls
on the bled image (colour, byte for byte), w2xc_convert_plane_nn2x_device / the grey RGB call (alpha, byte for byte) and the CPU oracle (alpha, the
project's uint8 gate).  References are computed once per (route, case, options) and shared."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from tools import gen_model
from oracle import oracle as orc
from test_rgba_api import bleed_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f (tests/test_gpu_scratch_poison.py)
Y_PLANES = [1, 32, 32, 64, 64, 128, 128, 1]
TOPO = {"yn": (Y_PLANES, gen_model.SEEDS["noise1"]), "ys": (Y_PLANES, gen_model.SEEDS["scale2.0x"]),
        "m7": ([3, 32, 32, 64, 64, 128, 128, 3], 301), "m4": ([3, 32, 64, 64, 3], 302)}          # m7 / m4: tests/test_gpu_rgb.py
P_USED = 3                                      # the bleed passes of the colour cases: every image has a zero region 2 P + 3 = 9 wide
# image -> (seed, (h, w), corner rectangle (rows, cols)): two tile columns with a ragged edge, odd sizes, more than one 8-row tile
IMG = {"a": (15, (24, 36), (6, 8)), "b": (16, (37, 53), (13, 13))}
# (name, noise model, scale model, image, iterations, shrink) per route: scale x2 and x4, noise, noise + scale (two models, two contexts), ratio 1.5
CASES = {"y": [("scale1", None, "ys", "b", 1, 0.0), ("scale2", None, "ys", "a", 2, 0.0), ("noise", "yn", None, "a", 0, 0.0),
               ("noise_scale", "yn", "ys", "b", 1, 0.0), ("ratio1.5", None, "ys", "b", 1, 0.75)],
         "rgb": [("scale1", None, "m7", "b", 1, 0.0), ("scale2", None, "m4", "a", 2, 0.0), ("noise", "m7", None, "a", 0, 0.0),
                 ("noise_scale", "m7", "m4", "b", 1, 0.0), ("ratio1.5", None, "m4", "b", 1, 0.75)]}
OPTS = {"default": {}, "direct": dict(kernel="KERNEL_DIRECT"), "fusion_off": dict(fusion="FUSION_OFF"), "bands": dict(band_rows=8),
        "bf16x3": dict(precision="PRECISION_BF16X3")}
ROUTE_OPTS = [(r, c[0], o) for r in ("y", "rgb") for c in CASES[r] for o in OPTS if not (r == "rgb" and o == "bf16x3")]   # (one 16-bit precision: Y route)


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@functools.lru_cache(maxsize=None)
def layers(name):
    return gen_model.synth_layers(*TOPO[name])


@pytest.fixture(scope="module")
def models(gpu):
    return {k: gpu._ModelSet.from_layers(layers(k)) for k in TOPO}


@functools.lru_cache(maxsize=None)
def image(name):
    """random colour and alpha bytes; alpha zeroed on rectangles that cover less than a quarter of the area: one in the corner (it touches two edges),
    one 9 x 9 inside (its centre is out of reach of P_USED passes), one 5 x 5 with an opaque pixel alone in its middle"""
    seed, (h, w), (ch, cw) = IMG[name]
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)
    a = img[:, :, 3]
    a[h - ch:, w - cw:] = 0
    a[2:11, 3:12] = 0
    a[12:17, 20:25] = 0
    a[14, 22] = 200
    assert (a == 0).sum() <= h * w // 4
    img.setflags(write=False)
    return img


def opts_of(gpu, name, **more):
    kw = {k: getattr(gpu, v) if isinstance(v, str) else v for k, v in OPTS[name].items()}
    kw.update(more)
    return gpu.make_opts(**kw) if kw else None


def case_of(route, name):
    return [c for c in CASES[route] if c[0] == name][0]


def final_size(h, w, it, shrink):
    H, W = h << it, w << it
    if shrink:
        W, H = int(float(W * shrink)), int(float(H * shrink))
    return H, W


def call3(gpu, models, route, img3, noise, scale, it, shrink, o):
    f = gpu.process_image_rgb_u8 if route == "rgb" else gpu.process_image_u8
    return f(np.ascontiguousarray(img3), models[noise] if noise else None, models[scale] if scale else None, it, o, shrink)


def call4(gpu, models, case, o, passes):
    _, noise, scale, img, it, shrink = case
    return gpu.process_image_rgba_u8(image(img), models[noise] if noise else None, models[scale] if scale else None, it, o, shrink, passes)


@functools.lru_cache(maxsize=None)
def bled(img, passes):
    out = bleed_ref(image(img), passes)
    out.setflags(write=False)
    return out


def nn2x_chain(gpu, ms, alpha, it, o):
    """clip(rint(255 x)) of convert_plane_nn2x_device applied `it` times to alpha * (1 / 255), rounded in torch fp32 (torch.round: half to even)"""
    st = torch.cuda.current_stream()
    x = torch.from_numpy(np.ascontiguousarray(alpha)).cuda().to(torch.float32) * torch.tensor(np.float32(1.0 / 255.0), device="cuda")
    for _ in range(it):
        h, w = x.shape
        y = torch.full((2 * h, 2 * w), float("nan"), dtype=torch.float32, device="cuda")
        ms.convert_nn2x_device(x.data_ptr(), w * 4, w, h, y.data_ptr(), 2 * w * 4, stream=st.cuda_stream, opts=o)
        x = y
    st.synchronize()
    return (x * 255.0).round().clamp(0, 255).to(torch.uint8).cpu().numpy()


# ---- 1. the bleed alone ----
def dev_bleed(gpu, img, passes):
    """w2xc_bleed_rgba_u8_device with strided input and output rows; the bytes behind the output rows must keep their 0xAB"""
    h, w, _ = img.shape
    irs, ors = w * 4 + 5, w * 3 + 7
    host = np.full((h, irs), 0x5A, np.uint8)
    host[:, :w * 4] = img.reshape(h, w * 4)
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((h + 1, ors), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    gpu.bleed_rgba_u8_device(d_in.data_ptr(), irs, w, h, passes, d_out.data_ptr(), ors, stream=st.cuda_stream)
    st.synchronize()
    b = d_out.cpu().numpy()
    assert (b[:h, w * 3:] == 0xAB).all() and (b[h] == 0xAB).all(), "bytes behind the output rows were written"
    assert np.array_equal(d_in.cpu().numpy(), host), "the input was written"
    return b[:h, :w * 3].reshape(h, w, 3).copy()


def reached(img, passes):
    """which pixels are opaque or filled after `passes` passes: white on the opaque pixels, black elsewhere, bled -- a mean of whites is white"""
    probe = np.zeros_like(img)
    probe[:, :, 3] = img[:, :, 3]
    probe[img[:, :, 3] > 0, :3] = 255
    return bleed_ref(probe, passes)[:, :, 0] == 255


@pytest.mark.parametrize("name", ["a", "b", "1x1", "1x7", "none"])
def test_bleed_equals_reference(gpu, name):
    if name in IMG:
        img = image(name)
    elif name == "none":                             # no opaque pixel at all: nothing to bleed from
        img = np.random.default_rng(3).integers(0, 256, (9, 11, 4)).astype(np.uint8)
        img[:, :, 3] = 0
    else:
        h, w = (1, 1) if name == "1x1" else (1, 7)
        img = np.random.default_rng(4).integers(0, 256, (h, w, 4)).astype(np.uint8)
        img[:, :, 3] = 0
        if w > 1:
            img[0, 1, 3] = 9                         # one opaque pixel: the colour moves one pixel per pass to either side
    for passes in (0, 1, 2, 3, 11):
        want = bleed_ref(img, passes)[:, :, :3]
        assert np.array_equal(dev_bleed(gpu, img, passes), want), (name, passes)
    if name in IMG:
        # the cases mean something: pixels change in every one of the first passes, and some stay out of reach
        assert all((bleed_ref(img, p + 1) != bleed_ref(img, p)).any() for p in range(3))
        assert not reached(img, P_USED).all()
        if name == "b":
            assert not reached(img, 11).all()


def test_bleed_trim_releases_and_next_call_allocates_again(gpu):
    img = image("a")
    want = bleed_ref(img, 3)[:, :, :3]
    assert np.array_equal(dev_bleed(gpu, img, 3), want)
    gpu.bleed_rgba_u8_trim()
    gpu.bleed_rgba_u8_trim()                             # nothing left: a no-op
    assert np.array_equal(dev_bleed(gpu, img, 3), want)


# ---- 2 + 3. colour bytes and alpha bytes, GPU against GPU, exact ----
@pytest.mark.parametrize("route,case,opt", ROUTE_OPTS, ids=["%s-%s-%s" % t for t in ROUTE_OPTS])
def test_colour_and_alpha_bytes(gpu, models, route, case, opt):
    _, noise, scale, img, it, shrink = c = case_of(route, case)
    o = opts_of(gpu, opt)
    got = call4(gpu, models, c, o, P_USED)
    h, w, _ = image(img).shape
    assert got.shape == final_size(h, w, it, shrink) + (4,) and got.dtype == np.uint8
    want = call3(gpu, models, route, bled(img, P_USED)[:, :, :3], noise, scale, it, shrink, o)
    assert np.array_equal(got[:, :, :3], want), "colour = the 3-channel call on the bled image"
    assert not np.array_equal(want, call3(gpu, models, route, image(img)[:, :, :3], noise, scale, it, shrink, o)), "the bleed shows in the result"
    alpha = image(img)[:, :, 3]
    if it == 0:
        assert np.array_equal(got[:, :, 3], alpha), "noise only: alpha out = alpha in"
    elif route == "rgb":
        grey = call3(gpu, models, route, np.dstack([alpha] * 3), None, scale, it, shrink, o)
        assert np.array_equal(got[:, :, 3], grey[:, :, 1]), "alpha = channel 1 of the scale-only RGB call on (A, A, A)"
    elif not shrink:
        assert np.array_equal(got[:, :, 3], nn2x_chain(gpu, models[scale], alpha, it, opts_of(gpu, opt, device=0))), "alpha = convert_plane_nn2x_device's plane, rounded"


@pytest.mark.parametrize("route", ["y", "rgb"])
def test_bleed_passes_argument(gpu, models, route):
    c = case_of(route, "noise_scale")
    _, noise, scale, img, it, shrink = c
    off = call4(gpu, models, c, None, 0)
    assert np.array_equal(off[:, :, :3], call3(gpu, models, route, image(img)[:, :, :3], noise, scale, it, shrink, None)), "bleed_passes = 0: the colour as it is"
    auto = len(layers(noise)) + len(layers(scale))           # < 0: the layer counts of the models given
    want = call3(gpu, models, route, bled(img, auto)[:, :, :3], noise, scale, it, shrink, None)
    got = call4(gpu, models, c, None, -1)
    assert np.array_equal(got[:, :, :3], want)
    assert not np.array_equal(got[:, :, :3], call4(gpu, models, c, None, P_USED)[:, :, :3])
    assert np.array_equal(got[:, :, 3], off[:, :, 3]), "alpha does not depend on the bleed"
    assert np.array_equal(call4(gpu, models, c, None, 1 << 30)[:, :, :3],
                          call3(gpu, models, route, bled(img, 52)[:, :, :3], noise, scale, it, shrink, None)), "passes beyond max(w, h) - 1 change nothing"


# ---- 3b. no scale pass but a shrink (the CLI's -m noise_scale --scale_ratio 0.3: 0 iterations, shrink 0.6): alpha is resized, not cropped ----
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_noise_with_shrink_resizes_alpha(gpu, models, route):
    noise, img, shrink = ("yn" if route == "y" else "m7"), "b", 0.6
    src = image(img)
    h, w, _ = src.shape
    H, W = final_size(h, w, 0, shrink)
    assert (H, W) == (22, 31) and (H, W) != (h, w)
    # the oracle's INTER_LINEAR on alpha / 255 (its float order is k_resize_linear's: the 3-channel shrink cases are byte-exact against it), rounded
    x = orc.resize_linear(src[:, :, 3].astype(np.float32) * np.float32(1 / 255), W, H)
    want_a = np.clip(np.rint(x * np.float32(255)), 0, 255).astype(np.uint8)
    assert not np.array_equal(want_a, src[:H, :W, 3])                      # (the crop would not pass)
    for opt in ("default", "fusion_off"):
        o = opts_of(gpu, opt)
        got = gpu.process_image_rgba_u8(src, models[noise], None, 0, o, shrink, P_USED)
        assert got.shape == (H, W, 4)
        assert np.array_equal(got[:, :, :3], call3(gpu, models, route, bled(img, P_USED)[:, :, :3], noise, None, 0, shrink, o)), opt
        assert np.array_equal(got[:, :, 3], want_a), opt
    assert np.array_equal(device_call(gpu, models, src, noise, None, 0, shrink, P_USED, in_pad=(1, 3, 2), out_pad=(2, 1, 3)), got)


# ---- 4. alpha against the oracle (Y route) ----
@functools.lru_cache(maxsize=None)
def oracle_alpha(case):
    _, _, scale, img, it, shrink = case_of("y", case)
    ls = layers(scale)
    o, n = orc.Oracle(ls), len(ls)
    x = image(img)[:, :, 3].astype(np.float32) * np.float32(1 / 255)
    for _ in range(it):
        up = orc.resize2x_nearest(x)
        h, w = up.shape
        t = np.pad(up[None], ((0, 0), (n, n), (n, n)), mode="edge")
        for l in range(n):
            t = o.filter(l, t, njob=4)
        x = np.ascontiguousarray(t[0, n:n + h, n:n + w])
    if shrink:
        H, W = final_size(image(img).shape[0], image(img).shape[1], it, shrink)
        x = orc.resize_linear(x, W, H)
    want = np.clip(np.rint(x * np.float32(255)), 0, 255).astype(np.uint8)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("case", ["scale1", "ratio1.5"])
def test_alpha_against_oracle(gpu, models, case):
    want = oracle_alpha(case)
    inside = float(((want >= 1) & (want <= 254)).mean())
    print("share of the expected alpha bytes in 1..254: %.3f" % inside)
    assert inside >= 0.3, "saturation must not hide the values"
    c = case_of("y", case)
    assert np.array_equal(call4(gpu, models, c, opts_of(gpu, "direct"), P_USED)[:, :, 3], want), "the reference-ordered kernels give the oracle's bytes"
    got = call4(gpu, models, c, None, P_USED)[:, :, 3]
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print("%s: max diff %d LSB on %.5f of the bytes" % (case, diff.max(), (diff != 0).mean()))
    assert diff.max() <= 1 and (diff != 0).mean() < 0.01, (case, int(diff.max()), float((diff != 0).mean()))


# ---- 5. alpha rides with Y: the launches of the 3-channel call ----
def test_launch_counts_equal_three_channel_call(gpu, models):
    img = np.random.default_rng(64).integers(0, 256, (64, 64, 4)).astype(np.uint8)
    o = gpu.make_opts(device=0, profile=1)
    counts = {}
    for name, f, src in (("rgba", gpu.process_image_rgba_u8, img), ("three", gpu.process_image_u8, np.ascontiguousarray(img[:, :, :3]))):
        for m in ("yn", "ys"):
            models[m].profile_reset(0)
        f(src, models["yn"], models["ys"], 2, o)
        torch.cuda.synchronize()
        counts[name] = [models[m].profile_read(0)[1] for m in ("yn", "ys")]
    print(counts)
    assert counts["three"] == [[0] + [1] * 6, [0] + [2] * 6]
    assert counts["rgba"] == counts["three"]


# ---- 6. host form, device form, ROIs ----
def device_call(gpu, models, src, noise, scale, it, shrink=0.0, passes=-1, in_pad=(0, 0, 0), out_pad=(0, 0, 0), **opt):
    """the device form with the input / output as an ROI: *_pad = (rows above, bytes in front of a row, bytes behind it); returns the output ROI after
    checking that every byte around it -- behind 4 W in each row included -- kept its 0xAB"""
    h, w, _ = src.shape
    H, W = final_size(h, w, it, shrink)
    ia, il, ir = in_pad
    oa, ol, orr = out_pad
    irs, ors = il + w * 4 + ir, ol + W * 4 + orr
    host = np.full((ia + h + 1, irs), 0x5A, np.uint8)
    host[ia:ia + h, il:il + w * 4] = src.reshape(h, w * 4)
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((oa + H + 1, ors), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    gpu.process_image_rgba_u8_device(d_in.data_ptr() + ia * irs + il, irs, w, h, d_out.data_ptr() + oa * ors + ol, ors,
                                     models[noise] if noise else None, models[scale] if scale else None, it, shrink, passes, stream=st.cuda_stream,
                                     opts=gpu.make_opts(device=0, **opt))
    st.synchronize()
    b = d_out.cpu().numpy()
    guard = np.ones(b.shape, bool)
    guard[oa:oa + H, ol:ol + W * 4] = False
    assert (b[guard] == 0xAB).all(), "bytes outside the output ROI were written"
    assert np.array_equal(d_in.cpu().numpy(), host), "the input was written"
    return b[oa:oa + H, ol:ol + W * 4].reshape(H, W, 4).copy()


@pytest.mark.parametrize("route", ["y", "rgb"])
def test_host_form_device_form_and_roi(gpu, models, route):
    for name in ("scale1", "noise", "ratio1.5"):
        c = case_of(route, name)
        _, noise, scale, img, it, shrink = c
        want = call4(gpu, models, c, None, -1)
        assert np.array_equal(device_call(gpu, models, image(img), noise, scale, it, shrink), want), name
        # 53 pixels = 212 bytes, 36 = 144: row strides that are no multiple of 4, an ROI inside larger buffers
        assert np.array_equal(device_call(gpu, models, image(img), noise, scale, it, shrink, in_pad=(2, 7, 6), out_pad=(3, 5, 6)), want), name
        assert np.array_equal(call4(gpu, models, c, None, -1), want), "repeated calls on one model are identical"


# ---- 7. nothing is read that the call did not write ----
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_scratch_independence_and_trim(gpu, models, route):
    for name in ("noise_scale", "ratio1.5"):
        c = case_of(route, name)
        first = call4(gpu, models, c, None, -1)
        for word in WORDS:
            for ms in models.values():
                ms.fill_scratch(word)
            assert np.array_equal(call4(gpu, models, c, None, -1), first), (name, hex(word))
        for ms in models.values():
            ms.trim()
        assert all(ms.fill_scratch(0) == 0 for ms in models.values()), "trim released every buffer, the RGBA call's included"
        assert np.array_equal(call4(gpu, models, c, None, -1), first), "after trim the next call allocates again"


# ---- 8. the CLI ----
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_cli_alpha_route(gpu, models, route, tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    scale = "ys" if route == "y" else "m4"
    gen_model.write_json(layers(scale), str(tmp_path / "scale2.0x_model.json"))
    src = np.random.default_rng(21).integers(1, 256, (20, 16, 4)).astype(np.uint8)
    src[:7, 10:, 3] = 0                                                        # a transparent corner
    flip = (lambda a: a) if route == "rgb" else (lambda a: np.ascontiguousarray(a[:, :, [2, 1, 0, 3]] if a.shape[2] == 4 else a[:, :, ::-1]))
    for name, arr in (("alpha", src), ("opaque", np.dstack([src[:, :, :3], np.full((20, 16), 255, np.uint8)]))):
        Image.fromarray(arr).save(str(tmp_path / (name + ".png")))
        assert cli.main(["-i", str(tmp_path / (name + ".png")), "-o", str(tmp_path / (name + "_out.png")), "-m", "scale", "--model_dir", str(tmp_path)]) == 0
        out = Image.open(str(tmp_path / (name + "_out.png")))
        got = np.asarray(out)
        if name == "alpha":
            assert out.mode == "RGBA" and got.shape == (40, 32, 4)
            want = flip(gpu.process_image_rgba_u8(flip(arr), None, models[scale], 1, gpu.make_opts(precision=gpu.PRECISION_FP32)))
        else:                                                                  # an alpha that is 255 everywhere: the bytes the CLI gave before
            assert out.mode == "RGB" and got.shape == (40, 32, 3)
            want = flip(call3(gpu, models, route, flip(np.ascontiguousarray(arr[:, :, :3])), None, scale, 1, 0.0, gpu.make_opts(precision=gpu.PRECISION_FP32)))
        assert np.array_equal(got, want), name
