"""GPU tests of the RGB-model surface: w2xc_convert_planes_nn2x_device, w2xc_process_image_rgb_u8_ex[_device] / _batch[_device], the colour building
blocks and the CLI route -- against an expectation composed from the CPU oracle (replicate pad by n, chained Oracle.filter, crop; resize2x_nearest and
resize_linear per plane; img * (1 / 255); clip(rint(255 x), 0, 255)), and against each other: the route whose first / last layer reads / writes the
uint8 image itself must give the bytes of the route through float planes.

Oracle results are computed once per (models, image, case) and shared (CASES / expected()).  Gate of the uint8 pipeline with the default (Winograd)
kernels: at most 1 LSB on fewer than 1 % of the bytes, the project's gate for the Y pipeline; a torch fp32 / fp64 restatement of these models and images
differs on <= 4e-5 of the bytes, by 1 LSB."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, assert_close
from tools import gen_model
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f
TOPO = {"m7": ([3, 32, 32, 64, 64, 128, 128, 3], 301), "m4": ([3, 32, 64, 64, 3], 302)}
IMG = {"a": (5, (24, 36, 3)), "b": (6, (37, 53, 3))}   # two tile columns with a ragged edge, odd sizes, more than one 8-row tile
# (name, noise model, scale model, image, iterations, shrink): scale x2 and x4, noise, noise + scale (two models, two contexts), ratio 1.5.
# With the oracle, 0.31 - 0.63 of the expected bytes of these cases lie in 1..254 (m4 as noise model in front of m7 would leave 0.23: not used).
CASES = [("scale1", None, "m7", "b", 1, 0.0), ("scale2", None, "m4", "a", 2, 0.0), ("noise", "m7", None, "a", 0, 0.0),
         ("noise_scale", "m7", "m4", "b", 1, 0.0), ("ratio1.5", None, "m4", "b", 1, 0.75), ("scale1_small", None, "m4", "a", 1, 0.0)]
CASE_IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@functools.lru_cache(maxsize=None)
def layers(name):
    return gen_model.synth_layers(*TOPO[name])


@functools.lru_cache(maxsize=None)
def image(name):
    seed, shape = IMG[name]
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


@pytest.fixture(scope="module")
def models(gpu):
    return {k: gpu._ModelSet.from_layers(layers(k)) for k in TOPO}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return orc.Oracle(layers(name))


def oracle_cnn(name, x):
    """convertWithModels' wrapper on the planes x (3, h, w): replicate pad by the layer count, every layer, crop -- all output planes"""
    n = len(layers(name))
    _, h, w = x.shape
    t = np.pad(x, ((0, 0), (n, n), (n, n)), mode="edge")
    for l in range(n):
        t = _oracle(name).filter(l, t, njob=4)
    return np.ascontiguousarray(t[:, n:n + h, n:n + w])


def to_planes(img):
    return np.ascontiguousarray((img.astype(np.float32) * np.float32(1 / 255)).transpose(2, 0, 1))


def to_u8(x):
    return np.ascontiguousarray(np.clip(np.rint(x * np.float32(255)), 0, 255).astype(np.uint8).transpose(1, 2, 0))


def final_size(h, w, it, shrink):
    H, W = h << it, w << it
    if shrink:
        W, H = int(float(W * shrink)), int(float(H * shrink))
    return H, W


@functools.lru_cache(maxsize=None)
def expected_planes(noise, scale, img, it, shrink):
    x = to_planes(image(img))
    if noise:
        x = oracle_cnn(noise, x)
    for _ in range(it):
        x = oracle_cnn(scale, np.stack([orc.resize2x_nearest(p) for p in x]))
    if shrink:
        H, W = final_size(image(img).shape[0], image(img).shape[1], it, shrink)
        x = np.stack([orc.resize_linear(p, W, H) for p in x])
    x.setflags(write=False)
    return x


def expected(case):
    _, noise, scale, img, it, shrink = case
    want = to_u8(expected_planes(noise, scale, img, it, shrink))
    want.setflags(write=False)
    return want


def run(gpu, models, case, **opt):
    _, noise, scale, img, it, shrink = case
    return gpu.process_image_rgb_u8(image(img), models[noise] if noise else None, models[scale] if scale else None, it,
                                    gpu.make_opts(**opt) if opt else None, shrink)


def gate(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print("%s: max diff %d LSB on %.5f of the bytes" % (what, diff.max(), (diff != 0).mean()))
    assert diff.max() <= 1 and (diff != 0).mean() < 0.01, (what, int(diff.max()), float((diff != 0).mean()))


def dev_planes(gpu, ms, x, nn2x, **opt):
    """convert_planes[_nn2x]_device on the host planes x (3, h, w) -> (3, h << nn2x, w << nn2x)"""
    _, h, w = x.shape
    H, W = h << nn2x, w << nn2x
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    f = ms.convert_planes_nn2x_device if nn2x else ms.convert_planes_device
    f(3, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), H * W * 4, W * 4, stream=st.cuda_stream, opts=gpu.make_opts(device=0, **opt))
    st.synchronize()
    return d_out.cpu().numpy()


# ---- 1. float planes: the values before the uint8 clip ----
@pytest.mark.parametrize("model,img", [("m7", "b"), ("m4", "a")])
def test_planes_nn2x_against_oracle(gpu, models, model, img):
    x = to_planes(image(img))
    want = expected_planes(None, model, img, 1, 0.0)
    outside = float(((want < 0) | (want > 1)).mean())
    print("share of the expected values outside [0, 1]: %.3f" % outside)
    assert outside > 0.3     # (this is the test the clip cannot help)
    fast = dev_planes(gpu, models[model], x, 1)
    assert_close(fast, want, "%s nn2x, default kernels" % model)
    direct = dev_planes(gpu, models[model], x, 1, kernel=gpu.KERNEL_DIRECT)
    assert np.array_equal(direct, want), "the reference-ordered kernel is bit-identical to the oracle"
    up = np.stack([orc.resize2x_nearest(p) for p in x])
    assert np.array_equal(fast, dev_planes(gpu, models[model], up, 0)), "nn2x folded into layer 1 == the explicitly upscaled planes"
    assert np.array_equal(direct, dev_planes(gpu, models[model], up, 0, kernel=gpu.KERNEL_DIRECT))


# ---- 2. the uint8 pipeline against the oracle ----
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_pipeline_against_oracle(gpu, models, case):
    want = expected(case)
    inside = float(((want >= 1) & (want <= 254)).mean())
    print("share of the expected bytes in 1..254: %.3f" % inside)
    assert inside >= 0.30, "the clip must not hide the values"
    assert want.shape[:2] == final_size(image(case[3]).shape[0], image(case[3]).shape[1], case[4], case[5])
    assert np.array_equal(run(gpu, models, case, kernel=gpu.KERNEL_DIRECT), want), "the reference-ordered kernels give the oracle's bytes"
    gate(run(gpu, models, case), want, case[0])


# a noise pass and no 2x step in front of the shrink: resize scales of 2 and above (the cases of CASES stay as they are: other tests index them)
NOISE_SHRINK = [("noise_shrink%g_%s" % (s, img), "m7", None, img, 0, s) for img in ("a", "b") for s in (0.3, 0.5, 0.6)]


@pytest.mark.parametrize("case", NOISE_SHRINK, ids=[c[0] for c in NOISE_SHRINK])
def test_noise_then_shrink_against_oracle(gpu, models, case):
    want = expected(case)
    assert want.shape[:2] == final_size(image(case[3]).shape[0], image(case[3]).shape[1], 0, case[5])
    assert np.array_equal(run(gpu, models, case, kernel=gpu.KERNEL_DIRECT), want), "the reference-ordered kernels give the oracle's bytes"
    gate(run(gpu, models, case), want, case[0])


# ---- 3. the uint8 first / last layers give the bytes of the route through float planes ----
def composed(gpu, models, case):
    """w2xc_u8_to_rgb_device -> convert_planes[_nn2x]_device per pass -> (the shrink: the oracle's resize_linear on the downloaded planes, the ABI
    has no such building block) -> w2xc_rgb_to_u8_device"""
    _, noise, scale, img, it, shrink = case
    src = image(img)
    h, w, _ = src.shape
    st = torch.cuda.current_stream()
    d_img = torch.from_numpy(src).cuda()
    d_pl = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    gpu.u8_to_rgb_device(d_img.data_ptr(), w * 3, w, h, d_pl.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    x = d_pl.cpu().numpy()
    assert np.array_equal(x, to_planes(src)), "u8 -> float planes is the oracle's expression"
    if noise:
        x = dev_planes(gpu, models[noise], x, 0)
    for _ in range(it):
        x = dev_planes(gpu, models[scale], x, 1)
    if shrink:
        H, W = final_size(h, w, it, shrink)
        x = np.stack([orc.resize_linear(p, W, H) for p in x])
    _, H, W = x.shape
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.rgb_to_u8_device(d_x.data_ptr(), W, H, d_out.data_ptr(), W * 3, stream=st.cuda_stream)
    st.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fused_equals_unfused(gpu, models, case):
    got = run(gpu, models, case)
    assert np.array_equal(got, run(gpu, models, case, fusion=gpu.FUSION_OFF)), "W2XC_FUSION_OFF: colour kernels around float planes"
    assert np.array_equal(got, composed(gpu, models, case)), "the explicit composition of the building blocks"
    assert np.array_equal(got, run(gpu, models, case, band_rows=8)), "several bands through the uint8 source and sink"
    assert np.array_equal(got, run(gpu, models, case, band_rows=8, fusion=gpu.FUSION_OFF))


# ---- 4. the fusion really happens: the float planes of both levels are never allocated ----
def test_fused_call_has_no_float_image(gpu):
    img = image("b")
    h, w, _ = img.shape
    used = {}
    for name, opt in (("default", {}), ("off", dict(fusion=gpu.FUSION_OFF))):
        ms = gpu._ModelSet.from_layers(layers("m7"))      # fresh: its scratch buffers have only this call's sizes
        gpu.process_image_rgb_u8(img, None, ms, 1, gpu.make_opts(**opt) if opt else None)
        used[name] = ms.fill_scratch(0)
    print("scratch bytes: %r; float planes of both levels: %d" % (used, 15 * w * h * 4))
    assert used["default"] < used["off"]
    assert used["off"] - used["default"] >= 15 * w * h * 4


# ---- 5. edges ----
def device_call(gpu, models, src, noise, scale, it, shrink=0.0, in_pad=(0, 0, 0), out_pad=(0, 0, 0), **opt):
    """the device form with the input / output as an ROI: *_pad = (rows above, bytes in front of a row, bytes behind it); returns the output ROI after
    checking that every byte around it kept its 0xAB"""
    h, w, _ = src.shape
    H, W = final_size(h, w, it, shrink)
    ia, il, ir = in_pad
    oa, ol, orr = out_pad
    irs, ors = il + w * 3 + ir, ol + W * 3 + orr
    host = np.full((ia + h + 1, irs), 0x5A, np.uint8)
    host[ia:ia + h, il:il + w * 3] = src.reshape(h, w * 3)
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((oa + H + 1, ors), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    gpu.process_image_rgb_u8_device(d_in.data_ptr() + ia * irs + il, irs, w, h, d_out.data_ptr() + oa * ors + ol, ors,
                                    models[noise] if noise else None, models[scale] if scale else None, it, shrink, stream=st.cuda_stream,
                                    opts=gpu.make_opts(device=0, **opt))
    st.synchronize()
    b = d_out.cpu().numpy()
    guard = np.ones(b.shape, bool)
    guard[oa:oa + H, ol:ol + W * 3] = False
    assert (b[guard] == 0xAB).all(), "bytes outside the output ROI were written"
    return b[oa:oa + H, ol:ol + W * 3].reshape(H, W, 3).copy()


@pytest.mark.parametrize("hw", [(1, 1), (9, 33)])      # 33 wide: one pixel in the second tile column
def test_tiny_and_ragged_images(gpu, models, hw):
    src = np.random.default_rng(40 + hw[1]).integers(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)
    want = to_u8(oracle_cnn("m4", np.stack([orc.resize2x_nearest(p) for p in to_planes(src)])))
    assert np.array_equal(gpu.process_image_rgb_u8(src, None, models["m4"], 1, gpu.make_opts(kernel=gpu.KERNEL_DIRECT)), want)
    got = gpu.process_image_rgb_u8(src, None, models["m4"], 1)
    gate(got, want, "%dx%d" % (hw[1], hw[0]))
    assert np.array_equal(got, gpu.process_image_rgb_u8(src, None, models["m4"], 1, gpu.make_opts(fusion=gpu.FUSION_OFF)))
    assert np.array_equal(got, device_call(gpu, models, src, None, "m4", 1, out_pad=(1, 5, 3)))


def test_input_and_output_as_roi(gpu, models):
    src = image("a")                                  # 36 pixels = 108 bytes per row
    want = run(gpu, models, CASES[5])                 # ("scale1_small", None, "m4", "a", 1, 0.0)
    in_pad = (2, 7, 150 - 108 - 7)
    assert sum(in_pad[1:]) + 108 == 150               # a row stride that is no multiple of 4
    for opt in ({}, dict(fusion=gpu.FUSION_OFF), dict(band_rows=8)):
        got = device_call(gpu, models, src, None, "m4", 1, in_pad=in_pad, out_pad=(3, 5, 6), **opt)   # (output rows 5 + 216 + 6 = 227 bytes apart)
        assert np.array_equal(got, want), opt
    noise_want = run(gpu, models, CASES[2])           # noise only: source and sink of ONE pass are both uint8
    assert np.array_equal(device_call(gpu, models, src, "m7", None, 0, in_pad=in_pad, out_pad=(1, 1, 2)), noise_want)


# ---- 6. batches ----
def batch_images(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3)).astype(np.uint8)


def device_batch(gpu, x, noise, scale, it, opts):
    n, h, w, _ = x.shape
    H, W = final_size(h, w, it, 0.0)
    irs, ors = w * 3 + 5, W * 3 + 7
    src = torch.full((n, h + 1, irs), 0x5A, dtype=torch.uint8)
    src[:, 1:, :w * 3] = torch.from_numpy(x.reshape(n, h, w * 3))
    d_in = src.cuda()
    d_out = torch.full((n, H + 2, ors), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    gpu.process_image_rgb_u8_batch_device(n, d_in.data_ptr() + irs, (h + 1) * irs, irs, w, h, d_out.data_ptr() + 2 * ors, (H + 2) * ors, ors,
                                          noise, scale, it, 0.0, stream=st.cuda_stream, opts=opts)
    st.synchronize()
    b = d_out.cpu().numpy()
    guard = np.ones(b.shape, bool)
    guard[:, 2:, :W * 3] = False
    assert (b[guard] == 0xAB).all(), "bytes outside the output images were written"
    return b[:, 2:, :W * 3].reshape(n, H, W, 3).copy()


@pytest.mark.parametrize("n", [1, 3, 5])
def test_batches_equal_single_calls(gpu, models, n):
    """160 x 168 images, x2, workspace_mb = 1: an image is 15 w h = 403 200 bytes of uint8 in and out with the uint8 layers (two per sub-batch: n = 3 and
    5 take two and three sub-batches) and 2.0 MB with W2XC_FUSION_OFF (one per sub-batch); the budget also cuts every image into bands"""
    h, w = 168, 160
    x = batch_images(n, h, w, 700 + n)
    ms = models["m4"]
    for opt in (dict(workspace_mb=1), dict(workspace_mb=1, fusion=gpu.FUSION_OFF), {}):
        o = gpu.make_opts(device=0, **opt)
        want = np.stack([gpu.process_image_rgb_u8(x[i], None, ms, 1, o) for i in range(n)])
        assert len({want[i].tobytes() for i in range(n)}) == n          # distinct images: an index mix-up cannot pass
        assert np.array_equal(device_batch(gpu, x, None, ms, 1, o), want), ("device form", opt)
        assert np.array_equal(gpu.process_image_rgb_u8_batch([x[i].copy() for i in range(n)], None, ms, 1, o), want), ("host form, pageable", opt)
        pin_in = torch.from_numpy(x.copy()).pin_memory()
        pin_out = torch.zeros((n, 2 * h, 2 * w, 3), dtype=torch.uint8).pin_memory()
        res = gpu.process_image_rgb_u8_batch(pin_in.numpy(), None, ms, 1, o, out=pin_out.numpy())
        assert np.array_equal(pin_out.numpy(), want) and np.shares_memory(res, pin_out.numpy()), ("host form, page-locked", opt)
    assert np.array_equal(want[0], gpu.process_image_rgb_u8(x[0], None, ms, 1))


def test_batch_noise_scale_small_images(gpu, models):
    x = batch_images(4, 24, 36, 77)
    want = np.stack([gpu.process_image_rgb_u8(x[i], models["m7"], models["m4"], 1) for i in range(4)])
    assert np.array_equal(gpu.process_image_rgb_u8_batch(x, models["m7"], models["m4"], 1), want)
    assert np.array_equal(device_batch(gpu, x, models["m7"], models["m4"], 1, gpu.make_opts(device=0)), want)
    shr = np.stack([gpu.process_image_rgb_u8(x[i], None, models["m4"], 1, None, 0.75) for i in range(4)])
    assert np.array_equal(gpu.process_image_rgb_u8_batch(x, None, models["m4"], 1, None, 0.75), shr)


# ---- 7. nothing is read that the call did not write ----
@pytest.mark.parametrize("fusion", ["auto", "off"])
def test_scratch_independence(gpu, models, fusion):
    case = CASES[3]      # noise + scale: both models' contexts
    opt = {} if fusion == "auto" else dict(fusion=gpu.FUSION_OFF)
    first = run(gpu, models, case, **opt)
    for word in WORDS:
        for ms in models.values():
            ms.fill_scratch(word)
        assert np.array_equal(run(gpu, models, case, **opt), first), hex(word)


# ---- 8. the CLI picks the RGB route by the model's first layer ----
def test_cli_rgb_route(gpu, tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    gen_model.write_json(layers("m4"), str(tmp_path / "scale2.0x_model.json"))
    src = np.random.default_rng(9).integers(0, 256, (20, 30, 3)).astype(np.uint8)
    Image.fromarray(src).save(str(tmp_path / "in.png"))
    assert cli.main(["-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "out.png"), "-m", "scale", "--model_dir", str(tmp_path)]) == 0
    got = np.asarray(Image.open(str(tmp_path / "out.png")).convert("RGB"))
    want = to_u8(oracle_cnn("m4", np.stack([orc.resize2x_nearest(p) for p in to_planes(src)])))    # PIL's RGB order as it is: no BGR swap
    gate(got, want, "CLI -m scale")
