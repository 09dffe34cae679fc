"""GPU tests of upconv head models (include/w2xc_hip.h, "upconv head models"): w2xc_convert_planes_up2x_device and the RGB image call with a head model as
scale model, against the torch float64 restatement of tests/upconv_ref.py and against each other.

Gate of the float planes: the project's fp32 gate against float64, max|gpu - ref| / max|ref| <= 1e-4 and elementwise <= 1e-4 |ref| + 1e-5 (SURVEY 8c,
derived for the Winograd chain; the head adds about 1e-6).  References are computed once per (model, size) and shared.  With W2XC_UPCONV_ERRORS naming a
file the measured errors of every parity case are appended to it (profiles/upconv_errors.txt is such a run)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import RTOL, ATOL
from tools import gen_model
import upconv_ref as ur

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f
# name -> (3x3 planes, head planes out, seed)
TOPO = {"pub": (ur.PUBLISHED, 3, gen_model.SEEDS["upconv7"]), "c32": ([3, 32], 3, 401), "c64y": ([1, 32, 64], 1, 402), "noise": ([3, 32, 32, 3], None, 403)}
# upconv4x4_head: tiles of 8 x 32 source pixels, w2xc_upconv_grid(tiles) = min(tiles, 512) workgroups (w2xc_pack.cpp) -- a strip of one tile row and 514
# tile columns (the last one a single pixel wide) has more tiles than workgroups: every workgroup walks a run of two tiles, the last runs are short or empty
STRIP = (8, 32 * 513 + 1)
assert -(-STRIP[1] // 32) > 512
# 40 x 70: 5 x 3 head tiles, the middle ones interior
PARITY = [("pub", 1, 1), ("pub", 17, 33), ("pub", 40, 70), ("c32", 17, 33), ("c64y", 17, 33), ("c32",) + STRIP]
DIRECT = [("pub", 1, 1), ("pub", 17, 33), ("pub", 40, 70)]


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


@functools.lru_cache(maxsize=None)
def source(name, h, w):
    x = np.random.default_rng(h * 1000 + w).random((arrays(name)[0][0][0], h, w), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, h, w):
    ref = ur.reference(*arrays(name), source(name, h, w))
    ref.setflags(write=False)
    return ref


def up2x(gpu, ms, x, in_pad=0, out_pad=0, **opt):
    """w2xc_convert_planes_up2x_device on the host planes x [n, h, w] -> [nout, 2h, 2w]; rows in_pad / out_pad floats longer than the planes,
    the output buffer pre-filled with a sentinel that must survive everywhere but in the planes"""
    n, h, w = x.shape
    nout = ms.planes(ms.n_layers - 1)[1]
    d_in = torch.zeros((n, h, w + in_pad), dtype=torch.float32, device="cuda")
    d_in[:, :, :w] = torch.from_numpy(np.array(x)).cuda()
    d_out = torch.full((nout, 2 * h + 1, 2 * w + out_pad), -7.25, dtype=torch.float32, device="cuda")
    ms.convert_planes_up2x_device(n, d_in.data_ptr(), d_in.stride(0) * 4, d_in.stride(1) * 4, w, h, d_out.data_ptr(), d_out.stride(0) * 4,
                                  d_out.stride(1) * 4, stream=torch.cuda.current_stream().cuda_stream, opts=gpu.make_opts(device=0, **opt))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:, 2 * h:, :] == -7.25).all() and (out[:, :, 2 * w:] == -7.25).all(), "bytes outside the output planes were written"
    return np.ascontiguousarray(out[:, :2 * h, :2 * w])


def gate(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    rel, worst = err.max() / np.abs(ref).max(), (err / (RTOL * np.abs(ref) + ATOL)).max()
    line = "%s: max|gpu - ref| / max|ref| = %.3g, worst elementwise err / (1e-4 |ref| + 1e-5) = %.3g" % (what, rel, worst)
    print(line)
    if os.environ.get("W2XC_UPCONV_ERRORS"):
        with open(os.environ["W2XC_UPCONV_ERRORS"], "a") as f:
            f.write(line + "\n")
    assert np.isfinite(got).all(), what
    assert rel <= RTOL and worst <= 1.0, line


# ---- orientation, to the bit ----
def test_orientation_single_taps(gpu):
    h, w = 5, 9
    x = ur.ramp_planes(3, h, w)
    w1 = np.zeros((32, 3, 3, 3), np.float32)
    for p in range(3):
        w1[p, p, 1, 1] = 1.0   # the one 3x3 layer copies source plane p to plane p of 32 (positive inputs: LeakyReLU is the identity)
    z = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="edge")   # pad 2, one valid layer: the source with a one-pixel replicated rim
    bias = np.array([0.125, -0.3, 0.7], np.float64)
    for r in range(4):
        for s in range(4):
            c0, o0 = (r + s) % 3, (4 * r + s) % 3
            hw = np.zeros((32, 3, 4, 4), np.float32)
            hw[c0, o0, r, s] = 1.0
            ms = gpu._ModelSet.from_layers([(3, 32, w1, np.zeros(32))], head=(hw, bias))
            got = up2x(gpu, ms, x)
            want = np.broadcast_to(bias.astype(np.float32)[:, None, None], (3, 2 * h, 2 * w)).copy()
            for Y in range(2 * h):
                for X in range(2 * w):
                    if (Y + 3 - r) % 2 == 0 and (X + 3 - s) % 2 == 0:   # Y = 2 i - 3 + r: weight [in][out][r][s]
                        want[o0, Y, X] = np.float32(z[c0, (Y + 3 - r) // 2, (X + 3 - s) // 2]) + np.float32(bias[o0])
            assert (want < 0).any()   # (a LeakyReLU behind the head would scale the negative bias)
            assert np.array_equal(got, want), (r, s, np.abs(got - want).max())


# ---- parity with float64 ----
@pytest.mark.parametrize("name,h,w", PARITY, ids=["%s-%dx%d" % c for c in PARITY])
def test_parity_default_kernels(gpu, models, name, h, w):
    ms = models[name]
    assert "conv3x3_direct" not in [ms.kernel_name(l) for l in range(ms.n_layers)]
    gate(up2x(gpu, ms, source(name, h, w)), reference(name, h, w), "%s %dx%d default" % (name, h, w))


@pytest.mark.parametrize("name,h,w", DIRECT, ids=["%s-%dx%d" % c for c in DIRECT])
def test_parity_direct_kernel(gpu, models, name, h, w):
    gate(up2x(gpu, models[name], source(name, h, w), kernel=1), reference(name, h, w), "%s %dx%d W2XC_KERNEL_DIRECT" % (name, h, w))


# ---- banding ----
@pytest.mark.parametrize("h,w", [(17, 33), (40, 70)])
def test_bands_give_the_bits_of_the_unbanded_call(gpu, models, h, w):
    ms, x = models["pub"], source("pub", h, w)
    whole = up2x(gpu, ms, x)
    for opt in ({"band_rows": 4}, {"band_rows": 8}, {"band_rows": 12}, {"workspace_mb": 1}):
        plan = ms.plan_rows(w, h, opts=gpu.make_opts(**opt))
        assert plan.n_bands > 1, opt
        assert np.array_equal(up2x(gpu, ms, x, **opt), whole), opt
    direct = up2x(gpu, ms, x, kernel=1)
    assert np.array_equal(up2x(gpu, ms, x, kernel=1, band_rows=5), direct)   # (one halo row per layer: any band height)


# ---- strides and guards ----
@pytest.mark.parametrize("name", ["pub", "c64y"])
def test_odd_strides_and_guards(gpu, models, name):
    x = source(name, 17, 33)
    assert np.array_equal(up2x(gpu, models[name], x, in_pad=3, out_pad=5), up2x(gpu, models[name], x))


# ---- the image call ----
def image(h, w, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def image_device(gpu, img, noise, scale, it, shrink=0.0, out_pad=0, **opt):
    h, w, _ = img.shape
    H, W = h << it, w << it
    if shrink:
        W, H = int(float(W * shrink)), int(float(H * shrink))
    d_in = torch.from_numpy(img).cuda()
    d_out = torch.full((H + 1, W * 3 + out_pad), 0xA5, dtype=torch.uint8, device="cuda")
    gpu.process_image_rgb_u8_device(d_in.data_ptr(), w * 3, w, h, d_out.data_ptr(), d_out.stride(0), noise, scale, it, shrink,
                                    stream=torch.cuda.current_stream().cuda_stream, opts=gpu.make_opts(device=0, **opt))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[H:] == 0xA5).all() and (out[:, W * 3:] == 0xA5).all(), "bytes outside the output image were written"
    return np.ascontiguousarray(out[:H, :W * 3]).reshape(H, W, 3)


def test_image_call_is_the_composition(gpu, models):
    ms, img = models["pub"], image(17, 33)
    h, w, _ = img.shape
    st = torch.cuda.current_stream().cuda_stream
    d_img = torch.from_numpy(img).cuda()
    d_x = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    d_y = torch.empty((3, 2 * h, 2 * w), dtype=torch.float32, device="cuda")
    d_o = torch.empty((2 * h, 2 * w, 3), dtype=torch.uint8, device="cuda")
    gpu.u8_to_rgb_device(d_img.data_ptr(), w * 3, w, h, d_x.data_ptr(), st)
    ms.convert_planes_up2x_device(3, d_x.data_ptr(), h * w * 4, w * 4, w, h, d_y.data_ptr(), 4 * h * w * 4, 2 * w * 4, stream=st, opts=gpu.make_opts(device=0))
    gpu.rgb_to_u8_device(d_y.data_ptr(), 2 * w, 2 * h, d_o.data_ptr(), 2 * w * 3, st)
    torch.cuda.synchronize()
    want = d_o.cpu().numpy()
    assert 0.2 < ((want > 0) & (want < 255)).mean()   # (not a saturated image)
    auto = image_device(gpu, img, None, ms, 1, out_pad=7)
    assert np.array_equal(auto, want)
    assert np.array_equal(image_device(gpu, img, None, ms, 1, fusion=1), want)        # W2XC_FUSION_OFF: through float planes
    assert np.array_equal(gpu.process_image_rgb_u8(img, None, ms, 1), want)           # the host call
    assert np.array_equal(image_device(gpu, img, None, ms, 1, band_rows=4), want)     # banded, the head writing uint8 rows


@pytest.mark.parametrize("noise,it,shrink", [("noise", 1, 0.0), (None, 2, 0.0), (None, 1, 0.75), ("noise", 2, 0.6)], ids=["noise", "x4", "ratio1.5", "noise-x4-ratio"])
def test_image_call_fusion_auto_equals_off(gpu, models, noise, it, shrink):
    img = image(13, 21, 6)
    n = models[noise] if noise else None
    auto = image_device(gpu, img, n, models["pub"], it, shrink)
    assert np.array_equal(auto, image_device(gpu, img, n, models["pub"], it, shrink, fusion=1))
    assert np.array_equal(auto, gpu.process_image_rgb_u8(img, n, models["pub"], it, None, shrink))
    if it == 2 and not noise and not shrink:   # two iterations are two passes of the plane call
        x = np.ascontiguousarray((img.astype(np.float32) * np.float32(1 / 255)).transpose(2, 0, 1))
        y = up2x(gpu, models["pub"], up2x(gpu, models["pub"], x))
        assert np.array_equal(auto, np.clip(np.rint(y * np.float32(255)), 0, 255).astype(np.uint8).transpose(1, 2, 0))


# ---- poison ----
def test_poisoned_scratch_changes_nothing(gpu, models):
    ms, x, img = models["pub"], source("pub", 17, 33), image(17, 33)
    planes, picture = up2x(gpu, ms, x), image_device(gpu, img, models["noise"], ms, 1, 0.75)
    for word in WORDS:
        assert ms.fill_scratch(word) > 0
        assert np.array_equal(up2x(gpu, ms, x), planes), hex(word)
        assert ms.fill_scratch(word) > 0 and models["noise"].fill_scratch(word) > 0
        assert np.array_equal(image_device(gpu, img, models["noise"], ms, 1, 0.75), picture), hex(word)


# ---- the constructor, after the first use ----
def test_add_head_after_first_use_is_refused(gpu):
    layers, head = ur.head_model([3, 32], 3, 404)
    ms = gpu._ModelSet.from_layers(layers)
    x = torch.zeros((3, 8, 8), dtype=torch.float32, device="cuda")
    y = torch.empty((32, 8, 8), dtype=torch.float32, device="cuda")
    ms.convert_planes_device(3, x.data_ptr(), 256, 32, 8, 8, y.data_ptr(), 256, 32, opts=gpu.make_opts(device=0))
    torch.cuda.synchronize()
    with pytest.raises(gpu.W2xcError) as e:
        ms.add_upconv_head(*head)
    assert e.value.code == -3 and not ms.has_head
