"""GPU tests of test-time augmentation (include/w2xc_hip.h, "TTA"): the spread / gather kernels bit for bit against numpy; the plane calls against
the composition a caller had before (numpy T_k, 8 single calls, numpy T_k^-1, the float32 sum in the stated order); the image calls against the public
building blocks around the plane TTA call, and against the CPU oracle; batches; launch counts; poisoned scratch.

T_k: horizontal flip if k & 1, then vertical flip if k & 2, then transpose if k & 4.  TILE = the kernels' tile edge (w2xc_tta.hip).

Oracle cases (ORACLE_Y / ORACLE_RGB, all on the 24 x 36 image): share of the expected bytes in 1..254, computed on the CPU with the oracle -- Y route:
scale 0.587, noise 0.477, noise_scale 0.496, ratio1.5 0.596; RGB route: scale 0.667, noise 0.466, ratio1.5 0.666 (the cases without TTA have
0.31 - 0.63).  None of them saturates; the tests assert >= 0.30 before they rely on the gate."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from tools import gen_model
from oracle import oracle as orc

import test_gpu_rgb as R   # TOPO, IMG, the images, the RGB oracle composition and the project's gate for the uint8 pipeline

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 32
WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f
F32 = np.float32


def T(k, x):
    if k & 1:
        x = x[..., :, ::-1]
    if k & 2:
        x = x[..., ::-1, :]
    if k & 4:
        x = np.swapaxes(x, -1, -2)
    return np.ascontiguousarray(x)


def Tinv(k, x):
    if k & 4:
        x = np.swapaxes(x, -1, -2)
    if k & 2:
        x = x[..., ::-1, :]
    if k & 1:
        x = x[..., :, ::-1]
    return np.ascontiguousarray(x)


def tta_mean(vs):
    a = vs[0] + vs[1]
    for v in vs[2:]:
        a = a + v
    assert a.dtype == np.float32
    return a * F32(0.125)


def test_transforms_are_the_dihedral_group():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    seen = set()
    for k in range(8):
        assert np.array_equal(Tinv(k, T(k, x)), x)
        assert T(k, x).shape == ((3, 4) if k < 4 else (4, 3))
        seen.add(T(k, x).tobytes())
    assert len(seen) == 8
    assert np.array_equal(T(5, x), x[:, ::-1].T) and np.array_equal(T(6, x), x[::-1, :].T)


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@pytest.fixture(scope="module")
def ymodels(gpu, noise1_layers, scale_layers):
    return {"noise": gpu._ModelSet.from_layers(noise1_layers), "scale": gpu._ModelSet.from_layers(scale_layers)}


@pytest.fixture(scope="module")
def rgbmodels(gpu):
    return {k: gpu._ModelSet.from_layers(R.layers(k)) for k in R.TOPO}


def stream():
    return torch.cuda.current_stream()


# ---- 1. spread and gather alone ----
SHAPES = [(1, 1), (1, TILE + 6), (TILE + 6, 1), (TILE + 1, 2 * TILE + 1), (TILE, TILE), (2 * TILE + 1, TILE + 1)]


def variant_planes(buf, ps, n, k, shape):
    """the n planes of variant k in a group buffer (4 n planes ps floats apart), and what lies behind each plane's last element"""
    q = shape[0] * shape[1]
    rows = buf.reshape(4 * n, ps)[(k & 3) * n:(k & 3) * n + n]
    return rows[:, :q].reshape((n,) + shape), rows[:, q:]


# the second trips of the kernels' two grid-stride loops (tta_grid: at most 65536 tiles, 65535 planes): 65537 tiles along x, along y; 65537 planes of one tile.
# The tile loop's second trip reuses the LDS tile behind its leading barrier.
SECOND_TRIPS = [((1, TILE * 65536 + 1), 1), ((TILE * 65536 + 1, 1), 1), ((1, 1), 65537)]
SECOND_TRIP_IDS = ["%dx%d-n%d" % (s + (n,)) for s, n in SECOND_TRIPS]


def check_spread(gpu, hw, n):
    h, w = hw
    rs, ps = w + 3, w * h + 5
    sps = h * rs + 7
    rng = np.random.default_rng(h * 1000 + w + n)
    src = rng.standard_normal((n, sps)).astype(np.float32)
    x = np.ascontiguousarray(src[:, :h * rs].reshape(n, h, rs)[:, :, :w])
    d_src = torch.from_numpy(src).cuda()
    d_up = torch.full((4 * n * ps,), float("nan"), dtype=torch.float32, device="cuda")
    d_tr = torch.full((4 * n * ps,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.tta_spread_device(d_src.data_ptr(), n, sps * 4, rs * 4, w, h, d_up.data_ptr(), d_tr.data_ptr(), ps * 4, stream=stream().cuda_stream)
    stream().synchronize()
    up, tr = d_up.cpu().numpy(), d_tr.cpu().numpy()
    for k in range(8):
        got, behind = variant_planes(up if k < 4 else tr, ps, n, k, (h, w) if k < 4 else (w, h))
        assert np.array_equal(got.view(np.uint32), T(k, x).view(np.uint32)), k
        assert np.isnan(behind).all(), "variant %d: floats behind a plane's last element were written" % k


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_spread_bit_for_bit(gpu, hw, n):
    check_spread(gpu, hw, n)


@pytest.mark.parametrize("hw,n", SECOND_TRIPS, ids=SECOND_TRIP_IDS)
def test_spread_second_trips(gpu, hw, n):
    check_spread(gpu, hw, n)


def check_gather(gpu, hw, n):
    h, w = hw
    rs, ps = w + 3, w * h + 5
    dps = h * rs + 7
    rng = np.random.default_rng(h * 1000 + w + n + 7)
    r = []   # r[k]: (n, h, w) for k < 4, (n, w, h) above; mixed magnitudes: a reordered sum rounds differently
    for k in range(8):
        shape = (n, h, w) if k < 4 else (n, w, h)
        r.append((rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32))
    want = tta_mean([Tinv(k, r[k]) for k in range(8)])
    if h * w * n >= 64:
        other = tta_mean([Tinv(k, r[k]) for k in (7, 6, 5, 4, 3, 2, 1, 0)])
        assert not np.array_equal(want, other), "the inputs must tell the order of the sum"
    groups = []
    for k0 in (0, 4):
        g = np.full((4 * n, ps), np.nan, np.float32)
        for k in range(k0, k0 + 4):
            g[(k & 3) * n:(k & 3) * n + n, :w * h] = r[k].reshape(n, -1)
        groups.append(torch.from_numpy(g).cuda())
    d_dst = torch.full((n, dps), float("nan"), dtype=torch.float32, device="cuda")
    gpu.tta_gather_device(groups[0].data_ptr(), groups[1].data_ptr(), ps * 4, n, w, h, d_dst.data_ptr(), dps * 4, rs * 4, stream=stream().cuda_stream)
    stream().synchronize()
    dst = d_dst.cpu().numpy()
    rows = dst[:, :h * rs].reshape(n, h, rs)
    assert np.array_equal(np.ascontiguousarray(rows[:, :, :w]).view(np.uint32), want.view(np.uint32))
    assert np.isnan(rows[:, :, w:]).all() and np.isnan(dst[:, h * rs:]).all(), "floats outside the plane's rows were written"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_gather_bit_for_bit(gpu, hw, n):
    check_gather(gpu, hw, n)


@pytest.mark.parametrize("hw,n", SECOND_TRIPS, ids=SECOND_TRIP_IDS)
def test_gather_second_trips(gpu, hw, n):
    check_gather(gpu, hw, n)


# ---- 2. plane calls == the composition a caller had before ----
def optsets(gpu):
    return [("default", {}), ("direct", dict(kernel=gpu.KERNEL_DIRECT)), ("fusion_off", dict(fusion=gpu.FUSION_OFF)),
            ("bf16x2", dict(precision=gpu.PRECISION_BF16X2)), ("bands", dict(band_rows=8))]


def single_plane(gpu, ms, x, nn2x, o):
    h, w = x.shape
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((h << nn2x, w << nn2x), float("nan"), dtype=torch.float32, device="cuda")
    f = ms.convert_nn2x_device if nn2x else ms.convert_device
    f(d_in.data_ptr(), w * 4, w, h, d_out.data_ptr(), (w << nn2x) * 4, stream=stream().cuda_stream, opts=o)
    stream().synchronize()
    return d_out.cpu().numpy()


def batch_tta(gpu, ms, x, nn2x, o):
    """convert_batch_tta_device on x (n, h, w), the planes and rows of both sides padded"""
    n, h, w = x.shape
    H, W = h << nn2x, w << nn2x
    src = np.full((n, h + 1, w + 3), 7.0, np.float32)
    src[:, :h, :w] = x
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((n, H + 1, W + 5), float("nan"), dtype=torch.float32, device="cuda")
    ms.convert_batch_tta_device(n, d_in.data_ptr(), (h + 1) * (w + 3) * 4, (w + 3) * 4, w, h, d_out.data_ptr(), (H + 1) * (W + 5) * 4, (W + 5) * 4,
                                nn2x=bool(nn2x), stream=stream().cuda_stream, opts=o)
    stream().synchronize()
    out = d_out.cpu().numpy()
    assert np.isnan(out[:, H:, :]).all() and np.isnan(out[:, :, W:]).all(), "floats outside the output planes were written"
    return out[:, :H, :W].copy()


@pytest.mark.parametrize("nn2x", [0, 1])
@pytest.mark.parametrize("hw", [(24, 24), (37, 53)], ids=["24x24", "37x53"])
def test_batch_tta_equals_composition(gpu, ymodels, hw, nn2x):
    h, w = hw
    ms = ymodels["scale" if nn2x else "noise"]
    x = np.random.default_rng(h + nn2x).random((3, h, w), dtype=np.float32)
    for name, opt in optsets(gpu):
        o = gpu.make_opts(device=0, **opt)
        want = np.stack([tta_mean([Tinv(k, single_plane(gpu, ms, T(k, x[i]), nn2x, o)) for k in range(8)]) for i in range(3)])
        got = batch_tta(gpu, ms, x, nn2x, o)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, "n = 3")
        if name in ("default", "bands"):
            assert np.array_equal(batch_tta(gpu, ms, x[1:2], nn2x, o).view(np.uint32), want[1:2].view(np.uint32)), (name, "n = 1")


def planes_tta(gpu, ms, x, nn2x, o):
    _, h, w = x.shape
    H, W = h << nn2x, w << nn2x
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
    ms.convert_planes_tta_device(3, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), H * W * 4, W * 4, nn2x=bool(nn2x),
                                 stream=stream().cuda_stream, opts=o)
    stream().synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("nn2x", [0, 1])
@pytest.mark.parametrize("hw", [(24, 24), (37, 53)], ids=["24x24", "37x53"])
def test_planes_tta_equals_composition(gpu, rgbmodels, hw, nn2x):
    h, w = hw
    ms = rgbmodels["m4"]
    x = np.random.default_rng(h + nn2x + 50).random((3, h, w), dtype=np.float32)
    for name, opt in optsets(gpu):
        want = tta_mean([Tinv(k, R.dev_planes(gpu, ms, T(k, x), nn2x, **opt)) for k in range(8)])
        got = planes_tta(gpu, ms, x, nn2x, gpu.make_opts(device=0, **opt))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


# ---- 3. image calls == the public building blocks around the plane TTA call ----
# (name, noise, scale, image, iterations, shrink): the models by role for the Y route, by TOPO name for the RGB route
Y_CASES = [("scale", None, "scale", "b", 1, 0.0), ("scale_x4", None, "scale", "a", 2, 0.0), ("noise", "noise", None, "a", 0, 0.0),
           ("noise_scale", "noise", "scale", "b", 1, 0.0), ("ratio1.5", None, "scale", "b", 1, 0.75)]
RGB_CASES = R.CASES[:5]   # scale1, scale2 (x4), noise, noise_scale, ratio1.5


def y_tta_plane(gpu, ms, y, nn2x, **opt):
    return batch_tta(gpu, ms, y[None], nn2x, gpu.make_opts(device=0, **opt))[0]


def composed_y(gpu, ymodels, case, **opt):
    """w2xc_u8_to_yuv_device -> per pass convert_batch_tta_device on Y, w2xc_resize2x_cubic_device on U and V -> (the shrink: the oracle's resize_linear
    on the downloaded planes, the ABI has no such building block) -> w2xc_yuv_to_u8_device"""
    _, noise, scale, img, it, shrink = case
    src = R.image(img)
    h, w, _ = src.shape
    lib, st = gpu.lib(), stream()
    d_img = torch.from_numpy(src).cuda()
    d = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    assert lib.w2xc_u8_to_yuv_device(d_img.data_ptr(), w * 3, w, h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), st.cuda_stream) == 0
    st.synchronize()
    y, u, v = d.cpu().numpy()
    if noise:
        y = y_tta_plane(gpu, ymodels[noise], y, 0, **opt)
    for _ in range(it):
        y = y_tta_plane(gpu, ymodels[scale], y, 1, **opt)
        uv = []
        for p in (u, v):
            d_p = torch.from_numpy(np.ascontiguousarray(p)).cuda()
            d_q = torch.full((2 * p.shape[0], 2 * p.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
            assert lib.w2xc_resize2x_cubic_device(d_p.data_ptr(), p.shape[1], p.shape[0], d_q.data_ptr(), st.cuda_stream) == 0
            st.synchronize()
            uv.append(d_q.cpu().numpy())
        u, v = uv
    if shrink:
        H, W = R.final_size(h, w, it, shrink)
        y, u, v = (orc.resize_linear(p, W, H) for p in (y, u, v))
    H, W = y.shape
    d_p = torch.from_numpy(np.stack([y, u, v])).cuda()
    d_out = torch.full((H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.w2xc_yuv_to_u8_device(d_p[0].data_ptr(), d_p[1].data_ptr(), d_p[2].data_ptr(), W, H, d_out.data_ptr(), W * 3, st.cuda_stream) == 0
    st.synchronize()
    return d_out.cpu().numpy()


def run_y(gpu, ymodels, case, tta=True, **opt):
    _, noise, scale, img, it, shrink = case
    return gpu.process_image_u8(R.image(img), ymodels[noise] if noise else None, ymodels[scale] if scale else None, it,
                                gpu.make_opts(**opt) if opt else None, shrink, tta=tta)


def tta_zero(gpu, name, img, noise, scale, it, shrink):
    """the *_tta entry point with tta = 0"""
    return gpu._image_host(getattr(gpu.lib(), name), name, img, 3, noise, scale, it, None, shrink, tail=(0,))


@pytest.mark.parametrize("case", Y_CASES, ids=[c[0] for c in Y_CASES])
def test_y_image_equals_building_blocks(gpu, ymodels, case):
    _, noise, scale, img, it, shrink = case
    got = run_y(gpu, ymodels, case)
    assert np.array_equal(got, composed_y(gpu, ymodels, case))
    plain = run_y(gpu, ymodels, case, tta=False)
    assert not np.array_equal(got, plain), "TTA changes the result"
    assert np.array_equal(tta_zero(gpu, "w2xc_process_image_u8_tta", R.image(img), ymodels[noise] if noise else None,
                                   ymodels[scale] if scale else None, it, shrink), plain), "tta = 0 is the call without TTA"


def composed_rgb(gpu, rgbmodels, case, **opt):
    """w2xc_u8_to_rgb_device -> convert_planes_tta_device per pass -> (the oracle's resize_linear) -> w2xc_rgb_to_u8_device"""
    _, noise, scale, img, it, shrink = case
    src = R.image(img)
    h, w, _ = src.shape
    st = stream()
    d_img = torch.from_numpy(src).cuda()
    d_pl = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    gpu.u8_to_rgb_device(d_img.data_ptr(), w * 3, w, h, d_pl.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    x = d_pl.cpu().numpy()
    o = gpu.make_opts(device=0, **opt)
    if noise:
        x = planes_tta(gpu, rgbmodels[noise], x, 0, o)
    for _ in range(it):
        x = planes_tta(gpu, rgbmodels[scale], x, 1, o)
    if shrink:
        H, W = R.final_size(h, w, it, shrink)
        x = np.stack([orc.resize_linear(p, W, H) for p in x])
    _, H, W = x.shape
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.rgb_to_u8_device(d_x.data_ptr(), W, H, d_out.data_ptr(), W * 3, stream=st.cuda_stream)
    st.synchronize()
    return d_out.cpu().numpy()


def run_rgb(gpu, rgbmodels, case, tta=True, **opt):
    _, noise, scale, img, it, shrink = case
    return gpu.process_image_rgb_u8(R.image(img), rgbmodels[noise] if noise else None, rgbmodels[scale] if scale else None, it,
                                    gpu.make_opts(**opt) if opt else None, shrink, tta=tta)


@pytest.mark.parametrize("case", RGB_CASES, ids=[c[0] for c in RGB_CASES])
def test_rgb_image_equals_building_blocks(gpu, rgbmodels, case):
    _, noise, scale, img, it, shrink = case
    got = run_rgb(gpu, rgbmodels, case)
    assert np.array_equal(got, composed_rgb(gpu, rgbmodels, case))
    assert np.array_equal(got, run_rgb(gpu, rgbmodels, case, fusion=gpu.FUSION_OFF)), "no uint8-fused layer under TTA either way"
    plain = run_rgb(gpu, rgbmodels, case, tta=False)
    assert not np.array_equal(got, plain), "TTA changes the result"
    assert np.array_equal(tta_zero(gpu, "w2xc_process_image_rgb_u8_tta", R.image(img), rgbmodels[noise] if noise else None,
                                   rgbmodels[scale] if scale else None, it, shrink), plain), "tta = 0 is the call without TTA"


# ---- 4. against the oracle ----
ORACLE_Y = [("scale", None, "scale", "a", 1, 0.0), ("noise", "noise", None, "a", 0, 0.0), ("noise_scale", "noise", "scale", "a", 1, 0.0),
            ("ratio1.5", None, "scale", "a", 1, 0.75)]
ORACLE_RGB = [("scale", None, "m4", "a", 1, 0.0), ("noise", "m7", None, "a", 0, 0.0), ("ratio1.5", None, "m4", "a", 1, 0.75)]


@functools.lru_cache(maxsize=None)
def y_oracle(role):
    return orc.Oracle(gen_model.synth_layers(seed=gen_model.SEEDS["noise1" if role == "noise" else "scale2.0x"]))


@functools.lru_cache(maxsize=None)
def expected_y(case):
    _, noise, scale, img, it, shrink = case
    src = R.image(img)
    y, u, v = orc.u8_to_yuv(src)
    if noise:
        y = tta_mean([Tinv(k, y_oracle(noise).convert(T(k, y))) for k in range(8)])
    for _ in range(it):
        y = tta_mean([Tinv(k, y_oracle(scale).convert(orc.resize2x_nearest(T(k, y)))) for k in range(8)])
        u, v = orc.resize2x_cubic(u), orc.resize2x_cubic(v)
    if shrink:
        H, W = R.final_size(src.shape[0], src.shape[1], it, shrink)
        y, u, v = (orc.resize_linear(p, W, H) for p in (y, u, v))
    want = orc.yuv_to_u8(y, u, v)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def expected_rgb(case):
    _, noise, scale, img, it, shrink = case
    src = R.image(img)
    x = R.to_planes(src)
    if noise:
        x = tta_mean([Tinv(k, R.oracle_cnn(noise, T(k, x))) for k in range(8)])
    for _ in range(it):
        x = tta_mean([Tinv(k, R.oracle_cnn(scale, np.stack([orc.resize2x_nearest(p) for p in T(k, x)]))) for k in range(8)])
    if shrink:
        H, W = R.final_size(src.shape[0], src.shape[1], it, shrink)
        x = np.stack([orc.resize_linear(p, W, H) for p in x])
    want = R.to_u8(x)
    want.setflags(write=False)
    return want


def inside_share(want):
    return float(((want >= 1) & (want <= 254)).mean())


@pytest.mark.parametrize("case", ORACLE_Y, ids=[c[0] for c in ORACLE_Y])
def test_y_image_against_oracle(gpu, ymodels, case):
    want = expected_y(case)
    print("share of the expected bytes in 1..254: %.3f" % inside_share(want))
    assert inside_share(want) >= 0.30, "the clip must not hide the values"
    assert np.array_equal(run_y(gpu, ymodels, case, kernel=gpu.KERNEL_DIRECT), want), "the reference-ordered kernels give the oracle's bytes"
    R.gate(run_y(gpu, ymodels, case), want, "Y " + case[0])


@pytest.mark.parametrize("case", ORACLE_RGB, ids=[c[0] for c in ORACLE_RGB])
def test_rgb_image_against_oracle(gpu, rgbmodels, case):
    want = expected_rgb(case)
    print("share of the expected bytes in 1..254: %.3f" % inside_share(want))
    assert inside_share(want) >= 0.30, "the clip must not hide the values"
    assert np.array_equal(run_rgb(gpu, rgbmodels, case, kernel=gpu.KERNEL_DIRECT), want), "the reference-ordered kernels give the oracle's bytes"
    R.gate(run_rgb(gpu, rgbmodels, case), want, "RGB " + case[0])


# ---- 5. batches ----
def device_batch(gpu, rgb, x, noise, scale, it, o):
    n, h, w, _ = x.shape
    H, W = h << it, w << it
    irs, ors = w * 3 + 5, W * 3 + 7
    src = torch.full((n, h + 1, irs), 0x5A, dtype=torch.uint8)
    src[:, 1:, :w * 3] = torch.from_numpy(x.reshape(n, h, w * 3))
    d_in = src.cuda()
    d_out = torch.full((n, H + 2, ors), 0xAB, dtype=torch.uint8, device="cuda")
    f = gpu.process_image_rgb_u8_batch_device if rgb else gpu.process_image_u8_batch_device
    f(n, d_in.data_ptr() + irs, (h + 1) * irs, irs, w, h, d_out.data_ptr() + 2 * ors, (H + 2) * ors, ors, noise, scale, it, 0.0,
      stream=stream().cuda_stream, opts=o, tta=True)
    stream().synchronize()
    b = d_out.cpu().numpy()
    guard = np.ones(b.shape, bool)
    guard[:, 2:, :W * 3] = False
    assert (b[guard] == 0xAB).all(), "bytes outside the output images were written"
    return b[:, 2:, :W * 3].reshape(n, H, W, 3).copy()


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_batches_equal_single_tta_calls(gpu, ymodels, rgbmodels, route, n):
    rgb = route == "rgb"
    h, w = 40, 52
    x = R.batch_images(n, h, w, 900 + n)
    noise, scale = (None, rgbmodels["m4"]) if rgb else (ymodels["noise"], ymodels["scale"])
    one = gpu.process_image_rgb_u8 if rgb else gpu.process_image_u8
    many = gpu.process_image_rgb_u8_batch if rgb else gpu.process_image_u8_batch
    # workspace_mb = 1: the planes of one 52 x 40 image under TTA are 0.5 MB on the Y route (two images per sub-batch) and 1.3 MB on the RGB route (one)
    for opt in ({}, dict(workspace_mb=1)):
        o = gpu.make_opts(device=0, **opt)
        want = np.stack([one(x[i], noise, scale, 1, o, tta=True) for i in range(n)])
        assert len({want[i].tobytes() for i in range(n)}) == n
        assert np.array_equal(device_batch(gpu, rgb, x, noise, scale, 1, o), want), ("device form", opt)
        assert np.array_equal(many([x[i].copy() for i in range(n)], noise, scale, 1, o, tta=True), want), ("host form", opt)
    assert not np.array_equal(want[0], one(x[0], noise, scale, 1, o))


@pytest.mark.parametrize("route", ["y", "rgb"])
def test_aux_follows_the_sub_batch_not_n(gpu, noise1_layers, scale_layers, route):
    rgb = route == "rgb"
    h, w = 40, 52
    used = {}
    for n in (2, 6):
        scale = gpu._ModelSet.from_layers(R.layers("m4") if rgb else scale_layers)   # fresh: its scratch has only this call's sizes
        x = R.batch_images(n, h, w, 5)
        device_batch(gpu, rgb, x, None, scale, 1, gpu.make_opts(device=0, workspace_mb=1))
        used[n] = scale.fill_scratch(0)
    print("scratch bytes by n: %r" % used)
    assert used[2] == used[6], "sub-batches of at most two images: the pipeline's memory does not grow with n"


# ---- 6. launch counts ----
def launches(ms):
    return ms.profile_read(0)[1]


@pytest.mark.parametrize("hw", [(64, 64), (48, 64)], ids=["64x64", "64x48"])
def test_launch_counts(gpu, scale_layers, hw):
    h, w = hw
    ms = gpu._ModelSet.from_layers(scale_layers)
    o = gpu.make_opts(device=0, profile=1)
    square = h == w

    def plain_batch(k, hh, ww):
        x = np.random.default_rng(1).random((k, hh, ww), dtype=np.float32)
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.empty((k, 2 * hh, 2 * ww), dtype=torch.float32, device="cuda")
        ms.profile_reset(0)
        ms.convert_batch_device(k, d_in.data_ptr(), hh * ww * 4, ww * 4, ww, hh, d_out.data_ptr(), 4 * hh * ww * 4, 2 * ww * 4, nn2x=True,
                                stream=stream().cuda_stream, opts=o)
        stream().synchronize()
        return launches(ms)
    want = plain_batch(8, h, w) if square else [a + b for a, b in zip(plain_batch(4, h, w), plain_batch(4, w, h))]
    assert sum(want) > 0
    img = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ms.profile_reset(0)
    gpu.process_image_u8(img, None, ms, 1, o, tta=True)
    got = launches(ms)
    ms.profile_reset(0)
    gpu.process_image_u8(img, None, ms, 1, o)
    once = launches(ms)
    print("launches per layer: TTA %r, batch %r, one plane %r" % (got, want, once))
    assert got == want


# ---- 7. poisoned scratch, strided ROIs in and out ----
def device_roi(gpu, rgb, src, noise, scale, it):
    h, w, _ = src.shape
    H, W = h << it, w << it
    irs, ors = 7 + w * 3 + 4, 5 + W * 3 + 6
    host = np.full((2 + h + 1, irs), 0x5A, np.uint8)
    host[2:2 + h, 7:7 + w * 3] = src.reshape(h, w * 3)
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((3 + H + 1, ors), 0xAB, dtype=torch.uint8, device="cuda")
    f = gpu.process_image_rgb_u8_device if rgb else gpu.process_image_u8_device
    f(d_in.data_ptr() + 2 * irs + 7, irs, w, h, d_out.data_ptr() + 3 * ors + 5, ors, noise, scale, it, 0.0, stream=stream().cuda_stream,
      opts=gpu.make_opts(device=0), tta=True)
    stream().synchronize()
    b = d_out.cpu().numpy()
    guard = np.ones(b.shape, bool)
    guard[3:3 + H, 5:5 + W * 3] = False
    assert (b[guard] == 0xAB).all(), "bytes outside the output ROI were written"
    return b[3:3 + H, 5:5 + W * 3].reshape(H, W, 3).copy()


@pytest.mark.parametrize("route", ["y", "rgb"])
def test_poisoned_scratch(gpu, ymodels, rgbmodels, route):
    rgb = route == "rgb"
    noise, scale = (rgbmodels["m7"], rgbmodels["m4"]) if rgb else (ymodels["noise"], ymodels["scale"])
    src = R.image("b")
    first = device_roi(gpu, rgb, src, noise, scale, 1)
    one = gpu.process_image_rgb_u8 if rgb else gpu.process_image_u8
    assert np.array_equal(first, one(src, noise, scale, 1, tta=True))
    for word in WORDS:
        for ms in (noise, scale):
            assert ms.fill_scratch(word) > 0
        assert np.array_equal(device_roi(gpu, rgb, src, noise, scale, 1), first), hex(word)


# ---- 8. the CLI ----
def test_cli_tta(gpu, tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    gen_model.write_json(R.layers("m4"), str(tmp_path / "scale2.0x_model.json"))
    src = np.random.default_rng(9).integers(0, 256, (20, 30, 3)).astype(np.uint8)
    Image.fromarray(src).save(str(tmp_path / "in.png"))
    assert cli.main(["-i", str(tmp_path / "in.png"), "-o", str(tmp_path / "out.png"), "-m", "scale", "--model_dir", str(tmp_path), "--tta", "1"]) == 0
    got = np.asarray(Image.open(str(tmp_path / "out.png")).convert("RGB"))
    ms = gpu._ModelSet.from_layers(R.layers("m4"))
    assert np.array_equal(got, gpu.process_image_rgb_u8(src, None, ms, 1, tta=True))
