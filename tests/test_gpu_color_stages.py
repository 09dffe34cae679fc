"""GPU tests of the stages around the CNN (w2xc_color.hip: the stage structs on k_px, k_bleed_tiled) through their public building blocks --
w2xc_u8_to_yuv_device, w2xc_yuv_to_u8_device, w2xc_u8_to_rgb_device, w2xc_rgb_to_u8_device, w2xc_resize2x_cubic_device, w2xc_resize_linear_device and
w2xc_bleed_rgba_u8_device -- where their float and loop logic can go wrong: sizes around a 256-thread block, odd row strides and base addresses with
guard bytes, to_u8 at its rounding ties and beyond int32, both border branches of the linear resize, inputs of mixed magnitude (a fused multiply-add
rounds differently on them), and the second trip of every grid-stride loop (more than 2^24 elements, more than 2^20 bleed tiles).

Every comparison is bit for bit against oracle.oracle (numpy's clip(rint(255 x)) / u8 * (1 / 255) for the RGB pair, as tests/test_gpu_rgb.py has them)
unless the test says otherwise.  Outputs are allocated pre-filled (NaN, 0xAB) and everything the call must not write is checked to have kept the fill."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from test_oracle_color import _keys_matrix
from test_rgba_api import bleed_ref

torch = pytest.importorskip("torch")
on_gpu = pytest.mark.gpu       # (the two tests of the expectations themselves need no device and run without one)

F32 = np.float32
TAIL = 8                                                                       # floats behind every float output: they stay NaN
SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (257, 1), (3, 85), (37, 53)]   # (h, w): 255 / 256 / 257 elements = the edge of a 256-thread block
IDS = ["%dx%d" % s for s in SHAPES]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def stream():
    return torch.cuda.current_stream()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def mixed(rng, shape):
    """magnitudes from 1e-3 to 1e3 side by side, as tests/test_gpu_tta.py::test_gather_bit_for_bit has them: a contracted a * b + c shows in the last bit"""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


# ---- the calls: inputs as the case wants them, outputs pre-filled, everything around the output checked ----
def u8_to_planes(gpu, route, img, pad=True):
    """w2xc_u8_to_yuv_device / w2xc_u8_to_rgb_device on the h x w x 3 image; pad: rows 3 w + 5 bytes apart from a base 1 byte into the allocation"""
    h, w, _ = img.shape
    rs, off = (3 * w + 5, 1) if pad else (3 * w, 0)
    host = np.full(off + h * rs, 0x5A, np.uint8)
    host[off:].reshape(h, rs)[:, :3 * w] = img.reshape(h, 3 * w)
    d_in = torch.from_numpy(host).cuda()
    d_pl = torch.full((3 * h * w + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    f = gpu.lib().w2xc_u8_to_yuv_device if route == "yuv" else gpu.lib().w2xc_u8_to_rgb_device
    p = d_pl.data_ptr()
    assert f(d_in.data_ptr() + off, rs, w, h, p, p + 4 * h * w, p + 8 * h * w, stream().cuda_stream) == 0, gpu.last_error()
    stream().synchronize()
    got = d_pl.cpu().numpy()
    assert np.isnan(got[3 * h * w:]).all(), "floats behind the planes were written"
    return got[:3 * h * w].reshape(3, h, w)


def planes_to_u8(gpu, route, x, pad=True):
    """w2xc_yuv_to_u8_device / w2xc_rgb_to_u8_device on the planes x (3, h, w); pad: rows 3 w + 7 bytes apart and one more row, all 0xAB afterwards"""
    _, h, w = x.shape
    ors, extra = (3 * w + 7, 1) if pad else (3 * w, 0)
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((h + extra, ors), 0xAB, dtype=torch.uint8, device="cuda")
    f = gpu.lib().w2xc_yuv_to_u8_device if route == "yuv" else gpu.lib().w2xc_rgb_to_u8_device
    p = d_x.data_ptr()
    assert f(p, p + 4 * h * w, p + 8 * h * w, w, h, d_out.data_ptr(), ors, stream().cuda_stream) == 0, gpu.last_error()
    stream().synchronize()
    b = d_out.cpu().numpy()
    assert (b[:h, 3 * w:] == 0xAB).all() and (b[h:] == 0xAB).all(), "bytes outside the output rows were written"
    return b[:h, :3 * w].reshape(h, w, 3)


def resize(gpu, x, dhw=None):
    """w2xc_resize_linear_device to dhw = (dh, dw), or w2xc_resize2x_cubic_device without one"""
    sh, sw = x.shape
    dh, dw = dhw if dhw else (2 * sh, 2 * sw)
    d_src = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_dst = torch.full((dh * dw + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    if dhw:
        gpu.resize_linear_device(d_src.data_ptr(), sw, sh, d_dst.data_ptr(), dw, dh, stream=stream().cuda_stream)
    else:
        assert gpu.lib().w2xc_resize2x_cubic_device(d_src.data_ptr(), sw, sh, d_dst.data_ptr(), stream().cuda_stream) == 0, gpu.last_error()
    stream().synchronize()
    got = d_dst.cpu().numpy()
    assert np.isnan(got[dh * dw:]).all(), "floats behind the plane were written"
    return got[:dh * dw].reshape(dh, dw)


# ---- the expectations ----
def want_planes(route, img):
    if route == "yuv":
        return np.stack(orc.u8_to_yuv(img))
    return np.ascontiguousarray((img.astype(np.float32) * F32(1 / 255)).transpose(2, 0, 1))


def rint_u8(x):
    """saturate(rint(255 x)), numpy's rint: half to even"""
    return np.clip(np.rint(np.asarray(x, np.float32) * F32(255)), 0, 255).astype(np.uint8)


def want_u8(route, x):
    if route == "yuv":
        return orc.yuv_to_u8(x[0], x[1], x[2])
    return np.ascontiguousarray(rint_u8(x).transpose(1, 2, 0))


# ---- B1. shapes and strides ----
@on_gpu
@pytest.mark.parametrize("route", ["yuv", "rgb"])
@pytest.mark.parametrize("hw", SHAPES, ids=IDS)
def test_u8_to_planes_shapes_and_strides(gpu, route, hw):
    h, w = hw
    img = np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert same_bits(u8_to_planes(gpu, route, img), want_planes(route, img))


@on_gpu
@pytest.mark.parametrize("route", ["yuv", "rgb"])
@pytest.mark.parametrize("hw", SHAPES, ids=IDS)
def test_planes_to_u8_shapes_and_strides(gpu, route, hw):
    h, w = hw
    x = np.random.default_rng(2000 * h + w).random((3, h, w), dtype=np.float32) * F32(1.4) - F32(0.2)      # both saturation ends
    got, want = planes_to_u8(gpu, route, x), want_u8(route, x)
    assert np.array_equal(got, want)
    if h * w >= 255:
        assert want.min() == 0 and want.max() == 255 and ((want > 0) & (want < 255)).mean() > 0.3, "the clip must not hide the values"


@on_gpu
@pytest.mark.parametrize("hw", SHAPES, ids=IDS)
def test_resize_linear_shapes(gpu, hw):
    """the shapes as DESTINATIONS of the pipelines' 0.75 (the source is 4/3 as large, rounded up): 255 / 256 / 257 output elements"""
    dh, dw = hw
    x = mixed(np.random.default_rng(3000 * dh + dw), ((4 * dh + 2) // 3, (4 * dw + 2) // 3))
    assert same_bits(resize(gpu, x, (dh, dw)), orc.resize_linear(x, dw, dh))


# ---- B2. to_u8: the ties of rint, saturation, products past int32 ----
SATURATION = [-1e10, -0.3, -1e-9, -0.0, 0.0, 1.0, 1.0 + 1e-3, 7.5, 1e10]     # (+-1e10: 255 x is past int32; NaN and +-Inf have no answer in the oracle)


@functools.lru_cache(maxsize=None)
def tie_list():
    """(values, where the exact ties lie in them, their k): c_k = float32((k + 0.5) / 255) with c_k * 255 == k + 0.5 exactly in float32, both
    float32 neighbours of each, and the saturation values"""
    ks = np.arange(255)
    c = ((ks + 0.5) / 255.0).astype(np.float32)
    exact = c * F32(255) == (ks + 0.5).astype(np.float32)
    assert exact.sum() >= 200 and (ks[exact] % 2 == 1).sum() >= 100, (int(exact.sum()), int((ks[exact] % 2 == 1).sum()))
    ties, k = c[exact], ks[exact]
    vals = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf)), np.array(SATURATION, np.float32)])
    vals.setflags(write=False)
    return vals, np.arange(ties.size), k


def check_ties(got, where, k):
    """every exact tie with odd k rounds up to k + 1, with even k stays k"""
    g = got[where].astype(np.int64)
    odd = k % 2 == 1
    assert np.array_equal(g[odd], k[odd] + 1), "ties with odd k"
    assert np.array_equal(g[~odd], k[~odd]), "ties with even k"


def test_tie_list_on_the_cpu_side():
    """(needs no device) the expectation itself: numpy rounds the list half to even, one ulp beside a tie decides"""
    vals, where, k = tie_list()
    want = rint_u8(vals)
    check_ties(want, where, k)
    n = where.size
    up, down = want[n:2 * n].astype(np.int64), want[2 * n:3 * n].astype(np.int64)             # one ulp above a tie, one below: k + 1 and k, unless the
    assert ((up == k + 1) | (up == want[:n])).all() and ((down == k) | (down == want[:n])).all()   # product rounds back onto the tie (small k)
    assert (up == k + 1).mean() > 0.9 and (down == k).mean() > 0.9
    assert want[3 * n:].tolist() == [0, 0, 0, 0, 0, 255, 255, 255, 255]


@on_gpu
@pytest.mark.parametrize("c", [0, 1, 2])
def test_rgb_to_u8_ties_and_saturation(gpu, c):
    vals, where, k = tie_list()
    rng = np.random.default_rng(70 + c)
    x = np.empty((3, 1, vals.size), np.float32)
    for p in range(3):
        x[p, 0] = vals if p == c else rng.permutation(vals)
    assert not np.array_equal(bits(x[(c + 1) % 3]), bits(x[(c + 2) % 3]))
    got = planes_to_u8(gpu, "rgb", x)
    assert np.array_equal(got, want_u8("rgb", x))
    check_ties(got[0, :, c], where, k)


@on_gpu
def test_yuv_to_u8_ties_and_saturation(gpu):
    """U = V = 0.5: the three channels equal Y exactly (tests/test_oracle_color.py::test_round_saturate)"""
    vals, where, k = tie_list()
    x = np.full((3, 1, vals.size), 0.5, np.float32)
    x[0, 0] = vals
    got = planes_to_u8(gpu, "yuv", x)
    assert np.array_equal(got, np.repeat(rint_u8(vals)[None, :, None], 3, axis=2))
    assert np.array_equal(got, orc.yuv_to_u8(x[0], x[1], x[2]))
    for ch in range(3):
        check_ties(got[0, :, ch], where, k)


# ---- B3. ResizeLinear alone ----
# (sh, sw, dh, dw): the exact 4/3 three-phase case, the pipelines' 0.75 on an odd width, a scale just above 1, above 3, exactly 2, thin and tiny planes --
# and three enlargements, the only way into the two clamp branches sx < 0 and sx >= sw - 1
LINEAR = [(40, 60, 30, 45), (74, 106, 55, 79), (52, 74, 51, 73), (20, 30, 11, 16), (64, 64, 19, 21), (36, 52, 18, 26), (9, 33, 5, 17), (3, 300, 2, 257),
          (1, 9, 1, 5), (7, 1, 4, 1), (2, 2, 1, 1), (1, 1, 1, 1), (1, 1, 3, 4), (17, 23, 34, 46), (5, 7, 13, 8),
          # three more enlargements.  Above, every fraction fx in the upper clamp's columns is dyadic (0.25, 0.125, 0.0625), and S * (1 - fx) + S * fx on
          # the one remaining tap then rounds back to S exactly: the branch `sx >= sw - 1` could be dropped unseen.  Here it is not (scales 5 / 13, 3 / 16, 11 / 31)
          (7, 5, 8, 13), (24, 3, 29, 16), (13, 11, 20, 31)]
LINEAR_IDS = ["%dx%d-%dx%d" % c for c in LINEAR]


def linear_axis(dn, sn):
    """one axis of cv::resize(INTER_LINEAR) from its definition: the source coordinate (d + 0.5) * (sn / dn) - 0.5 in double, rounded to float32 as
    OpenCV does; its floor and fraction; below 0 and from sn - 1 on the tap is clamped into the plane with fraction 0; the second tap is the next one"""
    f = ((np.arange(dn) + 0.5) * (float(sn) / dn) - 0.5).astype(np.float32).astype(np.float64)
    s0 = np.floor(f)
    t = f - s0
    lo, hi = s0 < 0, s0 >= sn - 1
    t[lo | hi] = 0.0
    s0[lo] = 0
    s0[hi] = sn - 1
    s0 = s0.astype(np.int64)
    return s0, np.minimum(s0 + 1, sn - 1), t


def linear_ref64(x, dhw):
    """the two taps per axis, horizontal then vertical, in float64"""
    x = x.astype(np.float64)
    dh, dw = dhw
    x0, x1, tx = linear_axis(dw, x.shape[1])
    y0, y1, ty = linear_axis(dh, x.shape[0])
    rows = x[:, x0] * (1 - tx) + x[:, x1] * tx
    return rows[y0] * (1 - ty)[:, None] + rows[y1] * ty[:, None]


def test_linear_axis_reaches_both_clamps():
    """(needs no device) the enlargements reach both border branches on both axes, the shrinks neither"""
    for (sh, sw, dh, dw) in LINEAR:
        for dn, sn in ((dw, sw), (dh, sh)):
            f = ((np.arange(dn) + 0.5) * (float(sn) / dn) - 0.5).astype(np.float32)
            if dn > sn:
                assert (np.floor(f) < 0).any() and (np.floor(f) >= sn - 1).any(), (sh, sw, dh, dw)
            elif sn > 1 and dn < sn:
                assert not (np.floor(f) < 0).any(), (sh, sw, dh, dw)


@on_gpu
@pytest.mark.parametrize("case", LINEAR, ids=LINEAR_IDS)
def test_resize_linear_alone(gpu, case):
    sh, sw, dh, dw = case
    rng = np.random.default_rng(sh + 7 * sw + 13 * dh + 29 * dw)
    x = rng.random((sh, sw), dtype=np.float32)
    got = resize(gpu, x, (dh, dw))
    assert same_bits(got, orc.resize_linear(x, dw, dh)), "[0, 1) input"
    # a second reference that shares no code with the oracle.  1 - fx, three roundings per row sum, 1 - fy and three for the column sum: each at most
    # 2^-24 of a value no larger than max |x|, and the row errors combine convexly
    err = float(np.abs(got.astype(np.float64) - linear_ref64(x, (dh, dw))).max())
    print("%s: max error against the float64 definition %.3g (bound %.3g)" % (case, err, 8 * 2.0 ** -24 * float(x.max())))
    assert err <= 8 * 2.0 ** -24 * float(np.abs(x).max())
    m = mixed(rng, (sh, sw))
    assert same_bits(resize(gpu, m, (dh, dw)), orc.resize_linear(m, dw, dh)), "mixed magnitudes"
    const = np.full((sh, sw), 0.37, np.float32)
    assert np.abs(resize(gpu, const, (dh, dw)) - 0.37).max() <= 1e-6


# ---- B4. Resize2xCubic alone ----
CUBIC = SHAPES + [(2, 2), (1, 2), (12, 9)]


@on_gpu
@pytest.mark.parametrize("hw", CUBIC, ids=["%dx%d" % s for s in CUBIC])
def test_resize2x_cubic_alone(gpu, hw):
    h, w = hw
    rng = np.random.default_rng(5000 * h + w)
    m = mixed(rng, (h, w))
    assert same_bits(resize(gpu, m), orc.resize2x_cubic(m)), "mixed magnitudes"
    x = rng.random((h, w), dtype=np.float32)
    want = _keys_matrix(h) @ x.astype(np.float64) @ _keys_matrix(w).T     # the dense float64 form of Keys' cubic, tests/test_oracle_color.py
    err = float(np.abs(resize(gpu, x) - want).max())
    print("%dx%d: max error against the float64 Keys matrix %.3g" % (h, w, err))
    assert err < 2e-6


# ---- B6. second trips of the grid-stride loops ----
# k_px runs at most 65536 x 256 = 2^24 threads along x: with more elements a thread takes a second one
BIG_H, BIG_W = 4096, 4097          # 16 781 312 pixels


@functools.lru_cache(maxsize=None)
def big_image():
    img = np.frombuffer(np.random.default_rng(11).bytes(BIG_H * BIG_W * 3), np.uint8).reshape(BIG_H, BIG_W, 3)
    assert img.shape[0] * img.shape[1] > 1 << 24
    return img


@on_gpu
@pytest.mark.parametrize("route", ["yuv", "rgb"])
def test_second_trip_colour_round_trip(gpu, route):
    img = big_image()
    x = u8_to_planes(gpu, route, img, pad=False)
    assert same_bits(x, want_planes(route, img))
    back = planes_to_u8(gpu, route, x, pad=False)
    assert np.array_equal(back, want_u8(route, x))
    assert np.array_equal(back, img), "u8 -> planes -> u8 is the identity on every byte"


@functools.lru_cache(maxsize=None)
def big_cubic():
    """a 2048 x 2049 plane and the oracle's 4096 x 4098 = 16 785 408 outputs"""
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((2048, 2049), dtype=np.float32) * F32(10.0) ** rng.integers(-3, 4, (2048, 2049)).astype(np.float32)).astype(np.float32)
    want = orc.resize2x_cubic(x)
    assert want.size > 1 << 24
    return x, want


@on_gpu
def test_second_trip_resize2x_cubic(gpu):
    x, want = big_cubic()
    assert same_bits(resize(gpu, x), want)


@on_gpu
def test_second_trip_resize_linear(gpu):
    """4096 x 4098 -> 4095 x 4099 = 16 785 405 outputs: one axis shrinks slightly, one enlarges, so the phase drifts across the whole plane"""
    _, x = big_cubic()
    assert 4095 * 4099 > 1 << 24
    assert same_bits(resize(gpu, x, (4095, 4099)), orc.resize_linear(x, 4099, 4095))


# The bleed: one row of 32 * 2^20 + 1 pixels = 2^25 + 1 pixels (RgbaBleedFirst / RgbaBleedPass take further k_px trips) = 2^20 + 1 tiles of 32 (k_bleed_tiled
# takes a second tile trip on LDS words the first one left).  Opaque random colour but for four transparent runs: at the left edge, across pixel 2^24 (the
# first k_px trip's end), across a tile border, and up to the right edge through the one-pixel last tile (the second tile trip).
BLEED_W = 32 * (1 << 20) + 1
BLEED_RUNS = [(0, 40), ((1 << 24) - 20, (1 << 24) + 20), (32 * 600000 - 22, 32 * 600000 + 23), ((1 << 25) - 30, (1 << 25) + 1)]


@functools.lru_cache(maxsize=None)
def bleed_image():
    img = np.frombuffer(np.random.default_rng(13).bytes(BLEED_W * 4), np.uint8).reshape(1, BLEED_W, 4).copy()
    img[0, :, 3] = 255
    for a, b in BLEED_RUNS:
        img[0, a:b, 3] = 0
    return img


@on_gpu
@pytest.mark.parametrize("passes", [1, 2, 16, 17])      # RgbaBleedFirst alone; k_bleed_tiled at its fewest and most passes; the chain of k_px launches
def test_second_trip_bleed(gpu, passes):
    img = bleed_image()
    assert [b - a for a, b in BLEED_RUNS] == [40, 40, 45, 31] and BLEED_RUNS[-1][1] == BLEED_W
    want = np.ascontiguousarray(img[:, :, :3])             # the source colour everywhere outside the runs
    for a, b in BLEED_RUNS:
        # a pass moves colour one pixel: inside a run the bleed of the slice that reaches passes + 2 pixels beyond it is the bleed of the row
        lo, hi = max(a - passes - 2, 0), min(b + passes + 2, BLEED_W)
        want[:, a:b] = bleed_ref(img[:, lo:hi], passes)[:, a - lo:b - lo, :3]
    ors = 3 * BLEED_W + 7
    d_in = torch.from_numpy(img.reshape(1, 4 * BLEED_W)).cuda()
    d_out = torch.full((2, ors), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.bleed_rgba_u8_device(d_in.data_ptr(), 4 * BLEED_W, BLEED_W, 1, passes, d_out.data_ptr(), ors, stream=stream().cuda_stream)
    stream().synchronize()
    if passes > 16:
        gpu.bleed_rgba_u8_trim()                           # (the chain's stamp plane: 2 bytes per pixel)
    b = d_out.cpu().numpy()
    assert (b[0, 3 * BLEED_W:] == 0xAB).all() and (b[1] == 0xAB).all(), "bytes outside the output row were written"
    got = b[0, :3 * BLEED_W].reshape(1, BLEED_W, 3)
    assert np.array_equal(got, want)
    a, e = BLEED_RUNS[1]                                   # the runs are longer than 2 x 17: colour has come in from both sides, the middle is unreached
    assert np.array_equal(got[0, a], img[0, a - 1, :3]) and np.array_equal(got[0, e - 1], img[0, e, :3])
    assert np.array_equal(got[0, (a + e) // 2], img[0, (a + e) // 2, :3])
