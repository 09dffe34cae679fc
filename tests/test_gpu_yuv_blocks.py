"""GPU tests of the building blocks of the YUV frame calls (csrc/w2xc_yuv.hip through w2xc_y8_to_plane_device, w2xc_plane_to_y8_device and
w2xc_chroma2x_u8_device).  Every comparison is equality of bytes or of float bits:
  * the luma stages against the torch expressions of include/w2xc_hip.h ("YUV frames"), and against their NumPy restatement (tests/yuv_ref.py);
  * the chroma kernel against the composed route torch u8 * (1 / 255) -> w2xc_resize2x_cubic_device -> clamp(round(255 v)) -> crop.
Every buffer has a sentinel rim -- in front, behind, between rows, between frames, and with 2-byte samples between the samples -- that must be intact."""
import functools

import numpy as np
import pytest

import yuv_ref as yr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
RIM_F = 8          # floats in front of and behind every float output: they stay NaN


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def stream():
    return torch.cuda.current_stream()


# ---- byte planes in a buffer with rims: n planes of rows x cols samples, px bytes apart ----
class Lay:
    def __init__(self, n, rows, cols, px=1, aligned=False):
        self.n, self.rows, self.cols, self.px = n, rows, cols, px
        self.row_bytes = px * (cols - 1) + 1
        if aligned:      # everything a multiple of 4: the dword path
            self.off, self.row = 16, (self.row_bytes + 3) // 4 * 4 + 4
            self.frame = self.rows * self.row + 8
        else:            # an odd base, odd rows, odd frames: the byte path
            self.off, self.row = 13, self.row_bytes + 3 - (self.row_bytes & 1)
            self.frame = self.rows * self.row + 5 - (self.rows * self.row & 1)
            assert self.row & 1 and self.frame & 1
        self.total = self.off + n * self.frame + 16

    def index(self):
        """the byte offset of every sample: (n, rows, cols)"""
        f, r, c = np.meshgrid(np.arange(self.n), np.arange(self.rows), np.arange(self.cols), indexing="ij")
        return self.off + f * self.frame + r * self.row + c * self.px

    def scatter(self, planes, fill):
        """the buffer: `fill` (a byte, or 'random': the bytes between 2-byte samples are another plane's) with the planes' samples in place"""
        if isinstance(fill, str):
            buf = np.random.default_rng(99).integers(0, 256, self.total, dtype=np.uint8)
        else:
            buf = np.full(self.total, fill, np.uint8)
        buf[self.index()] = planes
        return buf

    def gather(self, buf, fill):
        """the planes, after checking that every byte that is no sample kept `fill`"""
        idx = self.index()
        rest = np.ones(self.total, bool)
        rest[idx] = False
        assert (buf[rest] == fill).all(), "bytes outside the samples were written: %d of them" % int((buf[rest] != fill).sum())
        return buf[idx]


# ---- the luma stages ----
def y8_to_plane(gpu, planes, rng, aligned=False):
    n, h, w = planes.shape
    lay = Lay(n, h, w, 1, aligned)
    d_src = torch.from_numpy(lay.scatter(planes, 0x5A)).cuda()
    ps = (w * h + 3) if n > 1 else w * h         # floats between the planes: not a round number
    d_dst = torch.full((2 * RIM_F + n * ps,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.y8_to_plane_device(d_src.data_ptr() + lay.off, n, lay.frame, lay.row, w, h, rng, d_dst.data_ptr() + 4 * RIM_F, 4 * ps, stream=stream().cuda_stream)
    stream().synchronize()
    got = d_dst.cpu().numpy()
    body = got[RIM_F:RIM_F + n * ps].reshape(n, ps)
    assert np.isnan(got[:RIM_F]).all() and np.isnan(got[RIM_F + n * ps:]).all() and np.isnan(body[:, w * h:]).all(), "floats outside the planes were written"
    return body[:, :w * h].reshape(n, h, w), d_src, lay


def plane_to_y8(gpu, x, rng, aligned=False):
    n, h, w = x.shape
    lay = Lay(n, h, w, 1, aligned)
    ps = (w * h + 5) if n > 1 else w * h
    src = np.full((n, ps), np.nan, np.float32)
    src[:, :w * h] = x.reshape(n, w * h)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((lay.total,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.plane_to_y8_device(d_src.data_ptr(), n, 4 * ps, w, h, rng, d_dst.data_ptr() + lay.off, lay.frame, lay.row, stream=stream().cuda_stream)
    stream().synchronize()
    return lay.gather(d_dst.cpu().numpy(), 0xAB)


def torch_luma_in(d_bytes, rng):
    y = d_bytes.to(torch.float32)
    if rng == yr.LIMITED:
        return (y - 16.0) * float(F32(1.0 / 219.0))
    return y * float(F32(1.0 / 255.0))


def torch_luma_out(d_y, rng):
    r = d_y * 219.0 + 16.0 if rng == yr.LIMITED else d_y * 255.0      # (two kernels: the product and the sum are not contracted)
    return torch.clamp(torch.round(r), 0, 255).to(torch.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


LUMA_SHAPES = [(1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 257, 1), (1, 16, 16), (3, 37, 53), (2, 3, 85)]     # (n, h, w): the edges of a 256-thread block


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned"])
@pytest.mark.parametrize("shape", LUMA_SHAPES, ids=["%dx%dx%d" % s for s in LUMA_SHAPES])
def test_y8_to_plane(gpu, shape, aligned, rng):
    n, h, w = shape
    planes = np.random.default_rng(n + 10 * h + 1000 * w).integers(0, 256, shape, dtype=np.uint8)
    got, _, _ = y8_to_plane(gpu, planes, rng, aligned)
    want = torch_luma_in(torch.from_numpy(planes).cuda(), rng).cpu().numpy()
    assert same_bits(got, want) and same_bits(got, yr.luma_in(planes, rng))


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
def test_luma_ends_on_all_256_values(gpu, rng):
    """every byte value, in: the expression's bits; out again: the identity"""
    planes = np.arange(256, dtype=np.uint8).reshape(1, 4, 64)
    y, _, _ = y8_to_plane(gpu, planes, rng)
    assert same_bits(y, torch_luma_in(torch.from_numpy(planes).cuda(), rng).cpu().numpy()) and same_bits(y, yr.luma_in(planes, rng))
    assert np.array_equal(plane_to_y8(gpu, y, rng), planes)


@functools.lru_cache(maxsize=None)
def out_values(rng):
    """values around every rounding tie of the output expression, beyond both clamps, and where the product is past int32"""
    k = np.arange(-2, 258)
    if rng == yr.LIMITED:
        c = ((k + 0.5 - 16.0) / 219.0).astype(np.float32)
    else:
        c = ((k + 0.5) / 255.0).astype(np.float32)
    vals = np.concatenate([c, np.nextafter(c, F32(np.inf)), np.nextafter(c, F32(-np.inf)),
                           np.array([-1e10, -3e9, -1e7, -1.0, -0.08, -1e-9, -0.0, 0.0, 1.0, 1.0 + 1e-3, 1.1, 7.5, 1e7, 3e9, 1e10, 3e38, -3e38], np.float32)])
    vals.setflags(write=False)
    return vals


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
def test_plane_to_y8_ties_clamps_and_int32(gpu, rng):
    vals = out_values(rng)
    x = vals.reshape(1, 1, vals.size)
    got = plane_to_y8(gpu, x, rng)
    want = torch_luma_out(torch.from_numpy(np.array(x)).cuda(), rng).cpu().numpy()
    with np.errstate(over="ignore"):       # (+-3e38: the product is an infinity, and saturates)
        assert np.array_equal(got, want) and np.array_equal(got, yr.luma_out(x, rng))
        # the list holds exact ties, and they went to even
        r = (vals * F32(219.0) + F32(16.0)) if rng == yr.LIMITED else vals * F32(255.0)
    tie = (r == np.floor(r) + F32(0.5)) & (r > 0) & (r < 255)
    assert tie.sum() >= 100, int(tie.sum())
    g = got.ravel()[tie].astype(np.int64)
    assert (g % 2 == 0).all() and (np.abs(g - r[tie]) == 0.5).all()
    assert (np.floor(r[tie]) % 2 == 1).sum() >= 100, "ties that round up and ties that round down"
    # (-1e-9, -0.0 and 0.0: byte 0 in full range, byte 16 in limited range; everything beyond the clamps, infinities of the product included, saturates)
    z, one = (16, 235) if rng == yr.LIMITED else (0, 255)
    assert got.ravel()[-17:].tolist() == [0] * 5 + [z] * 3 + [one] * 2 + [255] * 5 + [255, 0]


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned"])
@pytest.mark.parametrize("shape", LUMA_SHAPES, ids=["%dx%dx%d" % s for s in LUMA_SHAPES])
def test_plane_to_y8(gpu, shape, aligned, rng):
    x = np.random.default_rng(sum(shape)).random(shape, dtype=np.float32) * F32(1.5) - F32(0.25)      # both saturation ends
    got = plane_to_y8(gpu, x, rng, aligned)
    want = torch_luma_out(torch.from_numpy(x).cuda(), rng).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got, yr.luma_out(x, rng))
    if x.size >= 255:
        assert want.min() == 0 and want.max() == 255 and ((want > 0) & (want < 255)).mean() > 0.3, "the clip must not hide the values"


# k_px runs at most 65536 x 256 = 2^24 threads along a plane: with more elements a thread takes a second one
BIG_H, BIG_W = 4096, 4097


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
def test_luma_second_trip(gpu, rng):
    assert BIG_H * BIG_W > 65536 * 256
    d_b = torch.randint(0, 256, (BIG_H * BIG_W + 64,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    src = d_b[32:32 + BIG_H * BIG_W]
    d_y = torch.full((BIG_H * BIG_W + 2 * RIM_F,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.y8_to_plane_device(src.data_ptr(), 1, 0, BIG_W, BIG_W, BIG_H, rng, d_y.data_ptr() + 4 * RIM_F, 4 * BIG_H * BIG_W, stream=stream().cuda_stream)
    stream().synchronize()
    y = d_y[RIM_F:RIM_F + BIG_H * BIG_W]
    assert torch.isnan(d_y[:RIM_F]).all() and torch.isnan(d_y[RIM_F + BIG_H * BIG_W:]).all()
    assert torch.equal(y.view(torch.int32), torch_luma_in(src, rng).view(torch.int32))
    d_o = torch.full((BIG_H * BIG_W + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.plane_to_y8_device(y.data_ptr(), 1, 4 * BIG_H * BIG_W, BIG_W, BIG_H, rng, d_o.data_ptr() + 32, 0, BIG_W, stream=stream().cuda_stream)
    stream().synchronize()
    assert (d_o[:32] == 0xAB).all() and (d_o[32 + BIG_H * BIG_W:] == 0xAB).all()
    assert torch.equal(d_o[32:32 + BIG_H * BIG_W], src), "bytes -> planes -> bytes is the identity"
    assert torch.equal(d_o[32:32 + BIG_H * BIG_W], torch_luma_out(y, rng))


# ---- the chroma kernel ----
def composed_chroma(gpu, planes, ow, oh):
    """the route of calls that exist without the kernel: torch u8 * (1 / 255), w2xc_resize2x_cubic_device per plane, torch clamp(round(255 v)), the crop"""
    n, ch, cw = planes.shape
    d_c = torch.from_numpy(planes).cuda().to(torch.float32) * float(F32(1.0 / 255.0))
    d_up = torch.empty((n, 2 * ch, 2 * cw), dtype=torch.float32, device="cuda")
    for i in range(n):
        assert gpu.lib().w2xc_resize2x_cubic_device(d_c[i].data_ptr(), cw, ch, d_up[i].data_ptr(), stream().cuda_stream) == 0, gpu.last_error()
    stream().synchronize()
    out = torch.clamp(torch.round(d_up * 255.0), 0, 255).to(torch.uint8)
    return out[:, :oh, :ow].cpu().numpy()


def chroma2x(gpu, planes, ow=None, oh=None, spx=1, dpx=1, src_aligned=False, dst_aligned=False):
    n, ch, cw = planes.shape
    ow, oh = 2 * cw if ow is None else ow, 2 * ch if oh is None else oh
    ls, ld = Lay(n, ch, cw, spx, src_aligned), Lay(n, oh, ow, dpx, dst_aligned)
    d_src = torch.from_numpy(ls.scatter(planes, "random" if spx == 2 else 0x5A)).cuda()
    d_dst = torch.full((ld.total,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.chroma2x_u8_device(d_src.data_ptr() + ls.off, n, ls.frame, ls.row, spx, cw, ch, d_dst.data_ptr() + ld.off, ld.frame, ld.row, dpx, ow, oh, stream=stream().cuda_stream)
    stream().synchronize()
    return ld.gather(d_dst.cpu().numpy(), 0xAB)


# cw x ch: the smallest, two tiny ones, and -- a tile is 32 x 16 quads, a plane of cw x ch samples has (cw + 1) x (ch + 1) of them -- one quad short of a tile
# edge, on it and past it in both directions, as quads (30 .. 32 x 14 .. 16) and as source samples (33 x 17)
CHROMA_SIZES = [(1, 1), (2, 3), (9, 17), (30, 14), (31, 15), (32, 16), (33, 17), (31, 16), (32, 15), (70, 40)]


@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "dwords"])
@pytest.mark.parametrize("size", CHROMA_SIZES, ids=["%dx%d" % s for s in CHROMA_SIZES])
def test_chroma2x_sizes(gpu, size, aligned):
    cw, ch = size
    planes = np.random.default_rng(cw * 100 + ch).integers(0, 256, (1, ch, cw), dtype=np.uint8)
    want = composed_chroma(gpu, planes, 2 * cw, 2 * ch)
    assert np.array_equal(want[0], yr.chroma2x(planes[0])), "the restatement of tests/yuv_ref.py"
    assert np.array_equal(chroma2x(gpu, planes, src_aligned=aligned, dst_aligned=aligned), want)
    # odd cropped output sizes: the chroma of an odd-sized frame
    for ow, oh in ((2 * cw - 1, 2 * ch - 1), (2 * cw - 1, 2 * ch), (2 * cw, 2 * ch - 1)):
        assert np.array_equal(chroma2x(gpu, planes, ow, oh, src_aligned=aligned, dst_aligned=not aligned), want[:, :oh, :ow]), (ow, oh)


@pytest.mark.parametrize("spx,dpx", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned"])
def test_chroma2x_sample_strides_and_frames(gpu, spx, dpx, aligned):
    """n = 3 planes with frame strides, planar and interleaved on either side: with 2-byte samples the bytes in between are another plane's -- random in the
    source, and in the destination they must stay what they were"""
    planes = np.random.default_rng(10 * spx + dpx).integers(0, 256, (3, 21, 37), dtype=np.uint8)
    want = composed_chroma(gpu, planes, 73, 41)
    assert np.array_equal(chroma2x(gpu, planes, 73, 41, spx, dpx, aligned, aligned), want)


def test_chroma2x_two_planes_interleave_in_either_order(gpu):
    """NV12 as two calls: U into the even bytes, V into the odd ones, neither touching the other's"""
    cw, ch = 19, 11
    rng = np.random.default_rng(8)
    u, v = rng.integers(0, 256, (1, ch, cw), dtype=np.uint8), rng.integers(0, 256, (1, ch, cw), dtype=np.uint8)
    wu, wv = composed_chroma(gpu, u, 2 * cw, 2 * ch), composed_chroma(gpu, v, 2 * cw, 2 * ch)
    src = np.stack([u[0], v[0]], axis=-1)                       # (ch, cw, 2)
    d_src = torch.from_numpy(src).cuda()
    for order in ((0, 1), (1, 0)):
        d_dst = torch.full((2 * ch, 2 * cw, 2), 0xAB, dtype=torch.uint8, device="cuda")
        for k in order:
            gpu.chroma2x_u8_device(d_src.data_ptr() + k, 1, 0, 2 * cw, 2, cw, ch, d_dst.data_ptr() + k, 0, 4 * cw, 2, 2 * cw, 2 * ch, stream=stream().cuda_stream)
            stream().synchronize()
            got = d_dst.cpu().numpy()
            assert np.array_equal(got[:, :, k], (wu, wv)[k][0])
            if k == order[0]:
                assert (got[:, :, 1 - k] == 0xAB).all(), "the other plane's bytes"
        assert np.array_equal(d_dst.cpu().numpy(), np.stack([wu[0], wv[0]], axis=-1))


@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "dwords"])
def test_chroma2x_constant_planes(gpu, aligned):
    """a constant plane of every byte value comes back as that value: the four coefficients sum to 1 within the rounding to a byte"""
    planes = np.repeat(np.arange(256, dtype=np.uint8), 6 * 5).reshape(256, 6, 5)
    got = chroma2x(gpu, planes, src_aligned=aligned)
    assert np.array_equal(got, np.repeat(np.arange(256, dtype=np.uint8), 12 * 10).reshape(256, 12, 10))
    assert np.array_equal(got, composed_chroma(gpu, planes, 10, 12))


@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "dwords"])
def test_chroma2x_checkerboard_saturates(gpu, aligned):
    board = (np.indices((35, 67)).sum(0) % 2 * 255).astype(np.uint8)
    stripes = np.zeros((35, 67), np.uint8)
    stripes[:, ::3] = 255
    stripes[::4] = 255
    planes = np.stack([board, 255 - board, stripes])
    want = composed_chroma(gpu, planes, 134, 70)
    float_up = yr.resize2x_cubic(stripes.astype(np.float32) * F32(1.0 / 255.0))
    assert float_up.min() < -0.05 and float_up.max() > 1.05, "the overshoot the clamp is there for"
    assert want.min() == 0 and want.max() == 255
    assert np.array_equal(chroma2x(gpu, planes, src_aligned=aligned, dst_aligned=aligned), want)


def test_chroma2x_more_tiles_than_workgroups(gpu):
    """the grid-stride loop's second trip: 3 planes of 863 x 415 samples are 2106 tile turns for 2048 workgroups, so workgroups 0 .. 57 take a second
    tile -- of the next plane's rows, on LDS words the first turn left"""
    n, cw, ch = 3, 863, 415
    turns, grid = yr.chroma_launch(2 * cw, 2 * ch, n)
    assert turns > grid == yr.GRID_MAX and turns == 27 * 26 * 3
    planes = np.random.default_rng(21).integers(0, 256, (n, ch, cw), dtype=np.uint8)
    want = composed_chroma(gpu, planes, 2 * cw, 2 * ch)
    for aligned in (True, False):
        assert np.array_equal(chroma2x(gpu, planes, src_aligned=aligned, dst_aligned=aligned), want)
