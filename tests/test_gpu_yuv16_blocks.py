"""GPU tests of the building blocks of the 16-bit YUV frame calls (csrc/w2xc_yuv16.hip, csrc/w2xc_yuv16_rgb.hip through w2xc_y16_to_plane_device,
w2xc_plane_to_y16_device, w2xc_chroma2x_u16_device, w2xc_yuv16_to_rgb_device and w2xc_rgb_to_yuv16_device).  Every comparison is equality of words or of
float bits with the NumPy restatement (tests/yuv16_ref.py); the chroma kernel also against the composed route torch u16 * (1 / M) ->
w2xc_resize2x_cubic_device -> clamp(round(M v)) -> crop.  Every buffer has a sentinel rim -- in front, behind, between rows, between frames, and with
interleaved samples between the samples -- that must be intact."""
import numpy as np
import pytest

import yuv_ref as yr
import yuv_rgb_ref as rr
import yuv16_ref as y16

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
RIM_F = 8            # floats in front of and behind every float output: they stay NaN
FILL = 0xABCD        # the word every buffer of words is filled with


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def stream():
    return torch.cuda.current_stream()


def to_dev(words):
    """a uint16 array on the device (as int16: the bits are what counts)"""
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint16).view(np.int16)).cuda()


def to_host(d):
    return d.cpu().numpy().view(np.uint16)


# ---- planes of words in a buffer with rims: n planes of rows x cols samples, px WORDS apart.  align (in words): 4 = every row on an 8-byte boundary,
#      2 = on a 4-byte boundary and no more, 1 = an odd base (one sample off), odd row and frame strides ----
class Lay16:
    def __init__(self, n, rows, cols, px=1, align=1):
        self.n, self.rows, self.cols, self.px, self.align = n, rows, cols, px, align
        self.row_words = px * (cols - 1) + 1
        if align == 4:
            self.off, self.row = 16, (self.row_words + 3) // 4 * 4 + 4
            self.frame = self.rows * self.row + 8
        elif align == 2:      # two samples off an 8-byte boundary
            self.off, self.row = 14, (self.row_words + 1) // 2 * 2 + 2
            self.row += 2 if self.row % 4 == 0 else 0
            self.frame = self.rows * self.row + 6 - (self.rows * self.row % 4)
            assert self.row % 4 == 2 and self.frame % 4 == 2
        else:
            self.off, self.row = 13, self.row_words + 3 - (self.row_words & 1)
            self.frame = self.rows * self.row + 5 - (self.rows * self.row & 1)
            assert self.row & 1 and self.frame & 1
        self.total = self.off + n * self.frame + 16

    def index(self):
        f, r, c = np.meshgrid(np.arange(self.n), np.arange(self.rows), np.arange(self.cols), indexing="ij")
        return self.off + f * self.frame + r * self.row + c * self.px

    def scatter(self, planes, fill=FILL):
        buf = np.random.default_rng(99).integers(0, 1 << 16, self.total).astype(np.uint16) if isinstance(fill, str) else np.full(self.total, fill, np.uint16)
        buf[self.index()] = planes
        return buf

    def gather(self, buf, fill=FILL):
        idx = self.index()
        rest = np.ones(self.total, bool)
        rest[idx] = False
        assert (buf[rest] == fill).all(), "words outside the samples were written: %d of them" % int((buf[rest] != fill).sum())
        return buf[idx]


def junk_words(values, depth, pack, seed=7):
    """the values as words whose ignored bits are set at random: the low bits of HIGH, the high bits of LOW"""
    w = y16.pack_words(values, depth, pack).astype(np.uint32)
    j = np.random.default_rng(seed).integers(0, 1 << 16, w.shape).astype(np.uint32)
    w |= (j & ((1 << (16 - depth)) - 1)) if pack == y16.HIGH else (j & (0xFFFF & ~y16.maxval(depth)))
    return w.astype(np.uint16)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


DEPTH_PACK = [(d, p) for d in (8, 10, 12, 16) for p in (y16.LOW, y16.HIGH)]
DP_IDS = ["d%d-%s" % (d, "high" if p else "low") for d, p in DEPTH_PACK]


# ---- the luma stages ----
def y16_to_plane(gpu, values, rng, depth, pack, align=1):
    n, h, w = values.shape
    lay = Lay16(n, h, w, 1, align)
    d_src = to_dev(lay.scatter(junk_words(values, depth, pack), 0x5A5A))
    ps = (w * h + 3) if n > 1 else w * h
    d_dst = torch.full((2 * RIM_F + n * ps,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.y16_to_plane_device(d_src.data_ptr() + 2 * lay.off, n, 2 * lay.frame, 2 * lay.row, w, h, rng, depth, pack, d_dst.data_ptr() + 4 * RIM_F, 4 * ps,
                            stream=stream().cuda_stream)
    stream().synchronize()
    got = d_dst.cpu().numpy()
    body = got[RIM_F:RIM_F + n * ps].reshape(n, ps)
    assert np.isnan(got[:RIM_F]).all() and np.isnan(got[RIM_F + n * ps:]).all() and np.isnan(body[:, w * h:]).all(), "floats outside the planes were written"
    return body[:, :w * h].reshape(n, h, w)


def plane_to_y16(gpu, x, rng, depth, pack, align=1):
    """-> the WORDS"""
    n, h, w = x.shape
    lay = Lay16(n, h, w, 1, align)
    ps = (w * h + 5) if n > 1 else w * h
    src = np.full((n, ps), np.nan, np.float32)
    src[:, :w * h] = x.reshape(n, w * h)
    d_src = torch.from_numpy(src).cuda()
    d_dst = to_dev(np.full(lay.total, FILL, np.uint16))
    gpu.plane_to_y16_device(d_src.data_ptr(), n, 4 * ps, w, h, rng, depth, pack, d_dst.data_ptr() + 2 * lay.off, 2 * lay.frame, 2 * lay.row, stream=stream().cuda_stream)
    stream().synchronize()
    return lay.gather(to_host(d_dst))


LUMA_SHAPES = [(1, 1, 1), (1, 2, 1), (1, 1, 2), (1, 3, 3), (1, 1, 255), (1, 1, 256), (1, 257, 1), (3, 37, 53), (2, 3, 85)]     # (n, h, w)


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("dp", DEPTH_PACK, ids=DP_IDS)
def test_luma_stages(gpu, dp, rng):
    depth, pack = dp
    for k, shape in enumerate(LUMA_SHAPES):
        align = (1, 2, 4)[k % 3]
        r = np.random.default_rng(sum(shape) + depth)
        values = r.integers(0, 1 << depth, shape).astype(np.uint16)
        got = y16_to_plane(gpu, values, rng, depth, pack, align)
        t = torch.from_numpy(values.astype(np.int32)).cuda().to(torch.float32)      # the header's expression, one torch kernel per operation
        t = (t - 16.0 * y16.step(depth)) * float(F32(1.0 / (219.0 * y16.step(depth)))) if rng == yr.LIMITED else t * float(F32(1.0 / y16.maxval(depth)))
        assert same_bits(got, y16.luma_in(values, rng, depth)) and same_bits(got, t.cpu().numpy()), (shape, align)
        x = r.random(shape, dtype=np.float32) * F32(1.5) - F32(0.25)               # both saturation ends
        words = plane_to_y16(gpu, x, rng, depth, pack, align)
        want = y16.luma_out(x, rng, depth)
        assert np.array_equal(words, y16.pack_words(want, depth, pack)), (shape, align)
        if x.size >= 255:
            assert want.min() == 0 and want.max() == y16.maxval(depth), "the clip must not hide the values"


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("dp", [(10, 0), (10, 1), (12, 0), (12, 1), (16, 0)], ids=["d10-low", "d10-high", "d12-low", "d12-high", "d16"])
def test_luma_ends_on_all_values(gpu, dp, rng):
    """every value 0 .. M (at 16 bits: a stride of 7 through them, and both ends): in, the expression's bits; out again, the identity"""
    depth, pack = dp
    M = y16.maxval(depth)
    v = np.arange(M + 1, dtype=np.uint32) if depth < 16 else np.unique(np.concatenate([np.arange(0, M + 1, 7), [M - 1, M]])).astype(np.uint32)
    v = np.resize(v, (v.size + 63) // 64 * 64).reshape(1, -1, 64).astype(np.uint16)
    y = y16_to_plane(gpu, v, rng, depth, pack)
    assert same_bits(y, y16.luma_in(v, rng, depth))
    assert np.array_equal(plane_to_y16(gpu, y, rng, depth, pack), y16.pack_words(v, depth, pack))


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("depth", [8, 10, 16])
def test_plane_to_y16_ties_clamps_and_int32(gpu, depth, rng):
    M, s = y16.maxval(depth), y16.step(depth)
    k = np.arange(-2, min(M, 3000) + 2)
    scale, off = (219.0 * s, 16.0 * s) if rng == yr.LIMITED else (float(M), 0.0)
    c = ((k + 0.5 - off) / scale).astype(np.float32)
    top = ((np.arange(M - 40, M + 3) + 0.5 - off) / scale).astype(np.float32)
    vals = np.concatenate([c, np.nextafter(c, F32(np.inf)), np.nextafter(c, F32(-np.inf)), top,
                           np.array([-1e10, -3e9, -1e7, -1.0, -0.08, -1e-9, -0.0, 0.0, 1.0, 1.0 + 1e-3, 1.1, 7.5, 1e7, 3e9, 1e10, 3e38, -3e38], np.float32)])
    x = vals.reshape(1, 1, vals.size)
    got = plane_to_y16(gpu, x, rng, depth, y16.LOW)
    with np.errstate(over="ignore"):
        assert np.array_equal(got, y16.luma_out(x, rng, depth))
        r = vals * F32(scale) + F32(off) if rng == yr.LIMITED else vals * F32(scale)
    tie = (r == np.floor(r) + F32(0.5)) & (r > 0) & (r < M)
    assert tie.sum() >= 8, int(tie.sum())
    g = got.ravel()[tie].astype(np.int64)
    assert (g % 2 == 0).all() and (np.abs(g - r[tie].astype(np.float64)) == 0.5).all()
    # (-1e-9, -0.0 and 0.0: the word of black; 1.0: the word of white; everything beyond the clamps, infinities of the product included, saturates)
    z, one = (16 * s, 235 * s) if rng == yr.LIMITED else (0, M)
    tail = got.ravel()[-17:].tolist()
    assert tail[:5] == [0] * 5 and tail[5:8] == [z] * 3 and tail[8] == one and one <= tail[9] <= M and tail[10:] == [M] * 5 + [M, 0]


# ---- the chroma kernel ----
def composed_chroma16(gpu, values, depth, ow, oh):
    """the route of calls that exist without the kernel: torch value * (1 / M), w2xc_resize2x_cubic_device per plane, torch clamp(round(M v)), the crop"""
    n, ch, cw = values.shape
    M = y16.maxval(depth)
    d_c = torch.from_numpy(values.astype(np.int32)).cuda().to(torch.float32) * float(F32(1.0 / M))
    d_up = torch.empty((n, 2 * ch, 2 * cw), dtype=torch.float32, device="cuda")
    for i in range(n):
        assert gpu.lib().w2xc_resize2x_cubic_device(d_c[i].data_ptr(), cw, ch, d_up[i].data_ptr(), stream().cuda_stream) == 0, gpu.last_error()
    stream().synchronize()
    out = torch.clamp(torch.round(d_up * float(M)), 0, M).to(torch.int32)
    return out[:, :oh, :ow].cpu().numpy().astype(np.uint16)


def chroma2x16(gpu, values, depth, ow=None, oh=None, spx=1, dpx=1, spack=0, dpack=0, salign=1, dalign=1):
    """-> the VALUES of the output (its words unpacked, after checking that they are packed as dpack says)"""
    n, ch, cw = values.shape
    ow, oh = 2 * cw if ow is None else ow, 2 * ch if oh is None else oh
    ls, ld = Lay16(n, ch, cw, spx, salign), Lay16(n, oh, ow, dpx, dalign)
    d_src = to_dev(ls.scatter(junk_words(values, depth, spack), "random" if spx == 2 else 0x5A5A))
    d_dst = to_dev(np.full(ld.total, FILL, np.uint16))
    gpu.chroma2x_u16_device(d_src.data_ptr() + 2 * ls.off, n, 2 * ls.frame, 2 * ls.row, spx, spack, cw, ch, depth, d_dst.data_ptr() + 2 * ld.off, 2 * ld.frame,
                            2 * ld.row, dpx, dpack, ow, oh, stream=stream().cuda_stream)
    stream().synchronize()
    words = ld.gather(to_host(d_dst))
    vals = y16.unpack(words, depth, dpack).astype(np.uint16)
    assert np.array_equal(words, y16.pack_words(vals, depth, dpack)), "the bits outside the value are zero"
    return vals


# cw x ch: the smallest; a tile is 32 x 16 quads and a plane of cw x ch samples has (cw + 1) x (ch + 1) of them: one short of a tile edge, on it, past it
CHROMA_SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (30, 14), (31, 15), (32, 16), (33, 17), (31, 16), (32, 15), (35, 20)]


@pytest.mark.parametrize("align", [1, 2, 4], ids=["odd", "4byte", "8byte"])
@pytest.mark.parametrize("size", CHROMA_SIZES, ids=["%dx%d" % s for s in CHROMA_SIZES])
def test_chroma2x_sizes(gpu, size, align):
    cw, ch = size
    depth = 10
    values = np.random.default_rng(cw * 100 + ch).integers(0, 1 << depth, (1, ch, cw)).astype(np.uint16)
    want = composed_chroma16(gpu, values, depth, 2 * cw, 2 * ch)
    assert np.array_equal(want[0], y16.chroma2x(values[0], depth)), "the restatement of tests/yuv16_ref.py"
    assert np.array_equal(chroma2x16(gpu, values, depth, salign=align, dalign=align), want)
    for ow, oh in ((2 * cw - 1, 2 * ch - 1), (2 * cw - 1, 2 * ch), (2 * cw, 2 * ch - 1)):      # odd cropped sizes: the chroma of an odd-sized frame
        assert np.array_equal(chroma2x16(gpu, values, depth, ow, oh, salign=align, dalign=(4, 1, 2)[align // 2]), want[:, :oh, :ow]), (ow, oh)


@pytest.mark.parametrize("dp", DEPTH_PACK, ids=DP_IDS)
def test_chroma2x_depths_packings_strides_and_frames(gpu, dp):
    """n = 3 planes with frame strides, planar and interleaved on either side, the packings of the two sides differing: with interleaved samples the words in
    between are another plane's -- random in the source, and in the destination they must stay what they were"""
    depth, pack = dp
    values = np.random.default_rng(depth + pack).integers(0, 1 << depth, (3, 21, 37)).astype(np.uint16)
    values[0, :2, :3] = y16.maxval(depth)
    want = composed_chroma16(gpu, values, depth, 73, 41)
    assert np.array_equal(want[1], y16.chroma2x(values[1], depth, 73, 41))
    for k, (spx, dpx) in enumerate(((1, 1), (1, 2), (2, 1), (2, 2))):
        for align in (1, 2, 4):
            got = chroma2x16(gpu, values, depth, 73, 41, spx, dpx, pack, (pack + k) & 1, align, align)
            assert np.array_equal(got, want), (spx, dpx, align)


def test_chroma2x_two_planes_interleave_in_either_order(gpu):
    """P010 chroma as two calls: U into the even words, V into the odd ones, neither touching the other's"""
    cw, ch, depth = 19, 11, 10
    r = np.random.default_rng(8)
    u, v = (r.integers(0, 1 << depth, (1, ch, cw)).astype(np.uint16) for _ in range(2))
    wu, wv = composed_chroma16(gpu, u, depth, 2 * cw, 2 * ch), composed_chroma16(gpu, v, depth, 2 * cw, 2 * ch)
    d_src = to_dev(np.stack([u[0], v[0]], axis=-1) << 6)                       # (ch, cw, 2), high-packed
    for order in ((0, 1), (1, 0)):
        d_dst = to_dev(np.full((2 * ch, 2 * cw, 2), FILL, np.uint16))
        for k in order:
            gpu.chroma2x_u16_device(d_src.data_ptr() + 2 * k, 1, 0, 4 * cw, 2, 1, cw, ch, depth, d_dst.data_ptr() + 2 * k, 0, 8 * cw, 2, 1, 2 * cw, 2 * ch,
                                    stream=stream().cuda_stream)
            stream().synchronize()
            got = to_host(d_dst)
            assert np.array_equal(got[:, :, k], (wu, wv)[k][0] << 6)
            if k == order[0]:
                assert (got[:, :, 1 - k] == FILL).all(), "the other plane's words"
        assert np.array_equal(to_host(d_dst), np.stack([wu[0], wv[0]], axis=-1) << 6)


@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_chroma2x_constants_and_checkerboard(gpu, depth):
    """constant planes come back as their value; a checkerboard of 0 / M overshoots and saturates at both clamps"""
    M = y16.maxval(depth)
    consts = np.unique(np.concatenate([np.arange(0, M + 1, max(1, M // 97)), [1, M - 1, M]])).astype(np.uint16)
    planes = np.repeat(consts, 6 * 5).reshape(consts.size, 6, 5)
    assert np.array_equal(chroma2x16(gpu, planes, depth, salign=4), np.repeat(consts, 12 * 10).reshape(consts.size, 12, 10))
    board = (np.indices((35, 67)).sum(0) % 2 * M).astype(np.uint16)
    stripes = np.zeros((35, 67), np.uint16)
    stripes[:, ::3] = M
    stripes[::4] = M
    planes = np.stack([board, M - board, stripes])
    want = composed_chroma16(gpu, planes, depth, 134, 70)
    up = yr.resize2x_cubic(stripes.astype(np.float32) * F32(1.0 / M))
    assert up.min() < -0.05 and up.max() > 1.05 and want.min() == 0 and want.max() == M, "the overshoot the clamp is there for"
    for align in (1, 4):
        assert np.array_equal(chroma2x16(gpu, planes, depth, salign=align, dalign=align), want)


def test_chroma2x_more_turns_than_workgroups(gpu):
    """the grid-stride loop's second trip: one tall thin plane of 2049 tiles for 2048 workgroups -- workgroup 0 takes a second tile, on LDS words the first
    turn left"""
    c = y16.CHROMA_SECOND_TRIP
    turns, grid = y16.chroma_launch(2 * c["cw"], 2 * c["ch"], c["n"])
    assert turns > grid == y16.GRID_MAX
    values = np.random.default_rng(21).integers(0, 1 << 10, (c["n"], c["ch"], c["cw"])).astype(np.uint16)
    want = composed_chroma16(gpu, values, 10, 2 * c["cw"], 2 * c["ch"])
    for align in (4, 1):
        assert np.array_equal(chroma2x16(gpu, values, 10, salign=align, dalign=align, dpack=1), want)


# ---- the two ends of the RGB route ----
STYLES = ("planar", "p010", "vu")      # two planes; interleaved with v = u + 1 sample; interleaved with u = v + 1


class Side16:
    """n frames of words in device buffers with rims and their Yuv16Planes; style: how the chroma planes lie"""

    def __init__(self, gpu, n, w, h, layout, style="planar", pack=0, align=1):
        self.n, self.w, self.h, self.style, self.pack = n, w, h, style, pack
        self.cw, self.ch = yr.chroma_size(w, h, layout)
        self.ly = Lay16(n, h, w, 1, align)
        self.by = to_dev(np.full(self.ly.total, FILL, np.uint16))
        s = gpu.Yuv16Planes()
        s.y, s.y_stride, s.y_frame_stride = self.by.data_ptr() + 2 * self.ly.off, 2 * self.ly.row, 2 * self.ly.frame
        s.c_px, s.pack = (1 if style == "planar" else 2), pack
        if self.cw:
            if style == "planar":
                self.lc = Lay16(n, self.ch, self.cw, 1, align)
                self.bc = [to_dev(np.full(self.lc.total, FILL, np.uint16)) for _ in range(2)]
                s.u, s.v = (b.data_ptr() + 2 * self.lc.off for b in self.bc)
            else:      # one plane of ch rows of 2 cw words
                self.lc = Lay16(n, self.ch, 2 * self.cw, 1, align)
                self.bc = [to_dev(np.full(self.lc.total, FILL, np.uint16))]
                first = self.bc[0].data_ptr() + 2 * self.lc.off
                s.u, s.v = (first, first + 2) if style == "p010" else (first + 2, first)
            s.c_stride, s.c_frame_stride = 2 * self.lc.row, 2 * self.lc.frame
        self.s = s

    def _pair(self, U, V):
        a, b = (U, V) if self.style == "p010" else (V, U)
        return np.stack([a, b], axis=-1).reshape(self.n, self.ch, 2 * self.cw)

    def upload(self, Y, U, V, depth, junk=True):
        """values in; the words carry random bits where the packing ignores them"""
        wd = (lambda a: junk_words(a, depth, self.pack)) if junk else (lambda a: y16.pack_words(a, depth, self.pack))
        self.by.copy_(to_dev(self.ly.scatter(wd(Y))))
        if self.cw:
            if self.style == "planar":
                for b, P in zip(self.bc, (U, V)):
                    b.copy_(to_dev(self.lc.scatter(wd(P))))
            else:
                self.bc[0].copy_(to_dev(self.lc.scatter(wd(self._pair(U, V)))))
        return self

    def download(self, depth, written=True):
        """(Y, U, V) VALUES; every word outside the planes kept its fill, and -- written: the planes are a call's output -- every word's bits outside the
        value are zero"""
        words = [self.ly.gather(to_host(self.by))]
        if self.cw:
            if self.style == "planar":
                words += [self.lc.gather(to_host(b)) for b in self.bc]
            else:
                uv = self.lc.gather(to_host(self.bc[0])).reshape(self.n, self.ch, self.cw, 2)
                k = 0 if self.style == "p010" else 1
                words += [np.ascontiguousarray(uv[..., k]), np.ascontiguousarray(uv[..., 1 - k])]
        vals = [y16.unpack(a, depth, self.pack).astype(np.uint16) for a in words]
        assert not written or all(np.array_equal(a, y16.pack_words(v, depth, self.pack)) for a, v in zip(words, vals)), "the bits outside the value are zero"
        return tuple(vals) + (None,) * (3 - len(vals))


def float_planes(n, w, h, even):
    """(floats between planes, between images): even -> every row of even-width planes on an 8-byte boundary (the float2 path), else odd plane strides"""
    ps = (w * h + 7) // 2 * 2 if even else w * h + 3 - (w * h & 1)
    return ps, 3 * ps + (2 if even else 1)


def to_rgb16(gpu, Y, U, V, layout, rng, matrix, depth, style="planar", pack=0, align=1, even=True):
    n, h, w = Y.shape
    side = Side16(gpu, n, w, h, layout, style, pack, align).upload(Y, U, V, depth)
    ps, is_ = float_planes(n, w, h, even)
    d = torch.full((2 * RIM_F + n * is_,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.yuv16_to_rgb_device(side.s, n, w, h, layout, rng, depth, matrix, d.data_ptr() + 4 * RIM_F, 4 * is_, 4 * ps, stream=stream().cuda_stream)
    stream().synchronize()
    got = d.cpu().numpy()
    body = got[RIM_F:RIM_F + n * is_].reshape(n, is_)
    planes = np.stack([body[:, p * ps:p * ps + w * h] for p in range(3)], axis=1).reshape(n, 3, h, w)
    mask = np.ones(is_, bool)
    for p in range(3):
        mask[p * ps:p * ps + w * h] = False
    assert np.isnan(got[:RIM_F]).all() and np.isnan(got[RIM_F + n * is_:]).all() and np.isnan(body[:, mask]).all(), "floats outside the planes were written"
    return planes


def from_rgb16(gpu, planes, layout, rng, matrix, depth, style="planar", pack=0, align=1, even=True):
    n, _, h, w = planes.shape
    ps, is_ = float_planes(n, w, h, even)
    src = np.full((n, is_), np.nan, np.float32)
    for p in range(3):
        src[:, p * ps:p * ps + w * h] = planes[:, p].reshape(n, w * h)
    d = torch.from_numpy(src).cuda()
    side = Side16(gpu, n, w, h, layout, style, pack, align)
    gpu.rgb_to_yuv16_device(d.data_ptr(), 4 * is_, 4 * ps, n, w, h, layout, rng, depth, matrix, side.s, stream=stream().cuda_stream)
    stream().synchronize()
    return side.download(depth)


def frames16(n, w, h, layout, depth, seed):
    r = np.random.default_rng(seed)
    cw, ch = yr.chroma_size(w, h, layout)
    return tuple(r.integers(0, 1 << depth, s).astype(np.uint16) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))


def check_both_ends(gpu, n, w, h, layout, rng, matrix, depth, style, pack, align, even, seed):
    Y, U, V = frames16(n, w, h, layout, depth, seed)
    got = to_rgb16(gpu, Y, U, V, layout, rng, matrix, depth, style, pack, align, even)
    for i in range(n):
        assert same_bits(got[i], y16.yuv16_to_rgb(Y[i], U[i], V[i], layout, rng, matrix, depth)), ("to rgb", w, h, layout, rng, matrix, depth, style, pack, align, even)
    planes = np.random.default_rng(seed + 1).random((n, 3, h, w), dtype=np.float32) * F32(1.3) - F32(0.15)
    back = from_rgb16(gpu, planes, layout, rng, matrix, depth, style, pack, align, even)
    for i in range(n):
        for name, g, w_ in zip("YUV", back, y16.rgb_to_yuv16(planes[i], layout, rng, matrix, depth)):
            assert np.array_equal(g[i], w_), ("from rgb", name, w, h, layout, rng, matrix, depth, style, pack, align, even)


RGB_SIZES = [(1, 1), (1, 2), (2, 1), (3, 3)] + [(w, h) for w in (63, 64, 65, 66) for h in (31, 32, 33, 34)]     # around one tile of 32 x 16 chroma samples


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("layout", rr.LAYOUTS, ids=["420", "422", "444"])
def test_rgb_ends_sizes(gpu, layout, style):
    for k, (w, h) in enumerate(RGB_SIZES):
        check_both_ends(gpu, 1, w, h, layout, yr.LIMITED, rr.BT2020, 10, style, k & 1, (1, 2, 4)[k % 3], bool(k % 2), 300 + k)


@pytest.mark.parametrize("dp", DEPTH_PACK, ids=DP_IDS)
def test_rgb_ends_grid(gpu, dp):
    """depths x packings x ranges x matrices x chroma layouts x plane styles, on odd and even frames, three frames with strides; the alignment of the planes
    and of the float rows goes round with the cases, so every load and store path meets every arithmetic"""
    depth, pack = dp
    k = 0
    for rng in (yr.FULL, yr.LIMITED):
        for matrix in rr.MATRICES:
            for layout in rr.LAYOUTS:
                for style in STYLES:
                    w, h = ((37, 19), (38, 18))[k & 1]
                    check_both_ends(gpu, 3, w, h, layout, rng, matrix, depth, style, pack, (4, 2, 1)[k % 3], (k // 3) % 2 == 0, 500 + k)
                    k += 1


def test_rgb_ends_u_and_v_are_not_swapped(gpu):
    """with a matrix the order of U and V shows: the three plane styles give one result, and swapping the planes another"""
    Y, U, V = frames16(1, 34, 18, yr.YUV_420, 10, 77)
    ref = to_rgb16(gpu, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709, 10, "planar")
    for style in ("p010", "vu"):
        assert same_bits(to_rgb16(gpu, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709, 10, style, align=2), ref)
    assert not same_bits(to_rgb16(gpu, Y, V, U, yr.YUV_420, yr.LIMITED, rr.BT709, 10, "p010", align=2), ref)


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_rgb_ends_on_all_values_and_extremes(gpu, depth):
    """every value 0 .. M (16 bits: a stride through them) as luma against every value as chroma, constant frames at the extremes, grey ramps at rounding ties"""
    M = y16.maxval(depth)
    v = np.arange(M + 1, dtype=np.uint32) if depth < 16 else np.unique(np.concatenate([np.arange(0, M + 1, 13), [M - 1, M]])).astype(np.uint32)
    v = np.resize(v, (v.size + 63) // 64 * 64).reshape(1, -1, 64).astype(np.uint16)
    U, V = v[:, ::-1, :].copy(), np.roll(v, 5, axis=1)
    for rng in (yr.FULL, yr.LIMITED):
        got = to_rgb16(gpu, v, U, V, yr.YUV_444, rng, rr.BT2020, depth, "p010", 1, 2)
        assert same_bits(got[0], y16.yuv16_to_rgb(v[0], U[0], V[0], yr.YUV_444, rng, rr.BT2020, depth))
        for cy in (0, M):
            for cu in (0, 128 * y16.step(depth), M):
                for cv in (0, M):
                    Y, Uc, Vc = (np.full((1, 6, 10), c, np.uint16) for c in (cy, cu, cv))
                    Uc, Vc = Uc[:, :3, :5], Vc[:, :3, :5]
                    got = to_rgb16(gpu, Y, Uc, Vc, yr.YUV_420, rng, rr.BT601, depth, "planar", 0, 4)
                    assert same_bits(got[0], y16.yuv16_to_rgb(Y[0], Uc[0], Vc[0], yr.YUV_420, rng, rr.BT601, depth))
        # grey planes at k + 0.5 of the luma word, and planes far outside [0, 1]: the clamps, past int32 too
        scale, off = (219.0 * y16.step(depth), 16.0 * y16.step(depth)) if rng == yr.LIMITED else (float(M), 0.0)
        x = ((np.arange(0, 2048) + 0.5 - off) / scale).astype(np.float32).reshape(1, 1, 32, 64)
        planes = np.repeat(x, 3, axis=1)
        planes[0, :, 0, :8] = np.array([-1e10, -3e9, -1.0, -0.08, 1.2, 3e9, 1e10, 3e38], np.float32)
        planes[0, 0, 3, 0:8:2] = np.array([1e10, -1e10, 3e38, -3e38], np.float32)    # red alone, one sample per block: chroma past both clamps
        with np.errstate(over="ignore", invalid="ignore"):
            want = y16.rgb_to_yuv16(planes[0], yr.YUV_420, rng, rr.BT709, depth)
        for g, w_ in zip(from_rgb16(gpu, planes, yr.YUV_420, rng, rr.BT709, depth, "p010", 1, 2), want):
            assert np.array_equal(g[0], w_)
        assert want[0].min() == 0 and want[0].max() == M and want[1].min() == 0 and want[1].max() == M


def test_rgb_to_yuv16_leaves_the_words_between_its_samples(gpu):
    """c_px = 2 with U and V in two buffers: the words between a plane's samples are left as they are"""
    n, w, h, depth = 2, 37, 19, 10
    cw, ch = yr.chroma_size(w, h, yr.YUV_420)
    planes = np.random.default_rng(5).random((n, 3, h, w), dtype=np.float32)
    side = Side16(gpu, n, w, h, yr.YUV_420, "planar", 1, 2)
    lc = Lay16(n, ch, cw, 2, 2)
    bufs = [to_dev(np.full(lc.total, FILL, np.uint16)) for _ in range(2)]
    side.s.u, side.s.v, side.s.c_px, side.s.c_stride, side.s.c_frame_stride = bufs[0].data_ptr() + 2 * lc.off, bufs[1].data_ptr() + 2 * lc.off, 2, 2 * lc.row, 2 * lc.frame
    d = torch.from_numpy(planes).cuda()
    gpu.rgb_to_yuv16_device(d.data_ptr(), 4 * 3 * w * h, 4 * w * h, n, w, h, yr.YUV_420, yr.LIMITED, depth, rr.BT709, side.s, stream=stream().cuda_stream)
    stream().synchronize()
    for i in range(n):
        want = y16.rgb_to_yuv16(planes[i], yr.YUV_420, yr.LIMITED, rr.BT709, depth)
        assert np.array_equal(side.ly.gather(to_host(side.by))[i], y16.pack_words(want[0], depth, 1))
        for b, w_ in zip(bufs, want[1:]):
            assert np.array_equal(lc.gather(to_host(b))[i], y16.pack_words(w_, depth, 1))


def test_rgb_ends_more_turns_than_workgroups(gpu):
    r = y16.RGB_SECOND_TRIP
    turns, grid = y16.launch(r["w"], r["h"], r["layout"], r["n"])
    assert turns > grid == rr.GRID_MAX
    check_both_ends(gpu, r["n"], r["w"], r["h"], r["layout"], yr.LIMITED, rr.BT2020, 10, "p010", 1, 2, False, 900)
