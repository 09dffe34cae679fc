"""GPU tests of the co-sited forms of the six tile kernels of the YUV frame calls (csrc/w2xc_yuv_sited.hip, w2xc_yuv16_sited.hip, w2xc_yuv_rgb_sited.hip,
w2xc_yuv16_rgb_sited.hip through w2xc_chroma2x_u8_sited_device, w2xc_chroma2x_u16_sited_device and, with the flags in `chroma`, w2xc_yuv8_to_rgb_device,
w2xc_rgb_to_yuv8_device, w2xc_yuv16_to_rgb_device, w2xc_rgb_to_yuv16_device).  Every comparison is equality of bytes, words or float bits with the NumPy restatement
of "Chroma siting" (tests/yuv_sited_ref.py).  The buffers and their sentinel rims -- in front, behind, between rows, planes and frames, and with interleaved
samples between the samples -- are those of the centred kernels' tests, whose helpers build them."""
import numpy as np
import pytest

from conftest import small_layers
import yuv_ref as yr
import yuv_rgb_ref as rr
import yuv16_ref as y16
import yuv_sited_ref as sr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_yuv_blocks import Lay, same_bits, stream   # noqa: E402
from test_gpu_yuv_blocks import chroma2x as chroma2x_centred   # noqa: E402
from test_gpu_yuv_rgb_blocks import NV12, NV21, PLANAR, RIM_F, Planes, make_side   # noqa: E402
from test_gpu_yuv16_blocks import FILL, Lay16, Side16, float_planes, junk_words, to_dev, to_host   # noqa: E402
from test_gpu_yuv16_blocks import chroma2x16 as chroma2x16_centred   # noqa: E402

F32 = np.float32
X, Y_, XY = sr.COSITED_X, sr.COSITED_Y, sr.COSITED_X | sr.COSITED_Y
FLAGS = (X, Y_, XY)
FLAG_IDS = ["x", "y", "xy"]
SITED_IDS = [sr.SITED_IDS[c] for c in sr.ALL_SITED]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


# ---- the bicubic 2x ----
def chroma2x8(gpu, planes, cosited, ow=None, oh=None, spx=1, dpx=1, src_aligned=False, dst_aligned=False):
    n, ch, cw = planes.shape
    ow, oh = 2 * cw if ow is None else ow, 2 * ch if oh is None else oh
    ls, ld = Lay(n, ch, cw, spx, src_aligned), Lay(n, oh, ow, dpx, dst_aligned)
    d_src = torch.from_numpy(ls.scatter(planes, "random" if spx == 2 else 0x5A)).cuda()
    d_dst = torch.full((ld.total,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.chroma2x_u8_sited_device(d_src.data_ptr() + ls.off, n, ls.frame, ls.row, spx, cw, ch, d_dst.data_ptr() + ld.off, ld.frame, ld.row, dpx, ow, oh, cosited,
                                 stream=stream().cuda_stream)
    stream().synchronize()
    return ld.gather(d_dst.cpu().numpy(), 0xAB)


def chroma2x16(gpu, values, depth, cosited, ow=None, oh=None, spx=1, dpx=1, spack=0, dpack=0, salign=1, dalign=1):
    """-> the VALUES of the output (its words unpacked, after checking that they are packed as dpack says)"""
    n, ch, cw = values.shape
    ow, oh = 2 * cw if ow is None else ow, 2 * ch if oh is None else oh
    ls, ld = Lay16(n, ch, cw, spx, salign), Lay16(n, oh, ow, dpx, dalign)
    d_src = to_dev(ls.scatter(junk_words(values, depth, spack), "random" if spx == 2 else 0x5A5A))
    d_dst = to_dev(np.full(ld.total, FILL, np.uint16))
    gpu.chroma2x_u16_sited_device(d_src.data_ptr() + 2 * ls.off, n, 2 * ls.frame, 2 * ls.row, spx, spack, cw, ch, depth, d_dst.data_ptr() + 2 * ld.off, 2 * ld.frame,
                                  2 * ld.row, dpx, dpack, ow, oh, cosited, stream=stream().cuda_stream)
    stream().synchronize()
    words = ld.gather(to_host(d_dst))
    vals = y16.unpack(words, depth, dpack).astype(np.uint16)
    assert np.array_equal(words, y16.pack_words(vals, depth, dpack)), "the bits outside the value are zero"
    return vals


def want2x(values, cosited, depth, ow=None, oh=None):
    return np.stack([sr.chroma2x(p, cosited, depth, ow, oh) for p in values])


# cw x ch: the smallest three; a tile is 32 x 16 quads and a plane of cw x ch samples has (cw + 1) x (ch + 1) of them: one short of a tile edge, on it, past it
CHROMA_SIZES = [(1, 1), (2, 2), (3, 3), (30, 14), (31, 15), (32, 16), (33, 17), (31, 16), (32, 15), (35, 20)]


@pytest.mark.parametrize("cosited", FLAGS, ids=FLAG_IDS)
def test_chroma2x_u8_sizes(gpu, cosited):
    for k, (cw, ch) in enumerate(CHROMA_SIZES):
        planes = np.random.default_rng(cw * 100 + ch).integers(0, 256, (1, ch, cw), dtype=np.uint8)
        want = want2x(planes, cosited, 8)
        for aligned in (False, True):
            assert np.array_equal(chroma2x8(gpu, planes, cosited, src_aligned=aligned, dst_aligned=aligned), want), (cw, ch, aligned)
        for ow, oh in ((2 * cw - 1, 2 * ch - 1), (2 * cw - 1, 2 * ch), (2 * cw, 2 * ch - 1)):      # odd cropped sizes: the chroma of an odd-sized frame
            assert np.array_equal(chroma2x8(gpu, planes, cosited, ow, oh, src_aligned=bool(k & 1), dst_aligned=not k & 1), want[:, :oh, :ow]), (cw, ch, ow, oh)


@pytest.mark.parametrize("cosited", FLAGS, ids=FLAG_IDS)
def test_chroma2x_u16_sizes(gpu, cosited):
    depth = 10
    for k, (cw, ch) in enumerate(CHROMA_SIZES):
        values = np.random.default_rng(cw * 100 + ch).integers(0, 1 << depth, (1, ch, cw)).astype(np.uint16)
        want = want2x(values, cosited, depth)
        for align in (1, 2, 4):
            assert np.array_equal(chroma2x16(gpu, values, depth, cosited, salign=align, dalign=align), want), (cw, ch, align)
        ow, oh = 2 * cw - 1, 2 * ch - 1
        assert np.array_equal(chroma2x16(gpu, values, depth, cosited, ow, oh, salign=(1, 2, 4)[k % 3], dalign=(4, 1, 2)[k % 3]), want[:, :oh, :ow]), (cw, ch)


def test_no_flag_is_the_centred_block(gpu):
    """the anchor: cosited = 0 through the new entry points is the existing block, byte for byte and word for word"""
    planes = np.random.default_rng(3).integers(0, 256, (2, 21, 37), dtype=np.uint8)
    assert np.array_equal(chroma2x8(gpu, planes, 0, 73, 41), chroma2x_centred(gpu, planes, 73, 41))
    assert np.array_equal(chroma2x8(gpu, planes, 0, 73, 41), np.stack([yr.chroma2x(p, 73, 41) for p in planes]))
    values = np.random.default_rng(4).integers(0, 1 << 12, (2, 21, 37)).astype(np.uint16)
    assert np.array_equal(chroma2x16(gpu, values, 12, 0, 73, 41, dpack=1), chroma2x16_centred(gpu, values, 12, 73, 41, dpack=1))
    for cosited in FLAGS:
        assert not np.array_equal(chroma2x8(gpu, planes, cosited, 73, 41), chroma2x_centred(gpu, planes, 73, 41)), "a flag must show"


@pytest.mark.parametrize("cosited", FLAGS, ids=FLAG_IDS)
def test_chroma2x_strides_frames_depths_and_packings(gpu, cosited):
    """n = 3 planes with frame strides, planar and interleaved on either side (NV12 / P010 chroma, one plane per call); with interleaved samples the samples in
    between are another plane's: random in the source, and in the destination they must stay what they were"""
    planes = np.random.default_rng(cosited).integers(0, 256, (3, 21, 37), dtype=np.uint8)
    planes[0, :2, :3] = 255
    want = want2x(planes, cosited, 8, 73, 41)
    for spx, dpx in ((1, 1), (1, 2), (2, 1), (2, 2)):
        for aligned in (False, True):
            assert np.array_equal(chroma2x8(gpu, planes, cosited, 73, 41, spx, dpx, aligned, aligned), want), (spx, dpx, aligned)
    for depth in (8, 10, 16):
        for pack in (y16.LOW, y16.HIGH):
            values = np.random.default_rng(depth + pack).integers(0, 1 << depth, (3, 21, 37)).astype(np.uint16)
            values[0, :2, :3] = y16.maxval(depth)
            want = want2x(values, cosited, depth, 73, 41)
            for k, (spx, dpx) in enumerate(((1, 1), (1, 2), (2, 1), (2, 2))):
                align = (1, 2, 4)[(k + depth) % 3]
                assert np.array_equal(chroma2x16(gpu, values, depth, cosited, 73, 41, spx, dpx, pack, (pack + k) & 1, align, align), want), (depth, pack, spx, dpx)


@pytest.mark.parametrize("cosited", FLAGS, ids=FLAG_IDS)
def test_chroma2x_constants_ramps_and_saturation(gpu, cosited):
    """constant planes come back as their value; the ramp 40 + 8 k comes out as 39 + 4 m on a co-sited axis (38 + 4 m on a centred one); a checkerboard of
    0 / M overshoots and saturates at both clamps"""
    for depth in (8, 10, 16):
        M = y16.maxval(depth)
        consts = np.unique(np.concatenate([np.arange(0, M + 1, max(1, M // 37)), [1, M - 1, M]])).astype(np.uint16)
        planes = np.repeat(consts, 6 * 5).reshape(consts.size, 6, 5)
        assert np.array_equal(chroma2x16(gpu, planes, depth, cosited, salign=4), np.repeat(consts, 12 * 10).reshape(consts.size, 12, 10))
        board = (np.indices((35, 67)).sum(0) % 2 * M).astype(np.uint16)
        stripes = np.zeros((35, 67), np.uint16)
        stripes[:, ::3] = M
        stripes[::4] = M
        planes = np.stack([board, M - board, stripes])
        want = want2x(planes, cosited, depth)
        assert want.min() == 0 and want.max() == M
        up = sr.resize2x_cubic(stripes.astype(F32) * F32(1.0 / M), bool(cosited & X), bool(cosited & Y_))
        assert up.min() < -0.05 and up.max() > 1.05, "the overshoot the clamp is there for"
        assert np.array_equal(chroma2x16(gpu, planes, depth, cosited, salign=4, dalign=4), want)
        if depth == 8:
            assert np.array_equal(chroma2x8(gpu, planes.astype(np.uint8), cosited, src_aligned=True), want)
    ramp = (40 + 8 * np.arange(16)).astype(np.uint8)
    m = np.arange(4, 28)
    for axis, bit in ((1, X), (0, Y_)):
        plane = np.tile(ramp, (6, 1)) if axis == 1 else np.tile(ramp[:, None], (1, 6))
        got = chroma2x8(gpu, plane[None], cosited)[0].astype(int)
        line = np.take(np.take(got, m, axis=axis), 3, axis=1 - axis)
        assert np.array_equal(line, (39 if cosited & bit else 38) + 4 * m), (axis, line)


def test_chroma2x_more_turns_than_workgroups(gpu):
    """the grid-stride loop's second trip: one tall thin plane of 2049 tiles for 2048 workgroups"""
    c = y16.CHROMA_SECOND_TRIP
    turns, grid = y16.chroma_launch(2 * c["cw"], 2 * c["ch"], c["n"])
    assert turns > grid == y16.GRID_MAX
    values = np.random.default_rng(21).integers(0, 1 << 10, (c["n"], c["ch"], c["cw"])).astype(np.uint16)
    assert np.array_equal(chroma2x16(gpu, values, 10, XY, salign=4, dalign=4, dpack=1), want2x(values, XY, 10))
    planes = (values >> 2).astype(np.uint8)
    assert yr.chroma_launch(2 * c["cw"], 2 * c["ch"], 1)[0] > yr.GRID_MAX
    assert np.array_equal(chroma2x8(gpu, planes, X), want2x(planes, X, 8))


@pytest.fixture(scope="module")
def y_scale(gpu):
    """a short one-plane scale model: the Y route of a frame call needs one for its luma; its chroma never meets it"""
    return gpu._ModelSet.from_layers(small_layers([1, 32, 32, 1], 32))


@pytest.mark.parametrize("cosited", FLAGS, ids=FLAG_IDS)
def test_chroma2x_every_load_path(gpu, y_scale, cosited):
    """every instantiation of the two 2x kernels that the launchers can ask the selectors for with this flag, picked by how the buffers lie -- k_chroma2x_u8_sited
    <DW 1> planar rows on 4-byte boundaries, <DW 0> odd addresses; k_chroma2x_u16_sited <LOAD 1> planar rows on 8-byte boundaries, <LOAD 0> odd addresses,
    <LOAD 2> interleaved with v = u + 1 and rows on 4-byte boundaries.  The blocks take one plane a call, so LOAD 2 is reached through the 16-bit Y frame call on
    P010 input, whose chroma is the 2x of its input whatever the model.  n = 2 frames of 33 x 17 samples: 2 x 2 tiles of 32 x 16 quads with a one-sample rim"""
    n, cw, ch, depth = 2, 33, 17, 10
    r = np.random.default_rng(1000 + cosited)
    planes = r.integers(0, 256, (n, ch, cw), dtype=np.uint8)
    want = want2x(planes, cosited, 8)
    for aligned in (False, True):
        assert np.array_equal(chroma2x8(gpu, planes, cosited, src_aligned=aligned, dst_aligned=aligned), want), aligned
    U, V = (r.integers(0, 1 << depth, (n, ch, cw)).astype(np.uint16) for _ in range(2))
    want_u, want_v = want2x(U, cosited, depth), want2x(V, cosited, depth)
    for align in (1, 4):
        assert np.array_equal(chroma2x16(gpu, U, depth, cosited, salign=align, dalign=align), want_u), align
    w, h = 2 * cw, 2 * ch
    Y = r.integers(0, 1 << depth, (n, h, w)).astype(np.uint16)
    i = Side16(gpu, n, w, h, yr.YUV_420, "p010", 1, 2).upload(Y, U, V, depth)
    o = Side16(gpu, n, 2 * w, 2 * h, yr.YUV_420, "planar", 0, 1)
    gpu.process_frames_yuv_u16_device(n, w, h, yr.YUV_420 | cosited, i.s, o.s, None, y_scale, 1, yr.FULL, stream=stream().cuda_stream, depth=depth)
    stream().synchronize()
    _, got_u, got_v = o.download(depth)
    assert np.array_equal(got_u, want_u) and np.array_equal(got_v, want_v)


# ---- the two ends of the RGB route ----
def to_rgb8(gpu, Y, U, V, chroma, rng, matrix, kind=PLANAR, aligned=False):
    n, h, w = Y.shape
    side = make_side(gpu, n, w, h, chroma & 0xF, kind, aligned).upload(Y, U, V)
    P = Planes(n, w, h, aligned)
    d = torch.full((P.total,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.yuv8_to_rgb_device(side.s, n, w, h, chroma, rng, matrix, d.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, stream=stream().cuda_stream)
    stream().synchronize()
    return P.gather(d.cpu().numpy())


def from_rgb8(gpu, x, chroma, rng, matrix, kind=PLANAR, aligned=False):
    n, _, h, w = x.shape
    P = Planes(n, w, h, aligned)
    d = torch.from_numpy(P.scatter(x)).cuda()
    side = make_side(gpu, n, w, h, chroma & 0xF, kind, aligned)
    gpu.rgb_to_yuv8_device(d.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, n, w, h, chroma, rng, matrix, side.s, stream=stream().cuda_stream)
    stream().synchronize()
    return side.download()   # (checks the rims)


def to_rgb16(gpu, Y, U, V, chroma, rng, matrix, depth, style="planar", pack=0, align=1, even=True):
    n, h, w = Y.shape
    side = Side16(gpu, n, w, h, chroma & 0xF, style, pack, align).upload(Y, U, V, depth)
    ps, is_ = float_planes(n, w, h, even)
    d = torch.full((2 * RIM_F + n * is_,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.yuv16_to_rgb_device(side.s, n, w, h, chroma, rng, depth, matrix, d.data_ptr() + 4 * RIM_F, 4 * is_, 4 * ps, stream=stream().cuda_stream)
    stream().synchronize()
    got = d.cpu().numpy()
    body = got[RIM_F:RIM_F + n * is_].reshape(n, is_)
    planes = np.stack([body[:, p * ps:p * ps + w * h] for p in range(3)], axis=1).reshape(n, 3, h, w)
    mask = np.ones(is_, bool)
    for p in range(3):
        mask[p * ps:p * ps + w * h] = False
    assert np.isnan(got[:RIM_F]).all() and np.isnan(got[RIM_F + n * is_:]).all() and np.isnan(body[:, mask]).all(), "floats outside the planes were written"
    return planes


def from_rgb16(gpu, planes, chroma, rng, matrix, depth, style="planar", pack=0, align=1, even=True):
    n, _, h, w = planes.shape
    ps, is_ = float_planes(n, w, h, even)
    src = np.full((n, is_), np.nan, np.float32)
    for p in range(3):
        src[:, p * ps:p * ps + w * h] = planes[:, p].reshape(n, w * h)
    d = torch.from_numpy(src).cuda()
    side = Side16(gpu, n, w, h, chroma & 0xF, style, pack, align)
    gpu.rgb_to_yuv16_device(d.data_ptr(), 4 * is_, 4 * ps, n, w, h, chroma, rng, depth, matrix, side.s, stream=stream().cuda_stream)
    stream().synchronize()
    return side.download(depth)


def frames(n, w, h, chroma, depth, seed):
    r = np.random.default_rng(seed)
    cw, ch = sr.chroma_size(w, h, chroma)
    dt = np.uint8 if depth == 8 else np.uint16
    return tuple(r.integers(0, 1 << depth, s).astype(dt) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))


def float_frames(n, w, h, seed):
    """R, G, B around and beyond [0, 1]"""
    return np.random.default_rng(seed).random((n, 3, h, w), dtype=np.float32) * F32(1.3) - F32(0.15)


def check8(gpu, n, w, h, chroma, rng, matrix, kind, aligned, seed):
    Y, U, V = frames(n, w, h, chroma, 8, seed)
    got = to_rgb8(gpu, Y, U, V, chroma, rng, matrix, kind, aligned)
    for i in range(n):
        assert same_bits(got[i], sr.yuv_to_rgb(Y[i], U[i], V[i], chroma, rng, matrix)), ("to rgb", w, h, hex(chroma), rng, matrix, kind, aligned)
    x = float_frames(n, w, h, seed + 1)
    back = from_rgb8(gpu, x, chroma, rng, matrix, kind, aligned)
    for i in range(n):
        for name, g, w_ in zip("YUV", back, sr.rgb_to_yuv(x[i], chroma, rng, matrix)):
            assert np.array_equal(g[i], w_), ("from rgb", name, w, h, hex(chroma), rng, matrix, kind, aligned, int((g[i] != w_).sum()))


def check16(gpu, n, w, h, chroma, rng, matrix, depth, style, pack, align, even, seed):
    Y, U, V = frames(n, w, h, chroma, depth, seed)
    Y, U, V = (a.astype(np.uint16) for a in (Y, U, V))
    got = to_rgb16(gpu, Y, U, V, chroma, rng, matrix, depth, style, pack, align, even)
    for i in range(n):
        assert same_bits(got[i], sr.yuv_to_rgb(Y[i], U[i], V[i], chroma, rng, matrix, depth)), ("to rgb", w, h, hex(chroma), rng, matrix, depth, style, pack, align, even)
    x = float_frames(n, w, h, seed + 1)
    back = from_rgb16(gpu, x, chroma, rng, matrix, depth, style, pack, align, even)
    for i in range(n):
        for name, g, w_ in zip("YUV", back, sr.rgb_to_yuv(x[i], chroma, rng, matrix, depth)):
            assert np.array_equal(g[i], w_), ("from rgb", name, w, h, hex(chroma), rng, matrix, depth, style, pack, align, even, int((g[i] != w_).sum()))


# luma sizes: the smallest three, and around one tile of 32 x 16 chroma samples in both directions -- one and two tiles each way, so a non-first tile's left
# column and top row are exchanged through memory
RGB_SIZES = [(1, 1), (2, 2), (3, 3)] + [(w, h) for w in (63, 64, 65, 66) for h in (31, 32, 33, 34)]
KINDS = (PLANAR, NV12, NV21)
STYLES = ("planar", "p010", "vu")


@pytest.mark.parametrize("chroma", sr.ALL_SITED, ids=SITED_IDS)
def test_rgb_ends_u8_sizes(gpu, chroma):
    for k, (w, h) in enumerate(RGB_SIZES):
        check8(gpu, 1, w, h, chroma, yr.LIMITED, rr.BT709, KINDS[k % 3], bool(k & 1), 300 + k)
    check8(gpu, 1, 130, 68, chroma, yr.FULL, rr.BT601, PLANAR, True, 340)       # 3 x 3 tiles (4:2:2: 3 x 5): an inner tile has neighbours on every side


@pytest.mark.parametrize("chroma", sr.ALL_SITED, ids=SITED_IDS)
def test_rgb_ends_u16_sizes(gpu, chroma):
    for k, (w, h) in enumerate(RGB_SIZES):
        check16(gpu, 1, w, h, chroma, yr.LIMITED, rr.BT2020, 10, STYLES[k % 3], k & 1, (1, 2, 4)[k % 3], bool(k % 2), 400 + k)
    check16(gpu, 1, 130, 68, chroma, yr.FULL, rr.BT709, 12, "p010", 1, 4, True, 440)


@pytest.mark.parametrize("chroma", sr.ALL_SITED, ids=SITED_IDS)
def test_rgb_ends_every_load_path(gpu, chroma):
    """every instantiation of the four RGB-route kernels that the launchers can ask the selectors for with this layout and these flags, picked by how the planes
    lie -- k_yuv8_to_rgb_sited <DW 1> rows on 4-byte boundaries, <DW 0> odd addresses; k_yuv16_to_rgb_sited <CM 1> planar chroma rows on 8-byte boundaries, <CM 2>
    P010 rows on 4-byte boundaries, <CM 0> odd addresses; k_rgb_to_yuv8_sited / k_rgb_to_yuv16_sited have one instantiation per pair and run in every check.
    n = 2 frames of 67 x 35 luma samples in 4:2:0, 67 x 17 in 4:2:2: chroma planes 34 wide, one tile of 32 x 16 chroma samples and a rim in both directions"""
    w, h = (67, 35) if chroma & 0xF == yr.YUV_420 else (67, 17)
    check8(gpu, 2, w, h, chroma, yr.LIMITED, rr.BT709, PLANAR, True, 700)
    check8(gpu, 2, w, h, chroma, yr.FULL, rr.BT601, PLANAR, False, 702)
    check16(gpu, 2, w, h, chroma, yr.LIMITED, rr.BT2020, 10, "planar", 0, 4, True, 704)
    check16(gpu, 2, w, h, chroma, yr.FULL, rr.BT709, 10, "p010", 1, 2, False, 706)
    check16(gpu, 2, w, h, chroma, yr.LIMITED, rr.BT601, 12, "planar", 1, 1, False, 708)


@pytest.mark.parametrize("chroma", sr.SITED_LAYOUTS, ids=[sr.SITED_IDS[c] for c in sr.SITED_LAYOUTS])
def test_rgb_ends_grid(gpu, chroma):
    """the three sited layouts x both ranges x three matrices, on planar / NV12 / NV21 bytes and planar / P010 / VU words at D = 8, 10, 16 with both packings,
    three frames with strides; the alignment of the planes and of the float rows goes round with the cases, so every load and store path meets every arithmetic"""
    k = 0
    for rng in (yr.FULL, yr.LIMITED):
        for matrix in rr.MATRICES:
            w, h = ((37, 19), (38, 18))[k & 1]
            check8(gpu, 3, w, h, chroma, rng, matrix, KINDS[k % 3], (k // 3) % 2 == 0, 500 + k)
            depth, pack = ((8, 0), (10, 1), (16, 0), (10, 0), (8, 1), (16, 1))[k]
            check16(gpu, 3, w, h, chroma, rng, matrix, depth, STYLES[(k + 1) % 3], pack, (4, 2, 1)[k % 3], (k // 3) % 2 == 0, 600 + k)
            k += 1


def test_no_flag_is_the_centred_end(gpu):
    """the anchor: without a flag the ends give the centred restatement's bits, and a flag shows"""
    Y, U, V = frames(2, 37, 19, yr.YUV_420, 8, 7)
    got = to_rgb8(gpu, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709)
    assert all(same_bits(got[i], rr.yuv8_to_rgb(Y[i], U[i], V[i], yr.YUV_420, yr.LIMITED, rr.BT709)) for i in range(2))
    x = float_frames(2, 37, 19, 8)
    back = from_rgb8(gpu, x, yr.YUV_420, yr.LIMITED, rr.BT709)
    for i in range(2):
        assert all(np.array_equal(g[i], w_) for g, w_ in zip(back, rr.rgb_to_yuv8(x[i], yr.YUV_420, yr.LIMITED, rr.BT709)))
    for chroma in sr.ALL_SITED[:2]:
        assert not same_bits(to_rgb8(gpu, Y, U, V, chroma, yr.LIMITED, rr.BT709), got)
        sited = from_rgb8(gpu, x, chroma, yr.LIMITED, rr.BT709)
        assert np.array_equal(sited[0], back[0]) and not np.array_equal(sited[1], back[1]), "luma does not depend on the siting, chroma does"


@pytest.mark.parametrize("chroma", sr.SITED_LAYOUTS, ids=[sr.SITED_IDS[c] for c in sr.SITED_LAYOUTS])
def test_rgb_ends_ramps_extremes_ties_and_clamps(gpu, chroma):
    layout = chroma & 0xF
    # a chroma ramp along x and its mirror image through the matrix, compared as the restatement's bits; constants stay put
    w, h = 62, 12
    cw, ch = sr.chroma_size(w, h, chroma)
    ramp = np.tile((40 + 6 * np.arange(cw)).astype(np.uint8), (ch, 1))[None]
    Y = np.full((1, h, w), 126, np.uint8)
    got = to_rgb8(gpu, Y, ramp, ramp[:, :, ::-1].copy(), chroma, yr.FULL, rr.BT601, PLANAR, True)
    assert same_bits(got[0], sr.yuv_to_rgb(Y[0], ramp[0], ramp[0, :, ::-1], chroma, yr.FULL, rr.BT601))
    for depth in (8, 10, 16):
        M, s = y16.maxval(depth), y16.step(depth)
        for rng in (yr.FULL, yr.LIMITED):
            for cy in (0, M):
                for cu, cv in ((0, M), (128 * s, 128 * s), (M, 0), (M, M)):
                    Yc, Uc, Vc = np.full((1, 6, 10), cy, np.uint16), np.full((1, ch_(6, layout), 5), cu, np.uint16), np.full((1, ch_(6, layout), 5), cv, np.uint16)
                    got = to_rgb16(gpu, Yc, Uc, Vc, chroma, rng, rr.BT2020, depth, "planar", 0, 4)
                    assert same_bits(got[0], sr.yuv_to_rgb(Yc[0], Uc[0], Vc[0], chroma, rng, rr.BT2020, depth))
            # grey planes at k + 0.5 of the luma word, and planes far outside [0, 1]: the clamps, past int32 too; one colour alone in single samples drives the
            # 1-2-1 mean past both chroma clamps and through infinities
            scale, off = (219.0 * s, 16.0 * s) if rng == yr.LIMITED else (float(M), 0.0)
            x = ((np.arange(0, 2048) + 0.5 - off) / scale).astype(np.float32).reshape(1, 1, 32, 64)
            planes = np.repeat(x, 3, axis=1)
            planes[0, :, 0, :8] = np.array([-1e10, -3e9, -1.0, -0.08, 1.2, 3e9, 1e10, 3e38], np.float32)
            planes[0, 0, 3, 0:8:2] = np.array([1e10, -1e10, 3e38, -3e38], np.float32)
            planes[0, 2, 5, 1:9:2] = np.array([1e10, -1e10, 3e38, -3e38], np.float32)      # odd columns: a neighbour's sample, not a chroma site
            with np.errstate(over="ignore", invalid="ignore"):
                want = sr.rgb_to_yuv(planes[0], chroma, rng, rr.BT709, depth)
            for g, w_ in zip(from_rgb16(gpu, planes, chroma, rng, rr.BT709, depth, "p010", 1, 2), want):
                assert np.array_equal(g[0], w_)
            assert want[0].min() == 0 and want[0].max() == M and want[1].min() == 0 and want[1].max() == M
            if depth == 8:
                for g, w_ in zip(from_rgb8(gpu, planes, chroma, rng, rr.BT709, NV12, True), want):
                    assert np.array_equal(g[0], w_)


def ch_(h, layout):
    return (h + 1) // 2 if layout == yr.YUV_420 else h


def test_rgb_ends_more_turns_than_workgroups(gpu):
    """2 x 1025 tiles for 2048 workgroups: a workgroup's second turn reuses its LDS rows (from RGB) and tiles (to RGB)"""
    r = sr.RGB_SECOND_TRIP
    turns, grid = rr.launch(r["w"], r["h"], yr.YUV_420, r["n"])
    assert turns > grid == rr.GRID_MAX
    check8(gpu, r["n"], r["w"], r["h"], sr.YUV_420_TOPLEFT, yr.LIMITED, rr.BT709, PLANAR, True, 900)
    check16(gpu, r["n"], r["w"], r["h"], yr.YUV_420 | sr.COSITED_Y, yr.LIMITED, rr.BT2020, 10, "p010", 1, 2, False, 910)
