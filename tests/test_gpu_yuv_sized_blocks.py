"""GPU tests of the chroma resize kernels of the sized YUV frame calls (csrc/w2xc_yuv_sized.hip, w2xc_yuv16_sized.hip through w2xc_chroma_resize_u8_device and
w2xc_chroma_resize_u16_device).  Every comparison is equality of bytes or words with the NumPy restatement of "Sized YUV frames" (tests/yuv_sized_ref.py), and
at exactly 2x with the bicubic 2x blocks themselves.  The buffers and their sentinel rims -- in front, behind, between rows, planes and frames, and with
interleaved samples between the samples -- are those of the 2x kernels' tests, whose helpers build them."""
import math

import numpy as np
import pytest

import yuv_ref as yr
import yuv16_ref as y16
import yuv_sited_ref as sr
import yuv_sized_ref as zr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_yuv_blocks import Lay, stream   # noqa: E402
from test_gpu_yuv16_blocks import FILL, Lay16, junk_words, to_dev, to_host   # noqa: E402
from test_gpu_yuv_sited_blocks import chroma2x8, chroma2x16   # noqa: E402

X, Y_, XY = sr.COSITED_X, sr.COSITED_Y, sr.COSITED_X | sr.COSITED_Y
# (layout's sub_x, sub_y, cosited): centred, left and top-left on 4:2:0; centred and left on 4:2:2; 4:4:4
FORMS = [(1, 1, 0), (1, 1, X), (1, 1, XY), (1, 0, 0), (1, 0, X), (0, 0, 0)]
FORM_IDS = ["420", "420left", "420topleft", "422", "422left", "444"]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def csize(w, h, sub_x, sub_y):
    return ((w + 1) // 2 if sub_x else w), ((h + 1) // 2 if sub_y else h)


def resize8(gpu, planes, luma, form, spx=1, dpx=1, src_aligned=False, dst_aligned=False):
    """planes (n, ch, cw) uint8 of frames of luma = (w, h, out_w, out_h) -> the (n, och, ocw) bytes of the block, rims checked"""
    w, h, out_w, out_h = luma
    sub_x, sub_y, cosited = form
    n, ch, cw = planes.shape
    assert (cw, ch) == csize(w, h, sub_x, sub_y)
    ow, oh = csize(out_w, out_h, sub_x, sub_y)
    ls, ld = Lay(n, ch, cw, spx, src_aligned), Lay(n, oh, ow, dpx, dst_aligned)
    d_src = torch.from_numpy(ls.scatter(planes, "random" if spx == 2 else 0x5A)).cuda()
    d_dst = torch.full((ld.total,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.chroma_resize_u8_device(d_src.data_ptr() + ls.off, n, ls.frame, ls.row, spx, cw, ch, d_dst.data_ptr() + ld.off, ld.frame, ld.row, dpx, ow, oh, w, h, out_w, out_h,
                                sub_x, sub_y, cosited, stream=stream().cuda_stream)
    stream().synchronize()
    return ld.gather(d_dst.cpu().numpy(), 0xAB)


def resize16(gpu, values, depth, luma, form, spx=1, dpx=1, spack=0, dpack=0, salign=1, dalign=1):
    """-> the VALUES of the output (its words unpacked, after checking that they are packed as dpack says)"""
    w, h, out_w, out_h = luma
    sub_x, sub_y, cosited = form
    n, ch, cw = values.shape
    assert (cw, ch) == csize(w, h, sub_x, sub_y)
    ow, oh = csize(out_w, out_h, sub_x, sub_y)
    ls, ld = Lay16(n, ch, cw, spx, salign), Lay16(n, oh, ow, dpx, dalign)
    d_src = to_dev(ls.scatter(junk_words(values, depth, spack), "random" if spx == 2 else 0x5A5A))
    d_dst = to_dev(np.full(ld.total, FILL, np.uint16))
    gpu.chroma_resize_u16_device(d_src.data_ptr() + 2 * ls.off, n, 2 * ls.frame, 2 * ls.row, spx, spack, cw, ch, depth, d_dst.data_ptr() + 2 * ld.off, 2 * ld.frame,
                                 2 * ld.row, dpx, dpack, ow, oh, w, h, out_w, out_h, sub_x, sub_y, cosited, stream=stream().cuda_stream)
    stream().synchronize()
    words = ld.gather(to_host(d_dst))
    vals = y16.unpack(words, depth, dpack).astype(np.uint16)
    assert np.array_equal(words, y16.pack_words(vals, depth, dpack)), "the bits outside the value are zero"
    return vals


def want(values, luma, form, depth=8):
    w, h, out_w, out_h = luma
    ow, oh = csize(out_w, out_h, form[0], form[1])
    return np.stack([zr.chroma_resize(p, ow, oh, w, h, out_w, out_h, form[0], form[1], form[2], depth) for p in values])


def rand8(n, luma, form, seed):
    cw, ch = csize(luma[0], luma[1], form[0], form[1])
    return np.random.default_rng(seed).integers(0, 256, (n, ch, cw), dtype=np.uint8)


def rand16(n, luma, form, depth, seed):
    cw, ch = csize(luma[0], luma[1], form[0], form[1])
    return np.random.default_rng(seed).integers(0, 1 << depth, (n, ch, cw)).astype(np.uint16)


# luma sizes (w, h, out_w, out_h).  4:2:0 chroma 1 x 1 -> 1 x 1, 1 x 1 -> 2 x 2 (even and odd luma), 3 x 5 -> 4 x 9
TINY = [(2, 2, 2, 2), (1, 1, 1, 1), (2, 2, 4, 4), (1, 1, 3, 3), (6, 10, 8, 18), (5, 9, 7, 17)]


def sweep():
    """output chroma 31 / 32 / 33 / 65 wide and 15 / 16 / 17 high (one short of a tile of 32 x 16 outputs, on it, past it, past two) at the ratios 1, 3 / 2, 2,
    8 / 3 by 9 / 4 and 4; every other case has an odd luma size, where chroma covers w + 1 columns"""
    cases, k = [], 0
    for ocw in (31, 32, 33, 65):
        for och in (15, 16, 17):
            for rx, ry in ((1, 1), (1.5, 1.5), (2, 2), (8 / 3, 9 / 4), (4, 4)):
                out_w, out_h = 2 * ocw - (k & 1), 2 * och - ((k >> 1) & 1)
                cases.append((max(1, math.ceil(out_w / rx)), max(1, math.ceil(out_h / ry)), out_w, out_h))
                k += 1
    return cases


SWEEP = sweep()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_resize_u8_sizes_and_ratios(gpu, form):
    # (on 4:4:4 the chroma of the sweep's luma sizes is twice as large: still seconds)
    for k, luma in enumerate(TINY + SWEEP):
        planes = rand8(1, luma, form, 1000 + k)
        aligned = bool(k & 1)
        got = resize8(gpu, planes, luma, form, src_aligned=aligned, dst_aligned=not aligned)
        assert np.array_equal(got, want(planes, luma, form)), (luma, form, aligned)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_resize_u16_sizes_and_ratios(gpu, form):
    depth = 10
    for k, luma in enumerate(TINY + SWEEP):
        values = rand16(1, luma, form, depth, 2000 + k)
        got = resize16(gpu, values, depth, luma, form, salign=(1, 2, 4)[k % 3], dalign=(4, 1, 2)[k % 3], dpack=k & 1)
        assert np.array_equal(got, want(values, luma, form, depth)), (luma, form)


def test_exact_ratios_the_issue_names(gpu):
    """64 x 36 luma at 3 / 2, 2, 8 / 3 by 9 / 4 and 4; 1 (the copy) on all 256 values"""
    for k, (out_w, out_h) in enumerate(((96, 54), (128, 72), (170, 81), (256, 144), (64, 36))):
        luma = (64, 36, out_w, out_h)
        for form in FORMS:
            planes = rand8(2, luma, form, 30 + k)
            assert np.array_equal(resize8(gpu, planes, luma, form, src_aligned=True, dst_aligned=True), want(planes, luma, form)), (luma, form)
    every = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    for form in FORMS[:3]:
        assert np.array_equal(resize8(gpu, every, (32, 32, 32, 32), form), every), "r = 1 copies"


@pytest.mark.parametrize("form", [FORMS[0], FORMS[2], FORMS[4]], ids=["420", "420topleft", "422left"])
def test_exactly_2x_is_the_2x_block(gpu, form):
    """the anchor: at r = 0.5 the block gives the bytes and words of w2xc_chroma2x_u8_sited_device / _u16_sited_device, the crop of an odd frame included"""
    for w, h in ((74, 42), (73, 41), (64, 32), (2, 2), (1, 1)):
        luma = (w, h, 2 * w, 2 * h)
        cw, ch = csize(w, h, form[0], form[1])
        ow, oh = csize(2 * w, 2 * h, form[0], form[1])
        assert ow <= 2 * cw and oh <= 2 * ch      # (4:2:2: y is not subsampled -- the 2x block doubles its rows, as the resize at r = 0.5 with o = 0.5)
        planes = rand8(2, luma, form, w)
        assert np.array_equal(resize8(gpu, planes, luma, form, src_aligned=True), chroma2x8(gpu, planes, form[2], ow, oh, src_aligned=True)), (w, h, form)
        values = rand16(2, luma, form, 12, w + 1)
        assert np.array_equal(resize16(gpu, values, 12, luma, form, dpack=1, salign=4, dalign=2), chroma2x16(gpu, values, 12, form[2], ow, oh, dpack=1, salign=4, dalign=2))


@pytest.mark.parametrize("form", [FORMS[1], FORMS[2], FORMS[3], FORMS[5]], ids=["420left", "420topleft", "422", "444"])
def test_resize_strides_frames_depths_and_packings(gpu, form):
    """n = 3 planes with frame strides, planar and interleaved on either side (NV12 / NV21 / P010 chroma, one plane per call), pointers one and two samples off,
    odd strides; with interleaved samples the samples in between are another plane's: random in the source, and in the destination they stay what they were"""
    luma = (45, 27, 68, 61)        # 1.51 x by 2.26 x, both sizes odd
    planes = rand8(3, luma, form, 5)
    planes[0, :2, :3] = 255
    w8 = want(planes, luma, form)
    for spx, dpx in ((1, 1), (1, 2), (2, 1), (2, 2)):
        for aligned in (False, True):
            assert np.array_equal(resize8(gpu, planes, luma, form, spx, dpx, aligned, aligned), w8), (spx, dpx, aligned)
    for depth in (8, 10, 16):
        for pack in (y16.LOW, y16.HIGH):
            values = rand16(3, luma, form, depth, depth + pack)
            values[0, :2, :3] = y16.maxval(depth)
            w16 = want(values, luma, form, depth)
            for k, (spx, dpx) in enumerate(((1, 1), (1, 2), (2, 1), (2, 2))):
                for align in (1, 2, 4):
                    got = resize16(gpu, values, depth, luma, form, spx, dpx, pack, (pack + k) & 1, align, (4, 1, 2)[(align + k) % 3])
                    assert np.array_equal(got, w16), (depth, pack, spx, dpx, align)


def test_resize_two_interleaved_planes_fill_in_either_order(gpu):
    """U and V of an NV12 / P010 destination filled by two calls, in either order: the second call keeps the first call's samples"""
    luma, form = (40, 24, 60, 36), FORMS[1]
    cw, ch = csize(40, 24, 1, 1)
    ow, oh = csize(60, 36, 1, 1)
    u, v = rand8(1, luma, form, 1), rand8(1, luma, form, 2)
    wu, wv = want(u, luma, form)[0], want(v, luma, form)[0]
    for first in (0, 1):
        d_dst = torch.full((oh * 2 * ow + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        for p in ((0, 1) if first == 0 else (1, 0)):
            src = torch.from_numpy(np.ascontiguousarray((u, v)[p][0])).cuda()
            gpu.chroma_resize_u8_device(src.data_ptr(), 1, cw * ch, cw, 1, cw, ch, d_dst.data_ptr() + 32 + p, 0, 2 * ow, 2, ow, oh, 40, 24, 60, 36, 1, 1, form[2],
                                        stream=stream().cuda_stream)
        stream().synchronize()
        got = d_dst.cpu().numpy()
        body = got[32:32 + oh * 2 * ow].reshape(oh, ow, 2)
        assert np.array_equal(body[:, :, 0], wu) and np.array_equal(body[:, :, 1], wv), first
        assert (got[:32] == 0xAB).all() and (got[32 + oh * 2 * ow:] == 0xAB).all()
    # words: the pair store of an aligned P010 destination is the frame calls' path; one plane per call takes the 16-bit stores
    u16, v16 = rand16(1, luma, form, 10, 3), rand16(1, luma, form, 10, 4)
    d_dst = to_dev(np.full(oh * 2 * ow + 64, FILL, np.uint16))
    for p in (1, 0):
        src = to_dev(y16.pack_words((u16, v16)[p][0], 10, 1))
        gpu.chroma_resize_u16_device(src.data_ptr(), 1, 2 * cw * ch, 2 * cw, 1, 1, cw, ch, 10, d_dst.data_ptr() + 2 * (32 + p), 0, 4 * ow, 2, 1, ow, oh, 40, 24, 60, 36, 1, 1,
                                     form[2], stream=stream().cuda_stream)
    stream().synchronize()
    got = to_host(d_dst)
    body = y16.unpack(got[32:32 + oh * 2 * ow].reshape(oh, ow, 2), 10, 1)
    assert np.array_equal(body[:, :, 0], want(u16, luma, form, 10)[0]) and np.array_equal(body[:, :, 1], want(v16, luma, form, 10)[0])
    assert (got[:32] == FILL).all() and (got[32 + oh * 2 * ow:] == FILL).all()


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_resize_constants_of_every_value_extremes_and_overshoot(gpu, depth):
    """a constant plane of EVERY value comes back as that value (one tiny plane per value: at depth 16 that is 65536 turns for 2048 workgroups); the two
    extremes; a checkerboard and stripes of 0 / M overshoot past both clamps and saturate"""
    M = y16.maxval(depth)
    luma, form = (4, 4, 6, 5), FORMS[1]          # chroma 2 x 2 -> 3 x 3
    consts = np.arange(M + 1).astype(np.uint16)
    planes = np.repeat(consts, 4).reshape(-1, 2, 2)
    got = resize16(gpu, planes, depth, luma, form, salign=4, dalign=4, dpack=1)
    assert np.array_equal(got, np.repeat(consts, 9).reshape(-1, 3, 3))
    if depth == 8:
        assert np.array_equal(resize8(gpu, planes.astype(np.uint8), luma, form), np.repeat(consts, 9).reshape(-1, 3, 3))
    luma = (134, 70, 200, 158)
    for form in (FORMS[0], FORMS[2]):
        cw, ch = csize(134, 70, 1, 1)
        board = (np.indices((ch, cw)).sum(0) % 2 * M).astype(np.uint16)
        stripes = np.zeros((ch, cw), np.uint16)
        stripes[:, ::3] = M
        stripes[::4] = M
        planes = np.stack([board, M - board, stripes, np.zeros_like(board), np.full_like(board, M)])
        w_ = want(planes, luma, form, depth)
        assert w_.min() == 0 and w_.max() == M and (w_[3] == 0).all() and (w_[4] == M).all()
        pre = zr.resize_cubic(stripes.astype(np.float32) * np.float32(1.0 / M), w_.shape[2], w_.shape[1], 134, 70, 200, 158, 0.5, 0.5)
        assert pre.min() < -0.05 and pre.max() > 1.05, "the overshoot the clamp is there for"
        assert np.array_equal(resize16(gpu, planes, depth, luma, form, salign=4, dalign=4), w_)
        if depth == 8:
            assert np.array_equal(resize8(gpu, planes.astype(np.uint8), luma, form, src_aligned=True), w_)


def test_resize_more_turns_than_workgroups(gpu):
    """the grid-stride loop's second trip: one tall thin plane of 1 x 2049 tiles for 2048 workgroups, at 3 / 2"""
    c = zr.SECOND_TRIP
    turns, grid = zr.launch(c["ow"], c["oh"], c["n"])
    assert turns > grid == zr.GRID_MAX
    out_w, out_h = 2 * c["ow"], 2 * c["oh"]
    luma = (math.ceil(out_w / 1.5), math.ceil(out_h / 1.5), out_w, out_h)
    form = FORMS[2]
    values = rand16(c["n"], luma, form, 10, 21)
    assert np.array_equal(resize16(gpu, values, 10, luma, form, salign=4, dalign=4, dpack=1), want(values, luma, form, 10))
    planes = (values >> 2).astype(np.uint8)
    assert np.array_equal(resize8(gpu, planes, luma, FORMS[1]), want(planes, luma, FORMS[1]))
