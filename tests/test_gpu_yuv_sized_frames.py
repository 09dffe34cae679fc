"""GPU tests of the sized YUV frame calls (w2xc_process_frames_yuv_u8[_rgb]_sized[_device], w2xc_process_frames_yuv_u16[_rgb]_sized[_device]; include/w2xc_hip.h,
"Sized YUV frames"): equality of bytes and words with the routes the header defines the calls as, composed from public calls with the same options -- the luma
blocks, w2xc_convert_batch_device once per 2x step, w2xc_resize_linear_device per plane and w2xc_chroma_resize_u8_device / _u16_device per chroma plane for the Y
calls; w2xc_yuv8_to_rgb_device / w2xc_yuv16_to_rgb_device, w2xc_convert_planes_batch_device / w2xc_convert_planes_up2x_batch_device once per step,
w2xc_resize_linear_device per plane, w2xc_rgb_to_yuv8_device / w2xc_rgb_to_yuv16_device for the RGB calls -- and, where iterations <= 1 and the output is the
last level, with the base calls.  Frames of at most 48 x 40 in, 144 x 96 out."""
import os

import numpy as np
import pytest

from conftest import small_layers
from tools import gen_model
import fp32_matrix as fm
import yuv_ref as yr
import yuv_rgb_ref as rr
import yuv16_ref as y16
import yuv_sited_ref as sr
import yuv_sized_ref as zr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_yuv16_frames as f16   # noqa: E402
import test_gpu_yuv_sited_frames as fs   # noqa: E402
from test_gpu_yuv_blocks import stream   # noqa: E402
from test_gpu_yuv_rgb_blocks import NV12, NV21, PLANAR   # noqa: E402
from test_gpu_yuv16_blocks import to_dev, to_host   # noqa: E402
from test_yuv16_api import stream16   # noqa: E402

models = f16.models          # the fixture: "y3" / "y7" Y models, "3" 3-32-3 models, "7" a deep three-plane chain, "head" a head model
FAMILIES, FAMILY_IDS, DEPTH = fs.FAMILIES, fs.FAMILY_IDS, fs.DEPTH
frames, side, upload, download, same, pick = fs.frames, fs.side, fs.upload, fs.download, fs.same, fs.pick
AUTO = zr.ITERATIONS_AUTO
# (w, h, out_w, out_h, iterations): one step with a shrink, two without one, two with an anamorphic one, and the same sizes with AUTO
SHRINK1, TWO, ANAMORPHIC = (48, 40, 72, 60, 1), (24, 20, 96, 80, 2), (36, 24, 96, 54, 2)
LAYOUTS = (yr.YUV_420, sr.YUV_420_LEFT, sr.YUV_420_TOPLEFT, yr.YUV_422, sr.YUV_422_LEFT, yr.YUV_444)
LAYOUT_IDS = ["420", "420left", "420topleft", "422", "422left", "444"]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def resolved(w, h, out_w, out_h, it):
    return zr.auto_iterations(w, h, out_w, out_h) if it == AUTO else it


# ---- the references: the routes of the header, from public calls on tight planes ----
def shrink(gpu, d, sw, sh, dw, dh):
    """w2xc_resize_linear_device on every plane of d (..., sh, sw) -> (..., dh, dw); d itself where the sizes agree"""
    if (sw, sh) == (dw, dh):
        return d
    lead = d.shape[:-2]
    src = d.reshape(-1, sh, sw)
    dst = torch.empty((src.shape[0], dh, dw), dtype=torch.float32, device="cuda")
    for p in range(src.shape[0]):
        gpu.resize_linear_device(src[p].data_ptr(), sw, sh, dst[p].data_ptr(), dw, dh, stream=stream().cuda_stream)
    return dst.reshape(*lead, dh, dw)


def composed_y(gpu, bits, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, opts=None):
    n, h, w = Y.shape
    st, D = stream().cuda_stream, DEPTH[bits]
    d_y = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    if bits == 8:
        d_b = torch.from_numpy(Y).cuda()
        gpu.y8_to_plane_device(d_b.data_ptr(), n, w * h, w, w, h, rng, d_y.data_ptr(), 4 * w * h, stream=st)
    else:
        d_b = to_dev(Y)
        gpu.y16_to_plane_device(d_b.data_ptr(), n, 2 * w * h, 2 * w, w, h, rng, D, y16.LOW, d_y.data_ptr(), 4 * w * h, stream=st)
    if noise is not None:
        d_n = torch.empty_like(d_y)
        noise.convert_batch_device(n, d_y.data_ptr(), 4 * w * h, 4 * w, w, h, d_n.data_ptr(), 4 * w * h, 4 * w, nn2x=False, stream=st, opts=opts)
        d_y = d_n
    lw, lh = w, h
    for _ in range(it):
        d_s = torch.empty((n, 2 * lh, 2 * lw), dtype=torch.float32, device="cuda")
        scale.convert_batch_device(n, d_y.data_ptr(), 4 * lw * lh, 4 * lw, lw, lh, d_s.data_ptr(), 16 * lw * lh, 8 * lw, nn2x=True, stream=st, opts=opts)
        d_y, lw, lh = d_s, 2 * lw, 2 * lh
    d_y = shrink(gpu, d_y, lw, lh, out_w, out_h)
    if bits == 8:
        d_o = torch.zeros((n, out_h, out_w), dtype=torch.uint8, device="cuda")
        gpu.plane_to_y8_device(d_y.data_ptr(), n, 4 * out_w * out_h, out_w, out_h, rng, d_o.data_ptr(), out_w * out_h, out_w, stream=st)
    else:
        d_o = to_dev(np.zeros((n, out_h, out_w), np.uint16))
        gpu.plane_to_y16_device(d_y.data_ptr(), n, 4 * out_w * out_h, out_w, out_h, rng, D, y16.LOW, d_o.data_ptr(), 2 * out_w * out_h, 2 * out_w, stream=st)
    stream().synchronize()
    oy = d_o.cpu().numpy() if bits == 8 else to_host(d_o)
    cw, ch = sr.chroma_size(w, h, chroma)
    ocw, och = sr.chroma_size(out_w, out_h, chroma)
    sx, sy = zr.subsampling(chroma)
    out = []
    for P in (U, V):
        if bits == 8:
            d_c, d_u = torch.from_numpy(P).cuda(), torch.zeros((n, och, ocw), dtype=torch.uint8, device="cuda")
            gpu.chroma_resize_u8_device(d_c.data_ptr(), n, cw * ch, cw, 1, cw, ch, d_u.data_ptr(), ocw * och, ocw, 1, ocw, och, w, h, out_w, out_h, sx, sy, chroma & 0x30,
                                        stream=st)
            stream().synchronize()
            out.append(d_u.cpu().numpy())
        else:
            d_c, d_u = to_dev(P), to_dev(np.zeros((n, och, ocw), np.uint16))
            gpu.chroma_resize_u16_device(d_c.data_ptr(), n, 2 * cw * ch, 2 * cw, 1, y16.LOW, cw, ch, D, d_u.data_ptr(), 2 * ocw * och, 2 * ocw, 1, y16.LOW, ocw, och, w, h,
                                         out_w, out_h, sx, sy, chroma & 0x30, stream=st)
            stream().synchronize()
            out.append(to_host(d_u))
    return oy, out[0], out[1]


def composed_rgb(gpu, bits, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, matrix, opts=None):
    n, h, w = Y.shape
    st, D = stream().cuda_stream, DEPTH[bits]
    src = upload(side(gpu, bits, n, w, h, chroma), bits, Y, U, V)
    d = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    if bits == 8:
        gpu.yuv8_to_rgb_device(src.s, n, w, h, chroma, rng, matrix, d.data_ptr(), 12 * w * h, 4 * w * h, stream=st)
    else:
        gpu.yuv16_to_rgb_device(src.s, n, w, h, chroma, rng, D, matrix, d.data_ptr(), 12 * w * h, 4 * w * h, stream=st)
    if noise is not None:
        d_n = torch.empty_like(d)
        noise.convert_planes_batch_device(n, 3, d.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, d_n.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, nn2x=False, stream=st,
                                          opts=opts)
        d = d_n
    lw, lh = w, h
    for _ in range(it):
        W, H = 2 * lw, 2 * lh
        d_s = torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda")
        if scale.has_head:
            scale.convert_planes_up2x_batch_device(n, 3, d.data_ptr(), 12 * lw * lh, 4 * lw * lh, 4 * lw, lw, lh, d_s.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, stream=st,
                                                   opts=opts)
        else:
            scale.convert_planes_batch_device(n, 3, d.data_ptr(), 12 * lw * lh, 4 * lw * lh, 4 * lw, lw, lh, d_s.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, nn2x=True,
                                              stream=st, opts=opts)
        d, lw, lh = d_s, W, H
    d = shrink(gpu, d, lw, lh, out_w, out_h)
    dst = side(gpu, bits, n, out_w, out_h, chroma)
    if bits == 8:
        gpu.rgb_to_yuv8_device(d.data_ptr(), 12 * out_w * out_h, 4 * out_w * out_h, n, out_w, out_h, chroma, rng, matrix, dst.s, stream=st)
    else:
        gpu.rgb_to_yuv16_device(d.data_ptr(), 12 * out_w * out_h, 4 * out_w * out_h, n, out_w, out_h, chroma, rng, D, matrix, dst.s, stream=st)
    stream().synchronize()
    return download(dst, bits)


def composed(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, opts=None, matrix=rr.BT709):
    it = resolved(Y.shape[2], Y.shape[1], out_w, out_h, it)
    if rgb:
        return composed_rgb(gpu, bits, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, matrix, opts)
    return composed_y(gpu, bits, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, opts)


def call_sized(gpu, bits, rgb, n, w, h, chroma, i, out_w, out_h, o, noise, scale, it, rng, matrix, opts):
    st = stream().cuda_stream
    if bits == 8 and rgb:
        gpu.process_frames_yuv_u8_rgb_sized_device(n, w, h, chroma, i.s, out_w, out_h, o.s, noise, scale, it, rng, matrix, stream=st, opts=opts)
    elif bits == 8:
        gpu.process_frames_yuv_u8_sized_device(n, w, h, chroma, i.s, out_w, out_h, o.s, noise, scale, it, rng, stream=st, opts=opts)
    elif rgb:
        gpu.process_frames_yuv_u16_rgb_sized_device(n, w, h, chroma, i.s, out_w, out_h, o.s, noise, scale, it, rng, matrix, stream=st, opts=opts, depth=DEPTH[bits])
    else:
        gpu.process_frames_yuv_u16_sized_device(n, w, h, chroma, i.s, out_w, out_h, o.s, noise, scale, it, rng, stream=st, opts=opts, depth=DEPTH[bits])


def run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, opts=None, matrix=rr.BT709, in_kind=PLANAR, out_kind=PLANAR, aligned=False):
    """the sized frame call on planes with rims"""
    n, h, w = Y.shape
    i = upload(side(gpu, bits, n, w, h, chroma, in_kind, aligned), bits, Y, U, V)
    o = side(gpu, bits, n, out_w, out_h, chroma, out_kind, aligned)
    call_sized(gpu, bits, rgb, n, w, h, chroma, i, out_w, out_h, o, noise, scale, it, rng, matrix, opts)
    stream().synchronize()
    return download(o, bits)      # (checks the rims)


# ---- the four families against their composed routes ----
@pytest.mark.parametrize("case", [SHRINK1, TWO, ANAMORPHIC, SHRINK1[:4] + (AUTO,), ANAMORPHIC[:4] + (AUTO,)], ids=["1-shrink", "2", "2-anamorphic", "auto-1", "auto-2"])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_sized_call_is_its_composed_route(gpu, models, family, case):
    """n = 3 on every kind of side, scale and noise_scale, and n = 1"""
    bits, rgb = family
    w, h, out_w, out_h, it = case
    noise, scale = pick(models, rgb)
    chroma = sr.YUV_420_LEFT
    Y, U, V = frames(bits, 3, w, h, chroma, 10 + w)
    want = composed(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED)
    assert want[0].shape == (3, out_h, out_w) and want[1].shape == (3,) + sr.chroma_size(out_w, out_h, chroma)[::-1]
    for k, (ik, ok) in enumerate(((PLANAR, PLANAR), (NV12, NV12), (NV21, PLANAR))):
        assert same(run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED, in_kind=ik, out_kind=ok, aligned=bool(k & 1)), want), (ik, ok)
    one = run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y[1:2], U[1:2], V[1:2], chroma, yr.LIMITED)
    assert same(one, tuple(a[1:2] for a in want)), "n = 1: frame 1 alone has the samples it has in the batch"
    want_s = composed(gpu, bits, rgb, None, scale, it, out_w, out_h, Y, U, V, chroma, yr.FULL)
    assert same(run_sized(gpu, bits, rgb, None, scale, it, out_w, out_h, Y, U, V, chroma, yr.FULL, out_kind=NV12, aligned=True), want_s), "scale alone"
    if not rgb:
        assert np.array_equal(want_s[1], want[1]) and np.array_equal(want_s[2], want[2]), "chroma does not depend on the models or the range"


@pytest.mark.parametrize("chroma", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_sitings_ranges_and_matrices(gpu, models, family, chroma):
    """every siting the layouts take, both ranges, three matrices, odd sizes on both sides; the noise pass alone at the input's size"""
    bits, rgb = family
    noise, scale = pick(models, rgb)
    k = LAYOUTS.index(chroma)
    for j, (w, h, out_w, out_h, it) in enumerate(((37, 21, 55, 33, 1), (21, 13, 75, 41, 2))):
        Y, U, V = frames(bits, 2, w, h, chroma, 20 + k)
        rng, matrix = (yr.FULL, yr.LIMITED)[(k + j) & 1], rr.MATRICES[(k + j) % 3]
        want = composed(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, matrix=matrix)
        assert same(run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, rng, matrix=matrix, in_kind=(PLANAR, NV12)[j], out_kind=(NV12, PLANAR)[j]), want)
    Y, U, V = frames(bits, 2, 37, 21, chroma, 30 + k)
    for it in (0, AUTO):
        want0 = composed(gpu, bits, rgb, noise, None, it, 37, 21, Y, U, V, chroma, yr.LIMITED)
        assert same(run_sized(gpu, bits, rgb, noise, None, it, 37, 21, Y, U, V, chroma, yr.LIMITED), want0)
        if not rgb:
            assert np.array_equal(want0[1], U) and np.array_equal(want0[2], V), "r = 1: chroma is copied"


@pytest.mark.parametrize("bits", [8, 16])
def test_head_model_deep_models_and_grey_frames(gpu, models, bits):
    _, head = models["head"]
    chroma = sr.YUV_420_TOPLEFT
    Y, U, V = frames(bits, 3, 20, 12, chroma, 50)
    for out_w, out_h, it in ((70, 40, 2), (30, 20, AUTO), (80, 48, 2)):
        want = composed(gpu, bits, True, None, head, it, out_w, out_h, Y, U, V, chroma, yr.FULL, matrix=rr.BT2020)
        assert same(run_sized(gpu, bits, True, None, head, it, out_w, out_h, Y, U, V, chroma, yr.FULL, matrix=rr.BT2020, out_kind=NV12, aligned=True), want)
    for deep, rgb in (("y7", False), ("7", True)):       # the 7-layer chains
        nd, sd = models[deep]
        Y, U, V = frames(bits, 2, 36, 24, yr.YUV_420, 51)
        want = composed(gpu, bits, rgb, nd, sd, 2, 96, 54, Y, U, V, yr.YUV_420, yr.LIMITED)
        assert same(run_sized(gpu, bits, rgb, nd, sd, 2, 96, 54, Y, U, V, yr.YUV_420, yr.LIMITED, in_kind=NV12, out_kind=NV12, aligned=True), want)
    # W2XC_YUV_400 through the Y call (the host form): luma alone
    noise, scale = models["y3"]
    Y, U, V = frames(bits, 2, 36, 24, yr.YUV_420, 52)
    host = gpu.process_frames_yuv_u8_sized if bits == 8 else gpu.process_frames_yuv_u16_sized
    got = host(Y, 96, 54, chroma=yr.YUV_400, noise=noise, scale=scale, iterations=2, range=gpu.RANGE_LIMITED, **(dict(depth=DEPTH[bits]) if bits == 16 else {}))
    assert len(got) == 1 and np.array_equal(got[0], composed(gpu, bits, False, noise, scale, 2, 96, 54, Y, U, V, yr.YUV_420, yr.LIMITED)[0])


@pytest.mark.parametrize("kw", [dict(fusion=1), dict(band_rows=16), dict(precision=4)], ids=["fusion_off", "band_rows_16", "fp16x2"])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_option_sets(gpu, models, family, kw):
    """W2XC_FUSION_OFF at n = 3; a band_rows that cuts every level's planes at n = 1; a split precision: both sides run the same passes"""
    bits, rgb = family
    noise, scale = pick(models, rgb, "7" if rgb else "y7")
    opts = gpu.make_opts(**kw)
    n = 1 if "band_rows" in kw else 3
    w, h, out_w, out_h, it = ANAMORPHIC
    for chroma in (yr.YUV_420, sr.YUV_420_TOPLEFT):
        Y, U, V = frames(bits, n, w, h, chroma, 70)
        want = composed(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED, opts=opts)
        assert same(run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED, opts=opts, in_kind=NV12, aligned=True), want), hex(chroma)


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_poisoned_scratch(gpu, models, family):
    bits, rgb = family
    noise, scale = pick(models, rgb, "7" if rgb else "y7")
    chroma = sr.YUV_420_LEFT
    w, h, out_w, out_h, it = ANAMORPHIC
    Y, U, V = frames(bits, 3, w, h, chroma, 80)
    want = composed(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED)
    assert same(run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED), want)     # (the contexts and their buffers exist now)
    for word in (0x7FC00000, 0x7149F2CA):
        assert noise.fill_scratch(word) > 0 and scale.fill_scratch(word) > 0
        assert same(run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED), want)


def count(names, what):
    return sum(1 for n in names if what in n)


def two_frame_opts(gpu, rgb, scale, w, h):
    """a workspace_mb under which the batched chain of the LAST scale pass (its source w x h) takes two frames at a time"""
    for mb in range(1, 4096):
        o = gpu.make_opts(workspace_mb=mb)
        ok, sub = scale.batch_plan(3 if rgb else 1, w, h, nn2x=True, opts=o)
        if ok and sub == 2:
            return o
        assert not ok or sub < 2, "no budget gives a sub-batch of 2"
    raise AssertionError("no budget found")


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_sub_batches_and_launch_lists(gpu, models, family):
    """n = 3 whole and as 2 + 1 (workspace_mb): the same samples; per sub-batch ONE chroma launch (Y route: the resize kernel; RGB route: one launch of each end)
    and ONE linear-resize launch, none where the output is the last level; and the passes between are the layer launches of two scale passes"""
    bits, rgb = family
    _, scale = pick(models, rgb, "7" if rgb else "y7")
    w, h, out_w, out_h, it = ANAMORPHIC
    n, chroma, tag = 3, sr.YUV_420_LEFT, ("8" if bits == 8 else "16")
    small = two_frame_opts(gpu, rgb, scale, 2 * w, 2 * h)
    Y, U, V = frames(bits, n, w, h, chroma, 61)
    want = composed(gpu, bits, rgb, None, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED)
    assert same(run_sized(gpu, bits, rgb, None, scale, it, out_w, out_h, Y, U, V, chroma, yr.LIMITED, opts=small, out_kind=NV12), want), "sub-batches of 2 + 1 change no sample"
    i = upload(side(gpu, bits, n, w, h, chroma), bits, Y, U, V)
    ends = ("k_yuv%s_to_rgb" % tag, "k_rgb_to_yuv%s" % tag) if rgb else ("k_chroma_resize_u%s" % tag,)
    convs = {}
    for ow, oh in ((out_w, out_h), (4 * w, 4 * h)):
        o = side(gpu, bits, n, ow, oh, chroma, NV12, True)
        for opts, subs in ((None, 1), (small, 2)):
            run = lambda: call_sized(gpu, bits, rgb, n, w, h, chroma, i, ow, oh, o, None, scale, it, yr.LIMITED, rr.BT709, opts)
            run()
            stream().synchronize()
            names = fm.kernel_names(run)
            convs[(ow, subs)] = [k for k in names if fm.is_fp32_conv(k)]
            for k in ends:
                assert count(names, k) == subs, (k, subs, names)
            assert count(names, "ResizeLinear") == (subs if (ow, oh) != (4 * w, 4 * h) else 0), names
            assert count(names, "k_chroma2x") == 0 and count(names, "ChromaCopy") == 0, names
    for subs in (1, 2):
        assert convs[(out_w, subs)] == convs[(4 * w, subs)] and convs[(out_w, subs)], "the CNN between the ends does not know the output size"


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_host_form_equals_device_form(gpu, models, family):
    bits, rgb = family
    noise, scale = pick(models, rgb)
    host = {(8, False): gpu.process_frames_yuv_u8_sized, (8, True): gpu.process_frames_yuv_u8_rgb_sized, (16, False): gpu.process_frames_yuv_u16_sized,
            (16, True): gpu.process_frames_yuv_u16_rgb_sized}[family]
    chroma = sr.YUV_420_LEFT
    w, h, out_w, out_h, it = ANAMORPHIC
    kw = dict(chroma=chroma, noise=noise, scale=scale, range=gpu.RANGE_FULL)
    kw.update(dict(matrix=rr.BT709) if rgb else {})
    kw.update(dict(depth=DEPTH[bits]) if bits == 16 else {})
    Y, U, V = frames(bits, 3, w, h, chroma, 90)
    want = run_sized(gpu, bits, rgb, noise, scale, it, out_w, out_h, Y, U, V, chroma, yr.FULL)
    assert same(host(Y, out_w, out_h, U, V, iterations=it, **kw), want)
    assert same(host(Y, out_w, out_h, U, V, **kw), want), "ITERATIONS_AUTO is the wrappers' default"
    if bits == 8:      # NV12 host planes in and out
        oy, ouv = host(Y, out_w, out_h, uv=np.stack([U, V], axis=-1), **kw)
        assert same((oy, np.ascontiguousarray(ouv[..., 0]), np.ascontiguousarray(ouv[..., 1])), want)
    else:              # P010 host planes in and out: high-packed words, interleaved chroma
        oy, ouv = host(Y << 6, out_w, out_h, uv=np.stack([U, V], axis=-1) << 6, pack=gpu.PACK_HIGH, **kw)
        assert same((oy >> 6, np.ascontiguousarray(ouv[..., 0]) >> 6, np.ascontiguousarray(ouv[..., 1]) >> 6), want)
        assert ((oy & 63) == 0).all() and ((ouv & 63) == 0).all()
    nd, sd = models["7" if rgb else "y7"]                      # (the 7-layer chains: a workspace budget exists under which they take two frames at a time)
    small = two_frame_opts(gpu, rgb, sd, 2 * w, 2 * h)         # sub-batches of 2 + 1: the second upload goes where the first frames were
    kw.update(noise=nd, scale=sd)
    assert same(host(Y, out_w, out_h, U, V, opts=small, **kw), run_sized(gpu, bits, rgb, nd, sd, it, out_w, out_h, Y, U, V, chroma, yr.FULL))


# ---- the anchor ----
@pytest.mark.parametrize("chroma", [yr.YUV_420, sr.YUV_420_TOPLEFT, yr.YUV_444], ids=["420", "420topleft", "444"])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_last_level_output_is_the_base_call(gpu, models, family, chroma):
    """iterations <= 1 with (out_w, out_h) = (W, H): byte for byte the base call, whose chroma kernels the engine runs there; the composed route through the
    resize block gives those samples too"""
    bits, rgb = family
    noise, scale = pick(models, rgb)
    w, h = 17, 33
    Y, U, V = frames(bits, 3, w, h, chroma, 99)
    for it, mode_scale in ((1, scale), (0, None)):
        base = fs.run_device(gpu, bits, rgb, noise, mode_scale, it, Y, U, V, chroma, yr.LIMITED, out_kind=NV12)
        for its in (it, AUTO):
            assert same(run_sized(gpu, bits, rgb, noise, mode_scale, its, w << it, h << it, Y, U, V, chroma, yr.LIMITED, out_kind=NV12), base), (it, its)
        assert same(composed(gpu, bits, rgb, noise, mode_scale, it, w << it, h << it, Y, U, V, chroma, yr.LIMITED), base)
    # (w, h) with a scale step taken: luma shrunk back, chroma copied
    got = run_sized(gpu, bits, rgb, noise, scale, 1, w, h, Y, U, V, chroma, yr.LIMITED)
    assert same(got, composed(gpu, bits, rgb, noise, scale, 1, w, h, Y, U, V, chroma, yr.LIMITED))
    if not rgb:
        assert np.array_equal(got[1], U) and np.array_equal(got[2], V)
    # exactly 2x behind two steps: the 2x chroma kernels' samples
    got = run_sized(gpu, bits, rgb, None, scale, 2, 2 * w, 2 * h, Y, U, V, chroma, yr.LIMITED)
    assert same(got, composed(gpu, bits, rgb, None, scale, 2, 2 * w, 2 * h, Y, U, V, chroma, yr.LIMITED))


# ---- the tools ----
def test_y4m_tools_with_size(gpu, models_dir, tmp_path):
    """--size and --scale_ratio on both tools, end to end: the sized call's samples, W and H of the written header"""
    y4m, y4m16 = fs.load_tool("w2xc_y4m"), fs.load_tool("w2xc_y4m16")
    noise = gpu._ModelSet.from_json(os.path.join(models_dir, "noise1_model.json"))
    scale = gpu._ModelSet.from_json(os.path.join(models_dir, "scale2.0x_model.json"))
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    data, fr = yr.y4m_stream(36, 24, "420mpeg2", 3, seed=95, extra=b"F24:1 Ip A1:1 XCOLORRANGE=FULL")
    src.write_bytes(data)
    Y, U, V = (np.stack([f[k] for f in fr]) for k in range(3))
    for extra, (ow, oh) in ((["--size", "96x54"], (96, 54)), (["--scale_ratio", "1.5"], (54, 36)), (["--size", "72x48"], (72, 48))):
        assert y4m.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--frames_per_call", "2", "--siting", "auto"] + extra) == 0
        want = gpu.process_frames_yuv_u8_sized(Y, ow, oh, U, V, chroma=sr.YUV_420_LEFT, noise=noise, scale=scale, range=gpu.RANGE_FULL)
        with open(dst, "rb") as f:
            hdr = y4m.read_header(f)
            assert (hdr.w, hdr.h) == (ow, oh) and hdr.get("C") == "420mpeg2" and hdr.get("F") == "24:1"
            assert same(y4m.read_frames(f, hdr, 10), want), extra
            assert f.read() == b""
    assert same(want, gpu.process_frames_yuv_u8(Y, U, V, chroma=sr.YUV_420_LEFT, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_FULL)), "72x48 is the 2x call"
    # three-plane models: the RGB call
    gen_model.write_json(small_layers([3, 32, 3], 31), str(tmp_path / "noise1_model.json"))
    gen_model.write_json(small_layers([3, 32, 3], 32), str(tmp_path / "scale2.0x_model.json"))
    n3, s3 = gpu._ModelSet.from_json(str(tmp_path / "noise1_model.json")), gpu._ModelSet.from_json(str(tmp_path / "scale2.0x_model.json"))
    assert y4m.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path), "--size", "96x54"]) == 0
    want = gpu.process_frames_yuv_u8_rgb_sized(Y, 96, 54, U, V, chroma=yr.YUV_420, scale=s3, range=gpu.RANGE_FULL, matrix=gpu.MATRIX_BT601)
    with open(dst, "rb") as f:
        assert same(y4m.read_frames(f, y4m.read_header(f), 10), want)
    # words
    data, fr, _ = stream16(36, 24, "420", 10, 3, seed=96, extra=b"F24:1 Ip A1:1 XCOLORRANGE=FULL")
    src.write_bytes(data)
    Y, U, V = (np.stack([f[k] for f in fr]) for k in range(3))
    assert y4m16.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--frames_per_call", "2", "--siting", "left", "--size", "96x54"]) == 0
    want = gpu.process_frames_yuv_u16_sized(Y, 96, 54, U, V, chroma=sr.YUV_420_LEFT, noise=noise, scale=scale, range=gpu.RANGE_FULL, depth=10)
    with open(dst, "rb") as f:
        hdr = y4m16.y4m.read_header(f)
        assert (hdr.w, hdr.h) == (96, 54) and hdr.get("C") == "420p10"
        assert same(y4m16.read_frames(f, hdr, 10), want)
    assert y4m16.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path), "--scale_ratio", "2.25"]) == 0
    want = gpu.process_frames_yuv_u16_rgb_sized(Y, 81, 54, U, V, chroma=yr.YUV_420, scale=s3, iterations=2, range=gpu.RANGE_FULL, matrix=gpu.MATRIX_BT601, depth=10)
    with open(dst, "rb") as f:
        hdr = y4m16.y4m.read_header(f)
        assert (hdr.w, hdr.h) == (81, 54)
        assert same(y4m16.read_frames(f, hdr, 10), want)
