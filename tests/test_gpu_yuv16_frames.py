"""GPU tests of the 16-bit YUV frame calls (w2xc_process_frames_yuv_u16[_device], w2xc_process_frames_yuv_u16_rgb[_device]): equality of words with the routes
the header defines the calls as, composed from public calls with the same options -- w2xc_y16_to_plane_device, w2xc_convert_batch_device (nn2x = 0, then 1),
w2xc_plane_to_y16_device and w2xc_chroma2x_u16_device per chroma plane for the Y call; w2xc_yuv16_to_rgb_device, w2xc_convert_planes_batch_device /
w2xc_convert_planes_up2x_batch_device, w2xc_rgb_to_yuv16_device for the RGB call -- over the modes, planar and P010 on either side with the packings
differing, depths 10 and 16, both ranges, the layouts, sub-batches, option sets, poisoned scratch, the host form, the launch list, the depth-8 anchor against
the 8-bit calls and the y4m16 tool.  Frames of at most 70 x 40."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, small_layers
from tools import gen_model
import fp32_matrix as fm
import yuv_ref as yr
import yuv_rgb_ref as rr
import yuv16_ref as y16
from test_gpu_yuv16_blocks import Side16, frames16, stream, to_dev, to_host
from test_yuv16_api import stream16

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEEP = [3, 32, 32, 64, 64, 128, 128, 3]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@pytest.fixture(scope="module")
def models(gpu):
    """(noise, scale) per kind: Y models -- a short chain and the 7-layer chain --, three-plane models -- 3-32-3, a 7-layer chain -- and a small head model"""
    ys = lambda seed: gpu._ModelSet.from_layers(small_layers([1, 32, 32, 1], seed))
    y7 = lambda name: gpu._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS[name]))
    short = lambda seed: gpu._ModelSet.from_layers(small_layers([3, 32, 3], seed))
    deep = lambda seed: gpu._ModelSet.from_layers(gen_model.synth_layers(DEEP, seed=seed))
    head_w = np.random.default_rng(8).standard_normal((64, 3, 4, 4)).astype(np.float32) * np.float32(0.05)
    head = gpu._ModelSet.from_layers(small_layers([3, 32, 32, 64, 64], 9), head=(head_w, None))
    noise3 = short(31)
    return {"y3": (ys(31), ys(32)), "y7": (y7("noise1"), y7("scale2.0x")), "3": (noise3, short(32)), "7": (deep(33), deep(34)), "head": (noise3, head)}


def is_rgb(which):
    return not which.startswith("y")


def pick(models, which, mode):
    noise, scale = models[which]
    return (noise if "noise" in mode else None), (scale if "scale" in mode else None), (1 if "scale" in mode else 0)


def frames(n, w, h, layout, depth, seed):
    Y, U, V = frames16(n, w, h, layout, depth, seed)
    return (Y, None, None) if layout == yr.YUV_400 else (Y, U, V)


# ---- the references: the routes of the header, from public calls on tight planes ----
def tight(values, depth, pack):
    return to_dev(y16.pack_words(values, depth, pack))


def composed_y(gpu, noise, scale, iterations, Y, U, V, layout, rng, depth, opts=None):
    """-> VALUES"""
    n, h, w = Y.shape
    st = stream().cuda_stream
    d_b = tight(Y, depth, y16.HIGH)
    d_y = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    gpu.y16_to_plane_device(d_b.data_ptr(), n, 2 * w * h, 2 * w, w, h, rng, depth, y16.HIGH, d_y.data_ptr(), 4 * w * h, stream=st)
    if noise is not None:
        d_n = torch.empty_like(d_y)
        noise.convert_batch_device(n, d_y.data_ptr(), 4 * w * h, 4 * w, w, h, d_n.data_ptr(), 4 * w * h, 4 * w, nn2x=False, stream=st, opts=opts)
        d_y = d_n
    W, H = w << iterations, h << iterations
    if iterations:
        d_s = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        scale.convert_batch_device(n, d_y.data_ptr(), 4 * w * h, 4 * w, w, h, d_s.data_ptr(), 4 * W * H, 4 * W, nn2x=True, stream=st, opts=opts)
        d_y = d_s
    d_o = to_dev(np.zeros((n, H, W), np.uint16))
    gpu.plane_to_y16_device(d_y.data_ptr(), n, 4 * W * H, W, H, rng, depth, y16.LOW, d_o.data_ptr(), 2 * W * H, 2 * W, stream=st)
    stream().synchronize()
    oy = to_host(d_o)
    if layout == yr.YUV_400:
        return oy, None, None
    if not iterations:
        return oy, U.copy(), V.copy()
    ocw, och = yr.out_chroma_size(w, h, layout)
    cw, ch = yr.chroma_size(w, h, layout)
    out = []
    for P in (U, V):
        d_c, d_u = tight(P, depth, y16.LOW), to_dev(np.zeros((n, och, ocw), np.uint16))
        gpu.chroma2x_u16_device(d_c.data_ptr(), n, 2 * cw * ch, 2 * cw, 1, y16.LOW, cw, ch, depth, d_u.data_ptr(), 2 * ocw * och, 2 * ocw, 1, y16.LOW, ocw, och, stream=st)
        stream().synchronize()
        out.append(to_host(d_u))
    return oy, out[0], out[1]


def composed_rgb(gpu, noise, scale, iterations, Y, U, V, layout, rng, depth, matrix, opts=None):
    n, h, w = Y.shape
    st = stream().cuda_stream
    src = Side16(gpu, n, w, h, layout).upload(Y, U, V, depth, junk=False)
    d = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    gpu.yuv16_to_rgb_device(src.s, n, w, h, layout, rng, depth, matrix, d.data_ptr(), 12 * w * h, 4 * w * h, stream=st)
    if noise is not None:
        d_n = torch.empty_like(d)
        noise.convert_planes_batch_device(n, 3, d.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, d_n.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, nn2x=False, stream=st,
                                          opts=opts)
        d = d_n
    W, H = w << iterations, h << iterations
    if iterations:
        d_s = torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda")
        if scale.has_head:
            scale.convert_planes_up2x_batch_device(n, 3, d.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, d_s.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, stream=st, opts=opts)
        else:
            scale.convert_planes_batch_device(n, 3, d.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, d_s.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, nn2x=True, stream=st,
                                              opts=opts)
        d = d_s
    dst = Side16(gpu, n, W, H, layout)
    gpu.rgb_to_yuv16_device(d.data_ptr(), 12 * W * H, 4 * W * H, n, W, H, layout, rng, depth, matrix, dst.s, stream=st)
    stream().synchronize()
    return dst.download(depth)


def composed(gpu, which, noise, scale, it, Y, U, V, layout, rng, depth, matrix=rr.BT2020, opts=None):
    if is_rgb(which):
        return composed_rgb(gpu, noise, scale, it, Y, U, V, layout, rng, depth, matrix, opts)
    return composed_y(gpu, noise, scale, it, Y, U, V, layout, rng, depth, opts)


def run_device(gpu, which, noise, scale, it, Y, U, V, layout, rng, depth, matrix=rr.BT2020, opts=None, i_style="planar", o_style="planar", i_pack=0, o_pack=0, align=1):
    """the frame call on planes with rims -> VALUES"""
    n, h, w = Y.shape
    i = Side16(gpu, n, w, h, layout, i_style, i_pack, align).upload(Y, U, V, depth)
    o = Side16(gpu, n, w << it, h << it, layout, o_style, o_pack, align)
    if is_rgb(which):
        gpu.process_frames_yuv_u16_rgb_device(n, w, h, layout, i.s, o.s, noise, scale, it, rng, matrix, stream=stream().cuda_stream, opts=opts, depth=depth)
    else:
        gpu.process_frames_yuv_u16_device(n, w, h, layout, i.s, o.s, noise, scale, it, rng, stream=stream().cuda_stream, opts=opts, depth=depth)
    stream().synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(i.download(depth, written=False), (Y, U, V)) if b is not None), "the input frames were written"
    return o.download(depth)


def same(got, want):
    assert len(got) == len(want) == 3
    for name, g, w_ in zip("YUV", got, want):
        assert (g is None) == (w_ is None), name
        if g is not None:
            assert g.shape == w_.shape and np.array_equal(g, w_), "%s: %d of %d words differ" % (name, int((g != w_).sum()), g.size)
    return True


# planar and P010 on either side, the packing differing between the sides
SIDE_CASES = [("planar", "planar", 0, 1), ("planar", "p010", 0, 1), ("p010", "planar", 1, 0), ("p010", "p010", 1, 0), ("vu", "p010", 1, 1)]
Y_LAYOUTS = [(17, 33, yr.YUV_420), (16, 32, yr.YUV_422), (16, 32, yr.YUV_444), (16, 32, yr.YUV_400)]


@pytest.mark.parametrize("depth", [10, 16])
@pytest.mark.parametrize("case", Y_LAYOUTS, ids=["420-17x33", "422-16x32", "444-16x32", "400-16x32"])
def test_y_call_layouts_sides_and_packings(gpu, models, case, depth):
    w, h, layout = case
    noise, scale, it = pick(models, "y7", "noise_scale")
    Y, U, V = frames(2, w, h, layout, depth, 40 + layout)
    want = composed(gpu, "y7", noise, scale, it, Y, U, V, layout, yr.LIMITED, depth)
    assert want[0].shape == (2, 2 * h, 2 * w) and (layout == yr.YUV_400 or want[1].shape == (2,) + yr.out_chroma_size(w, h, layout)[::-1])
    for k, (i_style, o_style, ip, op) in enumerate(SIDE_CASES if layout != yr.YUV_400 else SIDE_CASES[:1]):
        for align in ((1, 2, 4) if k < 4 else (2,)):
            assert same(run_device(gpu, "y7", noise, scale, it, Y, U, V, layout, yr.LIMITED, depth, None, None, i_style, o_style, ip, op, align), want), (i_style, o_style, align)


@pytest.mark.parametrize("depth", [10, 16])
@pytest.mark.parametrize("layout", rr.LAYOUTS, ids=["420", "422", "444"])
def test_rgb_call_layouts_sides_and_packings(gpu, models, layout, depth):
    w, h = 17, 33
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(2, w, h, layout, depth, 45 + layout)
    want = composed(gpu, "7", noise, scale, it, Y, U, V, layout, yr.LIMITED, depth)
    assert want[0].shape == (2, 2 * h, 2 * w) and want[1].shape == (2,) + yr.chroma_size(2 * w, 2 * h, layout)[::-1]
    for k, (i_style, o_style, ip, op) in enumerate(SIDE_CASES):
        for align in ((1, 2, 4) if k < 4 else (2,)):
            assert same(run_device(gpu, "7", noise, scale, it, Y, U, V, layout, yr.LIMITED, depth, rr.BT2020, None, i_style, o_style, ip, op, align), want), (i_style, o_style, align)


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("mode", ["noise", "scale", "noise_scale"])
@pytest.mark.parametrize("which", ["y3", "y7", "3", "7", "head"])
def test_modes_ranges_and_models(gpu, models, which, mode, rng):
    """mode noise is iterations = 0: on the Y route the chroma values are copied -- repacked, from planar planes into interleaved ones too"""
    noise, scale, it = pick(models, which, mode)
    depth = 10 if rng == yr.LIMITED else 16
    Y, U, V = frames(3, 17, 33, yr.YUV_420, depth, 50)
    want = composed(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, rng, depth)
    if it == 0 and not is_rgb(which):
        assert np.array_equal(want[1], U) and np.array_equal(want[2], V)
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, rng, depth), want)
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, rng, depth, o_style="p010", i_pack=0, o_pack=1, align=2), want)
    other = composed(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, 1 - rng, depth)
    assert not np.array_equal(other[0], want[0]), "the two ranges are two results"


@pytest.mark.parametrize("size", [(65, 33), (66, 34), (63, 31), (64, 32)], ids=lambda s: "%dx%d" % s)
def test_y_call_chroma_paths_around_a_tile(gpu, models, size):
    """the (U, V) pair loads and pair stores of the chroma kernel are reached through the frame call alone: chroma planes around one tile of quads, every
    combination of planar and interleaved sides at every alignment, against the single-plane block calls"""
    w, h = size
    noise, scale, it = pick(models, "y3", "scale")
    Y, U, V = frames(2, w, h, yr.YUV_420, 10, 46)
    want = composed(gpu, "y3", noise, scale, it, Y, U, V, yr.YUV_420, yr.FULL, 10)
    for i_style, o_style, ip, op in SIDE_CASES:
        for align in (1, 2, 4):
            assert same(run_device(gpu, "y3", noise, scale, it, Y, U, V, yr.YUV_420, yr.FULL, 10, None, None, i_style, o_style, ip, op, align), want), (i_style, o_style, align)


def sub_batch_opts(gpu, which, noise, scale, w, h, want_sub):
    """a workspace_mb under which the batched chains of the call's passes take want_sub frames at the least: the plan is host arithmetic (w2xc_batch_plan)"""
    planes = 3 if is_rgb(which) else 1
    for mb in range(1, 4096):
        o = gpu.make_opts(workspace_mb=mb)
        plans = [scale.batch_plan(planes, w, h, opts=o, up2x=True) if scale.has_head else scale.batch_plan(planes, w, h, nn2x=True, opts=o)]
        if noise is not None:
            plans.append(noise.batch_plan(planes, w, h, nn2x=False, opts=o))
        if not all(b for b, _ in plans):
            continue
        sub = min(s for _, s in plans)
        if sub == want_sub:
            return o
        assert sub < want_sub, "no budget gives a sub-batch of %d" % want_sub
    raise AssertionError("no budget found")


@pytest.mark.parametrize("which,w,h", [("y7", 17, 33), ("7", 17, 33), ("head", 40, 24)], ids=["y7-17x33", "7-17x33", "head-40x24"])
def test_frame_counts_and_sub_batches(gpu, models, which, w, h):
    noise, scale, it = pick(models, which, "noise_scale")
    noise = None if which == "head" else noise
    Y, U, V = frames(3, w, h, yr.YUV_420, 10, 60)
    want = composed(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10)
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10), want)
    one = run_device(gpu, which, noise, scale, it, Y[1:2], U[1:2], V[1:2], yr.YUV_420, yr.LIMITED, 10)
    assert same(one, tuple(a[1:2] for a in want)), "n = 1: frame 1 alone has the words it has in the batch"
    small = sub_batch_opts(gpu, which, noise, scale, w, h, 2)
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10, opts=small, o_style="p010", align=2),
                composed(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10, opts=small))
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10, opts=small), want), "sub-batches of 2 + 1 change no word"


def count(names, what):
    return sum(1 for n in names if what in n)


def test_launch_lists(gpu, models):
    """one of each new end per sub-batch, one launch per layer of the batched chain, and none of the 8-bit ends"""
    n, w, h = 3, 17, 33
    Y, U, V = frames(n, w, h, yr.YUV_420, 10, 61)
    for which, ends in (("y7", ("Y16ToPlane", "PlaneToY16", "k_chroma2x_u16")), ("7", ("k_yuv16_to_rgb", "k_rgb_to_yuv16"))):
        noise, scale, it = pick(models, which, "noise_scale")
        i = Side16(gpu, n, w, h, yr.YUV_420, "planar", 0, 4).upload(Y, U, V, 10)
        o = Side16(gpu, n, 2 * w, 2 * h, yr.YUV_420, "p010", 1, 2)
        for opts, subs in ((None, 1), (sub_batch_opts(gpu, which, noise, scale, w, h, 2), 2)):
            if is_rgb(which):
                run = lambda: gpu.process_frames_yuv_u16_rgb_device(n, w, h, yr.YUV_420, i.s, o.s, noise, scale, it, yr.LIMITED, rr.BT2020, stream=stream().cuda_stream,
                                                                    opts=opts, depth=10)
            else:
                run = lambda: gpu.process_frames_yuv_u16_device(n, w, h, yr.YUV_420, i.s, o.s, noise, scale, it, yr.LIMITED, stream=stream().cuda_stream, opts=opts, depth=10)
            run()
            stream().synchronize()
            names = fm.kernel_names(run)
            for end in ends:
                assert count(names, end) == subs, (end, names)
            for stage in ("Y8ToPlane", "PlaneToY8", "k_chroma2x_u8", "k_yuv8_to_rgb", "k_rgb_to_yuv8", "U8ToYuv", "YuvToU8", "Resize2xCubic", "U8ToRgb", "RgbToU8",
                          "ChromaCopy"):
                assert count(names, stage) == 0, (stage, names)
            # the passes between the ends are those of the 8-bit calls: the batch kernels, once per layer launch (layers 1 + 2 fused, the last layer in its
            # gather); on the RGB route the remainder of one frame behind a sub-batch of two is the single-image sequence
            conv = [k for k in names if fm.is_fp32_conv(k)]
            per_pass = [sum(1 for l in range(m.n_layers) if not m.kernel_name(l).startswith("(")) for m in (noise, scale)]
            if not is_rgb(which):
                assert len(conv) == subs * sum(per_pass) and all("_batch" in k for k in conv), conv
            elif subs == 1:
                assert len(conv) == sum(per_pass) and all("_batch" in k for k in conv), conv
            else:
                assert sum(1 for k in conv if "_batch" in k) == sum(per_pass) and len(conv) > sum(per_pass), conv
    # iterations = 0 on the Y route: the copy stage instead of the chroma kernel
    noise, _, _ = pick(models, "y7", "noise")
    o0 = Side16(gpu, n, w, h, yr.YUV_420, "p010", 1, 2)
    run = lambda: gpu.process_frames_yuv_u16_device(n, w, h, yr.YUV_420, i.s, o0.s, noise, None, 0, yr.LIMITED, stream=stream().cuda_stream, depth=10)
    run()
    stream().synchronize()
    names = fm.kernel_names(run)
    assert count(names, "ChromaCopy16") == count(names, "Y16ToPlane") == count(names, "PlaneToY16") == 1 and count(names, "k_chroma2x_u16") == 0, names


@pytest.mark.parametrize("which", ["y7", "7"])
@pytest.mark.parametrize("kw", [dict(fusion=1), dict(band_rows=16), dict(precision=4)], ids=["fusion_off", "band_rows_16", "fp16x2"])
def test_option_sets(gpu, models, which, kw):
    """W2XC_FUSION_OFF at n = 3; a band_rows that cuts the 66-row plane at n = 1; a split precision: both sides run the same passes"""
    noise, scale, it = pick(models, which, "noise_scale")
    opts = gpu.make_opts(**kw)
    n = 1 if "band_rows" in kw else 3
    Y, U, V = frames(n, 17, 33, yr.YUV_420, 10, 70)
    want = composed(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10, opts=opts)
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10, opts=opts, i_style="p010", i_pack=1, align=2), want)


@pytest.mark.parametrize("which", ["y7", "7"])
@pytest.mark.parametrize("word", [0x7FC00000, 0x7149F2CA], ids=["nan", "1e30"])
def test_poisoned_scratch(gpu, models, which, word):
    noise, scale, it = pick(models, which, "noise_scale")
    Y, U, V = frames(3, 17, 33, yr.YUV_420, 10, 80)
    want = composed(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10)
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10), want)     # (the contexts and their buffers exist now)
    assert noise.fill_scratch(word) > 0 and scale.fill_scratch(word) > 0
    assert same(run_device(gpu, which, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, 10), want)


@pytest.mark.parametrize("which", ["y7", "7"])
def test_host_form_equals_device_form(gpu, models, which):
    noise, scale, it = pick(models, which, "noise_scale")
    host = gpu.process_frames_yuv_u16_rgb if is_rgb(which) else gpu.process_frames_yuv_u16
    extra = dict(matrix=rr.BT2020) if is_rgb(which) else {}
    for layout, w, h in ((yr.YUV_420, 17, 33), (yr.YUV_444, 16, 32)) + (() if is_rgb(which) else ((yr.YUV_400, 16, 32),)):
        Y, U, V = frames(3, w, h, layout, 10, 90 + layout)
        want = run_device(gpu, which, noise, scale, it, Y, U, V, layout, yr.FULL, 10)
        kw = dict(chroma=layout, noise=noise, scale=scale, iterations=it, range=gpu.RANGE_FULL, depth=10, **extra)
        got = host(Y, U, V, **kw)
        assert same(tuple(got) + (None,) * (3 - len(got)), want)
        small = sub_batch_opts(gpu, which, noise, scale, w, h, 2)      # sub-batches of 2 + 1: the second upload goes where the first frames were
        got = host(Y, U, V, opts=small, **kw)
        assert same(tuple(got) + (None,) * (3 - len(got)), want)
        if layout != yr.YUV_400:   # P010 host planes in and out: high-packed words, interleaved chroma; and P010 in with low-packed planar planes out
            uv = np.stack([U, V], axis=-1) << 6
            oy, ouv = host(Y << 6, uv=uv, pack=gpu.PACK_HIGH, **kw)
            assert same((oy >> 6, np.ascontiguousarray(ouv[..., 0]) >> 6, np.ascontiguousarray(ouv[..., 1]) >> 6), want)
            assert ((oy & 63) == 0).all() and ((ouv & 63) == 0).all()
            assert same(host(Y << 6, uv=uv, pack=gpu.PACK_HIGH, out_pack=gpu.PACK_LOW, out_nv12=False, **kw), want)


# ---- the anchors ----
@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("which", ["y7", "7", "head"])
def test_depth_8_words_give_the_8_bit_calls_bytes(gpu, models, which, rng):
    """a frame of bytes widened to low-packed words at depth = 8 gives, word for byte, the output of the 8-bit call on the bytes"""
    noise, scale, it = pick(models, which, "noise_scale")
    for layout in (yr.YUV_420, yr.YUV_444) + (() if is_rgb(which) else (yr.YUV_400,)):
        Y, U, V = frames(3, 17, 33, layout, 8, 100 + layout)
        b = lambda a: None if a is None else a.astype(np.uint8)
        kw = dict(chroma=layout, noise=noise, scale=scale, iterations=it, range=rng)
        if is_rgb(which):
            want = gpu.process_frames_yuv_u8_rgb(b(Y), b(U), b(V), matrix=rr.BT709, **kw)
            got = gpu.process_frames_yuv_u16_rgb(Y, U, V, matrix=rr.BT709, depth=8, **kw)
            dev = run_device(gpu, which, noise, scale, it, Y, U, V, layout, rng, 8, rr.BT709, i_style="p010", o_style="p010", align=2)
        else:
            want = gpu.process_frames_yuv_u8(b(Y), b(U), b(V), **kw)
            got = gpu.process_frames_yuv_u16(Y, U, V, depth=8, **kw)
            dev = run_device(gpu, which, noise, scale, it, Y, U, V, layout, rng, 8, i_style="p010" if U is not None else "planar",
                             o_style="p010" if U is not None else "planar", align=2)
        assert len(got) == len(want)
        for g, w_, d in zip(got, want, dev):
            assert g.dtype == np.uint16 and w_.dtype == np.uint8 and np.array_equal(g, w_) and np.array_equal(d, w_)


def test_y4m16_tool_matches_the_host_call(gpu, models_dir, tmp_path):
    spec = importlib.util.spec_from_file_location("w2xc_y4m16", os.path.join(ROOT, "tools", "w2xc_y4m16.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    data, fr, layout = stream16(17, 33, "420", 10, 3, seed=95, extra=b"F24:1 Ip A1:1 XCOLORRANGE=FULL")
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    assert tool.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--frames_per_call", "2"]) == 0
    noise = gpu._ModelSet.from_json(os.path.join(models_dir, "noise1_model.json"))
    scale = gpu._ModelSet.from_json(os.path.join(models_dir, "scale2.0x_model.json"))
    Y, U, V = (np.stack([f[k] for f in fr]) for k in range(3))
    want = gpu.process_frames_yuv_u16(Y, U, V, chroma=yr.YUV_420, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_FULL, depth=10)
    with open(dst, "rb") as f:
        hdr = tool.y4m.read_header(f)
        assert (hdr.w, hdr.h) == (34, 66) and hdr.get("F") == "24:1" and hdr.get("C") == "420p10" and hdr.colour_range() == "full"
        got = tool.read_frames(f, hdr, 10)
        assert f.read() == b""
    assert same(got, want) and int(want[1].max()) > 255, "ten bits went through, not eight"
    # without XCOLORRANGE --range decides, and limited is another result
    src.write_bytes(data.replace(b" XCOLORRANGE=FULL", b""))
    assert tool.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--range", "limited"]) == 0
    with open(dst, "rb") as f:
        got2 = tool.read_frames(f, tool.y4m.read_header(f), 10)
    lim = gpu.process_frames_yuv_u16(Y, U, V, chroma=yr.YUV_420, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_LIMITED, depth=10)
    assert same(got2, lim) and not np.array_equal(got2[0], got[0])
