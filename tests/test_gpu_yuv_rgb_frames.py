"""GPU tests of YUV frames through RGB models (w2xc_process_frames_yuv_u8_rgb[_device]): equality of bytes with the route the header defines the call as,
composed from public calls -- w2xc_yuv8_to_rgb_device, w2xc_convert_planes_batch_device with nn2x = 0 (noise) and nn2x = 1 (scale) or
w2xc_convert_planes_up2x_batch_device (a head model), w2xc_rgb_to_yuv8_device, all with the same options -- over the modes, planar and NV12 on either side,
the layouts, both ranges, the matrices, sub-batches, option sets that change how a pass runs, poisoned scratch, the host form, the launch list and the y4m
tool.  Models: short random three-plane chains (3-32-3), a 7-layer 3-32-32-64-64-128-128-3 chain (one launch per layer for a sub-batch), and a head model."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, small_layers
from tools import gen_model
import fp32_matrix as fm
import yuv_ref as yr
import yuv_rgb_ref as rr
from test_gpu_yuv_blocks import stream
from test_gpu_yuv_frames import Side, count, frames, same
from test_gpu_yuv_rgb_blocks import NV12, NV21, PLANAR, make_side

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
    """(noise, scale) per kind; the head model pairs with the short noise model"""
    short = lambda seed: gpu._ModelSet.from_layers(small_layers([3, 32, 3], seed))
    deep = lambda seed: gpu._ModelSet.from_layers(gen_model.synth_layers(DEEP, seed=seed))
    head_w = np.random.default_rng(8).standard_normal((64, 3, 4, 4)).astype(np.float32) * np.float32(0.05)
    head = gpu._ModelSet.from_layers(small_layers([3, 32, 32, 64, 64], 9), head=(head_w, None))
    noise3 = short(31)
    return {"3": (noise3, short(32)), "7": (deep(33), deep(34)), "head": (noise3, head)}


def pick(models, which, mode):
    noise, scale = models[which]
    return (noise if "noise" in mode else None), (scale if "scale" in mode else None), (1 if "scale" in mode else 0)


# ---- the reference: the route of the header, from public calls ----
def composed(gpu, noise, scale, iterations, Y, U, V, layout, rng, matrix, opts=None):
    n, h, w = Y.shape
    st = stream().cuda_stream
    src = Side(gpu, n, w, h, layout).upload(Y, U, V)
    d = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    gpu.yuv8_to_rgb_device(src.s, n, w, h, layout, rng, matrix, d.data_ptr(), 12 * w * h, 4 * w * h, stream=st)
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
    dst = Side(gpu, n, W, H, layout)
    gpu.rgb_to_yuv8_device(d.data_ptr(), 12 * W * H, 4 * W * H, n, W, H, layout, rng, matrix, dst.s, stream=st)
    stream().synchronize()
    return dst.download()


def run_device(gpu, noise, scale, iterations, Y, U, V, layout, rng, matrix, opts=None, in_nv12=False, out_nv12=False, aligned=False):
    n, h, w = Y.shape
    i = make_side(gpu, n, w, h, layout, in_nv12, aligned).upload(Y, U, V)
    o = make_side(gpu, n, w << iterations, h << iterations, layout, out_nv12, aligned)
    gpu.process_frames_yuv_u8_rgb_device(n, w, h, layout, i.s, o.s, noise, scale, iterations, rng, matrix, stream=stream().cuda_stream, opts=opts)
    stream().synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(i.download(), (Y, U, V))), "the input frames were written"
    return o.download()


LAYOUT_CASES = [(17, 33, yr.YUV_420), (17, 33, yr.YUV_422), (17, 33, yr.YUV_444)]
KIND_IDS = {PLANAR: "planar", NV12: "nv12", NV21: "nv21"}
SIDES = [(c, i, o) for c in LAYOUT_CASES for i in (PLANAR, NV12) for o in (PLANAR, NV12)] + [(LAYOUT_CASES[0], NV21, NV21), (LAYOUT_CASES[0], NV21, PLANAR),
                                                                                            (LAYOUT_CASES[1], PLANAR, NV21), (LAYOUT_CASES[2], NV12, NV21)]


@pytest.mark.parametrize("case,in_nv12,out_nv12", SIDES, ids=["%d-%s-%s" % ((420, 422, 444)[c[2]], KIND_IDS[i], KIND_IDS[o]) for c, i, o in SIDES])
def test_layouts_planar_and_nv12(gpu, models, case, in_nv12, out_nv12):
    w, h, layout = case
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(2, w, h, layout, 40 + layout)
    want = composed(gpu, noise, scale, it, Y, U, V, layout, yr.LIMITED, rr.BT709)
    assert want[0].shape == (2, 2 * h, 2 * w) and want[1].shape == (2,) + yr.chroma_size(2 * w, 2 * h, layout)[::-1]
    for aligned in (False, True):
        assert same(run_device(gpu, noise, scale, it, Y, U, V, layout, yr.LIMITED, rr.BT709, None, in_nv12, out_nv12, aligned), want)


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("mode", ["noise", "scale", "noise_scale"])
@pytest.mark.parametrize("which", ["3", "7", "head"])
def test_modes_ranges_and_models(gpu, models, which, mode, rng):
    noise, scale, it = pick(models, which, mode)
    Y, U, V = frames(3, 17, 33, yr.YUV_420, 50)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng, rr.BT601)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng, rr.BT601), want)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng, rr.BT601, out_nv12=True), want)
    # the two ranges and the matrices are different results
    assert not np.array_equal(composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, 1 - rng, rr.BT601)[0], want[0])
    other = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng, rr.BT2020)
    assert not np.array_equal(other[0], want[0])
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng, rr.BT2020), other)


def sub_batch_opts(gpu, noise, scale, w, h, want_sub):
    """a workspace_mb under which the batched chains of the call's passes take want_sub images at the least: the plan is host arithmetic (w2xc_batch_plan)"""
    for mb in range(1, 4096):
        o = gpu.make_opts(workspace_mb=mb)
        plans = [scale.batch_plan(3, w, h, opts=o, up2x=True) if scale.has_head else scale.batch_plan(3, w, h, nn2x=True, opts=o)]
        if noise is not None:
            plans.append(noise.batch_plan(3, w, h, nn2x=False, opts=o))
        if not all(b for b, _ in plans):      # (a budget below one whole image: bands, the per-image launch sequence)
            continue
        sub = min(s for _, s in plans)
        if sub == want_sub:
            return o
        assert sub < want_sub, "no budget gives a sub-batch of %d" % want_sub
    raise AssertionError("no budget found")


@pytest.mark.parametrize("which,w,h", [("7", 17, 33), ("head", 40, 24)], ids=["7-17x33", "head-40x24"])   # (sizes at which a budget exists that takes two of three)
def test_frame_counts_and_sub_batches(gpu, models, which, w, h):
    noise, scale, it = pick(models, which, "noise_scale")
    noise = None if which == "head" else noise   # (the short noise model's sub-batch is never the smaller one)
    Y, U, V = frames(3, w, h, yr.YUV_420, 60)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709), want)
    one = run_device(gpu, noise, scale, it, Y[1:2], U[1:2], V[1:2], yr.YUV_420, yr.LIMITED, rr.BT709)
    assert same(one, tuple(a[1:2] for a in want)), "n = 1: frame 1 alone has the bytes it has in the batch"
    small = sub_batch_opts(gpu, noise, scale, w, h, 2)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709, small),
                composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709, small))
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709, small), want), "sub-batches of 2 + 1 change no byte"


def test_launch_list(gpu, models):
    """one k_yuv8_to_rgb and one k_rgb_to_yuv8 per sub-batch, one launch per layer of the batched chain, none of the stages of the byte-image route or of the Y
    frame call"""
    noise, scale, it = pick(models, "7", "noise_scale")
    n, w, h = 3, 17, 33
    Y, U, V = frames(n, w, h, yr.YUV_420, 61)
    i = Side(gpu, n, w, h, yr.YUV_420).upload(Y, U, V)
    o = Side(gpu, n, 2 * w, 2 * h, yr.YUV_420, nv12=True)
    for opts, subs in ((None, 1), (sub_batch_opts(gpu, noise, scale, w, h, 2), 2)):
        run = lambda: gpu.process_frames_yuv_u8_rgb_device(n, w, h, yr.YUV_420, i.s, o.s, noise, scale, it, yr.LIMITED, rr.BT709, stream=stream().cuda_stream, opts=opts)
        run()                                # (weights, workspaces: not in the trace)
        stream().synchronize()
        names = fm.kernel_names(run)
        assert count(names, "k_yuv8_to_rgb") == count(names, "k_rgb_to_yuv8") == subs, names
        for stage in ("U8ToRgb", "RgbToU8", "U8ToYuv", "YuvToU8", "k_chroma2x_u8", "Y8ToPlane", "PlaneToY8", "ChromaCopy", "Resize2xCubic"):
            assert count(names, stage) == 0, (stage, names)
        # the passes are run_batch_planes': for a sub-batch of three the batch kernels, once per layer launch (the remainder of one frame behind a sub-batch of
        # two is the single-image sequence)
        conv = [k for k in names if fm.is_fp32_conv(k)]
        per_pass = [sum(1 for l in range(m.n_layers) if not m.kernel_name(l).startswith("(")) for m in (noise, scale)]
        if subs == 1:
            assert len(conv) == sum(per_pass) and all("_batch" in k for k in conv), conv
        else:
            assert sum(1 for k in conv if "_batch" in k) == sum(per_pass) and len(conv) > sum(per_pass), conv
    # a head model: its own 2x, the same two ends
    noise, scale, it = pick(models, "head", "noise_scale")
    run = lambda: gpu.process_frames_yuv_u8_rgb_device(n, w, h, yr.YUV_420, i.s, o.s, noise, scale, it, yr.LIMITED, rr.BT709, stream=stream().cuda_stream)
    run()
    stream().synchronize()
    names = fm.kernel_names(run)
    assert count(names, "k_yuv8_to_rgb") == count(names, "k_rgb_to_yuv8") == 1 and count(names, "upconv4x4_head_batch") == 1, names
    # a split precision with a head model is refused, before anything is launched
    with pytest.raises(gpu.W2xcError) as e:
        gpu.process_frames_yuv_u8_rgb_device(n, w, h, yr.YUV_420, i.s, o.s, noise, scale, it, yr.LIMITED, rr.BT709, stream=stream().cuda_stream,
                                             opts=gpu.make_opts(precision=gpu.PRECISION_FP16X2))
    assert e.value.code == gpu.ERR_UNSUPPORTED


OPTION_SETS = [("7", dict(fusion=1), 3, 17, 33), ("7", dict(band_rows=16), 1, 17, 33), ("7", dict(precision=4), 3, 17, 33), ("head", dict(fusion=1), 3, 17, 33),
               ("head", dict(band_rows=8), 1, 17, 33), ("7", dict(), 3, 40, 24)]


@pytest.mark.parametrize("which,kw,n,w,h", OPTION_SETS, ids=["fusion_off", "band_rows_16_n1", "fp16x2", "head_fusion_off", "head_band_rows_8_n1", "40x24"])
def test_option_sets(gpu, models, which, kw, n, w, h):
    """W2XC_FUSION_OFF, a band_rows that cuts the plane of one frame, a split precision, another size: both sides run the same passes"""
    assert (gpu.FUSION_OFF, gpu.PRECISION_FP16X2) == (1, 4)
    noise, scale, it = pick(models, which, "noise_scale")
    opts = gpu.make_opts(**kw)
    Y, U, V = frames(n, w, h, yr.YUV_420, 70)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709, opts)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709, opts), want)


@pytest.mark.parametrize("word", [0x00000000, 0x7FC00000, 0x7149F2CA], ids=["zeros", "nan", "1e30"])
def test_poisoned_scratch(gpu, models, word):
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(3, 17, 33, yr.YUV_420, 80)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709), want)     # (the contexts and their buffers exist now)
    assert noise.fill_scratch(word) > 0 and scale.fill_scratch(word) > 0
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709), want)


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=["420", "422", "444"])
def test_host_form_equals_device_form(gpu, models, case):
    w, h, layout = case
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(3, w, h, layout, 90 + layout)
    kw = dict(chroma=layout, noise=noise, scale=scale, iterations=it, range=gpu.RANGE_FULL, matrix=gpu.MATRIX_BT2020)
    want = run_device(gpu, noise, scale, it, Y, U, V, layout, yr.FULL, rr.BT2020)
    assert same(gpu.process_frames_yuv_u8_rgb(Y, U, V, **kw), want)
    small = sub_batch_opts(gpu, noise, scale, w, h, 2)      # sub-batches of 2 + 1: the second upload goes where the first frames were
    assert same(gpu.process_frames_yuv_u8_rgb(Y, U, V, opts=small, **kw), want)
    uv = np.stack([U, V], axis=-1)
    oy, ouv = gpu.process_frames_yuv_u8_rgb(Y, uv=uv, **kw)
    assert same((oy, np.ascontiguousarray(ouv[..., 0]), np.ascontiguousarray(ouv[..., 1])), want)
    assert same(gpu.process_frames_yuv_u8_rgb(Y, uv=uv, out_nv12=False, **kw), want)
    # NV21 host planes on both sides (u = v + 1), through the C entry point: V is the first byte of a pair
    vu, ovu, oy = np.ascontiguousarray(uv[..., ::-1]), np.zeros_like(ouv), np.zeros_like(oy)
    si, so = gpu.YuvPlanes(), gpu.YuvPlanes()
    for s_, y_, c_ in ((si, Y, vu), (so, oy, ovu)):
        s_.y, s_.y_stride, s_.y_frame_stride = y_.ctypes.data, y_.strides[1], y_.strides[0]
        s_.v, s_.u, s_.c_stride, s_.c_frame_stride, s_.c_px = c_.ctypes.data, c_.ctypes.data + 1, c_.strides[1], c_.strides[0], 2
    rc = gpu.lib().w2xc_process_frames_yuv_u8_rgb(noise.handle, scale.handle, 3, w, h, layout, gpu.RANGE_FULL, gpu.MATRIX_BT2020, si, so, it, small)
    assert rc == gpu.OK, gpu.last_error()
    assert same((oy, np.ascontiguousarray(ovu[..., 1]), np.ascontiguousarray(ovu[..., 0])), want)
    swapped = gpu.process_frames_yuv_u8_rgb(Y, V, U, **kw)
    assert not np.array_equal(swapped[0], want[0]), "with a colour matrix the order of U and V shows in luma"


def test_y4m_tool_matches_the_host_call(gpu, tmp_path):
    spec = importlib.util.spec_from_file_location("w2xc_y4m", os.path.join(ROOT, "tools", "w2xc_y4m.py"))
    y4m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(y4m)
    gen_model.write_json(small_layers([3, 32, 3], 31), str(tmp_path / "noise1_model.json"))
    gen_model.write_json(small_layers([3, 32, 3], 32), str(tmp_path / "scale2.0x_model.json"))
    data, fr = yr.y4m_stream(17, 33, "420", 3, seed=95, extra=b"F24:1 Ip A1:1 XCOLORRANGE=FULL")
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    noise = gpu._ModelSet.from_json(str(tmp_path / "noise1_model.json"))
    scale = gpu._ModelSet.from_json(str(tmp_path / "scale2.0x_model.json"))
    Y, U, V = (np.stack([f[k] for f in fr]) for k in range(3))
    results = {}
    for arg, matrix in ((None, gpu.MATRIX_BT601), ("bt2020", gpu.MATRIX_BT2020)):   # (33 rows: the default is bt601)
        argv = [str(src), str(dst), "-m", "noise_scale", "--model_dir", str(tmp_path), "--frames_per_call", "2"] + (["--matrix", arg] if arg else [])
        assert y4m.main(argv) == 0
        want = gpu.process_frames_yuv_u8_rgb(Y, U, V, chroma=yr.YUV_420, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_FULL, matrix=matrix)
        with open(dst, "rb") as f:
            hdr = y4m.read_header(f)
            assert (hdr.w, hdr.h) == (34, 66) and hdr.get("F") == "24:1" and hdr.get("C") == "420" and hdr.colour_range() == "full"
            got = y4m.read_frames(f, hdr, 10)
            assert f.read() == b""
        assert same(got, want)
        results[arg] = got
    assert not np.array_equal(results[None][0], results["bt2020"][0])
