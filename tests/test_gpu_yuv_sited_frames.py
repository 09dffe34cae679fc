"""GPU tests of the YUV frame calls with chroma siting flags in `chroma` (w2xc_process_frames_yuv_u8[_rgb][_device], w2xc_process_frames_yuv_u16[_rgb][_device];
include/w2xc_hip.h, "Chroma siting"): equality of bytes and words with the routes the header defines the calls as, composed from public calls with the same
options and the same `chroma` value at both ends -- luma as the centred calls' routes have it and w2xc_chroma2x_u8_sited_device /
w2xc_chroma2x_u16_sited_device per chroma plane for the Y calls; w2xc_yuv8_to_rgb_device / w2xc_yuv16_to_rgb_device, w2xc_convert_planes_batch_device /
w2xc_convert_planes_up2x_batch_device, w2xc_rgb_to_yuv8_device / w2xc_rgb_to_yuv16_device for the RGB calls -- for the three sited layouts, a Y model, a 3-32-3
model and a head model, n = 1 / 3 / 2 + 1, a cutting band_rows, W2XC_FUSION_OFF, poisoned scratch, the host form, the launch list and the y4m tools.  Frames of at
most 66 x 34."""
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
import yuv_sited_ref as sr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_yuv_frames as f8   # noqa: E402
import test_gpu_yuv_rgb_frames as f8r   # noqa: E402
import test_gpu_yuv16_frames as f16   # noqa: E402
from test_gpu_yuv_blocks import stream   # noqa: E402
from test_gpu_yuv_rgb_blocks import NV12, NV21, PLANAR, make_side   # noqa: E402
from test_gpu_yuv16_blocks import Side16, to_dev, to_host   # noqa: E402
from test_yuv16_api import stream16   # noqa: E402

models = f16.models          # the fixture: "y3" / "y7" Y models, "3" 3-32-3 models, "7" a deep three-plane chain, "head" a head model
SITED = sr.SITED_LAYOUTS
SITED_IDS = [sr.SITED_IDS[c] for c in SITED]
FAMILIES = [(8, False), (8, True), (16, False), (16, True)]        # (bits, rgb): the four families of frame calls, device and host form each
FAMILY_IDS = ["u8", "u8_rgb", "u16", "u16_rgb"]
DEPTH = {8: 8, 16: 10}


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def frames(bits, n, w, h, chroma, seed):
    r = np.random.default_rng(seed)
    cw, ch = sr.chroma_size(w, h, chroma)
    dt = np.uint8 if bits == 8 else np.uint16
    return tuple(r.integers(0, 1 << DEPTH[bits], s).astype(dt) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))


# ---- the references: the routes of the header, from public calls on tight planes ----
def composed_y(gpu, bits, noise, scale, it, Y, U, V, chroma, rng, opts=None):
    """luma: the centred call's route (it has no chroma in it); chroma: the sited block per plane, with the call's flags"""
    n, h, w = Y.shape
    if bits == 8:
        oy = f8.composed(gpu, noise, scale, it, Y, None, None, yr.YUV_400, rng, opts)[0]
    else:
        oy = f16.composed_y(gpu, noise, scale, it, Y, None, None, yr.YUV_400, rng, DEPTH[bits], opts)[0]
    if not it:
        return oy, U.copy(), V.copy()
    cw, ch = sr.chroma_size(w, h, chroma)
    ocw, och = sr.chroma_size(2 * w, 2 * h, chroma)
    st, out = stream().cuda_stream, []
    for P in (U, V):
        if bits == 8:
            d_c, d_u = torch.from_numpy(P).cuda(), torch.zeros((n, och, ocw), dtype=torch.uint8, device="cuda")
            gpu.chroma2x_u8_sited_device(d_c.data_ptr(), n, cw * ch, cw, 1, cw, ch, d_u.data_ptr(), ocw * och, ocw, 1, ocw, och, chroma & 0x30, stream=st)
            stream().synchronize()
            out.append(d_u.cpu().numpy())
        else:
            d_c, d_u = to_dev(P), to_dev(np.zeros((n, och, ocw), np.uint16))
            gpu.chroma2x_u16_sited_device(d_c.data_ptr(), n, 2 * cw * ch, 2 * cw, 1, y16.LOW, cw, ch, DEPTH[bits], d_u.data_ptr(), 2 * ocw * och, 2 * ocw, 1, y16.LOW, ocw,
                                          och, chroma & 0x30, stream=st)
            stream().synchronize()
            out.append(to_host(d_u))
    return oy, out[0], out[1]


def side(gpu, bits, n, w, h, chroma, kind=PLANAR, aligned=False):
    """one side of a call in device buffers with rims: bytes planar / NV12 / NV21, words planar / P010 / VU"""
    if bits == 8:
        return make_side(gpu, n, w, h, chroma & 0xF, kind, aligned)
    style = {PLANAR: "planar", NV12: "p010", NV21: "vu"}[kind]
    return Side16(gpu, n, w, h, chroma & 0xF, style, 1 if kind else 0, 4 if aligned else 1)


def upload(s, bits, Y, U, V):
    return s.upload(Y, U, V) if bits == 8 else s.upload(Y, U, V, DEPTH[bits])


def download(s, bits):
    return s.download() if bits == 8 else s.download(DEPTH[bits])


def composed_rgb(gpu, bits, noise, scale, it, Y, U, V, chroma, rng, matrix, opts=None):
    n, h, w = Y.shape
    st = stream().cuda_stream
    src = upload(side(gpu, bits, n, w, h, chroma), bits, Y, U, V)
    d = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    if bits == 8:
        gpu.yuv8_to_rgb_device(src.s, n, w, h, chroma, rng, matrix, d.data_ptr(), 12 * w * h, 4 * w * h, stream=st)
    else:
        gpu.yuv16_to_rgb_device(src.s, n, w, h, chroma, rng, DEPTH[bits], matrix, d.data_ptr(), 12 * w * h, 4 * w * h, stream=st)
    if noise is not None:
        d_n = torch.empty_like(d)
        noise.convert_planes_batch_device(n, 3, d.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, d_n.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, nn2x=False, stream=st,
                                          opts=opts)
        d = d_n
    W, H = w << it, h << it
    if it:
        d_s = torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda")
        if scale.has_head:
            scale.convert_planes_up2x_batch_device(n, 3, d.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, d_s.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, stream=st, opts=opts)
        else:
            scale.convert_planes_batch_device(n, 3, d.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, d_s.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, nn2x=True, stream=st,
                                              opts=opts)
        d = d_s
    dst = side(gpu, bits, n, W, H, chroma)
    if bits == 8:
        gpu.rgb_to_yuv8_device(d.data_ptr(), 12 * W * H, 4 * W * H, n, W, H, chroma, rng, matrix, dst.s, stream=st)
    else:
        gpu.rgb_to_yuv16_device(d.data_ptr(), 12 * W * H, 4 * W * H, n, W, H, chroma, rng, DEPTH[bits], matrix, dst.s, stream=st)
    stream().synchronize()
    return download(dst, bits)


def composed(gpu, bits, rgb, noise, scale, it, Y, U, V, chroma, rng, opts=None, matrix=rr.BT709):
    if rgb:
        return composed_rgb(gpu, bits, noise, scale, it, Y, U, V, chroma, rng, matrix, opts)
    return composed_y(gpu, bits, noise, scale, it, Y, U, V, chroma, rng, opts)


def call_device(gpu, bits, rgb, n, w, h, chroma, i, o, noise, scale, it, rng, matrix, opts):
    st = stream().cuda_stream
    if bits == 8 and rgb:
        gpu.process_frames_yuv_u8_rgb_device(n, w, h, chroma, i.s, o.s, noise, scale, it, rng, matrix, stream=st, opts=opts)
    elif bits == 8:
        gpu.process_frames_yuv_u8_device(n, w, h, chroma, i.s, o.s, noise, scale, it, rng, stream=st, opts=opts)
    elif rgb:
        gpu.process_frames_yuv_u16_rgb_device(n, w, h, chroma, i.s, o.s, noise, scale, it, rng, matrix, stream=st, opts=opts, depth=DEPTH[bits])
    else:
        gpu.process_frames_yuv_u16_device(n, w, h, chroma, i.s, o.s, noise, scale, it, rng, stream=st, opts=opts, depth=DEPTH[bits])


def run_device(gpu, bits, rgb, noise, scale, it, Y, U, V, chroma, rng, opts=None, matrix=rr.BT709, in_kind=PLANAR, out_kind=PLANAR, aligned=False):
    """the frame call on planes with rims"""
    n, h, w = Y.shape
    i = upload(side(gpu, bits, n, w, h, chroma, in_kind, aligned), bits, Y, U, V)
    o = side(gpu, bits, n, w << it, h << it, chroma, out_kind, aligned)
    call_device(gpu, bits, rgb, n, w, h, chroma, i, o, noise, scale, it, rng, matrix, opts)
    stream().synchronize()
    return download(o, bits)      # (checks the rims)


def same(got, want):
    assert len(got) == len(want) == 3
    for name, g, w_ in zip("YUV", got, want):
        assert g.shape == w_.shape and np.array_equal(g, w_), "%s: %d of %d samples differ" % (name, int((g != w_).sum()), g.size)
    return True


def pick(models, rgb, which=None):
    """(noise, scale) for a family: a Y model pair, the 3-32-3 pair, or the head model as scale model"""
    return models[which or ("3" if rgb else "y3")]


# ---- the four families x the three sited layouts ----
@pytest.mark.parametrize("chroma", SITED, ids=SITED_IDS)
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_frame_call_is_its_composed_route(gpu, models, family, chroma):
    """n = 3 on every kind of side, n = 1, and sub-batches of 2 + 1"""
    bits, rgb = family
    noise, scale = pick(models, rgb)
    w, h = 17, 33
    Y, U, V = frames(bits, 3, w, h, chroma, 40 + chroma)
    want = composed(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED)
    for k, (ik, ok) in enumerate(((PLANAR, PLANAR), (NV12, PLANAR), (PLANAR, NV12), (NV21, NV12))):
        assert same(run_device(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED, in_kind=ik, out_kind=ok, aligned=bool(k & 1)), want), (ik, ok)
    one = run_device(gpu, bits, rgb, noise, scale, 1, Y[1:2], U[1:2], V[1:2], chroma, yr.LIMITED)
    assert same(one, tuple(a[1:2] for a in want)), "n = 1: frame 1 alone has the samples it has in the batch"
    deep = "7" if rgb else "y7"        # (the 7-layer chains: a workspace budget exists under which they take two frames at a time)
    nd, sd = models[deep]
    small = f16.sub_batch_opts(gpu, deep, nd, sd, w, h, 2)
    want_d = composed(gpu, bits, rgb, nd, sd, 1, Y, U, V, chroma, yr.LIMITED, opts=small)
    assert same(run_device(gpu, bits, rgb, nd, sd, 1, Y, U, V, chroma, yr.LIMITED, opts=small, out_kind=NV12), want_d)
    assert same(run_device(gpu, bits, rgb, nd, sd, 1, Y, U, V, chroma, yr.LIMITED), want_d), "sub-batches of 2 + 1 change no sample"
    # the noise pass alone: the Y route copies chroma, the RGB route converts it at both ends
    want0 = composed(gpu, bits, rgb, noise, None, 0, Y, U, V, chroma, yr.FULL)
    assert same(run_device(gpu, bits, rgb, noise, None, 0, Y, U, V, chroma, yr.FULL, in_kind=NV12), want0)
    if not rgb:
        assert np.array_equal(want0[1], U) and np.array_equal(want0[2], V)


@pytest.mark.parametrize("chroma", SITED, ids=SITED_IDS)
@pytest.mark.parametrize("bits", [8, 16])
def test_head_model_and_deep_y_model(gpu, models, bits, chroma):
    noise, head = models["head"]
    Y, U, V = frames(bits, 3, 40, 24, chroma, 50)
    want = composed(gpu, bits, True, None, head, 1, Y, U, V, chroma, yr.FULL, matrix=rr.BT2020)
    assert same(run_device(gpu, bits, True, None, head, 1, Y, U, V, chroma, yr.FULL, matrix=rr.BT2020, out_kind=NV12, aligned=True), want)
    n7, s7 = models["y7"]
    Y, U, V = frames(bits, 2, 66, 34, chroma, 51)        # chroma planes past one tile of quads
    want = composed(gpu, bits, False, n7, s7, 1, Y, U, V, chroma, yr.LIMITED)
    for kinds in ((PLANAR, NV12), (NV12, NV12)):
        for aligned in (False, True):
            assert same(run_device(gpu, bits, False, n7, s7, 1, Y, U, V, chroma, yr.LIMITED, in_kind=kinds[0], out_kind=kinds[1], aligned=aligned), want)


@pytest.mark.parametrize("kw", [dict(fusion=1), dict(band_rows=16)], ids=["fusion_off", "band_rows_16"])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_option_sets(gpu, models, family, kw):
    """W2XC_FUSION_OFF at n = 3; a band_rows that cuts the 66-row plane at n = 1: both sides run the same passes"""
    bits, rgb = family
    noise, scale = pick(models, rgb, "7" if rgb else "y7")
    opts = gpu.make_opts(**kw)
    n = 1 if "band_rows" in kw else 3
    for chroma in SITED:
        Y, U, V = frames(bits, n, 17, 33, chroma, 70)
        want = composed(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED, opts=opts)
        assert same(run_device(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED, opts=opts, in_kind=NV12, aligned=True), want), hex(chroma)


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_poisoned_scratch(gpu, models, family):
    bits, rgb = family
    noise, scale = pick(models, rgb, "7" if rgb else "y7")
    chroma = sr.YUV_420_TOPLEFT
    Y, U, V = frames(bits, 3, 17, 33, chroma, 80)
    want = composed(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED)
    assert same(run_device(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED), want)     # (the contexts and their buffers exist now)
    for word in (0x7FC00000, 0x7149F2CA):
        assert noise.fill_scratch(word) > 0 and scale.fill_scratch(word) > 0
        assert same(run_device(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED), want)


@pytest.mark.parametrize("chroma", SITED, ids=SITED_IDS)
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_host_form_equals_device_form(gpu, models, family, chroma):
    bits, rgb = family
    noise, scale = pick(models, rgb)
    host = {(8, False): gpu.process_frames_yuv_u8, (8, True): gpu.process_frames_yuv_u8_rgb, (16, False): gpu.process_frames_yuv_u16,
            (16, True): gpu.process_frames_yuv_u16_rgb}[family]
    kw = dict(chroma=chroma, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_FULL)
    kw.update(dict(matrix=rr.BT709) if rgb else {})
    kw.update(dict(depth=DEPTH[bits]) if bits == 16 else {})
    Y, U, V = frames(bits, 3, 17, 33, chroma, 90)
    want = run_device(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.FULL)
    assert same(host(Y, U, V, **kw), want)
    oy, ouv = host(Y, uv=np.stack([U, V], axis=-1), **kw)         # interleaved host planes in and out
    assert same((oy, np.ascontiguousarray(ouv[..., 0]), np.ascontiguousarray(ouv[..., 1])), want)
    deep = "7" if rgb else "y7"
    nd, sd = models[deep]
    small = f16.sub_batch_opts(gpu, deep, nd, sd, 17, 33, 2)      # sub-batches of 2 + 1: the second upload goes where the first frames were
    kw.update(noise=nd, scale=sd)
    assert same(host(Y, U, V, opts=small, **kw), run_device(gpu, bits, rgb, nd, sd, 1, Y, U, V, chroma, yr.FULL))


def count(names, what):
    return sum(1 for n in names if what in n)


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_launch_lists(gpu, models, family):
    """one sited kernel per end and sub-batch, none of the centred tile kernels, and the passes between the ends as many layer launches as without a flag"""
    bits, rgb = family
    noise, scale = pick(models, rgb, "7" if rgb else "y7")
    n, w, h = 3, 17, 33
    tag = "8" if bits == 8 else "16"
    sited = ("k_yuv%s_to_rgb_sited" % tag, "k_rgb_to_yuv%s_sited" % tag) if rgb else ("k_chroma2x_u%s_sited" % tag,)
    centred = ("k_yuv%s_to_rgb<" % tag, "k_rgb_to_yuv%s<" % tag, "k_chroma2x_u%s<" % tag)
    small = f16.sub_batch_opts(gpu, "7" if rgb else "y7", noise, scale, w, h, 2)
    convs = {}
    for chroma in SITED + (yr.YUV_420,):
        Y, U, V = frames(bits, n, w, h, chroma, 61)
        i = upload(side(gpu, bits, n, w, h, chroma), bits, Y, U, V)
        o = side(gpu, bits, n, 2 * w, 2 * h, chroma, NV12, True)
        for opts, subs in ((None, 1), (small, 2)):
            run = lambda: call_device(gpu, bits, rgb, n, w, h, chroma, i, o, noise, scale, 1, yr.LIMITED, rr.BT709, opts)
            run()
            stream().synchronize()
            names = fm.kernel_names(run)
            convs[(chroma, subs)] = [k for k in names if fm.is_fp32_conv(k)]
            for k in sited:
                assert count(names, k) == (subs if chroma & 0x30 else 0), (hex(chroma), k, names)
            if chroma & 0x30:
                for k in centred:
                    assert count(names, k) == 0, (hex(chroma), k, names)
    for chroma in (sr.YUV_420_LEFT, sr.YUV_420_TOPLEFT):
        for subs in (1, 2):
            assert convs[(chroma, subs)] == convs[(yr.YUV_420, subs)] and convs[(chroma, subs)], "the CNN between the ends does not know the siting"


# ---- the anchor ----
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_no_flag_gives_the_existing_calls_samples(gpu, models, family):
    """without a flag a call gives the samples of its centred route, composed by the existing tests' references; with one, other chroma (and, through a
    colour matrix, other luma) but the same luma on the Y route"""
    bits, rgb = family
    noise, scale = pick(models, rgb)
    Y, U, V = frames(bits, 3, 17, 33, yr.YUV_420, 99)
    got = run_device(gpu, bits, rgb, noise, scale, 1, Y, U, V, yr.YUV_420, yr.LIMITED)
    if bits == 8:
        want = f8r.composed(gpu, noise, scale, 1, Y, U, V, yr.YUV_420, yr.LIMITED, rr.BT709) if rgb else f8.composed(gpu, noise, scale, 1, Y, U, V, yr.YUV_420, yr.LIMITED)
    else:
        want = f16.composed(gpu, "3" if rgb else "y3", noise, scale, 1, Y, U, V, yr.YUV_420, yr.LIMITED, DEPTH[bits], rr.BT709)
    assert same(got, want)
    for chroma in (sr.YUV_420_LEFT, sr.YUV_420_TOPLEFT):
        sited = run_device(gpu, bits, rgb, noise, scale, 1, Y, U, V, chroma, yr.LIMITED)
        assert not np.array_equal(sited[1], got[1]) and not np.array_equal(sited[2], got[2])
        assert np.array_equal(sited[0], got[0]) != rgb


# ---- the tools ----
def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_y4m_tool_siting(gpu, models_dir, tmp_path):
    """--siting auto on a C420mpeg2 stream is the YUV_420_LEFT call; the default stays the centred call; the C tag is passed on"""
    y4m = load_tool("w2xc_y4m")
    data, fr = yr.y4m_stream(17, 33, "420mpeg2", 3, seed=95, extra=b"F24:1 Ip A1:1 XCOLORRANGE=FULL")
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    noise = gpu._ModelSet.from_json(os.path.join(models_dir, "noise1_model.json"))
    scale = gpu._ModelSet.from_json(os.path.join(models_dir, "scale2.0x_model.json"))
    Y, U, V = (np.stack([f[k] for f in fr]) for k in range(3))
    results = {}
    for siting, chroma in ((None, yr.YUV_420), ("auto", sr.YUV_420_LEFT), ("left", sr.YUV_420_LEFT), ("topleft", sr.YUV_420_TOPLEFT), ("center", yr.YUV_420)):
        argv = [str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--frames_per_call", "2"] + (["--siting", siting] if siting else [])
        assert y4m.main(argv) == 0
        want = gpu.process_frames_yuv_u8(Y, U, V, chroma=chroma, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_FULL)
        with open(dst, "rb") as f:
            hdr = y4m.read_header(f)
            assert (hdr.w, hdr.h) == (34, 66) and hdr.get("C") == "420mpeg2"
            got = y4m.read_frames(f, hdr, 10)
            assert f.read() == b""
        assert same(got, want), siting
        results[siting] = got
    assert not np.array_equal(results[None][1], results["auto"][1]) and not np.array_equal(results["auto"][1], results["topleft"][1])
    # three-plane models: the RGB call with the same flags
    gen_model.write_json(small_layers([3, 32, 3], 31), str(tmp_path / "noise1_model.json"))
    gen_model.write_json(small_layers([3, 32, 3], 32), str(tmp_path / "scale2.0x_model.json"))
    n3, s3 = gpu._ModelSet.from_json(str(tmp_path / "noise1_model.json")), gpu._ModelSet.from_json(str(tmp_path / "scale2.0x_model.json"))
    assert y4m.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", str(tmp_path), "--siting", "auto"]) == 0
    want = gpu.process_frames_yuv_u8_rgb(Y, U, V, chroma=sr.YUV_420_LEFT, noise=n3, scale=s3, iterations=1, range=gpu.RANGE_FULL, matrix=gpu.MATRIX_BT601)
    with open(dst, "rb") as f:
        assert same(y4m.read_frames(f, y4m.read_header(f), 10), want)


def test_y4m16_tool_siting(gpu, models_dir, tmp_path):
    """the CxxxpD tags name no siting: auto is the centred call, left the YUV_420_LEFT call"""
    tool = load_tool("w2xc_y4m16")
    data, fr, layout = stream16(17, 33, "420", 10, 3, seed=96, extra=b"F24:1 Ip A1:1 XCOLORRANGE=FULL")
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    noise = gpu._ModelSet.from_json(os.path.join(models_dir, "noise1_model.json"))
    scale = gpu._ModelSet.from_json(os.path.join(models_dir, "scale2.0x_model.json"))
    Y, U, V = (np.stack([f[k] for f in fr]) for k in range(3))
    for siting, chroma in (("auto", yr.YUV_420), ("left", sr.YUV_420_LEFT), ("topleft", sr.YUV_420_TOPLEFT)):
        assert tool.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--frames_per_call", "2", "--siting", siting]) == 0
        want = gpu.process_frames_yuv_u16(Y, U, V, chroma=chroma, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_FULL, depth=10)
        with open(dst, "rb") as f:
            hdr = tool.y4m.read_header(f)
            assert hdr.get("C") == "420p10"
            assert same(tool.read_frames(f, hdr, 10), want), siting
