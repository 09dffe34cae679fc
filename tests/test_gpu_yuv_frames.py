"""GPU tests of the YUV frame calls (w2xc_process_frames_yuv_u8[_device]): equality of bytes with the composed route from public calls --
w2xc_y8_to_plane_device, w2xc_convert_batch_device with nn2x = 0 / 1 and the same options, w2xc_plane_to_y8_device for luma; torch u8 * (1 / 255),
w2xc_resize2x_cubic_device, clamp(round(255 v)) and the crop for chroma (tests/test_gpu_yuv_blocks.py::composed_chroma) -- over the chroma layouts, planar
and NV12 on either side, both ranges, the three modes, sub-batches, option sets that change how the luma pass runs, poisoned scratch, the host form, the
launch list and the y4m tool.  Models: tools/gen_model.py's 7-layer 1-32-32-64-64-128-128-1 chain (one launch per layer for a sub-batch) and a 3-layer
1-32-32-1 chain (the per-image launch sequence)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, small_layers
from tools import gen_model
import fp32_matrix as fm
import yuv_ref as yr
from test_gpu_yuv_blocks import Lay, composed_chroma, stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@pytest.fixture(scope="module")
def models(gpu):
    return {"7": (gpu._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["noise1"])),
                  gpu._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]))),
            "3": (gpu._ModelSet.from_layers(small_layers([1, 32, 32, 1], 31)), gpu._ModelSet.from_layers(small_layers([1, 32, 32, 1], 32)))}


def pick(models, which, mode):
    noise, scale = models[which]
    return (noise if "noise" in mode else None), (scale if "scale" in mode else None), (1 if "scale" in mode else 0)


def frames(n, w, h, layout, seed):
    """random frames whose luma keeps clear of neither clamp: (Y, U, V), U = V = None without chroma"""
    rng = np.random.default_rng(seed)
    cw, ch = yr.chroma_size(w, h, layout)
    Y = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if layout == yr.YUV_400:
        return Y, None, None
    return Y, rng.integers(0, 256, (n, ch, cw), dtype=np.uint8), rng.integers(0, 256, (n, ch, cw), dtype=np.uint8)


# ---- the reference: the composed route ----
def composed(gpu, noise, scale, iterations, Y, U, V, layout, rng, opts=None):
    n, h, w = Y.shape
    st = stream().cuda_stream
    d_b = torch.from_numpy(Y).cuda()
    d_y = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    gpu.y8_to_plane_device(d_b.data_ptr(), n, w * h, w, w, h, rng, d_y.data_ptr(), 4 * w * h, stream=st)
    if noise is not None:
        d_n = torch.empty_like(d_y)
        noise.convert_batch_device(n, d_y.data_ptr(), 4 * w * h, 4 * w, w, h, d_n.data_ptr(), 4 * w * h, 4 * w, nn2x=False, stream=st, opts=opts)
        d_y = d_n
    W, H = w << iterations, h << iterations
    if iterations:
        d_s = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        scale.convert_batch_device(n, d_y.data_ptr(), 4 * w * h, 4 * w, w, h, d_s.data_ptr(), 4 * W * H, 4 * W, nn2x=True, stream=st, opts=opts)
        d_y = d_s
    d_o = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    gpu.plane_to_y8_device(d_y.data_ptr(), n, 4 * W * H, W, H, rng, d_o.data_ptr(), W * H, W, stream=st)
    stream().synchronize()
    oy = d_o.cpu().numpy()
    if layout == yr.YUV_400:
        return oy, None, None
    if not iterations:
        return oy, U.copy(), V.copy()
    ocw, och = yr.out_chroma_size(w, h, layout)
    return oy, composed_chroma(gpu, U, ocw, och), composed_chroma(gpu, V, ocw, och)


# ---- one side of the device call: planes in device buffers with rims, planar or NV12 ----
class Side:
    def __init__(self, gpu, n, w, h, layout, nv12=False, aligned=False):
        self.n, self.w, self.h, self.nv12 = n, w, h, nv12
        self.cw, self.ch = yr.chroma_size(w, h, layout)
        self.ly = Lay(n, h, w, 1, aligned)
        self.by = torch.full((self.ly.total,), 0xAB, dtype=torch.uint8, device="cuda")
        s = gpu.YuvPlanes()
        s.y, s.y_stride, s.y_frame_stride = self.by.data_ptr() + self.ly.off, self.ly.row, self.ly.frame
        s.c_px = 2 if nv12 else 1
        if self.cw:
            if nv12:   # one plane of ch rows of cw two-byte samples: U the even bytes, V the odd ones
                self.lc = Lay(n, self.ch, 2 * self.cw, 1, aligned)
                self.bc = [torch.full((self.lc.total,), 0xAB, dtype=torch.uint8, device="cuda")]
                s.u = self.bc[0].data_ptr() + self.lc.off
                s.v = s.u + 1
            else:
                self.lc = Lay(n, self.ch, self.cw, 1, aligned)
                self.bc = [torch.full((self.lc.total,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
                s.u, s.v = self.bc[0].data_ptr() + self.lc.off, self.bc[1].data_ptr() + self.lc.off
            s.c_stride, s.c_frame_stride = self.lc.row, self.lc.frame
        self.s = s

    def upload(self, Y, U, V):
        self.by.copy_(torch.from_numpy(self.ly.scatter(Y, 0xAB)))
        if self.cw:
            if self.nv12:
                self.bc[0].copy_(torch.from_numpy(self.lc.scatter(np.stack([U, V], axis=-1).reshape(self.n, self.ch, 2 * self.cw), 0xAB)))
            else:
                for b, P in zip(self.bc, (U, V)):
                    b.copy_(torch.from_numpy(self.lc.scatter(P, 0xAB)))
        return self

    def download(self):
        """(Y, U, V); every byte outside the planes must have kept its fill"""
        Y = self.ly.gather(self.by.cpu().numpy(), 0xAB)
        if not self.cw:
            return Y, None, None
        if self.nv12:
            uv = self.lc.gather(self.bc[0].cpu().numpy(), 0xAB).reshape(self.n, self.ch, self.cw, 2)
            return Y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])
        return (Y,) + tuple(self.lc.gather(b.cpu().numpy(), 0xAB) for b in self.bc)


def run_device(gpu, noise, scale, iterations, Y, U, V, layout, rng, opts=None, in_nv12=False, out_nv12=False, aligned=False):
    n, h, w = Y.shape
    i = Side(gpu, n, w, h, layout, in_nv12, aligned).upload(Y, U, V)
    o = Side(gpu, n, w << iterations, h << iterations, layout, out_nv12, aligned)
    gpu.process_frames_yuv_u8_device(n, w, h, layout, i.s, o.s, noise, scale, iterations, rng, stream=stream().cuda_stream, opts=opts)
    stream().synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(i.download(), (Y, U, V)) if a is not None), "the input frames were written"
    return o.download()


def same(got, want):
    assert len(got) == len(want) == 3
    for name, g, w_ in zip("YUV", got, want):
        assert (g is None) == (w_ is None), name
        if g is not None:
            assert g.shape == w_.shape and np.array_equal(g, w_), "%s: %d of %d bytes differ" % (name, int((g != w_).sum()), g.size)
    return True


LAYOUT_CASES = [(17, 33, yr.YUV_420), (16, 32, yr.YUV_422), (16, 32, yr.YUV_444), (16, 32, yr.YUV_400)]


SIDES = [(c, i, o) for c in LAYOUT_CASES for i in (False, True) for o in (False, True) if c[2] != yr.YUV_400 or not (i or o)]     # (4:0:0 has nothing to interleave)


@pytest.mark.parametrize("case,in_nv12,out_nv12", SIDES, ids=["%d-%dx%d-%s-%s" % ((420, 422, 444, 400)[c[2]], c[0], c[1], "nv12" if i else "planar", "nv12" if o else "planar")
                                                               for c, i, o in SIDES])
def test_layouts_planar_and_nv12(gpu, models, case, in_nv12, out_nv12):
    w, h, layout = case
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(2, w, h, layout, 40 + layout)
    want = composed(gpu, noise, scale, it, Y, U, V, layout, yr.LIMITED)
    assert want[0].shape == (2, 2 * h, 2 * w) and (layout == yr.YUV_400 or want[1].shape == (2,) + yr.out_chroma_size(w, h, layout)[::-1])
    for aligned in (False, True):
        assert same(run_device(gpu, noise, scale, it, Y, U, V, layout, yr.LIMITED, None, in_nv12, out_nv12, aligned), want)


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("mode", ["noise", "scale", "noise_scale"])
@pytest.mark.parametrize("which", ["7", "3"])
def test_modes_and_ranges(gpu, models, which, mode, rng):
    """mode noise is iterations = 0: the chroma bytes are copied -- from planar planes into interleaved ones too"""
    noise, scale, it = pick(models, which, mode)
    Y, U, V = frames(3, 17, 33, yr.YUV_420, 50)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng)
    if it == 0:
        assert np.array_equal(want[1], U) and np.array_equal(want[2], V)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng), want)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, rng, out_nv12=True), want)
    # the two ranges are two results: the luma bytes differ
    other = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, 1 - rng)
    assert not np.array_equal(other[0], want[0]) and np.array_equal(other[1], want[1]), "range does not touch chroma"


def sub_batch_opts(gpu, scale, w, h, want_sub):
    """a workspace_mb under which the batched chain of the scale pass takes want_sub planes: the plan is host arithmetic (w2xc_batch_plan)"""
    for mb in range(1, 4096):
        o = gpu.make_opts(workspace_mb=mb)
        batched, sub = scale.batch_plan(1, w, h, nn2x=True, opts=o)
        if not batched:      # (a budget below one whole image: bands, the per-image launch sequence)
            continue
        if sub == want_sub:
            return o
        assert sub < want_sub, "no budget gives a sub-batch of %d" % want_sub
    raise AssertionError("no budget found")


def count(names, what):
    return sum(1 for n in names if what in n)


def test_frame_counts_and_sub_batches(gpu, models):
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(3, 17, 33, yr.YUV_420, 60)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED), want)
    one = run_device(gpu, noise, scale, it, Y[1:2], U[1:2], V[1:2], yr.YUV_420, yr.LIMITED)
    assert same(one, tuple(a[1:2] for a in want)), "n = 1: frame 1 alone has the bytes it has in the batch"
    small = sub_batch_opts(gpu, scale, 17, 33, 2)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, small), composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, small))
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, small), want), "sub-batches of 2 + 1 change no byte"


def test_launch_list(gpu, models):
    """one Y8ToPlane, one PlaneToY8 and one k_chroma2x_u8 per sub-batch, one launch per layer of the batched chain, and none of the RGB detour's stages"""
    noise, scale, it = pick(models, "7", "noise_scale")
    n, w, h = 3, 17, 33
    Y, U, V = frames(n, w, h, yr.YUV_420, 61)
    i = Side(gpu, n, w, h, yr.YUV_420).upload(Y, U, V)
    o = Side(gpu, n, 2 * w, 2 * h, yr.YUV_420, nv12=True)
    for opts, subs in ((None, 1), (sub_batch_opts(gpu, scale, w, h, 2), 2)):
        run = lambda: gpu.process_frames_yuv_u8_device(n, w, h, yr.YUV_420, i.s, o.s, noise, scale, it, yr.LIMITED, stream=stream().cuda_stream, opts=opts)
        run()                                # (weights, workspaces: not in the trace)
        stream().synchronize()
        names = fm.kernel_names(run)
        assert count(names, "Y8ToPlane") == count(names, "PlaneToY8") == count(names, "k_chroma2x_u8") == subs, names
        for stage in ("U8ToYuv", "YuvToU8", "Resize2xCubic", "U8ToRgb", "RgbToU8", "ChromaCopy"):
            assert count(names, stage) == 0, (stage, names)
        # the luma passes are run_batch's: the batch kernels, once per layer launch and sub-batch (layers 1 + 2 fused, the last layer in its gather)
        conv = [k for k in names if fm.is_fp32_conv(k)]
        per_pass = [sum(1 for l in range(m.n_layers) if not m.kernel_name(l).startswith("(")) for m in (noise, scale)]
        assert per_pass == [6, 6] and len(conv) == subs * sum(per_pass) and all("_batch" in k for k in conv), conv
    # iterations = 0: the copy stage instead of the chroma kernel
    o0 = Side(gpu, n, w, h, yr.YUV_420, nv12=True)
    run = lambda: gpu.process_frames_yuv_u8_device(n, w, h, yr.YUV_420, i.s, o0.s, noise, None, 0, yr.LIMITED, stream=stream().cuda_stream)
    run()
    stream().synchronize()
    names = fm.kernel_names(run)
    assert count(names, "ChromaCopy") == count(names, "Y8ToPlane") == count(names, "PlaneToY8") == 1 and count(names, "k_chroma2x_u8") == 0, names


@pytest.mark.parametrize("kw", [dict(fusion=1), dict(band_rows=16), dict(precision=4), dict(kernel=4)], ids=["fusion_off", "band_rows_16", "fp16x2", "winograd32"])
def test_option_sets(gpu, models, kw):
    """W2XC_FUSION_OFF, a band_rows that cuts the 66-row plane, a split precision, a named kernel: both sides run the same luma pass"""
    assert (gpu.FUSION_OFF, gpu.PRECISION_FP16X2, gpu.KERNEL_WINOGRAD32) == (1, 4, 4)
    noise, scale, it = pick(models, "7", "noise_scale")
    opts = gpu.make_opts(**kw)
    Y, U, V = frames(3, 17, 33, yr.YUV_420, 70)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, opts)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED, opts), want)


@pytest.mark.parametrize("word", [0x00000000, 0x7FC00000, 0x7149F2CA], ids=["zeros", "nan", "1e30"])
def test_poisoned_scratch(gpu, models, word):
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(3, 17, 33, yr.YUV_420, 80)
    want = composed(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED)
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED), want)     # (the contexts and their buffers exist now)
    assert noise.fill_scratch(word) > 0 and scale.fill_scratch(word) > 0
    assert same(run_device(gpu, noise, scale, it, Y, U, V, yr.YUV_420, yr.LIMITED), want)


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=["420-17x33", "422-16x32", "444-16x32", "400-16x32"])
def test_host_form_equals_device_form(gpu, models, case):
    w, h, layout = case
    noise, scale, it = pick(models, "7", "noise_scale")
    Y, U, V = frames(3, w, h, layout, 90 + layout)
    want = run_device(gpu, noise, scale, it, Y, U, V, layout, yr.FULL)
    got = gpu.process_frames_yuv_u8(Y, U, V, chroma=layout, noise=noise, scale=scale, iterations=it, range=gpu.RANGE_FULL)
    assert same(tuple(got) + (None,) * (3 - len(got)), want)
    small = sub_batch_opts(gpu, scale, w, h, 2)      # sub-batches of 2 + 1: the second upload goes where the first frames were
    got = gpu.process_frames_yuv_u8(Y, U, V, chroma=layout, noise=noise, scale=scale, iterations=it, range=gpu.RANGE_FULL, opts=small)
    assert same(tuple(got) + (None,) * (3 - len(got)), want)
    if layout != yr.YUV_400:   # NV12 in and out, and NV12 in with planar planes out
        uv = np.stack([U, V], axis=-1)
        oy, ouv = gpu.process_frames_yuv_u8(Y, uv=uv, chroma=layout, noise=noise, scale=scale, iterations=it, range=gpu.RANGE_FULL)
        assert same((oy, np.ascontiguousarray(ouv[..., 0]), np.ascontiguousarray(ouv[..., 1])), want)
        assert same(gpu.process_frames_yuv_u8(Y, uv=uv, chroma=layout, noise=noise, scale=scale, iterations=it, range=gpu.RANGE_FULL, out_nv12=False), want)
        # noise only: the chroma bytes come back as they are
        got = gpu.process_frames_yuv_u8(Y, U, V, chroma=layout, noise=noise, range=gpu.RANGE_FULL, out_nv12=True)
        assert np.array_equal(got[1][..., 0], U) and np.array_equal(got[1][..., 1], V)


def test_y4m_tool_matches_the_host_call(gpu, models_dir, tmp_path):
    spec = importlib.util.spec_from_file_location("w2xc_y4m", os.path.join(ROOT, "tools", "w2xc_y4m.py"))
    y4m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(y4m)
    data, fr = yr.y4m_stream(17, 33, "420mpeg2", 3, seed=95, extra=b"F24:1 Ip A1:1 XCOLORRANGE=FULL")
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    assert y4m.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--frames_per_call", "2"]) == 0
    noise = gpu._ModelSet.from_json(os.path.join(models_dir, "noise1_model.json"))
    scale = gpu._ModelSet.from_json(os.path.join(models_dir, "scale2.0x_model.json"))
    Y, U, V = (np.stack([f[k] for f in fr]) for k in range(3))
    want = gpu.process_frames_yuv_u8(Y, U, V, chroma=yr.YUV_420, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_FULL)
    with open(dst, "rb") as f:
        hdr = y4m.read_header(f)
        assert (hdr.w, hdr.h) == (34, 66) and hdr.get("F") == "24:1" and hdr.get("A") == "1:1" and hdr.colour_range() == "full"
        got = y4m.read_frames(f, hdr, 10)
        assert f.read() == b""
    assert same(got, want)
    # the stream's XCOLORRANGE beats --range; without one --range decides, and limited is another result
    data2 = data.replace(b" XCOLORRANGE=FULL", b"")
    src.write_bytes(data2)
    assert y4m.main([str(src), str(dst), "-m", "noise_scale", "--model_dir", models_dir, "--range", "limited"]) == 0
    with open(dst, "rb") as f:
        got2 = y4m.read_frames(f, y4m.read_header(f), 10)
    lim = gpu.process_frames_yuv_u8(Y, U, V, chroma=yr.YUV_420, noise=noise, scale=scale, iterations=1, range=gpu.RANGE_LIMITED)
    assert same(got2, lim) and not np.array_equal(got2[0], got[0])
