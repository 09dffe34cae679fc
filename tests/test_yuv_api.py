"""CPU tests of the YUV frame calls (revision 0.4.1.7: w2xc_process_frames_yuv_u8[_device] and their building blocks w2xc_y8_to_plane_device,
w2xc_plane_to_y8_device, w2xc_chroma2x_u8_device): the symbols and their Python mirrors, the ABI that stays as it was, every refusal of the header's
"YUV frames" section before a device is touched, the chroma sizes, the YUV4MPEG2 reader / writer / tool (tools/w2xc_y4m.py), and the NumPy restatement of
the arithmetic (tests/yuv_ref.py) against the oracle's cubic primitive.  The GPU side: tests/test_gpu_yuv_blocks.py, tests/test_gpu_yuv_frames.py."""
import ctypes as C
import importlib.util
import io
import os

import numpy as np
import pytest

from conftest import ROOT, small_layers
from oracle import oracle as orc
from tools import gen_model

import yuv_ref as yr

NEW = ("w2xc_process_frames_yuv_u8_device", "w2xc_process_frames_yuv_u8", "w2xc_y8_to_plane_device", "w2xc_plane_to_y8_device", "w2xc_chroma2x_u8_device")


@pytest.fixture(scope="module")
def y4m():
    spec = importlib.util.spec_from_file_location("w2xc_y4m", os.path.join(ROOT, "tools", "w2xc_y4m.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def models(w2xc):
    """a Y noise model and a Y scale model (3 layers: small), an RGB model, a one-plane head model"""
    y = lambda seed: w2xc._ModelSet.from_layers(small_layers([1, 32, 32, 1], seed))
    rgb = w2xc._ModelSet.from_layers(small_layers([3, 32, 32, 3], 7))
    head_w = np.random.default_rng(8).standard_normal((32, 1, 4, 4)).astype(np.float32) * np.float32(0.05)
    head = w2xc._ModelSet.from_layers(small_layers([1, 32, 32], 9), head=(head_w, None))
    return {"noise": y(5), "scale": y(6), "rgb": rgb, "head": head}


def test_symbols_and_wrappers_exist(w2xc):
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    for name in ("process_frames_yuv_u8", "process_frames_yuv_u8_device", "y8_to_plane_device", "plane_to_y8_device", "chroma2x_u8_device", "yuv_chroma_size", "YuvPlanes"):
        assert hasattr(w2xc, name), name
    assert (w2xc.YUV_420, w2xc.YUV_422, w2xc.YUV_444, w2xc.YUV_400) == yr.LAYOUTS and (w2xc.RANGE_FULL, w2xc.RANGE_LIMITED) == (yr.FULL, yr.LIMITED)
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    for name, val in (("W2XC_YUV_420", 0), ("W2XC_YUV_422", 1), ("W2XC_YUV_444", 2), ("W2XC_YUV_400", 3), ("W2XC_RANGE_FULL", 0), ("W2XC_RANGE_LIMITED", 1)):
        assert __import__("re").search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert "left-sited" in hdr and "CENTRED" in hdr, "the header says how chroma is sited"
    # struct w2xc_yuv_planes: three pointers, four strides, one int, in the header's order
    assert [f[0] for f in w2xc.YuvPlanes._fields_] == ["y", "y_stride", "y_frame_stride", "u", "v", "c_stride", "c_frame_stride", "c_px"]
    assert C.sizeof(w2xc.YuvPlanes) == 64


def test_the_abi_stays(w2xc):
    assert C.sizeof(w2xc.Opts) == 56 and w2xc.make_opts().struct_size == 56
    assert w2xc.lib().w2xc_version() == b"w2xc_hip 0.4.1.6.1 (gfx950)"


@pytest.mark.parametrize("layout", yr.LAYOUTS)
@pytest.mark.parametrize("w,h", [(16, 32), (17, 33), (16, 33), (17, 32), (1, 1), (2, 3)])
def test_chroma_sizes(w2xc, y4m, layout, w, h):
    cw, ch = w2xc.yuv_chroma_size(w, h, layout)
    want = {yr.YUV_420: ((w + 1) // 2, (h + 1) // 2), yr.YUV_422: ((w + 1) // 2, h), yr.YUV_444: (w, h), yr.YUV_400: (0, 0)}[layout]
    assert (cw, ch) == want == yr.chroma_size(w, h, layout) == y4m.chroma_size(w, h, layout)
    # the output's chroma planes: those of a 2w x 2h frame -- the leading part of the 2cw x 2ch enlargement
    ocw, och = yr.out_chroma_size(w, h, layout)
    assert (ocw, och) == w2xc.yuv_chroma_size(2 * w, 2 * h, layout) and ocw <= 2 * cw and och <= 2 * ch
    if layout != yr.YUV_400:
        assert ocw == (2 * w + 1) // 2 if layout != yr.YUV_444 else ocw == 2 * cw
        assert och == (2 * h + 1) // 2 if layout == yr.YUV_420 else och == 2 * ch
        assert 2 * cw - ocw == (w & 1 if layout != yr.YUV_444 else 0) and 2 * ch - och == (h & 1 if layout == yr.YUV_420 else 0)


# ---- refusals: all of them before a device is touched (this machine may have none: a call that passes them answers ERR_HIP) ----
class Frames:
    """host planes of n frames and their YuvPlanes, tight unless told otherwise"""

    def __init__(self, w2xc, n, w, h, layout, px=1):
        cw, ch = yr.chroma_size(w, h, layout)
        self.y = np.zeros((n, h, w), np.uint8)
        self.c = np.zeros((n, 2, max(ch, 1), max(cw, 1)), np.uint8) if px == 1 else np.zeros((n, max(ch, 1), max(cw, 1), 2), np.uint8)
        s = w2xc.YuvPlanes()
        s.y, s.y_stride, s.y_frame_stride = self.y.ctypes.data, w, w * h
        if px == 1:
            s.u, s.v, s.c_stride, s.c_frame_stride = self.c.ctypes.data, self.c.ctypes.data + self.c.strides[1], max(cw, 1), self.c.strides[0]
        else:
            s.u, s.v, s.c_stride, s.c_frame_stride = self.c.ctypes.data, self.c.ctypes.data + 1, 2 * max(cw, 1), self.c.strides[0]
        s.c_px = px
        self.s = s


def call(w2xc, noise, scale, n, w, h, layout, rng, i, o, iterations, device=False):
    h_ = lambda m: m.handle if m is not None else None
    pi = C.byref(i) if i is not None else None
    po = C.byref(o) if o is not None else None
    if device:
        return w2xc.lib().w2xc_process_frames_yuv_u8_device(h_(noise), h_(scale), n, w, h, layout, rng, pi, po, iterations, None, None)
    return w2xc.lib().w2xc_process_frames_yuv_u8(h_(noise), h_(scale), n, w, h, layout, rng, pi, po, iterations, None)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(w2xc, models, device):
    N, S = models["noise"], models["scale"]
    n, w, h, lay = 2, 17, 9, yr.YUV_420
    i, o = Frames(w2xc, n, w, h, lay), Frames(w2xc, n, 2 * w, 2 * h, lay)
    o0 = Frames(w2xc, n, w, h, lay)
    run = lambda *a, **k: call(w2xc, *a, device=device, **k)
    if device and w2xc.device_count() > 0:
        pytest.skip("these planes are host memory: the device form is given them only where no device can be reached")
    good = (w2xc.ERR_HIP,) if w2xc.device_count() <= 0 else (w2xc.OK,)   # what a call that passes every check answers
    assert run(N, S, n, w, h, lay, yr.LIMITED, i.s, o.s, 1) in good, w2xc.last_error()
    assert run(N, None, n, w, h, lay, yr.FULL, i.s, o0.s, 0) in good, w2xc.last_error()
    A, P, U = w2xc.ERR_ARG, w2xc.ERR_PLANES, w2xc.ERR_UNSUPPORTED
    # the models
    assert run(models["rgb"], S, n, w, h, lay, 0, i.s, o.s, 1) == P
    assert run(N, models["rgb"], n, w, h, lay, 0, i.s, o.s, 1) == P
    assert run(N, models["head"], n, w, h, lay, 0, i.s, o.s, 1) == U and "upconv head" in w2xc.last_error()
    assert run(models["head"], S, n, w, h, lay, 0, i.s, o.s, 1) == U
    assert run(None, None, n, w, h, lay, 0, i.s, o.s, 1) == A
    assert run(N, None, n, w, h, lay, 0, i.s, o.s, 1) == A          # iterations = 1 without a scale model
    assert run(None, S, n, w, h, lay, 0, i.s, o0.s, 0) == A         # nothing to do
    for it in (-1, 2, 5):
        assert run(N, S, n, w, h, lay, 0, i.s, o.s, it) == A
    # counts, sizes, enumerations, null sides
    assert run(N, S, 0, w, h, lay, 0, i.s, o.s, 1) == A and run(N, S, -3, w, h, lay, 0, i.s, o.s, 1) == A
    assert run(N, S, n, 0, h, lay, 0, i.s, o.s, 1) == A and run(N, S, n, w, -1, lay, 0, i.s, o.s, 1) == A
    assert run(N, S, n, w, h, 4, 0, i.s, o.s, 1) == A and run(N, S, n, w, h, -1, 0, i.s, o.s, 1) == A
    assert run(N, S, n, w, h, lay, 2, i.s, o.s, 1) == A and run(N, S, n, w, h, lay, -1, i.s, o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, None, o.s, 1) == A and run(N, S, n, w, h, lay, 0, i.s, None, 1) == A

    def broken(side, **kw):
        t = w2xc.YuvPlanes()
        C.memmove(C.byref(t), C.byref(side), C.sizeof(t))
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    cw, ch = yr.chroma_size(w, h, lay)
    for field in ("y", "u", "v"):
        assert run(N, S, n, w, h, lay, 0, broken(i.s, **{field: None}), o.s, 1) == A
        assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, **{field: None}), 1) == A
    # strides below the row's bytes, frame strides below a plane
    assert run(N, S, n, w, h, lay, 0, broken(i.s, y_stride=w - 1), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, y_stride=2 * w - 1), 1) == A
    assert run(N, S, n, w, h, lay, 0, broken(i.s, c_stride=cw - 1), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, c_stride=w - 1), 1) == A
    assert run(N, S, n, w, h, lay, 0, broken(i.s, y_frame_stride=w * h - 1), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, c_frame_stride=w * h - 1), 1) == A
    for px in (0, 3, -1):
        assert run(N, S, n, w, h, lay, 0, broken(i.s, c_px=px), o.s, 1) == A
        assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, c_px=px), 1) == A
    # interleaved chroma needs rows of 2 (cw - 1) + 1 bytes: the planar stride is too short
    assert run(N, S, n, w, h, lay, 0, broken(i.s, c_px=2), o.s, 1) == A
    # overlaps: an output plane on an input plane, two output planes on each other, output frames on each other
    assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, y=i.s.y), 1) == A
    assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, u=i.s.u), 1) == A
    assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, v=o.s.u), 1) == A
    assert run(N, S, n, w, h, lay, 0, i.s, broken(o.s, u=o.s.y), 1) == A
    assert run(N, S, n, w, h, lay, 0, broken(i.s, v=i.s.u), o.s, 1) in good, "input planes may share memory"
    if not device:   # host planes with c_px = 2 are NV12 / NV21: two interleaved planes of one buffer
        i2 = Frames(w2xc, n, w, h, lay, px=2)
        assert run(N, S, n, w, h, lay, 0, i2.s, o.s, 1) in good and run(N, S, n, w, h, lay, 0, broken(i2.s, u=i2.s.v, v=i2.s.u), o.s, 1) in good
        assert run(N, S, n, w, h, lay, 0, broken(i2.s, v=i2.s.u + 3), o.s, 1) == A and "NV12" in w2xc.last_error()
    # W2XC_YUV_400: the chroma pointers are ignored, null included
    assert run(N, S, n, w, h, yr.YUV_400, 0, broken(i.s, u=None, v=None, c_px=77), broken(o.s, u=None, v=None, c_px=0), 1) in good, w2xc.last_error()
    assert run(N, S, n, w, h, yr.YUV_400, 0, broken(i.s, y=None), o.s, 1) == A


def test_interleaved_sides_pass_the_checks(w2xc, models):
    """NV12 on either side: v = u + 1 is ONE range of bytes, not two planes that overlap"""
    if w2xc.device_count() > 0:
        pytest.skip("with a device the call would run: tests/test_gpu_yuv_frames.py")
    n, w, h = 2, 17, 9
    for lay in (yr.YUV_420, yr.YUV_422, yr.YUV_444):
        i, o = Frames(w2xc, n, w, h, lay, px=2), Frames(w2xc, n, 2 * w, 2 * h, lay, px=2)
        assert call(w2xc, models["noise"], models["scale"], n, w, h, lay, 0, i.s, o.s, 1) == w2xc.ERR_HIP, w2xc.last_error()


def test_block_refusals(w2xc):
    lib = w2xc.lib()
    A = w2xc.ERR_ARG
    b, f = np.zeros(4096, np.uint8), np.zeros(4096, np.float32)
    pb, pf = b.ctypes.data, f.ctypes.data
    w, h = 8, 4
    y8 = lambda *a: lib.w2xc_y8_to_plane_device(*a, None)
    assert y8(None, 1, 32, 8, w, h, 0, pf, 128) == A and y8(pb, 1, 32, 8, w, h, 0, None, 128) == A
    assert y8(pb, 0, 32, 8, w, h, 0, pf, 128) == A and y8(pb, 1, 32, 8, 0, h, 0, pf, 128) == A and y8(pb, 1, 32, 8, w, 0, 0, pf, 128) == A
    assert y8(pb, 1, 32, 7, w, h, 0, pf, 128) == A                       # a stride below the row
    assert y8(pb, 2, 31, 8, w, h, 0, pf, 128) == A and y8(pb, 2, 32, 8, w, h, 0, pf, 124) == A    # frames / planes that overlap
    assert y8(pb, 1, 32, 8, w, h, 2, pf, 128) == A and y8(pb, 1, 32, 8, w, h, 0, pf, 130) == A    # the range; a plane stride that is no multiple of 4
    p8 = lambda *a: lib.w2xc_plane_to_y8_device(*a, None)
    assert p8(None, 1, 128, w, h, 0, pb, 32, 8) == A and p8(pf, 1, 128, w, h, 0, None, 32, 8) == A
    assert p8(pf, 1, 128, w, h, 0, pb, 32, 7) == A and p8(pf, 1, 128, w, h, 3, pb, 32, 8) == A and p8(pf, 2, 124, w, h, 0, pb, 32, 8) == A
    assert p8(pf, -1, 128, w, h, 0, pb, 32, 8) == A
    c2 = lambda *a: lib.w2xc_chroma2x_u8_device(*a, None)
    src, dst = pb, pb + 1024
    assert c2(None, 1, 32, 8, 1, w, h, dst, 128, 16, 1, 16, 8) == A and c2(src, 1, 32, 8, 1, w, h, None, 128, 16, 1, 16, 8) == A
    for px in (0, 3):
        assert c2(src, 1, 32, 8, px, w, h, dst, 128, 16, 1, 16, 8) == A and c2(src, 1, 32, 8, 1, w, h, dst, 128, 16, px, 16, 8) == A
    assert c2(src, 1, 32, 8, 1, w, h, dst, 128, 16, 1, 17, 8) == A and c2(src, 1, 32, 8, 1, w, h, dst, 128, 16, 1, 16, 9) == A   # outside the enlargement
    assert c2(src, 1, 32, 8, 1, w, h, dst, 128, 16, 1, 0, 8) == A
    assert c2(src, 1, 32, 7, 1, w, h, dst, 128, 16, 1, 16, 8) == A and c2(src, 1, 32, 8, 1, w, h, dst, 128, 15, 1, 16, 8) == A
    assert c2(src, 1, 32, 14, 2, w, h, dst, 256, 32, 2, 16, 8) == A and c2(src, 1, 64, 15, 2, w, h, dst, 256, 30, 2, 16, 8) == A
    assert c2(src, 2, 31, 8, 1, w, h, dst, 128, 16, 1, 16, 8) == A and c2(src, 2, 32, 8, 1, w, h, dst, 127, 16, 1, 16, 8) == A
    assert c2(src, 1, 32, 8, 1, w, h, src + 16, 128, 16, 1, 16, 8) == A                                                          # overlap
    assert c2(src, 0, 32, 8, 1, w, h, dst, 128, 16, 1, 16, 8) == A


# ---- the restatement against the oracle ----
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (9, 17), (8, 12), (5, 40)])
def test_restated_cubic_has_the_oracles_bits(oracle_built, h, w):
    """the sizes of tests/test_oracle_color.py::test_cubic's kind, and the inputs the chroma rule feeds it: byte / 255"""
    rng = np.random.default_rng(100 * h + w)
    for x in (rng.random((h, w), dtype=np.float32), rng.integers(0, 256, (h, w), dtype=np.uint8).astype(np.float32) * np.float32(1.0 / 255.0),
              (rng.standard_normal((h, w)) * 10.0 ** rng.integers(-3, 4, (h, w))).astype(np.float32)):
        a, b = yr.resize2x_cubic(x), orc.resize2x_cubic(x)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_restated_chroma_rule(oracle_built):
    rng = np.random.default_rng(3)
    C8 = rng.integers(0, 256, (9, 17), dtype=np.uint8)
    full = yr.chroma2x(C8)
    want = np.clip(np.rint(orc.resize2x_cubic(C8.astype(np.float32) * np.float32(1.0 / 255.0)) * np.float32(255)), 0, 255).astype(np.uint8)
    assert np.array_equal(full, want) and np.array_equal(yr.chroma2x(C8, 33, 17), want[:17, :33])
    for v in (0, 1, 127, 128, 254, 255):   # a constant plane comes back as that value
        assert (yr.chroma2x(np.full((5, 7), v, np.uint8)) == v).all()
    board = (np.indices((6, 8)).sum(0) % 2 * 255).astype(np.uint8)
    out = yr.chroma2x(board)
    assert out.min() == 0 and out.max() == 255, "overshoot saturates at both ends"


def test_restated_luma_ends():
    Y = np.arange(256, dtype=np.uint8)
    full, lim = yr.luma_in(Y, yr.FULL), yr.luma_in(Y, yr.LIMITED)
    assert full.dtype == lim.dtype == np.float32
    assert full[255] == 1.0 and full[0] == 0.0 and lim[16] == 0.0 and abs(lim[235] - 1.0) < 1e-6 and lim[0] < 0 and lim[255] > 1
    # the round trip is the identity on every byte, in either range
    assert np.array_equal(yr.luma_out(full, yr.FULL), Y) and np.array_equal(yr.luma_out(lim, yr.LIMITED), Y)
    # saturation at both clamps, past int32 too; ties go to even
    big = np.array([-1e10, -1.0, -0.08, 1.2, 3.0, 1e10], np.float32)
    assert yr.luma_out(big, yr.LIMITED).tolist() == [0, 0, 0, 255, 255, 255] and yr.luma_out(big, yr.FULL).tolist() == [0, 0, 0, 255, 255, 255]
    ties = (np.array([0.5, 1.5, 2.5, 100.5, 101.5]) / 219.0).astype(np.float32)   # y * 219 + 16 lands on k + 0.5 where the product is exact
    r = ties * np.float32(219) + np.float32(16)
    exact = r == np.floor(r) + 0.5
    assert exact.any()
    assert np.array_equal(yr.luma_out(ties, yr.LIMITED)[exact], (2 * np.round(r[exact] / 2)).astype(np.uint8))


def test_chroma_launch_rule_matches_the_launcher():
    src = open(os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc", "w2xc_kernels.h")).read()
    for name, val in (("W2XC_CHROMA_TQX", yr.TQX), ("W2XC_CHROMA_TQY", yr.TQY), ("W2XC_CHROMA_GRID_MAX", yr.GRID_MAX)):
        assert "#define %s %d" % (name, val) in src
    # the rule is written once, in w2xc_host_geom.hpp (chroma2x_tile_grid on yuv_tile_grid; tests/cpp/host_geom_test.cpp runs it against the expressions the
    # launchers had), and the launcher calls it with the tile, the cap and a turn per tile and PLANE
    squeeze = lambda name: " ".join(open(os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc", name)).read().split())
    geom, hip = squeeze("w2xc_host_geom.hpp"), squeeze("w2xc_yuv.hip")
    assert geom.count("yuv_tile_grid((ow / 2 + tqx) / tqx, (oh / 2 + tqy) / tqy, per_tile, cap)") == 1
    assert geom.count("turns = tiles * per_tile") == 1 and geom.count("(unsigned)(turns > cap ? cap : turns)") == 1
    assert "chroma2x_tile_grid(ow, oh, (long long)n * npl, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX)" in hip and "/ CH_TQX" not in hip
    assert yr.chroma_launch(1, 1, 1) == (1, 1) and yr.chroma_launch(63, 31, 2) == (2, 2) and yr.chroma_launch(64, 32, 1) == (4, 4)
    assert yr.chroma_launch(1920, 1080, 16) == (31 * 34 * 16, 2048)   # quads 0 .. 960: 961 of them, 31 tiles across


# ---- YUV4MPEG2 ----
@pytest.mark.parametrize("tag", [None, "420jpeg", "420mpeg2", "420paldv", "420", "422", "444", "mono"])
def test_y4m_round_trip(y4m, tag):
    data, frames = yr.y4m_stream(17, 9, tag, 3, seed=11)
    fin = io.BytesIO(data)
    hdr = y4m.read_header(fin)
    assert (hdr.w, hdr.h) == (17, 9) and not hdr.interlaced and hdr.get("F") == "30000:1001" and hdr.get("A") == "1:1"
    out = io.BytesIO()
    y4m.write_header(out, hdr)
    total = 0
    while True:
        y, u, v = y4m.read_frames(fin, hdr, 2)     # groups of two: 2 + 1
        if y.shape[0] == 0:
            break
        for k in range(y.shape[0]):
            assert np.array_equal(y[k], frames[total + k][0])
            if tag != "mono":
                assert np.array_equal(u[k], frames[total + k][1]) and np.array_equal(v[k], frames[total + k][2])
        assert (u is None) == (tag == "mono")
        total += y.shape[0]
        y4m.write_frames(out, y, u, v)
    assert total == 3
    if tag == "mono":   # (the generator writes chroma planes of 0 bytes for Cmono)
        assert all(f[1].size == 0 for f in frames)
    assert out.getvalue() == data, "byte for byte"


def nearest2x(y, u, v, layout, full):
    up = lambda a: None if a is None else np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    return up(y), up(u), up(v)


def test_y4m_tool_rewrites_the_header(y4m):
    data, frames = yr.y4m_stream(16, 8, "420mpeg2", 3, seed=12, extra=b"F25:1 Ip A128:117 XYSCSS=420MPEG2 XCOLORRANGE=FULL")
    out = io.BytesIO()
    seen = []
    def process(y, u, v, layout, full):
        seen.append((y.shape[0], layout, full))
        return nearest2x(y, u, v, layout, full)
    assert y4m.convert_stream(io.BytesIO(data), out, process, 1, "limited", 2) == 3
    assert seen == [(2, yr.YUV_420, True), (1, yr.YUV_420, True)], "groups of --frames_per_call, the stream's own range"
    out.seek(0)
    hdr = y4m.read_header(out)
    assert (hdr.w, hdr.h) == (32, 16) and hdr.get("F") == "25:1" and hdr.get("A") == "128:117" and hdr.get("C") == "420mpeg2" and hdr.get("I") == "p"
    assert hdr.colour_range() == "full" and ("X", "YSCSS=420MPEG2") in hdr.fields
    y, u, v = y4m.read_frames(out, hdr, 10)
    assert y.shape == (3, 16, 32) and u.shape == v.shape == (3, 8, 16) and np.array_equal(y[2][::2, ::2], frames[2][0])
    # no XCOLORRANGE: --range decides; a noise-only run keeps the size
    data, _ = yr.y4m_stream(16, 8, "444", 1, seed=13)
    seen.clear()
    out = io.BytesIO()
    y4m.convert_stream(io.BytesIO(data), out, lambda y, u, v, l, f: (seen.append((l, f)), (y, u, v))[1], 0, "limited", 8)
    assert seen == [(yr.YUV_444, False)] and out.getvalue() == data


@pytest.mark.parametrize("field", ["It", "Ib", "Im"])
def test_y4m_tool_refuses_interlaced_input(y4m, tmp_path, capsys, field):
    data, _ = yr.y4m_stream(16, 8, "420jpeg", 1, seed=14, extra=b"F25:1 %s A1:1" % field.encode())
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    assert y4m.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path)]) == 2
    assert "interlaced" in capsys.readouterr().err and not dst.exists()
    with pytest.raises(y4m.Y4mError):
        y4m.convert_stream(io.BytesIO(data), io.BytesIO(), nearest2x, 1)


def test_y4m_tool_refuses_what_it_cannot_read(y4m):
    for bad in (b"YUV4MPEG2 W16 H8 C420p10\n", b"YUV4MPEG2 W16 H8 C444alpha\n", b"RIFF....", b"YUV4MPEG2 H8\n", b"YUV4MPEG2 W16 H8 XCOLORRANGE=WIDE\n"):
        with pytest.raises(y4m.Y4mError):
            hdr = y4m.read_header(io.BytesIO(bad))
            hdr.layout, hdr.colour_range()
    data, _ = yr.y4m_stream(16, 8, "420", 1, seed=15)
    with pytest.raises(y4m.Y4mError):
        fin = io.BytesIO(data[:-5])
        y4m.read_frames(fin, y4m.read_header(fin), 1)
