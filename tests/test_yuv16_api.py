"""CPU tests of the 16-bit YUV frame calls (revision 0.4.1.9: w2xc_process_frames_yuv_u16[_rgb][_device] and the five blocks w2xc_y16_to_plane_device,
w2xc_plane_to_y16_device, w2xc_chroma2x_u16_device, w2xc_yuv16_to_rgb_device, w2xc_rgb_to_yuv16_device): the symbols and their Python mirrors, the ABI that
stays, every refusal before a device is touched, the NumPy restatement (tests/yuv16_ref.py) against the 8-bit restatements and its own properties for every
depth, the y4m16 tool, the launch rules and the new kernels' registers.  The GPU side: tests/test_gpu_yuv16_blocks.py, tests/test_gpu_yuv16_frames.py."""
import ctypes as C
import importlib.util
import inspect
import io
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, small_layers

import yuv_ref as yr
import yuv_rgb_ref as rr
import yuv16_ref as y16

F32 = np.float32
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")
FRAME_CALLS = ("w2xc_process_frames_yuv_u16_device", "w2xc_process_frames_yuv_u16", "w2xc_process_frames_yuv_u16_rgb_device", "w2xc_process_frames_yuv_u16_rgb")
BLOCKS = ("w2xc_y16_to_plane_device", "w2xc_plane_to_y16_device", "w2xc_chroma2x_u16_device", "w2xc_yuv16_to_rgb_device", "w2xc_rgb_to_yuv16_device")


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def y4m16():
    return load_tool("w2xc_y4m16")


@pytest.fixture(scope="module")
def models(w2xc):
    y = lambda seed: w2xc._ModelSet.from_layers(small_layers([1, 32, 32, 1], seed))
    rgb = lambda seed: w2xc._ModelSet.from_layers(small_layers([3, 32, 32, 3], seed))
    head_w = np.random.default_rng(8).standard_normal((32, 1, 4, 4)).astype(np.float32) * np.float32(0.05)
    head1 = w2xc._ModelSet.from_layers(small_layers([1, 32, 32], 9), head=(head_w, None))
    head3_w = np.random.default_rng(9).standard_normal((32, 3, 4, 4)).astype(np.float32) * np.float32(0.05)
    head3 = w2xc._ModelSet.from_layers(small_layers([3, 32, 32], 10), head=(head3_w, None))
    return {"noise": y(5), "scale": y(6), "rgb_noise": rgb(7), "rgb_scale": rgb(11), "head1": head1, "head3": head3}


# ---- the boundary ----
def test_symbols_wrappers_and_the_abi(w2xc):
    lib = C.CDLL(w2xc.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    for name in FRAME_CALLS + BLOCKS:
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
    for name in ("process_frames_yuv_u16", "process_frames_yuv_u16_device", "process_frames_yuv_u16_rgb", "process_frames_yuv_u16_rgb_device", "y16_to_plane_device",
                 "plane_to_y16_device", "chroma2x_u16_device", "yuv16_to_rgb_device", "rgb_to_yuv16_device", "Yuv16Planes", "PACK_LOW", "PACK_HIGH"):
        assert hasattr(w2xc, name), name
    assert (w2xc.PACK_LOW, w2xc.PACK_HIGH) == (y16.LOW, y16.HIGH) == (0, 1)
    assert re.search(r"#define\s+W2XC_PACK_LOW\s+0\b", hdr) and re.search(r"#define\s+W2XC_PACK_HIGH\s+1\b", hdr)
    assert "16-bit YUV frames (revision 0.4.1.9)" in hdr and hdr.count("\"16-bit YUV frames\" below") == 2, "the two 8-bit sections say where words live"
    for left_out in ("different depths on the two sides", "big-endian words", "v210", "uint16-fused"):
        assert left_out in hdr, left_out
    # struct w2xc_yuv16_planes: w2xc_yuv_planes and one more int
    assert [f[0] for f in w2xc.Yuv16Planes._fields_] == [f[0] for f in w2xc.YuvPlanes._fields_] + ["pack"]
    assert C.sizeof(w2xc.Yuv16Planes) == C.sizeof(w2xc.YuvPlanes) == 64 and w2xc.Yuv16Planes.pack.offset == w2xc.YuvPlanes.c_px.offset + 4
    # the ABI stays
    assert C.sizeof(w2xc.Opts) == 56 and w2xc.make_opts().struct_size == 56
    assert w2xc.lib().w2xc_version() == b"w2xc_hip 0.4.1.6.1 (gfx950)"


def test_wrapper_keywords(w2xc):
    for name, old in (("process_frames_yuv_u16", "process_frames_yuv_u8"), ("process_frames_yuv_u16_rgb", "process_frames_yuv_u8_rgb")):
        new, ref = inspect.signature(getattr(w2xc, name)).parameters, inspect.signature(getattr(w2xc, old)).parameters
        assert list(new)[:len(ref)] == list(ref) and list(new)[len(ref):] == ["depth", "pack", "out_pack"], name
        assert all(new[k].default == ref[k].default for k in ref), name
    for name, old in (("process_frames_yuv_u16_device", "process_frames_yuv_u8_device"), ("process_frames_yuv_u16_rgb_device", "process_frames_yuv_u8_rgb_device")):
        new, ref = inspect.signature(getattr(w2xc, name)).parameters, inspect.signature(getattr(w2xc, old)).parameters
        assert list(new) == list(ref) + ["depth"], name
    with pytest.raises(ValueError, match="uint16"):
        w2xc.process_frames_yuv_u16(np.zeros((1, 4, 4), np.uint8), chroma=w2xc.YUV_400)
    with pytest.raises(ValueError, match="u and v"):
        w2xc.process_frames_yuv_u16(np.zeros((1, 4, 4), np.uint16))
    with pytest.raises(ValueError, match="uv must be"):
        w2xc.process_frames_yuv_u16_rgb(np.zeros((1, 4, 4), np.uint16), uv=np.zeros((1, 2, 3, 2), np.uint16))


# ---- refusals: all of them before a device is touched (this machine may have none: a call that passes them answers ERR_HIP) ----
class Frames16:
    """host planes of n frames of words and their Yuv16Planes, tight"""

    def __init__(self, w2xc, n, w, h, layout, px=1, pack=0):
        cw, ch = yr.chroma_size(w, h, layout)
        self.y = np.zeros((n, h, w), np.uint16)
        self.c = np.zeros((n, 2, max(ch, 1), max(cw, 1)), np.uint16) if px == 1 else np.zeros((n, max(ch, 1), max(cw, 1), 2), np.uint16)
        s = w2xc.Yuv16Planes()
        s.y, s.y_stride, s.y_frame_stride = self.y.ctypes.data, 2 * w, 2 * w * h
        if px == 1:
            s.u, s.v, s.c_stride, s.c_frame_stride = self.c.ctypes.data, self.c.ctypes.data + self.c.strides[1], 2 * max(cw, 1), self.c.strides[0]
        else:
            s.u, s.v, s.c_stride, s.c_frame_stride = self.c.ctypes.data, self.c.ctypes.data + 2, 4 * max(cw, 1), self.c.strides[0]
        s.c_px, s.pack = px, pack
        self.s = s


def call16(w2xc, rgb, device, noise, scale, n, w, h, layout, rng, depth, i, o, iterations, matrix=1):
    h_ = lambda m: m.handle if m is not None else None
    pi = C.byref(i) if i is not None else None
    po = C.byref(o) if o is not None else None
    lib = w2xc.lib()
    head = (h_(noise), h_(scale), n, w, h, layout, rng, depth) + ((matrix,) if rgb else ())
    if device:
        return (lib.w2xc_process_frames_yuv_u16_rgb_device if rgb else lib.w2xc_process_frames_yuv_u16_device)(*head, pi, po, iterations, None, None)
    return (lib.w2xc_process_frames_yuv_u16_rgb if rgb else lib.w2xc_process_frames_yuv_u16)(*head, pi, po, iterations, None)


def broken(w2xc, side, **kw):
    t = w2xc.Yuv16Planes()
    C.memmove(C.byref(t), C.byref(side), C.sizeof(t))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


@pytest.mark.parametrize("rgb", [False, True], ids=["y", "rgb"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_frame_call_refusals(w2xc, models, device, rgb):
    N, S = (models["rgb_noise"], models["rgb_scale"]) if rgb else (models["noise"], models["scale"])
    n, w, h, lay, D = 2, 17, 9, yr.YUV_420, 10
    i, o, o0 = Frames16(w2xc, n, w, h, lay), Frames16(w2xc, n, 2 * w, 2 * h, lay, pack=1), Frames16(w2xc, n, w, h, lay)
    run = lambda *a, **k: call16(w2xc, rgb, device, *a, **k)
    bk = lambda side, **kw: broken(w2xc, side, **kw)
    A, P, U = w2xc.ERR_ARG, w2xc.ERR_PLANES, w2xc.ERR_UNSUPPORTED
    # (the planes are host memory: the device form is given good arguments only where no device can be reached)
    passes = not (device and w2xc.device_count() > 0)
    good = (w2xc.ERR_HIP,) if w2xc.device_count() <= 0 else (w2xc.OK,)
    if passes:
        assert run(N, S, n, w, h, lay, yr.LIMITED, D, i.s, o.s, 1) in good, w2xc.last_error()
        assert run(N, None, n, w, h, lay, yr.FULL, 16, i.s, o0.s, 0) in good, w2xc.last_error()
        assert run(N, S, n, w, h, lay, yr.FULL, 8, i.s, o.s, 1) in good, w2xc.last_error()
    # what the 8-bit call refuses, with its code: the models
    if rgb:
        assert run(models["noise"], S, n, w, h, lay, 0, D, i.s, o.s, 1) == P and run(N, models["scale"], n, w, h, lay, 0, D, i.s, o.s, 1) == P
        assert run(models["head3"], S, n, w, h, lay, 0, D, i.s, o.s, 1) == U, "a head model as noise model"
        assert run(N, S, n, w, h, yr.YUV_400, 0, D, i.s, o.s, 1) == A and "w2xc_process_frames_yuv_u16*" in w2xc.last_error()
        for m in (-1, 3):
            assert run(N, S, n, w, h, lay, 0, D, i.s, o.s, 1, matrix=m) == A
        if passes:
            assert run(N, models["head3"], n, w, h, lay, 0, D, i.s, o.s, 1) in good, w2xc.last_error()
    else:
        assert run(models["rgb_noise"], S, n, w, h, lay, 0, D, i.s, o.s, 1) == P and run(N, models["rgb_scale"], n, w, h, lay, 0, D, i.s, o.s, 1) == P
        assert run(N, models["head1"], n, w, h, lay, 0, D, i.s, o.s, 1) == U and "upconv head" in w2xc.last_error()
        if passes:
            assert run(N, S, n, w, h, yr.YUV_400, 0, D, bk(i.s, u=None, v=None, c_px=77), bk(o.s, u=None, v=None, c_px=0), 1) in good, w2xc.last_error()
    assert run(None, None, n, w, h, lay, 0, D, i.s, o.s, 1) == A and run(N, None, n, w, h, lay, 0, D, i.s, o.s, 1) == A
    assert run(None, S, n, w, h, lay, 0, D, i.s, o0.s, 0) == A
    for it in (-1, 2):
        assert run(N, S, n, w, h, lay, 0, D, i.s, o.s, it) == A
    assert run(N, S, 0, w, h, lay, 0, D, i.s, o.s, 1) == A and run(N, S, n, 0, h, lay, 0, D, i.s, o.s, 1) == A and run(N, S, n, w, -1, lay, 0, D, i.s, o.s, 1) == A
    assert run(N, S, n, w, h, 4, 0, D, i.s, o.s, 1) == A and run(N, S, n, w, h, lay, 2, D, i.s, o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, D, None, o.s, 1) == A and run(N, S, n, w, h, lay, 0, D, i.s, None, 1) == A
    for field in ("y", "u", "v"):
        assert run(N, S, n, w, h, lay, 0, D, bk(i.s, **{field: None}), o.s, 1) == A and run(N, S, n, w, h, lay, 0, D, i.s, bk(o.s, **{field: None}), 1) == A
    for px in (0, 3):
        assert run(N, S, n, w, h, lay, 0, D, bk(i.s, c_px=px), o.s, 1) == A and run(N, S, n, w, h, lay, 0, D, i.s, bk(o.s, c_px=px), 1) == A
    assert run(N, S, n, w, h, lay, 0, D, i.s, bk(o.s, y=i.s.y), 1) == A and run(N, S, n, w, h, lay, 0, D, i.s, bk(o.s, v=o.s.u), 1) == A     # overlaps
    # the new refusals: depth, pack, odd pointers, odd strides, strides below the row at 2 bytes per sample
    for d in (7, 17, 0, -1):
        assert run(N, S, n, w, h, lay, 0, d, i.s, o.s, 1) == A and "depth" in w2xc.last_error()
    for pk in (2, -1):
        assert run(N, S, n, w, h, lay, 0, D, bk(i.s, pack=pk), o.s, 1) == A and "pack" in w2xc.last_error()
        assert run(N, S, n, w, h, lay, 0, D, i.s, bk(o.s, pack=pk), 1) == A
    cw, ch = yr.chroma_size(w, h, lay)
    for field in ("y", "u", "v"):
        assert run(N, S, n, w, h, lay, 0, D, bk(i.s, **{field: getattr(i.s, field) + 1}), o.s, 1) == A, field
        assert run(N, S, n, w, h, lay, 0, D, i.s, bk(o.s, **{field: getattr(o.s, field) + 1}), 1) == A, field
    big = Frames16(w2xc, n, 2 * w + 4, 2 * h + 4, lay)      # (room for wider strides)
    bi, bo = bk(big.s, y_stride=2 * w + 2, y_frame_stride=(2 * w + 2) * h, c_stride=2 * cw + 2, c_frame_stride=(2 * cw + 2) * ch * 2), o.s
    if passes:
        assert run(N, S, n, w, h, lay, 0, D, bi, bo, 1) in good, w2xc.last_error()
    assert run(N, S, n, w, h, lay, 0, D, bk(bi, y_stride=2 * w + 1), bo, 1) == A and run(N, S, n, w, h, lay, 0, D, bk(bi, c_stride=2 * cw + 1), bo, 1) == A
    assert run(N, S, n, w, h, lay, 0, D, bk(bi, y_frame_stride=(2 * w + 2) * h + 1), bo, 1) == A
    assert run(N, S, n, w, h, lay, 0, D, bk(bi, c_frame_stride=(2 * cw + 2) * ch * 2 + 1), bo, 1) == A
    assert run(N, S, n, w, h, lay, 0, D, bk(i.s, y_stride=2 * w - 2), o.s, 1) == A, "w samples are 2 w bytes"
    assert run(N, S, n, w, h, lay, 0, D, bk(i.s, y_stride=w), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, D, bk(i.s, c_stride=2 * cw - 2), o.s, 1) == A and run(N, S, n, w, h, lay, 0, D, i.s, bk(o.s, c_stride=2 * w - 2), 1) == A
    assert run(N, S, n, w, h, lay, 0, D, bk(i.s, y_frame_stride=2 * w * h - 2), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, D, bk(i.s, c_px=2), o.s, 1) == A, "interleaved chroma needs rows of 2 (2 (cw - 1) + 1) bytes"
    if not device:   # host planes with c_px = 2: P010, v = u +- 1 SAMPLE
        i2 = Frames16(w2xc, n, w, h, lay, px=2, pack=1)
        if passes:
            assert run(N, S, n, w, h, lay, 0, D, i2.s, o.s, 1) in good and run(N, S, n, w, h, lay, 0, D, bk(i2.s, u=i2.s.v, v=i2.s.u), o.s, 1) in good
        assert run(N, S, n, w, h, lay, 0, D, bk(i2.s, v=i2.s.u + 6), o.s, 1) == A and "interleave" in w2xc.last_error()


def test_the_8_bit_calls_refuse_what_they_refused(w2xc, models):
    """the 8-bit frame calls share their checks with the new ones: their refusals and their passes stay"""
    import test_yuv_api as t8
    n, w, h, lay = 2, 17, 9, yr.YUV_420
    i, o = t8.Frames(w2xc, n, w, h, lay), t8.Frames(w2xc, n, 2 * w, 2 * h, lay)
    N, S = models["noise"], models["scale"]
    good = (w2xc.ERR_HIP,) if w2xc.device_count() <= 0 else (w2xc.OK,)
    assert t8.call(w2xc, N, S, n, w, h, lay, yr.LIMITED, i.s, o.s, 1) in good
    odd = w2xc.YuvPlanes()
    C.memmove(C.byref(odd), C.byref(i.s), C.sizeof(odd))
    odd.y_stride, odd.y_frame_stride = w, w * h          # 17 and 153: odd strides are fine for bytes
    assert t8.call(w2xc, N, S, n, w, h, lay, yr.LIMITED, odd, o.s, 1) in good
    assert t8.call(w2xc, models["rgb_noise"], S, n, w, h, lay, 0, i.s, o.s, 1) == w2xc.ERR_PLANES
    assert t8.call(w2xc, N, S, n, w, h, lay, 0, None, o.s, 1) == w2xc.ERR_ARG
    lib = w2xc.lib()
    h_ = lambda m: m.handle
    R, RS = models["rgb_noise"], models["rgb_scale"]
    assert lib.w2xc_process_frames_yuv_u8_rgb(h_(R), h_(RS), n, w, h, lay, 0, 1, C.byref(i.s), C.byref(o.s), 1, None) in good
    assert lib.w2xc_process_frames_yuv_u8_rgb(h_(R), h_(RS), n, w, h, yr.YUV_400, 0, 1, C.byref(i.s), C.byref(o.s), 1, None) == w2xc.ERR_ARG
    assert "w2xc_process_frames_yuv_u8*" in w2xc.last_error()
    assert lib.w2xc_process_frames_yuv_u8_rgb(h_(R), h_(RS), n, w, h, lay, 0, 3, C.byref(i.s), C.byref(o.s), 1, None) == w2xc.ERR_ARG
    assert lib.w2xc_yuv8_to_rgb_device(None, 1, w, h, lay, 0, 1, 1 << 20, 4096, 1024, None) == w2xc.ERR_ARG


def test_block_refusals(w2xc):
    lib = w2xc.lib()
    A = w2xc.ERR_ARG
    b, f = np.zeros(8192, np.uint16), np.zeros(8192, np.float32)
    pb, pf = b.ctypes.data, f.ctypes.data
    w, h, D = 8, 4, 10
    y16_ = lambda *a: lib.w2xc_y16_to_plane_device(*a, None)
    #      src  n  frame row  w  h  range depth pack dst plane
    assert y16_(None, 1, 64, 16, w, h, 0, D, 0, pf, 128) == A and y16_(pb, 1, 64, 16, w, h, 0, D, 0, None, 128) == A
    assert y16_(pb, 0, 64, 16, w, h, 0, D, 0, pf, 128) == A and y16_(pb, 1, 64, 16, 0, h, 0, D, 0, pf, 128) == A and y16_(pb, 1, 64, 16, w, 0, 0, D, 0, pf, 128) == A
    assert y16_(pb, 1, 64, 14, w, h, 0, D, 0, pf, 128) == A, "a stride below 2 w bytes"
    assert y16_(pb, 2, 62, 16, w, h, 0, D, 0, pf, 128) == A and y16_(pb, 2, 64, 16, w, h, 0, D, 0, pf, 124) == A
    assert y16_(pb, 1, 64, 16, w, h, 2, D, 0, pf, 128) == A and y16_(pb, 1, 64, 16, w, h, 0, D, 0, pf, 130) == A
    assert y16_(pb, 1, 64, 16, w, h, 0, 7, 0, pf, 128) == A and y16_(pb, 1, 64, 16, w, h, 0, 17, 0, pf, 128) == A
    assert y16_(pb, 1, 64, 16, w, h, 0, D, 2, pf, 128) == A and y16_(pb, 1, 64, 16, w, h, 0, D, -1, pf, 128) == A
    assert y16_(pb + 1, 1, 64, 16, w, h, 0, D, 0, pf, 128) == A and y16_(pb, 1, 64, 17, w, h, 0, D, 0, pf, 128) == A and y16_(pb, 2, 65, 16, w, h, 0, D, 0, pf, 128) == A
    p16 = lambda *a: lib.w2xc_plane_to_y16_device(*a, None)
    #     src n plane w  h range depth pack dst frame row
    assert p16(None, 1, 128, w, h, 0, D, 0, pb, 64, 16) == A and p16(pf, 1, 128, w, h, 0, D, 0, None, 64, 16) == A
    assert p16(pf, 1, 128, w, h, 0, D, 0, pb, 64, 14) == A and p16(pf, 1, 128, w, h, 3, D, 0, pb, 64, 16) == A and p16(pf, 2, 124, w, h, 0, D, 0, pb, 64, 16) == A
    assert p16(pf, -1, 128, w, h, 0, D, 0, pb, 64, 16) == A and p16(pf, 1, 128, w, h, 0, 18, 0, pb, 64, 16) == A and p16(pf, 1, 128, w, h, 0, D, 5, pb, 64, 16) == A
    assert p16(pf, 1, 128, w, h, 0, D, 0, pb + 1, 64, 16) == A and p16(pf, 1, 128, w, h, 0, D, 0, pb, 64, 17) == A and p16(pf, 2, 128, w, h, 0, D, 0, pb, 65, 16) == A
    c2 = lambda *a: lib.w2xc_chroma2x_u16_device(*a, None)
    src, dst = pb, pb + 2048
    #      src n frame row px pack cw ch depth dst frame row px pack ow oh
    ok = (src, 1, 64, 16, 1, 0, w, h, D, dst, 256, 32, 1, 1, 16, 8)
    def but(**kw):
        names = ("src", "n", "sframe", "srow", "spx", "spack", "cw", "ch", "depth", "dst", "dframe", "drow", "dpx", "dpack", "ow", "oh")
        a = dict(zip(names, ok))
        a.update(kw)
        return c2(*[a[k] for k in names])
    assert but(src=None) == A and but(dst=None) == A and but(n=0) == A
    for px in (0, 3):
        assert but(spx=px) == A and but(dpx=px) == A
    assert but(ow=17) == A and but(oh=9) == A and but(ow=0) == A, "outside the enlargement"
    assert but(srow=14) == A and but(drow=30) == A and but(spx=2, srow=28) == A and but(dpx=2, drow=60, dframe=512) == A
    assert but(n=2, sframe=62) == A and but(n=2, dframe=254) == A
    assert but(dst=src + 16) == A, "overlap"
    assert but(depth=7) == A and but(depth=17) == A and but(spack=2) == A and but(dpack=-1) == A
    assert but(src=src + 1) == A and but(dst=dst + 1) == A and but(srow=17) == A and but(drow=33) == A and but(n=2, sframe=65) == A and but(n=2, dframe=257) == A
    # the two ends of the RGB route
    fr = Frames16(w2xc, 2, w, h, yr.YUV_420)
    plane = 4 * w * h
    to = lambda s, n=2, ww=w, hh=h, lay=yr.YUV_420, rng=0, d=D, m=1, rgb=pf, is_=3 * plane, ps=plane: lib.w2xc_yuv16_to_rgb_device(
        C.byref(s) if s is not None else None, n, ww, hh, lay, rng, d, m, rgb, is_, ps, None)
    back = lambda s, n=2, ww=w, hh=h, lay=yr.YUV_420, rng=0, d=D, m=1, rgb=pf, is_=3 * plane, ps=plane: lib.w2xc_rgb_to_yuv16_device(
        rgb, is_, ps, n, ww, hh, lay, rng, d, m, C.byref(s) if s is not None else None, None)
    for fn in (to, back):
        assert fn(None) == A and fn(fr.s, rgb=None) == A and fn(fr.s, n=0) == A and fn(fr.s, ww=0) == A and fn(fr.s, hh=-2) == A
        assert fn(fr.s, lay=yr.YUV_400) == A and fn(fr.s, lay=7) == A and fn(fr.s, rng=2) == A and fn(fr.s, m=3) == A
        assert fn(fr.s, d=7) == A and fn(fr.s, d=17) == A
        assert fn(fr.s, ps=plane - 4) == A and fn(fr.s, ps=plane + 2) == A and fn(fr.s, is_=3 * plane - 4) == A
        assert fn(broken(w2xc, fr.s, pack=2)) == A and fn(broken(w2xc, fr.s, y=fr.s.y + 1)) == A and fn(broken(w2xc, fr.s, u=fr.s.u + 1)) == A
        assert fn(broken(w2xc, fr.s, y_stride=2 * w + 1)) == A and fn(broken(w2xc, fr.s, c_stride=2 * (w // 2) - 2)) == A and fn(broken(w2xc, fr.s, c_px=3)) == A
        assert fn(broken(w2xc, fr.s, y=pf)) == A, "the frames on the float planes"


# ---- the restatement ----
def test_depth_8_is_the_8_bit_restatement():
    rng_ = np.random.default_rng(1)
    Y8 = rng_.integers(0, 256, (9, 17), dtype=np.uint8)
    for rng in (yr.FULL, yr.LIMITED):
        a, b = y16.luma_in(Y8, rng, 8), yr.luma_in(Y8, rng)
        assert a.dtype == F32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        x = (rng_.random((9, 17), dtype=np.float32) * F32(1.4) - F32(0.2))
        assert np.array_equal(y16.luma_out(x, rng, 8), yr.luma_out(x, rng))
    C8 = rng_.integers(0, 256, (9, 17), dtype=np.uint8)
    assert np.array_equal(y16.chroma2x(C8, 8), yr.chroma2x(C8)) and np.array_equal(y16.chroma2x(C8, 8, 33, 17), yr.chroma2x(C8, 33, 17))
    for layout in rr.LAYOUTS:
        cw, ch = yr.chroma_size(17, 9, layout)
        U, V = rng_.integers(0, 256, (ch, cw), dtype=np.uint8), rng_.integers(0, 256, (ch, cw), dtype=np.uint8)
        for rng in (yr.FULL, yr.LIMITED):
            for matrix in rr.MATRICES:
                a, b = y16.yuv16_to_rgb(Y8, U, V, layout, rng, matrix, 8), rr.yuv8_to_rgb(Y8, U, V, layout, rng, matrix)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (layout, rng, matrix)
                planes = rng_.random((3, 9, 17), dtype=np.float32) * F32(1.3) - F32(0.15)
                for g, w_ in zip(y16.rgb_to_yuv16(planes, layout, rng, matrix, 8), rr.rgb_to_yuv8(planes, layout, rng, matrix)):
                    assert g.dtype == np.uint16 and np.array_equal(g, w_), (layout, rng, matrix)


@pytest.mark.parametrize("depth", y16.DEPTHS)
def test_every_value_returns_through_both_ends(depth):
    """all 2^D values, both ranges: luma in -> luma out, and the chroma scale and offset of the RGB route, are the identity; neutral chroma stays neutral"""
    M = y16.maxval(depth)
    v = np.arange(M + 1, dtype=np.uint32)
    assert v.size == 1 << depth
    for rng in (yr.FULL, yr.LIMITED):
        y = y16.luma_in(v, rng, depth)
        assert y.dtype == F32 and np.array_equal(y16.luma_out(y, rng, depth), v), (depth, rng)
        c = y16.chroma_in(v.astype(F32), rng, depth)
        assert c.dtype == F32 and np.array_equal(y16.chroma_out(c, rng, depth), v), (depth, rng)
        mid = 128 * y16.step(depth)
        assert c[mid] == 0.0 and y16.chroma_out(np.zeros(3, F32), rng, depth).tolist() == [mid] * 3
    lim = y16.luma_in(v, yr.LIMITED, depth)
    assert lim[16 * y16.step(depth)] == 0.0 and abs(lim[235 * y16.step(depth)] - 1.0) < 1e-6 and y16.luma_in(v, yr.FULL, depth)[M] == 1.0


@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_ties_go_to_even_and_both_clamps_saturate(depth):
    M, s = y16.maxval(depth), y16.step(depth)
    k = np.arange(0, min(M, 4000))
    for rng in (yr.FULL, yr.LIMITED):
        scale, off = (F32(219.0 * s), F32(16.0 * s)) if rng == yr.LIMITED else (F32(float(M)), F32(0.0))
        x = ((k + 0.5 - float(off)) / float(scale)).astype(F32)
        r = x * scale + off
        tie = (r == np.floor(r) + F32(0.5)) & (r > 0) & (r < M)
        assert tie.sum() >= 8, (depth, rng, int(tie.sum()))
        got = y16.luma_out(x, rng, depth).astype(np.int64)
        assert (got[tie] % 2 == 0).all() and (np.abs(got[tie] - r[tie].astype(np.float64)) == 0.5).all()
        big = np.array([-1e10, -3e9, -1.0, -0.08, 1.2, 3.0, 3e9, 1e10], F32)
        assert y16.luma_out(big, rng, depth).tolist() == [0] * 4 + [M] * 4
        assert y16.chroma_out(big, rng, depth).tolist() == [0] * 3 + [y16.chroma_out(F32(-0.08), rng, depth)] + [M] * 4
    board = (np.indices((6, 8)).sum(0) % 2 * M).astype(np.uint16)
    out = y16.chroma2x(board, depth)
    assert out.min() == 0 and out.max() == M, "cubic overshoot saturates at both ends"
    for c in (0, 1, M // 2, M - 1, M):
        assert (y16.chroma2x(np.full((5, 7), c, np.uint16), depth) == c).all()


@pytest.mark.parametrize("depth", y16.DEPTHS)
def test_packings(depth):
    M = y16.maxval(depth)
    v = np.random.default_rng(depth).integers(0, M + 1, 1000).astype(np.uint16)
    v[:2] = (0, M)
    lo, hi = y16.pack_words(v, depth, y16.LOW), y16.pack_words(v, depth, y16.HIGH)
    assert np.array_equal(lo, v) and np.array_equal(hi, (v.astype(np.uint32) << (16 - depth)).astype(np.uint16))
    assert np.array_equal(y16.unpack(lo, depth, y16.LOW), v) and np.array_equal(y16.unpack(hi, depth, y16.HIGH), v)
    junk = np.random.default_rng(depth + 100).integers(0, 1 << 16, 1000).astype(np.uint16)
    if depth < 16:
        # HIGH ignores the low bits, LOW masks the high bits
        assert np.array_equal(y16.unpack(hi | (junk & ((1 << (16 - depth)) - 1)), depth, y16.HIGH), v)
        assert np.array_equal(y16.unpack(lo | (junk & ~np.uint16(M)), depth, y16.LOW), v)
        assert ((hi & ((1 << (16 - depth)) - 1)) == 0).all() and ((lo >> depth) == 0).all()
    else:
        assert np.array_equal(lo, hi), "at 16 bits the two packings are the same"


def test_the_kernels_share_one_definition_of_the_arithmetic():
    """lerp31, clamp01, to_ycc, chroma_row_sum and the matrix constants live in w2xc_yuv_px.h alone; cubic_coeffs in w2xc_px.h alone"""
    px = open(os.path.join(CSRC, "w2xc_yuv_px.h")).read()
    files = {n: open(os.path.join(CSRC, n)).read() for n in ("w2xc_yuv.hip", "w2xc_yuv_rgb.hip", "w2xc_yuv16.hip", "w2xc_yuv16_rgb.hip")}
    for fn in ("float lerp31(", "float clamp01(", "YCC to_ycc(", "float chroma_row_sum(", "bool matrix_weights("):
        assert px.count(fn) == 1, fn
        for name, text in files.items():
            assert fn not in text and '#include "w2xc_yuv_px.h"' in text, (fn, name)
    for name, text in files.items():
        assert "void cubic_coeffs(" not in text, name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in mk and "w2xc_yuv16.o" in mk and "w2xc_yuv16_rgb.o" in mk


# ---- the tool ----
def stream16(w, h, tag, depth, n, seed, extra=b"F30000:1001 Ip A1:1"):
    layout = {"420": yr.YUV_420, "422": yr.YUV_422, "444": yr.YUV_444, "mono": yr.YUV_400}[tag]
    cw, ch = yr.chroma_size(w, h, layout)
    rng = np.random.default_rng(seed)
    ctag = ("mono%d" % depth) if tag == "mono" else "%sp%d" % (tag, depth)
    head = b"YUV4MPEG2 W%d H%d %s C%s\n" % (w, h, extra, ctag.encode())
    frames, body = [], b""
    for _ in range(n):
        f = tuple(rng.integers(0, 1 << depth, s, dtype=np.uint16) for s in ((h, w), (ch, cw), (ch, cw)))
        frames.append(f)
        body += b"FRAME\n" + b"".join(a.astype("<u2").tobytes() for a in f)
    return head + body, frames, layout


@pytest.mark.parametrize("depth", [9, 10, 12, 14, 16])
@pytest.mark.parametrize("tag", ["420", "422", "444", "mono"])
def test_y4m16_round_trip(y4m16, tag, depth):
    data, frames, layout = stream16(17, 9, tag, depth, 3, seed=depth)
    fin = io.BytesIO(data)
    hdr = y4m16.y4m.read_header(fin)
    assert y4m16.header_format(hdr) == (layout, depth)
    out = io.BytesIO()
    y4m16.y4m.write_header(out, hdr)
    total = 0
    while True:
        y, u, v = y4m16.read_frames(fin, hdr, 2)
        if y.shape[0] == 0:
            break
        assert y.dtype.itemsize == 2 and (u is None) == (tag == "mono")
        for k in range(y.shape[0]):
            assert np.array_equal(y[k], frames[total + k][0])
            if tag != "mono":
                assert np.array_equal(u[k], frames[total + k][1]) and np.array_equal(v[k], frames[total + k][2])
        total += y.shape[0]
        y4m16.write_frames(out, y, u, v)
    assert total == 3 and out.getvalue() == data, "byte for byte"


def test_y4m16_rewrites_w_and_h(y4m16):
    data, frames, _ = stream16(16, 8, "420", 10, 3, seed=12, extra=b"F25:1 Ip A128:117 XCOLORRANGE=FULL")
    out, seen = io.BytesIO(), []
    def process(y, u, v, layout, full):
        seen.append((y.shape[0], y.dtype.itemsize, layout, full))
        up = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
        return up(y), up(u), up(v)
    assert y4m16.convert_stream(io.BytesIO(data), out, process, 1, "limited", 2) == 3
    assert seen == [(2, 2, yr.YUV_420, True), (1, 2, yr.YUV_420, True)]
    out.seek(0)
    hdr = y4m16.y4m.read_header(out)
    assert (hdr.w, hdr.h) == (32, 16) and hdr.get("F") == "25:1" and hdr.get("A") == "128:117" and hdr.get("C") == "420p10" and hdr.colour_range() == "full"
    y, u, v = y4m16.read_frames(out, hdr, 10)
    assert y.shape == (3, 16, 32) and u.shape == v.shape == (3, 8, 16) and np.array_equal(y[2][::2, ::2], frames[2][0]) and out.read() == b""


def test_y4m16_refusals(y4m16, tmp_path, capsys):
    for tag in ("420jpeg", "420", "422", "444", "mono", "420p8", "420p11", "444alpha", "mono8", "420p10x"):
        with pytest.raises(y4m16.Y4mError):
            y4m16.format_of(tag)
    with pytest.raises(y4m16.Y4mError, match="w2xc_y4m.py"):
        y4m16.header_format(y4m16.y4m.read_header(io.BytesIO(b"YUV4MPEG2 W16 H8\n")))       # no C tag: C420jpeg, 8 bits
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    for field in ("It", "Ib", "Im"):
        data, _, _ = stream16(16, 8, "420", 10, 1, seed=14, extra=b"F25:1 %s A1:1" % field.encode())
        src.write_bytes(data)
        assert y4m16.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path)]) == 2
        assert "interlaced" in capsys.readouterr().err and not dst.exists()
    src.write_bytes(yr.y4m_stream(16, 8, "420mpeg2", 1, seed=15)[0])
    assert y4m16.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path)]) == 2
    err = capsys.readouterr().err
    assert "w2xc_y4m16:" in err and "8-bit streams: tools/w2xc_y4m.py" in err and not dst.exists()
    # and the 8-bit tool goes on refusing words, naming this tool
    with pytest.raises(y4m16.Y4mError, match="w2xc_y4m16.py"):
        y4m16.y4m.read_header(io.BytesIO(b"YUV4MPEG2 W16 H8 C420p10\n")).layout


def test_y4m16_routes_by_model_kind(y4m16):
    """the routing is tools/w2xc_y4m.py's own: one-plane models the Y call, three-plane models (and the upconv schema) the RGB call; Cmono only with Y models"""
    assert y4m16.y4m.model_route(1, 1) == "y" and y4m16.y4m.model_route(None, 3) == "rgb" and y4m16.y4m.model_route(3, None) == "rgb"
    with pytest.raises(y4m16.Y4mError):
        y4m16.y4m.model_route(1, 3)
    with pytest.raises(y4m16.Y4mError):
        y4m16.y4m.check_route("rgb", y4m16.format_of("mono10")[0])
    y4m16.y4m.check_route("y", y4m16.format_of("mono10")[0])
    src = open(os.path.join(ROOT, "tools", "w2xc_y4m16.py")).read()
    assert "y4m.run_tool(" in src and "process_frames_yuv_u16_rgb(" in src and "process_frames_yuv_u16(" in src and "y4m.build_parser(" in src
    opts = {a.dest for a in y4m16.y4m.build_parser()._actions}
    assert {"mode", "noise_level", "model_dir", "range", "matrix", "frames_per_call"} <= opts


# ---- the kernels ----
def test_launch_rules_match_the_launchers():
    src = open(os.path.join(CSRC, "w2xc_kernels.h")).read()
    for name, val in (("W2XC_CHROMA_TQX", y16.TQX), ("W2XC_CHROMA_TQY", y16.TQY), ("W2XC_CHROMA_GRID_MAX", y16.GRID_MAX), ("W2XC_YUVRGB_TCX", rr.TCX),
                      ("W2XC_YUVRGB_TCY", rr.TCY), ("W2XC_YUVRGB_GRID_MAX", rr.GRID_MAX)):
        assert "#define %s %d" % (name, val) in src
    # the two rules are written once, in w2xc_host_geom.hpp, for the launchers of both widths (tests/cpp/host_geom_test.cpp runs them against the expressions
    # the launchers had); here a turn of the chroma kernel is a tile of a FRAME (n, not n * npl)
    squeeze = lambda name: " ".join(open(os.path.join(CSRC, name)).read().split())
    geom, hip = squeeze("w2xc_host_geom.hpp"), squeeze("w2xc_yuv16.hip")
    assert geom.count("yuv_tile_grid((ow / 2 + tqx) / tqx, (oh / 2 + tqy) / tqy, per_tile, cap)") == 1
    assert geom.count("yuv_tile_grid((cw + tcx - 1) / tcx, (ch + tcy - 1) / tcy, n, cap)") == 1
    assert geom.count("turns = tiles * per_tile") == 1 and geom.count("(unsigned)(turns > cap ? cap : turns)") == 1
    assert "chroma2x_tile_grid(ow, oh, n, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX)" in hip and "/ CH_TQX" not in hip
    assert "sizeof(*p.p)" in squeeze("w2xc_yuv_tile.h"), "rows_align: the alignment of a plane's rows in BYTES"
    prologue = squeeze("w2xc_yuv_launch.h")      # (the load paths of the words: one copy for the 2x launcher, every siting, and the resize launcher)
    assert prologue.count("su.px == 1 && ((salign | (sv ? reinterpret_cast<size_t>(sv) : 0)) & 7) == 0") == 1
    assert prologue.count("su.px == 2 && sv == su.p + 1 && (salign & 3) == 0") == 1 and "chroma_prologue_u16(" in hip and "salign" not in hip
    hip = squeeze("w2xc_yuv16_rgb.hip")
    assert hip.count("yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX)") == 2 and "/ YR_TCX" not in hip
    assert y16.chroma_launch(1, 1, 1) == (1, 1) and y16.chroma_launch(63, 31, 2) == (2, 2) and y16.chroma_launch(64, 32, 1) == (4, 4)
    assert y16.chroma_launch(960, 540, 8) == (16 * 17 * 8, 2048), "U and V of a frame are ONE turn"
    assert y16.chroma_load_path(True, 8, False) == 1 and y16.chroma_load_path(True, 4, False) == 0 and y16.chroma_load_path(False, 4, True) == 2
    assert y16.chroma_load_path(False, 2, True) == 0 and y16.chroma_load_path(False, 8, False) == 0
    assert y16.launch is rr.launch


def test_second_trip_shapes_have_more_turns_than_workgroups():
    c = y16.CHROMA_SECOND_TRIP
    turns, grid = y16.chroma_launch(2 * c["cw"], 2 * c["ch"], c["n"])
    assert turns == 2049 > grid == y16.GRID_MAX
    r = y16.RGB_SECOND_TRIP
    turns, grid = y16.launch(r["w"], r["h"], r["layout"], r["n"])
    assert turns == 2 * 1025 > grid == rr.GRID_MAX


def test_new_kernels_no_spill_no_scratch(w2xc):
    lib_dir = os.path.dirname(w2xc.LIB_PATH)
    want = {"w2xc_yuv16.o": {"Y16ToPlane": 1, "PlaneToY16": 1, "ChromaCopy16": 1, "k_chroma2x_u16": 3}, "w2xc_yuv16_rgb.o": {"k_yuv16_to_rgb": 9, "k_rgb_to_yuv16": 3}}
    for obj, kernels in want.items():
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(lib_dir, obj)], capture_output=True, text=True, check=True).stdout
        rows = {}
        for line in out.splitlines():
            m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
            if m:
                rows[m.group(1)] = dict(vspill=int(m.group(4)), sspill=int(m.group(5)), scratch=int(m.group(6)))
        for k, count in kernels.items():
            assert len([n for n in rows if k in n]) == count, (k, sorted(rows))
        assert len(rows) == sum(kernels.values()), sorted(rows)
        for name, r in rows.items():
            assert r == dict(vspill=0, sspill=0, scratch=0), (name, r)
