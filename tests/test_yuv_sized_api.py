"""CPU tests of the sized YUV frame calls (revision 0.4.1.11: w2xc_process_frames_yuv_u8[_rgb]_sized[_device], w2xc_process_frames_yuv_u16[_rgb]_sized[_device]
and the two blocks w2xc_chroma_resize_u8_device / w2xc_chroma_resize_u16_device): the symbols, the header section, the bindings and the ABI that stays; every
refusal, before a device is touched, of the eight calls and the two blocks, and the base calls' refusals unchanged; the NumPy restatement
(tests/yuv_sized_ref.py) against the 2x restatements at r = 0.5, as the identity at r = 1 and on ramps at r = 2 / 3; the window bound of the kernels
(tests/cpp/yuv_sized_geom_test.cpp on w2xc_host_geom.hpp); the y4m tools' --size and --scale_ratio; the new objects' registers.  The GPU side:
tests/test_gpu_yuv_sized_blocks.py, tests/test_gpu_yuv_sized_frames.py."""
import ctypes as C
import inspect
import io
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import yuv_ref as yr
import yuv16_ref as y16
import yuv_sited_ref as sr
import yuv_sized_ref as zr
import test_yuv_api as t8
import test_yuv16_api as t16

F32 = np.float32
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")
models = t16.models                       # the fixture: Y, RGB and head models
FRAME_CALLS = tuple("w2xc_process_frames_yuv_%s%s_sized%s" % (d, r, f) for d in ("u8", "u16") for r in ("", "_rgb") for f in ("", "_device"))
BLOCKS = ("w2xc_chroma_resize_u8_device", "w2xc_chroma_resize_u16_device")
SITINGS = (0, sr.COSITED_X, sr.COSITED_Y, sr.COSITED_X | sr.COSITED_Y)


@pytest.fixture(scope="module")
def y4m():
    return t16.load_tool("w2xc_y4m")


@pytest.fixture(scope="module")
def y4m16():
    return t16.load_tool("w2xc_y4m16")


# ---- the boundary ----
def test_symbols_header_bindings_and_the_abi(w2xc):
    lib = C.CDLL(w2xc.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    assert len(FRAME_CALLS) == 8
    for name in FRAME_CALLS + BLOCKS:
        assert hasattr(lib, name) and name in w2xc.ABI_SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(w2xc, name[len("w2xc_"):]), name
    assert w2xc.ITERATIONS_AUTO == zr.ITERATIONS_AUTO == -1 and re.search(r"#define\s+W2XC_ITERATIONS_AUTO\s+\(-1\)", hdr)
    # the section: behind "Chroma siting", once, with the arithmetic written out and its own Left out
    at = hdr.index("Sized YUV frames (revision 0.4.1.11)")
    assert at > hdr.index("Chroma siting (revision 0.4.1.10)") and hdr.count("Sized YUV frames (revision 0.4.1.11)") == 1
    section = hdr[at:hdr.index("the building blocks on contiguous float planes")]
    flat = " ".join(section.replace("\n *", " ").split())
    for phrase in ("pos = (m + o) * r - o", "s = floor(pos)", "t = (float)(pos - s)", "r = (double)w / out_w", "0.25 on a co-sited one", "w <= out_w <= W and h <= out_h <= H",
                   "the smallest k with (w << k) >= out_w and (h << k) >= out_h", "exactly (0, 1, 0, 0)", "w2xc_resize_linear_device", "w2xc_convert_batch_device with nn2x = 1",
                   "before a device is touched", "DEFINED", "byte for byte, what the base call gives", "35 x 19"):
        assert phrase in flat, phrase
    left_out = flat[flat.index("Left out:"):flat.index("#define")]
    for item in ("output smaller than the input", "antialiasing", "shrink-and-quantise", "TTA", "different depths or sitings", "multi-device striping", "submit / wait"):
        assert item in left_out, item
    # the older sections keep their lists and point here
    assert hdr.count("\"Sized YUV frames\" below") == 4 and "\"Sized YUV frames\" below" not in section
    assert " ".join(hdr[:at].replace("\n *", " ").split()).count("more than one 2x step") == 4, "the earlier sections' lists stay as history"
    # each sized call is its base call with out_w, out_h in front of the output planes
    proto = lambda name: " ".join(re.search(r"\bint %s\(([^;]*)\);" % name, hdr).group(1).split())
    for name in FRAME_CALLS:
        base = name.replace("_sized", "")
        out = "d_out" if name.endswith("_device") else "out"
        planes = "w2xc_yuv16_planes" if "u16" in name else "w2xc_yuv_planes"
        assert proto(name) == proto(base).replace("const %s *%s," % (planes, out), "int out_w, int out_h, const %s *%s," % (planes, out)), name
    for name, twin in zip(BLOCKS, ("w2xc_chroma2x_u8_sited_device", "w2xc_chroma2x_u16_sited_device")):
        assert proto(name) == proto(twin).replace("int oh, int cosited,", "int oh, int w, int h, int out_w, int out_h, int sub_x, int sub_y, int cosited,"), name
    # the ABI stays
    assert C.sizeof(w2xc.Opts) == 56 and w2xc.make_opts().struct_size == 56
    assert w2xc.lib().w2xc_version() == b"w2xc_hip 0.4.1.6.1 (gfx950)"
    assert C.sizeof(w2xc.Yuv16Planes) == C.sizeof(w2xc.YuvPlanes) == 64


def test_wrapper_arguments(w2xc):
    for name in ("process_frames_yuv_u8", "process_frames_yuv_u8_rgb", "process_frames_yuv_u16", "process_frames_yuv_u16_rgb"):
        new, ref = inspect.signature(getattr(w2xc, name + "_sized")).parameters, inspect.signature(getattr(w2xc, name)).parameters
        assert list(new) == ["y", "out_w", "out_h"] + list(ref)[1:], name
        assert new["iterations"].default == w2xc.ITERATIONS_AUTO
        new, ref = inspect.signature(getattr(w2xc, name + "_sized_device")).parameters, inspect.signature(getattr(w2xc, name + "_device")).parameters
        at = list(ref).index("d_out")
        assert list(new) == list(ref)[:at] + ["out_w", "out_h"] + list(ref)[at:], name
    for new, old in (("chroma_resize_u8_device", "chroma2x_u8_sited_device"), ("chroma_resize_u16_device", "chroma2x_u16_sited_device")):
        a, b = list(inspect.signature(getattr(w2xc, new)).parameters), list(inspect.signature(getattr(w2xc, old)).parameters)
        assert a == b[:-2] + ["w", "h", "out_w", "out_h", "sub_x", "sub_y", "cosited", "stream"], new
    for case in ((1280, 720, 1920, 1080, 1), (960, 540, 3840, 2160, 2), (720, 480, 1920, 1080, 2), (1440, 1080, 3840, 2160, 2), (64, 64, 64, 64, 0), (64, 64, 65, 64, 1),
                 (10, 10, 160, 160, 4), (10, 10, 161, 10, 5), (3, 5, 4, 9, 1)):
        assert w2xc.sized_iterations(*case[:4]) == zr.auto_iterations(*case[:4]) == case[4], case


# ---- refusals, all before a device is touched (without a device a call that passes the checks answers ERR_HIP) ----
def sized_call(w2xc, bits, rgb, device, noise, scale, n, w, h, layout, i, out_w, out_h, o, iterations, rng=1, depth=10, matrix=1):
    h_ = lambda m: m.handle if m is not None else None
    lib = w2xc.lib()
    fn = getattr(lib, "w2xc_process_frames_yuv_u%d%s_sized%s" % (bits, "_rgb" if rgb else "", "_device" if device else ""))
    head = (h_(noise), h_(scale), n, w, h, layout, rng) + ((depth,) if bits == 16 else ()) + ((matrix,) if rgb else ())
    pi, po = (C.byref(i) if i is not None else None), (C.byref(o) if o is not None else None)
    return fn(*head, pi, out_w, out_h, po, iterations, None, None) if device else fn(*head, pi, out_w, out_h, po, iterations, None)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("rgb", [False, True], ids=["y", "rgb"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sized_frame_call_refusals(w2xc, models, device, rgb, bits):
    N, S = (models["rgb_noise"], models["rgb_scale"]) if rgb else (models["noise"], models["scale"])
    n, w, h, lay = 2, 17, 9, yr.YUV_420
    F = (lambda W, H: t8.Frames(w2xc, n, W, H, lay)) if bits == 8 else (lambda W, H: t16.Frames16(w2xc, n, W, H, lay))
    i, big = F(w, h), F(16 * w, 16 * h)          # (output planes large enough for every size tried: tight strides are given per case)
    A, P, U = w2xc.ERR_ARG, w2xc.ERR_PLANES, w2xc.ERR_UNSUPPORTED
    passes = not (device and w2xc.device_count() > 0)          # (host planes: the device form is given good arguments only where no device is reached)
    good = (w2xc.ERR_HIP,) if w2xc.device_count() <= 0 else (w2xc.OK,)

    def run(noise, scale, ow, oh, it, i_=i.s, n_=n, w_=w, h_=h, lay_=lay, **kw):
        o = F(max(ow, 1), max(oh, 1)) if 0 < ow <= 16 * w and 0 < oh <= 16 * h else big
        return sized_call(w2xc, bits, rgb, device, noise, scale, n_, w_, h_, lay_, i_, ow, oh, o.s, it, **kw)

    AUTO = w2xc.ITERATIONS_AUTO
    if passes:
        for ow, oh, it in ((2 * w, 2 * h, 1), (w, h, 0), (w, h, 1), (w + 8, h + 4, 1), (4 * w, 4 * h, 2), (3 * w, 2 * h + 1, 2), (2 * w, 2 * h, 2), (16 * w, 16 * h, 4),
                           (16 * w, h, 4), (w + 1, h, AUTO), (3 * w, 3 * h, AUTO), (w, h, AUTO), (2 * w, 4 * h, AUTO), (9 * w, 9 * h, AUTO)):
            assert run(N, S, ow, oh, it) in good, (ow, oh, it, w2xc.last_error())
        assert run(N, None, w, h, 0) in good and run(N, None, w, h, AUTO) in good, "no 2x step: a noise model alone will do"
    # each bound of out_w / out_h
    for ow, oh, it in ((w - 1, h, 1), (w, h - 1, 1), (2 * w + 1, 2 * h, 1), (2 * w, 2 * h + 1, 1), (4 * w + 1, 4 * h, 2), (0, h, 1), (w, 0, 1), (-1, -1, 1), (w + 1, h, 0),
                       (w, h + 1, 0), (2 * w, 2 * h, 0), (16 * w + 1, h, 4), (w, 16 * h + 1, 4)):
        assert run(N, S, ow, oh, it) == A and "output size" in w2xc.last_error(), (ow, oh, it, w2xc.last_error())
    # iterations: 0 .. 4 or AUTO; AUTO that four steps do not reach
    for it in (5, -2, 17, -3):
        assert run(N, S, 2 * w, 2 * h, it) == A and "iterations must be 0 .. 4" in w2xc.last_error(), it
    assert run(N, S, 16 * w + 1, h, AUTO) == A and run(N, S, w, 16 * h + 1, AUTO) == A and "iterations must be 0 .. 4" in w2xc.last_error()
    assert run(N, S, w - 1, h, AUTO) == A and "output size" in w2xc.last_error(), "AUTO resolves to 0 and the size is below the input"
    # the models, as before -- about the RESOLVED count
    assert run(None, None, 2 * w, 2 * h, 1) == A and run(N, None, 2 * w, 2 * h, 1) == A and "scale model" in w2xc.last_error()
    assert run(N, None, 2 * w, 2 * h, AUTO) == A and "scale model" in w2xc.last_error()
    assert run(N, None, 3 * w, 3 * h, 2) == A and run(None, S, w, h, 0) == A and run(None, S, w, h, AUTO) == A
    if rgb:
        assert run(models["noise"], S, 2 * w, 2 * h, 1) == P and run(N, models["scale"], 3 * w, 3 * h, 2) == P
        assert run(models["head3"], S, 2 * w, 2 * h, 1) == U, "a head model as noise model"
        assert run(N, S, 2 * w, 2 * h, 1, lay_=yr.YUV_400) == A
        for m in (-1, 3):
            assert run(N, S, 2 * w, 2 * h, 1, matrix=m) == A
        if passes:
            assert run(N, models["head3"], 3 * w, 3 * h, 2) in good, w2xc.last_error()
    else:
        assert run(models["rgb_noise"], S, 2 * w, 2 * h, 1) == P and run(N, models["head1"], 3 * w, 3 * h, 2) == U
    # everything else the base call refuses
    assert run(N, S, 2 * w, 2 * h, 1, n_=0) == A and run(N, S, 2 * w, 2 * h, 1, w_=0) == A and run(N, S, 2 * w, 2 * h, 1, h_=-1) == A
    assert run(N, S, 2 * w, 2 * h, 1, w_=(1 << 22) + 1) == A
    assert run(N, S, 2 * w, 2 * h, 1, lay_=4) == A and run(N, S, 2 * w, 2 * h, 1, rng=2) == A and run(N, S, 2 * w, 2 * h, 1, lay_=yr.YUV_444 | 0x10) == A
    assert run(N, S, 2 * w, 2 * h, 1, i_=None) == A
    o = F(3 * w, 3 * h)
    mk = t16.broken if bits == 16 else (lambda w2, side, **kw: _broken8(w2, side, **kw))
    assert sized_call(w2xc, bits, rgb, device, N, S, n, w, h, lay, i.s, 3 * w, 3 * h, None, 2) == A
    for field in ("y", "u", "v"):
        assert sized_call(w2xc, bits, rgb, device, N, S, n, w, h, lay, i.s, 3 * w, 3 * h, mk(w2xc, o.s, **{field: None}), 2) == A
    assert sized_call(w2xc, bits, rgb, device, N, S, n, w, h, lay, i.s, 3 * w, 3 * h, mk(w2xc, o.s, c_px=3), 2) == A
    assert sized_call(w2xc, bits, rgb, device, N, S, n, w, h, lay, i.s, 3 * w, 3 * h, mk(w2xc, o.s, y=i.s.y), 2) == A, "overlap"
    # the output planes are those of an out_w x out_h frame: strides below ITS rows are refused, its own pass
    unit = bits // 8
    ocw = (3 * w + 1) // 2
    assert sized_call(w2xc, bits, rgb, device, N, S, n, w, h, lay, i.s, 3 * w, 3 * h, mk(w2xc, o.s, y_stride=unit * (3 * w - 1)), 2) == A
    assert sized_call(w2xc, bits, rgb, device, N, S, n, w, h, lay, i.s, 3 * w, 3 * h, mk(w2xc, o.s, c_stride=unit * (ocw - 1)), 2) == A
    small = F(2 * w, 2 * h)
    assert sized_call(w2xc, bits, rgb, device, N, S, n, w, h, lay, i.s, 3 * w, 3 * h, small.s, 2) == A, "planes of a 2w x 2h frame do not hold a 3w x 3h one"
    if bits == 16:
        for d in (7, 17):
            assert run(N, S, 2 * w, 2 * h, 1, depth=d) == A and "depth" in w2xc.last_error()


def _broken8(w2xc, side, **kw):
    t = w2xc.YuvPlanes()
    C.memmove(C.byref(t), C.byref(side), C.sizeof(t))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_the_base_calls_refuse_what_they_refused(w2xc, models):
    """iterations = 2 (and AUTO's -1) stay refused by all eight base calls, in the words they had"""
    n, w, h, lay = 2, 17, 9, yr.YUV_420
    good = (w2xc.ERR_HIP,) if w2xc.device_count() <= 0 else (w2xc.OK,)
    i8, o8, o84 = t8.Frames(w2xc, n, w, h, lay), t8.Frames(w2xc, n, 2 * w, 2 * h, lay), t8.Frames(w2xc, n, 4 * w, 4 * h, lay)
    i16, o16, o164 = t16.Frames16(w2xc, n, w, h, lay), t16.Frames16(w2xc, n, 2 * w, 2 * h, lay), t16.Frames16(w2xc, n, 4 * w, 4 * h, lay)
    lib, h_ = w2xc.lib(), (lambda m: m.handle)
    for device in (False, True):
        for rgb in (False, True):
            N, S = (models["rgb_noise"], models["rgb_scale"]) if rgb else (models["noise"], models["scale"])
            fn8 = getattr(lib, "w2xc_process_frames_yuv_u8%s%s" % ("_rgb" if rgb else "", "_device" if device else ""))
            tail = (None, None) if device else (None,)
            for it, o in ((2, o84), (-1, o8), (5, o8)):
                head = (h_(N), h_(S), n, w, h, lay, 1) + ((1,) if rgb else ())
                assert fn8(*head, C.byref(i8.s), C.byref(o.s), it, *tail) == w2xc.ERR_ARG and "iterations must be 0 or 1 (got %d)" % it in w2xc.last_error(), (device, rgb, it)
                assert t16.call16(w2xc, rgb, device, N, S, n, w, h, lay, 1, 10, i16.s, (o164 if it == 2 else o16).s, it) == w2xc.ERR_ARG
                assert "iterations must be 0 or 1 (got %d)" % it in w2xc.last_error()
            if not device or w2xc.device_count() <= 0:
                assert t16.call16(w2xc, rgb, device, N, S, n, w, h, lay, 1, 10, i16.s, o16.s, 1) in good, w2xc.last_error()


def test_block_refusals(w2xc):
    lib, A = w2xc.lib(), w2xc.ERR_ARG
    b = np.zeros(16384, np.uint16)
    src, dst = b.ctypes.data, b.ctypes.data + 8192
    cw, ch = 8, 4
    base8 = dict(src=src, n=1, sframe=32, srow=8, spx=1, cw=cw, ch=ch, dst=dst, dframe=256, drow=16, dpx=1, ow=12, oh=6, w=16, h=8, out_w=24, out_h=12, sub_x=1, sub_y=1,
                 cosited=0)
    order8 = list(base8)

    def c8(**kw):
        a = dict(base8, **kw)
        return lib.w2xc_chroma_resize_u8_device(*[a[k] for k in order8], None)

    base16 = dict(src=src, n=1, sframe=64, srow=16, spx=1, spack=0, cw=cw, ch=ch, depth=10, dst=dst, dframe=512, drow=32, dpx=1, dpack=0, ow=12, oh=6, w=16, h=8, out_w=24,
                  out_h=12, sub_x=1, sub_y=1, cosited=0)
    order16 = list(base16)

    def c16(**kw):
        a = dict(base16, **kw)
        return lib.w2xc_chroma_resize_u16_device(*[a[k] for k in order16], None)

    for fn in (c8, c16):
        if w2xc.device_count() <= 0:
            assert fn() == w2xc.ERR_HIP, w2xc.last_error()
            for ok in (dict(cosited=0x30), dict(cosited=0x10, sub_y=0), dict(sub_x=0, sub_y=0), dict(out_w=16, out_h=8), dict(out_w=16 * 16 + 5, out_h=8), dict(ow=1, oh=1),
                       dict(ow=100, oh=3, drow=400 if fn is c16 else 200, dframe=2048)):
                assert fn(**ok) == w2xc.ERR_HIP, (ok, w2xc.last_error())
        # the size rule: the output is never smaller than the input; sizes of at least 1
        for bad in (dict(out_w=15), dict(out_h=7), dict(w=0), dict(h=0), dict(w=-4, out_w=-2), dict(out_w=(1 << 22) + 1), dict(ow=0), dict(oh=0), dict(oh=-1)):
            assert fn(**bad) == A, bad
        assert fn(out_w=15) == A and "never smaller" in w2xc.last_error()
        # the subsampling flags and the siting
        for bad in (dict(sub_x=2), dict(sub_y=-1), dict(cosited=0x10, sub_x=0), dict(cosited=0x20, sub_y=0), dict(cosited=0x30, sub_x=0, sub_y=0), dict(cosited=1),
                    dict(cosited=0x40), dict(cosited=-1)):
            assert fn(**bad) == A, bad
        # what the 2x blocks refuse
        for bad in (dict(src=None), dict(dst=None), dict(n=0), dict(cw=0), dict(ch=0), dict(spx=3), dict(dpx=0), dict(srow=7 if fn is c8 else 14), dict(drow=11 if fn is c8 else 22),
                    dict(dst=src), dict(n=2, sframe=8)):
            assert fn(**bad) == A, bad
    assert c16(src=src + 1) == A and c16(dst=dst + 1) == A and c16(srow=17) == A and c16(drow=33) == A and c16(depth=7) == A and c16(depth=17) == A
    assert c16(spack=2) == A and c16(dpack=-1) == A


# ---- the restatement ----
def test_half_ratio_is_the_2x_restatement():
    """r = 0.5: every output sample, column 0 and the crop included, for all four siting combinations, on sizes 1 .. 9 and on tile-edge sizes"""
    r = np.random.default_rng(11)
    sizes = [(w, h) for w in range(1, 10) for h in (1, 2, 5, 9)] + [(31, 15), (32, 16), (33, 17), (63, 31), (64, 32), (65, 33), (129, 3)]
    for w, h in sizes:
        for cosited in SITINGS:
            cw, ch = yr.chroma_size(w, h, yr.YUV_420)
            ocw, och = yr.chroma_size(2 * w, 2 * h, yr.YUV_420)
            c8 = r.integers(0, 256, (ch, cw), dtype=np.uint8)
            got = zr.chroma_resize(c8, ocw, och, w, h, 2 * w, 2 * h, 1, 1, cosited)
            assert got.dtype == np.uint8 and np.array_equal(got, sr.chroma2x(c8, cosited, 8, ocw, och)), (w, h, cosited)
            if not cosited:
                assert np.array_equal(got, yr.chroma2x(c8, ocw, och))
            cd = r.integers(0, 1 << 10, (ch, cw)).astype(np.uint16)
            assert np.array_equal(zr.chroma_resize(cd, ocw, och, w, h, 2 * w, 2 * h, 1, 1, cosited, 10), sr.chroma2x(cd, cosited, 10, ocw, och)), (w, h, cosited)
    # the positions themselves
    for o, (t_odd, t_even) in ((0.5, (0.25, 0.75)), (0.25, (0.375, 0.875))):
        s, t = zr.positions(40, 20, 40, o)
        m = np.arange(40)
        assert np.array_equal(s, (m + 1) // 2 - 1) and (t[1::2] == F32(t_odd)).all() and (t[0::2] == F32(t_even)).all()
    # 4:2:2 and 4:4:4 through the frame's rule: an axis that is not subsampled has o = 0.5 whatever the flags, and sizes follow the layout
    c = r.integers(0, 256, (9, 7), dtype=np.uint8)
    assert np.array_equal(zr.frame_chroma(c, 13, 9, 26, 18, sr.YUV_422_LEFT), sr.chroma2x(c, sr.COSITED_X, 8, 13, 18))
    c = r.integers(0, 256, (9, 13), dtype=np.uint8)
    assert np.array_equal(zr.frame_chroma(c, 13, 9, 26, 18, yr.YUV_444), yr.chroma2x(c, 26, 18))


def test_unit_ratio_is_the_identity():
    """r = 1: t = 0, cubic_coeffs(0) is exactly (0, 1, 0, 0) and every value returns: all 256 bytes, all values of depths 10 and 16"""
    c = yr.cubic_coeffs(F32(0.0))
    assert [float(x) for x in c] == [0.0, 1.0, 0.0, 0.0]
    for o in (0.5, 0.25):
        s, t = zr.positions(50, 99, 99, o)
        assert np.array_equal(s, np.arange(50)) and (t == 0).all()
    b = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for cosited in SITINGS:
        assert np.array_equal(zr.chroma_resize(b, 16, 16, 32, 32, 32, 32, 1, 1, cosited), b)
    for depth in (10, 16):
        v = np.arange(1 << depth).astype(np.uint16).reshape(-1, 256)
        assert np.array_equal(zr.chroma_resize(v, 256, v.shape[0], 512, 2 * v.shape[0], 512, 2 * v.shape[0], 1, 1, 0, depth), v)
    # one axis at r = 1, the other enlarged: the rows are those of the 1-D case
    p = np.random.default_rng(2).integers(0, 256, (6, 10), dtype=np.uint8)
    wide = zr.chroma_resize(p, 15, 6, 20, 12, 30, 12, 1, 1, 0)
    order = np.array([3, 0, 5, 1, 4, 2])
    assert wide.shape == (6, 15) and np.array_equal(zr.chroma_resize(p[order], 15, 6, 20, 12, 30, 12, 1, 1, 0), wide[order]), "r = 1 in y: a row comes from its own row alone"
    tall = zr.chroma_resize(p, 10, 9, 20, 12, 20, 18, 1, 1, sr.COSITED_Y)
    assert tall.shape == (9, 10) and np.array_equal(zr.chroma_resize(p[:, ::-1], 10, 9, 20, 12, 20, 18, 1, 1, sr.COSITED_Y), tall[:, ::-1])


def test_ramps_at_two_thirds():
    """r = 2 / 3 (720p -> 1080p): C[k] = 40 + 6 k.  Output m sits at source (m + o) * 2 / 3 - o: 40 + 4 m + 6 (2 o / 3 - o) = 40 + 4 m - 2 o -- 39 centred, 39.5 co-sited,
    before Keys' cubic (A = -0.75) adds its ripple of less than half a step and the rounding; constants stay put; the slope is 4 per output sample"""
    k = np.arange(40)
    m = np.arange(6, 48)
    for depth in (8, 10):
        ramp = (40 + 6 * k).astype(np.uint8 if depth == 8 else np.uint16)
        for cosited in SITINGS:
            for axis, bit in ((1, sr.COSITED_X), (0, sr.COSITED_Y)):
                plane = np.tile(ramp, (8, 1)) if axis == 1 else np.tile(ramp[:, None], (1, 8))
                w, h = (80, 16) if axis == 1 else (16, 80)
                ow, oh = (60, 8) if axis == 1 else (8, 60)
                out_w, out_h = (120, 16) if axis == 1 else (16, 120)
                up = zr.chroma_resize(plane, ow, oh, w, h, out_w, out_h, 1, 1, cosited, depth).astype(int)
                line = np.take(np.take(up, m, axis=axis), 3, axis=1 - axis)
                ideal = 40 + 4 * m - 2 * (0.25 if cosited & bit else 0.5)
                assert np.abs(line - ideal).max() <= 1.0, (depth, cosited, axis, line - ideal)
                assert np.array_equal(np.diff(line[::3]), np.full(len(line[::3]) - 1, 12)), "the pattern repeats every 3 outputs = 2 sources = 12 steps"
                assert (np.take(up, m, axis=axis) == np.expand_dims(line, 1 - axis)).all(), "constant along the other axis (r = 1 there)"
        for value in (0, 1, 128, (1 << depth) - 2, (1 << depth) - 1):
            plane = np.full((7, 9), value, np.uint16)
            assert (zr.chroma_resize(plane, 13, 10, 18, 14, 27, 21, 1, 1, sr.COSITED_X, depth) == value).all()
    # a checkerboard overshoots and saturates at both ends
    board = (np.indices((20, 30)).sum(0) % 2 * 255).astype(np.uint8)
    out = zr.chroma_resize(board, 45, 30, 60, 40, 90, 60)
    assert out.min() == 0 and out.max() == 255
    pre = zr.resize_cubic(board.astype(F32) * F32(1.0 / 255.0), 45, 30, 60, 40, 90, 60, 0.5, 0.5)
    assert pre.min() < -0.05 and pre.max() > 1.05, "the overshoot the clamp is there for"


def test_auto_and_the_size_rule():
    for w, h, ow, oh, k in ((1280, 720, 1920, 1080, 1), (1920, 1080, 3840, 2160, 1), (960, 540, 3840, 2160, 2), (720, 480, 1920, 1080, 2), (1440, 1080, 3840, 2160, 2),
                            (48, 40, 72, 60, 1), (36, 24, 96, 54, 2), (5, 5, 5, 5, 0), (5, 5, 80, 5, 4), (5, 5, 81, 5, 5)):
        assert zr.auto_iterations(w, h, ow, oh) == k
        assert zr.size_ok(w, h, ow, oh, k) == (k <= 4)
        if 0 < k <= 4:
            assert not zr.size_ok(w, h, ow, oh, k - 1), "AUTO is the smallest count that holds the size"
    assert zr.launch(960, 540, 16) == (30 * 34 * 16, 2048) and zr.launch(1, 1, 1) == (1, 1)
    assert zr.launch(zr.SECOND_TRIP["ow"], zr.SECOND_TRIP["oh"], 1) == (2049, 2048)


# ---- the host geometry: the window bound ----
def test_window_bound_and_sized_geometry():
    cpp = os.path.join(ROOT, "tests", "cpp")
    os.makedirs(os.path.join(cpp, "_build"), exist_ok=True)
    exe = os.path.join(cpp, "_build", "yuv_sized_geom_test")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(cpp, "yuv_sized_geom_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all sized-frame geometry properties hold" in r.stdout
    geom = open(os.path.join(CSRC, "w2xc_host_geom.hpp")).read()
    for name in ("chroma_resize_pos(", "chroma_resize_origin(", "chroma_resize_tile_grid(", "sized_auto_iterations(", "chroma_axis("):
        assert name in geom, name
    # the kernels take the rule from there, and the shared arithmetic from its one home
    for f in ("w2xc_yuv_sized.hip", "w2xc_yuv16_sized.hip"):
        text = open(os.path.join(CSRC, f)).read()
        for name in ("chroma_resize_origin(", "chroma_resize_pos(", "chroma_resize_tile_grid(", "cubic_coeffs(", "chroma_row_sum(", "turn += gridDim.x", "CH_LD", "W2XC_CHROMA_GRID_MAX"):
            assert name in text, (f, name)
        for defined_elsewhere in ("void cubic_coeffs(", "float chroma_row_sum(", "to_u8(float", "unsigned to_u16("):
            assert defined_elsewhere not in text, (f, defined_elsewhere)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "w2xc_yuv_sized.o" in mk and "w2xc_yuv16_sized.o" in mk and "-ffp-contract=off" in mk


# ---- the tools ----
def test_tool_options(y4m, y4m16, tmp_path, capsys):
    ap = y4m.build_parser()
    a = ap.parse_args(["a", "b"])
    assert a.size is None and a.scale_ratio is None
    assert ap.parse_args(["a", "b", "--size", "1920x1080"]).size == "1920x1080" and ap.parse_args(["a", "b", "--scale_ratio", "1.5"]).scale_ratio == 1.5
    plan = y4m.output_plan
    # neither option: the tool's old rule, and the base calls
    assert plan(1280, 720, None, None, True, True) == (1, None) and plan(1280, 720, None, None, True, False) == (0, None)
    # --size: AUTO's rule
    assert plan(1280, 720, "1920x1080", None, False, True) == (1, (1920, 1080)) and plan(960, 540, "3840X2160", None, False, True) == (2, (3840, 2160))
    assert plan(720, 480, "1920x1080", None, True, True) == (2, (1920, 1080)) and plan(64, 64, "64x64", None, True, False) == (0, (64, 64))
    assert plan(10, 10, "160x160", None, False, True) == (4, (160, 160))
    for w, h, ow, oh in ((1280, 720, 1920, 1080), (17, 9, 40, 9), (5, 5, 80, 5)):
        assert plan(w, h, "%dx%d" % (ow, oh), None, True, True)[0] == zr.auto_iterations(w, h, ow, oh) == y4m.auto_iterations(w, h, ow, oh)
    # --scale_ratio: the reference's rule
    assert plan(1280, 720, None, 1.5, False, True) == (1, (1920, 1080)) and plan(1280, 720, None, 2.0, False, True) == (1, (2560, 1440))
    assert plan(720, 480, None, 2.25, False, True) == (2, (1620, 1080)) and plan(100, 50, None, 4.0, False, True) == (2, (400, 200))
    assert plan(100, 50, None, 1.0, True, False) == (0, (100, 50)) and plan(101, 51, None, 1.3, True, True) == (1, (131, 66))
    for bad in (lambda: plan(64, 64, "63x64", None, True, True), lambda: plan(64, 64, "64x63", None, True, True), lambda: plan(10, 10, "161x10", None, True, True),
                lambda: plan(64, 64, "64", None, True, True), lambda: plan(64, 64, "0x64", None, True, True), lambda: plan(64, 64, "axb", None, True, True),
                lambda: plan(64, 64, "96x96", 1.5, True, True), lambda: plan(64, 64, None, 0.5, True, True), lambda: plan(64, 64, None, 16.5, True, True),
                lambda: plan(64, 64, None, float("nan"), True, True), lambda: plan(64, 64, "96x96", None, True, False), lambda: plan(64, 64, None, 1.5, True, False),
                lambda: plan(64, 64, None, 1.0, False, True), lambda: plan(64, 64, "64x64", None, False, True)):
        with pytest.raises(y4m.Y4mError):
            bad()
    # the written header follows, in both tools
    data, frames = yr.y4m_stream(16, 8, "420mpeg2", 2, seed=4)
    seen = []

    def process(y, u, v, layout, full):
        seen.append(y.shape)
        n = y.shape[0]
        return np.zeros((n, 12, 24), np.uint8), np.zeros((n, 6, 12), np.uint8), np.ones((n, 6, 12), np.uint8)
    out = io.BytesIO()
    assert y4m.convert_stream(io.BytesIO(data), out, process, 1, size=(24, 12)) == 2 and seen == [(2, 8, 16)]
    out.seek(0)
    hdr = y4m.read_header(out)
    assert (hdr.w, hdr.h) == (24, 12) and hdr.get("C") == "420mpeg2" and hdr.get("F") == "30000:1001" and hdr.get("A") == "1:1"
    y, u, v = y4m.read_frames(out, hdr, 8)
    assert y.shape == (2, 12, 24) and u.shape == (2, 6, 12) and (v == 1).all()
    data16 = t16.stream16(16, 8, "420", 10, 1, seed=5)[0]
    out = io.BytesIO()
    z = lambda *s: np.zeros(s, np.uint16)
    assert y4m16.convert_stream(io.BytesIO(data16), out, lambda y, u, v, layout, full: (z(1, 12, 24), z(1, 6, 12), z(1, 6, 12)), 1, size=(24, 12)) == 1
    out.seek(0)
    hdr = y4m.read_header(out)
    assert (hdr.w, hdr.h) == (24, 12) and hdr.get("C") == "420p10"
    # without the options the header doubles as before
    out = io.BytesIO()
    up = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    assert y4m.convert_stream(io.BytesIO(data), out, lambda y, u, v, layout, full: (up(y), up(u), up(v)), 1) == 2
    out.seek(0)
    hdr = y4m.read_header(out)
    assert (hdr.w, hdr.h) == (32, 16)
    # a size the stream rules out is refused before a model is loaded or the output exists, in both tools' voice
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    assert y4m.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path), "--size", "15x8"]) == 2
    err = capsys.readouterr().err
    assert "w2xc_y4m:" in err and "never smaller" in err and not dst.exists()
    assert y4m.main([str(src), str(dst), "-m", "noise", "--model_dir", str(tmp_path), "--scale_ratio", "1.5"]) == 2
    assert "scale model" in capsys.readouterr().err and not dst.exists()
    src.write_bytes(data16)
    assert y4m16.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path), "--size", "300x8"]) == 2
    err = capsys.readouterr().err
    assert "w2xc_y4m16:" in err and "16 times" in err and not dst.exists()
    for tool, call in ((y4m, "process_frames_yuv_u8_sized"), (y4m16, "process_frames_yuv_u16_sized")):
        text = open(os.path.join(ROOT, "tools", tool.__name__ + ".py")).read()
        assert call in text and call.replace("_sized", "_rgb_sized") in text and "--size" in text and "--scale_ratio" in text


# ---- the kernels ----
def test_resize_kernels_no_spill_no_scratch(w2xc):
    lib_dir = os.path.dirname(w2xc.LIB_PATH)
    want = {"w2xc_yuv_sized.o": {"k_chroma_resize_u8": 2}, "w2xc_yuv16_sized.o": {"k_chroma_resize_u16": 3}}
    twins = {"w2xc_yuv_sized.o": "w2xc_yuv_sited.o", "w2xc_yuv16_sized.o": "w2xc_yuv16_sited.o"}

    def rows_of(obj):
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(lib_dir, obj)], capture_output=True, text=True, check=True).stdout
        rows = {}
        for line in out.splitlines():
            m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+) lds\s+(\d+)", line)
            if m:
                rows[m.group(1)] = dict(vspill=int(m.group(4)), sspill=int(m.group(5)), scratch=int(m.group(6)), vgpr=int(m.group(2)), lds=int(m.group(7)))
        return rows
    for obj, kernels in want.items():
        rows = rows_of(obj)
        for k, count in kernels.items():
            assert len([n for n in rows if k in n]) == count, (k, sorted(rows))
        assert len(rows) == sum(kernels.values()), sorted(rows)
        for name, r in rows.items():
            assert (r["vspill"], r["sspill"], r["scratch"]) == (0, 0, 0), (name, r)
            assert r["vgpr"] <= 64, (name, r)                     # (eight waves a SIMD, as the 2x kernels)
        assert {r["lds"] for r in rows.values()} == {r["lds"] for r in rows_of(twins[obj]).values()}, "the window the 2x kernels stage: 19 rows of 37 floats a plane"
