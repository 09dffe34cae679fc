"""CPU tests of chroma siting (revision 0.4.1.10: the flags W2XC_CHROMA_COSITED_X / _Y in the `chroma` of the eight YUV frame calls and the four ends of the RGB
route, and the two new blocks w2xc_chroma2x_u8_sited_device / w2xc_chroma2x_u16_sited_device): the symbols, the constants, the header section and the ABI that
stays; every refusal, before a device is touched, through all eight frame calls and the six blocks; the NumPy restatement (tests/yuv_sited_ref.py) against the
centred restatements and on ramps, where the siting shows as an offset; the y4m tools' --siting; the launch rules and the new objects' registers.  The GPU side:
tests/test_gpu_yuv_sited_blocks.py, tests/test_gpu_yuv_sited_frames.py."""
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
import yuv_rgb_ref as rr
import yuv16_ref as y16
import yuv_sited_ref as sr
import test_yuv_api as t8
import test_yuv16_api as t16

F32 = np.float32
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")
models = t16.models                       # the fixture: Y, RGB and head models
NEW_SYMBOLS = ("w2xc_chroma2x_u8_sited_device", "w2xc_chroma2x_u16_sited_device")
REFUSED = (-1, 4, 7, 0x40, 0x13 | 0x40, 0x80, 0x100, 0x14, 0x1F,                     # negative, other bits, layouts outside 0 .. 3
           yr.YUV_444 | 0x10, yr.YUV_444 | 0x20, yr.YUV_444 | 0x30, yr.YUV_400 | 0x10, yr.YUV_400 | 0x20, yr.YUV_400 | 0x30,   # no subsampled axis
           yr.YUV_422 | 0x20, yr.YUV_422 | 0x30)                                      # 4:2:2 does not subsample y


@pytest.fixture(scope="module")
def y4m():
    return t16.load_tool("w2xc_y4m")


@pytest.fixture(scope="module")
def y4m16():
    return t16.load_tool("w2xc_y4m16")


# ---- the boundary ----
def test_symbols_constants_header_and_the_abi(w2xc):
    lib = C.CDLL(w2xc.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in w2xc.ABI_SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
    for name in ("chroma2x_u8_sited_device", "chroma2x_u16_sited_device", "CHROMA_COSITED_X", "CHROMA_COSITED_Y", "YUV_420_LEFT", "YUV_420_TOPLEFT", "YUV_422_LEFT"):
        assert hasattr(w2xc, name), name
    assert (w2xc.CHROMA_COSITED_X, w2xc.CHROMA_COSITED_Y) == (sr.COSITED_X, sr.COSITED_Y) == (0x10, 0x20)
    assert (w2xc.YUV_420_LEFT, w2xc.YUV_420_TOPLEFT, w2xc.YUV_422_LEFT) == sr.SITED_LAYOUTS == (0x10, 0x30, 0x11)
    assert re.search(r"#define\s+W2XC_CHROMA_COSITED_X\s+0x10\b", hdr) and re.search(r"#define\s+W2XC_CHROMA_COSITED_Y\s+0x20\b", hdr)
    for name in ("W2XC_YUV_420_LEFT", "W2XC_YUV_420_TOPLEFT", "W2XC_YUV_422_LEFT"):
        assert re.search(r"#define\s+%s\s+\(" % name, hdr), name
    # the new section stands behind the 16-bit one, and the three sections before it are as they were
    at = hdr.index("Chroma siting (revision 0.4.1.10)")
    assert at > hdr.index("16-bit YUV frames (revision 0.4.1.9)") and hdr.count("Chroma siting (revision 0.4.1.10)") == 1
    section = hdr[at:hdr.index("the building blocks on contiguous float planes")]
    assert hdr.count("\"16-bit YUV frames\" below") == 2 and "\"16-bit YUV frames\" below" not in section
    for decimal in ("1.5748", "1.8556", "1.402", "1.772"):
        assert decimal not in section
    flat = " ".join(section.replace("\n *", " ").split())      # (the comment's line breaks taken out)
    for phrase in ("m / 2 - 0.125", "0.375", "0.875", "0.5f * C[j] + 0.5f * C[min(j + 1, last)]", "(l + r) * 0.25f + m * 0.5f", "((a + b) + (c + d)) * 0.25f",
                   "w2xc_chroma2x_u8_sited_device", "before a device is touched"):
        assert phrase in flat, phrase
    left_out = section[section.index("Left out:"):section.index("#define")]
    assert "left-sited" not in left_out and "PAL-DV" in left_out and "TTA" in left_out and "shrink" in left_out
    assert hdr[:at].count("left-sited chroma") >= 3, "the earlier sections' lists stay as they were"
    # the ABI stays
    assert C.sizeof(w2xc.Opts) == 56 and w2xc.make_opts().struct_size == 56
    assert w2xc.lib().w2xc_version() == b"w2xc_hip 0.4.1.6.1 (gfx950)"
    # the Python mirrors of the two blocks: their centred twins' arguments with `cosited` behind `oh`
    for new, old in (("chroma2x_u8_sited_device", "chroma2x_u8_device"), ("chroma2x_u16_sited_device", "chroma2x_u16_device")):
        a, b = list(inspect.signature(getattr(w2xc, new)).parameters), list(inspect.signature(getattr(w2xc, old)).parameters)
        assert a == b[:-1] + ["cosited", "stream"], new
    # sizes do not depend on the flags
    for chroma in sr.ALL_SITED:
        for w, h in ((1, 1), (17, 9), (64, 32)):
            assert w2xc.yuv_chroma_size(w, h, chroma) == yr.chroma_size(w, h, chroma & 0xF) == sr.chroma_size(w, h, chroma)
    with pytest.raises(ValueError):
        w2xc.yuv_chroma_size(8, 8, 7)
    # ... in the launchers either: ONE decoder gives the layout and the flags, frame_geometry takes the layout, and no launcher masks a flag off
    px = open(os.path.join(CSRC, "w2xc_yuv_px.h")).read()
    assert px.count("bool chroma_layout(int chroma, ChromaLayout *c)") == 1 and "bool frame_geometry(int w, int h, int layout," in px
    assert "chroma &= 0xF" not in px and "sited_layout" not in px


def test_the_rule_of_acceptance():
    ok = [c for c in range(-2, 0x82) if sr.accepted(c)]
    assert ok == [0, 1, 2, 3, 0x10, 0x11, 0x20, 0x30]
    assert all(not sr.accepted(c) for c in REFUSED) and all(sr.accepted(c) for c in sr.ALL_SITED)


# ---- refusals and passes, all before a device is touched (without a device a call that passes the checks answers ERR_HIP) ----
def frame_calls(w2xc, models):
    """the eight frame calls as f(chroma) -> code, on arguments that are good for the layout the value names (planes of full size where it names none)"""
    n, w, h = 2, 16, 8
    calls = {}
    for device in (False, True):
        for rgb in (False, True):
            N, S = (models["rgb_noise"], models["rgb_scale"]) if rgb else (models["noise"], models["scale"])

            def f8(chroma, device=device, rgb=rgb, N=N, S=S):
                lay = chroma & 0xF if 0 <= (chroma & 0xF) <= 3 and chroma >= 0 else yr.YUV_444      # planes large enough whatever the value means
                i, o = t8.Frames(w2xc, n, w, h, yr.YUV_444 if lay == yr.YUV_400 else lay), t8.Frames(w2xc, n, 2 * w, 2 * h, yr.YUV_444 if lay == yr.YUV_400 else lay)
                lib, h_ = w2xc.lib(), (lambda m: m.handle)
                if rgb:
                    fn = lib.w2xc_process_frames_yuv_u8_rgb_device if device else lib.w2xc_process_frames_yuv_u8_rgb
                    head = (h_(N), h_(S), n, w, h, chroma, yr.LIMITED, rr.BT709, C.byref(i.s), C.byref(o.s), 1)
                else:
                    fn = lib.w2xc_process_frames_yuv_u8_device if device else lib.w2xc_process_frames_yuv_u8
                    head = (h_(N), h_(S), n, w, h, chroma, yr.LIMITED, C.byref(i.s), C.byref(o.s), 1)
                return fn(*head, None, None) if device else fn(*head, None)

            def f16(chroma, device=device, rgb=rgb, N=N, S=S):
                lay = chroma & 0xF if 0 <= (chroma & 0xF) <= 3 and chroma >= 0 else yr.YUV_444
                lay = yr.YUV_444 if lay == yr.YUV_400 else lay
                i, o = t16.Frames16(w2xc, n, w, h, lay), t16.Frames16(w2xc, n, 2 * w, 2 * h, lay)
                return t16.call16(w2xc, rgb, device, N, S, n, w, h, chroma, yr.LIMITED, 10, i.s, o.s, 1)

            tag = ("device" if device else "host") + ("_rgb" if rgb else "")
            calls["u8_" + tag], calls["u16_" + tag] = f8, f16
    return calls


def test_frame_calls_refuse_and_accept(w2xc, models):
    A = w2xc.ERR_ARG
    no_device = w2xc.device_count() <= 0
    calls = frame_calls(w2xc, models)
    assert len(calls) == 8
    for name, f in calls.items():
        for chroma in REFUSED:
            assert f(chroma) == A, (name, hex(chroma))
        assert f(7) == A and "unknown chroma layout 7" in w2xc.last_error(), name
        assert f(4) == A and "unknown chroma layout 4" in w2xc.last_error(), name
        assert f(-1) == A and "unknown chroma layout -1" in w2xc.last_error(), name
        assert f(yr.YUV_422 | 0x20) == A and "does not subsample" in w2xc.last_error(), name
        # every flagged value passes the checks; so do the unflagged ones, as before (the device forms are given host planes: only where no device is reached)
        if no_device or "host" in name:
            good = (w2xc.ERR_HIP,) if no_device else (w2xc.OK,)
            for chroma in sr.ALL_SITED + (yr.YUV_420, yr.YUV_422, yr.YUV_444):
                assert f(chroma) in good, (name, hex(chroma), w2xc.last_error())


def test_rgb_blocks_refuse_and_accept(w2xc):
    lib, A = w2xc.lib(), w2xc.ERR_ARG
    n, w, h = 2, 8, 4
    f = np.zeros(3 * n * w * h + 64, np.float32)
    pf, ps, is_ = f.ctypes.data, 4 * w * h, 12 * w * h
    f8, f16 = t8.Frames(w2xc, n, w, h, yr.YUV_444), t16.Frames16(w2xc, n, w, h, yr.YUV_444)
    blocks = {
        "yuv8_to_rgb": lambda c: lib.w2xc_yuv8_to_rgb_device(C.byref(f8.s), n, w, h, c, 0, 1, pf, is_, ps, None),
        "rgb_to_yuv8": lambda c: lib.w2xc_rgb_to_yuv8_device(pf, is_, ps, n, w, h, c, 0, 1, C.byref(f8.s), None),
        "yuv16_to_rgb": lambda c: lib.w2xc_yuv16_to_rgb_device(C.byref(f16.s), n, w, h, c, 0, 10, 1, pf, is_, ps, None),
        "rgb_to_yuv16": lambda c: lib.w2xc_rgb_to_yuv16_device(pf, is_, ps, n, w, h, c, 0, 10, 1, C.byref(f16.s), None),
    }
    for name, fn in blocks.items():
        for chroma in REFUSED:
            assert fn(chroma) == A, (name, hex(chroma))
        assert fn(yr.YUV_400) == A and fn(7) == A and "unknown chroma layout 7" in w2xc.last_error()
        if w2xc.device_count() <= 0:
            for chroma in sr.ALL_SITED + (yr.YUV_420, yr.YUV_422, yr.YUV_444):
                assert fn(chroma) == w2xc.ERR_HIP, (name, hex(chroma), w2xc.last_error())


def test_chroma2x_sited_blocks_refuse_and_accept(w2xc):
    lib, A = w2xc.lib(), w2xc.ERR_ARG
    b = np.zeros(8192, np.uint16)
    src, dst = b.ctypes.data, b.ctypes.data + 4096
    w, h = 8, 4
    c8 = lambda cosited, *a: lib.w2xc_chroma2x_u8_sited_device(*(a or (src, 1, 32, 8, 1, w, h, dst, 128, 16, 1, 16, 8)), cosited, None)
    c16 = lambda cosited, *a: lib.w2xc_chroma2x_u16_sited_device(*(a or (src, 1, 64, 16, 1, 0, w, h, 10, dst, 256, 32, 1, 0, 16, 8)), cosited, None)
    for fn in (c8, c16):
        for bad in (-1, 1, 2, 3, 0x0F, 0x40, 0x31, 0x11, 0x70, 0x100):
            assert fn(bad) == A and "cosited" in w2xc.last_error(), hex(bad)
        if w2xc.device_count() <= 0:
            for ok in (0, 0x10, 0x20, 0x30):
                assert fn(ok) == w2xc.ERR_HIP, (hex(ok), w2xc.last_error())
    # what the centred blocks refuse stays refused with a flag
    assert c8(0x10, None, 1, 32, 8, 1, w, h, dst, 128, 16, 1, 16, 8) == A and c8(0x10, src, 1, 32, 8, 1, w, h, dst, 128, 16, 1, 17, 8) == A
    assert c8(0x30, src, 1, 32, 7, 1, w, h, dst, 128, 16, 1, 16, 8) == A and c8(0x20, src, 1, 32, 8, 3, w, h, dst, 128, 16, 1, 16, 8) == A
    assert c16(0x10, src + 1, 1, 64, 16, 1, 0, w, h, 10, dst, 256, 32, 1, 0, 16, 8) == A and c16(0x10, src, 1, 64, 16, 1, 0, w, h, 17, dst, 256, 32, 1, 0, 16, 8) == A
    assert c16(0x30, src, 1, 64, 16, 1, 2, w, h, 10, dst, 256, 32, 1, 0, 16, 8) == A


# ---- the restatement ----
def test_no_flag_is_the_centred_restatement():
    r = np.random.default_rng(1)
    for cw, ch in ((1, 1), (2, 3), (9, 17), (33, 5)):
        c8 = r.integers(0, 256, (ch, cw), dtype=np.uint8)
        assert np.array_equal(sr.chroma2x(c8, 0), yr.chroma2x(c8)) and sr.chroma2x(c8, 0).dtype == np.uint8
        for depth in (10, 16):
            cd = r.integers(0, 1 << depth, (ch, cw)).astype(np.uint16)
            assert np.array_equal(sr.chroma2x(cd, 0, depth, 2 * cw - 1, 2 * ch - 1), y16.chroma2x(cd, depth, 2 * cw - 1, 2 * ch - 1))
    for layout in rr.LAYOUTS:
        for w, h in ((1, 1), (7, 5), (16, 10)):
            cw, ch = yr.chroma_size(w, h, layout)
            c8 = r.integers(0, 256, (ch, cw), dtype=np.uint8)
            assert np.array_equal(sr.chroma_at_luma(c8, w, h, layout), rr.chroma_at_luma(c8, w, h, layout))
            x = r.standard_normal((h, w)).astype(F32)
            assert np.array_equal(sr.chroma_down(x, layout), rr._block_mean(x, layout))
            Y, U, V = r.integers(0, 256, (h, w), dtype=np.uint8), c8, r.integers(0, 256, (ch, cw), dtype=np.uint8)
            rgb = r.random((3, h, w), dtype=F32) * F32(1.3) - F32(0.15)
            for rng in (yr.FULL, yr.LIMITED):
                assert np.array_equal(sr.yuv_to_rgb(Y, U, V, layout, rng, rr.BT709), rr.yuv8_to_rgb(Y, U, V, layout, rng, rr.BT709))
                for a, b in zip(sr.rgb_to_yuv(rgb, layout, rng, rr.BT601), rr.rgb_to_yuv8(rgb, layout, rng, rr.BT601)):
                    assert np.array_equal(a, b)
                for a, b in zip(sr.rgb_to_yuv(rgb, layout, rng, rr.BT2020, 12), y16.rgb_to_yuv16(rgb, layout, rng, rr.BT2020, 12)):
                    assert np.array_equal(a, b)


def test_positions_of_the_co_sited_2x():
    """output m reads sx = floor(m / 2 - 0.125) with t = 0.375 (odd m) or 0.875 (even m): outputs 2q - 1 and 2q share sx = q - 1, as the centred quads do"""
    taps, c = sr._axis(12, True)
    m = np.arange(24)
    sx = taps[1]                                      # the tap at sx, clamped
    assert np.array_equal(sx, np.clip((m + 1) // 2 - 1, 0, 11))
    c375, c875 = yr.cubic_coeffs(F32(0.375)), yr.cubic_coeffs(F32(0.875))
    for k in range(4):
        assert (c[k][1::2] == c375[k]).all() and (c[k][0::2] == c875[k]).all()
    taps0, c0 = sr._axis(12, False)
    assert all(np.array_equal(a, b) for a, b in zip(taps, taps0)), "the taps are the centred ones: only t differs"
    assert (c0[1][1::2] == yr.cubic_coeffs(F32(0.25))[1]).all()


@pytest.mark.parametrize("depth", [8, 10])
def test_ramps_show_the_siting(depth):
    """C[k] = 40 + 8 k: the co-sited 2x gives 39 + 4 m at every interior sample where the centred one gives 38 + 4 m (Keys' A = -0.75 does not reproduce a ramp
    exactly: -0.33 for even m and +0.23 for odd m before the rounding, so the slope must stay 8); co-sited chroma at luma x is 40 + 4 x exactly; the 1-2-1 mean of
    a luma-resolution ramp is its value at 2k exactly"""
    k = np.arange(16)
    ramp = (40 + 8 * k).astype(np.uint8 if depth == 8 else np.uint16)
    m = np.arange(4, 28)
    for flags in (sr.COSITED_X, sr.COSITED_Y, sr.COSITED_X | sr.COSITED_Y):
        for axis, bit in ((1, sr.COSITED_X), (0, sr.COSITED_Y)):
            plane = np.tile(ramp, (6, 1)) if axis == 1 else np.tile(ramp[:, None], (1, 6))      # a ramp along `axis`, constant along the other
            up, up0 = sr.chroma2x(plane, flags, depth).astype(int), sr.chroma2x(plane, 0, depth).astype(int)
            line, line0 = np.take(np.take(up, m, axis=axis), 3, axis=1 - axis), np.take(np.take(up0, m, axis=axis), 3, axis=1 - axis)
            assert np.array_equal(line, (39 if flags & bit else 38) + 4 * m) and np.array_equal(line0, 38 + 4 * m), (flags, axis, line, line0)
            assert (np.take(up, m, axis=axis) == np.expand_dims(line, 1 - axis)).all(), "constant along the other axis"
    # chroma at luma resolution
    x = np.arange(31)
    at = sr.chroma_at_luma(np.tile(ramp, (4, 1)), 31, 8, sr.YUV_420_LEFT)
    assert np.array_equal(at[0], (40 + 4 * x).astype(F32)) and (at == at[0]).all()
    at = sr.chroma_at_luma(np.tile(ramp[:, None], (1, 4)), 8, 31, sr.YUV_420_TOPLEFT)
    assert np.array_equal(at[:, 0], (40 + 4 * x).astype(F32)) and (at == at[:, :1]).all()
    centred = rr._up_axis(ramp.astype(F32)[None, :], 1, 31)[0]
    assert np.array_equal(centred[2:-2], (38 + 4 * x[2:-2]).astype(F32)), "the centred rule puts sample k at luma 2k + 0.5"
    # the 1-2-1 mean of a ramp at luma resolution is its value at 2k (interior); the box mean is the value at 2k + 0.5
    luma_ramp = (np.arange(32).astype(F32) * F32(0.25))[None, :].repeat(8, axis=0)          # multiples of 1 / 4: every operation exact
    down = sr.chroma_down(luma_ramp, sr.YUV_420_LEFT)
    assert np.array_equal(down[:, 1:], luma_ramp[::2, 2::2]) and np.array_equal(down[:, 0], F32(0.25) * luma_ramp[::2, 1]), "the left edge clamps: (P0 + P1) / 4 + P0 / 2"
    assert np.array_equal(sr.chroma_down(luma_ramp, yr.YUV_420)[:, :], luma_ramp[::2, 0::2] + F32(0.125))
    down = sr.chroma_down(luma_ramp.T.copy(), sr.YUV_420_TOPLEFT)
    assert np.array_equal(down[1:, :], luma_ramp.T[2::2, ::2])
    assert np.array_equal(sr.chroma_down(luma_ramp, sr.YUV_422_LEFT), sr._down_axis(luma_ramp, 1, True))


@pytest.mark.parametrize("chroma", sr.ALL_SITED, ids=[sr.SITED_IDS[c] for c in sr.ALL_SITED])
def test_constants_and_neutral_chroma_stay_put(chroma):
    layout, cx, cy = sr.split(chroma)
    flags = chroma & 0x30
    for depth in (8, 10, 16):
        M = y16.maxval(depth)
        for value in (0, 1, 128 * y16.step(depth), M - 1, M):
            plane = np.full((5, 7), value, np.uint16)
            assert (sr.chroma2x(plane, flags, depth) == value).all()
            assert (sr.chroma_at_luma(plane, *((14, 10) if layout == yr.YUV_420 else (14, 5)), chroma) == F32(value)).all()
        # grey in, grey out: neutral chroma gives R = G = B = y, and equal planes give the neutral chroma value
        for rng in (yr.FULL, yr.LIMITED):
            w, h = 9, 7
            cw, ch = sr.chroma_size(w, h, chroma)
            Y = np.random.default_rng(depth).integers(0, M + 1, (h, w)).astype(np.uint16)
            mid = np.full((ch, cw), 128 * y16.step(depth), np.uint16)
            rgb = sr.yuv_to_rgb(Y, mid, mid, chroma, rng, rr.BT709, depth)
            assert np.array_equal(rgb[0], rgb[1]) and np.array_equal(rgb[1], rgb[2])
            g = np.random.default_rng(depth + 1).random((h, w), dtype=F32)
            _, U, V = sr.rgb_to_yuv(np.stack([g, g, g]), chroma, rng, rr.BT601, depth)
            assert (np.abs(U.astype(int) - 128 * y16.step(depth)) <= 1).all() and (np.abs(V.astype(int) - 128 * y16.step(depth)) <= 1).all()
            flat = np.full((3, h, w), F32(0.5))
            _, U, V = sr.rgb_to_yuv(flat, chroma, rng, rr.BT2020, depth)
            assert (U == U[0, 0]).all() and (V == V[0, 0]).all(), "a constant picture has constant chroma, edges included"


# ---- the tools ----
def test_siting_option_of_the_tools(y4m, y4m16, tmp_path, capsys):
    L = y4m.LAYOUTS
    assert (y4m.COSITED_X, y4m.COSITED_Y) == (sr.COSITED_X, sr.COSITED_Y)
    ap = y4m.build_parser()
    assert ap.parse_args(["a", "b"]).siting == "center"
    for s in ("center", "left", "topleft", "auto"):
        assert ap.parse_args(["a", "b", "--siting", s]).siting == s
    with pytest.raises(SystemExit):
        ap.parse_args(["a", "b", "--siting", "right"])
    # center: whatever the tag says -- the default keeps every stream on the centred call
    for tag in (None, "420", "420jpeg", "420mpeg2", "420paldv"):
        assert y4m.siting_flags("center", tag, L["420"]) == 0
    # auto: by the tag
    assert y4m.siting_flags("auto", "420mpeg2", L["420"]) == sr.COSITED_X and y4m.siting_flags("auto", "422", L["422"]) == sr.COSITED_X
    for tag, lay in ((None, "420"), ("420", "420"), ("420jpeg", "420"), ("444", "444"), ("mono", "mono"), ("420p10", "420"), ("422p10", "422"), ("444p16", "444")):
        assert y4m.siting_flags("auto", tag, L[lay]) == 0, tag
    with pytest.raises(y4m.Y4mError, match="different lines"):
        y4m.siting_flags("auto", "420paldv", L["420"])
    # left / topleft: on the axes the layout subsamples
    assert [y4m.siting_flags("left", None, L[k]) for k in ("420", "422", "444", "mono")] == [0x10, 0x10, 0, 0]
    assert [y4m.siting_flags("topleft", None, L[k]) for k in ("420", "422", "444", "mono")] == [0x30, 0x10, 0, 0]
    assert y4m.siting_flags("left", "420paldv", L["420"]) == 0x10, "a named siting is taken at its word"
    for lay in L.values():
        for s in y4m.SITINGS:
            assert sr.accepted(lay | y4m.siting_flags(s, "422" if lay == 1 else None, lay))
    # the paldv refusal comes before a model is loaded or the output exists, in both tools' voice
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(yr.y4m_stream(16, 8, "420paldv", 1, seed=3)[0])
    assert y4m.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path), "--siting", "auto"]) == 2
    err = capsys.readouterr().err
    assert "w2xc_y4m:" in err and "C420paldv" in err and "different lines" in err and not dst.exists()
    # the flags reach the frame calls or-ed onto the layout, and the C tag is passed on unchanged
    for tool, call in ((y4m, "process_frames_yuv_u8"), (y4m16, "process_frames_yuv_u16")):
        text = open(os.path.join(ROOT, "tools", tool.__name__ + ".py")).read()
        assert "chroma=layout | flags" in text and call in text and "--siting" in text
    data, _ = yr.y4m_stream(16, 8, "420mpeg2", 2, seed=4)
    out = io.BytesIO()
    up = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    assert y4m.convert_stream(io.BytesIO(data), out, lambda y, u, v, layout, full: (up(y), up(u), up(v)), 1) == 2
    out.seek(0)
    assert y4m.read_header(out).get("C") == "420mpeg2"


# ---- the kernels ----
def test_launch_rules_and_shared_bodies():
    squeeze = lambda name: " ".join(open(os.path.join(CSRC, name)).read().split())
    sited = {n: squeeze(n) for n in ("w2xc_yuv_sited.hip", "w2xc_yuv16_sited.hip", "w2xc_yuv_rgb_sited.hip", "w2xc_yuv16_rgb_sited.hip")}
    # the grids are the centred launchers' rules: a kernel family has ONE launcher, in its centred file, that computes the grid once for every siting; the
    # sited files launch nothing and hand out their instantiations
    centred = {n: squeeze(n.replace("_sited", "")) for n in sited}
    assert centred["w2xc_yuv_sited.hip"].count("chroma2x_tile_grid(ow, oh, (long long)n * npl, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX)") == 1
    assert centred["w2xc_yuv16_sited.hip"].count("chroma2x_tile_grid(ow, oh, n, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX)") == 1
    for name in ("w2xc_yuv_rgb_sited.hip", "w2xc_yuv16_rgb_sited.hip"):
        assert centred[name].count("yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX)") == 2
    for name, text in sited.items():
        assert "__launch_bounds__(256)" in text and "hipLaunchKernelGGL" not in text and "_tile_grid(" not in text and "hipError_t" not in text, name
        assert "dim3(256)" in centred[name] and centred[name].count("_sited_kernel(") == text.count("_sited_kernel(") >= 1, name
    kernels_h = squeeze("w2xc_kernels.h")
    assert "_sited(" not in kernels_h and kernels_h.count("hipError_t w2xc_launch_chroma2x_u") == 2
    # one body per kernel, included by the centred kernel's file and by the sited one; the bodies hold the loops, the .hip files none
    pairs = {"w2xc_chroma2x_u8_body.inc": ("w2xc_yuv.hip", "w2xc_yuv_sited.hip"), "w2xc_chroma2x_u16_body.inc": ("w2xc_yuv16.hip", "w2xc_yuv16_sited.hip"),
             "w2xc_yuv8_to_rgb_body.inc": ("w2xc_yuv_rgb.hip", "w2xc_yuv_rgb_sited.hip"), "w2xc_rgb_to_yuv8_body.inc": ("w2xc_yuv_rgb.hip", "w2xc_yuv_rgb_sited.hip"),
             "w2xc_yuv16_to_rgb_body.inc": ("w2xc_yuv16_rgb.hip", "w2xc_yuv16_rgb_sited.hip"),
             "w2xc_rgb_to_yuv16_body.inc": ("w2xc_yuv16_rgb.hip", "w2xc_yuv16_rgb_sited.hip")}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for inc, files in pairs.items():
        assert "turn += gridDim.x" in squeeze(inc) and inc in mk
        for f in files:
            text = open(os.path.join(CSRC, f)).read()
            assert text.count('#include "%s"' % inc) == 1 and "turn += gridDim.x" not in text, (inc, f)
    # the per-sample functions of the co-sited forms have one definition each
    px, tile = open(os.path.join(CSRC, "w2xc_yuv_px.h")).read(), open(os.path.join(CSRC, "w2xc_yuv_tile.h")).read()
    every = [open(os.path.join(CSRC, n)).read() for n in os.listdir(CSRC) if n.endswith((".hip", ".inc", ".h", ".hpp", ".cpp"))]
    for fn, home in (("float lerp11(", px), ("float mean121(", px), ("void chroma_at_luma_sited(", tile), ("void row_chroma(", tile), ("void top_row_chroma(", tile)):
        assert home.count(fn) == 1 and sum(t.count(fn) for t in every) == 1, fn
    for obj in ("w2xc_yuv_sited.o", "w2xc_yuv_rgb_sited.o", "w2xc_yuv16_sited.o", "w2xc_yuv16_rgb_sited.o"):
        assert obj in mk
    assert "-ffp-contract=off" in mk
    # the launch rules the GPU tests rely on: the second-trip shapes have more turns than workgroups
    c = y16.CHROMA_SECOND_TRIP
    assert y16.chroma_launch(2 * c["cw"], 2 * c["ch"], c["n"]) == (2049, 2048)
    assert rr.launch(sr.RGB_SECOND_TRIP["w"], sr.RGB_SECOND_TRIP["h"], yr.YUV_420, 1) == (2 * 1025, 2048)


def test_sited_kernels_no_spill_no_scratch(w2xc):
    lib_dir = os.path.dirname(w2xc.LIB_PATH)
    want = {"w2xc_yuv_sited.o": {"k_chroma2x_u8_sited": 6}, "w2xc_yuv16_sited.o": {"k_chroma2x_u16_sited": 9},
            "w2xc_yuv_rgb_sited.o": {"k_yuv8_to_rgb_sited": 8, "k_rgb_to_yuv8_sited": 4}, "w2xc_yuv16_rgb_sited.o": {"k_yuv16_to_rgb_sited": 12, "k_rgb_to_yuv16_sited": 4}}
    for obj, kernels in want.items():
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(lib_dir, obj)], capture_output=True, text=True, check=True).stdout
        rows = {}
        for line in out.splitlines():
            m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+) lds\s+(\d+)", line)
            if m:
                rows[m.group(1)] = dict(vspill=int(m.group(4)), sspill=int(m.group(5)), scratch=int(m.group(6)), vgpr=int(m.group(2)), lds=int(m.group(7)))
        for k, count in kernels.items():
            assert len([n for n in rows if k in n]) == count, (k, sorted(rows))
        assert len(rows) == sum(kernels.values()), sorted(rows)
        for name, r in rows.items():
            assert (r["vspill"], r["sspill"], r["scratch"]) == (0, 0, 0), (name, r)
            assert r["vgpr"] <= 64, (name, r)       # (the centred kernels' most is 56: the exchanges must not cost occupancy)
            if "rgb_to_yuv" in name:
                assert r["lds"] in (0, 4096), (name, r)    # the row exchange of a co-sited y axis: 2 x 16 x 32 floats
