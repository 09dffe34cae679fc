"""CPU tests of the RGBA surface (w2xc_process_image_rgba_u8_ex[_device], w2xc_bleed_rgba_u8_device): declared and exported, every argument error comes
back as W2XC_ERR_ARG / W2XC_ERR_PLANES before a device is touched (so also on a box without one), the Python wrappers check shapes and types, the new
colour kernels neither spill nor use scratch, the CLI's alpha decision routes correctly -- and bleed_ref, the numpy restatement of the colour bleed of
include/w2xc_hip.h that tests/test_gpu_rgba.py expects of the GPU, gives three hand-computed cases."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, small_layers

LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")
SYMBOLS = ("w2xc_process_image_rgba_u8_ex_device", "w2xc_process_image_rgba_u8_ex", "w2xc_bleed_rgba_u8_device", "w2xc_bleed_rgba_u8_trim")


def bleed_ref(img_hw4, passes):
    """The colour bleed as include/w2xc_hip.h states it, on an h x w x 4 uint8 array: mask = alpha > 0; `passes` times, each pass reading only what the
    pass before left: a pixel with mask 0 and n > 0 masked pixels among the in-bounds pixels of its 3x3 window becomes (2 sum + n) // (2 n) per channel
    and its mask 1; every other pixel is unchanged.  Returns h x w x 4: the bled colour, the alpha bytes as they were."""
    img = np.asarray(img_hw4)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4
    h, w, _ = img.shape
    col = img[:, :, :3].astype(np.int64)
    mask = img[:, :, 3] > 0
    for _ in range(passes):
        new_col, new_mask = col.copy(), mask.copy()
        for y in range(h):
            for x in range(w):
                if mask[y, x]:
                    continue
                ys, xs = slice(max(y - 1, 0), min(y + 2, h)), slice(max(x - 1, 0), min(x + 2, w))
                m = mask[ys, xs]
                n = int(m.sum())
                if n > 0:
                    s = col[ys, xs][m].sum(axis=0)
                    new_col[y, x] = (2 * s + n) // (2 * n)
                    new_mask[y, x] = True
        col, mask = new_col, new_mask
    out = img.copy()
    out[:, :, :3] = col.astype(np.uint8)
    return out


def test_bleed_ref_single_pixel_spreads_one_ring_per_pass():
    img = np.zeros((4, 4, 4), np.uint8)
    img[:, :, :3] = (99, 98, 97)                  # what lies under the transparent pixels
    img[0, 0] = (10, 20, 30, 255)
    assert np.array_equal(bleed_ref(img, 0), img)
    for p in (1, 2, 3, 4):
        got = bleed_ref(img, p)
        for y in range(4):
            for x in range(4):
                want = (10, 20, 30) if max(y, x) <= p else (99, 98, 97)      # ring p = Chebyshev distance p from the pixel
                assert tuple(got[y, x, :3]) == want, (p, y, x)
        assert np.array_equal(got[:, :, 3], img[:, :, 3])                     # alpha is not the bleed's to change


def test_bleed_ref_two_neighbours_round_half_up():
    img = np.zeros((3, 3, 4), np.uint8)
    img[0, 0] = (10, 0, 255, 1)                   # alpha 1 is opaque for the mask: alpha > 0
    img[0, 2] = (13, 1, 255, 200)
    got = bleed_ref(img, 1)
    # (0, 1) and (1, 1) see both: (2 * 23 + 2) // 4 = 12 (11.5 up), (2 * 1 + 2) // 4 = 1 (0.5 up), 255; (1, 0) sees (0, 0) only, (1, 2) sees (0, 2) only
    assert tuple(got[0, 1, :3]) == (12, 1, 255) and tuple(got[1, 1, :3]) == (12, 1, 255)
    assert tuple(got[1, 0, :3]) == (10, 0, 255) and tuple(got[1, 2, :3]) == (13, 1, 255)
    assert (got[2, :, :3] == 0).all()             # row 2: not reached in one pass
    got2 = bleed_ref(img, 2)
    # pass 2 reads pass 1's image: (2, 0) sees (1, 0), (1, 1) = 10, 12 -> 11; (2, 1) sees 10, 12, 13 -> (70 + 3) // 6 = 12; (2, 2) sees 12, 13 -> 13 (12.5 up)
    assert [int(v) for v in got2[2, :, 0]] == [11, 12, 13]
    assert np.array_equal(got2[:2], got[:2])


def test_bleed_ref_out_of_reach_keeps_its_bytes():
    img = np.zeros((3, 3, 4), np.uint8)
    img[:, :, :3] = np.arange(27).reshape(3, 3, 3) + 70
    img[0, 0, 3] = 255
    got = bleed_ref(img, 1)
    for y, x in ((0, 2), (1, 2), (2, 0), (2, 1), (2, 2)):
        assert np.array_equal(got[y, x], img[y, x]), (y, x)
    assert np.array_equal(got[1, 1, :3], img[0, 0, :3])
    none = img.copy()
    none[0, 0, 3] = 0                              # no opaque pixel at all: nothing ever changes
    assert np.array_equal(bleed_ref(none, 5), none)
    full = img.copy()
    full[:, :, 3] = 255                            # no transparent pixel: the identity
    assert np.array_equal(bleed_ref(full, 5), full)


def test_symbols_declared_exported_and_wrapped(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    for name in ("process_image_rgba_u8", "process_image_rgba_u8_device", "bleed_rgba_u8_device", "bleed_rgba_u8_trim"):
        assert callable(getattr(w2xc, name)), name
    lib.w2xc_version.restype = C.c_char_p
    assert lib.w2xc_version().startswith(b"w2xc_hip 0.4.1")
    assert C.sizeof(w2xc.Opts) == 56              # w2xc_opts did not grow


@pytest.fixture(scope="module")
def y_a(w2xc):
    return w2xc._ModelSet.from_layers(small_layers([1, 16, 1], seed=21))


@pytest.fixture(scope="module")
def y_b(w2xc):
    return w2xc._ModelSet.from_layers(small_layers([1, 32, 1], seed=22))


@pytest.fixture(scope="module")
def rgb_a(w2xc):
    return w2xc._ModelSet.from_layers(small_layers([3, 32, 3], seed=11))


@pytest.fixture(scope="module")
def rgb_b(w2xc):
    return w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=12))


def _h(ms):
    return ms.handle if ms is not None else None


def test_device_form_argument_errors(w2xc, y_a, y_b, rgb_a, rgb_b):
    """fake device addresses: every one of these must be refused by the argument checks, never dereferenced"""
    lib = w2xc.lib()
    A, B = 0x10000000, 0x90000000
    w, h = 64, 48
    rs, ors = w * 4, 2 * w * 4

    def one(nm, sm, d_in, irs, ww, hh, d_out, ors_, it, shrink=0.0, passes=-1):
        return lib.w2xc_process_image_rgba_u8_ex_device(_h(nm), _h(sm), C.c_void_p(d_in), irs, ww, hh, C.c_void_p(d_out), ors_, it, shrink, passes, None, None)
    E, P = w2xc.ERR_ARG, w2xc.ERR_PLANES
    for nm, sm in ((y_a, y_b), (rgb_a, rgb_b)):
        assert one(nm, sm, 0, rs, w, h, B, ors, 1) == E                             # null input
        assert one(nm, sm, A, rs, w, h, 0, ors, 1) == E                             # null output
        for ww, hh in ((0, h), (w, 0), (-3, h), (w, -1)):
            assert one(nm, sm, A, rs, ww, hh, B, ors, 1) == E                       # non-positive sizes
        assert one(nm, sm, A, rs - 1, w, h, B, ors, 1) == E                         # input rows below 4 w
        assert one(nm, sm, A, w * 3, w, h, B, ors, 1) == E                          # ... the 3-channel stride is not enough
        assert one(nm, sm, A, rs, w, h, B, ors - 1, 1) == E                         # output rows below 4 W
        assert one(nm, sm, A, rs, w, h, B, 2 * w * 3, 1) == E
        for it in (-1, 5):
            assert one(nm, sm, A, rs, w, h, B, 1 << 14, it) == E                    # iterations outside 0..4
        for shrink in (-0.5, 1.0, 1.5):
            assert one(nm, sm, A, rs, w, h, B, ors, 1, shrink) == E                 # shrink_ratio outside [0, 1)
        assert one(nm, sm, A, 4, 1, 1, B, 8, 1, 0.25) == E                          # the shrink leaves an empty image
        assert one(nm, None, A, rs, w, h, B, ors, 1) == E                           # iterations without a scale model
        assert one(None, None, A, rs, w, h, B, ors, 1) == E                         # no model at all
        assert one(None, sm, A, rs, w, h, B, rs, 0) == E                            # nothing to do
        assert one(nm, None, A, rs, w, h, A + rs, rs, 0) == E                       # the output overlaps the input
        assert one(nm, None, A, rs, w, h, A, rs, 0) == E                            # in place
    # a Y model beside an RGB one, in either order; models that are neither kind (2 planes; 3 -> 1; 1 -> 3)
    assert one(y_a, rgb_b, A, rs, w, h, B, ors, 1) == P
    assert one(rgb_a, y_b, A, rs, w, h, B, ors, 1) == P
    for planes in ([2, 16, 2], [2, 16, 1], [3, 16, 1], [1, 16, 3]):
        bad = w2xc._ModelSet.from_layers(small_layers(planes, seed=30 + planes[0] + planes[2]))
        assert one(bad, None, A, rs, w, h, B, rs, 0) == P, planes
        assert one(None, bad, A, rs, w, h, B, ors, 1) == P, planes
    if w2xc.device_count() == 0:                                                    # valid arguments: no CPU fallback, and only now a device is asked for
        assert one(y_a, y_b, A, rs, w, h, B, ors, 1) == w2xc.ERR_HIP
        assert one(rgb_a, rgb_b, A, rs, w, h, B, ors, 1, 0.75, 0) == w2xc.ERR_HIP
        assert one(y_a, None, A, rs, w, h, B, rs, 0, 0.0, 1 << 30) == w2xc.ERR_HIP  # passes beyond max(w, h) - 1 are not run: no error


def test_host_form_argument_errors(w2xc, y_a, y_b, rgb_a, rgb_b):
    lib = w2xc.lib()
    w, h = 40, 24
    src = np.zeros((h, w, 4), np.uint8)
    out = np.zeros((2 * h, 2 * w, 4), np.uint8)
    same = np.zeros((h, w, 4), np.uint8)
    rs, ors = w * 4, 2 * w * 4

    def one(nm, sm, i_, irs, ww, hh, o_, ors_, it, shrink=0.0, passes=-1):
        return lib.w2xc_process_image_rgba_u8_ex(_h(nm), _h(sm), i_, irs, ww, hh, o_, ors_, it, shrink, passes, None)
    E, P = w2xc.ERR_ARG, w2xc.ERR_PLANES
    I, O, S = src.ctypes.data, out.ctypes.data, same.ctypes.data
    for nm, sm in ((y_a, y_b), (rgb_a, rgb_b)):
        assert one(nm, sm, None, rs, w, h, O, ors, 1) == E
        assert one(nm, sm, I, rs, w, h, None, ors, 1) == E
        assert one(nm, sm, I, rs, 0, h, O, ors, 1) == E
        assert one(nm, sm, I, rs, w, -4, O, ors, 1) == E
        assert one(nm, sm, I, rs - 1, w, h, O, ors, 1) == E
        assert one(nm, sm, I, rs, w, h, O, ors - 1, 1) == E
        assert one(nm, sm, I, rs, w, h, O, ors, 5) == E
        assert one(nm, sm, I, rs, w, h, O, ors, -1) == E
        assert one(nm, sm, I, rs, w, h, O, ors, 1, 1.0) == E
        assert one(nm, sm, I, rs, w, h, O, ors, 1, -0.1) == E
        assert one(nm, None, I, rs, w, h, O, ors, 1) == E
        assert one(None, None, I, rs, w, h, O, ors, 1) == E
        assert one(None, sm, I, rs, w, h, S, rs, 0) == E
        assert one(nm, None, I, rs, w, h, I + 8, rs, 0) == E                        # the output overlaps the input
    assert one(y_a, rgb_b, I, rs, w, h, O, ors, 1) == P
    assert one(rgb_a, y_b, I, rs, w, h, O, ors, 1) == P
    two = w2xc._ModelSet.from_layers(small_layers([2, 16, 2], seed=5))
    assert one(two, None, I, rs, w, h, S, rs, 0) == P
    assert one(None, two, I, rs, w, h, O, ors, 1) == P
    if w2xc.device_count() == 0:
        assert one(y_a, y_b, I, rs, w, h, O, ors, 1) == w2xc.ERR_HIP
        assert one(rgb_a, rgb_b, I, rs, w, h, O, ors, 1) == w2xc.ERR_HIP


def test_bleed_block_argument_errors(w2xc):
    lib = w2xc.lib()
    A, B = 0x10000000, 0x90000000
    w, h = 20, 12

    def call(d_in, irs, ww, hh, passes, d_out, ors):
        return lib.w2xc_bleed_rgba_u8_device(C.c_void_p(d_in), irs, ww, hh, passes, C.c_void_p(d_out), ors, None)
    E = w2xc.ERR_ARG
    assert call(0, w * 4, w, h, 1, B, w * 3) == E
    assert call(A, w * 4, w, h, 1, 0, w * 3) == E
    assert call(A, w * 4, 0, h, 1, B, w * 3) == E
    assert call(A, w * 4, w, -1, 1, B, w * 3) == E
    assert call(A, w * 4 - 1, w, h, 1, B, w * 3) == E                               # input rows below 4 w
    assert call(A, w * 4, w, h, 1, B, w * 3 - 1) == E                               # output rows below 3 w
    assert call(A, w * 4, w, h, -1, B, w * 3) == E                                  # the building block has no automatic pass count
    assert call(A, w * 4, w, h, 1, A + 16, w * 3) == E                              # the output overlaps the input
    if w2xc.device_count() == 0:
        assert call(A, w * 4, w, h, 3, B, w * 3) == w2xc.ERR_HIP
    assert lib.w2xc_bleed_rgba_u8_trim() == w2xc.OK                                 # nothing to release: no device is touched


def test_python_wrapper_checks(w2xc, y_a, y_b):
    g = w2xc.process_image_rgba_u8
    with pytest.raises(ValueError):
        g(np.zeros((8, 8, 4), np.float32), y_a)                                     # wrong dtype
    with pytest.raises(ValueError):
        g(np.zeros((8, 8), np.uint8), y_a)                                          # wrong rank
    with pytest.raises(ValueError):
        g(np.zeros((8, 8, 3), np.uint8), y_a)                                       # three channels: that is process_image_u8
    with pytest.raises(ValueError):
        g(np.zeros((8, 8, 2), np.uint8), y_a)
    with pytest.raises(w2xc.W2xcError) as ei:
        g(np.zeros((8, 8, 4), np.uint8), None, None)
    assert ei.value.code == w2xc.ERR_ARG
    with pytest.raises(w2xc.W2xcError) as ei:
        g(np.zeros((8, 8, 4), np.uint8), y_a, None, 1)                              # iterations without a scale model
    assert ei.value.code == w2xc.ERR_ARG
    if w2xc.device_count() == 0:
        with pytest.raises(w2xc.W2xcError) as ei:
            g(np.zeros((8, 8, 4), np.uint8), y_a, y_b, 1, None, 0.0, 2)
        assert ei.value.code == w2xc.ERR_HIP   # (no CPU fallback)


def test_rgba_colour_kernels_no_spill_no_scratch(w2xc):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, "w2xc_color.o")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vspill=int(m.group(4)), scratch=int(m.group(6)))
    for k in ("RgbaBleedFirst", "RgbaBleedPass", "AlphaToPlane", "AlphaToGrey", "MergeRgbaF32", "MergeRgbaU8"):   # stage names, in the mangled k_px<Stage>
        hit = [name for name in rows if k in name]
        assert len(hit) == 1, (k, sorted(rows))
        assert rows[hit[0]] == dict(vspill=0, scratch=0), (hit[0], rows[hit[0]])


def _cli():
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_alpha_decision():
    cli = _cli()
    rgba = np.full((6, 5, 4), 255, np.uint8)
    assert cli.wants_alpha(rgba) is False                       # an alpha that is 255 everywhere: the 3-channel route, as before
    rgba[3, 2, 3] = 254
    assert cli.wants_alpha(rgba) is True                        # one byte of 254: the RGBA call
    rgba[3, 2, 3] = 0
    assert cli.wants_alpha(rgba) is True
    assert cli.wants_alpha(np.zeros((6, 5, 3), np.uint8)) is False
    assert cli.wants_alpha(np.zeros((6, 5), np.uint8)) is False
