"""CPU tests of the batch forms of the RGBA call (w2xc_process_image_rgba_u8_batch[_device], revision 0.4.1.3): declared, exported and wrapped, every
argument error comes back as W2XC_ERR_ARG / W2XC_ERR_PLANES before a device is touched (so also on a box without one), the Python wrapper checks shapes
and types, the tiled bleed kernel neither spills nor uses scratch, and the CLI groups its transparent inputs by size."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, small_layers

LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")
SYMBOLS = ("w2xc_process_image_rgba_u8_batch_device", "w2xc_process_image_rgba_u8_batch")
STAGES = ("RgbaBleedFirst", "RgbaBleedPass", "AlphaToPlane", "AlphaToGrey", "MergeRgbaF32", "MergeRgbaU8")


def test_symbols_declared_exported_and_wrapped(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    for name in ("process_image_rgba_u8_batch", "process_image_rgba_u8_batch_device"):
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
    rs, ims = w * 4, w * 4 * h                    # input row / image stride
    ors, oms = 2 * w * 4, 2 * w * 4 * 2 * h       # output row / image stride for one iteration

    def call(nm, sm, n, d_in, iis, irs, ww, hh, d_out, ois, ors_, it, shrink=0.0, passes=-1):
        return lib.w2xc_process_image_rgba_u8_batch_device(_h(nm), _h(sm), n, C.c_void_p(d_in), iis, irs, ww, hh, C.c_void_p(d_out), ois, ors_, it,
                                                           shrink, passes, None, None)
    E, P = w2xc.ERR_ARG, w2xc.ERR_PLANES
    for nm, sm in ((y_a, y_b), (rgb_a, rgb_b)):
        for n in (0, -1):
            assert call(nm, sm, n, A, ims, rs, w, h, B, oms, ors, 1) == E                  # n < 1
        assert call(nm, sm, 2, 0, ims, rs, w, h, B, oms, ors, 1) == E                      # null input
        assert call(nm, sm, 2, A, ims, rs, w, h, 0, oms, ors, 1) == E                      # null output
        for ww, hh in ((0, h), (w, 0), (-3, h), (w, -1)):
            assert call(nm, sm, 2, A, ims, rs, ww, hh, B, oms, ors, 1) == E                # non-positive sizes
        assert call(nm, sm, 2, A, ims, rs - 1, w, h, B, oms, ors, 1) == E                  # input rows below 4 w
        assert call(nm, sm, 2, A, ims, w * 3, w, h, B, oms, ors, 1) == E                   # ... the 3-channel stride is not enough
        assert call(nm, sm, 2, A, ims, rs, w, h, B, oms, ors - 1, 1) == E                  # output rows below 4 W
        assert call(nm, sm, 2, A, ims, rs, w, h, B, oms, 2 * w * 3, 1) == E
        assert call(nm, sm, 3, A, ims, rs, w, h, B, oms - ors, ors, 1) == E                # output images overlap each other
        assert call(nm, sm, 3, A, ims, rs, w, h, A + ims, oms, ors, 1) == E                # outputs overlap the inputs
        assert call(nm, None, 1, A, 0, rs, w, h, A, 0, rs, 0) == E                         # in place
        # everything the single RGBA call refuses
        for it in (-1, 5):
            assert call(nm, sm, 2, A, ims, rs, w, h, B, 1 << 28, 1 << 14, it) == E         # iterations outside 0..4
        for shrink in (-0.5, 1.0, 1.5):
            assert call(nm, sm, 2, A, ims, rs, w, h, B, oms, ors, 1, shrink) == E          # shrink_ratio outside [0, 1)
        assert call(nm, sm, 2, A, 4, 4, 1, 1, B, 64, 8, 1, 0.25) == E                      # the shrink leaves an empty image
        assert call(None, None, 2, A, ims, rs, w, h, B, oms, ors, 1) == E                  # no model at all
        assert call(nm, None, 2, A, ims, rs, w, h, B, oms, ors, 1) == E                    # iterations without a scale model
        assert call(None, sm, 2, A, ims, rs, w, h, B, ims, rs, 0) == E                     # nothing to do
    assert call(y_a, None, 2, A, 1 << 21, 70000 * 4, 70000, 2, B, 1 << 21, 70000 * 4, 0, 0.0, 1 << 30) == E   # more than 65534 effective bleed passes
    # a Y model beside an RGB one, in either order; models that are neither kind
    assert call(y_a, rgb_b, 2, A, ims, rs, w, h, B, oms, ors, 1) == P
    assert call(rgb_a, y_b, 2, A, ims, rs, w, h, B, oms, ors, 1) == P
    for planes in ([2, 16, 2], [2, 16, 1], [3, 16, 1], [1, 16, 3]):
        bad = w2xc._ModelSet.from_layers(small_layers(planes, seed=30 + planes[0] + planes[2]))
        assert call(bad, None, 2, A, ims, rs, w, h, B, ims, rs, 0) == P, planes
        assert call(None, bad, 2, A, ims, rs, w, h, B, oms, ors, 1) == P, planes
    if w2xc.device_count() == 0:                                                           # valid arguments: no CPU fallback, and only now a device is asked for
        assert call(y_a, y_b, 2, A, ims, rs, w, h, B, oms, ors, 1) == w2xc.ERR_HIP
        assert call(rgb_a, rgb_b, 3, A, ims + 13, rs + 1, w, h, B, oms + 7, ors + 3, 1, 0.75, 0) == w2xc.ERR_HIP
        assert call(y_a, None, 1, A, 0, rs, w, h, B, 0, rs, 0, 0.0, 1 << 30) == w2xc.ERR_HIP


def test_host_form_argument_errors(w2xc, y_a, y_b, rgb_a, rgb_b):
    lib = w2xc.lib()
    w, h, n = 40, 24, 3
    ins = [np.zeros((h, w, 4), np.uint8) for _ in range(n)]
    outs = np.zeros((n, 2 * h, 2 * w, 4), np.uint8)
    same = np.zeros((n, h, w, 4), np.uint8)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def call(nm, sm, n_, ip, irs, ww, hh, op, ors, it, shrink=0.0, passes=-1):
        return lib.w2xc_process_image_rgba_u8_batch(_h(nm), _h(sm), n_, ip, irs, ww, hh, op, ors, it, shrink, passes, None)
    ip = arr([a.ctypes.data for a in ins])
    op = arr([outs[i].ctypes.data for i in range(n)])
    op0 = arr([same[i].ctypes.data for i in range(n)])
    rs, ors = w * 4, 2 * w * 4
    E, P = w2xc.ERR_ARG, w2xc.ERR_PLANES
    for nm, sm in ((y_a, y_b), (rgb_a, rgb_b)):
        assert call(nm, sm, 0, ip, rs, w, h, op, ors, 1) == E
        assert call(nm, sm, -2, ip, rs, w, h, op, ors, 1) == E
        assert call(nm, sm, n, None, rs, w, h, op, ors, 1) == E
        assert call(nm, sm, n, ip, rs, w, h, None, ors, 1) == E
        assert call(nm, sm, n, arr([ins[0].ctypes.data, None, ins[2].ctypes.data]), rs, w, h, op, ors, 1) == E       # a null in[i]
        assert call(nm, sm, n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, None]), ors, 1) == E     # a null out[i]
        assert call(nm, sm, n, ip, rs, 0, h, op, ors, 1) == E
        assert call(nm, sm, n, ip, rs, w, -4, op, ors, 1) == E
        assert call(nm, sm, n, ip, rs, w, h, op, ors, 5) == E
        assert call(nm, sm, n, ip, rs, w, h, op, ors, -1) == E
        assert call(nm, sm, n, ip, rs, w, h, op, ors, 1, 1.0) == E
        assert call(nm, sm, n, ip, rs, w, h, op, ors, 1, -0.1) == E
        assert call(nm, sm, n, ip, 4, 1, 1, op, 8, 1, 0.25) == E                                                     # empty after the shrink
        assert call(nm, sm, n, ip, rs - 1, w, h, op, ors, 1) == E                                                    # rows below 4 w
        assert call(nm, sm, n, ip, rs, w, h, op, ors - 4, 1) == E                                                    # rows below 4 W
        assert call(nm, sm, n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, outs[0].ctypes.data + 64]), ors, 1) == E   # outputs overlap
        assert call(nm, None, n, ip, rs, w, h, arr([same[0].ctypes.data, ins[1].ctypes.data, same[2].ctypes.data]), rs, 0) == E       # output = an input
        assert call(nm, None, 1, ip, rs, w, h, ip, rs, 0) == E                                                       # n = 1, in place
        assert call(None, None, n, ip, rs, w, h, op, ors, 1) == E
        assert call(nm, None, n, ip, rs, w, h, op, ors, 1) == E
        assert call(None, sm, n, ip, rs, w, h, op0, rs, 0) == E
    assert call(y_a, rgb_b, n, ip, rs, w, h, op, ors, 1) == P
    assert call(rgb_a, y_b, n, ip, rs, w, h, op, ors, 1) == P
    two = w2xc._ModelSet.from_layers(small_layers([2, 16, 2], seed=5))
    assert call(two, None, n, ip, rs, w, h, op0, rs, 0) == P
    assert call(None, two, n, ip, rs, w, h, op, ors, 1) == P
    if w2xc.device_count() == 0:
        assert call(y_a, y_b, n, ip, rs, w, h, op, ors, 1) == w2xc.ERR_HIP     # valid arguments: no CPU fallback
        assert call(rgb_a, rgb_b, n, ip, rs, w, h, op, ors, 1) == w2xc.ERR_HIP
        assert call(y_a, y_b, 1, ip, rs, w, h, op, ors, 1) == w2xc.ERR_HIP


def test_python_wrapper_checks(w2xc, y_a, y_b):
    f = w2xc.process_image_rgba_u8_batch
    with pytest.raises(ValueError):
        f([], y_a)                                                                          # empty batch
    with pytest.raises(ValueError):
        f(np.zeros((0, 8, 8, 4), np.uint8), y_a)                                            # empty batch, array form
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 4), np.uint8), np.zeros((8, 9, 4), np.uint8)], y_a)              # mixed sizes
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 4), np.float32), y_a)                                          # wrong dtype
    with pytest.raises(ValueError):
        f(np.zeros((8, 8, 4), np.uint8), y_a)                                               # one image is not a batch
    with pytest.raises(ValueError):
        f([np.zeros((8, 8), np.uint8)], y_a)                                                # wrong rank
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 3), np.uint8)], y_a)                                             # three channels: that is process_image_u8_batch
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.uint8)], y_a)
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 4), np.uint8), None, y_b, 1, out=np.zeros((2, 8, 8, 4), np.uint8))       # out of the wrong shape
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 4), np.uint8), None, y_b, 1, out=np.zeros((2, 16, 16, 3), np.uint8))     # ... of three channels
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 4), np.uint8), None, y_b, 1, out=np.zeros((2, 16, 16, 4), np.float32))   # out of the wrong dtype
    with pytest.raises(w2xc.W2xcError) as ei:
        f(np.zeros((2, 8, 8, 4), np.uint8), None, None)
    assert ei.value.code == w2xc.ERR_ARG
    if w2xc.device_count() == 0:
        with pytest.raises(w2xc.W2xcError) as ei:
            f(np.zeros((2, 8, 8, 4), np.uint8), y_a, y_b, 1, None, 0.0, 2)
        assert ei.value.code == w2xc.ERR_HIP   # (no CPU fallback)
    # the 3-channel wrappers share the checks and keep theirs
    with pytest.raises(ValueError):
        w2xc.process_image_u8_batch([np.zeros((8, 8, 4), np.uint8)], y_a)


def test_tiled_bleed_kernel_no_spill_no_scratch(w2xc):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, "w2xc_color.o")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+) lds\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vspill=int(m.group(4)), scratch=int(m.group(6)), lds=int(m.group(7)))
    hit = [name for name in rows if "k_bleed_tiled" in name]
    assert len(hit) == 1, sorted(rows)
    assert not any(k in hit[0] for k in STAGES), hit[0]                        # its name holds none of the six stage names
    assert rows[hit[0]]["vspill"] == 0 and rows[hit[0]]["scratch"] == 0, rows[hit[0]]
    assert 0 < rows[hit[0]]["lds"] <= 64 * 1024, rows[hit[0]]                  # the tile and its halo: static LDS
    for k in STAGES:                                                           # one kernel per stage: one image runs the batch form with n = 1
        stage = [name for name in rows if k in name]
        assert len(stage) == 1, (k, sorted(rows))
        assert rows[stage[0]]["vspill"] == 0 and rows[stage[0]]["scratch"] == 0, (stage[0], rows[stage[0]])


def _cli():
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_groups_alpha_inputs_by_size():
    cli = _cli()
    files = [("a.png", (16, 20)), ("b.png", (32, 20)), ("c.png", (16, 20)), ("d.png", (16, 21)), ("e.png", [16, 20]), ("f.png", (32, 20))]
    singles, batches = cli.group_alpha(files, "scale", 1, 2.0)
    assert singles == ["d.png"]                                                # alone with its size: the single call
    assert batches == [["a.png", "c.png", "e.png"], ["b.png", "f.png"]]        # a group of two or more is one batch call, in order of first appearance
    assert cli.group_alpha([], "scale", 1, 2.0) == ([], [])
    assert cli.group_alpha([("x.png", (4, 4))], "noise", 2, 1.0) == (["x.png"], [])
    assert cli.group_alpha([("x.png", (4, 4)), ("y.png", (4, 4))], "noise", 2, 1.0) == ([], [["x.png", "y.png"]])
