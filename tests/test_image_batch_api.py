"""CPU tests of the image batch entry points (w2xc_process_image_u8_batch / w2xc_process_image_u8_batch_device): declared and exported, every
argument error comes back as W2XC_ERR_ARG / W2XC_ERR_PLANES before a device is touched (so also on a box without one), the Python wrapper checks
shapes and types, the four batch colour kernels neither spill nor use scratch, and the CLI groups several inputs by size."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, small_layers
from tools import gen_model

LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")
SYMBOLS = ("w2xc_process_image_u8_batch", "w2xc_process_image_u8_batch_device")


def test_symbols_declared_and_exported(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    lib.w2xc_version.restype = C.c_char_p
    assert lib.w2xc_version().startswith(b"w2xc_hip 0.4")


@pytest.fixture(scope="module")
def noise1(w2xc):
    return w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["noise1"]))


@pytest.fixture(scope="module")
def scale2(w2xc):
    return w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]))


def _h(ms):
    return ms.handle if ms is not None else None


def test_device_form_argument_errors(w2xc, noise1, scale2):
    """fake device addresses: every one of these must be refused by the argument checks, never dereferenced"""
    lib = w2xc.lib()
    A, B = 0x10000000, 0x90000000
    w, h = 64, 48
    rs, ims = w * 3, w * 3 * h                    # input row / image stride
    ors, oms = 2 * w * 3, 2 * w * 3 * 2 * h       # output row / image stride for one iteration

    def call(nm, sm, n, d_in, iis, irs, ww, hh, d_out, ois, ors_, it, shrink=0.0):
        return lib.w2xc_process_image_u8_batch_device(_h(nm), _h(sm), n, C.c_void_p(d_in), iis, irs, ww, hh, C.c_void_p(d_out), ois, ors_, it,
                                                      shrink, None, None)
    E = w2xc.ERR_ARG
    for n in (0, -1):
        assert call(noise1, scale2, n, A, ims, rs, w, h, B, oms, ors, 1) == E                  # n < 1
    assert call(noise1, scale2, 2, 0, ims, rs, w, h, B, oms, ors, 1) == E                      # null input
    assert call(noise1, scale2, 2, A, ims, rs, w, h, 0, oms, ors, 1) == E                      # null output
    for ww, hh in ((0, h), (w, 0), (-3, h), (w, -1)):
        assert call(noise1, scale2, 2, A, ims, rs, ww, hh, B, oms, ors, 1) == E                # non-positive sizes
    for it in (-1, 5):
        assert call(noise1, scale2, 2, A, ims, rs, w, h, B, 1 << 28, 1 << 14, it) == E         # iterations outside 0..4
    for shrink in (-0.5, 1.0, 1.5):
        assert call(noise1, scale2, 2, A, ims, rs, w, h, B, oms, ors, 1, shrink) == E          # bad shrink_ratio
    assert call(noise1, scale2, 2, A, 3, 3, 1, 1, B, 64, 6, 1, 0.25) == E                      # the shrink leaves an empty image (2 * 0.25 -> 0)
    assert call(noise1, scale2, 2, A, ims, rs - 1, w, h, B, oms, ors, 1) == E                  # input rows below 3 w
    assert call(noise1, scale2, 2, A, ims, rs, w, h, B, oms, ors - 1, 1) == E                  # output rows below 3 W
    assert call(noise1, scale2, 3, A, ims, rs, w, h, B, oms - ors, ors, 1) == E                # output images overlap each other
    assert call(noise1, scale2, 3, A, ims, rs, w, h, A + ims, oms, ors, 1) == E                # outputs overlap the inputs
    assert call(noise1, None, 1, A, 0, rs, w, h, A, 0, rs, 0) == E                             # in place
    # the three cases the single-image call refuses (check_process_args)
    assert call(None, None, 2, A, ims, rs, w, h, B, oms, ors, 1) == E                          # no model at all
    assert call(noise1, None, 2, A, ims, rs, w, h, B, oms, ors, 1) == E                        # iterations without a scale model
    assert call(None, scale2, 2, A, ims, rs, w, h, B, ims, rs, 0) == E                         # nothing to do
    # a multi-plane model, in either role: W2XC_ERR_PLANES
    ms3 = w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=5))
    assert call(ms3, None, 2, A, ims, rs, w, h, B, ims, rs, 0) == w2xc.ERR_PLANES
    assert call(noise1, ms3, 2, A, ims, rs, w, h, B, oms, ors, 1) == w2xc.ERR_PLANES


def test_host_form_argument_errors(w2xc, noise1, scale2):
    lib = w2xc.lib()
    w, h, n = 40, 24, 3
    ins = [np.zeros((h, w, 3), np.uint8) for _ in range(n)]
    outs = np.zeros((n, 2 * h, 2 * w, 3), np.uint8)
    same = np.zeros((n, h, w, 3), np.uint8)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def call(nm, sm, n_, ip, irs, ww, hh, op, ors, it, shrink=0.0):
        return lib.w2xc_process_image_u8_batch(_h(nm), _h(sm), n_, ip, irs, ww, hh, op, ors, it, shrink, None)
    ip = arr([a.ctypes.data for a in ins])
    op = arr([outs[i].ctypes.data for i in range(n)])
    op0 = arr([same[i].ctypes.data for i in range(n)])
    rs, ors = w * 3, 2 * w * 3
    E = w2xc.ERR_ARG
    assert call(noise1, scale2, 0, ip, rs, w, h, op, ors, 1) == E
    assert call(noise1, scale2, -2, ip, rs, w, h, op, ors, 1) == E
    assert call(noise1, scale2, n, None, rs, w, h, op, ors, 1) == E
    assert call(noise1, scale2, n, ip, rs, w, h, None, ors, 1) == E
    assert call(noise1, scale2, n, arr([ins[0].ctypes.data, None, ins[2].ctypes.data]), rs, w, h, op, ors, 1) == E       # a null in[i]
    assert call(noise1, scale2, n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, None]), ors, 1) == E     # a null out[i]
    assert call(noise1, scale2, n, ip, rs, 0, h, op, ors, 1) == E
    assert call(noise1, scale2, n, ip, rs, w, -4, op, ors, 1) == E
    assert call(noise1, scale2, n, ip, rs, w, h, op, ors, 5) == E
    assert call(noise1, scale2, n, ip, rs, w, h, op, ors, -1) == E
    assert call(noise1, scale2, n, ip, rs, w, h, op, ors, 1, 1.0) == E
    assert call(noise1, scale2, n, ip, rs, w, h, op, ors, 1, -0.1) == E
    assert call(noise1, scale2, n, ip, 3, 1, 1, op, 6, 1, 0.25) == E                                                    # empty after the shrink
    assert call(noise1, scale2, n, ip, rs - 1, w, h, op, ors, 1) == E
    assert call(noise1, scale2, n, ip, rs, w, h, op, ors - 3, 1) == E
    assert call(noise1, scale2, n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, outs[0].ctypes.data + 64]), ors, 1) == E   # outputs overlap
    assert call(noise1, None, n, ip, rs, w, h, arr([same[0].ctypes.data, ins[1].ctypes.data, same[2].ctypes.data]), rs, 0) == E           # output = an input
    assert call(None, None, n, ip, rs, w, h, op, ors, 1) == E
    assert call(noise1, None, n, ip, rs, w, h, op, ors, 1) == E
    assert call(None, scale2, n, ip, rs, w, h, op0, rs, 0) == E
    ms3 = w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=5))
    assert call(ms3, None, n, ip, rs, w, h, op0, rs, 0) == w2xc.ERR_PLANES
    assert call(None, ms3, n, ip, rs, w, h, op, ors, 1) == w2xc.ERR_PLANES
    if w2xc.device_count() == 0:
        assert call(noise1, scale2, n, ip, rs, w, h, op, ors, 1) == w2xc.ERR_HIP     # valid arguments: no CPU fallback


def test_python_wrapper_checks(w2xc, noise1, scale2):
    f = w2xc.process_image_u8_batch
    with pytest.raises(ValueError):
        f([], noise1)                                                                       # empty batch
    with pytest.raises(ValueError):
        f(np.zeros((0, 8, 8, 3), np.uint8), noise1)                                         # empty batch, array form
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8)], noise1)           # mixed shapes
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 3), np.float32), noise1)                                       # wrong dtype
    with pytest.raises(ValueError):
        f(np.zeros((8, 8, 3), np.uint8), noise1)                                            # one image is not a batch
    with pytest.raises(ValueError):
        f([np.zeros((8, 8), np.uint8)], noise1)                                             # wrong rank
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 4), np.uint8)], noise1)                                          # four channels
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 3), np.uint8), None, scale2, 1, out=np.zeros((2, 8, 8, 3), np.uint8))     # out of the wrong shape
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 3), np.uint8), None, scale2, 1, out=np.zeros((2, 16, 16, 3), np.float32))  # out of the wrong dtype
    if w2xc.device_count() == 0:
        with pytest.raises(w2xc.W2xcError) as ei:
            f(np.zeros((2, 8, 8, 3), np.uint8), noise1, scale2, 1)
        assert ei.value.code == w2xc.ERR_HIP   # (no CPU fallback)
        assert hasattr(w2xc, "process_image_u8_batch_device")


def test_batch_colour_kernels_no_spill_no_scratch(w2xc):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, "w2xc_color.o")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vspill=int(m.group(4)), scratch=int(m.group(6)))
    for k in ("U8ToYuv", "Resize2xCubic", "ResizeLinear", "YuvToU8"):   # the stage names, as they stand in the mangled k_px<Stage>
        hit = [name for name in rows if k in name]
        assert len(hit) == 1, (k, sorted(rows))
        assert rows[hit[0]] == dict(vspill=0, scratch=0), (hit[0], rows[hit[0]])


def _cli():
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_groups_inputs_by_size():
    cli = _cli()
    files = [("/d/a.png", (64, 64)), ("/d/b.jpg", (32, 48)), ("/d/c.png", (64, 64)), ("/d/d.png", (48, 32)), ("/d/e.v2.png", (32, 48))]
    got = cli.group_inputs(files, "noise_scale", 2, 2.0)
    assert got == [((64, 64), ["/d/a.png", "/d/c.png"], ["/d/a(noise_scale)(Level2)(x2.000000).png", "/d/c(noise_scale)(Level2)(x2.000000).png"]),
                   ((32, 48), ["/d/b.jpg", "/d/e.v2.png"], ["/d/b(noise_scale)(Level2)(x2.000000).png", "/d/e.v2(noise_scale)(Level2)(x2.000000).png"]),
                   ((48, 32), ["/d/d.png"], ["/d/d(noise_scale)(Level2)(x2.000000).png"])]
    assert cli.group_inputs([("x.png", (5, 7))], "scale", 1, 1.5) == [((5, 7), ["x.png"], ["x(scale)(x1.500000).png"])]
    assert cli.group_inputs([], "scale", 1, 2.0) == []


def test_cli_several_inputs_and_output_flag():
    cli = _cli()
    ap = cli.build_parser()
    a = cli.check_inputs(ap, ap.parse_args(["-i", "a.png", "b.png", "-i", "c.png", "-m", "scale"]))
    assert a.input_file == ["a.png", "b.png", "c.png"] and a.output_file == "(auto)"
    a = cli.check_inputs(ap, ap.parse_args(["-i", "a.png", "-o", "out.png"]))          # one input: -o as before
    assert a.input_file == ["a.png"] and a.output_file == "out.png"
    with pytest.raises(SystemExit) as ei:
        cli.check_inputs(ap, ap.parse_args(["-i", "a.png", "b.png", "-o", "out.png"]))
    assert ei.value.code == 2
