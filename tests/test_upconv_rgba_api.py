"""The RGBA call for upconv head models (revision 0.4.1.6.2: w2xc_process_image_rgba_u8_up2x_batch[_device]), everything that needs no GPU: the symbols in
the header, the library and the binding, every refusal of the two calls (before a device is touched: this runs on a machine without one), the CLI's routing
of transparent inputs, and the weight image of the alpha head (tests/cpp/upconv_alpha_pack_test.cpp, reached as tests/test_upconv_pack.py reaches the
packers).  The GPU side is tests/test_gpu_upconv_rgba.py; what the EXISTING calls answer for a head model stays pinned by tests/test_upconv_api.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tools import gen_model
import upconv_ref as ur

ERR_ARG, ERR_PLANES, ERR_UNSUPPORTED = -3, -4, -6
C_SYMBOLS = ("w2xc_process_image_rgba_u8_up2x_batch_device", "w2xc_process_image_rgba_u8_up2x_batch")
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")


def head_set(w2xc, planes, nout, seed):
    layers, head = ur.head_model(list(planes), nout, seed)
    return w2xc._ModelSet.from_layers(layers, head=head), layers


@pytest.fixture(scope="module")
def sets(w2xc):
    c32, layers = head_set(w2xc, (3, 32), 3, 401)
    c64y, _ = head_set(w2xc, (1, 32, 64), 1, 402)
    return {"c32": c32, "c64y": c64y, "plain": w2xc._ModelSet.from_layers(layers),
            "noise": w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 32, 3], 9)),
            "ynoise": w2xc._ModelSet.from_layers(gen_model.synth_layers([1, 32, 1], 10))}


# ---- the symbols and the documents ----
def test_symbols_are_declared_exported_bound_and_wrapped(w2xc):
    header = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in C_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym          # declared
        assert getattr(w2xc.lib(), sym) is not None                  # exported
        assert sym in w2xc.ABI_SYMBOLS and sym in integration, sym
    assert callable(w2xc.process_image_rgba_u8_up2x_batch) and callable(w2xc.process_image_rgba_u8_up2x_batch_device)
    names = w2xc.process_image_rgba_u8_up2x_batch.__code__.co_varnames[:8]
    assert names == ("imgs", "noise", "scale", "iterations", "opts", "shrink_ratio", "bleed_passes", "out")


def test_revision_is_found_by_the_symbols(w2xc):
    assert C.sizeof(w2xc.Opts) == 56
    # the version string stays what callers compare it with: the revision is the presence of the symbols, and the documents say so
    assert w2xc.lib().w2xc_version().decode() == "w2xc_hip 0.4.1.6.1 (gfx950)"
    for name in (os.path.join("include", "w2xc_hip.h"), "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "0.4.1.6.2" in text and "0.4.1.6.1" in text, name


# ---- the refusals ----
def test_device_form_refusals(w2xc, sets):
    """fake device addresses: every one of these must be refused by the argument checks, never dereferenced"""
    L = w2xc.lib()
    A, B = 0x10000000, 0x90000000
    w, h = 64, 48
    rs, ims = w * 4, w * 4 * h
    ors, oms = 2 * w * 4, 2 * w * 4 * 2 * h
    head, noise, plain = sets["c32"], sets["noise"], sets["plain"]
    split = w2xc.make_opts(precision=w2xc.PRECISION_BF16X2)

    def call(mn=None, ms=head, n=2, d_in=A, iis=ims, irs=rs, ww=w, hh=h, d_out=B, ois=oms, ors_=ors, it=1, shrink=0.0, passes=-1, opts=None):
        return L.w2xc_process_image_rgba_u8_up2x_batch_device(mn.handle if mn else None, ms.handle if ms else None, n, C.c_void_p(d_in), iis, irs, ww, hh,
                                                              C.c_void_p(d_out), ois, ors_, it, shrink, passes, None,
                                                              C.byref(opts) if opts is not None else None)
    cases = {
        # what w2xc_process_image_rgb_u8_up2x_batch* refuses
        "a scale model without a head": (call(ms=plain), ERR_ARG),
        "a scale model without a head, iterations = 0": (call(mn=noise, ms=plain, it=0, ois=ims, ors_=rs), ERR_ARG),
        "no scale model": (call(mn=noise, ms=None, it=0, ois=ims, ors_=rs), ERR_ARG),
        "a head model as noise model": (call(mn=head), ERR_UNSUPPORTED),
        "a split precision": (call(opts=split), ERR_UNSUPPORTED),
        "a one-plane head model": (call(ms=sets["c64y"]), ERR_PLANES),
        "a Y noise model": (call(mn=sets["ynoise"]), ERR_PLANES),
        # what the RGBA batch calls refuse
        "n = 0": (call(n=0), ERR_ARG),
        "n < 0": (call(n=-1), ERR_ARG),
        "null input": (call(d_in=0), ERR_ARG),
        "null output": (call(d_out=0), ERR_ARG),
        "input rows below 4 w": (call(irs=rs - 1), ERR_ARG),
        "input rows of a 3-channel image": (call(irs=3 * w), ERR_ARG),
        "output rows below 4 W": (call(ors_=ors - 1), ERR_ARG),
        "output images overlap each other": (call(n=3, ois=oms - ors), ERR_ARG),
        "outputs overlap the inputs": (call(n=3, d_out=A + ims), ERR_ARG),
        "in place, n = 1": (call(mn=noise, n=1, d_out=A, it=0, ois=0, ors_=rs), ERR_ARG),
        "iterations = 5": (call(it=5, ois=1 << 28, ors_=1 << 14), ERR_ARG),
        "shrink_ratio = 1": (call(shrink=1.0), ERR_ARG),
        "more than 65534 effective bleed passes": (call(mn=noise, iis=1 << 21, irs=70000 * 4, ww=70000, hh=2, ois=1 << 21, ors_=70000 * 4, it=0,
                                                        passes=1 << 30), ERR_ARG),
        "an extent above 2^28": (call(iis=1 << 40, irs=1 << 30, ww=(1 << 27) + 1, hh=2, ois=1 << 41, ors_=1 << 31), ERR_ARG),
    }
    for what, (rc, want) in cases.items():
        assert rc == want, (what, rc, want, w2xc.last_error())
    if w2xc.device_count() == 0:   # valid arguments: no CPU fallback, and only now a device is asked for
        assert call() == w2xc.ERR_HIP
        assert call(mn=noise, n=1, iis=0, ois=0, passes=3) == w2xc.ERR_HIP
        assert call(n=3, iis=ims + 13, irs=rs + 1, ois=oms + 7, ors_=ors + 3, shrink=0.75, passes=0) == w2xc.ERR_HIP


def test_host_form_refusals(w2xc, sets):
    L = w2xc.lib()
    w, h, n = 40, 24, 3
    ins = [np.zeros((h, w, 4), np.uint8) for _ in range(n)]
    outs = np.zeros((n, 2 * h, 2 * w, 4), np.uint8)
    head, noise, plain = sets["c32"], sets["noise"], sets["plain"]
    split = w2xc.make_opts(precision=w2xc.PRECISION_BF16X2)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)
    ip = arr([a.ctypes.data for a in ins])
    op = arr([outs[i].ctypes.data for i in range(n)])
    rs, ors = w * 4, 2 * w * 4

    def call(mn=None, ms=head, n_=n, ip_=ip, irs=rs, op_=op, ors_=ors, it=1, shrink=0.0, passes=-1, opts=None):
        return L.w2xc_process_image_rgba_u8_up2x_batch(mn.handle if mn else None, ms.handle if ms else None, n_, ip_, irs, w, h, op_, ors_, it, shrink, passes,
                                                       C.byref(opts) if opts is not None else None)
    cases = {
        "a scale model without a head": (call(ms=plain), ERR_ARG),
        "a head model as noise model": (call(mn=head), ERR_UNSUPPORTED),
        "a split precision": (call(opts=split), ERR_UNSUPPORTED),
        "a one-plane head model": (call(ms=sets["c64y"]), ERR_PLANES),
        "n = 0": (call(n_=0), ERR_ARG),
        "null input array": (call(ip_=None), ERR_ARG),
        "null output array": (call(op_=None), ERR_ARG),
        "a null in[i]": (call(ip_=arr([ins[0].ctypes.data, None, ins[2].ctypes.data])), ERR_ARG),
        "a null out[i]": (call(op_=arr([outs[0].ctypes.data, outs[1].ctypes.data, None])), ERR_ARG),
        "input rows below 4 w": (call(irs=rs - 1), ERR_ARG),
        "output rows below 4 W": (call(ors_=ors - 4), ERR_ARG),
        "outputs overlap each other": (call(op_=arr([outs[0].ctypes.data, outs[1].ctypes.data, outs[0].ctypes.data + 64])), ERR_ARG),
        "an output is an input": (call(op_=arr([outs[0].ctypes.data, ins[1].ctypes.data, outs[2].ctypes.data])), ERR_ARG),
    }
    for what, (rc, want) in cases.items():
        assert rc == want, (what, rc, want, w2xc.last_error())
    if w2xc.device_count() == 0:
        assert call() == w2xc.ERR_HIP
        assert call(n_=1) == w2xc.ERR_HIP


def test_existing_rgba_calls_go_on_refusing_a_head_model(w2xc, sets):
    L = w2xc.lib()
    A, B = 0x10000000, 0x90000000
    w, h = 16, 8
    m = sets["c32"].handle
    assert L.w2xc_process_image_rgba_u8_ex_device(None, m, C.c_void_p(A), 4 * w, w, h, C.c_void_p(B), 8 * w, 1, 0.0, -1, None, None) == ERR_UNSUPPORTED
    assert L.w2xc_process_image_rgba_u8_batch_device(None, m, 2, C.c_void_p(A), 4 * w * h, 4 * w, w, h, C.c_void_p(B), 16 * w * h, 8 * w, 1, 0.0, -1, None,
                                                     None) == ERR_UNSUPPORTED


def test_python_wrapper_checks(w2xc, sets):
    f = w2xc.process_image_rgba_u8_up2x_batch
    with pytest.raises(ValueError):
        f([], None, sets["c32"], 1)
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 3), np.uint8)], None, sets["c32"], 1)          # three channels: that is process_image_rgb_u8_up2x_batch
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 4), np.uint8), None, sets["c32"], 1, out=np.zeros((2, 8, 8, 4), np.uint8))
    with pytest.raises(w2xc.W2xcError) as e:
        f(np.zeros((2, 8, 8, 4), np.uint8), None, sets["plain"], 1)
    assert e.value.code == ERR_ARG and "upconv head" in str(e.value)


# ---- the CLI's routing ----
def test_cli_routes_transparent_inputs_of_a_head_model():
    from tools import w2xc_cli
    assert w2xc_cli.head_alpha_routes([["a.png", "b.png"], ["c.png"]]) == [("rgba_up2x_batch", ["a.png", "b.png"]), ("rgba_up2x_batch", ["c.png"])]
    assert w2xc_cli.head_alpha_routes([]) == [] and w2xc_cli.head_alpha_routes([[]]) == []
    # a lone file is a batch of one; the groups are group_inputs', in order of first appearance
    groups = [files for _, files, _ in w2xc_cli.group_inputs([("a.png", (4, 4)), ("b.png", (8, 4)), ("c.png", (4, 4))], "scale", 1, 2.0)]
    assert w2xc_cli.head_alpha_routes(groups) == [("rgba_up2x_batch", ["a.png", "c.png"]), ("rgba_up2x_batch", ["b.png"])]
    # the functions that existed keep their behaviour: main hands head_routes an empty list of transparent inputs
    for tta in (0, 1):
        with pytest.raises(SystemExit):
            w2xc_cli.head_routes(tta, ["t.png"], [["a.png"]])
    with pytest.raises(SystemExit):
        w2xc_cli.check_head(True, 0, ["t.png"], [])
    assert w2xc_cli.head_routes(0, [], [["a.png"]]) == [("single", ["a.png"])]
    with pytest.raises(SystemExit):
        w2xc_cli.check_tta(1, ["t.png"])                                  # --tta 1 with transparency stays check_tta's refusal
    assert "w2xc_process_image_rgba_u8_up2x_batch" in w2xc_cli.__doc__


# ---- the alpha head's weight image ----
def test_alpha_head_image_is_channel_1_of_the_full_image():
    os.makedirs(os.path.join(CPP, "_build"), exist_ok=True)
    exe = os.path.join(CPP, "_build", "upconv_alpha_pack_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(CPP, "upconv_alpha_pack_test.cpp"),
                    os.path.join(CSRC, "w2xc_pack.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all alpha head packer properties hold" in r.stdout
