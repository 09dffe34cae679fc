"""CPU tests of w2xc_resize_linear_device (include/w2xc_hip.h, revision 0.4.1.4): declared in the header, exported, in the ctypes table and wrapped;
every argument error comes back as W2XC_ERR_ARG before a device is touched (fake device addresses are never dereferenced), a valid call without a device
returns W2XC_ERR_HIP; w2xc_opts keeps its 56 bytes.  What the call computes is tests/test_gpu_color_stages.py's."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

A, B = 0x10000000, 0x90000000    # fake device addresses
NAME = "w2xc_resize_linear_device"


def test_symbol_declared_exported_wrapped(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    assert re.search(r"\bint %s\(const float \*d_src, int sw, int sh, float \*d_dst, int dw, int dh, void \*hip_stream\);" % NAME, hdr)
    assert hasattr(lib, NAME)
    assert NAME in w2xc.ABI_SYMBOLS
    f = getattr(w2xc.lib(), NAME)
    assert f.restype is C.c_int and len(f.argtypes) == 7
    assert callable(w2xc.resize_linear_device)
    assert w2xc.resize_linear_device.__code__.co_varnames[:7] == ("d_src", "sw", "sh", "d_dst", "dw", "dh", "stream")
    assert w2xc.resize_linear_device.__defaults__ == (0,)


def test_version_and_opts_size(w2xc):
    lib = C.CDLL(w2xc.LIB_PATH)
    lib.w2xc_version.restype = C.c_char_p
    assert lib.w2xc_version().startswith(b"w2xc_hip 0.4.1")
    assert C.sizeof(w2xc.Opts) == 56
    assert w2xc.make_opts().struct_size == 56


def test_argument_errors_before_a_device(w2xc):
    E = w2xc.ERR_ARG

    def call(d_src, sw, sh, d_dst, dw, dh):
        return w2xc.lib().w2xc_resize_linear_device(C.c_void_p(d_src), sw, sh, C.c_void_p(d_dst), dw, dh, None)
    assert call(0, 60, 40, B, 45, 30) == E                      # null pointers
    assert call(A, 60, 40, 0, 45, 30) == E
    assert call(0, 60, 40, 0, 45, 30) == E
    for bad in (0, -1, -(1 << 31)):                             # every size, zero and negative
        assert call(A, bad, 40, B, 45, 30) == E
        assert call(A, 60, bad, B, 45, 30) == E
        assert call(A, 60, 40, B, bad, 30) == E
        assert call(A, 60, 40, B, 45, bad) == E
    assert call(A, 0, 0, B, 0, 0) == E
    assert w2xc.last_error()
    with pytest.raises(w2xc.W2xcError) as ei:
        w2xc.resize_linear_device(A, 60, 40, B, 0, 30)
    assert ei.value.code == E
    with pytest.raises(w2xc.W2xcError) as ei:
        w2xc.resize_linear_device(0, 60, 40, B, 45, 30)
    assert ei.value.code == E


def test_valid_call_without_a_device(w2xc):
    if w2xc.device_count() != 0:
        return     # (with a device the GPU tests run the call)
    assert w2xc.lib().w2xc_resize_linear_device(C.c_void_p(A), 60, 40, C.c_void_p(B), 45, 30, None) == w2xc.ERR_HIP   # no CPU fallback
    with pytest.raises(w2xc.W2xcError) as ei:
        w2xc.resize_linear_device(A, 1, 1, B, 3, 4)
    assert ei.value.code == w2xc.ERR_HIP
