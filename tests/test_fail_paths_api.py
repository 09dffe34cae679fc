"""w2xc_debug_fail_nth without a device: the symbol, the header's text and the binding are there, bad arguments arm nothing, and a process in which no call
reaches a device counts no event.  What the seam is for runs on the GPU: tests/test_gpu_fail_paths.py, through the loop of tests/fail_cases.py."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
import fail_cases as fc
import stream_cases as sc
import test_stream_cases as tsc

HEADER = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
KINDS = {"ALLOC": 1, "COPY": 2, "LAUNCH": 3}


def test_symbol_header_and_binding(w2xc):
    lib = C.CDLL(w2xc.LIB_PATH)
    assert hasattr(lib, "w2xc_debug_fail_nth") and "w2xc_debug_fail_nth" in w2xc.ABI_SYMBOLS
    assert re.search(r"long long\s+w2xc_debug_fail_nth\s*\(\s*int kind\s*,\s*long long nth\s*\)\s*;", HEADER)
    for name, value in KINDS.items():
        assert re.search(r"#define\s+W2XC_DEBUG_FAIL_%s\s+%d\b" % (name, value), HEADER), name
        assert getattr(w2xc, "DEBUG_FAIL_" + name) == value == getattr(fc, name)
    # the header says what each kind returns and what the call is: a test aid beside w2xc_debug_fill_scratch
    doc = HEADER[HEADER.index("w2xc_debug_fill_scratch(w2xc_model *m"):HEADER.index("long long w2xc_debug_fail_nth")]
    assert "Test aid" in doc and "W2XC_ERR_NOMEM" in doc and "W2XC_ERR_HIP" in doc and "disarm" in doc
    assert callable(w2xc.debug_fail_nth)
    # additive: the options struct and the version string stay
    assert C.sizeof(w2xc.Opts) == 56 and w2xc.lib().w2xc_version() == b"w2xc_hip 0.4.1.6.1 (gfx950)"


def test_bad_arguments_arm_nothing(w2xc):
    for kind in (0, 4, -1, 1 << 20):
        assert w2xc.debug_fail_nth(kind, 1) == -1 and w2xc.debug_fail_nth(kind, 0) == -1
    for kind in KINDS.values():
        assert w2xc.debug_fail_nth(kind, -1) == -1 and w2xc.debug_fail_nth(kind, -(1 << 40)) == -1
        assert w2xc.debug_fail_nth(kind, 0) >= 0


def test_without_a_device_the_counters_read_zero(w2xc, noise1_layers):
    """a call that is refused before a device is touched, or that finds no device, is no event; arming and disarming alone count nothing"""
    if w2xc.device_count() > 0:
        return      # (on a GPU machine the events are counted by tests/test_gpu_fail_paths.py)
    ms = w2xc._ModelSet.from_layers(noise1_layers)
    for kind in KINDS.values():
        w2xc.debug_fail_nth(kind, 0)
        assert w2xc.debug_fail_nth(kind, 3) == 0
    x = np.zeros((17, 33), np.float32)
    for call in (lambda: ms.convert(x), lambda: ms.filter(0, [x]), lambda: ms.convert_batch(np.stack([x, x]))):
        try:
            call()
            raise AssertionError("a compute call came back without a device")
        except w2xc.W2xcError as e:
            assert e.code == w2xc.ERR_HIP
    for kind in KINDS.values():
        assert w2xc.debug_fail_nth(kind, 0) == 0, "an event without a device"
        assert w2xc.debug_fail_nth(kind, 0) == 0


def test_the_stream_table_is_still_complete(w2xc):
    """the new entry point takes no stream and is no device call: tests/test_stream_cases.py's table needs no row for it"""
    assert tsc.uncovered(w2xc, sc.ROWS) == []
    assert "w2xc_debug_fail_nth" not in tsc.stream_prototypes()
    assert "debug_fail_nth" not in tsc.device_callables(w2xc)


def test_the_loop_names_every_buffer_of_the_engine():
    """fail_cases.BUFFERS is every `what` of a Scratch::reserve in the engine's sources and upload's: an ALLOC message names one of them"""
    csrc = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")
    found = set()
    for f in os.listdir(csrc):
        if f.endswith((".cpp", ".hpp")):
            text = open(os.path.join(csrc, f)).read()
            found |= set(re.findall(r"\breserve\([^;]*?\"([^\"]+)\"\s*\)", text))
    found.add("a weight image")     # upload's (w2xc_model.cpp, below)
    assert {"the activation workspace", "the band buffer", "the job flags", "the input rows"} <= found
    assert found == set(fc.BUFFERS), sorted(found ^ set(fc.BUFFERS))
    assert "for a weight image failed" in open(os.path.join(csrc, "w2xc_model.cpp")).read()
