"""CPU tests of the batch entry points (w2xc_convert_batch / w2xc_convert_batch_device): declared and exported, every argument error comes back as
W2XC_ERR_ARG / W2XC_ERR_PLANES before a device is touched (so also on a box without one), the Python wrapper checks shapes, and the batch kernels'
objects meet the bar of the kernels they are made from (no VGPR spill, no scratch, no SGPR -> VMEM hazard inside asm statements)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, small_layers
from tools import gen_model

LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")
BATCH_OBJS = ["w2xc_wino4_b.o", "w2xc_wino4_bf.o", "w2xc_first2_wino4_b.o", "w2xc_gather_batch.o"]


def _objs(w2xc):
    return [os.path.join(LIB, o) for o in BATCH_OBJS]


def test_batch_symbols_declared_and_exported(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in ("w2xc_convert_batch", "w2xc_convert_batch_device"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    lib.w2xc_version.restype = C.c_char_p
    assert lib.w2xc_version().startswith(b"w2xc_hip 0.4")


@pytest.fixture(scope="module")
def noise1(w2xc):
    return w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["noise1"]))


def _dev(w2xc, ms, n, nn2x, d_in, ips, irs, w, h, d_out, ops, ors, opts=None):
    return w2xc.lib().w2xc_convert_batch_device(ms.handle if ms is not None else None, n, nn2x, C.c_void_p(d_in), ips, irs, w, h, C.c_void_p(d_out),
                                                ops, ors, None, C.byref(opts) if opts is not None else None)


def test_device_form_argument_errors(w2xc, noise1):
    """fake device addresses: every one of these must be refused by the argument checks, never dereferenced"""
    A, B = 0x10000000, 0x90000000
    w, h = 64, 48
    rs, ps = w * 4, w * 4 * h
    good = (A, ps, rs, w, h, B, ps * 4, rs * 2)
    E = w2xc.ERR_ARG
    assert _dev(w2xc, None, 2, 0, *good) == E                                    # null model
    for n in (0, -1):
        assert _dev(w2xc, noise1, n, 0, *good) == E                              # n < 1
    assert _dev(w2xc, noise1, 2, 2, *good) == E                                  # nn2x not 0 / 1
    assert _dev(w2xc, noise1, 2, 0, 0, ps, rs, w, h, B, ps, rs) == E             # null input
    assert _dev(w2xc, noise1, 2, 0, A, ps, rs, w, h, 0, ps, rs) == E             # null output
    for ww, hh in ((0, h), (w, 0), (-3, h), (w, -1)):
        assert _dev(w2xc, noise1, 2, 0, A, ps, rs, ww, hh, B, ps, rs) == E       # non-positive sizes
    assert _dev(w2xc, noise1, 2, 0, A, ps, rs - 4, w, h, B, ps, rs) == E         # short input rows
    assert _dev(w2xc, noise1, 2, 1, A, ps, rs, w, h, B, 4 * ps, rs) == E         # nn2x: output rows hold 2 w
    assert _dev(w2xc, noise1, 2, 0, A, ps, rs + 2, w, h, B, ps, rs) == E         # stride not a multiple of 4
    assert _dev(w2xc, noise1, 2, 0, A, ps + 2, rs, w, h, B, ps, rs) == E         # plane stride not a multiple of 4
    assert _dev(w2xc, noise1, 3, 0, A, ps, rs, w, h, B, ps - rs, rs) == E        # output planes overlap each other
    assert _dev(w2xc, noise1, 3, 0, A, ps, rs, w, h, A + ps, ps, rs) == E        # outputs overlap the inputs
    assert _dev(w2xc, noise1, 1, 0, A, 0, rs, w, h, A, 0, rs) == E               # in place
    # a multi-plane model: W2XC_ERR_PLANES
    ms3 = w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=5))
    assert _dev(w2xc, ms3, 2, 0, *good) == w2xc.ERR_PLANES


def test_host_form_argument_errors(w2xc, noise1):
    lib = w2xc.lib()
    w, h, n = 40, 24, 3
    ins = [np.zeros((h, w), np.float32) for _ in range(n)]
    outs = np.zeros((n, h, w), np.float32)

    def call(ms, n_, nn2x, ip, irs, ww, hh, op, ors):
        return lib.w2xc_convert_batch(ms.handle if ms is not None else None, n_, nn2x, ip, irs, ww, hh, op, ors, None)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)
    ip = arr([a.ctypes.data for a in ins])
    op = arr([outs[i].ctypes.data for i in range(n)])
    E = w2xc.ERR_ARG
    assert call(None, n, 0, ip, w * 4, w, h, op, w * 4) == E
    assert call(noise1, 0, 0, ip, w * 4, w, h, op, w * 4) == E
    assert call(noise1, n, 0, None, w * 4, w, h, op, w * 4) == E
    assert call(noise1, n, 0, ip, w * 4, w, h, None, w * 4) == E
    assert call(noise1, n, 0, arr([ins[0].ctypes.data, None, ins[2].ctypes.data]), w * 4, w, h, op, w * 4) == E   # a null plane
    assert call(noise1, n, 0, ip, w * 4, 0, h, op, w * 4) == E
    assert call(noise1, n, 0, ip, w * 4 - 4, w, h, op, w * 4) == E
    assert call(noise1, n, 1, ip, w * 4, w, h, op, w * 4) == E                 # nn2x output rows too short
    assert call(noise1, n, 0, ip, w * 4, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, outs[0].ctypes.data + 64]), w * 4) == E   # outputs overlap
    assert call(noise1, n, 0, ip, w * 4, w, h, arr([outs[0].ctypes.data, ins[1].ctypes.data, outs[2].ctypes.data]), w * 4) == E          # output = an input
    # the same input plane twice is fine as far as the arguments go (it then needs a device)
    ms3 = w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=5))
    assert call(ms3, n, 0, ip, w * 4, w, h, op, w * 4) == w2xc.ERR_PLANES


def test_python_wrapper_checks_shapes(w2xc, noise1):
    with pytest.raises(ValueError):
        noise1.convert_batch(np.zeros((4, 5), np.float32))                           # 2-D array: not a batch
    with pytest.raises(ValueError):
        noise1.convert_batch([np.zeros((8, 8), np.float32), np.zeros((8, 9), np.float32)])   # mixed sizes
    with pytest.raises(ValueError):
        noise1.convert_batch([])
    with pytest.raises(ValueError):
        noise1.convert_batch(np.zeros((2, 8, 8), np.float32), nn2x=True, out=np.zeros((2, 8, 8), np.float32))   # out of the wrong shape
    if w2xc.device_count() == 0:
        with pytest.raises(w2xc.W2xcError) as ei:
            noise1.convert_batch(np.zeros((2, 8, 8), np.float32))
        assert ei.value.code == w2xc.ERR_HIP   # (no CPU fallback)


def _resources(obj):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), obj], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vspill=int(m.group(4)), scratch=int(m.group(6)))
    return rows


@pytest.mark.parametrize("obj,pattern,count", [
    ("w2xc_wino4_b.o", r"conv3x3_wino4_batchI.*ELb0EEv", 6),
    ("w2xc_wino4_bf.o", r"conv3x3_wino4_batchI.*ELb1EEv", 4),
    ("w2xc_first2_wino4_b.o", r"conv3x3_first2_wino4_batch", 1),
    ("w2xc_gather_batch.o", r"conv3x3_last_gather_x4_batch", 1),
])
def test_batch_kernels_built_without_spills_or_scratch(w2xc, obj, pattern, count):
    rows = {k: v for k, v in _resources(os.path.join(LIB, obj)).items() if re.search(pattern, k)}
    assert len(rows) == count, (obj, sorted(rows))
    bad = {k: v for k, v in rows.items() if v["vspill"] or v["scratch"]}
    assert not bad, bad


@pytest.mark.parametrize("obj", BATCH_OBJS)
def test_batch_kernels_no_sgpr_vmem_hazard(w2xc, obj):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_sgpr_vmem_hazard.py"), os.path.join(LIB, obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "hazards found: 0" in r.stdout


def test_existing_kernels_keep_their_names_in_their_objects(w2xc):
    """the batch forms live in objects of their own: the one-image objects hold no batch kernel, the batch objects no one-image kernel"""
    for obj in ("w2xc_wino4_p.o", "w2xc_wino4_f.o", "w2xc_first2_wino4.o"):
        assert not any("batch" in k for k in _resources(os.path.join(LIB, obj))), obj
    for obj in BATCH_OBJS:
        assert all("batch" in k for k in _resources(os.path.join(LIB, obj))), obj
