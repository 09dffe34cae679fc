"""CPU tests of the batched chain of multi-plane (RGB) models, revision 0.4.1.5: w2xc_convert_planes_batch_device and w2xc_batch_plan are declared,
exported, in the ctypes table and wrapped; every argument error is refused before a device is touched (so also on a box without one); w2xc_batch_plan --
pure host arithmetic -- pins which models and option sets run the batched chain and how a sub-batch shrinks with the workspace budget; and the objects of the
new batch kernels meet the bar of the kernels they are made from (no VGPR spill, no scratch, no SGPR -> VMEM hazard inside asm statements)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, small_layers

LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")
NEW = ("w2xc_convert_planes_batch_device", "w2xc_batch_plan")
RGB7 = [3, 32, 32, 64, 64, 128, 128, 3]
BATCHED = {"rgb7": RGB7, "rgb4": [3, 32, 64, 64, 3], "rgb3": [3, 32, 64, 3], "first_planar64": [3, 64, 64, 3], "first_planar128": [3, 128, 128, 3],
           "wino_behind_wino4": [3, 32, 64, 32, 64, 3], "two_layers": [3, 32, 3], "y7": [1, 32, 32, 64, 64, 128, 128, 1]}


@pytest.fixture(scope="module")
def sets(w2xc):
    return {k: w2xc._ModelSet.from_layers(small_layers(v, seed=400 + i)) for i, (k, v) in enumerate(sorted(BATCHED.items()))}


def test_symbols_declared_exported_and_wrapped(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS, name
    assert callable(getattr(w2xc._ModelSet, "convert_planes_batch_device"))
    assert callable(getattr(w2xc._ModelSet, "batch_plan"))
    lib.w2xc_version.restype = C.c_char_p
    assert lib.w2xc_version().startswith(b"w2xc_hip 0.4.1")
    assert C.sizeof(w2xc.Opts) == 56
    for doc in ("INTEGRATION.md", os.path.join("waifu2x-converter-cpp_amd", "csrc", "w2xc_model.cpp")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "0.4.1.5" in text and all(n in text for n in NEW), doc


def _dev(w2xc, ms, n, nn2x, nin, d_in, iis, ips, irs, w, h, d_out, ois, ops, ors, opts=None):
    return w2xc.lib().w2xc_convert_planes_batch_device(ms.handle if ms is not None else None, n, nn2x, nin, C.c_void_p(d_in), iis, ips, irs, w, h,
                                                       C.c_void_p(d_out), ois, ops, ors, None, C.byref(opts) if opts is not None else None)


def test_argument_errors_without_a_device(w2xc, sets):
    """fake device addresses: every one of these is refused by the argument checks, never dereferenced"""
    ms = sets["rgb4"]
    A, B = 0x10000000, 0x90000000
    w, h = 64, 48
    rs, ps = w * 4, w * 4 * h
    im = 3 * ps
    E = w2xc.ERR_ARG

    def call(n=2, nn2x=0, nin=3, d_in=A, iis=im, ips=ps, irs=rs, ww=w, hh=h, d_out=B, ois=im, ops=ps, ors=rs, m=ms, opts=None):
        return _dev(w2xc, m, n, nn2x, nin, d_in, iis, ips, irs, ww, hh, d_out, ois, ops, ors, opts)
    assert call(m=None) == E                                           # null model
    for n in (0, -1):
        assert call(n=n) == E                                          # n < 1
    assert call(nn2x=2) == E and call(nn2x=-1) == E                    # nn2x not 0 / 1
    assert call(d_in=0) == E and call(d_out=0) == E                    # null pointers
    for ww, hh in ((0, h), (w, 0), (-3, h), (w, -1)):
        assert call(ww=ww, hh=hh) == E                                 # non-positive sizes
    assert call(irs=rs - 4) == E and call(ors=rs - 4) == E             # short rows
    assert call(nn2x=1, ois=4 * im, ops=4 * ps, ors=rs) == E           # nn2x: output rows hold 2 w
    assert call(irs=rs + 2) == E and call(ors=rs + 2) == E             # row strides: multiples of 4
    assert call(ips=ps + 2) == E and call(ops=ps + 2) == E             # plane strides: multiples of 4
    assert call(iis=im + 2) == E and call(ois=im + 2) == E             # image strides: multiples of 4
    assert call(ips=ps - rs) == E and call(ops=ps - rs) == E           # planes of an image overlap
    assert call(nin=0) == E                                            # no input plane
    assert call(n=3, ois=im - rs) == E                                 # output images overlap each other
    assert call(n=3, d_out=A + im) == E                                # outputs overlap the inputs
    assert call(n=1, d_out=A) == E                                     # in place
    assert call(opts=w2xc.make_opts(precision=77)) in (E, w2xc.ERR_UNSUPPORTED)   # unknown precision
    assert call(nin=1, iis=ps) == w2xc.ERR_PLANES                      # the model takes three planes
    assert call(m=sets["y7"]) == w2xc.ERR_PLANES                       # ... or one
    assert "planes" in w2xc.last_error()


def test_batch_plan_argument_errors(w2xc, sets):
    ms = sets["rgb4"]
    lib = w2xc.lib()
    b, s = C.c_int(-1), C.c_int(-1)
    E = w2xc.ERR_ARG
    assert lib.w2xc_batch_plan(None, 3, 64, 64, 0, None, C.byref(b), C.byref(s)) == E
    assert lib.w2xc_batch_plan(ms.handle, 3, 64, 64, 0, None, None, C.byref(s)) == E
    assert lib.w2xc_batch_plan(ms.handle, 3, 64, 64, 0, None, C.byref(b), None) == E
    assert lib.w2xc_batch_plan(ms.handle, 3, 64, 64, 2, None, C.byref(b), C.byref(s)) == E
    assert lib.w2xc_batch_plan(ms.handle, 3, 0, 64, 0, None, C.byref(b), C.byref(s)) == E
    assert lib.w2xc_batch_plan(ms.handle, 3, 64, -1, 0, None, C.byref(b), C.byref(s)) == E
    assert lib.w2xc_batch_plan(ms.handle, 1, 64, 64, 0, None, C.byref(b), C.byref(s)) == w2xc.ERR_PLANES
    with pytest.raises(w2xc.W2xcError) as ei:
        ms.batch_plan(2, 64, 64)
    assert ei.value.code == w2xc.ERR_PLANES


@pytest.mark.parametrize("name", sorted(BATCHED))
@pytest.mark.parametrize("nn2x", [False, True])
def test_batch_plan_default_options_batched(w2xc, sets, name, nn2x):
    nin = BATCHED[name][0]
    for w, h in ((1, 1), (33, 9), (64, 64), (53, 37), (512, 512)):
        batched, sub = sets[name].batch_plan(nin, w, h, nn2x)
        assert batched == 1 and sub >= 1, (name, w, h, batched, sub)
        assert (batched, sub) == sets[name].batch_plan(nin, w, h, nn2x, w2xc.make_opts()), "explicit default options"


def test_batch_plan_not_batched(w2xc, sets):
    ms = sets["rgb7"]
    for p in (w2xc.PRECISION_BF16, w2xc.PRECISION_BF16X2, w2xc.PRECISION_BF16X3, w2xc.PRECISION_FP16X2):
        assert ms.batch_plan(3, 64, 64, True, w2xc.make_opts(precision=p)) == (0, 1), p
    for k in (w2xc.KERNEL_DIRECT, w2xc.KERNEL_MFMA, w2xc.KERNEL_WINOGRAD, w2xc.KERNEL_WINOGRAD32, w2xc.KERNEL_WINOGRAD4):
        assert ms.batch_plan(3, 64, 64, True, w2xc.make_opts(kernel=k)) == (0, 1), k
    assert ms.batch_plan(3, 64, 64, True, w2xc.make_opts(fusion=w2xc.FUSION_PROG)) == (0, 1)
    for f in (w2xc.FUSION_OFF, w2xc.FUSION_ON, w2xc.FUSION_FIRST, w2xc.FUSION_LAST, w2xc.FUSION_GATHER_LAUNCH):
        assert ms.batch_plan(3, 64, 64, True, w2xc.make_opts(fusion=f))[0] == 1, f   # (the uint8 forms and the float forms both have batch kernels)
    # a workspace so small that the image is banded
    o = w2xc.make_opts(workspace_mb=1)
    plan = ms.plan_rows(256, 256, opts=o)
    assert plan.band_rows < 256
    assert ms.batch_plan(3, 128, 128, True, o) == (0, 1)
    assert ms.batch_plan(3, 128, 128, True, w2xc.make_opts(band_rows=64)) == (0, 1)
    # three planes in, one plane out: no chain of either kind
    m31 = w2xc._ModelSet.from_layers(small_layers([3, 32, 64, 64, 1], seed=431))
    assert m31.batch_plan(3, 64, 64) == (0, 1)
    # a plane count without conv3x3_first / a mid layer without a fast kernel
    m2 = w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=432))
    assert m2.batch_plan(3, 64, 64) == (0, 1)
    m48 = w2xc._ModelSet.from_layers(small_layers([3, 32, 48, 3], seed=433))
    assert m48.batch_plan(3, 64, 64) == (0, 1)


def test_sub_batch_shrinks_with_the_workspace(w2xc, sets):
    for name in ("rgb7", "y7"):
        ms, nin = sets[name], BATCHED[name][0]
        subs = []
        for mb in (16384, 4096, 1024, 256, 64):
            batched, sub = ms.batch_plan(nin, 64, 64, True, w2xc.make_opts(workspace_mb=mb))
            assert batched == 1 and sub >= 1, (name, mb)
            subs.append(sub)
        assert subs == sorted(subs, reverse=True) and subs[0] > subs[-1], (name, subs)
        assert subs[-1] * 4 <= subs[-2], (name, subs)   # (floor(B / per) * 4 <= floor(4 B / per))
        assert ms.batch_plan(nin, 64, 64, True)[1] == subs[0], "workspace_mb = 0 is the 16 GiB default"


# ---- the new kernels' objects ----
def _resources(obj):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), obj], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vspill=int(m.group(4)), scratch=int(m.group(6)))
    return rows


NEW_OBJS = [("w2xc_conv_batch.o", r"conv3x3_first_batch", 12), ("w2xc_conv_batch.o", r"conv3x3_last_batch", 6), ("w2xc_wino_b.o", r"conv3x3_wino_batch", 3),
            ("w2xc_wino4_bi.o", r"conv3x3_wino4_batch_lILi32E.*Lb1EEv", 4), ("w2xc_wino4_bo.o", r"conv3x3_wino4_batch_lI.*Lb0ELb0EEv", 4)]


@pytest.mark.parametrize("obj,pattern,count", NEW_OBJS)
def test_new_batch_kernels_built_without_spills_or_scratch(w2xc, obj, pattern, count):
    rows = {k: v for k, v in _resources(os.path.join(LIB, obj)).items() if re.search(pattern, k)}
    assert len(rows) == count, (obj, sorted(rows))
    bad = {k: v for k, v in rows.items() if v["vspill"] or v["scratch"]}
    assert not bad, bad


@pytest.mark.parametrize("obj", sorted({o for o, _, _ in NEW_OBJS}))
def test_new_batch_kernels_no_sgpr_vmem_hazard(w2xc, obj):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_sgpr_vmem_hazard.py"), os.path.join(LIB, obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "hazards found: 0" in r.stdout


def test_batch_forms_live_in_objects_of_their_own(w2xc):
    for obj in ("w2xc_kernels.o", "w2xc_wino.o", "w2xc_wino4_p.o", "w2xc_wino4_n.o"):
        assert not any("batch" in k for k in _resources(os.path.join(LIB, obj))), obj
    for obj in sorted({o for o, _, _ in NEW_OBJS}):
        assert all("batch" in k for k in _resources(os.path.join(LIB, obj))), obj
