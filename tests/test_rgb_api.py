"""CPU tests of the RGB-model surface (w2xc_process_image_rgb_u8_ex[_device], w2xc_process_image_rgb_u8_batch[_device],
w2xc_convert_planes_nn2x_device, w2xc_u8_to_rgb_device, w2xc_rgb_to_u8_device): declared and exported, every argument error comes back as
W2XC_ERR_ARG / W2XC_ERR_PLANES before a device is touched (so also on a box without one), the Python wrappers check shapes and types, the new
kernels neither spill nor use scratch, the CLI picks the route by the model's first layer -- and the Y entry points still refuse RGB models."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, small_layers

LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")
SYMBOLS = ("w2xc_process_image_rgb_u8_ex_device", "w2xc_process_image_rgb_u8_ex", "w2xc_process_image_rgb_u8_batch_device",
           "w2xc_process_image_rgb_u8_batch", "w2xc_convert_planes_nn2x_device", "w2xc_u8_to_rgb_device", "w2xc_rgb_to_u8_device")


def test_symbols_declared_and_exported(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    for name in ("process_image_rgb_u8", "process_image_rgb_u8_device", "process_image_rgb_u8_batch", "process_image_rgb_u8_batch_device",
                 "u8_to_rgb_device", "rgb_to_u8_device"):
        assert callable(getattr(w2xc, name)), name
    assert callable(w2xc._ModelSet.convert_planes_nn2x_device)
    lib.w2xc_version.restype = C.c_char_p
    assert lib.w2xc_version().startswith(b"w2xc_hip 0.4.1")   # the additive revision that carries these symbols (ABI history)


@pytest.fixture(scope="module")
def rgb_a(w2xc):
    return w2xc._ModelSet.from_layers(small_layers([3, 32, 3], seed=11))


@pytest.fixture(scope="module")
def rgb_b(w2xc):
    return w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=12))


@pytest.fixture(scope="module")
def odd_models(w2xc):
    """1 -> 1, 3 -> 1, 1 -> 3: none of them is an RGB model"""
    return [w2xc._ModelSet.from_layers(small_layers(p, seed=13 + i)) for i, p in enumerate(([1, 16, 1], [3, 16, 1], [1, 16, 3]))]


def _h(ms):
    return ms.handle if ms is not None else None


def test_device_batch_form_argument_errors(w2xc, rgb_a, rgb_b, odd_models):
    """fake device addresses: every one of these must be refused by the argument checks, never dereferenced"""
    lib = w2xc.lib()
    A, B = 0x10000000, 0x90000000
    w, h = 64, 48
    rs, ims = w * 3, w * 3 * h                    # input row / image stride
    ors, oms = 2 * w * 3, 2 * w * 3 * 2 * h       # output row / image stride for one iteration

    def call(nm, sm, n, d_in, iis, irs, ww, hh, d_out, ois, ors_, it, shrink=0.0):
        return lib.w2xc_process_image_rgb_u8_batch_device(_h(nm), _h(sm), n, C.c_void_p(d_in), iis, irs, ww, hh, C.c_void_p(d_out), ois, ors_, it,
                                                          shrink, None, None)
    E = w2xc.ERR_ARG
    for n in (0, -1):
        assert call(rgb_a, rgb_b, n, A, ims, rs, w, h, B, oms, ors, 1) == E                    # n < 1
    assert call(rgb_a, rgb_b, 2, 0, ims, rs, w, h, B, oms, ors, 1) == E                        # null input
    assert call(rgb_a, rgb_b, 2, A, ims, rs, w, h, 0, oms, ors, 1) == E                        # null output
    for ww, hh in ((0, h), (w, 0), (-3, h), (w, -1)):
        assert call(rgb_a, rgb_b, 2, A, ims, rs, ww, hh, B, oms, ors, 1) == E                  # non-positive sizes
    for it in (-1, 5):
        assert call(rgb_a, rgb_b, 2, A, ims, rs, w, h, B, 1 << 28, 1 << 14, it) == E           # iterations outside 0..4
    for shrink in (-0.5, 1.0, 1.5):
        assert call(rgb_a, rgb_b, 2, A, ims, rs, w, h, B, oms, ors, 1, shrink) == E            # bad shrink_ratio
    assert call(rgb_a, rgb_b, 2, A, 3, 3, 1, 1, B, 64, 6, 1, 0.25) == E                        # the shrink leaves an empty image (2 * 0.25 -> 0)
    assert call(rgb_a, rgb_b, 2, A, ims, rs - 1, w, h, B, oms, ors, 1) == E                    # input rows below 3 w
    assert call(rgb_a, rgb_b, 2, A, ims, rs, w, h, B, oms, ors - 1, 1) == E                    # output rows below 3 W
    assert call(rgb_a, rgb_b, 3, A, ims, rs, w, h, B, oms - ors, ors, 1) == E                  # output images overlap each other
    assert call(rgb_a, rgb_b, 3, A, ims, rs, w, h, A + ims, oms, ors, 1) == E                  # outputs overlap the inputs
    assert call(rgb_a, None, 1, A, 0, rs, w, h, A, 0, rs, 0) == E                              # in place
    assert call(None, None, 2, A, ims, rs, w, h, B, oms, ors, 1) == E                          # no model at all
    assert call(rgb_a, None, 2, A, ims, rs, w, h, B, oms, ors, 1) == E                         # iterations without a scale model
    assert call(None, rgb_b, 2, A, ims, rs, w, h, B, ims, rs, 0) == E                          # nothing to do
    # models that are not 3 -> 3, in either role, and a Y noise model beside an RGB scale model: W2XC_ERR_PLANES
    P = w2xc.ERR_PLANES
    for bad in odd_models:
        assert call(bad, None, 2, A, ims, rs, w, h, B, ims, rs, 0) == P
        assert call(None, bad, 2, A, ims, rs, w, h, B, oms, ors, 1) == P
        assert call(rgb_a, bad, 2, A, ims, rs, w, h, B, oms, ors, 1) == P
    assert call(odd_models[0], rgb_b, 2, A, ims, rs, w, h, B, oms, ors, 1) == P
    # the single-image device form: the same checks, and an output that overlaps the input
    def one(nm, sm, d_in, irs, ww, hh, d_out, ors_, it, shrink=0.0):
        return lib.w2xc_process_image_rgb_u8_ex_device(_h(nm), _h(sm), C.c_void_p(d_in), irs, ww, hh, C.c_void_p(d_out), ors_, it, shrink, None, None)
    assert one(rgb_a, rgb_b, 0, rs, w, h, B, ors, 1) == E
    assert one(rgb_a, rgb_b, A, rs, w, h, 0, ors, 1) == E
    assert one(rgb_a, rgb_b, A, rs, 0, h, B, ors, 1) == E
    assert one(rgb_a, rgb_b, A, rs, w, h, B, ors, 5) == E
    assert one(rgb_a, rgb_b, A, rs, w, h, B, ors, 1, 1.0) == E
    assert one(rgb_a, rgb_b, A, rs - 1, w, h, B, ors, 1) == E
    assert one(rgb_a, rgb_b, A, rs, w, h, B, ors - 1, 1) == E
    assert one(rgb_a, None, A, rs, w, h, A + rs, rs, 0) == E                                   # overlap
    assert one(None, None, A, rs, w, h, B, ors, 1) == E
    assert one(rgb_a, None, A, rs, w, h, B, ors, 1) == E
    assert one(None, rgb_b, A, rs, w, h, B, rs, 0) == E
    for bad in odd_models:
        assert one(None, bad, A, rs, w, h, B, ors, 1) == P
    assert one(odd_models[0], rgb_b, A, rs, w, h, B, ors, 1) == P
    if w2xc.device_count() == 0:
        assert one(rgb_a, rgb_b, A, rs, w, h, B, ors, 1) == w2xc.ERR_HIP                       # valid arguments: no CPU fallback
        assert call(rgb_a, rgb_b, 2, A, ims, rs, w, h, B, oms, ors, 1) == w2xc.ERR_HIP


def test_host_batch_form_argument_errors(w2xc, rgb_a, rgb_b, odd_models):
    lib = w2xc.lib()
    w, h, n = 40, 24, 3
    ins = [np.zeros((h, w, 3), np.uint8) for _ in range(n)]
    outs = np.zeros((n, 2 * h, 2 * w, 3), np.uint8)
    same = np.zeros((n, h, w, 3), np.uint8)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def call(nm, sm, n_, ip, irs, ww, hh, op, ors, it, shrink=0.0):
        return lib.w2xc_process_image_rgb_u8_batch(_h(nm), _h(sm), n_, ip, irs, ww, hh, op, ors, it, shrink, None)
    ip = arr([a.ctypes.data for a in ins])
    op = arr([outs[i].ctypes.data for i in range(n)])
    op0 = arr([same[i].ctypes.data for i in range(n)])
    rs, ors = w * 3, 2 * w * 3
    E = w2xc.ERR_ARG
    assert call(rgb_a, rgb_b, 0, ip, rs, w, h, op, ors, 1) == E
    assert call(rgb_a, rgb_b, -2, ip, rs, w, h, op, ors, 1) == E
    assert call(rgb_a, rgb_b, n, None, rs, w, h, op, ors, 1) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, None, ors, 1) == E
    assert call(rgb_a, rgb_b, n, arr([ins[0].ctypes.data, None, ins[2].ctypes.data]), rs, w, h, op, ors, 1) == E       # a null in[i]
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, None]), ors, 1) == E     # a null out[i]
    assert call(rgb_a, rgb_b, n, ip, rs, 0, h, op, ors, 1) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, -4, op, ors, 1) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, op, ors, 5) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, op, ors, -1) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, op, ors, 1, 1.0) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, op, ors, 1, -0.1) == E
    assert call(rgb_a, rgb_b, n, ip, 3, 1, 1, op, 6, 1, 0.25) == E                                                    # empty after the shrink
    assert call(rgb_a, rgb_b, n, ip, rs - 1, w, h, op, ors, 1) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, op, ors - 3, 1) == E
    assert call(rgb_a, rgb_b, n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, outs[0].ctypes.data + 64]), ors, 1) == E   # outputs overlap
    assert call(rgb_a, None, n, ip, rs, w, h, arr([same[0].ctypes.data, ins[1].ctypes.data, same[2].ctypes.data]), rs, 0) == E           # output = an input
    assert call(None, None, n, ip, rs, w, h, op, ors, 1) == E
    assert call(rgb_a, None, n, ip, rs, w, h, op, ors, 1) == E
    assert call(None, rgb_b, n, ip, rs, w, h, op0, rs, 0) == E
    P = w2xc.ERR_PLANES
    for bad in odd_models:
        assert call(bad, None, n, ip, rs, w, h, op0, rs, 0) == P
        assert call(None, bad, n, ip, rs, w, h, op, ors, 1) == P
    assert call(odd_models[0], rgb_b, n, ip, rs, w, h, op, ors, 1) == P                       # a Y noise model beside an RGB scale model
    # the single-image host form
    def one(nm, sm, i_, irs, ww, hh, o_, ors_, it, shrink=0.0):
        return lib.w2xc_process_image_rgb_u8_ex(_h(nm), _h(sm), i_, irs, ww, hh, o_, ors_, it, shrink, None)
    assert one(rgb_a, rgb_b, None, rs, w, h, outs[0].ctypes.data, ors, 1) == E
    assert one(rgb_a, rgb_b, ins[0].ctypes.data, rs, w, h, outs[0].ctypes.data, ors - 1, 1) == E
    assert one(None, rgb_b, ins[0].ctypes.data, rs, w, h, same[0].ctypes.data, rs, 0) == E
    assert one(None, odd_models[1], ins[0].ctypes.data, rs, w, h, outs[0].ctypes.data, ors, 1) == P
    if w2xc.device_count() == 0:
        assert call(rgb_a, rgb_b, n, ip, rs, w, h, op, ors, 1) == w2xc.ERR_HIP     # valid arguments: no CPU fallback
        assert call(rgb_a, rgb_b, 1, ip, rs, w, h, op, ors, 1) == w2xc.ERR_HIP
        assert one(rgb_a, rgb_b, ins[0].ctypes.data, rs, w, h, outs[0].ctypes.data, ors, 1) == w2xc.ERR_HIP


def test_planes_nn2x_and_building_block_argument_errors(w2xc, rgb_a):
    lib = w2xc.lib()
    A, B = 0x10000000, 0x90000000
    w, h = 20, 12
    ps, rs, ops, ors = w * h * 4, w * 4, 4 * w * h * 4, 2 * w * 4

    def call(m, n_in, d_in, ips, irs, ww, hh, d_out, ops_, ors_):
        return lib.w2xc_convert_planes_nn2x_device(_h(m), n_in, C.c_void_p(d_in), ips, irs, ww, hh, C.c_void_p(d_out), ops_, ors_, None, None)
    E = w2xc.ERR_ARG
    assert call(None, 3, A, ps, rs, w, h, B, ops, ors) == E
    assert call(rgb_a, 3, 0, ps, rs, w, h, B, ops, ors) == E
    assert call(rgb_a, 3, A, ps, rs, w, h, 0, ops, ors) == E
    assert call(rgb_a, 3, A, ps, rs, 0, h, B, ops, ors) == E
    assert call(rgb_a, 3, A, ps, rs, w, -1, B, ops, ors) == E
    assert call(rgb_a, 0, A, ps, rs, w, h, B, ops, ors) == E
    assert call(rgb_a, 3, A, ps, rs - 4, w, h, B, ops, ors) == E                   # input rows below 4 w
    assert call(rgb_a, 3, A, ps, rs, w, h, B, ops, rs) == E                        # output rows below 4 * 2 w
    assert call(rgb_a, 3, A, ps, rs + 2, w, h, B, ops, ors) == E                   # not a multiple of 4
    assert call(rgb_a, 3, A, ps - 4, rs, w, h, B, ops, ors) == E                   # input planes overlap
    assert call(rgb_a, 3, A, ps, rs, w, h, B, ps, ors) == E                        # output planes of the SOURCE size overlap
    for fn, args in ((lib.w2xc_u8_to_rgb_device, lambda i, s, ww, p: (C.c_void_p(i), s, ww, h, C.c_void_p(p), C.c_void_p(p + ps), C.c_void_p(p + 2 * ps), None)),
                     (lib.w2xc_rgb_to_u8_device, lambda i, s, ww, p: (C.c_void_p(p), C.c_void_p(p + ps), C.c_void_p(p + 2 * ps), ww, h, C.c_void_p(i), s, None))):
        assert fn(*args(0, w * 3, w, B)) == E
        assert fn(*args(A, w * 3, w, 0)) == E
        assert fn(*args(A, w * 3 - 1, w, B)) == E
        assert fn(*args(A, w * 3, 0, B)) == E


def test_python_wrapper_checks(w2xc, rgb_a, rgb_b):
    f = w2xc.process_image_rgb_u8_batch
    with pytest.raises(ValueError):
        f([], rgb_a)                                                                        # empty batch
    with pytest.raises(ValueError):
        f(np.zeros((0, 8, 8, 3), np.uint8), rgb_a)                                          # empty batch, array form
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8)], rgb_a)            # mixed shapes
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 3), np.float32), rgb_a)                                        # wrong dtype
    with pytest.raises(ValueError):
        f(np.zeros((8, 8, 3), np.uint8), rgb_a)                                             # one image is not a batch
    with pytest.raises(ValueError):
        f([np.zeros((8, 8), np.uint8)], rgb_a)                                              # wrong rank
    with pytest.raises(ValueError):
        f([np.zeros((8, 8, 4), np.uint8)], rgb_a)                                           # four channels
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 3), np.uint8), None, rgb_b, 1, out=np.zeros((2, 8, 8, 3), np.uint8))      # out of the wrong shape
    with pytest.raises(ValueError):
        f(np.zeros((2, 8, 8, 3), np.uint8), None, rgb_b, 1, out=np.zeros((2, 16, 16, 3), np.float32))  # out of the wrong dtype
    g = w2xc.process_image_rgb_u8
    with pytest.raises(ValueError):
        g(np.zeros((8, 8, 3), np.float32), rgb_a)
    with pytest.raises(ValueError):
        g(np.zeros((8, 8), np.uint8), rgb_a)
    with pytest.raises(ValueError):
        g(np.zeros((8, 8, 1), np.uint8), rgb_a)
    with pytest.raises(w2xc.W2xcError) as ei:
        g(np.zeros((8, 8, 3), np.uint8), None, None)
    assert ei.value.code == w2xc.ERR_ARG
    if w2xc.device_count() == 0:
        for call in (lambda: f(np.zeros((2, 8, 8, 3), np.uint8), rgb_a, rgb_b, 1), lambda: g(np.zeros((8, 8, 3), np.uint8), rgb_a, rgb_b, 1)):
            with pytest.raises(w2xc.W2xcError) as ei:
                call()
            assert ei.value.code == w2xc.ERR_HIP   # (no CPU fallback)


def test_y_entry_points_still_refuse_rgb_models(w2xc, rgb_a):
    """what tests/test_image_batch_api.py pins, seen from this side: the Y calls did not start to accept three-plane models"""
    lib = w2xc.lib()
    w, h, n = 16, 8, 2
    ins = [np.zeros((h, w, 3), np.uint8) for _ in range(n)]
    outs = np.zeros((n, h, w, 3), np.uint8)
    ip = (C.c_void_p * n)(*[a.ctypes.data for a in ins])
    op = (C.c_void_p * n)(*[outs[i].ctypes.data for i in range(n)])
    assert lib.w2xc_process_image_u8_batch(rgb_a.handle, None, n, ip, w * 3, w, h, op, w * 3, 0, 0.0, None) == w2xc.ERR_PLANES
    assert lib.w2xc_process_image_u8_batch_device(rgb_a.handle, None, n, C.c_void_p(0x10000000), w * 3 * h, w * 3, w, h, C.c_void_p(0x90000000),
                                                  w * 3 * h, w * 3, 0, 0.0, None, None) == w2xc.ERR_PLANES


def test_plan_rows_unchanged_for_rgb_models(w2xc):
    """w2xc_plan_rows plans a 3 -> ... -> 3 model as before: no fused first / last layers (those are the one-plane fusions), same workspaces with
    every fusion setting -- the uint8 forms of the first and last layer change no geometry"""
    from tools import gen_model
    ms = w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 32, 32, 64, 64, 128, 128, 3], 301))
    plans = [ms.plan_rows(106, 74, opts=w2xc.make_opts(fusion=f)) for f in (w2xc.FUSION_AUTO, w2xc.FUSION_OFF)]
    for p in plans:
        assert (p.n_layers, p.halo_rows_per_layer, p.n_bands, p.fused_first, p.fused_last) == (7, 4, 1, 0, 0)
    assert list(plans[0].workspace_bytes) == list(plans[1].workspace_bytes)
    assert [ms.kernel_name(l) for l in (0, 6)] == ["conv3x3_first", "conv3x3_last"]


def test_new_kernels_no_spill_no_scratch(w2xc):
    def rows(obj):
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, obj)], capture_output=True,
                             text=True, check=True).stdout
        r = {}
        for line in out.splitlines():
            m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
            if m:
                r[m.group(1)] = dict(vspill=int(m.group(4)), scratch=int(m.group(6)))
        return r
    colour = rows("w2xc_color.o")
    # the stage names, as they stand in the mangled k_px<Stage>.  Two stages where there were four kernels: the one-image kernels are gone, one image is
    # the same kernel launched with n = 1
    for k in ("U8ToRgb", "RgbToU8"):
        hit = [name for name in colour if k in name]
        assert len(hit) == 1, (k, sorted(colour))
        assert colour[hit[0]] == dict(vspill=0, scratch=0), (hit[0], colour[hit[0]])
    conv = rows("w2xc_kernels.o")
    # the uint8 instantiations: conv3x3_first<3, NBT, PLANAR, true> (Itanium: ...ELb?ELb1EE) and conv3x3_last<CIN, 3, true>
    first = [name for name in conv if re.search(r"conv3x3_firstILi3ELi\dELb[01]ELb1EE", name)]
    last = [name for name in conv if re.search(r"conv3x3_lastILi\d+ELi3ELb1EE", name)]
    assert len(first) == 6 and len(last) == 3, (first, last)
    for name in first + last:
        assert conv[name] == dict(vspill=0, scratch=0), (name, conv[name])


def _cli():
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_route_by_first_layer():
    cli = _cli()
    assert cli.model_route(None, ("scale2.0x_model.json", 3)) == "rgb"
    assert cli.model_route(("noise1_model.json", 3), ("scale2.0x_model.json", 3)) == "rgb"
    assert cli.model_route(("noise1_model.json", 1), None) == "y"
    assert cli.model_route(("noise1_model.json", 1), ("scale2.0x_model.json", 1)) == "y"
    with pytest.raises(SystemExit) as ei:                       # mixed kinds: a message, not a traceback
        cli.model_route(("noise1_model.json", 1), ("scale2.0x_model.json", 3))
    assert "mixed model kinds" in str(ei.value.code) and "noise1_model.json" in str(ei.value.code)
    with pytest.raises(SystemExit):
        cli.model_route(None, ("scale2.0x_model.json", 2))
