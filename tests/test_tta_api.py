"""CPU tests of the test-time-augmentation surface (include/w2xc_hip.h, "TTA"): the twelve symbols are declared, exported and mirrored and w2xc_opts
keeps its 56 bytes; every argument error of every new call comes back before a device is touched (fake device addresses are never dereferenced), valid
calls without a device return W2XC_ERR_HIP; the two kernels neither spill nor use scratch; the CLI parses --tta and refuses it with transparency."""
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
IMAGE_SYMBOLS = ("w2xc_process_image_u8_tta", "w2xc_process_image_u8_tta_device", "w2xc_process_image_u8_batch_tta",
                 "w2xc_process_image_u8_batch_tta_device", "w2xc_process_image_rgb_u8_tta", "w2xc_process_image_rgb_u8_tta_device",
                 "w2xc_process_image_rgb_u8_batch_tta", "w2xc_process_image_rgb_u8_batch_tta_device")
SYMBOLS = IMAGE_SYMBOLS + ("w2xc_convert_batch_tta_device", "w2xc_convert_planes_tta_device", "w2xc_tta_spread_device", "w2xc_tta_gather_device")
A, B, D = 0x10000000, 0x90000000, 0x50000000    # fake device addresses


def test_symbols_declared_exported_mirrored(w2xc):
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    lib.w2xc_version.restype = C.c_char_p
    assert lib.w2xc_version().startswith(b"w2xc_hip 0.4.1")
    assert C.sizeof(w2xc.Opts) == 56
    o = w2xc.make_opts()
    assert o.struct_size == 56


@pytest.fixture(scope="module")
def noise1(w2xc):
    return w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["noise1"]))


@pytest.fixture(scope="module")
def scale2(w2xc):
    return w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]))


@pytest.fixture(scope="module")
def rgb3(w2xc):
    return w2xc._ModelSet.from_layers(small_layers([3, 16, 3], seed=5))


def _h(ms):
    return ms.handle if ms is not None else None


W, H = 64, 48
RS, IMS, ORS, OMS = W * 3, W * 3 * H, 2 * W * 3, 2 * W * 3 * 2 * H


def single_device(w2xc, rgb):
    f = w2xc.lib().w2xc_process_image_rgb_u8_tta_device if rgb else w2xc.lib().w2xc_process_image_u8_tta_device
    return lambda nm, sm, d_in, irs, w, h, d_out, ors, it, tta, shrink=0.0: f(_h(nm), _h(sm), C.c_void_p(d_in), irs, w, h, C.c_void_p(d_out), ors, it,
                                                                             shrink, None, None, tta)


def batch_device(w2xc, rgb):
    f = w2xc.lib().w2xc_process_image_rgb_u8_batch_tta_device if rgb else w2xc.lib().w2xc_process_image_u8_batch_tta_device
    return lambda nm, sm, n, d_in, iis, irs, w, h, d_out, ois, ors, it, tta, shrink=0.0: f(_h(nm), _h(sm), n, C.c_void_p(d_in), iis, irs, w, h,
                                                                                          C.c_void_p(d_out), ois, ors, it, shrink, None, None, tta)


@pytest.mark.parametrize("rgb", [False, True], ids=["y", "rgb"])
def test_image_device_forms_argument_errors(w2xc, noise1, scale2, rgb3, rgb):
    E = w2xc.ERR_ARG
    nm, sm = (rgb3, rgb3) if rgb else (noise1, scale2)
    one, many = single_device(w2xc, rgb), batch_device(w2xc, rgb)
    for tta in (2, -1, 8):
        assert one(nm, sm, A, RS, W, H, B, ORS, 1, tta) == E                               # tta outside {0, 1}
        assert many(nm, sm, 2, A, IMS, RS, W, H, B, OMS, ORS, 1, tta) == E
    for tta in (0, 1):
        assert one(nm, sm, 0, RS, W, H, B, ORS, 1, tta) == E                               # null pointers
        assert one(nm, sm, A, RS, W, H, 0, ORS, 1, tta) == E
        assert many(nm, sm, 2, 0, IMS, RS, W, H, B, OMS, ORS, 1, tta) == E
        assert many(nm, sm, 2, A, IMS, RS, W, H, 0, OMS, ORS, 1, tta) == E
        assert one(nm, sm, A, RS - 1, W, H, B, ORS, 1, tta) == E                           # strides too small
        assert one(nm, sm, A, RS, W, H, B, ORS - 1, 1, tta) == E
        assert many(nm, sm, 2, A, IMS, RS - 1, W, H, B, OMS, ORS, 1, tta) == E
        assert many(nm, sm, 2, A, IMS, RS, W, H, B, OMS, ORS - 1, 1, tta) == E
        assert many(nm, sm, 3, A, IMS, RS, W, H, B, OMS - ORS, ORS, 1, tta) == E           # output images overlap each other
        assert many(nm, sm, 3, A, IMS, RS, W, H, A + IMS, OMS, ORS, 1, tta) == E           # outputs overlap the inputs
        assert many(nm, sm, 0, A, IMS, RS, W, H, B, OMS, ORS, 1, tta) == E                 # n < 1
        assert one(None, None, A, RS, W, H, B, ORS, 1, tta) == E                           # no model
        assert one(nm, None, A, RS, W, H, B, ORS, 1, tta) == E                             # iterations without a scale model
        assert one(nm, sm, A, RS, W, H, B, ORS, 5, tta) == E
        assert one(nm, sm, A, RS, W, H, B, ORS, 1, tta, 1.0) == E                          # bad shrink_ratio
        if rgb:
            assert one(nm, sm, A, RS, W, H, A + RS, ORS, 1, tta) == E                      # the output overlaps the input
    # a Y model in an RGB call, an RGB model in a Y call: W2XC_ERR_PLANES, before a device is touched
    P = w2xc.ERR_PLANES
    rone, rmany = single_device(w2xc, True), batch_device(w2xc, True)
    for tta in (0, 1):
        assert rone(noise1, None, A, RS, W, H, B, RS, 0, tta) == P
        assert rone(rgb3, scale2, A, RS, W, H, B, ORS, 1, tta) == P
        assert rmany(None, scale2, 2, A, IMS, RS, W, H, B, OMS, ORS, 1, tta) == P
    yone, ymany = single_device(w2xc, False), batch_device(w2xc, False)
    assert yone(rgb3, None, A, RS, W, H, B, RS, 0, 1) == P
    assert ymany(noise1, rgb3, 2, A, IMS, RS, W, H, B, OMS, ORS, 1, 1) == P


@pytest.mark.parametrize("rgb", [False, True], ids=["y", "rgb"])
def test_image_host_forms_argument_errors(w2xc, noise1, scale2, rgb3, rgb):
    lib = w2xc.lib()
    E = w2xc.ERR_ARG
    nm, sm = (rgb3, rgb3) if rgb else (noise1, scale2)
    w, h, n = 40, 24, 3
    img = np.zeros((h, w, 3), np.uint8)
    out = np.zeros((2 * h, 2 * w, 3), np.uint8)
    ins = [np.zeros((h, w, 3), np.uint8) for _ in range(n)]
    outs = np.zeros((n, 2 * h, 2 * w, 3), np.uint8)
    one = lib.w2xc_process_image_rgb_u8_tta if rgb else lib.w2xc_process_image_u8_tta
    many = lib.w2xc_process_image_rgb_u8_batch_tta if rgb else lib.w2xc_process_image_u8_batch_tta

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)
    ip, op = arr([a.ctypes.data for a in ins]), arr([outs[i].ctypes.data for i in range(n)])
    rs, ors = w * 3, 2 * w * 3
    for tta in (2, -1):
        assert one(_h(nm), _h(sm), img.ctypes.data, rs, w, h, out.ctypes.data, ors, 1, 0.0, None, tta) == E
        assert many(_h(nm), _h(sm), n, ip, rs, w, h, op, ors, 1, 0.0, None, tta) == E
    for tta in (0, 1):
        assert one(_h(nm), _h(sm), None, rs, w, h, out.ctypes.data, ors, 1, 0.0, None, tta) == E
        assert one(_h(nm), _h(sm), img.ctypes.data, rs, w, h, None, ors, 1, 0.0, None, tta) == E
        assert one(_h(nm), _h(sm), img.ctypes.data, rs - 1, w, h, out.ctypes.data, ors, 1, 0.0, None, tta) == E
        assert one(_h(nm), _h(sm), img.ctypes.data, rs, w, h, out.ctypes.data, ors - 1, 1, 0.0, None, tta) == E
        assert many(_h(nm), _h(sm), n, None, rs, w, h, op, ors, 1, 0.0, None, tta) == E
        assert many(_h(nm), _h(sm), n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, None]), ors, 1, 0.0, None, tta) == E
        assert many(_h(nm), _h(sm), n, ip, rs, w, h, op, ors - 3, 1, 0.0, None, tta) == E
        assert many(_h(nm), _h(sm), n, ip, rs, w, h, arr([outs[0].ctypes.data, outs[1].ctypes.data, outs[0].ctypes.data + 64]), ors, 1, 0.0, None, tta) == E
        if w2xc.device_count() == 0:     # valid arguments: no CPU fallback
            assert one(_h(nm), _h(sm), img.ctypes.data, rs, w, h, out.ctypes.data, ors, 1, 0.0, None, tta) == w2xc.ERR_HIP
            assert many(_h(nm), _h(sm), n, ip, rs, w, h, op, ors, 1, 0.0, None, tta) == w2xc.ERR_HIP
    other = scale2 if rgb else rgb3     # a model of the other kind
    assert one(_h(other), None, img.ctypes.data, rs, w, h, img.ctypes.data + 0, rs, 0, 0.0, None, 1) in (w2xc.ERR_PLANES, E)
    assert one(_h(nm), _h(other), img.ctypes.data, rs, w, h, out.ctypes.data, ors, 1, 0.0, None, 1) == w2xc.ERR_PLANES
    assert many(_h(nm), _h(other), n, ip, rs, w, h, op, ors, 1, 0.0, None, 1) == w2xc.ERR_PLANES


def test_python_keyword(w2xc, noise1, scale2):
    for f in (w2xc.process_image_u8, w2xc.process_image_rgb_u8, w2xc.process_image_u8_batch, w2xc.process_image_rgb_u8_batch,
              w2xc.process_image_u8_device, w2xc.process_image_rgb_u8_device, w2xc.process_image_u8_batch_device,
              w2xc.process_image_rgb_u8_batch_device):
        assert f.__kwdefaults__ is None and "tta" in f.__code__.co_varnames and f.__defaults__[-1] is False, f.__name__
    assert hasattr(w2xc._ModelSet, "convert_batch_tta_device") and hasattr(w2xc._ModelSet, "convert_planes_tta_device")
    if w2xc.device_count() == 0:
        with pytest.raises(w2xc.W2xcError) as ei:
            w2xc.process_image_u8(np.zeros((8, 8, 3), np.uint8), noise1, scale2, 1, tta=True)
        assert ei.value.code == w2xc.ERR_HIP
        with pytest.raises(w2xc.W2xcError) as ei:
            w2xc.process_image_u8_batch(np.zeros((2, 8, 8, 3), np.uint8), noise1, scale2, 1, tta=True)
        assert ei.value.code == w2xc.ERR_HIP


def test_plane_calls_argument_errors(w2xc, noise1, scale2, rgb3):
    lib = w2xc.lib()
    E = w2xc.ERR_ARG
    w, h = 40, 24

    def batch(ms, n, nn2x, d_in, ips, irs, ww, hh, d_out, ops, ors):
        return lib.w2xc_convert_batch_tta_device(_h(ms), n, nn2x, C.c_void_p(d_in), ips, irs, ww, hh, C.c_void_p(d_out), ops, ors, None, None)
    ps, PS = w * h * 4, 4 * w * h * 4
    assert batch(None, 2, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert batch(scale2, 0, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert batch(scale2, 2, 2, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == E                  # nn2x outside {0, 1}
    assert batch(scale2, 2, 1, 0, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert batch(scale2, 2, 1, A, ps, w * 4, w, h, 0, PS, 2 * w * 4) == E
    assert batch(scale2, 2, 1, A, ps, w * 4 - 4, w, h, B, PS, 2 * w * 4) == E              # strides too small
    assert batch(scale2, 2, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4 - 4) == E
    assert batch(scale2, 2, 1, A, ps, w * 4 + 2, w, h, B, PS, 2 * w * 4) == E              # not a multiple of 4
    assert batch(scale2, 2, 1, A, ps, w * 4, 0, h, B, PS, 2 * w * 4) == E
    assert batch(scale2, 2, 1, A, ps, w * 4, w, h, B, PS - 8, 2 * w * 4) == E              # output planes overlap each other
    assert batch(scale2, 2, 0, A, ps, w * 4, w, h, A + ps, ps, w * 4) == E                 # outputs overlap the inputs
    assert batch(rgb3, 2, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == w2xc.ERR_PLANES

    def planes(ms, n_in, nn2x, d_in, ips, irs, ww, hh, d_out, ops, ors, opts=None):
        return lib.w2xc_convert_planes_tta_device(_h(ms), n_in, nn2x, C.c_void_p(d_in), ips, irs, ww, hh, C.c_void_p(d_out), ops, ors, None,
                                                  C.byref(opts) if opts is not None else None)
    assert planes(None, 3, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert planes(rgb3, 3, 2, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert planes(rgb3, 3, -1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert planes(rgb3, 0, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert planes(rgb3, 3, 1, 0, ps, w * 4, w, h, B, PS, 2 * w * 4) == E
    assert planes(rgb3, 3, 1, A, ps, w * 4, w, h, 0, PS, 2 * w * 4) == E
    assert planes(rgb3, 3, 1, A, ps, w * 4 - 4, w, h, B, PS, 2 * w * 4) == E
    assert planes(rgb3, 3, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4 - 4) == E
    assert planes(rgb3, 3, 1, A, ps - 4, w * 4, w, h, B, PS, 2 * w * 4) == E               # input planes overlap
    assert planes(rgb3, 3, 1, A, ps, w * 4, w, h, B, PS - 4, 2 * w * 4) == E
    assert planes(rgb3, 3, 0, A, ps, w * 4, w, -2, B, ps, w * 4) == E
    assert planes(rgb3, 1, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == w2xc.ERR_PLANES     # the model takes three planes
    assert planes(scale2, 3, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4) == w2xc.ERR_PLANES
    assert planes(rgb3, 3, 1, A, ps, w * 4, w, h, B, PS, 2 * w * 4, w2xc.make_opts(precision=w2xc.PRECISION_BF16)) == w2xc.ERR_UNSUPPORTED


def test_building_blocks_argument_errors(w2xc):
    lib = w2xc.lib()
    E = w2xc.ERR_ARG
    w, h, n = 40, 24, 2
    ps = w * h * 4

    def spread(d_src, n_, sps, srs, ww, hh, d_up, d_tr, vps):
        return lib.w2xc_tta_spread_device(C.c_void_p(d_src), n_, sps, srs, ww, hh, C.c_void_p(d_up), C.c_void_p(d_tr), vps, None)

    def gather(d_up, d_tr, vps, n_, ww, hh, d_dst, dps, drs):
        return lib.w2xc_tta_gather_device(C.c_void_p(d_up), C.c_void_p(d_tr), vps, n_, ww, hh, C.c_void_p(d_dst), dps, drs, None)
    for ptrs in ((0, B, D), (A, 0, D), (A, B, 0)):
        assert spread(ptrs[0], n, ps, w * 4, w, h, ptrs[1], ptrs[2], ps) == E
        assert gather(ptrs[1], ptrs[2], ps, n, w, h, ptrs[0], ps, w * 4) == E
    assert spread(A, 0, ps, w * 4, w, h, B, D, ps) == E and gather(B, D, ps, 0, w, h, A, ps, w * 4) == E
    assert spread(A, n, ps, w * 4, 0, h, B, D, ps) == E and gather(B, D, ps, n, w, -1, A, ps, w * 4) == E
    assert spread(A, n, ps, w * 4 - 4, w, h, B, D, ps) == E and gather(B, D, ps, n, w, h, A, ps, w * 4 - 4) == E        # rows below 4 w
    assert spread(A, n, ps, w * 4 + 1, w, h, B, D, ps) == E and gather(B, D, ps + 2, n, w, h, A, ps, w * 4) == E        # not multiples of 4
    assert spread(A, n, ps - 4, w * 4, w, h, B, D, ps) == E and gather(B, D, ps, n, w, h, A, ps - 4, w * 4) == E        # planes overlap
    assert spread(A, n, ps, w * 4, w, h, B, D, ps - 4) == E and gather(B, D, ps - 4, n, w, h, A, ps, w * 4) == E        # variant stride below a plane
    assert spread(A, n, ps, w * 4, w, h, B, B + 4 * n * ps - 4, ps) == E                                                # the two groups overlap
    assert gather(B, D, ps, n, w, h, B + 4, ps, w * 4) == E                                                             # the result overlaps a group
    if w2xc.device_count() == 0:
        assert spread(A, n, ps, w * 4, w, h, B, D, ps) == w2xc.ERR_HIP
        assert gather(B, D, ps, n, w, h, A, ps, w * 4) == w2xc.ERR_HIP


def test_device_forms_without_a_device(w2xc, noise1, scale2, rgb3):
    if w2xc.device_count() != 0:
        return     # (with a device the GPU tests run these calls)
    H_ = w2xc.ERR_HIP
    assert single_device(w2xc, False)(noise1, scale2, A, RS, W, H, B, ORS, 1, 1) == H_
    assert single_device(w2xc, True)(rgb3, rgb3, A, RS, W, H, B, ORS, 1, 1) == H_
    assert batch_device(w2xc, False)(noise1, scale2, 2, A, IMS, RS, W, H, B, OMS, ORS, 1, 1) == H_
    assert batch_device(w2xc, True)(rgb3, rgb3, 2, A, IMS, RS, W, H, B, OMS, ORS, 1, 1) == H_
    lib = w2xc.lib()
    ps = W * H * 4
    assert lib.w2xc_convert_batch_tta_device(_h(scale2), 2, 1, C.c_void_p(A), ps, W * 4, W, H, C.c_void_p(B), 4 * ps, 2 * W * 4, None, None) == H_
    assert lib.w2xc_convert_planes_tta_device(_h(rgb3), 3, 1, C.c_void_p(A), ps, W * 4, W, H, C.c_void_p(B), 4 * ps, 2 * W * 4, None, None) == H_


def test_tta_kernels_no_spill_no_scratch(w2xc):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, "w2xc_tta.o")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vspill=int(m.group(4)), sspill=int(m.group(5)), scratch=int(m.group(6)))
    for k in ("k_tta_spread", "k_tta_gather"):
        hit = [name for name in rows if k in name]
        assert len(hit) == 1, (k, sorted(rows))
        assert rows[hit[0]] == dict(vspill=0, sspill=0, scratch=0), (hit[0], rows[hit[0]])


def _cli():
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_parses_tta_and_refuses_it_with_alpha():
    cli = _cli()
    ap = cli.build_parser()
    assert ap.parse_args(["-i", "a.png"]).tta == 0
    assert ap.parse_args(["-i", "a.png", "--tta", "1"]).tta == 1
    assert ap.parse_args(["-i", "a.png", "b.png", "-t", "1", "-m", "scale"]).tta == 1
    with pytest.raises(SystemExit) as ei:
        ap.parse_args(["-i", "a.png", "--tta", "2"])
    assert ei.value.code == 2
    cli.check_tta(0, ["a.png"])
    cli.check_tta(1, [])
    with pytest.raises(SystemExit) as ei:
        cli.check_tta(1, ["a.png", "b.png"])
    assert "a.png" in str(ei.value.code) and "transparency" in str(ei.value.code)
