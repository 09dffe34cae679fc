"""CPU tests of YUV frames through RGB models (revision 0.4.1.8: w2xc_process_frames_yuv_u8_rgb[_device] and the two ends w2xc_yuv8_to_rgb_device,
w2xc_rgb_to_yuv8_device): the symbols and their Python mirrors, the ABI that stays as it was, every refusal of the header's section before a device is touched,
what the existing frame call goes on refusing, the y4m tool's routing, and the NumPy restatement of the arithmetic (tests/yuv_rgb_ref.py) held to float64 and
to its own round trip.  The GPU side: tests/test_gpu_yuv_rgb_blocks.py, tests/test_gpu_yuv_rgb_frames.py."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, small_layers

import yuv_ref as yr
import yuv_rgb_ref as rr
from test_yuv_api import Frames

NEW = ("w2xc_process_frames_yuv_u8_rgb_device", "w2xc_process_frames_yuv_u8_rgb", "w2xc_yuv8_to_rgb_device", "w2xc_rgb_to_yuv8_device")


@pytest.fixture(scope="module")
def y4m():
    spec = importlib.util.spec_from_file_location("w2xc_y4m", os.path.join(ROOT, "tools", "w2xc_y4m.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def head_of(nin, nout, seed):
    return np.random.default_rng(seed).standard_normal((nin, nout, 4, 4)).astype(np.float32) * np.float32(0.05)


@pytest.fixture(scope="module")
def models(w2xc):
    """RGB noise and scale models, a three-plane head model, a Y model, a one-plane head model, a 3 -> 1 model"""
    rgb = lambda seed: w2xc._ModelSet.from_layers(small_layers([3, 32, 3], seed))
    return {"noise": rgb(5), "scale": rgb(6), "head": w2xc._ModelSet.from_layers(small_layers([3, 32, 32], 9), head=(head_of(32, 3, 8), None)),
            "y": w2xc._ModelSet.from_layers(small_layers([1, 32, 1], 7)),
            "head1": w2xc._ModelSet.from_layers(small_layers([1, 32, 32], 10), head=(head_of(32, 1, 11), None)),
            "3to1": w2xc._ModelSet.from_layers(small_layers([3, 32, 1], 12))}


def test_symbols_and_wrappers_exist(w2xc):
    lib = C.CDLL(w2xc.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in w2xc.ABI_SYMBOLS
    for name in ("process_frames_yuv_u8_rgb", "process_frames_yuv_u8_rgb_device", "yuv8_to_rgb_device", "rgb_to_yuv8_device"):
        assert hasattr(w2xc, name), name
    assert (w2xc.MATRIX_BT601, w2xc.MATRIX_BT709, w2xc.MATRIX_BT2020) == rr.MATRICES
    hdr = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    for name, val in (("W2XC_MATRIX_BT601", 0), ("W2XC_MATRIX_BT709", 1), ("W2XC_MATRIX_BT2020", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    sec = hdr[hdr.index("YUV frames through RGB models"):]
    # the constants as expressions of the two luma weights, not as decimals; the exactness of the chroma step; what is left out
    for text in ("Kg = 1.0 - Kr - Kb", "cRV = 2.0 * (1.0 - Kr)", "cBU = 2.0 * (1.0 - Kb)", "cGV = Kr * cRV / Kg", "cGU = Kb * cBU / Kg", "iRV = 1.0 / cRV", "iBU = 1.0 / cBU",
                 "exact in", "Left out: left-sited chroma"):
        assert text in sec, text
    for Kr, Kb in rr.WEIGHTS.values():
        assert "Kr = %s" % Kr in sec and "Kb = %s" % Kb in sec
    assert not re.search(r"1\.5748|1\.8556|1\.402\b|1\.772\b", sec), "no decimals of derived constants"


def test_the_abi_stays(w2xc):
    assert C.sizeof(w2xc.Opts) == 56 and w2xc.make_opts().struct_size == 56
    assert w2xc.lib().w2xc_version() == b"w2xc_hip 0.4.1.6.1 (gfx950)"
    assert C.sizeof(w2xc.YuvPlanes) == 64


def test_wrapper_keywords(w2xc):
    host = inspect.signature(w2xc.process_frames_yuv_u8_rgb).parameters
    assert list(host)[:4] == ["y", "u", "v", "uv"]
    for k in ("chroma", "noise", "scale", "iterations", "range", "matrix", "opts", "out_nv12"):
        assert k in host, k
    assert host["matrix"].default == w2xc.MATRIX_BT709 and host["range"].default == w2xc.RANGE_LIMITED and host["chroma"].default == w2xc.YUV_420
    dev = inspect.signature(w2xc.process_frames_yuv_u8_rgb_device).parameters
    assert list(dev)[:6] == ["n", "w", "h", "chroma", "d_in", "d_out"]
    for k in ("noise", "scale", "iterations", "range", "matrix", "stream", "opts"):
        assert k in dev, k
    assert list(inspect.signature(w2xc.yuv8_to_rgb_device).parameters) == ["d_src", "n", "w", "h", "chroma", "range", "matrix", "d_rgb", "image_stride_bytes",
                                                                            "plane_stride_bytes", "stream"]
    assert list(inspect.signature(w2xc.rgb_to_yuv8_device).parameters) == ["d_rgb", "image_stride_bytes", "plane_stride_bytes", "n", "w", "h", "chroma", "range",
                                                                            "matrix", "d_dst", "stream"]
    # the Y call's wrapper is what it was
    assert "matrix" not in inspect.signature(w2xc.process_frames_yuv_u8).parameters


# ---- refusals: all of them before a device is touched (this machine may have none: a call that passes them answers ERR_HIP) ----
def call(w2xc, noise, scale, n, w, h, layout, rng, matrix, i, o, iterations, device=False, opts=None):
    h_ = lambda m: m.handle if m is not None else None
    pi = C.byref(i) if i is not None else None
    po = C.byref(o) if o is not None else None
    op = C.byref(opts) if opts is not None else None
    if device:
        return w2xc.lib().w2xc_process_frames_yuv_u8_rgb_device(h_(noise), h_(scale), n, w, h, layout, rng, matrix, pi, po, iterations, None, op)
    return w2xc.lib().w2xc_process_frames_yuv_u8_rgb(h_(noise), h_(scale), n, w, h, layout, rng, matrix, pi, po, iterations, op)


def broken(w2xc, side, **kw):
    t = w2xc.YuvPlanes()
    C.memmove(C.byref(t), C.byref(side), C.sizeof(t))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(w2xc, models, device):
    if device and w2xc.device_count() > 0:
        pytest.skip("these planes are host memory: the device form is given them only where no device can be reached")
    N, S, H = models["noise"], models["scale"], models["head"]
    n, w, h, lay, M = 2, 17, 9, yr.YUV_420, rr.BT709
    i, o, o0 = Frames(w2xc, n, w, h, lay), Frames(w2xc, n, 2 * w, 2 * h, lay), Frames(w2xc, n, w, h, lay)
    run = lambda *a, **k: call(w2xc, *a, device=device, **k)
    good = (w2xc.ERR_HIP,) if w2xc.device_count() <= 0 else (w2xc.OK,)   # what a call that passes every check answers
    A, P, U = w2xc.ERR_ARG, w2xc.ERR_PLANES, w2xc.ERR_UNSUPPORTED
    assert run(N, S, n, w, h, lay, yr.LIMITED, M, i.s, o.s, 1) in good, w2xc.last_error()
    assert run(N, None, n, w, h, lay, yr.FULL, rr.BT601, i.s, o0.s, 0) in good, w2xc.last_error()
    assert run(N, H, n, w, h, lay, yr.FULL, rr.BT2020, i.s, o.s, 1) in good, w2xc.last_error()
    assert run(None, H, n, w, h, lay, yr.FULL, M, i.s, o.s, 1) in good, w2xc.last_error()
    # the models: three planes to three planes; a head model is a scale model only
    for bad in ("y", "3to1", "head1"):
        assert run(models[bad], S, n, w, h, lay, 0, M, i.s, o.s, 1) in (P, U), bad
        assert run(N, models[bad], n, w, h, lay, 0, M, i.s, o.s, 1) == P, bad
    assert run(models["y"], None, n, w, h, lay, 0, M, i.s, o0.s, 0) == P
    assert run(H, S, n, w, h, lay, 0, M, i.s, o.s, 1) == U and "upconv head" in w2xc.last_error()
    assert run(H, None, n, w, h, lay, 0, M, i.s, o0.s, 0) == U
    # the options the plane batch calls refuse
    assert run(N, S, n, w, h, lay, 0, M, i.s, o.s, 1, opts=w2xc.make_opts(precision=77)) == U
    for prec in (w2xc.PRECISION_BF16, w2xc.PRECISION_BF16X2, w2xc.PRECISION_BF16X3, w2xc.PRECISION_FP16X2):
        assert run(None, H, n, w, h, lay, 0, M, i.s, o.s, 1, opts=w2xc.make_opts(precision=prec)) == U, prec
        assert run(N, S, n, w, h, lay, 0, M, i.s, o.s, 1, opts=w2xc.make_opts(precision=prec)) in good, w2xc.last_error()
    # the passes
    assert run(None, None, n, w, h, lay, 0, M, i.s, o.s, 1) == A
    assert run(N, None, n, w, h, lay, 0, M, i.s, o.s, 1) == A          # iterations = 1 without a scale model
    assert run(None, S, n, w, h, lay, 0, M, i.s, o0.s, 0) == A         # nothing to do
    for it in (-1, 2, 5):
        assert run(N, S, n, w, h, lay, 0, M, i.s, o.s, it) == A
    # counts, sizes, enumerations, null sides
    assert run(N, S, 0, w, h, lay, 0, M, i.s, o.s, 1) == A and run(N, S, -3, w, h, lay, 0, M, i.s, o.s, 1) == A
    assert run(N, S, n, 0, h, lay, 0, M, i.s, o.s, 1) == A and run(N, S, n, w, -1, lay, 0, M, i.s, o.s, 1) == A
    assert run(N, S, n, w, h, 4, 0, M, i.s, o.s, 1) == A and run(N, S, n, w, h, -1, 0, M, i.s, o.s, 1) == A
    assert run(N, S, n, w, h, yr.YUV_400, 0, M, i.s, o.s, 1) == A and "W2XC_YUV_400" in w2xc.last_error()
    assert run(N, S, n, w, h, lay, 2, M, i.s, o.s, 1) == A and run(N, S, n, w, h, lay, -1, M, i.s, o.s, 1) == A
    for m in (-1, 3, 709):
        assert run(N, S, n, w, h, lay, 0, m, i.s, o.s, 1) == A and "matrix" in w2xc.last_error()
    assert run(N, S, n, w, h, lay, 0, M, None, o.s, 1) == A and run(N, S, n, w, h, lay, 0, M, i.s, None, 1) == A
    br = lambda side, **kw: broken(w2xc, side, **kw)
    cw, ch = yr.chroma_size(w, h, lay)
    for field in ("y", "u", "v"):
        assert run(N, S, n, w, h, lay, 0, M, br(i.s, **{field: None}), o.s, 1) == A
        assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, **{field: None}), 1) == A
    assert run(N, S, n, w, h, lay, 0, M, br(i.s, y_stride=w - 1), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, y_stride=2 * w - 1), 1) == A
    assert run(N, S, n, w, h, lay, 0, M, br(i.s, c_stride=cw - 1), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, c_stride=w - 1), 1) == A
    assert run(N, S, n, w, h, lay, 0, M, br(i.s, y_frame_stride=w * h - 1), o.s, 1) == A
    assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, c_frame_stride=w * h - 1), 1) == A
    for px in (0, 3, -1):
        assert run(N, S, n, w, h, lay, 0, M, br(i.s, c_px=px), o.s, 1) == A
        assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, c_px=px), 1) == A
    assert run(N, S, n, w, h, lay, 0, M, br(i.s, c_px=2), o.s, 1) == A   # the planar stride is too short for interleaved rows
    assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, y=i.s.y), 1) == A
    assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, v=o.s.u), 1) == A
    assert run(N, S, n, w, h, lay, 0, M, i.s, br(o.s, u=o.s.y), 1) == A
    if not device:   # host planes with c_px = 2 are NV12 / NV21
        i2 = Frames(w2xc, n, w, h, lay, px=2)
        assert run(N, S, n, w, h, lay, 0, M, i2.s, o.s, 1) in good and run(N, S, n, w, h, lay, 0, M, br(i2.s, u=i2.s.v, v=i2.s.u), o.s, 1) in good
        assert run(N, S, n, w, h, lay, 0, M, br(i2.s, v=i2.s.u + 3), o.s, 1) == A and "NV12" in w2xc.last_error()


def test_the_y_frame_call_still_refuses_these_models(w2xc, models):
    import test_yuv_api as ty
    n, w, h, lay = 2, 17, 9, yr.YUV_420
    i, o = Frames(w2xc, n, w, h, lay), Frames(w2xc, n, 2 * w, 2 * h, lay)
    for device in (False, True):
        if device and w2xc.device_count() > 0:
            continue
        assert ty.call(w2xc, None, models["scale"], n, w, h, lay, 0, i.s, o.s, 1, device=device) == w2xc.ERR_PLANES
        assert ty.call(w2xc, models["noise"], models["scale"], n, w, h, lay, 0, i.s, o.s, 1, device=device) == w2xc.ERR_PLANES
        assert ty.call(w2xc, None, models["head"], n, w, h, lay, 0, i.s, o.s, 1, device=device) in (w2xc.ERR_UNSUPPORTED, w2xc.ERR_PLANES)
        assert ty.call(w2xc, None, models["head1"], n, w, h, lay, 0, i.s, o.s, 1, device=device) == w2xc.ERR_UNSUPPORTED


def test_block_refusals(w2xc):
    lib = w2xc.lib()
    A = w2xc.ERR_ARG
    n, w, h, lay = 2, 8, 4, yr.YUV_420
    fr = Frames(w2xc, n, w, h, lay)
    f = np.zeros(3 * n * w * h + 64, np.float32)
    pf, ps, is_ = f.ctypes.data, 4 * w * h, 12 * w * h
    to = lambda s, n_, w_, h_, lay_, rng, m, p, is__, ps_: lib.w2xc_yuv8_to_rgb_device(C.byref(s) if s is not None else None, n_, w_, h_, lay_, rng, m, p, is__, ps_, None)
    back = lambda s, n_, w_, h_, lay_, rng, m, p, is__, ps_: lib.w2xc_rgb_to_yuv8_device(p, is__, ps_, n_, w_, h_, lay_, rng, m, C.byref(s) if s is not None else None, None)
    good = (w2xc.ERR_HIP, w2xc.OK)
    for fn in (to, back):
        assert fn(None, n, w, h, lay, 0, 0, pf, is_, ps) == A and fn(fr.s, n, w, h, lay, 0, 0, None, is_, ps) == A
        assert fn(fr.s, 0, w, h, lay, 0, 0, pf, is_, ps) == A and fn(fr.s, n, 0, h, lay, 0, 0, pf, is_, ps) == A and fn(fr.s, n, w, -2, lay, 0, 0, pf, is_, ps) == A
        assert fn(fr.s, n, w, h, yr.YUV_400, 0, 0, pf, is_, ps) == A and fn(fr.s, n, w, h, 4, 0, 0, pf, is_, ps) == A and fn(fr.s, n, w, h, -1, 0, 0, pf, is_, ps) == A
        assert fn(fr.s, n, w, h, lay, 2, 0, pf, is_, ps) == A and fn(fr.s, n, w, h, lay, -1, 0, pf, is_, ps) == A
        assert fn(fr.s, n, w, h, lay, 0, 3, pf, is_, ps) == A and fn(fr.s, n, w, h, lay, 0, -1, pf, is_, ps) == A
        assert fn(fr.s, n, w, h, lay, 0, 0, pf, is_, ps - 4) == A and fn(fr.s, n, w, h, lay, 0, 0, pf, is_ - 4, ps) == A     # planes / images that overlap
        assert fn(fr.s, n, w, h, lay, 0, 0, pf, is_, ps + 2) == A and fn(fr.s, n, w, h, lay, 0, 0, pf, is_ + 2, ps) == A     # no multiples of 4
        assert fn(broken(w2xc, fr.s, y=None), n, w, h, lay, 0, 0, pf, is_, ps) == A and fn(broken(w2xc, fr.s, v=None), n, w, h, lay, 0, 0, pf, is_, ps) == A
        assert fn(broken(w2xc, fr.s, y_stride=w - 1), n, w, h, lay, 0, 0, pf, is_, ps) == A and fn(broken(w2xc, fr.s, c_px=3), n, w, h, lay, 0, 0, pf, is_, ps) == A
        assert fn(broken(w2xc, fr.s, c_frame_stride=3), n, w, h, lay, 0, 0, pf, is_, ps) == A
        assert fn(broken(w2xc, fr.s, y=pf + 16), n, w, h, lay, 0, 0, pf, is_, ps) == A, "the two sides overlap"
    assert back(broken(w2xc, fr.s, v=fr.s.u), n, w, h, lay, 0, 0, pf, is_, ps) == A, "written planes on each other"
    if w2xc.device_count() <= 0:
        assert to(fr.s, n, w, h, lay, 1, 2, pf, is_, ps) in good and to(broken(w2xc, fr.s, v=fr.s.u), n, w, h, lay, 0, 0, pf, is_, ps) in good


# ---- the y4m tool ----
def test_y4m_tool_routes_by_the_models(y4m, tmp_path, capsys):
    assert y4m.model_route(1, 1) == "y" and y4m.model_route(None, 1) == "y" and y4m.model_route(3, None) == "rgb" and y4m.model_route(3, 3) == "rgb"
    for bad in ((1, 3), (3, 1), (2, None), (None, 4)):
        with pytest.raises(y4m.Y4mError):
            y4m.model_route(*bad)
    assert y4m.default_matrix(719) == "bt601" and y4m.default_matrix(720) == "bt709" and y4m.default_matrix(1080) == "bt709" and y4m.default_matrix(1) == "bt601"
    assert y4m.MATRICES == {"bt601": rr.BT601, "bt709": rr.BT709, "bt2020": rr.BT2020}
    ap = y4m.build_parser()
    assert ap.parse_args(["a", "b"]).matrix is None and ap.parse_args(["a", "b", "--matrix", "bt2020"]).matrix == "bt2020"
    with pytest.raises(SystemExit):
        ap.parse_args(["a", "b", "--matrix", "smpte240m"])
    assert "bt709 when H >= 720, else bt601" in " ".join(ap.format_help().split())
    y4m.check_route("y", y4m.LAYOUTS["mono"])
    y4m.check_route("rgb", y4m.LAYOUTS["420"])
    with pytest.raises(y4m.Y4mError):
        y4m.check_route("rgb", y4m.LAYOUTS["mono"])


def test_y4m_tool_refuses_mono_with_rgb_models(y4m, w2xc, tmp_path, capsys):
    from tools import gen_model
    gen_model.write_json(small_layers([3, 32, 3], 21), str(tmp_path / "scale2.0x_model.json"))
    data, _ = yr.y4m_stream(16, 8, "mono", 1, seed=14)
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(data)
    assert y4m.main([str(src), str(dst), "-m", "scale", "--model_dir", str(tmp_path)]) == 2
    assert "Cmono" in capsys.readouterr().err and not dst.exists()


# ---- the restatement ----
@pytest.mark.parametrize("matrix", rr.MATRICES)
def test_constants(matrix):
    k = rr.constants64(matrix)
    assert abs(k["Kr"] + k["Kg"] + k["Kb"] - 1.0) < 1e-15
    # the textbook values the expressions give
    want = {rr.BT601: (1.402, 1.772, 0.714136, 0.344136), rr.BT709: (1.5748, 1.8556, 0.468124, 0.187324), rr.BT2020: (1.4746, 1.8814, 0.571353, 0.164553)}[matrix]
    got = (k["cRV"], k["cBU"], k["cGV"], k["cGU"])
    assert np.allclose(got, want, rtol=0, atol=1e-6)
    assert all(v.dtype == np.float32 for v in rr.constants(matrix).values())


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED])
@pytest.mark.parametrize("matrix", rr.MATRICES)
def test_neutral_chroma_stays_neutral(matrix, rng):
    Y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for lay in rr.LAYOUTS:
        cw, ch = yr.chroma_size(16, 16, lay)
        grey = np.full((ch, cw), 128, np.uint8)
        rgb = rr.yuv8_to_rgb(Y, grey, grey, lay, rng, matrix)
        y = np.clip(yr.luma_in(Y, rng), np.float32(0), np.float32(1))
        for p in rgb:   # R = G = B = y, bit for bit
            assert np.array_equal(p.view(np.uint32), y.view(np.uint32))
        # R = G = B gives U = V = 128, whatever the grey (beyond [0, 1] too)
        v = np.linspace(-0.5, 1.5, 16 * 16, dtype=np.float32).reshape(16, 16)
        Yb, U, V = rr.rgb_to_yuv8(np.stack([v, v, v]), lay, rng, matrix)
        assert (U == 128).all() and (V == 128).all() and U.shape == (ch, cw)
        assert np.abs(Yb.astype(int) - yr.luma_out(v, rng).astype(int)).max() <= 1   # (y' is v up to a few roundings)


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED])
@pytest.mark.parametrize("matrix", rr.MATRICES)
def test_in_gamut_triples_return_through_both_ends(matrix, rng):
    """4:4:4: every (Y, U, V) of a fixed random sample has its RGB checked in float64; the triples whose RGB lies inside [0, 1] come back as the same bytes
    (the fp32 error times 255 is about 3e-4, far from a rounding tie at integer inputs)."""
    g = np.random.default_rng(1234)
    n = 64 * 64
    Y = g.integers(32, 225, n, dtype=np.uint8).reshape(64, 64)
    U = g.integers(112, 145, n, dtype=np.uint8).reshape(64, 64)
    V = g.integers(112, 145, n, dtype=np.uint8).reshape(64, 64)
    k = rr.constants64(matrix)
    y = (Y.astype(np.float64) - 16.0) / 219.0 if rng == yr.LIMITED else Y.astype(np.float64) / 255.0
    kc = 224.0 if rng == yr.LIMITED else 255.0
    cb, cr = (U.astype(np.float64) - 128.0) / kc, (V.astype(np.float64) - 128.0) / kc
    want = np.stack([y + k["cRV"] * cr, y - k["cGU"] * cb - k["cGV"] * cr, y + k["cBU"] * cb])
    rgb = rr.yuv8_to_rgb(Y, U, V, yr.YUV_444, rng, matrix)
    assert np.abs(rgb - np.clip(want, 0.0, 1.0)).max() < 4e-7, "a few fp32 roundings of values of at most 1"
    inside = ((want >= 0.0) & (want <= 1.0)).all(axis=0)
    assert inside.mean() >= 0.2, "the in-gamut share of the sample: %g" % inside.mean()
    Y2, U2, V2 = rr.rgb_to_yuv8(rgb, yr.YUV_444, rng, matrix)
    assert np.array_equal(Y2[inside], Y[inside]) and np.array_equal(U2[inside], U[inside]) and np.array_equal(V2[inside], V[inside])


def test_chroma_at_luma_is_exact_and_sited():
    C8 = np.array([[0, 255, 16], [240, 1, 128]], np.uint8)
    up = rr.chroma_at_luma(C8, 5, 3, yr.YUV_420)
    # row 0 of the horizontal step, by hand: x = 0 reads j = 0 and j' = -1 clamped to 0; x = 1: 0.75 * 0 + 0.25 * 255; x = 2: 0.75 * 255 + 0.25 * 0;
    # x = 3: 0.75 * 255 + 0.25 * 16; x = 4: 0.75 * 16 + 0.25 * 255
    want = np.array([[0, 63.75, 191.25, 195.25, 75.75]], np.float64)
    h0 = rr.chroma_at_luma(C8[:1], 5, 1, yr.YUV_422)
    assert np.array_equal(h0.astype(np.float64), want)
    # every value is a multiple of 1 / 16: exact in fp32, so the order of the two steps is a convention
    assert np.array_equal(up * 16, np.rint(up * 16))
    other = rr._up_axis(rr._up_axis(C8.astype(np.float32), 0, 3), 1, 5)
    assert np.array_equal(up, other)
    assert np.array_equal(rr.chroma_at_luma(C8, 3, 2, yr.YUV_444), C8.astype(np.float32))
    const = rr.chroma_at_luma(np.full((4, 4), 77, np.uint8), 7, 8, yr.YUV_420)
    assert (const == 77).all()


def test_block_mean_replicates_at_odd_edges():
    c = np.arange(15, dtype=np.float32).reshape(3, 5)
    m = rr._block_mean(c, yr.YUV_420)
    assert m.shape == (2, 3)
    assert m[0, 0] == (0 + 1 + 5 + 6) / 4 and m[0, 2] == (4 + 4 + 9 + 9) / 4 and m[1, 0] == (10 + 11 + 10 + 11) / 4 and m[1, 2] == 14
    m = rr._block_mean(c, yr.YUV_422)
    assert m.shape == (3, 3) and m[1, 0] == 5.5 and m[1, 2] == 9
    assert rr._block_mean(c, yr.YUV_444) is c


def test_launch_rule_matches_the_launchers():
    src = open(os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc", "w2xc_kernels.h")).read()
    for name, val in (("W2XC_YUVRGB_TCX", rr.TCX), ("W2XC_YUVRGB_TCY", rr.TCY), ("W2XC_YUVRGB_GRID_MAX", rr.GRID_MAX)):
        assert "#define %s %d" % (name, val) in src
    # the rule is written once, in w2xc_host_geom.hpp (yuv_rgb_tile_grid on yuv_tile_grid; tests/cpp/host_geom_test.cpp runs it against the expressions the
    # launchers had), and both launchers call it with the tile, the cap and a turn per tile and frame
    squeeze = lambda name: " ".join(open(os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc", name)).read().split())
    geom, hip = squeeze("w2xc_host_geom.hpp"), squeeze("w2xc_yuv_rgb.hip")
    assert geom.count("yuv_tile_grid((cw + tcx - 1) / tcx, (ch + tcy - 1) / tcy, n, cap)") == 1
    assert geom.count("turns = tiles * per_tile") == 1 and geom.count("(unsigned)(turns > cap ? cap : turns)") == 1
    assert hip.count("yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX)") == 2 and "/ YR_TCX" not in hip
    assert rr.launch(1, 1, yr.YUV_420, 1) == (1, 1) and rr.launch(64, 32, yr.YUV_420, 1) == (1, 1) and rr.launch(65, 33, yr.YUV_420, 1) == (4, 4)
    assert rr.launch(64, 32, yr.YUV_444, 3) == (12, 12) and rr.launch(64, 32, yr.YUV_422, 1) == (2, 2)
    assert rr.launch(1920, 1080, yr.YUV_420, 8) == (30 * 34 * 8, 2048)
    turns, grid = rr.launch(**rr.SECOND_TRIP)
    assert turns > grid == rr.GRID_MAX, "the GPU tests' second-trip shape has more tiles than workgroups"
    assert 3 * rr.SECOND_TRIP["w"] * rr.SECOND_TRIP["h"] * 4 < 64 << 20
