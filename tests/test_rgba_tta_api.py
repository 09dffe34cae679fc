"""TTA for the RGBA image calls (revision 0.4.1.6.3: w2xc_process_image_rgba_u8_batch_tta[_device], w2xc_process_image_rgba_u8_up2x_batch_tta[_device],
w2xc_tta_spread_u8_device, w2xc_tta_gather_u8_device), everything that needs no GPU: the symbols in the header, the library and the binding, the Python
keywords, every refusal of both families and of the two building blocks (before a device is touched: this runs on a machine without one), the CLI's
--tta_alpha routing, and the registers of the new kernels.  The GPU side is tests/test_gpu_rgba_tta.py and tests/test_gpu_tta_u8_blocks.py."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tools import gen_model
import upconv_ref as ur

ERR_ARG, ERR_PLANES, ERR_UNSUPPORTED = -3, -4, -6
C_SYMBOLS = ("w2xc_process_image_rgba_u8_batch_tta_device", "w2xc_process_image_rgba_u8_batch_tta", "w2xc_process_image_rgba_u8_up2x_batch_tta_device",
             "w2xc_process_image_rgba_u8_up2x_batch_tta", "w2xc_tta_spread_u8_device", "w2xc_tta_gather_u8_device")
LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")


@pytest.fixture(scope="module")
def sets(w2xc):
    layers, head = ur.head_model([3, 32], 3, 401)
    y1, yhead = ur.head_model([1, 32, 64], 1, 402)
    return {"head": w2xc._ModelSet.from_layers(layers, head=head), "head_y": w2xc._ModelSet.from_layers(y1, head=yhead),
            "rgb": w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 32, 3], 9)),
            "y": w2xc._ModelSet.from_layers(gen_model.synth_layers([1, 32, 1], 10)),
            "two": w2xc._ModelSet.from_layers(gen_model.synth_layers([2, 32, 2], 11))}


# ---- the symbols, the documents, the keywords ----
def test_symbols_are_declared_exported_bound_and_documented(w2xc):
    header = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in C_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert getattr(w2xc.lib(), sym) is not None
        assert sym in w2xc.ABI_SYMBOLS and sym in integration, sym
    assert "0.4.1.6.3" in header and "0.4.1.6.3" in integration
    assert "There is no TTA form of the RGBA call" not in header and "Not built: TTA" not in header
    # the revision is found by the symbols: the struct and the version string stay
    assert C.sizeof(w2xc.Opts) == 56
    assert w2xc.lib().w2xc_version().decode() == "w2xc_hip 0.4.1.6.1 (gfx950)"


def test_python_keywords(w2xc):
    for name in ("process_image_rgba_u8", "process_image_rgba_u8_device", "process_image_rgba_u8_batch", "process_image_rgba_u8_batch_device",
                 "process_image_rgba_u8_up2x_batch", "process_image_rgba_u8_up2x_batch_device"):
        params = inspect.signature(getattr(w2xc, name)).parameters
        assert list(params)[-1] == "tta" and params["tta"].default is False, name
    assert list(inspect.signature(w2xc.tta_spread_u8_device).parameters) == [
        "d_src", "n", "image_stride_bytes", "stride_bytes", "px_bytes", "ch0", "ch_step", "w", "h", "d_up", "d_tr", "variant_plane_stride_bytes", "stream"]
    assert list(inspect.signature(w2xc.tta_gather_u8_device).parameters) == [
        "d_up", "d_tr", "variant_plane_stride_bytes", "n", "planes_per_image", "first_plane", "n_ch", "w", "h", "d_dst", "image_stride_bytes", "stride_bytes",
        "px_bytes", "byte0", "stream"]
    # tta=False is the entry without the argument, tta=True the new one
    assert w2xc._tta_entry("w2xc_process_image_rgba_u8_batch", False)[0] is w2xc.lib().w2xc_process_image_rgba_u8_batch
    for name in ("w2xc_process_image_rgba_u8_batch", "w2xc_process_image_rgba_u8_batch_device", "w2xc_process_image_rgba_u8_up2x_batch",
                 "w2xc_process_image_rgba_u8_up2x_batch_device"):
        entry, tail = w2xc._tta_entry(name, True)
        assert entry.__name__ == name.replace("_device", "") + "_tta" + ("_device" if name.endswith("_device") else "") and tail == (1,)


# ---- the refusals of the image calls: both families, device and host form ----
A, B = 0x10000000, 0x90000000
W, H = 64, 48


def device_call(w2xc, up2x, mn, ms, n=2, d_in=A, iis=W * 4 * H, irs=W * 4, ww=W, hh=H, d_out=B, ois=2 * W * 4 * 2 * H, ors=2 * W * 4, it=1, shrink=0.0,
                passes=-1, opts=None, tta=1):
    f = w2xc.lib().w2xc_process_image_rgba_u8_up2x_batch_tta_device if up2x else w2xc.lib().w2xc_process_image_rgba_u8_batch_tta_device
    return f(mn.handle if mn else None, ms.handle if ms else None, n, C.c_void_p(d_in), iis, irs, ww, hh, C.c_void_p(d_out), ois, ors, it, shrink, passes, None,
             C.byref(opts) if opts is not None else None, tta)


@pytest.mark.parametrize("family", ["rgb", "y", "head"])
def test_device_form_refusals(w2xc, sets, family):
    """fake device addresses: every one of these must be refused by the argument checks, never dereferenced"""
    up2x = family == "head"
    ms = sets[family]
    mn = sets["y"] if family == "y" else sets["rgb"]
    ims, rs = W * 4 * H, W * 4

    def call(**kw):
        kw.setdefault("ms", ms)
        kw.setdefault("mn", None)
        return device_call(w2xc, up2x, **kw)
    cases = {
        "tta = -1": (call(tta=-1), ERR_ARG),
        "tta = 2": (call(tta=2), ERR_ARG),
        "n = 0": (call(n=0), ERR_ARG),
        "n < 0": (call(n=-1), ERR_ARG),
        "null input": (call(d_in=0), ERR_ARG),
        "null output": (call(d_out=0), ERR_ARG),
        "input rows below 4 w": (call(irs=rs - 1), ERR_ARG),
        "input rows of a 3-channel image": (call(irs=3 * W), ERR_ARG),
        "output rows below 4 W": (call(ors=2 * rs - 1), ERR_ARG),
        "output images overlap each other": (call(n=3, ois=4 * ims - 2 * rs), ERR_ARG),
        "outputs overlap the inputs": (call(n=3, d_out=A + ims), ERR_ARG),
        "in place, n = 1": (call(mn=mn, n=1, d_out=A, it=0, ois=0, ors=rs), ERR_ARG),
        "iterations = 5": (call(it=5, ois=1 << 28, ors=1 << 14), ERR_ARG),
        "shrink_ratio = 1": (call(shrink=1.0), ERR_ARG),
        "more than 65534 effective bleed passes": (call(mn=mn, iis=1 << 21, irs=70000 * 4, ww=70000, hh=2, ois=1 << 21, ors=70000 * 4, it=0, passes=1 << 30),
                                                   ERR_ARG),
        "an extent above 2^28": (call(iis=1 << 40, irs=1 << 30, ww=(1 << 27) + 1, hh=2, ois=1 << 41, ors=1 << 31), ERR_ARG),
        "a model of two planes": (call(mn=sets["two"]) if up2x else call(ms=sets["two"]), ERR_PLANES),
    }
    if up2x:
        cases.update({
            "a scale model without a head": (call(ms=sets["rgb"]), ERR_ARG),
            "no scale model": (call(mn=mn, ms=None, it=0, ois=ims, ors=rs), ERR_ARG),
            "a head model as noise model": (call(mn=ms), ERR_UNSUPPORTED),
            "a 16-bit precision with a head model": (call(opts=w2xc.make_opts(precision=w2xc.PRECISION_BF16X2)), ERR_UNSUPPORTED),
            "a one-plane head model": (call(ms=sets["head_y"]), ERR_PLANES),
            "a Y noise model": (call(mn=sets["y"]), ERR_PLANES),
        })
    else:
        cases.update({
            "a head model": (call(ms=sets["head"]), ERR_UNSUPPORTED),
            "a head model as noise model": (call(mn=sets["head"]), ERR_UNSUPPORTED),
            "no model": (call(ms=None), ERR_ARG),
            "iterations without a scale model": (call(mn=mn, ms=None), ERR_ARG),
            "a Y model beside an RGB one": (call(mn=sets["y"] if family == "rgb" else sets["rgb"]), ERR_PLANES),
        })
    for what, (rc, want) in cases.items():
        assert rc == want, (family, what, rc, want, w2xc.last_error())
    # tta = 0 and the sibling without the argument: the same refusals
    f0 = w2xc.lib().w2xc_process_image_rgba_u8_up2x_batch_device if up2x else w2xc.lib().w2xc_process_image_rgba_u8_batch_device
    for kw in (dict(n=0), dict(irs=rs - 1), dict(d_out=0), dict(shrink=1.0)):
        a = dict(n=2, d_in=A, iis=ims, irs=rs, d_out=B, ois=4 * ims, ors=2 * rs, it=1, shrink=0.0)
        a.update(kw)
        rc0 = f0(None, ms.handle, a["n"], C.c_void_p(a["d_in"]), a["iis"], a["irs"], W, H, C.c_void_p(a["d_out"]), a["ois"], a["ors"], a["it"], a["shrink"], -1,
                 None, None)
        assert rc0 == call(tta=0, **kw) == call(tta=1, **kw) == ERR_ARG, kw
    if w2xc.device_count() == 0:   # valid arguments: no CPU fallback, and only now a device is asked for
        for tta in (0, 1):
            assert call(tta=tta) == w2xc.ERR_HIP
            assert call(mn=mn, n=1, iis=0, ois=0, passes=3, tta=tta) == w2xc.ERR_HIP
            assert call(n=3, iis=ims + 13, irs=rs + 1, ois=4 * ims + 7, ors=2 * rs + 3, shrink=0.75, passes=0, tta=tta) == w2xc.ERR_HIP


@pytest.mark.parametrize("family", ["rgb", "y", "head"])
def test_host_form_refusals(w2xc, sets, family):
    up2x = family == "head"
    f = w2xc.lib().w2xc_process_image_rgba_u8_up2x_batch_tta if up2x else w2xc.lib().w2xc_process_image_rgba_u8_batch_tta
    w, h, n = 40, 24, 3
    ins = [np.zeros((h, w, 4), np.uint8) for _ in range(n)]
    outs = np.zeros((n, 2 * h, 2 * w, 4), np.uint8)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)
    ip = arr([a.ctypes.data for a in ins])
    op = arr([outs[i].ctypes.data for i in range(n)])
    rs, ors = w * 4, 2 * w * 4

    def call(mn=None, ms=sets[family], n_=n, ip_=ip, irs=rs, op_=op, ors_=ors, it=1, shrink=0.0, passes=-1, opts=None, tta=1):
        return f(mn.handle if mn else None, ms.handle if ms else None, n_, ip_, irs, w, h, op_, ors_, it, shrink, passes,
                 C.byref(opts) if opts is not None else None, tta)
    cases = {
        "tta = -1": (call(tta=-1), ERR_ARG),
        "tta = 2": (call(tta=2), ERR_ARG),
        "n = 0": (call(n_=0), ERR_ARG),
        "null input array": (call(ip_=None), ERR_ARG),
        "null output array": (call(op_=None), ERR_ARG),
        "a null in[i]": (call(ip_=arr([ins[0].ctypes.data, None, ins[2].ctypes.data])), ERR_ARG),
        "a null out[i]": (call(op_=arr([outs[0].ctypes.data, outs[1].ctypes.data, None])), ERR_ARG),
        "input rows below 4 w": (call(irs=rs - 1), ERR_ARG),
        "output rows below 4 W": (call(ors_=ors - 4), ERR_ARG),
        "outputs overlap each other": (call(op_=arr([outs[0].ctypes.data, outs[1].ctypes.data, outs[0].ctypes.data + 64])), ERR_ARG),
        "an output is an input": (call(op_=arr([outs[0].ctypes.data, ins[1].ctypes.data, outs[2].ctypes.data])), ERR_ARG),
        "a head model where it does not belong": (call(mn=sets["head"]), ERR_UNSUPPORTED),
    }
    if up2x:
        cases["a scale model without a head"] = (call(ms=sets["rgb"]), ERR_ARG)
        cases["a 16-bit precision with a head model"] = (call(opts=w2xc.make_opts(precision=w2xc.PRECISION_BF16X2)), ERR_UNSUPPORTED)
        cases["a one-plane head model"] = (call(ms=sets["head_y"]), ERR_PLANES)
    else:
        cases["a head model as scale model"] = (call(ms=sets["head"]), ERR_UNSUPPORTED)
    for what, (rc, want) in cases.items():
        assert rc == want, (family, what, rc, want, w2xc.last_error())
    if w2xc.device_count() == 0:
        for tta in (0, 1):
            assert call(tta=tta) == w2xc.ERR_HIP
            assert call(n_=1, tta=tta) == w2xc.ERR_HIP


def test_existing_rgba_calls_keep_their_arguments(w2xc, sets):
    """no tta argument on the calls that existed, and a head model stays refused there"""
    L = w2xc.lib()
    w, h = 16, 8
    assert len(L.w2xc_process_image_rgba_u8_batch_device.argtypes) + 1 == len(L.w2xc_process_image_rgba_u8_batch_tta_device.argtypes)
    assert len(L.w2xc_process_image_rgba_u8_up2x_batch.argtypes) + 1 == len(L.w2xc_process_image_rgba_u8_up2x_batch_tta.argtypes)
    m = sets["head"].handle
    assert L.w2xc_process_image_rgba_u8_batch_device(None, m, 2, C.c_void_p(A), 4 * w * h, 4 * w, w, h, C.c_void_p(B), 16 * w * h, 8 * w, 1, 0.0, -1, None,
                                                     None) == ERR_UNSUPPORTED


# ---- the refusals of the two building blocks ----
def test_spread_u8_refusals(w2xc):
    f = w2xc.lib().w2xc_tta_spread_u8_device
    w, h, n = 10, 6, 2
    vs = w * h * 4
    UP, TR = 0x20000000, 0x30000000

    def call(src=A, n_=n, iis=4 * w * h, rs=4 * w, px=4, ch0=0, step=1, ww=w, hh=h, up=UP, tr=TR, vs_=vs):
        return f(C.c_void_p(src), n_, iis, rs, px, ch0, step, ww, hh, C.c_void_p(up), C.c_void_p(tr), vs_, None)
    cases = {
        "null source": call(src=0), "null upright group": call(up=0), "null transposed group": call(tr=0),
        "n = 0": call(n_=0), "n < 0": call(n_=-3), "w = 0": call(ww=0), "h < 0": call(hh=-1),
        "a row stride below a row": call(rs=4 * w - 1), "an image stride below an image": call(iis=4 * w * h - 1),
        "a variant stride below a plane": call(vs_=vs - 4), "a variant stride that is no multiple of 4": call(vs_=vs + 2),
        "pixels of 2 bytes": call(px=2), "pixels of 5 bytes": call(px=5),
        "ch0 < 0": call(ch0=-1), "ch_step < 0": call(step=-1, ch0=3), "ch0 outside the pixel": call(ch0=4, step=0),
        "the last channel outside the pixel": call(ch0=2, step=1), "colour of 3-byte pixels from byte 1": call(px=3, rs=3 * w, iis=3 * w * h, ch0=1),
        "the groups overlap each other": call(tr=UP + 4 * 3 * n * vs - 4),
        "the upright group overlaps the source": call(up=A + 4 * w * h * n - 1),
        "the transposed group overlaps the source": call(tr=A - 4 * 3 * n * vs + 1),
    }
    for what, rc in cases.items():
        assert rc == ERR_ARG, (what, rc, w2xc.last_error())


def test_gather_u8_refusals(w2xc):
    f = w2xc.lib().w2xc_tta_gather_u8_device
    w, h, n = 10, 6, 2
    vs = w * h * 4
    UP, TR = 0x20000000, 0x30000000

    def call(up=UP, tr=TR, vs_=vs, n_=n, ppi=3, first=0, nch=3, ww=w, hh=h, dst=A, iis=4 * w * h, rs=4 * w, px=4, byte0=0):
        return f(C.c_void_p(up), C.c_void_p(tr), vs_, n_, ppi, first, nch, ww, hh, C.c_void_p(dst), iis, rs, px, byte0, None)
    cases = {
        "null destination": call(dst=0), "null upright group": call(up=0), "null transposed group": call(tr=0),
        "n = 0": call(n_=0), "w = 0": call(ww=0), "h = 0": call(hh=0), "no planes per image": call(ppi=0), "no channel": call(nch=0),
        "a row stride below a row": call(rs=4 * w - 1), "an image stride below an image": call(iis=4 * w * h - 1),
        "a variant stride below a plane": call(vs_=vs - 4), "a variant stride that is no multiple of 4": call(vs_=vs + 1),
        "pixels of 1 byte": call(px=1), "pixels of 8 bytes": call(px=8),
        "byte0 < 0": call(byte0=-1), "the last byte outside the pixel": call(byte0=2), "alpha into byte 4": call(first=1, nch=1, byte0=4),
        "three bytes from byte 1 of 3-byte pixels": call(px=3, rs=3 * w, iis=3 * w * h, byte0=1),
        "first_plane < 0": call(first=-1, nch=1), "planes outside the image's": call(first=1), "two planes of a one-plane result": call(ppi=1, nch=2, byte0=2),
        "the groups overlap each other": call(tr=UP + 4 * 3 * n * vs - 4),
        "the upright group overlaps the destination": call(up=A + 4 * w * h * n - 1),
        "the transposed group overlaps the destination": call(tr=A - 4 * 3 * n * vs + 1),
    }
    for what, rc in cases.items():
        assert rc == ERR_ARG, (what, rc, w2xc.last_error())


# ---- the CLI ----
def _cli():
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_tta_alpha_parses_and_the_default_still_refuses():
    cli = _cli()
    ap = cli.build_parser()
    assert ap.parse_args(["-i", "a.png"]).tta_alpha == 0
    assert ap.parse_args(["-i", "a.png", "--tta", "1", "--tta_alpha", "1"]).tta_alpha == 1
    with pytest.raises(SystemExit):
        ap.parse_args(["-i", "a.png", "--tta_alpha", "2"])
    with pytest.raises(SystemExit) as ei:
        cli.check_tta(1, ["a.png", "b.png"])
    msg = str(ei.value.code)
    assert "a.png" in msg and "b.png" in msg and "transparency" in msg and "--tta_alpha" in msg
    with pytest.raises(SystemExit):
        cli.check_tta(1, ["a.png"], 0)
    cli.check_tta(1, ["a.png"], 1)      # the opt-in
    cli.check_tta(0, ["a.png"], 0)
    cli.check_tta(0, ["a.png"], 1)
    cli.check_tta(1, [], 0)


def test_cli_routes_under_tta_alpha():
    cli = _cli()
    groups = [files for _, files, _ in cli.group_inputs([("a.png", (4, 4)), ("b.png", (8, 4)), ("c.png", (4, 4))], "scale", 1, 2.0)]
    assert groups == [["a.png", "c.png"], ["b.png"]]
    # one call per size group, a file alone a batch of one; per model kind
    assert cli.alpha_tta_routes(False, groups) == [("rgba_batch_tta", ["a.png", "c.png"]), ("rgba_batch_tta", ["b.png"])]
    assert cli.alpha_tta_routes(True, groups) == [("rgba_up2x_batch_tta", ["a.png", "c.png"]), ("rgba_up2x_batch_tta", ["b.png"])]
    assert cli.alpha_tta_routes(False, []) == [] and cli.alpha_tta_routes(True, [[]]) == [] and cli.alpha_tta_routes(False, [[]]) == []
    # the pure helpers that existed keep their results
    assert cli.head_alpha_routes(groups) == [("rgba_up2x_batch", ["a.png", "c.png"]), ("rgba_up2x_batch", ["b.png"])]
    assert cli.head_routes(1, [], [["a.png"], ["b.png", "c.png"]]) == [("up2x_batch", ["a.png"]), ("up2x_batch", ["b.png", "c.png"])]
    assert cli.head_routes(0, [], [["a.png"], ["b.png", "c.png"]]) == [("single", ["a.png"]), ("up2x_batch", ["b.png", "c.png"])]
    assert cli.group_alpha([("a.png", (4, 4)), ("b.png", (8, 4)), ("c.png", (4, 4))], "scale", 1, 2.0) == (["b.png"], [["a.png", "c.png"]])
    assert "--tta_alpha" in cli.__doc__


def test_cli_main_refuses_transparent_inputs_under_tta_alone(tmp_path):
    """before a model is run: the decision is check_tta's, on the decoded images"""
    from PIL import Image
    cli = _cli()
    gen_model.write_json(gen_model.synth_layers([3, 32, 3], 9), str(tmp_path / "scale2.0x_model.json"))
    rgba = np.full((6, 5, 4), 200, np.uint8)
    rgba[2:4, 1:3, 3] = 17
    Image.fromarray(rgba).save(tmp_path / "t.png")
    args = ["-i", str(tmp_path / "t.png"), "-m", "scale", "--model_dir", str(tmp_path), "--tta", "1"]
    with pytest.raises(SystemExit) as ei:
        cli.main(args)
    assert "--tta_alpha" in str(ei.value.code)


# ---- the kernels' registers ----
def test_u8_tta_kernels_no_spill_no_scratch(w2xc):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, "w2xc_tta_u8.o")], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vspill=int(m.group(4)), sspill=int(m.group(5)), scratch=int(m.group(6)))
    assert len([n for n in rows if "k_ttau8_spread" in n]) == 2 and len([n for n in rows if "k_ttau8_gather" in n]) == 1, sorted(rows)
    for name, r in rows.items():
        assert "k_tta_spread" not in name and "k_tta_gather" not in name, name     # (tests/test_tta_api.py counts those names in w2xc_tta.o)
        assert r == dict(vspill=0, sspill=0, scratch=0), (name, r)
