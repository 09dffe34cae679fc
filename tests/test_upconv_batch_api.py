"""The batch and TTA forms of upconv head models (revision 0.4.1.6.1), everything that needs no GPU: the new symbols in the header, the library and the
binding, the refusals of the new calls (before a device is touched: this runs on a machine without one), w2xc_batch_plan with nn2x = 2, and the CLI's
routing.  The GPU side is tests/test_gpu_upconv_batch.py; what the EXISTING calls answer for a head model stays pinned by tests/test_upconv_api.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tools import gen_model
import upconv_ref as ur

ERR_ARG, ERR_PLANES, ERR_UNSUPPORTED = -3, -4, -6
# the three C entry points of the revision, and the four Python wrappers around them and the plan
C_SYMBOLS = ("w2xc_convert_planes_up2x_batch_device", "w2xc_process_image_rgb_u8_up2x_batch_device", "w2xc_process_image_rgb_u8_up2x_batch")


def head_set(w2xc, planes, nout, seed):
    layers, head = ur.head_model(list(planes), nout, seed)
    return w2xc._ModelSet.from_layers(layers, head=head), layers


@pytest.fixture(scope="module")
def sets(w2xc):
    pub, _ = head_set(w2xc, ur.PUBLISHED, 3, gen_model.SEEDS["upconv7"])
    c32, layers = head_set(w2xc, (3, 32), 3, 401)
    c64y, _ = head_set(w2xc, (1, 32, 64), 1, 402)
    return {"pub": pub, "c32": c32, "c64y": c64y, "plain": w2xc._ModelSet.from_layers(layers),
            "noise": w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 32, 3], 9))}


# ---- the symbols and the documents ----
def test_symbols_are_declared_exported_bound_and_wrapped(w2xc):
    header = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in C_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym          # declared
        assert getattr(w2xc.lib(), sym) is not None                  # exported
        assert sym in w2xc.ABI_SYMBOLS and sym in integration, sym
    assert callable(w2xc._ModelSet.convert_planes_up2x_batch_device)
    assert callable(w2xc.process_image_rgb_u8_up2x_batch) and callable(w2xc.process_image_rgb_u8_up2x_batch_device)
    assert "up2x" in w2xc._ModelSet.batch_plan.__code__.co_varnames


def test_revision(w2xc):
    assert C.sizeof(w2xc.Opts) == 56
    assert w2xc.lib().w2xc_version().decode() == "w2xc_hip 0.4.1.6.1 (gfx950)"
    for name in (os.path.join("include", "w2xc_hip.h"), "INTEGRATION.md"):
        assert "0.4.1.6.1" in open(os.path.join(ROOT, name)).read(), name


# ---- the refusals of the plane call ----
def test_plane_batch_refusals(w2xc, sets):
    L = w2xc.lib()
    w, h, n = 8, 6, 2
    src = np.zeros((n, 3, h, w), np.float32)
    dst = np.zeros((n, 3, 2 * h, 2 * w), np.float32)
    pi, po = src.ctypes.data, dst.ctypes.data
    iis, ips, irs = src.strides[:3]
    ois, ops, ors = dst.strides[:3]
    m = sets["c32"].handle

    def call(model=m, n_=n, nin=3, pi_=pi, iis_=iis, ips_=ips, irs_=irs, po_=po, ois_=ois, ops_=ops, ors_=ors, opts=None):
        return L.w2xc_convert_planes_up2x_batch_device(model, n_, nin, pi_, iis_, ips_, irs_, w, h, po_, ois_, ops_, ors_, None,
                                                       C.byref(opts) if opts is not None else None)
    cases = {
        "null model": (call(model=None), ERR_ARG),
        "null input": (call(pi_=None), ERR_ARG),
        "null output": (call(po_=None), ERR_ARG),
        "n = 0": (call(n_=0), ERR_ARG),
        "n < 0": (call(n_=-1), ERR_ARG),
        "short input rows": (call(irs_=4 * w - 4), ERR_ARG),
        "short output rows": (call(ors_=4 * w), ERR_ARG),          # (the output rows are 2w floats)
        "odd row stride": (call(irs_=4 * w + 2), ERR_ARG),
        "odd image stride": (call(iis_=iis + 2), ERR_ARG),
        "short output plane stride": (call(ops_=ors * h), ERR_ARG),    # (2h rows per plane)
        "output images overlap each other": (call(ois_=ois - 4), ERR_ARG),
        "output overlaps input": (call(po_=pi + 64), ERR_ARG),
        "a model without a head": (call(model=sets["plain"].handle), ERR_ARG),
        "a plane count the model does not take": (call(nin=1, ips_=0), ERR_PLANES),
        "a split precision": (call(opts=w2xc.make_opts(precision=w2xc.PRECISION_BF16X2)), ERR_UNSUPPORTED),
    }
    for what, (rc, want) in cases.items():
        assert rc == want, (what, rc, want)
    with pytest.raises(w2xc.W2xcError) as e:
        sets["plain"].convert_planes_up2x_batch_device(n, 3, pi, iis, ips, irs, w, h, po, ois, ops, ors)
    assert e.value.code == ERR_ARG and "no upconv head" in str(e.value)


# ---- the refusals of the image calls ----
def test_image_batch_refusals(w2xc, sets):
    L = w2xc.lib()
    w, h, n = 8, 6, 2
    src = np.zeros((n, h, w, 3), np.uint8)
    dst = np.zeros((n, 2 * h, 2 * w, 3), np.uint8)
    pi, po = src.ctypes.data, dst.ctypes.data
    iis, irs = src.strides[:2]
    ois, ors = dst.strides[:2]
    head, noise, plain = sets["c32"].handle, sets["noise"].handle, sets["plain"].handle
    split = w2xc.make_opts(precision=w2xc.PRECISION_BF16X2)

    def dev(mn=None, ms=head, n_=n, pi_=pi, iis_=iis, irs_=irs, po_=po, ois_=ois, ors_=ors, it=1, opts=None, tta=0):
        return L.w2xc_process_image_rgb_u8_up2x_batch_device(mn, ms, n_, pi_, iis_, irs_, w, h, po_, ois_, ors_, it, 0.0, None,
                                                             C.byref(opts) if opts is not None else None, tta)

    def host(mn=None, ms=head, n_=n, ins=None, irs_=irs, outs=None, ors_=ors, it=1, opts=None, tta=0, null_in=False, null_out=False):
        ip = (C.c_void_p * n)(*(ins if ins is not None else [src[i].ctypes.data for i in range(n)]))
        op = (C.c_void_p * n)(*(outs if outs is not None else [dst[i].ctypes.data for i in range(n)]))
        return L.w2xc_process_image_rgb_u8_up2x_batch(mn, ms, n_, None if null_in else ip, irs_, w, h, None if null_out else op, ors_, it, 0.0,
                                                      C.byref(opts) if opts is not None else None, tta)
    cases = {
        "device: null input": (dev(pi_=None), ERR_ARG),
        "device: null output": (dev(po_=None), ERR_ARG),
        "device: n = 0": (dev(n_=0), ERR_ARG),
        "device: short input rows": (dev(irs_=3 * w - 1), ERR_ARG),
        "device: short output rows": (dev(ors_=3 * w), ERR_ARG),
        "device: output images overlap each other": (dev(ois_=ois - 1), ERR_ARG),
        "device: output overlaps input": (dev(po_=pi + 16), ERR_ARG),
        "device: no scale model": (dev(mn=noise, ms=None, it=0), ERR_ARG),
        "device: a scale model without a head": (dev(ms=plain), ERR_ARG),
        "device: a head model as noise model": (dev(mn=head), ERR_UNSUPPORTED),
        "device: a split precision": (dev(opts=split), ERR_UNSUPPORTED),
        "device: tta = 2": (dev(tta=2), ERR_ARG),
        "device: tta = -1": (dev(tta=-1), ERR_ARG),
        "host: null input array": (host(null_in=True), ERR_ARG),
        "host: null output array": (host(null_out=True), ERR_ARG),
        "host: a null image": (host(ins=[src[0].ctypes.data, None]), ERR_ARG),
        "host: n = 0": (host(n_=0), ERR_ARG),
        "host: short input rows": (host(irs_=3 * w - 1), ERR_ARG),
        "host: outputs overlap each other": (host(outs=[po, po + 8]), ERR_ARG),
        "host: output overlaps input": (host(outs=[po, pi]), ERR_ARG),
        "host: a scale model without a head": (host(ms=plain), ERR_ARG),
        "host: a head model as noise model": (host(mn=head), ERR_UNSUPPORTED),
        "host: a split precision": (host(opts=split), ERR_UNSUPPORTED),
        "host: tta = 2": (host(tta=2), ERR_ARG),
    }
    for what, (rc, want) in cases.items():
        assert rc == want, (what, rc, want)
    # a one-plane head model is no RGB model
    assert dev(ms=sets["c64y"].handle) == ERR_PLANES


# ---- the plan ----
def test_batch_plan_of_the_head_call(w2xc, sets):
    for name in ("pub", "c32"):
        batched, sub = sets[name].batch_plan(3, 70, 40, up2x=True)
        assert batched == 1 and sub >= 1, name
        assert sets[name].batch_plan(3, 70, 40) == (0, 1)                  # the calls nn2x = 0 / 1 plan refuse a head model: as before
        assert sets[name].batch_plan(3, 70, 40, nn2x=True) == (0, 1)
        assert sets[name].batch_plan(3, 70, 40, up2x=True, opts=w2xc.make_opts(kernel=1))[0] == 0          # W2XC_KERNEL_DIRECT
        assert sets[name].batch_plan(3, 70, 40, up2x=True, opts=w2xc.make_opts(band_rows=8))[0] == 0       # more than one band
    assert sets["c64y"].batch_plan(1, 70, 40, up2x=True) == (0, 1)         # a one-plane head model: the single-image sequence per image
    with pytest.raises(w2xc.W2xcError) as e:
        sets["plain"].batch_plan(3, 70, 40, up2x=True)
    assert e.value.code == ERR_ARG
    with pytest.raises(w2xc.W2xcError) as e:
        sets["pub"].batch_plan(3, 70, 40, up2x=True, opts=w2xc.make_opts(precision=w2xc.PRECISION_BF16X2))
    assert e.value.code == ERR_UNSUPPORTED
    bp = C.c_int(0)
    assert w2xc.lib().w2xc_batch_plan(sets["pub"].handle, 3, 70, 40, 3, None, C.byref(bp), C.byref(bp)) == ERR_ARG


def test_sub_batch_shrinks_with_the_workspace(w2xc, sets):
    ms = sets["pub"]
    subs = [ms.batch_plan(3, 64, 64, up2x=True, opts=w2xc.make_opts(workspace_mb=mb)) for mb in (4096, 256, 64, 16)]
    assert all(b == 1 for b, _ in subs), subs
    counts = [s for _, s in subs]
    assert counts == sorted(counts, reverse=True) and counts[0] > counts[-1] >= 1, counts
    # the budget is bytes: 16 times the workspace holds 16 times the images (up to one image's rounding)
    assert counts[1] // 16 <= counts[3] <= counts[1] // 16 + 1, counts


# ---- the CLI's routing ----
def test_cli_routes_head_models_to_the_batch_call():
    from tools import w2xc_cli
    assert w2xc_cli.head_routes(0, [], [["a.png", "b.png"], ["c.png"]]) == [("up2x_batch", ["a.png", "b.png"]), ("single", ["c.png"])]
    assert w2xc_cli.head_routes(1, [], [["a.png"], ["b.png", "c.png"]]) == [("up2x_batch", ["a.png"]), ("up2x_batch", ["b.png", "c.png"])]
    assert w2xc_cli.head_routes(0, [], []) == []
    for tta in (0, 1):
        with pytest.raises(SystemExit) as e:
            w2xc_cli.head_routes(tta, ["t.png"], [["a.png", "b.png"]])
        assert "upconv" in str(e.value) and "t.png" in str(e.value)
