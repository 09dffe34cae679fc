"""upconv head models, everything that needs no GPU: the float64 restatement against the index formula of the header, the JSON loader, the constructor,
kernel selection (no layer of the published topology on conv3x3_direct), the band plan, the refusals of every entry point that does not run a head
model, and the documents.  The GPU side is tests/test_gpu_upconv.py, the packer tests/test_upconv_pack.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from tools import gen_model
import upconv_ref as ur

ERR_JSON, ERR_ARG, ERR_UNSUPPORTED = -2, -3, -6
SIZES = [(1, 1), (5, 9), (17, 33)]


def small_head_model(w2xc, planes=(3, 16, 32), nout=3, seed=7, bias=True):
    layers, head = ur.head_model(list(planes), nout, seed, bias)
    return w2xc._ModelSet.from_layers(layers, head=head), layers, head


# ---- the restatement ----
@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_equals_the_index_formula(h, w):
    layers, head = ur.head_model([3, 8, 16], 3, 11)
    x = np.random.default_rng(h * 100 + w).random((3, h, w))
    z = ur.chain_z(layers, x, 3).numpy()
    assert z.shape == (16, h + 2, w + 2)   # n - 1 valid layers of a pad-n source leave a one-pixel rim
    want = ur.head_formula(z, *head)
    got = F.conv_transpose2d(torch.from_numpy(z)[None], torch.from_numpy(head[0].astype(np.float64)),
                             torch.from_numpy(head[1].astype(np.float32).astype(np.float64)), stride=2, padding=3)[0].numpy()
    assert got.shape == want.shape == (3, 2 * h, 2 * w)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    assert np.abs(ur.reference(layers, head, x) - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def test_pad_by_layer_count_equals_the_chain_on_the_pad1_source():
    # valid_{n-1}(pad_n(x)) == "replicate-pad by the layer count" of the (n - 1)-layer chain run on the pad-1 source
    layers, _ = ur.head_model([3, 8, 16], 3, 12)
    x = np.random.default_rng(3).random((3, 5, 9))
    x1 = F.pad(torch.from_numpy(x)[None], (1, 1, 1, 1), mode="replicate")[0].numpy()
    assert np.array_equal(ur.chain_z(layers, x, 3).numpy(), ur.chain_z(layers, x1, 2).numpy())


# ---- the loader ----
@pytest.mark.parametrize("bias", [True, False])
def test_json_round_trip(w2xc, tmp_path, bias):
    layers, head = ur.head_model([3, 16, 32], 3, 21, bias)
    path = gen_model.write_json(layers, str(tmp_path / "up.json"), head=head)
    ms = w2xc._ModelSet.from_json(path)
    assert ms.has_head and ms.n_layers == 3
    assert [ms.planes(l) for l in range(3)] == [(3, 16), (16, 32), (32, 3)]   # what the model declares, the head as the last layer
    for l, (nin, nout, w, b) in enumerate(layers):
        gi, go, gw, gb = ms.layer_arrays(l)
        assert (gi, go) == (nin, nout) and np.array_equal(gw, w) and np.array_equal(gb, b)
    _, _, hw, hb = ms.layer_arrays(2)
    assert hw.shape == (32, 3, 4, 4) and np.array_equal(hw, head[0])
    assert np.array_equal(hb, head[1] if bias else np.zeros(3))
    same = w2xc._ModelSet.from_layers(layers, head=head)
    assert same.has_head and [same.kernel_name(l) for l in range(3)] == [ms.kernel_name(l) for l in range(3)]


def _head_json(tmp_path, name, edit, planes=(3, 16, 32)):
    layers, head = ur.head_model(list(planes), 3, 22)
    path = gen_model.write_json(layers, str(tmp_path / name), head=head)
    with open(path) as f:
        objs = json.load(f)
    objs = edit(objs) or objs
    with open(path, "w") as f:
        json.dump(objs, f)
    return path


def _load_rc(w2xc, path):
    h = C.c_void_p()
    rc = w2xc.lib().w2xc_model_load_json(os.fsencode(path), C.byref(h))
    if rc == 0:
        w2xc.lib().w2xc_model_free(h)
    return rc


def test_loader_refusals(w2xc, tmp_path):
    def drop(*keys):
        def edit(objs):
            for k in keys:
                del objs[-1][k]
        return edit
    assert _load_rc(w2xc, _head_json(tmp_path, "nostride.json", drop("dW", "dH"))) == ERR_UNSUPPORTED
    assert _load_rc(w2xc, _head_json(tmp_path, "nopad.json", drop("padW", "padH"))) == ERR_UNSUPPORTED
    assert "only 3x3 is supported" in w2xc.last_error()
    assert _load_rc(w2xc, _head_json(tmp_path, "notlast.json", lambda o: o[:1] + [o[-1]] + o[1:-1])) == ERR_UNSUPPORTED
    assert _load_rc(w2xc, _head_json(tmp_path, "class.json", lambda o: o[-1].update(class_name="nn.SpatialConvolutionMM"))) == ERR_UNSUPPORTED
    assert _load_rc(w2xc, _head_json(tmp_path, "outer.json", lambda o: o[-1].update(weight=o[-1]["weight"][:-1]))) == ERR_JSON
    assert _load_rc(w2xc, _head_json(tmp_path, "inner.json", lambda o: o[-1].update(weight=[wi[:-1] for wi in o[-1]["weight"]]))) == ERR_JSON
    # the non-square message stays
    assert _load_rc(w2xc, _head_json(tmp_path, "nonsq.json", lambda o: o[-1].update(kH=3))) == ERR_UNSUPPORTED
    assert "not square" in w2xc.last_error()
    assert _load_rc(w2xc, _head_json(tmp_path, "ok.json", lambda o: None)) == 0


# ---- the constructor ----
def test_add_head_twice_is_refused(w2xc):
    ms, layers, head = small_head_model(w2xc)
    with pytest.raises(w2xc.W2xcError) as e:
        ms.add_upconv_head(*head)
    assert e.value.code == ERR_ARG
    plain = w2xc._ModelSet.from_layers(layers)
    assert not plain.has_head and plain.n_layers == 2
    w = np.zeros((32, 2, 4, 4), np.float32)
    assert w2xc.lib().w2xc_model_add_upconv_head(plain.handle, 2, w.ctypes.data, None) == ERR_ARG   # 1 or 3 planes
    assert w2xc.lib().w2xc_model_add_upconv_head(plain.handle, 3, None, None) == ERR_ARG


# ---- kernel selection ----
def test_published_topology_has_no_layer_on_the_direct_kernel(w2xc):
    ms, _, _ = small_head_model(w2xc, ur.PUBLISHED, 3, gen_model.SEEDS["upconv7"])
    names = [ms.kernel_name(l) for l in range(ms.n_layers)]
    assert ms.n_layers == 7 and "conv3x3_direct" not in names, names
    assert names == ["conv3x3_first", "conv3x3_wino", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_wino4", "upconv4x4_head"]
    assert [ms.planes(l) for l in range(7)] == [(3, 16), (16, 32), (32, 64), (64, 128), (128, 128), (128, 256), (256, 3)]
    direct = w2xc.make_opts(kernel=1)   # W2XC_KERNEL_DIRECT: the 3x3 chain on the direct kernel, the head stays the head kernel
    assert [ms.kernel_name(l, direct) for l in range(7)] == ["conv3x3_direct"] * 6 + ["upconv4x4_head"]


def test_a_headless_model_keeps_its_selection(w2xc):
    ms = w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 16, 32, 128, 256, 3], 5))
    assert [ms.kernel_name(l) for l in range(5)] == ["conv3x3_direct", "conv3x3_direct", "conv3x3_wino4", "conv3x3_direct", "conv3x3_direct"]
    assert [ms.planes(l) for l in range(5)] == [(3, 16), (16, 32), (32, 128), (128, 256), (256, 3)]


# ---- the plan ----
@pytest.mark.parametrize("band", [4, 8])
def test_plan_bands_tile_the_plane(w2xc, band):
    ms, _, _ = small_head_model(w2xc, ur.PUBLISHED, 3, gen_model.SEEDS["upconv7"])
    H, W, n = 17, 33, 7
    for kernel, hl in ((0, 4), (4, 1)):   # the default F(4x4) geometry; W2XC_KERNEL_WINOGRAD32: one halo row per layer
        plan = ms.plan_rows(W, H, opts=w2xc.make_opts(band_rows=band, kernel=kernel))
        assert (plan.n_layers, plan.halo_rows_per_layer, plan.band_rows) == (n, hl, band)
        assert plan.n_bands == -(-H // band)
        covered = []
        for a in range(0, H, plan.band_rows):
            b = min(H, a + plan.band_rows)
            assert ms.plan_region(plan, H, n, a, b) == (a, b)   # the head: source rows [a, b) = output rows [2a, 2b)
            covered += list(range(2 * a, 2 * b))
            t, bt = ms.plan_region(plan, H, n - 1, a, b)       # layer n - 1 in plane rows; z row i = plane row i - 1
            if hl == 1:
                assert (t + 1, bt + 1) == (a, b + 2)           # exactly the z rows [a, b + 2) the head reads
            else:
                assert t + 1 <= a and bt + 1 >= b + 2 and t >= -1 and bt <= H + 1
        assert covered == list(range(2 * H))   # no gap, no overlap


def test_plan_refuses_what_has_no_kernel(w2xc):
    ms, _, _ = small_head_model(w2xc)
    with pytest.raises(w2xc.W2xcError) as e:
        ms.plan_rows(33, 17, opts=w2xc.make_opts(precision=2))   # split precisions with a head model
    assert e.value.code == ERR_UNSUPPORTED
    odd, _, _ = small_head_model(w2xc, (3, 32, 48))
    with pytest.raises(w2xc.W2xcError) as e:
        odd.plan_rows(33, 17)
    assert e.value.code == ERR_UNSUPPORTED


# ---- the refusals: no device is touched (this runs on a machine without one) ----
def test_every_other_entry_point_refuses_a_head_model(w2xc):
    ms, layers, head = small_head_model(w2xc)
    one, _, _ = small_head_model(w2xc, (1, 32), 1)
    noise = w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 32, 3], 9))
    L = w2xc.lib()
    w, h = 8, 6
    buf_in = np.zeros((4, 4 * h, 4 * w), np.float32)
    buf_out = np.zeros((4, 4 * h, 4 * w), np.float32)
    pi, po = buf_in.ctypes.data, buf_out.ctypes.data
    rs, ps = buf_in.strides[1], buf_in.strides[0]
    ptrs_in = (C.c_void_p * 1)(pi)
    ptrs_out = (C.c_void_p * 1)(po)
    m3, m1 = ms.handle, one.handle
    calls = {
        "convert_plane": lambda: L.w2xc_convert_plane(m1, pi, rs, w, h, po, rs, 1, None),
        "convert_plane_device": lambda: L.w2xc_convert_plane_device(m1, pi, rs, w, h, po, rs, None, None),
        "convert_plane_nn2x": lambda: L.w2xc_convert_plane_nn2x(m1, pi, rs, w, h, po, rs, None),
        "convert_plane_nn2x_device": lambda: L.w2xc_convert_plane_nn2x_device(m1, pi, rs, w, h, po, rs, None, None),
        "convert_plane_rows": lambda: L.w2xc_convert_plane_rows(m1, pi, rs, 0, h, w, h, 0, 0, h, po, rs, None),
        "convert_rows_device": lambda: L.w2xc_convert_rows_device(m1, pi, rs, h, 0, w, h, 0, h, po, rs, None, None),
        "convert_planes_device": lambda: L.w2xc_convert_planes_device(m3, 3, pi, ps, rs, w, h, po, ps, rs, None, None),
        "convert_planes_nn2x_device": lambda: L.w2xc_convert_planes_nn2x_device(m3, 3, pi, ps, rs, w, h, po, ps, rs, None, None),
        "convert_batch": lambda: L.w2xc_convert_batch(m1, 1, 0, ptrs_in, rs, w, h, ptrs_out, rs, None),
        "convert_batch_device": lambda: L.w2xc_convert_batch_device(m1, 1, 0, pi, ps, rs, w, h, po, ps, rs, None, None),
        "convert_planes_batch_device": lambda: L.w2xc_convert_planes_batch_device(m3, 1, 0, 3, pi, 3 * ps, ps, rs, w, h, po, 3 * ps, ps, rs, None, None),
        "convert_batch_tta_device": lambda: L.w2xc_convert_batch_tta_device(m1, 1, 0, pi, ps, rs, w, h, po, ps, rs, None, None),
        "convert_planes_tta_device": lambda: L.w2xc_convert_planes_tta_device(m3, 3, 0, pi, ps, rs, w, h, po, ps, rs, None, None),
        "layer_filter(head)": lambda: L.w2xc_layer_filter(m3, 2, 32, ptrs_in, rs, w, h, ptrs_out, rs, None),
        "layer_filter_device(head)": lambda: L.w2xc_layer_filter_device(m3, 2, 32, pi, ps, rs, 1, w, h, po, ps, rs, 1, None, None),
        # the Y route, and everything around the RGB route but its single-image call
        "process_image_u8_ex": lambda: L.w2xc_process_image_u8_ex(None, m1, pi, rs, w, h, po, rs, 1, 0.0, None),
        "process_image_u8_ex_device": lambda: L.w2xc_process_image_u8_ex_device(None, m1, pi, rs, w, h, po, rs, 1, 0.0, None, None),
        "scale2x_image_u8": lambda: L.w2xc_scale2x_image_u8(m1, pi, rs, w, h, po, rs, 1, None),
        "process_image_u8_batch": lambda: L.w2xc_process_image_u8_batch(None, m1, 1, ptrs_in, rs, w, h, ptrs_out, rs, 1, 0.0, None),
        "process_image_u8_batch_device": lambda: L.w2xc_process_image_u8_batch_device(None, m1, 1, pi, ps, rs, w, h, po, ps, rs, 1, 0.0, None, None),
        "process_image_rgb_u8_batch": lambda: L.w2xc_process_image_rgb_u8_batch(None, m3, 1, ptrs_in, rs, w, h, ptrs_out, rs, 1, 0.0, None),
        "process_image_rgb_u8_batch_device": lambda: L.w2xc_process_image_rgb_u8_batch_device(None, m3, 1, pi, ps, rs, w, h, po, ps, rs, 1, 0.0, None, None),
        "process_image_rgb_u8_tta": lambda: L.w2xc_process_image_rgb_u8_tta(None, m3, pi, rs, w, h, po, rs, 1, 0.0, None, 1),
        "process_image_rgb_u8_tta_device": lambda: L.w2xc_process_image_rgb_u8_tta_device(None, m3, pi, rs, w, h, po, rs, 1, 0.0, None, None, 1),
        "process_image_rgba_u8_ex": lambda: L.w2xc_process_image_rgba_u8_ex(None, m3, pi, rs, w, h, po, rs, 1, 0.0, -1, None),
        "process_image_rgba_u8_ex_device": lambda: L.w2xc_process_image_rgba_u8_ex_device(None, m3, pi, rs, w, h, po, rs, 1, 0.0, -1, None, None),
        "process_image_rgba_u8_batch": lambda: L.w2xc_process_image_rgba_u8_batch(None, m3, 1, ptrs_in, rs, w, h, ptrs_out, rs, 1, 0.0, -1, None),
        "process_image_rgba_u8_batch_device": lambda: L.w2xc_process_image_rgba_u8_batch_device(None, m3, 1, pi, ps, rs, w, h, po, ps, rs, 1, 0.0, -1, None, None),
        # a head model is a scale model: never the noise model
        "rgb_ex(noise=head)": lambda: L.w2xc_process_image_rgb_u8_ex(m3, None, pi, rs, w, h, po, rs, 0, 0.0, None),
        "rgb_ex_device(noise=head)": lambda: L.w2xc_process_image_rgb_u8_ex_device(m3, noise.handle, pi, rs, w, h, po, rs, 1, 0.0, None, None),
    }
    for name, call in calls.items():
        assert call() == ERR_UNSUPPORTED, (name, w2xc.last_error())
        msg = w2xc.last_error()
        assert "w2xc_convert_planes_up2x_device" in msg and "w2xc_process_image_rgb_u8_ex" in msg, (name, msg)
    # the C++ adapter's convertWithModels is w2xc_convert_plane (include/w2xc/convertRoutine.hpp); the Python one likewise
    with pytest.raises(w2xc.W2xcError) as e:
        one.convert(np.zeros((h, w), np.float32))
    assert e.value.code == ERR_UNSUPPORTED
    assert one.batch_plan(1, w, h) == (0, 1)   # w2xc_batch_plan: not batched
    # the plane call wants a head model
    plain = w2xc._ModelSet.from_layers(layers)
    assert L.w2xc_convert_planes_up2x_device(plain.handle, 3, pi, ps, rs, w, h, po, ps, rs, None, None) == ERR_ARG


# ---- the CLI's checks ----
def test_cli_refuses_what_a_head_model_cannot_run():
    from tools import w2xc_cli
    w2xc_cli.check_head(False, 1, ["a.png"], [["b.png", "c.png"]])   # no head model: not this check's business
    w2xc_cli.check_head(True, 0, [], [["a.png"], ["b.png"]])         # inputs of different sizes: one call each
    for args in ((True, 1, [], [["a.png"]]), (True, 0, ["t.png"], []), (True, 0, [], [["a.png", "b.png"], ["c.png"]])):
        with pytest.raises(SystemExit) as e:
            w2xc_cli.check_head(*args)
        assert "upconv" in str(e.value)


# ---- the documents ----
def test_documents_name_the_revision_and_the_symbols(w2xc):
    assert C.sizeof(w2xc.Opts) == 56
    assert "0.4.1.6" in w2xc.lib().w2xc_version().decode()
    header = open(os.path.join(ROOT, "include", "w2xc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (header, integration):
        assert "0.4.1.6" in text
        for sym in ("w2xc_model_add_upconv_head", "w2xc_model_has_head", "w2xc_convert_planes_up2x_device"):
            assert sym in text, sym
    for sym in ("w2xc_model_add_upconv_head", "w2xc_model_has_head", "w2xc_convert_planes_up2x_device"):
        assert sym in w2xc.ABI_SYMBOLS
