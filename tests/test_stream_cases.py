"""The table of device entry points (tests/stream_cases.py) is complete -- checked without a GPU: every callable of the package whose name ends in `_device`
has a row, every prototype of include/w2xc_hip.h with a `hip_stream` parameter is named by one, and a device call that comes without a row is reported here."""
import inspect
import os
import re

from conftest import ROOT
import stream_cases as sc

HEADER = os.path.join(ROOT, "include", "w2xc_hip.h")


def stream_prototypes():
    """the names of the header's prototypes that take `hip_stream`"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {name for name, args in re.findall(r"\b(w2xc_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S) if "hip_stream" in args}


def device_callables(w2xc):
    """name -> callable, module level and _ModelSet (a leading underscore: a helper of the package, no entry point)"""
    found = {n: getattr(w2xc, n) for n in dir(w2xc) if n.endswith("_device") and not n.startswith("_") and callable(getattr(w2xc, n))}
    found.update({"_ModelSet." + n: getattr(w2xc._ModelSet, n) for n in dir(w2xc._ModelSet) if n.endswith("_device") and not n.startswith("_")})
    return found


def uncovered(w2xc, rows):
    """what the table lacks: callables without a row, `tta=` forms without one, prototypes no row names"""
    out = []
    for name, fn in sorted(device_callables(w2xc).items()):
        mine = [r for r in rows if r.py == name]
        if not mine:
            out.append(name)
        elif "tta" in inspect.signature(fn).parameters and {r.tta for r in mine} != {False, True}:
            out.append(name + "(tta=)")
    return out + sorted(stream_prototypes() - {r.symbol for r in rows})


def test_the_header_scan_finds_the_stream_prototypes_and_nothing_else():
    """the first and the last prototype with a stream, one whose arguments span lines, none of the host forms and helpers around them"""
    protos = stream_prototypes()
    assert {"w2xc_convert_plane_device", "w2xc_process_frames_yuv_u16_rgb_sized_device", "w2xc_layer_filter_device"} <= protos
    assert all(p.endswith("_device") for p in protos), sorted(protos)
    text = open(HEADER).read()
    assert all(re.search(r"\b%s\s*\(" % p, text) for p in protos)
    # every `void *hip_stream` of the header belongs to a prototype that was found
    assert len(re.findall(r"void\s*\*\s*hip_stream", text)) == len(protos)


def test_every_device_call_has_a_row(w2xc):
    assert uncovered(w2xc, sc.ROWS) == []
    calls = device_callables(w2xc)
    for name in ("_ModelSet.filter_device", "_ModelSet.convert_rows_device", "_ModelSet.scale2x_image_u8_device", "process_frames_yuv_u16_rgb_sized_device"):
        assert name in calls, name


def test_every_row_names_a_symbol_of_the_header_and_a_callable(w2xc):
    protos, calls = stream_prototypes(), device_callables(w2xc)
    for r in sc.ROWS:
        assert r.symbol in protos and r.symbol in w2xc.ABI_SYMBOLS, r.id
        assert r.py is None or r.py in calls, r.id
        assert r.family in ("model", "frame", "block") and callable(r.build), r.id
        assert r.waits is None, "%s: a call that waits for the device names its source line, and the header says so" % r.id


def test_a_missing_row_and_a_new_device_call_are_reported(w2xc, monkeypatch):
    without = tuple(r for r in sc.ROWS if r.py != "chroma2x_u8_sited_device")
    assert uncovered(w2xc, without) == ["chroma2x_u8_sited_device", "w2xc_chroma2x_u8_sited_device"]
    without = tuple(r for r in sc.ROWS if not (r.py == "process_image_u8_device" and r.tta))
    assert uncovered(w2xc, without) == ["process_image_u8_device(tta=)", "w2xc_process_image_u8_tta_device"]
    without = tuple(r for r in sc.ROWS if r.symbol != "w2xc_resize2x_cubic_device")
    assert uncovered(w2xc, without) == ["w2xc_resize2x_cubic_device"]
    monkeypatch.setattr(w2xc, "sharpen_device", lambda d_in, d_out, stream=0: None, raising=False)
    monkeypatch.setattr(w2xc._ModelSet, "convert_mirror_device", lambda self, d_in, d_out, stream=0: None, raising=False)
    assert uncovered(w2xc, sc.ROWS) == ["_ModelSet.convert_mirror_device", "sharpen_device"]


def test_the_variant_rows_the_frame_rows_and_the_control_rows(w2xc):
    ids = {r.id for r in sc.ROWS}
    assert {"convert-banded", "convert-prog", "convert_batch-sub2"} <= ids
    frames = [r for r in sc.ROWS if r.family == "frame"]
    assert sorted(r.py for r in frames) == sorted("process_frames_yuv_u%d%s%s_device" % (b, c, s) for b in (8, 16) for c in ("", "_rgb") for s in ("", "_sized"))
    assert [sc.BY_ID[i].family for i in sc.CONTROL] == ["model", "frame", "block"]


def test_the_banded_row_has_bands_and_the_batch_row_sub_batches(w2xc):
    """host arithmetic: w2xc_plan_rows and w2xc_batch_plan"""
    ctx = sc.Ctx(w2xc)
    ms = ctx.model("yn")
    for v in (0, 1):
        h, w = sc.size(v)
        assert ms.plan_rows(w, h, opts=ctx.opts()).n_bands == 1
        assert ms.plan_rows(w, h, opts=ctx.opts(band_rows=8)).n_bands > 1
        o = sc.sub_batch_opts(ctx, ms, 1, w, h, 2)
        assert ms.batch_plan(1, w, h, False, o) == (1, 2), "3 planes run as 2 + 1"
        assert ms.batch_plan(1, w, h, False, ctx.opts())[1] >= 3
