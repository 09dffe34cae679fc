"""Every selection decision of csrc/w2xc_select.cpp as text: one line per (topology, options, plane), taken through the entry points that need no device --
w2xc_layer_kernel_name per layer, w2xc_plan_rows (all fields, both workspace sizes) and w2xc_batch_plan (batched, sub-batch).  Together they expose the
kind and the mid variant of every layer, both fusions, the halo geometry, the band height, and -- through the workspace bytes -- out_terms, the planar
layouts and the tap-plane halves; a refused call is its error code and message.

    python tools/select_sweep.py            the lines on stdout
    python tools/select_sweep.py --write    tests/golden/select_sweep.txt.gz (what tests/test_select_sweep.py compares against, line for line)

The fixture was recorded from the library BEFORE the selection predicates became the resolved chain (resolve_chain) and is not to be regenerated for a
change that is meant to keep the decisions; one that moves a decision regenerates it and shows the diff of the lines.
Regenerated once since: plan_rows refuses a plane that conv3x3_wino4 cannot address in any band -- the 108 lines of 2000000x64 whose chain runs conv3x3_wino4 on
32 NHWC planes went from a plan (whose launch failed) to that refusal, and the plane 1300000x64 joined so that the fused-first give-up stays on record.

A line:   <topology> p<precision>k<kernel>f<fusion> <plane> | <kernel codes, one letter per layer> | <plan> | <batch plan>
    plan = n_layers,halo,band_rows,n_bands,fused_first,fused_last,ws0,ws1    batch plan = batched,sub_batch    refusal = !<code>:<message>"""
import gzip
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402
from tools import gen_model  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "select_sweep.txt.gz")

# (planes of the 3x3 layers, output planes of an upconv head or 0)
TOPOLOGIES = [
    ([1, 32, 32, 64, 64, 128, 128, 1], 0),   # the scale model
    ([3, 32, 32, 64, 64, 128, 128, 3], 0),   # the RGB model
    ([1, 32, 1], 0),                         # two layers
    ([1, 32, 32, 1], 0), ([1, 32, 64, 1], 0),            # n = 3: the two fusions compete in the 16-bit modes
    ([1, 32, 32, 32, 1], 0), ([1, 32, 32, 64, 1], 0),    # n = 4: they compete in fp32
    ([1, 32, 32, 64, 64, 1], 0),             # n = 5: the shortest batch chain
    ([1, 64, 64, 1], 0),
    ([1, 32, 128, 128, 1], 0),
    ([3, 32, 3], 0), ([3, 64, 64, 3], 0), ([3, 128, 3], 0),   # three planes in and out
    ([1, 16, 1], 0), ([1, 32, 48, 1], 0),    # shapes with no fast kernel
    ([3, 16, 32, 64, 128, 128, 256], 3),     # upconv_7: the 128 -> 256 layer in front of a three-plane head
    ([1, 16, 32, 64, 128, 128, 256], 1),     # the same behind one plane, a one-plane head
    ([1, 32, 64], 1),                        # a short one-plane head model
]
SCALE = TOPOLOGIES[0][0]

# one letter per kernel name (a name that is not listed prints as it is)
CODES = {"conv3x3_direct": "d", "conv3x3_mfma": "m", "conv3x3_wino": "w", "conv3x3_wino4": "W", "conv3x3_first": "f", "conv3x3_last": "l",
         "conv3x3_split": "s", "conv3x3_first_split": "F", "conv3x3_last_gather": "g", "conv3x3_first2_split": "S", "(in_next_layer)": "<",
         "conv3x3_first2_wino4": "2", "upconv4x4_head": "u", "(in_previous_layer)": ">"}


def option_sets(w2xc):
    """fp32: every kernel x every fusion; each 16-bit precision: {AUTO, DIRECT} x every fusion"""
    fusions = range(w2xc.FUSION_AUTO, w2xc.FUSION_PROG + 1)
    for kernel in range(w2xc.KERNEL_AUTO, w2xc.KERNEL_WINOGRAD4 + 1):
        for fusion in fusions:
            yield w2xc.PRECISION_FP32, kernel, fusion
    for precision in (w2xc.PRECISION_BF16, w2xc.PRECISION_BF16X2, w2xc.PRECISION_BF16X3, w2xc.PRECISION_FP16X2):
        for kernel in (w2xc.KERNEL_AUTO, w2xc.KERNEL_DIRECT):
            for fusion in fusions:
                yield precision, kernel, fusion


def _refusal(e):
    return "!%d:%s" % (e.code, str(e).split(": ", 1)[1].replace("\n", "\\n"))


def _line(w2xc, ms, tag, head, n_in, name, plan_args, batch_wh, **okw):
    names = "".join(CODES.get(k, "[%s]" % k) for k in (ms.kernel_name(l, w2xc.make_opts(**okw)) for l in range(ms.n_layers)))
    try:
        p = ms.plan_rows(*plan_args, opts=w2xc.make_opts(**okw))
        plan = "%d,%d,%d,%d,%d,%d,%d,%d" % (p.n_layers, p.halo_rows_per_layer, p.band_rows, p.n_bands, p.fused_first, p.fused_last,
                                          p.workspace_bytes[0], p.workspace_bytes[1])
    except w2xc.W2xcError as e:
        plan = _refusal(e)
    batch = "-"
    if batch_wh:
        try:
            batch = "%d,%d" % ms.batch_plan(n_in, batch_wh[0], batch_wh[1], up2x=bool(head), opts=w2xc.make_opts(**okw))
        except w2xc.W2xcError as e:
            batch = _refusal(e)
    return "%s p%dk%df%d %s | %s | %s | %s" % (tag, okw["precision"], okw["kernel"], okw["fusion"], name, names, plan, batch)


def sweep_lines(w2xc):
    lines, later = [], []
    for planes, head in TOPOLOGIES:
        layers = gen_model.synth_layers(planes, 7)
        ms = w2xc._ModelSet.from_layers(layers, head=gen_model.synth_head(planes[-1], head, 7) if head else None)
        tag = "-".join(map(str, planes)) + ("^%d" % head if head else "")
        n = ms.n_layers
        for precision, kernel, fusion in option_sets(w2xc):
            okw = dict(precision=precision, kernel=kernel, fusion=fusion)
            lines.append(_line(w2xc, ms, tag, head, planes[0], "64x64", (64, 64), (64, 64), **okw))
            # banded: the solver's repeated workspace evaluation is on record
            lines.append(_line(w2xc, ms, tag, head, planes[0], "3000x4000/64M", (3000, 4000), (3000, 4000), workspace_mb=64, **okw))
            # too wide for the fused first layers -- and for conv3x3_wino4 on 32 NHWC planes (24 in_rs 4 >= 2^32, which no band changes): every chain that
            # has such a layer is refused, whatever the fusion
            lines.append(_line(w2xc, ms, tag, head, planes[0], "2000000x64", (2000000, 64), (2000000, 64), **okw))
            # too wide for the fused first layers only: FUSION_AUTO gives that fusion up, an explicit request is refused (behind the lines of the first
            # recording, which keep their places)
            later.append(_line(w2xc, ms, tag, head, planes[0], "1300000x64", (1300000, 64), (1300000, 64), **okw))
            if planes == SCALE and not head:   # a row view with the minimum halo: refused under KERNEL_AUTO in fp32
                ra, rb = w2xc.shard_rows(600, 3, 1)
                y0, y1 = w2xc.shard_view(600, ra, rb, n)
                lines.append(_line(w2xc, ms, tag, head, planes[0], "128x600[%d,%d)min" % (ra, rb), (128, 600, ra, rb, y0, y1 - y0), None, **okw))
    return lines + later


def read_fixture(path=FIXTURE):
    with gzip.open(path, "rt", encoding="utf-8") as f:
        return f.read().splitlines()


def write_fixture(lines, path=FIXTURE):
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, compresslevel=9, mtime=0) as f:   # (no name, no time: the same lines give the same bytes)
        f.write(("\n".join(lines) + "\n").encode("utf-8"))
    with open(path, "wb") as f:
        f.write(raw.getvalue())
    return len(raw.getvalue())


if __name__ == "__main__":
    out = sweep_lines(graft.load_package())
    if "--write" in sys.argv[1:]:
        print("%d lines, %d bytes -> %s" % (len(out), write_fixture(out), FIXTURE))
    else:
        print("\n".join(out))
