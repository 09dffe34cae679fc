"""Byte offsets past 2^31 and 2^32 inside ONE layer's activation buffer (TEST INFRASTRUCTURE: tests/test_plan_limits.py holds the plans to the launchers'
limits with the arithmetic here, tests/test_gpu_far_offsets.py runs the case table, tests/test_far_offsets.py checks table and checker on the CPU).
This module imports neither torch nor the library.

Three parts:
* the launchers' 32-bit rules and the strides of a plan's launches, restated as plain integer arithmetic, each with the source line it restates (QUOTES);
* the case table: the smallest planes at which a kernel family's buffer crosses 2^31 / 2^32 bytes, and the rows at which it does;
* the checker: float64 references of 48 x 48 windows computed from a crop, and the comparison of a plane with its banded twin and those windows.

Left out, covered by the arithmetic of tests/test_plan_limits.py only: conv3x3_wino4's planar-input lane offsets above 2^31 (planes of 683 MiB x 64
planes, about 43 GiB per buffer) and PROG's tap-plane rule (a band of 2^30 pixels)."""
import collections
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")

TWO31, TWO32, GIB = 1 << 31, 1 << 32, 1 << 30
# w2xc_opts fields (include/w2xc_hip.h; tests/test_far_offsets.py compares them with the package's)
KERNEL_AUTO, KERNEL_DIRECT, KERNEL_MFMA, KERNEL_WINOGRAD32, KERNEL_WINOGRAD4 = 0, 1, 2, 4, 5
FUSION_AUTO, FUSION_OFF, FUSION_LAST, FUSION_GATHER_LAUNCH, FUSION_PROG = 0, 1, 4, 5, 6
PRECISION = {"fp32": 0, "bf16": 1, "bf16x2": 2, "bf16x3": 3, "fp16x2": 4}
TERMS = {"bf16": 1, "bf16x2": 2, "bf16x3": 3, "fp16x2": 2}
FIRST2, WINO4, GATHER, IN_NEXT, IN_PREV, HEAD, DIRECT = ("conv3x3_first2_wino4", "conv3x3_wino4", "conv3x3_last_gather", "(in_next_layer)", "(in_previous_layer)",
                                                         "upconv4x4_head", "conv3x3_direct")

# (file, line, text that line holds): what the arithmetic below restates.  tests/test_far_offsets.py reads the lines, so a moved one shows.
QUOTES = [
    ("w2xc_wino4.hip", 378, "if (24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_wino4.hip", 381, "if (3 * d.in_cs * 4 + 24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_wino4.hip", 511, "if (24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_wino4.hip", 514, "if (3 * d.in_cs * 4 + 24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_wino4.hip", 523, "if (3 * d.in_cs * 4 + 24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_first2_wino4.hip", 87, "if (12ll * d.out_cs * 4 + ((long long)d.out_h + 8) * d.out_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_first2_wino4.hip", 109, "if (12ll * d.out_cs * 4 + ((long long)d.out_h + 8) * d.out_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_wino4.hip", 290, "(long long)d.out_h * d.out_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;"),
    ("w2xc_rows.cpp", 204, "(long long)d.out_h * d.out_rs * 4 < (1ll << 32) &&"),
    ("w2xc_wino4.hip", 282, "const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 3) + 15) / 16;"),
    ("w2xc_wino4.hip", 283, "const long long items = (long long)tiles_x * tiles_y * (COUT / 64);"),
    ("w2xc_wino4.hip", 284, "if (items >= (1ll << 31)) return hipErrorInvalidValue;"),
    ("w2xc_wino4.hip", 418, "if (items * b.batch >= (1ll << 31)) return hipErrorInvalidValue;"),
    ("w2xc_wino4.hip", 436, "if (items * b.batch >= (1ll << 31)) return hipErrorInvalidValue;"),
    ("w2xc_first2_wino4.hip", 88, "const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 3) + 7) / 8;"),
    ("w2xc_first2_wino4.hip", 112, "if (items * b.batch >= (1ll << 31)) return hipErrorInvalidValue;"),
    # the layouts between layers (resolve_chain, pass 7) and the strides (layer_desc)
    ("w2xc_select.cpp", 162, "if (c.layer[l].kind == W2XC_K_FIRST2_WINO4) planar = true;"),
    ("w2xc_select.cpp", 163, "else if (c.layer[l + 1].wino4) planar = hl[l + 1].nin != 32;"),
    ("w2xc_select.cpp", 164, "else if (c.layer[l].wino4) planar = c.layer[l + 1].kind == W2XC_K_DIRECT;"),
    ("w2xc_select.cpp", 173, "c.prog_gather = T == 0 && c.fused_last && o.fusion != W2XC_FUSION_GATHER_LAUNCH && w2xc_wino4_prog_supported(hl[n - 2].nin, hl[n - 2].nout) &&"),
]


def ru32(v):
    return (v + 31) & ~31


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a plan's launches
# ---------------------------------------------------------------------------------------------------------------------------------------------
# layer k (1-based) of a band: the rows [top, top + out_h) x out_w pixels it computes and the buffer it writes -- kind "planar" (cout planes of out_cs
# floats, rows of out_rs), "nhwc" (rows of out_rs = out_w x cout floats), "taps" (the halves x 9 partial tap planes of a fused last layer), "terms" (the
# 16-bit term planes of the split pipeline) or "out" (the caller's planes); bytes = the size of that buffer
Launch = collections.namedtuple("Launch", "k name cin cout top out_h out_w kind out_rs out_cs bytes")


def planar_outs(names, nin):
    """resolve_chain's pass 7 on the kernel names of the fp32 path: is the output of layer l (0-based) planar"""
    n = len(names)
    planar = [False] * n
    for l in range(n - 1):
        if names[l] == FIRST2:
            planar[l] = True
        elif names[l + 1] == WINO4:
            planar[l] = nin[l + 1] != 32
        elif names[l] == WINO4:
            planar[l] = names[l + 1] == DIRECT
    return planar


def launches(names, io, w, regions, fusion=FUSION_AUTO, terms=0):
    """the launches of one band: names per layer (w2xc_layer_kernel_name), io = [(nin, nout)] per layer, regions = [(top, bottom)] per layer
    (w2xc_plan_region), the call's w2xc_opts.fusion; terms: 16-bit terms per activation of the split pipeline (0: fp32).  Strides as layer_desc forms
    them: planar out_rs = (out_w + 31) & ~31, out_cs = out_rs x out_h; NHWC out_rs = out_w x nout."""
    n = len(names)
    planar = planar_outs(names, [a for a, _ in io]) if terms == 0 else [False] * n
    fused_last = names[-1] in (GATHER, IN_PREV)
    prog_gather = (terms == 0 and fused_last and fusion != FUSION_GATHER_LAUNCH and n >= 3 and io[n - 2][0] in (64, 128) and io[n - 2][1] in (64, 128) and
                   planar[n - 3])
    out = []
    for k in range(1, n + 1):
        (cin, cout), (top, bottom) = io[k - 1], regions[k - 1]
        out_h, out_w = bottom - top, w + 2 * (n - k)
        if names[k - 1] == IN_NEXT:
            out.append(Launch(k, names[k - 1], cin, cout, top, out_h, out_w, "none", 0, 0, 0))
        elif k == n:
            out.append(Launch(k, names[k - 1], cin, cout, top, out_h, out_w, "out", 0, 0, 0))
        elif k == n - 1 and fused_last:
            halves = cout // 64 if terms == 0 else None   # (16-bit: w2xc_split_halves; the tap planes are not what these tests mean)
            rs = ru32(out_w) if prog_gather else out_w
            out.append(Launch(k, names[k - 1], cin, cout, top, out_h, out_w, "taps", rs, rs * out_h, (halves or 0) * 9 * rs * out_h * 4))
        elif terms and names[k] == "conv3x3_split":
            out.append(Launch(k, names[k - 1], cin, cout, top, out_h, out_w, "terms", out_w * 16, 0, terms * out_h * out_w * cout * 2))
        elif planar[k - 1]:
            rs = ru32(out_w)
            out.append(Launch(k, names[k - 1], cin, cout, top, out_h, out_w, "planar", rs, rs * out_h, cout * rs * out_h * 4))
        else:
            out.append(Launch(k, names[k - 1], cin, cout, top, out_h, out_w, "nhwc", out_w * cout, 1, out_h * out_w * cout * 4))
    return out


def violations(ls, batch=1):
    """the launcher rules a band's launches break (fp32 path): [(layer, rule, value)] -- every entry is a launch that comes back hipErrorInvalidValue"""
    bad = []
    for L in ls:
        if L.name == WINO4:
            src = ls[L.k - 2]
            if src.name == IN_NEXT:
                src = None
            if src is not None and src.kind == "planar":
                v = 3 * src.out_cs * 4 + 24 * src.out_rs * 4          # w2xc_wino4.hip:381,514,523
                if v >= TWO32:
                    bad.append((L.k, "3 in_cs 4 + 24 in_rs 4 < 2^32", v))
            elif src is not None and src.kind == "nhwc" and L.cin == 32:
                v = 24 * src.out_rs * 4                               # w2xc_wino4.hip:378,511
                if v >= TWO32:
                    bad.append((L.k, "24 in_rs 4 < 2^32", v))
            items = ((L.out_w + 31) // 32) * ((L.out_h + (L.top & 3) + 15) // 16) * (L.cout // 64)   # w2xc_wino4.hip:282-284, :418, :436
            if items * batch >= TWO31:
                bad.append((L.k, "items x batch < 2^31", items * batch))
        elif L.name == FIRST2:
            v = 12 * L.out_cs * 4 + (L.out_h + 8) * L.out_rs * 4       # w2xc_first2_wino4.hip:87,109
            if v >= TWO32:
                bad.append((L.k, "12 out_cs 4 + (out_h + 8) out_rs 4 < 2^32", v))
            items = ((L.out_w + 31) // 32) * ((L.out_h + (L.top & 3) + 7) // 8)                       # w2xc_first2_wino4.hip:88, :112
            if items * batch >= TWO31:
                bad.append((L.k, "items x batch < 2^31", items * batch))
    return bad


def prog_finishes(L):
    """PROG's rule (w2xc_wino4.hip:290) on the tap planes of launch L.  No plan can break it: prog_eligible (w2xc_rows.cpp:204) asks the same question
    first and leaves a band that fails it to the gather launch, which is bit-identical."""
    return L.kind == "taps" and L.out_h * L.out_rs * 4 < TWO32


def first2_lane_offset(L):
    """the largest 32-bit lane offset conv3x3_first2_wino4 forms over its output planes (the left side of its launcher's rule)"""
    return 12 * L.out_cs * 4 + (L.out_h + 8) * L.out_rs * 4


def crossing(L, threshold):
    """(plane row, column) of the pixel of launch L's buffer whose bytes hold byte offset `threshold`; None where the buffer ends below it.  A planar
    buffer crosses inside some plane c: every output pixel sums all planes, so the row is what places the window."""
    if L.bytes <= threshold:
        return None
    if L.kind == "planar":
        inside = threshold % (L.out_cs * 4)
        return L.top + inside // (L.out_rs * 4), min(L.out_w - 1, (inside % (L.out_rs * 4)) // 4)
    if L.kind == "nhwc":
        return L.top + threshold // (L.out_rs * 4), (threshold % (L.out_rs * 4)) // (L.cout * 4)
    if L.kind == "terms":   # [term][16-plane group][y][x][16] of 2-byte values: inside one group's plane
        inside = threshold % (L.out_h * L.out_w * 32)
        return L.top + inside // (L.out_w * 32), (inside % (L.out_w * 32)) // 32
    raise ValueError(L.kind)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
# id; planes: of the 3x3 layers; head: output planes of an upconv head or 0; opts: w2xc_opts fields; mode: "fp32" or a 16-bit precision; size: (h, w);
# entry: "plane" (_ModelSet.convert_device), "host" (_ModelSet.convert), "up2x" (convert_planes_up2x_device), "filter" (filter_device on `layer`);
# names: w2xc_layer_kernel_name per layer with these options; meant: the 1-based layers whose output buffers must cross `threshold` bytes;
# gates: "fp32" (conftest.RTOL / ATOL elementwise, max-norm 1e-4), "f4x4" (that and the project's 4e-5) or a key of SPLIT_BOUND; layer: for "filter"
FarCase = collections.namedtuple("FarCase", "id planes head opts mode size entry names meant threshold gates layer")
H8, W8 = 2052, 4100          # 8 413 200 pixels: more than 2^23, neither side a multiple of a tile
assert H8 * W8 > 1 << 23 and H8 % 16 and W8 % 32
SPLIT_BOUND = {"bf16": 1e-2, "bf16x2": 1e-4, "bf16x3": 2e-5, "fp16x2": 2e-5}   # tests/test_gpu_split_matrix.py MAX_BOUND (bf16: and mean <= 1e-3)
F4X4_GATE = 4e-5                                                                 # tests/test_gpu_fp32_matrix.py
WIN = 48


def split_size(mode):
    """the smallest plane of the aspect of 2052 x 4100 (w = 2 h - 4) at which layer 1's term planes of [1, 128, 128, 1] -- T terms x 128 planes x 2 bytes
    over (h + 4) x (w + 4) pixels (RowPlan::ws_need: one halo row per layer, two layers behind) -- exceed 2^32 bytes"""
    T = TERMS[mode]
    h = 8
    while (h + 4) * (2 * h - 4 + 4) * 128 * 2 * T <= TWO32:
        h += 1
    return h, 2 * h - 4


def first2_height(w=8192, n=5):
    """the smallest height at which conv3x3_first2_wino4's lane offsets over a plane `w` wide pass 2^31: its region is h + 2 (n - 2) rows of
    roundup32(w + 2 (n - 2)) floats"""
    rs = ru32(w + 2 * (n - 2))
    h = 8
    while 12 * rs * (h + 2 * (n - 2)) * 4 + (h + 2 * (n - 2) + 8) * rs * 4 <= TWO31:
        h += 1
    return h


def _cases():
    F, M, W, L, W4, G = "conv3x3_first", "conv3x3_mfma", "conv3x3_wino", "conv3x3_last", WINO4, GATHER
    c = []

    def add(id, planes, names, meant, threshold, gates, head=0, opts=None, mode="fp32", size=(H8, W8), entry="plane", layer=None):
        c.append(FarCase(id, tuple(planes), head, dict(opts or {}), mode, size, entry, tuple(names), tuple(meant), threshold, gates, layer))

    add("mfma", [1, 128, 128, 1], [F, M, L], (1, 2), TWO32, "fp32", opts=dict(kernel=KERNEL_MFMA, fusion=FUSION_OFF))
    add("wino", [1, 128, 128, 1], [F, W, L], (1, 2), TWO32, "fp32", opts=dict(kernel=KERNEL_WINOGRAD32, fusion=FUSION_OFF))
    # what W2XC_KERNEL_AUTO runs: conv3x3_first writes 128 planar planes, conv3x3_wino4 FUSE7 the tap planes, the gather finishes; the host entry
    # runs the same layers with conv3x3_wino4 PROG finishing the last layer itself (run_prog, w2xc_rows.cpp)
    add("auto_device", [1, 128, 128, 1], [F, W4, G], (1,), TWO32, "f4x4")
    add("auto_host", [1, 128, 128, 1], [F, W4, G], (1,), TWO32, "f4x4", entry="host")
    add("direct", [1, 128, 1], [DIRECT, DIRECT], (1,), TWO32, "fp32", opts=dict(kernel=KERNEL_DIRECT))
    for mode in ("bf16", "bf16x2", "bf16x3", "fp16x2"):
        add("split_" + mode, [1, 128, 128, 1], ["conv3x3_first_split", "conv3x3_split", G], (1,), TWO32, mode, mode=mode, size=split_size(mode))
    # conv3x3_first2_wino4's lane offsets past 2^31.  [1, 32, 32, 64, 64, 1] is the shortest chain that runs it with the default options (it needs a
    # conv3x3_wino4 layer behind it and, with four layers, loses to the fused last layer).  At the 64-Mi-float cap the 64 planes of layer 3 alone are
    # 17 GiB, more than a case may take: the height is the smallest that crosses 2^31 instead, and the cap itself is held on the plan (no memory)
    add("first2", [1, 32, 32, 64, 64, 1], [IN_NEXT, FIRST2, W4, W4, G], (2,), TWO31, "f4x4", size=(first2_height(), 8192))
    add("head", [3, 128, 256], [F, W4, HEAD], (2,), TWO32, "f4x4", head=3, size=(2052, 2052), entry="up2x")
    # Model::filter, 128 -> 128 on planar planes with the MFMA kernel: both repacks and both NHWC buffers of the filter cache
    add("filter", [1, 128, 128, 1], [M], (1,), TWO32, "fp32", opts=dict(kernel=KERNEL_MFMA), entry="filter", layer=1)
    return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the refusal: [1, 32, 64, 1] runs conv3x3_wino4<32, 64> on the 32 NHWC planes of conv3x3_first, rows of (w + 4) x 32 floats: 24 in_rs 4 >= 2^32
REFUSED = dict(planes=(1, 32, 64, 1), size=(4, 1398144), rule="24 in_rs 4 < 2^32")
assert 24 * (REFUSED["size"][1] + 4) * 32 * 4 >= TWO32 > 24 * (1398080 + 4) * 32 * 4
CAP_BYTES = 20 * GIB


def io_of(case):
    io = list(zip(case.planes[:-1], case.planes[1:]))
    return io + [(case.planes[-1], case.head)] if case.head else io


def filter_launch(case):
    """the NHWC buffers of the filter cache as launches: the input repacked, the output before it is repacked (w2xc_filter.cpp: nhwc[ob ^ 1], nhwc[ob])"""
    h, w = case.size
    cin, cout = io_of(case)[case.layer]
    return [Launch(1, "repack", cin, cin, 0, h, w, "nhwc", w * cin, 1, h * w * cin * 4), Launch(2, case.names[0], cin, cout, 0, h, w, "nhwc", w * cout, 1, h * w * cout * 4)]


def windows(case, ls):
    """the 48 x 48 output windows of a case, as (y0, y1, x0, x1) in SOURCE coordinates of the call (a head model's outputs are twice that): the four
    corners, and around every pixel at which a meant buffer crosses 2^31 and 2^32"""
    h, w = case.size
    s = WIN // 2 if case.head else WIN

    def clip(y, x):
        y0, x0 = max(0, min(h - s, y - s // 2)), max(0, min(w - s, x - s // 2))
        return (y0, min(h, y0 + s), x0, min(w, x0 + s))
    out = [clip(0, 0), clip(0, w), clip(h, 0), clip(h, w)]
    for k in case.meant:
        for t in (TWO31, TWO32):
            at = crossing(ls[k - 1], t)
            if at is not None:
                out.append(clip(at[0], at[1]))
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def window_reference(model, x, n, win, up=1, take=None):
    """the reference of output window win = (y0, y1, x0, x1) (source coordinates) of `model` on planes x [c, h, w]: model -- a function [c, hh, ww] ->
    [co, up hh, up ww] that continues its input by replication, n = its layer count -- runs on the edge-padded planes cropped to the window plus 2 n
    pixels a side, and those 2 n pixels are cropped off the result: the crop's own border, n pixels deep, never reaches the window.
    take(ys, xs) -> x[:, ys][:, :, xs] as a numpy array, for planes that are not one (a device tensor)."""
    y0, y1, x0, x1 = win
    c, h, w = x.shape
    ys = np.clip(np.arange(y0 - 2 * n, y1 + 2 * n), 0, h - 1)
    xs = np.clip(np.arange(x0 - 2 * n, x1 + 2 * n), 0, w - 1)
    out = np.asarray(model(np.ascontiguousarray(take(ys, xs) if take else x[:, ys][:, :, xs])), np.float64)
    m = 2 * n * up
    assert out.shape[1:] == (up * len(ys), up * len(xs)), out.shape
    return out[:, m:out.shape[1] - m, m:out.shape[2] - m]


def window_errors(got, ref, gates, rtol=1e-4, atol=1e-5):
    """(err / range, worst elementwise err / (rtol |ref| + atol), mean err / range, the bound on err / range) of one window against its float64
    reference; the range is the window's own, at most the plane's"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    scale = float(np.abs(ref).max())
    bound = {"fp32": rtol, "f4x4": F4X4_GATE}.get(gates) or SPLIT_BOUND[gates]
    return float(err.max()) / scale, float((err / (rtol * np.abs(ref) + atol)).max()), float(err.mean()) / scale, bound


def window_ok(got, ref, gates):
    if not np.isfinite(got).all():
        return False
    e, worst, mean, bound = window_errors(got, ref, gates)
    if gates in ("fp32", "f4x4"):
        return e <= bound and e <= 1e-4 and worst <= 1.0
    return e <= bound and (gates != "bf16" or mean <= 1e-3)


def check_plane(got, twin, wins, refs, gates, up=1):
    """what is wrong with result planes `got` [c, H, W]: not the bits of the banded twin, or a window outside its gate -- a list of strings, empty when
    all is well.  wins in source coordinates, refs the float64 windows."""
    bad = []
    if got.shape != twin.shape or not np.array_equal(got.view(np.uint32), twin.view(np.uint32)):
        rows = np.flatnonzero((got.view(np.uint32) != twin.view(np.uint32)).any(axis=(0, 2))) if got.shape == twin.shape else []
        bad.append("not the bits of the banded twin: %d rows differ, the first %s" % (len(rows), rows[:1]))
    for (y0, y1, x0, x1), ref in zip(wins, refs):
        g = got[:, up * y0:up * y1, up * x0:up * x1]
        if not window_ok(g, ref, gates):
            bad.append("window rows [%d,%d) columns [%d,%d): err/range %.3g, worst elementwise %.3g, mean %.3g (bound %.3g)"
                       % ((up * y0, up * y1, up * x0, up * x1) + (window_errors(g, ref, gates) if np.isfinite(g).all() else (np.inf,) * 4)))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a case against the library's own plan (w2xc: the package, ms: the case's _ModelSet; host arithmetic only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def model_arrays(case, seed=4100):
    from tools import gen_model
    layers = gen_model.synth_layers(list(case.planes), seed)
    return layers, (gen_model.synth_head(case.planes[-1], case.head, seed) if case.head else None)


def opts_kw(case, **more):
    return dict(case.opts, precision=PRECISION[case.mode], **more)


def planned(w2xc, ms, case):
    """(the row plan, the kernel name of every layer, the launches of the one band) of a case -- asserting what the case is there for: ONE band, the
    kernels the table names, and every meant buffer ending past the case's threshold"""
    h, w = case.size
    if case.entry == "filter":
        o = w2xc.make_opts(**dict(opts_kw(case), fusion=FUSION_OFF))   # (filter_on_device runs its layer with the fusions off)
        names = [ms.kernel_name(case.layer, o)]
        assert names == list(case.names), names
        ls = filter_launch(case)
        plan = None
    else:
        o = w2xc.make_opts(**opts_kw(case))
        plan = ms.plan_rows(w, h, opts=o)
        assert plan.n_bands == 1 and plan.band_rows == h, (plan.n_bands, plan.band_rows)
        names = [ms.kernel_name(l, o) for l in range(ms.n_layers)]
        assert names == list(case.names), names
        regions = [ms.plan_region(plan, h, k, 0, h) for k in range(1, ms.n_layers + 1)]
        ls = launches(names, io_of(case), w, regions, case.opts.get("fusion", FUSION_AUTO), TERMS.get(case.mode, 0))
        assert not violations(ls)
    for k in case.meant:
        assert ls[k - 1].bytes - 4 > case.threshold, (case.id, k, ls[k - 1])
    if case.id == "first2":
        assert first2_lane_offset(ls[1]) > TWO31
    return plan, names, ls


def device_bytes(case, plan, ls):
    """the device memory of a case: the engine's buffers (the plan's two workspaces; Model::filter: the two NHWC buffers) plus the test's tensors"""
    h, w = case.size
    up = 2 if case.head else 1
    if case.entry == "filter":
        cin, cout = io_of(case)[case.layer]
        return sum(l.bytes for l in ls) + (cin * h * w + cout * h * w) * 4
    nin, nout = case.planes[0], case.head or case.planes[-1]
    tensors = 0 if case.entry == "host" else nin * h * (w + 3) * 4 + nout * (up * h + 1) * (up * w + 5) * 4
    return plan.workspace_bytes[0] + plan.workspace_bytes[1] + tensors
