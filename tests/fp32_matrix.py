"""The case table of the fp32 kernel matrix (TEST INFRASTRUCTURE; tests/test_fp32_matrix.py checks it on the CPU, tests/test_gpu_fp32_matrix.py runs
it): short models and public calls that put every instantiation of the fp32 convolution kernels -- every symbol of the built objects that matches
conv3x3_ or upconv4x4_head and is no 16-bit (split) kernel -- into a launch whose kernel names the profiler reports.

A key names one instantiation: (kernel, (template arguments...)), e.g. ("conv3x3_wino4", (128, 64, True, False, True, False)); a kernel that is no
template has ().  The template arguments, as the sources declare them:
    conv3x3_first[_batch]     <CIN, NBT = cout / 32, PLANAR (planar planes out), U8 (interleaved uint8 image in)>
    conv3x3_last[_batch]      <CIN, COUT, U8 (interleaved uint8 image out)>
    conv3x3_mfma2             <CIN, COUT, MB, NB, WM, WN, E>
    conv3x3_wino[_batch]      <CIN, COUT>
    conv3x3_wino4             <CIN, COUT, OUT_PLANAR, IN_NHWC, FUSE7 (the one-plane last layer in the epilogue), PROG (... and its gather)>
    conv3x3_wino4_batch       <CIN, COUT, FUSE7>                     (planar in and out)
    conv3x3_wino4_batch_l     <CIN, COUT, OUT_PLANAR, IN_NHWC>
    upconv4x4_head[_batch]    <CIN, NOUT, U8>
Loops the sizes here do not send round a second time: the grid-stride loops of conv3x3_last_gather_x4[_batch] (past 65536 workgroups: 67 M pixels)
and conv3x3_direct, which has none.
"""
import functools
import os
import re
import subprocess
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")
LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")

# w2xc_opts.kernel / .fusion (include/w2xc_hip.h; tests/test_fp32_matrix.py compares them with the package's)
KERNEL_AUTO, KERNEL_DIRECT, KERNEL_MFMA, KERNEL_WINOGRAD32 = 0, 1, 2, 4
FUSION_AUTO, FUSION_OFF, FUSION_PROG = 0, 1, 6


# ---------------------------------------------------------------------------------------------------------------------------------------------
# names -> keys
# ---------------------------------------------------------------------------------------------------------------------------------------------
def key_of_name(name):
    """the key of a kernel name in either spelling -- the Itanium symbol (_Z13conv3x3_wino4ILi128ELi64ELb1ELb0ELb1ELb0EEv12W2xcConvDescii; only Li and Lb
    template arguments occur) or the demangled form (void conv3x3_wino4<128, 64, true, false, true, false>(W2xcConvDesc, int, int)); None where the name
    is neither"""
    name = name.strip()
    m = re.match(r"_Z(\d+)", name)
    if m:
        n = int(m.group(1))
        base, rest = name[m.end():m.end() + n], name[m.end() + n:]
        if len(base) != n or not re.fullmatch(r"\w+", base):
            return None
        args = []
        if rest.startswith("I"):
            pos = 1
            while not rest.startswith("E", pos):
                a = re.compile(r"L([ib])(\d+)E").match(rest, pos)
                if not a:
                    return None
                args.append(bool(int(a.group(2))) if a.group(1) == "b" else int(a.group(2)))
                pos = a.end()
        return (base, tuple(args))
    m = re.match(r"(?:void\s+)?(\w+)\s*(?:<([^<>]*)>)?\s*(?:\(|$)", name)
    if not m:
        return None
    args = []
    for a in (m.group(2).split(",") if m.group(2) is not None else []):
        a = a.strip()
        if a in ("true", "false"):
            args.append(a == "true")
        elif re.fullmatch(r"\d+", a):
            args.append(int(a))
        else:
            return None
    return (m.group(1), tuple(args))


def is_fp32_conv(kernel):
    """the kernels of the matrix, by name (symbol, demangled name or the kernel name of a key)"""
    return re.search(r"conv3x3_|upconv4x4_head", kernel) is not None and "split" not in kernel


def kernel_objects():
    """the objects csrc/Makefile builds from .hip sources: the OBJ line (with its continuation lines) without $(ENGINE)"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    line = re.search(r"^OBJ\s*=(.*)$", text, re.M).group(1)
    objs = re.findall(r"\.\./lib/(\w+\.o)", line)
    assert objs and "$(ENGINE)" in line, line
    return objs


def kernel_symbols(obj):
    """the .name notes of the gfx950 code object inside a built object, as tools/kernel_resources.sh reads them"""
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, obj)], capture_output=True, text=True, check=True).stdout
    return [line.split()[0] for line in out.splitlines() if line.strip()]


@functools.lru_cache(maxsize=None)
def built_symbols():
    return tuple(s for o in kernel_objects() for s in kernel_symbols(o) if is_fp32_conv(s))


def built_keys():
    """the key of every fp32 convolution kernel in the built objects"""
    return {key_of_name(s) for s in built_symbols()}


def kernel_names(run):
    """the names of the device kernels `run` launches, in order (torch's profiler listens to the HIP runtime, whoever launches).
    `run` is the profiler's one active step behind a warm-up step with a kernel of its own: tracing that has only just been switched on has been
    seen to miss the first launches of its window (a whole library call, with the torch kernels behind it reported), and the warm-up step is the
    profiler's own means against that -- its events are discarded."""
    import torch
    from torch.profiler import profile, schedule, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], schedule=schedule(wait=0, warmup=1, active=1, repeat=1)) as prof:
        torch.zeros(64, device="cuda").add_(1.0)
        torch.cuda.synchronize()
        prof.step()
        run()
        torch.cuda.synchronize()
        prof.step()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]


def launched_keys(names):
    """the fp32 convolution keys among profiler names; a name of the matrix's kernels that does not parse is an error"""
    keys = set()
    for n in names:
        if is_fp32_conv(n):
            k = key_of_name(n)
            assert k is not None, "unparsed kernel name %r" % n
            keys.add(k)
    return keys


# ---------------------------------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------------------------------
DIRECT = ("conv3x3_direct", ())
FIRST2, FIRST2_B = ("conv3x3_first2_wino4", ()), ("conv3x3_first2_wino4_batch", ())
GATHER, GATHER4, GATHER4_B = ("conv3x3_last_gather", ()), ("conv3x3_last_gather_x4", ()), ("conv3x3_last_gather_x4_batch", ())
MID = (32, 64, 128)
WIDE = (64, 128)
HEAD_C = (32, 64, 128, 256)
# conv3x3_mfma2: the tile shape w2xc_launch_conv picks per (cin, cout) -- MB, NB, WM, WN (w2xc_kernels.hip: 8 waves wherever cout >= 64), E = 1
MFMA_TILE = {32: (2, 1, 4, 1), 64: (2, 1, 4, 2), 128: (2, 2, 4, 2)}
MFMA_DEAD = {64: (2, 2, 4, 1), 128: (4, 2, 2, 2)}   # the 4-wave shapes of cout 64 / 128: instantiated, never picked


def first(cin, cout, planar=False, u8=False, batch=False): return ("conv3x3_first_batch" if batch else "conv3x3_first", (cin, cout // 32, planar, u8))
def last(cin, cout, u8=False, batch=False): return ("conv3x3_last_batch" if batch else "conv3x3_last", (cin, cout, u8))
def mfma(cin, cout): return ("conv3x3_mfma2", (cin, cout) + MFMA_TILE[cout] + (1,))
def wino(cin, cout, batch=False): return ("conv3x3_wino_batch" if batch else "conv3x3_wino", (cin, cout))
def w4(cin, cout, out_planar, in_nhwc=False, fuse7=False, prog=False): return ("conv3x3_wino4", (cin, cout, out_planar, in_nhwc, fuse7, prog))
def w4b(cin, cout, fuse7=False): return ("conv3x3_wino4_batch", (cin, cout, fuse7))
def w4bl(cin, cout, out_planar, in_nhwc): return ("conv3x3_wino4_batch_l", (cin, cout, out_planar, in_nhwc))
def head(cin, nout, u8=False, batch=False): return ("upconv4x4_head_batch" if batch else "upconv4x4_head", (cin, nout, u8))


def family_of(kernel):
    """the name w2xc_layer_kernel_name gives the layer a kernel runs"""
    base = re.sub(r"(_x4)?(_batch(_l)?)?$", "", kernel)
    return "conv3x3_mfma" if base == "conv3x3_mfma2" else base


# Instantiations no public call launches, each with the condition that keeps it out (file:line of this commit's sources).
_PLANAR32 = ("w2xc_select.cpp:163 resolve_chain(), the layouts: `else if (c.layer[l + 1].wino4) planar = hl[l + 1].nin != 32;` -- a first layer writes planar "
             "planes only for a conv3x3_wino4 consumer with 64 / 128 input planes, so a 32-plane first layer always writes NHWC (and Model::filter goes "
             "through NHWC: w2xc_filter.cpp:35 `writes_nhwc = (kind == W2XC_K_MFMA || kind == W2XC_K_FIRST)`)")
_W8 = ("w2xc_kernels.hip:512 w2xc_launch_conv(): `const bool w8 = d.cout >= 64;` and the cases of cout 64 / 128 choose `w8 ? <8-wave shape> : <this one>`: "
       "w8 is true in every one of them")
UNREACHABLE = {("conv3x3_mfma2", (cin, cout) + MFMA_DEAD[cout] + (1,)): _W8 for cin in MID for cout in WIDE}
UNREACHABLE.update({
    first(1, 32, planar=True): _PLANAR32,
    first(3, 32, planar=True): _PLANAR32,
    first(3, 32, planar=True, u8=True): _PLANAR32,
    first(3, 32, planar=True, batch=True): _PLANAR32,
    first(3, 32, planar=True, u8=True, batch=True): _PLANAR32,
    GATHER: ("w2xc_split.hip:1034 w2xc_launch_last_gather(): `if (d.in_ps <= 1 && d.out_ps == 1)` launches conv3x3_last_gather_x4 -- layer_desc "
             "(w2xc_select.cpp:417) gives every fused-last producer `d.out_ps = 1`, and the gather's layer is always last_direct "
             "(w2xc_select.cpp:315-316: its one plane goes to the caller's plane, `d.out_ps = 1`, w2xc_select.cpp:408)"),
})

# ---------------------------------------------------------------------------------------------------------------------------------------------
# sizes and the grid rules
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (h, w).  Layer k of n computes (h + 2 (n - k)) x (w + 2 (n - k)) pixels, so the tile edges move per layer.
#   1x1     every tile is an edge tile in both directions
#   4x4     the smallest plane conv3x3_wino4 PROG runs on (w2xc_rows.cpp:204 prog_eligible(): `P.w >= 4`): stands in for 1x1 in the PROG cases
#   17x33   one row and one column past a tile edge at the output, ragged pixel quads
#   tall    one tile column, >= 258 tile rows at 16-row tiles: more items than the 256 workgroups of w2xc_persistent_grid, every workgroup walks on
#   tall4   the same four pixels wide, for the PROG cases
#   wide    one tile row, >= 258 tile columns: the same through the other coordinate of the tile decode
#   xwide   one tile row of 514 tile columns: more than the 512 workgroups conv3x3_first2_wino4 gets (two per CU)
#   strip   tests/test_gpu_upconv.py's STRIP: one row of 514 head tiles for the 512 workgroups of w2xc_upconv_grid
SIZES = {"1x1": (1, 1), "4x4": (4, 4), "17x33": (17, 33), "tall": (4120, 3), "tall4": (4120, 4), "wide": (3, 8230), "xwide": (3, 32 * 513 + 1), "strip": (8, 32 * 513 + 1)}
SMALL, SMALL_PROG = ("1x1", "17x33"), ("4x4", "17x33")
SECOND_TRIP = ("tall", "tall4", "wide", "xwide", "strip")
FIRST_TPW = LAST_TPW = 4   # tiles a workgroup of conv3x3_first / conv3x3_last walks (w2xc_kernels.hip, w2xc_conv_batch.hip)


def persistent_grid(items, per_cu=1):
    """w2xc_persistent_grid (w2xc_launch.hpp)"""
    return min(per_cu * 256, (items + 7) & ~7)


def upconv_grid(ntiles):
    """w2xc_upconv_grid (w2xc_pack.cpp)"""
    return min(ntiles, 512)


def launch_shape(kernel, cout, out_h, out_w, py=0, batch=1):
    """(items, workgroups) of a launch of `kernel` (a family name, or a batch form's) over out_h x out_w pixels whose first row is py rows into a Winograd
    block, for `batch` images: the launchers' arithmetic (launch_wino4[_batch], launch_wino, launch_mfma2, launch_first / launch_last /
    launch_tiles_batch, w2xc_launch_first2_wino4[_batch], launch_upconv[_batch])"""
    tx = -(-out_w // 32)
    fam = family_of(kernel)
    if fam == "conv3x3_wino4":
        items = tx * ((out_h + (py & 3) + 15) // 16) * (cout // 64) * batch
        return items, persistent_grid(items)
    if fam == "conv3x3_wino":
        items = tx * ((out_h + (py & 1) + 15) // 16) * (cout // 32) * batch
        return items, persistent_grid(items)
    if fam == "conv3x3_mfma":
        items = tx * -(-out_h // 8)
        return items, persistent_grid(items)
    if fam in ("conv3x3_first", "conv3x3_last"):
        items = tx * -(-out_h // 8) * batch
        return items, -(-items // FIRST_TPW)
    if fam == "conv3x3_first2_wino4":
        items = tx * ((out_h + (py & 3) + 7) // 8) * batch
        return items, persistent_grid(items, 2)
    if fam == "upconv4x4_head":
        items = tx * -(-out_h // 8) * batch
        return items, upconv_grid(items)
    raise ValueError(kernel)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
# id; family: the kernel family the case is there for (the per-family error figures of tests/test_gpu_fp32_matrix.py); entry: the public call --
#   plane         _ModelSet.convert_device                          one plane in, one out
#   planes        _ModelSet.convert_planes_device                   n planes in, every plane of the last layer out
#   up2x          _ModelSet.convert_planes_up2x_device              a head model
#   *_batch       convert_batch_device / convert_planes_batch_device / convert_planes_up2x_batch_device on `batch` images
#   rgb_u8        process_image_rgb_u8_device: the model as noise model -- a head model: as scale model, one iteration -- on a uint8 image
#   rgb_u8_batch  process_image_rgb_u8_batch_device / process_image_rgb_u8_up2x_batch_device on `batch` images
#   rgba_u8       process_image_rgba_u8_up2x_batch_device on `batch` RGBA images (1: the single-image launches), a head model as scale model
#   rgba_u8_tta   ... its TTA form on one image: the 8 variants are the images of a batch, the alpha head has the float sink
# The host calls (_ModelSet.convert, .filter) are no entries: they launch through the same layer_kind / launch_layer as the device calls, in row chunks
# (and PROG through the host hooks: the keys of the W2XC_FUSION_PROG cases), so they reach no key of their own; nor is band_rows a field of a case -- a
# banded run launches the kernels of the unbanded one and is held to its bits by the parity tests of each call.
# planes: of the 3x3 layers; head: planes out of an upconv head behind them, or None; opts: w2xc_opts fields; sizes: names of SIZES;
# keys: the exact set of fp32 convolution keys the call launches; layer_names: w2xc_layer_kernel_name per layer with these options;
# focus: (1-based layer, cout) whose launch the second-trip sizes are there for, or None
Case = namedtuple("Case", "id family entry planes head opts batch sizes keys layer_names focus")
FLOAT_SINGLE, FLOAT_BATCH = ("plane", "planes", "up2x"), ("plane_batch", "planes_batch", "up2x_batch")
U8_ENTRIES = ("rgb_u8", "rgb_u8_batch", "rgba_u8", "rgba_u8_tta")
N1 = "(in_next_layer)"


def nbt(c): return c // 32


def _cases():
    out = []

    def add(id, family, entry, planes, keys, names, head=None, opts=None, batch=1, sizes=SMALL, focus=None):
        out.append(Case(id, family, entry, tuple(planes), head, dict(opts or {}), batch, tuple(sizes), frozenset(keys), tuple(names), focus))

    def trips(narrow_wide, both=("tall", "wide")):
        return SMALL + tuple(both) if narrow_wide else SMALL

    # ---- conv3x3_direct
    add("direct", "direct", "plane", [1, 32, 1], {DIRECT}, ["conv3x3_direct"] * 2, opts=dict(kernel=KERNEL_DIRECT))

    # ---- w2xc_opts.kernel = MFMA / WINOGRAD32: [1, cin, cout, 1], conv3x3_first<1, .> in front and conv3x3_last<., 1> behind (no fusion with these kernels)
    for cin in MID:
        for cout in MID:
            ends = (cin, cout) in ((32, 32), (128, 128))
            add("mfma2_%d_%d" % (cin, cout), "mfma2", "plane", [1, cin, cout, 1], {first(1, cin), mfma(cin, cout), last(cout, 1)},
                ["conv3x3_first", "conv3x3_mfma", "conv3x3_last"], opts=dict(kernel=KERNEL_MFMA), sizes=trips(ends), focus=(2, cout))
            add("wino_%d_%d" % (cin, cout), "wino", "plane", [1, cin, cout, 1], {first(1, cin), wino(cin, cout), last(cout, 1)},
                ["conv3x3_first", "conv3x3_wino", "conv3x3_last"], opts=dict(kernel=KERNEL_WINOGRAD32), sizes=trips(ends), focus=(2, cout))

    # ---- conv3x3_first / conv3x3_last around NHWC planes: [3, c, 3] -- float planes, uint8 images, and both as batches (one workgroup walks FIRST_TPW
    #      tiles image-major: with 3 images of 6 / 3 tiles a workgroup's run straddles two images)
    for c in MID:
        add("rgb_%d" % c, "first", "planes", [3, c, 3], {first(3, c), last(c, 3)}, ["conv3x3_first", "conv3x3_last"], focus=(1, c))
        add("rgb_%d_batch" % c, "first", "planes_batch", [3, c, 3], {first(3, c, batch=True), last(c, 3, batch=True)}, ["conv3x3_first", "conv3x3_last"],
            batch=3, focus=(1, c))
        add("rgb_%d_u8" % c, "first", "rgb_u8", [3, c, 3], {first(3, c, u8=True), last(c, 3, u8=True)}, ["conv3x3_first", "conv3x3_last"])
        add("rgb_%d_u8_batch" % c, "first", "rgb_u8_batch", [3, c, 3], {first(3, c, u8=True, batch=True), last(c, 3, u8=True, batch=True)},
            ["conv3x3_first", "conv3x3_last"], batch=3)

    # ---- conv3x3_wino4 between three-plane ends
    # [3, c1, c2, 3]: planar planes in (conv3x3_first PLANAR in front), NHWC out (conv3x3_last behind)
    for c1 in WIDE:
        for c2 in WIDE:
            ends = (c1, c2) in ((64, 64), (128, 128))
            names = ["conv3x3_first", "conv3x3_wino4", "conv3x3_last"]
            add("w4_pn_%d_%d" % (c1, c2), "wino4", "planes", [3, c1, c2, 3], {first(3, c1, planar=True), w4(c1, c2, False), last(c2, 3)}, names,
                sizes=trips(ends), focus=(2, c2))
            add("w4_pn_%d_%d_batch" % (c1, c2), "wino4", "planes_batch", [3, c1, c2, 3],
                {first(3, c1, planar=True, batch=True), w4bl(c1, c2, False, False), last(c2, 3, batch=True)}, names, batch=3,
                sizes=SMALL + (("tall",) if ends else ()), focus=(2, c2))
        # ... the same ends on uint8 images: conv3x3_first PLANAR U8
        add("w4_pn_%d_64_u8" % c1, "first", "rgb_u8", [3, c1, 64, 3], {first(3, c1, planar=True, u8=True), w4(c1, 64, False), last(64, 3, u8=True)},
            ["conv3x3_first", "conv3x3_wino4", "conv3x3_last"])
        add("w4_pn_%d_64_u8_batch" % c1, "first", "rgb_u8_batch", [3, c1, 64, 3],
            {first(3, c1, planar=True, u8=True, batch=True), w4bl(c1, 64, False, False), last(64, 3, u8=True, batch=True)},
            ["conv3x3_first", "conv3x3_wino4", "conv3x3_last"], batch=3)
    for c in WIDE:
        # [3, 32, c, 3]: 32 NHWC planes in, NHWC out
        names = ["conv3x3_first", "conv3x3_wino4", "conv3x3_last"]
        add("w4_nn_32_%d" % c, "wino4", "planes", [3, 32, c, 3], {first(3, 32), w4(32, c, False, True), last(c, 3)}, names, sizes=trips(True), focus=(2, c))
        add("w4_nn_32_%d_batch" % c, "wino4", "planes_batch", [3, 32, c, 3], {first(3, 32, batch=True), w4bl(32, c, False, True), last(c, 3, batch=True)}, names,
            batch=3, sizes=SMALL + ("tall",), focus=(2, c))
        # [3, 32, c, 64, 3]: 32 NHWC planes in, planar out (a conv3x3_wino4 layer with c planes in behind)
        names = ["conv3x3_first", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_last"]
        add("w4_np_32_%d" % c, "wino4", "planes", [3, 32, c, 64, 3], {first(3, 32), w4(32, c, True, True), w4(c, 64, False), last(64, 3)}, names,
            sizes=trips(True), focus=(2, c))
        add("w4_np_32_%d_batch" % c, "wino4", "planes_batch", [3, 32, c, 64, 3],
            {first(3, 32, batch=True), w4bl(32, c, True, True), w4bl(c, 64, False, False), last(64, 3, batch=True)}, names, batch=3,
            sizes=SMALL + ("tall",), focus=(2, c))
    # [3, c, 32, 3]: W2XC_KERNEL_AUTO sends a layer with 32 planes out to conv3x3_wino; its batch form
    for c in MID:
        add("wino_%d_32_batch" % c, "wino", "planes_batch", [3, c, 32, 3], {first(3, c, batch=True), wino(c, 32, batch=True), last(32, 3, batch=True)},
            ["conv3x3_first", "conv3x3_wino", "conv3x3_last"], batch=3, sizes=SMALL + (("tall",) if c != 64 else ()), focus=(2, 32))

    # ---- the one-plane chains: the fused last layer (FUSE7), its gather, PROG, conv3x3_first2_wino4
    for c1 in WIDE:
        for c2 in WIDE:
            ends = (c1, c2) in ((64, 64), (128, 128))
            # [1, c1, c2, 1]: layer 2 carries the last layer's taps; conv3x3_last_gather_x4 finishes, or -- W2XC_FUSION_PROG -- the launch itself
            add("w4_f7_%d_%d" % (c1, c2), "wino4", "plane", [1, c1, c2, 1], {first(1, c1, planar=True), w4(c1, c2, True, False, True), GATHER4},
                ["conv3x3_first", "conv3x3_wino4", "conv3x3_last_gather"], sizes=trips(ends), focus=(2, c2))
            add("w4_prog_%d_%d" % (c1, c2), "wino4", "plane", [1, c1, c2, 1], {first(1, c1, planar=True), w4(c1, c2, True, False, True, True)},
                ["conv3x3_first", "conv3x3_wino4", "(in_previous_layer)"], opts=dict(fusion=FUSION_PROG), sizes=SMALL_PROG + (("tall4", "wide") if ends else ()),
                focus=(2, c2))
            # [1, c1, c2, 64, 1]: planar in and out
            add("w4_pp_%d_%d" % (c1, c2), "wino4", "plane", [1, c1, c2, 64, 1],
                {first(1, c1, planar=True), w4(c1, c2, True), w4(c2, 64, True, False, True), GATHER4},
                ["conv3x3_first", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_last_gather"], sizes=trips(ends), focus=(2, c2))
            # the batched chain: [1, 32, 32, c1, c2, 1] (FUSE7 batch form), [1, 32, 32, c1, c2, 64, 1] (planar in and out)
            add("y_f7_%d_%d_batch" % (c1, c2), "wino4", "plane_batch", [1, 32, 32, c1, c2, 1], {FIRST2_B, w4b(32, c1), w4b(c1, c2, True), GATHER4_B},
                [N1, "conv3x3_first2_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_last_gather"], batch=3,
                sizes=SMALL + (("tall",) if ends else ()), focus=(4, c2))
            add("y_pp_%d_%d_batch" % (c1, c2), "wino4", "plane_batch", [1, 32, 32, c1, c2, 64, 1],
                {FIRST2_B, w4b(32, c1), w4b(c1, c2), w4b(c2, 64, True), GATHER4_B},
                [N1, "conv3x3_first2_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_last_gather"], batch=3,
                sizes=SMALL + (("tall",) if ends else ()), focus=(4, c2))
    for c in WIDE:
        # [1, 32, c, 1]: FUSE7 on 32 NHWC planes (conv3x3_first writes them)
        add("w4_f7_32_%d" % c, "wino4", "plane", [1, 32, c, 1], {first(1, 32), w4(32, c, True, True, True), GATHER4},
            ["conv3x3_first", "conv3x3_wino4", "conv3x3_last_gather"], sizes=trips(True), focus=(2, c))
        # [1, 32, c, 64, 1]: 32 NHWC planes in, planar out, in a one-plane chain
        add("y_np_32_%d" % c, "wino4", "plane", [1, 32, c, 64, 1], {first(1, 32), w4(32, c, True, True), w4(c, 64, True, False, True), GATHER4},
            ["conv3x3_first", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_last_gather"])
        # [1, 32, 32, c, 64, 1]: conv3x3_first2_wino4 writes 32 planar planes: conv3x3_wino4<32, c> planar in and out
        add("first2_pp_%d" % c, "first2", "plane", [1, 32, 32, c, 64, 1], {FIRST2, w4(32, c, True), w4(c, 64, True, False, True), GATHER4},
            [N1, "conv3x3_first2_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_last_gather"],
            sizes=SMALL + (("tall", "xwide") if c == 64 else ()), focus=(2, 32))
        # [1, 32, 32, c, 32, 1]: ... and NHWC out (conv3x3_wino<c, 32> behind), conv3x3_last<32, 1> unfused
        add("first2_pn_%d" % c, "wino4", "plane", [1, 32, 32, c, 32, 1], {FIRST2, w4(32, c, False), wino(c, 32), last(32, 1)},
            [N1, "conv3x3_first2_wino4", "conv3x3_wino4", "conv3x3_wino", "conv3x3_last"], sizes=trips(True), focus=(3, c))
    add("first2_batch", "first2", "plane_batch", [1, 32, 32, 64, 64, 1], {FIRST2_B, w4b(32, 64), w4b(64, 64, True), GATHER4_B},
        [N1, "conv3x3_first2_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_last_gather"], batch=2, sizes=("tall",), focus=(2, 32))

    # ---- upconv head models: [3, c] + head (c = 256: [3, 128, 256], the 128 -> 256 layer on conv3x3_wino4), one- and three-plane heads
    for c in HEAD_C:
        wide = c == 256
        for nin in (3, 1):
            nout = nin
            planes = [nin, 128, 256] if wide else [nin, c]
            names = (["conv3x3_first", "conv3x3_wino4"] if wide else ["conv3x3_first"]) + ["upconv4x4_head"]

            def chain(batch=False, u8=False, nin=nin, wide=wide, c=c):
                if wide:
                    return {first(nin, 128, planar=True, u8=u8, batch=batch), w4bl(128, 256, False, False) if batch else w4(128, 256, False)}
                return {first(nin, c, u8=u8, batch=batch)}
            add("head_%d_%d" % (c, nout), "upconv", "up2x", planes, chain() | {head(c, nout)}, names, head=nout,
                sizes=SMALL + (("strip",) if (c, nout) == (32, 1) else ()), focus=(len(planes), nout))
            if nin == 1:
                continue
            add("head_%d_3_batch" % c, "upconv", "up2x_batch", planes, chain(batch=True) | {head(c, 3, batch=True)}, names, head=3, batch=3,
                sizes=SMALL + (("strip",) if c in (32, 256) else ()), focus=(len(planes), 3))
            add("head_%d_3_u8" % c, "upconv", "rgb_u8", planes, chain(u8=True) | {head(c, 3, True)}, names, head=3,
                sizes=SMALL + (("strip",) if c == 32 else ()), focus=(len(planes), 3))
            add("head_%d_3_u8_batch" % c, "upconv", "rgb_u8_batch", planes, chain(batch=True, u8=True) | {head(c, 3, True, batch=True)}, names, head=3, batch=3)
            # the RGBA calls: the colour pass and the alpha pass (the alpha byte as three planes, channel 1 of the head alone)
            add("head_%d_rgba" % c, "upconv", "rgba_u8", planes, chain(u8=True) | {head(c, 3, True), head(c, 1, True)}, names, head=3)
            add("head_%d_rgba_batch" % c, "upconv", "rgba_u8", planes, chain(batch=True, u8=True) | {head(c, 3, True, batch=True), head(c, 1, True, batch=True)},
                names, head=3, batch=3)
            add("head_%d_rgba_tta" % c, "upconv", "rgba_u8_tta", planes, chain(batch=True) | {head(c, 3, batch=True), head(c, 1, batch=True)}, names, head=3)
    # the head's own second trip: one tile row of 514 tiles; c = 256 behind conv3x3_direct (3 -> 256 has no fast kernel), the float64 reference of the
    # 128 -> 256 layer on that strip would take a minute
    add("head_32_strip", "upconv", "up2x", [3, 32], {first(3, 32), head(32, 3)}, ["conv3x3_first", "upconv4x4_head"], head=3, sizes=("strip",), focus=(2, 3))
    add("head_256_strip", "upconv", "up2x", [3, 256], {DIRECT, head(256, 3)}, ["conv3x3_direct", "upconv4x4_head"], head=3, sizes=("strip",), focus=(2, 3))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def covered_keys():
    keys = set()
    for c in CASES:
        keys |= c.keys
    return keys


def n_layers(case):
    return len(case.planes) - 1 + (1 if case.head else 0)


def n_out(case):
    return case.head if case.head else case.planes[-1]


def focus_launch(case, size):
    """(kernel family, items, workgroups) of the launch a second-trip size is there for: layer k of n computes h + 2 (n - k) rows from row -(n - k) on
    (the whole plane is one band: RowPlan::region), the head walks the source pixels"""
    k, cout = case.focus
    n = n_layers(case)
    h, w = SIZES[size]
    name = case.layer_names[k - 1]
    grow = 0 if name == "upconv4x4_head" else 2 * (n - k)
    items, grid = launch_shape(name, cout, h + grow, w + grow, py=(-(n - k)) & 3, batch=case.batch)
    return name, items, grid


# ---------------------------------------------------------------------------------------------------------------------------------------------
# models, inputs, float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------------
def seed_of(case):
    return 2300 + CASES.index(case)


def model_arrays(case, seed):
    """(layers, head or None) of tools/gen_model.py's seeded weights"""
    from tools import gen_model
    layers = gen_model.synth_layers(list(case.planes), seed)
    return layers, (gen_model.synth_head(case.planes[-1], case.head, seed) if case.head else None)


def source_of(case, size, seed, image=0):
    """image `image` of the case's input at a size: float planes [nin, h, w] in [0, 1), or -- the uint8 entries -- an image [h, w, 3 or 4]"""
    h, w = SIZES[size]
    rng = np.random.default_rng(40 + 7 * h + w + seed + 1000003 * image)
    if case.entry in U8_ENTRIES:
        img = rng.integers(0, 256, (h, w, 4 if case.entry.startswith("rgba") else 3)).astype(np.uint8)
        if img.shape[2] == 4 and h * w > 1:
            img[:max(1, h // 3), :max(1, w // 3), 3] = 0       # a transparent block for the bleed, an opaque one
            img[h - max(1, h // 4):, w - max(1, w // 4):, 3] = 255
        return img
    return rng.random((case.planes[0], h, w), dtype=np.float32)


def float_planes(img):
    """x = u8 / 255 as the image calls form it, (float)byte * (float)(1.0 / 255.0): [3, h, w] of an [h, w, 3] image"""
    return np.ascontiguousarray((img.astype(np.float32) * np.float32(1.0 / 255.0)).transpose(2, 0, 1))


def to_u8(v):
    """saturate(rint(255 v)) as the image calls round: the fp32 product, half to even"""
    return np.clip(np.rint(np.asarray(v, np.float32) * np.float32(255.0)), 0, 255).astype(np.uint8)


def reference(layers, head, x):
    """(float64 result of the model on x [nin, h, w], the largest |activation| its last layer reads).  3x3 chains: upconv_ref.chain_z, cropped by the
    valid convolutions themselves (padding = the layer count); head models: upconv_ref.reference; one plane in and out: the oracle's float64
    restatement of convertWithModels (oracle.Oracle.convert_f64)."""
    import upconv_ref as ur
    if head is not None:
        z = ur.chain_z(layers, x, len(layers) + 1)
        return ur.reference(layers, head, x), float(z.abs().max())
    n = len(layers)
    z = ur.chain_z(layers[:-1], x, n) if n > 1 else None
    reads = float(z.abs().max()) if n > 1 else float(np.abs(x).max())
    if layers[0][0] == 1 and layers[-1][1] == 1:
        from oracle import oracle as orc
        return orc.Oracle(layers).convert_f64(x[0])[None], reads
    return ur.chain_z(layers, x, n).numpy(), reads


@functools.lru_cache(maxsize=None)
def conditioned(case_id, size, tries=32):
    """(seed, layers, head, source, float64 reference) of a case at a size -- the rule of split_matrix.model_plane_reference: the first of a fixed seed
    sequence whose REFERENCE output range is at least 1/8 of the largest activation the last layer reads (a 1x1 plane has one output value per plane;
    where it is a near-cancellation, "error over range" is the error times the cancellation factor, whatever computes it).  The uint8 entries round
    the result to bytes, so there the reference must also leave a tenth of the values (one value of a 1x1 plane) strictly inside (0, 1): an image of
    saturated bytes would compare nothing.  The choice looks at the reference only, never at a GPU result.  The source is image 0 of the case; the
    reference of a uint8 entry is that of the colour planes u8 / 255."""
    case = BY_ID[case_id]
    for k in range(tries):
        seed = seed_of(case) + 100 * k
        layers, head = model_arrays(case, seed)
        src = source_of(case, size, seed)
        x = float_planes(src[:, :, :3]) if case.entry in U8_ENTRIES else src
        ref, reads = reference(layers, head, x)
        if float(np.abs(ref).max()) < reads / 8:
            continue
        if case.entry in U8_ENTRIES:
            inside = (ref > 0) & (ref < 1)
            if inside.mean() < 0.1 and not (ref.size <= 12 and inside.any()):
                continue
        ref.setflags(write=False)
        return seed, layers, head, src, ref
    raise AssertionError("no well-conditioned weights and source in %d seeds: %s %s" % (tries, case_id, size))
