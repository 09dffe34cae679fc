"""The case table of the 16-bit kernel matrix (TEST INFRASTRUCTURE; tests/test_split_emulation.py checks it on the CPU,
tests/test_gpu_split_matrix.py runs it): short models that put every instantiation of conv3x3_split, conv3x3_first2_split
and conv3x3_first_split (csrc/w2xc_split.hip) at a known layer.  A key names one instantiation:
    (kernel_name, cin, cout, mode, out_terms)      out_terms: T (term planes), 0 (fp32), 9 (tap planes of a fused last layer)."""
from collections import namedtuple

import numpy as np

import bf16_ref
from bf16_ref import FUSION_AUTO, FUSION_FIRST, FUSION_LAST, FUSION_OFF, K_FIRST2_SPLIT, K_FIRST_SPLIT, K_MID_SPLIT

MODES = ["bf16", "bf16x2", "bf16x3", "fp16x2"]
MID = (32, 64, 128)

# (h, w).  Tiles are 32 px x 8 or 16 rows and layer k's plane is w + 2 (n - k) wide, so the edges move per layer.
#   1x1    every tile is an edge tile in both directions
#   17x33  one row and one column past a tile edge at the output, ragged pixel quads
#   tall   one tile column, >= 258 tile rows even at 16-row tiles: the grid is capped at 256 workgroups (w2xc_persistent_grid) and split into
#          8 chunks, one per XCD, so workgroups of every chunk take a second tile (weight ring, A double buffer, epoch schedule hand over)
#   wide   one tile row, >= 258 tile columns: the same second trip through the other coordinate of the tile decode
SIZES = {"1x1": (1, 1), "17x33": (17, 33), "tall": (4120, 3), "wide": (3, 8230)}
SECOND_TRIP = ("tall", "wide")
ALL, NO_WIDE, SMALL = ("1x1", "17x33", "tall", "wide"), ("1x1", "17x33", "tall"), ("1x1", "17x33")

# Mirror of launch_split_t's table (csrc/w2xc_split.hip): (rows per tile = MB * WM, wave columns = WN) per (terms, cin, cout).
# WN is also the number of partial tap-plane sets a fused-last epilogue writes: w2xc_split_halves must answer the same.
def split_tile(terms, cin, cout):
    if terms == 1:
        return {(32, 32): (8, 1), (32, 64): (16, 1), (32, 128): (8, 2), (64, 32): (8, 1), (64, 64): (16, 2), (64, 128): (8, 2),
                (128, 32): (8, 1), (128, 64): (8, 1), (128, 128): (16, 2)}[(cin, cout)]
    if terms == 2:
        return (16, 1 if cout == 32 else 2)
    return (8, 2) if cout == 128 else (16, 1)


# id, planes, w2xc_opts.fusion, layer under test (0-based), its kernel, cin, cout, out_terms ("T" = the mode's term count), sizes, planes in
Case = namedtuple("Case", "id planes fusion layer kernel cin cout ot sizes n_in")


def _cases():
    out = []
    for cin in MID:
        for cout in MID:
            # no first fusion, so the 32-plane-input shapes run the mid kernel; layer 3 (cout -> 32) makes layer 2's output term planes
            out.append(Case("split_%d_%d_otT" % (cin, cout), [1, cin, cout, 32, 1], FUSION_LAST, 1, K_MID_SPLIT, cin, cout, "T", ALL, 1))
            # three layers: fuse_first stands back for fuse_last (w2xc_select.cpp), layer 2 carries the last layer's taps
            out.append(Case("split_%d_%d_ot9" % (cin, cout), [1, cin, cout, 1], FUSION_AUTO, 1, K_MID_SPLIT, cin, cout, 9, ALL, 1))
            # last layer unfused: fp32 out.  With 32 planes in, W2XC_FUSION_FIRST would run layer 2 inside conv3x3_first2_split
            # (the first2 cases below); W2XC_FUSION_OFF keeps it the mid kernel.
            out.append(Case("split_%d_%d_ot0" % (cin, cout), [1, cin, cout, 1], FUSION_OFF if cin == 32 else FUSION_FIRST, 1, K_MID_SPLIT,
                            cin, cout, 0, NO_WIDE, 1))
    for cout in MID:
        out.append(Case("first2_%d_otT" % cout, [1, 32, cout, 32, 1], FUSION_AUTO, 1, K_FIRST2_SPLIT, 32, cout, "T", ALL, 1))
        out.append(Case("first2_%d_ot0" % cout, [1, 32, cout, 1], FUSION_FIRST, 1, K_FIRST2_SPLIT, 32, cout, 0, NO_WIDE, 1))
        # three planes in, through w2xc_convert_planes_device (layer 2, cout -> 32 with fp32 out in front of a plain 32 -> 3 last layer, rides along)
        out.append(Case("first_3_%d" % cout, [3, cout, 32, 3], FUSION_AUTO, 0, K_FIRST_SPLIT, 3, cout, "T", NO_WIDE, 3))
    return out


CASES = _cases()


def seed_of(case):
    return 1300 + CASES.index(case)


def model_plane_reference(case, mode, size, tries=32):
    """(layers, plane (n_in, h, w), float64-accumulated reference) of a case at a size.
    The tests' bounds are fractions of the OUTPUT RANGE, which presumes a range of the size of what the last layer sums.  A 1x1 plane has ONE
    output value (and a constant padded input, so that value is a property of the weights): where it is a near-cancellation of the last layer's
    9 cin products, "error over range" is the error times the cancellation factor, whatever computes it.  So a case takes the first (weights,
    plane) of a fixed seed sequence whose REFERENCE output range is at least 1/8 of the largest activation the last layer reads -- with the
    He-scaled weights of tools/gen_model.py the typical range is ~0.5 of it.  The choice looks at the emulation only, never at a GPU result."""
    from tools import gen_model
    h, w = SIZES[size]
    for k in range(tries):
        layers = gen_model.synth_layers(case.planes, seed_of(case) + 100 * k)
        x = np.random.default_rng(40 + h + seed_of(case) + 100 * k).random((case.n_in, h, w), dtype=np.float32)
        trace = []
        want = bf16_ref.convert_mode_emulated(layers, x, mode, n_in=case.n_in, fusion=case.fusion, trace=trace)
        if float(np.abs(want).max()) >= trace[-1] / 8:
            return layers, x, want
    raise AssertionError("no well-conditioned weights and plane in %d seeds: %s %s %s" % (tries, case.id, mode, size))


def precision_of(w2xc, mode):
    return {"bf16": w2xc.PRECISION_BF16, "bf16x2": w2xc.PRECISION_BF16X2, "bf16x3": w2xc.PRECISION_BF16X3, "fp16x2": w2xc.PRECISION_FP16X2}[mode]


def terms_of(mode):
    return bf16_ref.MODES[mode][0]


def key_of(case, mode):
    """the instantiation the case is there for"""
    return (case.kernel, case.cin, case.cout, mode, terms_of(mode) if case.ot == "T" else case.ot)


def keys_of(case, mode):
    """the keys a (case, mode) covers: the layer under test, and conv3x3_first_split where it runs layer 1 (it "comes with" the mid cases)"""
    flow = bf16_ref.split_dataflow(case.planes, mode, case.fusion)
    keys = {key_of(case, mode)}
    if flow[0][0] == K_FIRST_SPLIT:
        keys.add((K_FIRST_SPLIT, flow[0][1], flow[0][2], mode, flow[0][3]))
    return keys


def all_keys():
    """every instantiation csrc/w2xc_split.hip has of the three kernels"""
    keys = set()
    for mode in MODES:
        T = terms_of(mode)
        for cout in MID:
            for cin in MID:
                keys |= {(K_MID_SPLIT, cin, cout, mode, ot) for ot in (T, 0, 9)}       # launch_split_t: 9 shapes x 4 modes x 3 output kinds
            keys |= {(K_FIRST2_SPLIT, 32, cout, mode, ot) for ot in (T, 0)}            # launch_first2_t: 3 x 4 x 2
            keys |= {(K_FIRST_SPLIT, cin, cout, mode, T) for cin in (1, 3)}            # launch_first_split_t<OT = T>: 2 x 3 x 4
    return keys


def layer_extent(case, size, layer):
    """(out_h, out_w) of 0-based layer `layer` of the whole plane in one band: layer k = layer + 1 computes h + 2 (n - k) rows"""
    h, w = SIZES[size]
    n = len(case.planes) - 1
    return h + 2 * (n - layer - 1), w + 2 * (n - layer - 1)


def tiles_at(case, mode, size, layer):
    cin, cout = case.planes[layer], case.planes[layer + 1]
    rows = split_tile(terms_of(mode), cin, cout)[0] if bf16_ref.split_dataflow(case.planes, mode, case.fusion)[layer][0] == K_MID_SPLIT else 8
    oh, ow = layer_extent(case, size, layer)
    return -(-ow // 32) * -(-oh // rows)
