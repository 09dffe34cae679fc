"""The row plan against the launchers' 32-bit limits, on the CPU: whatever w2xc_plan_rows grants must be launchable.

conv3x3_wino4 and conv3x3_first2_wino4 address activations with 32-bit lane offsets and count items in int; their launchers answer a descriptor past
those limits with hipErrorInvalidValue -- in the middle of a call, after the layers in front have run.  plan_rows (csrc/w2xc_select.cpp) is where a
band's height is decided, so it is where such a band has to be shortened, or the plane refused (W2XC_ERR_UNSUPPORTED, before a device is touched) where
no band helps.  tests/far_offsets.py restates the rules and the strides of a plan's launches as plain integer arithmetic and quotes the source lines
(tests/test_far_offsets.py reads them); this file walks a grid of topologies, plane sizes, budgets and options through w2xc_plan_rows and
w2xc_plan_region and asserts that no launch of any plan breaks a rule of the kernel w2xc_layer_kernel_name names for it.

The rules: 3 in_cs 4 + 24 in_rs 4 < 2^32 (conv3x3_wino4, planar planes in), 24 in_rs 4 < 2^32 (conv3x3_wino4, 32 NHWC planes in), 12 out_cs 4 +
(out_h + 8) out_rs 4 < 2^32 (conv3x3_first2_wino4), items x batch < 2^31 (the batch forms, and since this test the single-image launch_wino4, which
formed the count in int unchecked), and PROG's out_h out_rs 4 < 2^32 -- which no plan can break: prog_eligible asks it before the launcher does and
leaves such a band to the gather launch (far_offsets.prog_finishes).

On the commit before this test the grid was red: e.g. [1, 32, 64, 1] at 1 398 144 x 4 planned conv3x3_wino4<32, 64> on NHWC rows of 24 in_rs 4 =
4 294 965 248 + ... >= 2^32 bytes (any plane from 1 398 098 pixels wide on, default options), and [1, 128, 128, 1] at 16384 x 25600 with workspace_mb =
262144 planned one band whose 128 planar planes break 3 in_cs 4 + 24 in_rs 4 < 2^32; no width or budget check stood in a caller's way."""
import pytest

from tools import gen_model
import far_offsets as fo

TOPOLOGIES = [([1, 32, 32, 64, 64, 128, 128, 1], 0), ([1, 32, 32, 1], 0), ([1, 32, 64, 64, 1], 0), ([1, 128, 128, 1], 0), ([3, 32, 64, 128, 3], 0),
              ([3, 16, 32, 64, 128, 128, 256], 3)]
WIDTHS = [64, 4100, 16384, 65536, 1398080, 1398144, 4194304]
HEIGHTS = [4, 2052, 16384, 4194304]
WORKSPACES = [0, 65536, 262144]          # 0: the default (16384)
OPTIONS = [dict(), dict(kernel=fo.KERNEL_WINOGRAD4), dict(fusion=fo.FUSION_OFF), dict(fusion=fo.FUSION_PROG)]
IDS = ["-".join(map(str, p)) + ("^%d" % h if h else "") for p, h in TOPOLOGIES]


def model(w2xc, planes, head):
    layers = gen_model.synth_layers(planes, 7)
    return w2xc._ModelSet.from_layers(layers, head=gen_model.synth_head(planes[-1], head, 7) if head else None)


def views(w2xc, h, n):
    """both halo geometries: the whole plane (four halo rows per layer under conv3x3_wino4), and the middle third of the rows on a view with n halo rows
    (one per layer; W2XC_KERNEL_AUTO refuses that view, a named kernel runs on it)"""
    yield 0, h, 0, h
    ra, rb = w2xc.shard_rows(h, 3, 1) if h >= 3 else (0, h)
    y0, y1 = w2xc.shard_view(h, ra, rb, n)
    yield ra, rb, y0, y1 - y0


def plan_violations(w2xc, ms, io, w, h, ra, rb, vy0, vh, okw):
    """[] or what is wrong with the plan of one grid point; None where the library refuses it with W2XC_ERR_ARG / W2XC_ERR_UNSUPPORTED"""
    opts = w2xc.make_opts(**okw)
    try:
        plan = ms.plan_rows(w, h, ra, rb, vy0, vh, opts=opts)
    except w2xc.W2xcError as e:
        return None if e.code in (w2xc.ERR_ARG, w2xc.ERR_UNSUPPORTED) else ["refused with code %d: %s" % (e.code, e)]
    n = ms.n_layers
    names = [ms.kernel_name(l, opts) for l in range(n)]
    if fo.FIRST2 in names and not plan.fused_first:   # W2XC_FUSION_AUTO gave the fused first layers up (plan_rows): the chain of W2XC_FUSION_LAST runs
        names = [ms.kernel_name(l, w2xc.make_opts(**dict(okw, fusion=fo.FUSION_LAST))) for l in range(n)]
    assert (fo.FIRST2 in names) == bool(plan.fused_first)
    band = plan.band_rows
    assert 1 <= band <= rb - ra and plan.n_bands == -(-(rb - ra) // band)
    bad = []
    # the first band, one in the middle (no plane edge clips its regions: the tallest) and the last
    starts = sorted({ra, ra + band * ((plan.n_bands - 1) // 2), ra + band * (plan.n_bands - 1)})
    for y0 in starts:
        y1 = min(rb, y0 + band)
        regions = [ms.plan_region(plan, h, k, y0, y1) for k in range(1, n + 1)]
        ls = fo.launches(names, io, w, regions, okw.get("fusion", fo.FUSION_AUTO))
        bad += [("band [%d,%d) of %d" % (y0, y1, plan.n_bands),) + v for v in fo.violations(ls)]
    # one band, default kernels: a batch may run one launch per layer for `sub` images at once
    if plan.n_bands == 1 and (ra, rb) == (0, h) and not okw.get("band_rows"):
        try:
            batched, sub = ms.batch_plan(io[0][0], w, h, up2x=ms.has_head, opts=opts)
        except w2xc.W2xcError:
            batched = 0
        if batched:
            regions = [ms.plan_region(plan, h, k, 0, h) for k in range(1, n + 1)]
            bad += [("batch of %d" % sub,) + v for v in fo.violations(fo.launches(names, io, w, regions), batch=sub)]
    return bad


@pytest.mark.parametrize("planes,head", TOPOLOGIES, ids=IDS)
def test_every_planned_launch_is_within_its_launchers_limits(w2xc, planes, head):
    ms = model(w2xc, planes, head)
    io = list(zip(planes[:-1], planes[1:])) + ([(planes[-1], head)] if head else [])
    n = ms.n_layers
    assert n == len(io)
    planned = refused = 0
    bad = []
    for w in WIDTHS:
        for h in HEIGHTS:
            for ra, rb, vy0, vh in views(w2xc, h, n):
                for ws in WORKSPACES:
                    for band_rows in (0, rb - ra):   # the solver's band, and one above every cap: the caller's band is shortened the same way
                        for o in OPTIONS:
                            okw = dict(o, workspace_mb=ws, band_rows=band_rows)
                            v = plan_violations(w2xc, ms, io, w, h, ra, rb, vy0, vh, okw)
                            if v is None:
                                refused += 1
                                continue
                            planned += 1
                            bad += [((w, h, (ra, rb), okw),) + x for x in v]
    print("%s: %d plans, %d refusals" % ("-".join(map(str, planes)), planned, refused))
    assert planned > refused and planned + refused == len(WIDTHS) * len(HEIGHTS) * 2 * len(WORKSPACES) * 2 * len(OPTIONS)
    assert not bad, "%d launches past a launcher's limit; the first:\n%s" % (len(bad), "\n".join(map(repr, bad[:6])))


def test_a_plane_no_band_makes_addressable_is_refused_with_its_width(w2xc):
    ms = model(w2xc, list(fo.REFUSED["planes"]), 0)
    h, w = fo.REFUSED["size"]
    for okw in (dict(), dict(fusion=fo.FUSION_OFF), dict(band_rows=4), dict(workspace_mb=1)):
        with pytest.raises(w2xc.W2xcError) as e:
            ms.plan_rows(w, h, opts=w2xc.make_opts(**okw))
        assert e.value.code == w2xc.ERR_UNSUPPORTED and str(w) in str(e.value), e.value
    # the widest plane the rule admits plans, and the F(2x2) and MFMA kernels have no such rule
    assert ms.plan_rows(1398097, h).n_bands == 1   # (layer 1 computes w + 4 pixels a row: 24 x 1398101 x 32 x 4 < 2^32)
    with pytest.raises(w2xc.W2xcError):
        ms.plan_rows(1398098, h)
    for kernel in (fo.KERNEL_WINOGRAD32, fo.KERNEL_MFMA, fo.KERNEL_DIRECT):
        assert ms.plan_rows(w, h, opts=w2xc.make_opts(kernel=kernel)).n_bands == 1


def test_the_caps_bind_where_the_rules_say(w2xc):
    """the band plan_rows grants is the tallest the rule admits, not merely a safe one: four rows more (a block row of the four-rows-per-layer geometry)
    break the rule that capped it"""
    ms = model(w2xc, [1, 128, 128, 1], 0)
    io = [(1, 128), (128, 128), (128, 1)]
    w, h = 16384, 25600          # planes of 16416 x 25604 = 420 Mi floats: 3 in_cs 4 alone is past 2^32
    o = w2xc.make_opts(workspace_mb=262144)
    plan = ms.plan_rows(w, h, opts=o)
    whole = [(1 + 128) * 4 * fo.ru32(w + 4) * (h + 4), 2 * 9 * 4 * fo.ru32(w + 2) * (h + 2)]
    assert sum(whole) < 262144 << 20 and plan.n_bands == 2, "the budget admits the whole plane in one band: the addressing cap binds"
    names = [ms.kernel_name(l, o) for l in range(3)]
    mid = 13                     # a band no plane edge clips, off the block rows at both ends: the tallest regions

    def broken(rows):
        regions = [ms.plan_region(plan, h, k, mid, mid + rows) for k in range(1, 4)]
        return fo.violations(fo.launches(names, io, w, regions))
    assert not broken(plan.band_rows)
    assert [v[1] for v in broken(plan.band_rows + 4)] == ["3 in_cs 4 + 24 in_rs 4 < 2^32"]
    # conv3x3_first2_wino4: the cap of 64 Mi floats a plane, as it was before the other rules joined it
    ms5 = model(w2xc, [1, 32, 32, 64, 64, 1], 0)
    rs = fo.ru32(8192 + 6)
    top = (64 << 20) // rs - 30          # region rows minus the halo of layer 2 (6 + 8 x 3)
    o = w2xc.make_opts(workspace_mb=65536)
    assert ms5.plan_rows(8192, top, opts=o).n_bands == 1
    p = ms5.plan_rows(8192, top + 1, opts=o)
    assert p.n_bands == 2 and p.band_rows == top & ~3
    assert ms5.plan_rows(8192, 16384, opts=w2xc.make_opts(workspace_mb=65536, band_rows=16384)).band_rows == top & ~3   # (a caller's band is shortened the same way)
