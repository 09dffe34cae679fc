"""The case table and the checker of tests/far_offsets.py on the CPU (tests/test_gpu_far_offsets.py runs the cases on a device): every source line the
arithmetic restates is where the table says, every case plans as one band of the kernels it names with its buffers past their thresholds, the window
reference equals the whole-plane reference wherever the window lies, and the comparison fails for what a wrapped offset would deliver."""
import os

import numpy as np
import pytest

from conftest import rand_plane
from oracle import oracle as orc
from tools import gen_model
import bf16_ref
import far_offsets as fo
import fp32_matrix as fm
import upconv_ref


def test_every_quoted_line_is_where_the_table_says():
    text = {}
    for f, line, quote in fo.QUOTES:
        lines = text.setdefault(f, open(os.path.join(fo.CSRC, f)).read().splitlines())
        assert quote in lines[line - 1], (f, line, lines[line - 1].strip())


def test_the_option_constants_are_the_packages(w2xc):
    assert (fo.KERNEL_AUTO, fo.KERNEL_DIRECT, fo.KERNEL_MFMA, fo.KERNEL_WINOGRAD32, fo.KERNEL_WINOGRAD4) == (
        w2xc.KERNEL_AUTO, w2xc.KERNEL_DIRECT, w2xc.KERNEL_MFMA, w2xc.KERNEL_WINOGRAD32, w2xc.KERNEL_WINOGRAD4)
    assert (fo.FUSION_AUTO, fo.FUSION_OFF, fo.FUSION_LAST, fo.FUSION_GATHER_LAUNCH, fo.FUSION_PROG) == (
        w2xc.FUSION_AUTO, w2xc.FUSION_OFF, w2xc.FUSION_LAST, w2xc.FUSION_GATHER_LAUNCH, w2xc.FUSION_PROG)
    assert fo.PRECISION == {"fp32": w2xc.PRECISION_FP32, "bf16": w2xc.PRECISION_BF16, "bf16x2": w2xc.PRECISION_BF16X2, "bf16x3": w2xc.PRECISION_BF16X3,
                            "fp16x2": w2xc.PRECISION_FP16X2}
    assert fo.TERMS == {m: bf16_ref.MODES[m][0] for m in fo.TERMS}


@pytest.mark.parametrize("case", fo.CASES, ids=[c.id for c in fo.CASES])
def test_a_case_plans_as_the_table_says(w2xc, case):
    layers, head = fo.model_arrays(case)
    ms = w2xc._ModelSet.from_layers(layers, head=head)
    plan, names, ls = fo.planned(w2xc, ms, case)
    # the kernels exist: the families of the fp32 matrix, the dataflow of the 16-bit emulation
    if case.mode == "fp32":
        families = {fm.family_of(k[0]) for k in fm.covered_keys()}
        assert set(names) - {fo.IN_NEXT} <= families, set(names) - families
    else:
        assert names == [f[0] for f in bf16_ref.split_dataflow(list(case.planes), case.mode)]
    total = fo.device_bytes(case, plan, ls)
    assert total <= fo.CAP_BYTES, "%s: %.1f GiB" % (case.id, total / fo.GIB)
    wins = fo.windows(case, ls)
    h, w = case.size
    assert len(wins) >= 5 and all(0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w for y0, y1, x0, x1 in wins), wins
    if plan is not None and case.mode == "fp32":
        # the workspaces the plan reports hold these launches: layer k writes workspace (k - 1) & 1 (RowPlan::ws_need sizes them by the unclipped halo)
        for i in (0, 1):
            mine = max([l.bytes for l in ls if (l.k - 1) & 1 == i and l.kind not in ("out", "none")] or [0])
            assert mine <= plan.workspace_bytes[i] <= mine * 1.02 + (1 << 20), (i, mine, plan.workspace_bytes[i])
    if case.mode != "fp32":      # the term planes are workspace 0, and the smallest plane of its aspect that takes them past 2^32
        assert plan.workspace_bytes[0] == ls[0].bytes > fo.TWO32
        o = w2xc.make_opts(**fo.opts_kw(case))
        assert ms.plan_rows(w - 2, h - 1, opts=o).workspace_bytes[0] <= fo.TWO32
    if case.id == "first2":      # the smallest height; and the cap itself on the plan: the tallest single band, one row more is two bands
        p = ms.plan_rows(w, h - 1)
        regions = [ms.plan_region(p, h - 1, k, 0, h - 1) for k in range(1, 6)]
        assert fo.first2_lane_offset(fo.launches(names, fo.io_of(case), w, regions)[1]) <= fo.TWO31
        top = (64 << 20) // fo.ru32(w + 6) - 30
        o = w2xc.make_opts(workspace_mb=65536)
        one, two = ms.plan_rows(w, top, opts=o), ms.plan_rows(w, top + 1, opts=o)
        assert (one.n_bands, two.n_bands) == (1, 2)
        regions = [ms.plan_region(one, top, k, 0, top) for k in range(1, 6)]
        lane = fo.first2_lane_offset(fo.launches(names, fo.io_of(case), w, regions)[1])
        assert 3 * fo.GIB < lane < fo.TWO32, lane


def test_the_refused_plane(w2xc):
    ms = w2xc._ModelSet.from_layers(gen_model.synth_layers(list(fo.REFUSED["planes"]), 4100))
    h, w = fo.REFUSED["size"]
    with pytest.raises(w2xc.W2xcError) as e:
        ms.plan_rows(w, h)
    assert e.value.code == w2xc.ERR_UNSUPPORTED and str(w) in str(e.value)


# ---- the checker ----
N3 = [1, 16, 16, 1]


def oracle_model(layers):
    ref = orc.Oracle(layers)
    return lambda c: ref.convert_f64(c[0])[None]


def test_window_reference_equals_the_whole_plane_reference(oracle_built):
    layers = gen_model.synth_layers(N3, 9)
    x = rand_plane(40, 50, 3)[None]
    model = oracle_model(layers)
    whole = model(x)
    for y0 in (0, 7, 24):
        for x0 in (0, 13, 34):
            win = (y0, y0 + 16, x0, x0 + 16)
            ref = fo.window_reference(model, x, 3, win)
            assert ref.shape == (1, 16, 16)
            assert np.allclose(ref, whole[:, y0:y0 + 16, x0:x0 + 16], rtol=0, atol=1e-13), (win, float(np.abs(ref - whole[:, y0:y0 + 16, x0:x0 + 16]).max()))


def test_window_reference_of_a_head_model_and_of_the_emulation():
    layers, head = upconv_ref.head_model([3, 8], 3, 5)
    x = np.random.default_rng(5).random((3, 20, 26), dtype=np.float32)
    model = lambda c: upconv_ref.reference(layers, head, c)
    whole = model(x)
    for win in ((0, 8, 0, 8), (12, 20, 18, 26), (5, 13, 9, 17)):
        y0, y1, x0, x1 = win
        assert np.allclose(fo.window_reference(model, x, 2, win, up=2), whole[:, 2 * y0:2 * y1, 2 * x0:2 * x1], rtol=0, atol=1e-13)
    layers = gen_model.synth_layers([1, 32, 32, 1], 6)
    x = rand_plane(24, 30, 4)[None]
    model = lambda c: bf16_ref.convert_mode_emulated(layers, c, "bf16x2", n_in=1)
    whole = model(x)
    for win in ((0, 8, 0, 8), (16, 24, 22, 30), (7, 15, 11, 19)):
        y0, y1, x0, x1 = win
        assert np.allclose(fo.window_reference(model, x, 3, win), whole[:, y0:y1, x0:x1], rtol=0, atol=1e-13)


def test_the_comparison_bites(oracle_built):
    """an array equal to the twin passes; the rows past a crossing replaced by the rows a wrapped address would deliver, or one wrong 4 x 4 block in the
    last tile, fail -- both against the twin and, the twin set aside, against the float64 windows"""
    layers = gen_model.synth_layers(N3, 9)
    x = rand_plane(40, 50, 3)[None]
    twin = orc.Oracle(layers).convert(x[0])[None]
    model = oracle_model(layers)
    cross, back = 23, 7          # the buffer's offset passes the threshold in row 23; 2^32 / row bytes = 7 rows
    wins = [(0, 16, 0, 16), (0, 16, 34, 50), (24, 40, 0, 16), (24, 40, 34, 50), (cross - 8, cross + 8, 17, 33)]
    refs = [fo.window_reference(model, x, 3, w) for w in wins]
    assert fo.check_plane(twin.copy(), twin, wins, refs, "fp32") == []
    wrapped = twin.copy()
    wrapped[:, cross:] = twin[:, cross - back:40 - back]
    assert not np.array_equal(wrapped[:, cross:], twin[:, cross:]), "random inputs: the rows differ"
    block = twin.copy()
    block[:, 36:40, 46:50] = twin[:, 32:36, 42:46]
    assert not np.array_equal(block, twin)
    for broken in (wrapped, block):
        bad = fo.check_plane(broken, twin, wins, refs, "fp32")
        assert any("twin" in b for b in bad) and any("window" in b for b in bad), bad
        assert any("window" in b for b in fo.check_plane(broken, broken, wins, refs, "fp32")), "the windows alone"
    assert fo.check_plane(np.where(np.arange(50) == 49, np.nan, twin).astype(np.float32), twin, wins, refs, "fp32")
