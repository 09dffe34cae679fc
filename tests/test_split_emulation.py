"""CPU tests of the 16-bit reference (tests/bf16_ref.py) and of the case table of the kernel matrix (tests/split_matrix.py): the Python
mirror of the engine's dataflow is pinned to the library's own selection code (w2xc_layer_kernel_name, w2xc_plan_rows: host code, no
device), the table is shown to cover every instantiation, and the emulation is tied to the fp32 oracle where the two must agree."""
import numpy as np
import pytest

import bf16_ref
import split_matrix as sm
from conftest import rand_plane, small_layers
from oracle import oracle as orc

CASE_MODES = [pytest.param(c, m, id="%s-%s" % (c.id, m)) for c in sm.CASES for m in sm.MODES]


def _opts(w2xc, case, mode, **kw):
    return w2xc.make_opts(precision=sm.precision_of(w2xc, mode), fusion=case.fusion, **kw)


@pytest.mark.parametrize("case,mode", CASE_MODES)
def test_dataflow_names_the_kernels_the_library_selects(w2xc, case, mode):
    ms = w2xc._ModelSet.from_layers(small_layers(case.planes, sm.seed_of(case)))
    flow = bf16_ref.split_dataflow(case.planes, mode, case.fusion)
    o = _opts(w2xc, case, mode)
    assert [f[0] for f in flow] == [ms.kernel_name(l, o) for l in range(ms.n_layers)]
    assert [(f[1], f[2]) for f in flow] == list(zip(case.planes[:-1], case.planes[1:]))
    # the case puts the instantiation it is there for at its layer
    T = sm.terms_of(mode)
    assert flow[case.layer] == (case.kernel, case.cin, case.cout, T if case.ot == "T" else case.ot)


def _workspace_bytes(case, mode, h, w):
    """RowPlan::ws_need (csrc/w2xc_select.cpp) for the whole plane in one band, from split_dataflow's out_terms alone: layer k's output
    goes to buffer (k - 1) & 1 and takes, per pixel, 2 T bytes per plane as term planes, 4 as fp32, and 9 tap planes of 4 bytes per
    wave column of the producing tile shape where the last layer is computed in its epilogue."""
    flow = bf16_ref.split_dataflow(case.planes, mode, case.fusion)
    n, T = len(flow), sm.terms_of(mode)
    need = [0, 0]
    for k in range(1, n + 1):
        name, cin, cout, ot = flow[k - 1]
        if k == n and cout == 1:
            break                                       # written straight to the caller's plane
        if k == 1 and name == bf16_ref.K_FUSED_AWAY:
            continue                                    # stays on chip
        px = sm.split_tile(T, cin, cout)[1] * 9 * 4 if ot == 9 else cout * (2 * ot if 1 <= ot <= 3 else 4)
        need[(k - 1) & 1] = max(need[(k - 1) & 1], (h + 2 * (n - k)) * (w + 2 * (n - k)) * px)
    return need


@pytest.mark.parametrize("case,mode", CASE_MODES)
def test_dataflow_out_terms_match_the_planned_workspace(w2xc, case, mode):
    """The bytes per element differ between the three output kinds (2 T, 4, wave columns x 9 x 4), so the workspace w2xc_plan_rows
    reports pins split_dataflow's out_terms -- and split_tile's wave columns -- to the library."""
    ms = w2xc._ModelSet.from_layers(small_layers(case.planes, sm.seed_of(case)))
    for (h, w) in ((17, 33), (40, 7)):
        p = ms.plan_rows(w, h, opts=_opts(w2xc, case, mode))
        assert p.n_bands == 1
        assert list(p.workspace_bytes) == _workspace_bytes(case, mode, h, w), (h, w)
    flow = bf16_ref.split_dataflow(case.planes, mode, case.fusion)
    assert p.fused_first == int(flow[0][0] == bf16_ref.K_FUSED_AWAY) and p.fused_last == int(flow[-1][0] == bf16_ref.K_LAST_GATHER)


def test_case_table_covers_every_instantiation():
    """Set equality, so a dropped case fails: 108 keys of conv3x3_split (9 shapes x 4 modes x out_terms T / 0 / 9), 24 of
    conv3x3_first2_split (3 x 4 x T / 0) and 24 of conv3x3_first_split (cin 1 / 3 x 3 x 4, always out_terms = T).
    No key is out of reach: layer_kind (csrc/w2xc_select.cpp) answers W2XC_K_FIRST_SPLIT exactly when layer 2 is a mid layer, whose
    input is then T term planes (out_terms_of), so conv3x3_first_split has no other output kind to reach; the fp32-output form of a
    32-planes-in mid layer needs W2XC_FUSION_OFF (with W2XC_FUSION_FIRST fuse_first hands that layer to conv3x3_first2_split)."""
    covered = set()
    for c in sm.CASES:
        for m in sm.MODES:
            covered |= sm.keys_of(c, m)
    want = sm.all_keys()
    assert len([k for k in want if k[0] == bf16_ref.K_MID_SPLIT]) == 108
    assert len([k for k in want if k[0] == bf16_ref.K_FIRST2_SPLIT]) == 24
    assert len([k for k in want if k[0] == bf16_ref.K_FIRST_SPLIT]) == 24
    assert covered == want, (sorted(want - covered), sorted(covered - want))
    assert len({c.id for c in sm.CASES}) == len(sm.CASES)


def test_case_sizes_follow_the_output_kind():
    for c in sm.CASES:
        assert set(sm.SMALL) <= set(c.sizes)
        if c.kernel != bf16_ref.K_FIRST_SPLIT:
            assert "tall" in c.sizes and (("wide" in c.sizes) == (c.ot != 0)), c.id
    # the second-trip sizes give more tiles than the persistent grid has workgroups, at the layer under test, for every tile shape
    for c in sm.CASES:
        for m in sm.MODES:
            for s in c.sizes:
                if s in sm.SECOND_TRIP:
                    assert sm.tiles_at(c, m, s, c.layer) > 256, (c.id, m, s)


def test_every_case_finds_well_conditioned_weights_at_the_small_sizes():
    """model_plane_reference's seed sequence ends for every case (the one-value output of a 1x1 plane is where it has to pass seeds over)"""
    for c in sm.CASES:
        for s in sm.SMALL:
            layers, x, want = sm.model_plane_reference(c, "bf16x3", s)
            assert x.shape == (c.n_in,) + sm.SIZES[s] and want.shape == (c.planes[-1],) + sm.SIZES[s]


def test_dataflow_refuses_what_the_engine_refuses():
    for planes in ([1, 5, 1], [32, 32, 1], [1, 32, 7, 1]):
        with pytest.raises(ValueError):
            bf16_ref.split_dataflow(planes, "bf16x3")
    # first -> last only: nothing to split
    assert [f[0] for f in bf16_ref.split_dataflow([1, 32, 1], "bf16")] == ["conv3x3_first", "conv3x3_last"]


@pytest.mark.parametrize("planes", [[1, 32, 64, 32, 1], [1, 64, 128, 1]])
def test_three_term_emulation_agrees_with_the_fp32_oracle(oracle_built, planes):
    """BF16X3 carries 24 bits per value: its float64-accumulated emulation and the fp32 reference differ at the level of two fp32
    summation orders, the project's stated 2e-5 of the output range."""
    layers = small_layers(planes, 77 + len(planes))
    x = rand_plane(23, 37, 4)
    want = orc.Oracle(layers).convert(x)
    scale = float(np.abs(want).max())
    for fusion in (bf16_ref.FUSION_AUTO, bf16_ref.FUSION_OFF):
        for acc in ("float64", "float32"):
            got = bf16_ref.convert_split_emulated(layers, x, 3, fusion=fusion, accumulate=acc)[0]
            assert np.abs(got - want).max() <= 2e-5 * scale, (fusion, acc, np.abs(got - want).max() / scale)


def test_one_term_first_last_model_is_plain_fp32(w2xc, oracle_built):
    """[1, 32, 1] has no mid layer: the engine runs conv3x3_first -> conv3x3_last, both fp32, and the activation between them is never
    rounded.  The emulation must do the same (one that rounded it to bf16 would be off by ~1e-3 of the range)."""
    planes = [1, 32, 1]
    layers = small_layers(planes, 403)
    ms = w2xc._ModelSet.from_layers(layers)
    o = w2xc.make_opts(precision=w2xc.PRECISION_BF16)
    assert [ms.kernel_name(l, o) for l in range(2)] == ["conv3x3_first", "conv3x3_last"]
    x = rand_plane(45, 77, 50)
    want = orc.Oracle(layers).convert(x)
    scale = float(np.abs(want).max())
    for got in (bf16_ref.convert_split_emulated(layers, x, 1)[0], bf16_ref.convert_bf16_emulated(layers, x)):
        err = float(np.abs(got - want).max())
        assert err <= 2e-6 * scale, err / scale      # fp32 level: 288 products of O(1) values summed in fp32 vs float64


def test_float32_accumulation_is_the_same_dataflow():
    """accumulate="float32" differs from float64 only by fp32 summation: at T = 3 at the 2e-5 level, at T = 1 by rounding flips (1e-2 / 1e-3 gates)."""
    layers = small_layers([1, 32, 64, 64, 1], 12)
    x = rand_plane(19, 35, 6)
    for mode, mx, mean in (("bf16x3", 2e-5, 2e-5), ("fp16x2", 2e-5, 2e-5), ("bf16", 1e-2, 1e-3)):
        a = bf16_ref.convert_mode_emulated(layers, x, mode)[0]
        b = bf16_ref.convert_mode_emulated(layers, x, mode, accumulate="float32")[0]
        scale = float(np.abs(a).max())
        assert np.abs(a - b).max() <= mx * scale and np.abs(a - b).mean() <= mean * scale, mode
        assert not np.array_equal(a, bf16_ref.convert_mode_emulated(layers, x, mode, fusion=bf16_ref.FUSION_OFF)[0]) or mode != "bf16"
