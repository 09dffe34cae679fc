"""Every selection decision of csrc/w2xc_select.cpp (resolve_chain and what plans with it), line for line against a recording taken BEFORE the free
predicates became one resolved table: tools/select_sweep.py regenerates the lines -- the kernel of every layer, every field of the row plan with both
workspace sizes, the batch plan, or the refusal with its code and message -- through entry points that need no device, and
tests/golden/select_sweep.txt.gz holds what the predicates answered.  No line is skipped; a refusal must be the same refusal."""
import itertools

import pytest

from tools import select_sweep


@pytest.fixture(scope="module")
def lines(w2xc):
    return select_sweep.sweep_lines(w2xc)


def test_every_decision_is_the_recorded_one(lines):
    want = select_sweep.read_fixture()
    diff = [(i, w, g) for i, (w, g) in enumerate(itertools.zip_longest(want, lines)) if w != g]
    assert not diff, "%d of %d lines differ; the first:\n%s" % (
        len(diff), len(want), "\n".join("line %d\n  recorded: %s\n  now:      %s" % d for d in diff[:8]))


def test_the_recording_covers_what_it_is_for(w2xc):
    """the cases the recording exists for are in it: the too-wide plane with both outcomes of the fused first layers (W2XC_FUSION_AUTO gives the fusion
    up, W2XC_FUSION_ON is refused), the plane too wide for conv3x3_wino4 on 32 NHWC planes (refused whatever the fusion), the banded plan, the minimum-halo refusal, both head models, and every option set of every topology"""
    want = select_sweep.read_fixture()
    by_key = {l.split(" | ")[0]: l.split(" | ")[1:] for l in want}
    assert len(by_key) == len(want)                                   # one line per (topology, options, plane)
    n_opts = len(list(select_sweep.option_sets(w2xc)))
    assert n_opts == 6 * 7 + 4 * 2 * 7
    assert len(want) == n_opts * (4 * len(select_sweep.TOPOLOGIES) + 1)
    scale = "-".join(map(str, select_sweep.SCALE))
    auto = by_key["%s p0k0f%d 1300000x64" % (scale, w2xc.FUSION_AUTO)]
    on = by_key["%s p0k0f%d 1300000x64" % (scale, w2xc.FUSION_ON)]
    assert auto[1].split(",")[4:6] == ["0", "1"]                      # planned, without the fused first layers
    assert on[1].startswith("!%d:plane too wide" % w2xc.ERR_UNSUPPORTED)
    # 2 000 000 pixels: the unfused chain's conv3x3_wino4<32, 64> would read 32 NHWC planes with 24 in_rs 4 >= 2^32 -- refused in the plan, with the width
    for fusion in (w2xc.FUSION_AUTO, w2xc.FUSION_ON, w2xc.FUSION_OFF):
        wide = by_key["%s p0k0f%d 2000000x64" % (scale, fusion)]
        assert wide[1].startswith("!%d:plane too wide (2000000 pixels)" % w2xc.ERR_UNSUPPORTED), wide
    assert by_key["%s p0k%df0 2000000x64" % (scale, w2xc.KERNEL_WINOGRAD32)][1][0] != "!"   # (the F(2x2) kernels have no such rule: planned)
    assert by_key["%s p0k0f0 64x64" % scale][1].split(",")[4:6] == ["1", "1"]
    assert int(by_key["%s p0k0f0 3000x4000/64M" % scale][1].split(",")[3]) > 1   # banded
    minv = [v for k, v in by_key.items() if k.endswith("min")]
    assert len(minv) == n_opts and sum(v[1].startswith("!%d:" % w2xc.ERR_ARG) and "halo rows" in v[1] for v in minv) >= 1
    assert any("^3 " in k for k in by_key) and any("^1 " in k for k in by_key)
