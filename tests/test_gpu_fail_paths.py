"""GPU tests of the failure paths (run with -m gpu on an MI355X): every path on which a call fails AFTER it has touched the device -- a buffer that cannot
grow, a weight image that cannot be allocated or uploaded, a layer launch that fails mid-band -- must return its documented code, leave nothing in flight and
nothing lost, and leave the model usable: the same call made again returns OK with the bits of an untouched model.  The failures are injected by
w2xc_debug_fail_nth (include/w2xc_hip.h) on the host, in place of the runtime call: nothing is exhausted, nothing faulty reaches the device.  The loop, the
case builders and the host-route groups are tests/fail_cases.py (its docstring says what is asserted for every k); DESIGN.md "Failure paths" argues, site by
site, what can be in flight when the failure lands and why nothing waits for a word that never comes.

In this process: the device entry points (they only enqueue).  In child processes, one per group: the host routes with their feeder, drainer, copy and unit
threads -- a thread that does not join ends the child at its time limit T and fails the test.  T = ten times the group's counting run (nothing armed) on the
MI355X and at least 60 s: a hang is unbounded, a slow run is not.  A child killed at T is a hang: find its cause by reading before the group runs again."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fail_cases as fc
import stream_cases as sc
from fail_cases import ALLOC, COPY, LAUNCH

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODEL_ROWS = [r.id for r in sc.ROWS if r.family in ("model", "frame")]
BLOCK_ROWS = [r.id for r in sc.ROWS if r.family == "block"]
# the counting run of each group's child on the MI355X (python tests/fail_cases.py <group> count: process start, imports and model set-up included), and its T
COUNTED_S = {"prog": 2.6, "tails": 2.4, "bands": 2.3, "routes": 2.4}
TIME_LIMIT_S = {g: max(60.0, 10.0 * s) for g, s in COUNTED_S.items()}


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    yield w2xc
    for kind in (ALLOC, COPY, LAUNCH):
        w2xc.debug_fail_nth(kind, 0)


# ---- every device entry point that takes a model: a buffer that cannot grow ----
@pytest.mark.parametrize("rid", MODEL_ROWS)
def test_device_call_survives_a_failed_allocation(gpu, rid):
    """each model, image and frame row of tests/stream_cases.py at its own shape, every scratch buffer released (w2xc_model_trim): each growth of the call
    fails once -- W2XC_ERR_NOMEM naming the buffer, the rims of the outputs intact, the call made again equal to an untouched model's, no scratch byte
    more or less"""
    E, named = fc.fail_loop(gpu, lambda: fc.StreamRun(gpu, torch, sc.BY_ID[rid]), ALLOC, what=rid)
    assert E >= 1 and named


def test_blocks_without_a_model_have_no_events(gpu):
    """the colour, YUV, TTA and resize blocks own no grow-only buffer, upload no weights and launch no model layer (the bleed's stamps are its own buffer, grown
    by the first call)"""
    for rid in BLOCK_ROWS:
        run = fc.StreamRun(gpu, torch, sc.BY_ID[rid])
        assert not run.models, rid
        want = run.call()
        for kind in (ALLOC, COPY, LAUNCH):
            gpu.debug_fail_nth(kind, 0)
        assert fc.same(run.call(), want), rid
        assert [gpu.debug_fail_nth(kind, 0) for kind in (ALLOC, COPY, LAUNCH)] == [0, 0, 0], rid


# ---- weights: the uploads of the model's first use and the lazily packed images, over the whole cold first call ----
def weight_case(gpu, name):
    x = fc.rand_plane(48, 40, 21) - 0.5
    if name == "head":       # w_alpha: the alpha head of the RGBA head call (noise "rn", scale "head" of tests/stream_cases.py)
        return lambda: fc.StreamRun(gpu, torch, sc.BY_ID["process_image_rgba_u8_up2x_batch"])
    layers, kw = {"product": (fc.PRODUCT, {}),                                        # get_ctx's uploads, then w_first2, w_wino4, w_last_wino4
                  "winograd32": (fc.PRODUCT, dict(kernel=gpu.KERNEL_WINOGRAD32)),     # w_wino
                  "split": (fc.SCALE, dict(precision=gpu.PRECISION_BF16X2))}[name]    # w_split, w_last_fused
    return lambda: fc.PlaneRun(gpu, torch, layers, x + (0.5 if name == "split" else 0.0), **kw)


@pytest.mark.parametrize("kind", [ALLOC, COPY], ids=["ALLOC", "COPY"])
@pytest.mark.parametrize("name", ["product", "winograd32", "split", "head"])
def test_weight_uploads_fail_clean(gpu, name, kind):
    """new models for every k.  A failed upload of a lazily packed image (w_first2, w_wino4, w_wino, w_last_wino4, w_split[*], w_last_fused[*]) must leave its
    pointer null: `packed` tests the pointer, and an image that was allocated but not filled would serve the next call garbage weights under W2XC_OK -- what
    upload did before it freed and nulled (read in the parent's w2xc_model.cpp / w2xc_rows.cpp; the COPY cases beyond get_ctx's uploads are the ones that
    catch it: run once on a build with that upload, all four COPY cases were red, the first at the first lazy image).  The events beyond get_ctx's own
    (w_direct, w_fast / w_alpha, bias per layer: context_uploads) are the lazy images and, for ALLOC, the workspaces"""
    make = weight_case(gpu, name)
    E, named = fc.fail_loop(gpu, make, kind, weights=True, what="weights-" + name, must_name=("a weight image",) if kind == ALLOC else ())
    assert E >= 1
    if name != "head":       # (w_alpha is one of the context's own uploads; Model::filter, the probe below, refuses a head model)
        base = context_uploads(gpu, make().models[0])
        assert E > base, "the call uploads lazily packed images beyond the context's own %d (%d events)" % (base, E)


def context_uploads(gpu, ms):
    """the uploads of get_ctx alone, counted: layer 1 of a new model as Model::filter on a 5 x 8 plane -- conv3x3_first has no lazily packed image"""
    nin, nout = ms.planes(0)
    h, w = 5, 8
    d_in = torch.zeros((nin, h, w), dtype=torch.float32, device="cuda")
    d_out = torch.empty((nout, h, w), dtype=torch.float32, device="cuda")
    gpu.debug_fail_nth(COPY, 0)
    ms.filter_device(0, nin, d_in.data_ptr(), (h * w, w, 1), w, h, d_out.data_ptr(), (h * w, w, 1), stream=0, opts=gpu.make_opts(device=0))
    torch.cuda.synchronize()
    return gpu.debug_fail_nth(COPY, 0)


# ---- a launch that fails: resident planes ----
class ProfiledRun(fc.PlaneRun):
    """PlaneRun with profile = 1; the launch counts of the call are part of its result: an event pair that went to `pending` without its launch, or one
    handed out twice, would count wrong or fail w2xc_profile_read"""

    def call(self):
        self.models[0].profile_reset(0)
        out = fc.PlaneRun.call(self)
        return out + [np.array(self.models[0].profile_read(0)[1], np.int32)]


def test_failed_launch_resident(gpu):
    """w2xc_convert_plane_device, the product topology at 48 x 40, every launch of the call failing once, without and with profiling events"""
    x = fc.rand_plane(48, 40, 22) - 0.5
    E0, _ = fc.fail_loop(gpu, lambda: fc.PlaneRun(gpu, torch, fc.PRODUCT, x), LAUNCH, what="launch-resident")
    E1, _ = fc.fail_loop(gpu, lambda: ProfiledRun(gpu, torch, fc.PRODUCT, x, profile=1), LAUNCH, what="launch-resident-profile")
    assert E0 == E1 >= 6      # (7 layers, layers 1 + 2 in one launch)


def test_failed_launch_mid_band_resident(gpu):
    """three bands (band_rows = 16 on 48 rows): a failed launch in band 2 or 3 comes behind bands that are already on the stream"""
    x = fc.rand_plane(48, 40, 23) - 0.5
    ms = gpu._ModelSet.from_layers(fc.PRODUCT())
    assert ms.plan_rows(40, 48, opts=gpu.make_opts(device=0, band_rows=16)).n_bands == 3
    E, _ = fc.fail_loop(gpu, lambda: fc.PlaneRun(gpu, torch, fc.PRODUCT, x, band_rows=16), LAUNCH, what="launch-three-bands")
    assert E >= 3 * 6


def test_failed_launch_batch_resident(gpu):
    """w2xc_convert_batch_device, n = 3 at 33 x 47: one launch per layer for the three images"""
    x = np.stack([fc.rand_plane(33, 47, 30 + i) - 0.5 for i in range(3)])
    E, _ = fc.fail_loop(gpu, lambda: fc.PlaneRun(gpu, torch, fc.PRODUCT, x), LAUNCH, what="launch-batch")
    assert E >= 6


# ---- the host routes, in children ----
@pytest.mark.parametrize("group", fc.GROUPS)
def test_host_routes_fail_and_recover(gpu, group):
    """tests/fail_cases.py <group>: ALLOC and LAUNCH over the host pipeline's strategies (prog pageable and page-locked; tail32, tail16, first chunks; four
    bands, three units), the host batch in 3 + 3 + 1 sub-batches, the Model::filter chain with filter_resident and a host image call"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(os.path.dirname(os.path.abspath(__file__)), "fail_cases.py"), group]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=TIME_LIMIT_S[group])
    except subprocess.TimeoutExpired as e:
        pytest.fail("group %s did not end within %.0f s -- a thread that does not join, or a wait for a word that never comes; its last lines:\n%s"
                    % (group, TIME_LIMIT_S[group], "\n".join((e.stdout or b"").decode(errors="replace").splitlines()[-5:])))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "group %s: every k passed" % group in r.stdout
