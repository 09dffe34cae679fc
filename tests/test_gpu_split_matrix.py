"""Every instantiation of the 16-bit convolution kernels (csrc/w2xc_split.hip: conv3x3_split 9 shapes x 4 modes x 3 output kinds,
conv3x3_first2_split, conv3x3_first_split) against the float64-accumulated emulation of the engine's dataflow (tests/bf16_ref.py), at the
sizes where these kernels can go wrong: 1x1 and 17x33 (edge tiles, ragged quads) and two planes that make workgroups of the persistent
grid take a second tile (tests/split_matrix.py has the case table and says why each size is there; tests/test_split_emulation.py shows
on the CPU that the table covers every instantiation and that the emulation's dataflow is the library's).

Bounds -- the project's own, set on short models like these (test_split_path_matches_its_emulation, test_bf16_path_matches_its_emulation):
  BF16X3, FP16X2   max |gpu - emu64| <= 2e-5 of the output range (two fp32 summation orders)
  BF16X2           <= 1e-4 (every activation is re-rounded to 16 bits: a last-bit difference of the fp32 sums moves results at 2^-17)
  BF16             max <= 1e-2 and mean <= 1e-3 of the range: a one-ulp bf16 rounding flip (2^-8 relative) is a legitimate difference between
                   two fp32 summation orders.  On the two many-pixel sizes also  mean |gpu - emu64| <= 4 mean |emu32 - emu64| + 2e-6 range,
                   emu32 being the same dataflow with float32 convolutions on the CPU: "the error class of another fp32 order", the construct of
                   test_cfg1_noise1_256.  The gate is measured on the references alone.
Weights and planes: split_matrix.model_plane_reference -- the first of a fixed seed sequence whose REFERENCE output is no near-cancellation
(a 1x1 plane has one output value; where it cancels to 1e-3 of what the last layer sums, an fp32-level error of 3e-8 reads as 3e-5 "of the range").
Each case also runs banded (w2xc_opts.band_rows) and must give the same bytes: band origins take the edge-tile paths at other offsets."""
import numpy as np
import pytest

import bf16_ref
import split_matrix as sm

pytestmark = pytest.mark.gpu

MAX_BOUND = {"bf16": 1e-2, "bf16x2": 1e-4, "bf16x3": 2e-5, "fp16x2": 2e-5}
PARAMS = [pytest.param(c, m, s, id="%s-%s-%s" % (c.id, m, s)) for c in sm.CASES for m in sm.MODES for s in c.sizes]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    return w2xc


def _run(gpu, ms, case, x, opts):
    if case.n_in == 1:
        return ms.convert(x, opts=opts)[None]
    import torch
    n_out, (h, w) = case.planes[-1], x.shape[1:]
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros((n_out, h, w), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    opts.device = 0
    ms.convert_planes_device(case.n_in, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), h * w * 4, w * 4,
                             stream=st.cuda_stream, opts=opts)
    st.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("case,mode,size", PARAMS)
def test_instantiation_matches_the_emulation(gpu, case, mode, size):
    layers, x, want = sm.model_plane_reference(case, mode, size)
    ms = gpu._ModelSet.from_layers(layers)
    prec = sm.precision_of(gpu, mode)
    opts = lambda **kw: gpu.make_opts(precision=prec, fusion=case.fusion, **kw)

    # the intended kernel runs at the intended layer, and every other layer runs what the emulation assumes
    flow = bf16_ref.split_dataflow(case.planes, mode, case.fusion)
    assert [ms.kernel_name(l, opts()) for l in range(ms.n_layers)] == [f[0] for f in flow]
    assert flow[case.layer] == (case.kernel, case.cin, case.cout, sm.terms_of(mode) if case.ot == "T" else case.ot)
    if size in sm.SECOND_TRIP:   # more tiles than the persistent grid has workgroups (256): a later change of tile shape cannot silently undo that
        assert sm.tiles_at(case, mode, size, case.layer) > 256

    xin = x if case.n_in > 1 else x[0]
    got = _run(gpu, ms, case, xin, opts())
    assert got.shape == want.shape and np.isfinite(got).all()
    scale = float(np.abs(want).max())
    diff = np.abs(got.astype(np.float64) - want)
    err, mean = float(diff.max()) / scale, float(diff.mean()) / scale
    tight = mode == "bf16" and size in sm.SECOND_TRIP
    ref32 = None
    if tight:
        want32 = bf16_ref.convert_mode_emulated(layers, x, mode, n_in=case.n_in, fusion=case.fusion, accumulate="float32")
        ref32 = float(np.abs(want32.astype(np.float64) - want).mean()) / scale
    print("SPLITMATRIX %-18s %-7s %-6s max/range %.3g mean/range %.3g%s"
          % (case.id, mode, size, err, mean, "" if ref32 is None else " emu32 mean/range %.3g" % ref32))
    assert err <= MAX_BOUND[mode], (err, scale)
    if mode == "bf16":
        assert mean <= 1e-3, mean
    if tight:
        assert mean <= 4 * ref32 + 2e-6, (mean, ref32)

    # banding is bit-identical by contract; band origins put the edge-tile stores at other rows
    banded = _run(gpu, ms, case, xin, opts(band_rows=8 if size == "tall" else 5))
    assert np.array_equal(got, banded)
