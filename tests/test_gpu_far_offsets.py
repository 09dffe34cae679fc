"""Every convolution kernel family on a layer buffer whose byte offsets pass 2^31 and 2^32 (tests/far_offsets.py has the case table, the arithmetic that
places the crossings and the checker; tests/test_far_offsets.py checks them on the CPU).  The kernels form offsets in 32 bits wherever a launcher's rule
or a unit of 16 bytes lets them; a kernel that wraps one reads or writes the wrong rows of a live buffer, and the result is finite and plausible.

Per case, before anything is compared (far_offsets.planned, from w2xc_plan_rows): the call runs in ONE band, the kernels are the table's, every meant
buffer ends past its threshold.  Then:
* the banded twin -- the same call with band_rows = 64, every buffer far below 2^31 -- must have the same bits on the whole plane (the banding contract
  every family here already has: tests/test_gpu_winograd.py, test_gpu_configs.py, test_gpu_parity.py, test_gpu_split_matrix.py, test_gpu_upconv.py).
  Model::filter has no banded form and no such contract: its case is held to the windows alone;
* 48 x 48 windows at the four corners and around the pixels at which a meant buffer crosses 2^31 and 2^32, against float64 of the window's own crop
  (far_offsets.window_reference) at the gate the family has elsewhere: conftest.RTOL / ATOL and max-norm 1e-4, the F(4x4) families also 4e-5, the
  16-bit modes against their emulation (tests/bf16_ref.py) at tests/test_gpu_split_matrix.py's bounds;
* a sentinel rim and odd row padding around input and output survive (the host entry takes contiguous NumPy planes: no rim there);
* the engine's scratch is filled with NaN words (w2xc_debug_fill_scratch) between the twin and the unbanded call: stale rows cannot pass for results.
Device memory is computed per case from the plan and the test's tensors, printed, and capped at 20 GiB; a device with less free memory skips the case
(not an MI355X).  With W2XC_FAR_OFFSETS_RECORD naming a file, one line per case is appended: profiles/far_offsets.txt is such a run.

Left out, held by the arithmetic of tests/test_plan_limits.py only: conv3x3_wino4's planar-input lane offsets above 2^31 (planes of 683 MiB x 64 planes,
about 43 GiB per buffer), PROG's tap-plane rule (a band of 2^30 pixels), and conv3x3_first2_wino4 at its 64-Mi-float cap (layer 3's 64 planes alone
are 17 GiB there; the case runs at the smallest height whose lane offsets pass 2^31, the cap is held on the plan in tests/test_far_offsets.py)."""
import os
import time

import numpy as np
import pytest

from conftest import rand_plane
from oracle import oracle as orc
from tools import gen_model
import bf16_ref
import far_offsets as fo
import upconv_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = -7.25
HEADER = """# Layer buffers past 2^31 / 2^32 bytes on one MI355X: W2XC_FAR_OFFSETS_RECORD=<this file> pytest tests/test_gpu_far_offsets.py -m gpu (written anew by
# every session).  Per case: plane h x w, the meant layers' buffers with their largest byte offset, the threshold, the kernel of every layer, the device bytes
# of the case (plan + tensors), the seconds of the unbanded call, the worst window error against float64 (the 16-bit modes: their emulation) over its
# gate, and whether the banded twin (band_rows = 64) had the same bits.
"""
_recorded = []


def record(line):
    print(line)
    path = os.environ.get("W2XC_FAR_OFFSETS_RECORD")
    if path:
        with open(path, "a" if _recorded else "w") as f:
            f.write(("" if _recorded else HEADER) + line + "\n")
        _recorded.append(line)


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_planes(ms, entry, x, opts):
    """x [nin, h, w] -> [nout, H, W] through a device entry; rows 3 floats longer than the input planes and 5 longer than the output planes, one more row
    per output plane, everything outside the planes a sentinel that must survive (run_float of tests/test_gpu_fp32_matrix.py)"""
    nin, h, w = x.shape
    up = 2 if entry == "up2x" else 1
    nout = ms.planes(ms.n_layers - 1)[1]
    H, W = h * up, w * up
    d_in = torch.full((nin, h, w + 3), SENT, dtype=torch.float32, device="cuda")
    d_in[:, :, :w] = torch.from_numpy(x).cuda()
    d_out = torch.full((nout, H + 1, W + 5), SENT, dtype=torch.float32, device="cuda")
    i_ps, i_rs = (4 * s for s in d_in.stride()[:2])
    o_ps, o_rs = (4 * s for s in d_out.stride()[:2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if entry == "plane":
        ms.convert_device(d_in.data_ptr(), i_rs, w, h, d_out.data_ptr(), o_rs, stream=stream(), opts=opts)
    else:
        ms.convert_planes_up2x_device(nin, d_in.data_ptr(), i_ps, i_rs, w, h, d_out.data_ptr(), o_ps, o_rs, stream=stream(), opts=opts)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert (d_out[:, H:, :] == SENT).all().item() and (d_out[:, :, W:] == SENT).all().item(), "floats outside the output planes were written"
    assert (d_in[:, :, w:] == SENT).all().item(), "the input's padding was written"
    out = d_out[:, :H, :W].contiguous().cpu().numpy()
    del d_in, d_out
    return out, dt


def run(gpu, ms, case, x, **okw):
    opts = gpu.make_opts(device=0, **fo.opts_kw(case, **okw))
    if case.entry == "host":
        t0 = time.perf_counter()
        out = ms.convert(x[0], opts=opts)[None]
        return out, time.perf_counter() - t0
    return run_planes(ms, case.entry, x, opts)


def reference_model(case, layers, head):
    """(the float64 model of a crop, its layer count, its scale)"""
    if case.entry == "filter":
        return (lambda c: upconv_ref.chain_z([layers[case.layer]], c, 1).numpy()), 1, 1
    if case.head:
        return (lambda c: upconv_ref.reference(layers, head, c)), len(layers) + 1, 2
    if case.mode != "fp32":
        return (lambda c: bf16_ref.convert_mode_emulated(layers, c, case.mode, n_in=1)), len(layers), 1
    ref = orc.Oracle(layers)
    return (lambda c: ref.convert_f64(c[0])[None]), len(layers), 1


def worst_over_gate(crops, wins, refs, gates, up):
    """the largest err / bound over the windows (crops: the result inside each), every window's figures printed"""
    worst = 0.0
    for g, (y0, y1, x0, x1), ref in zip(crops, wins, refs):
        e, elem, mean, bound = fo.window_errors(g, ref, gates)
        print("  window rows [%d,%d) columns [%d,%d): err/range %.3g (bound %.3g), worst elementwise err / (1e-4 |ref| + 1e-5) %.3g, mean/range %.3g"
              % (up * y0, up * y1, up * x0, up * x1, e, bound, elem, mean))
        worst = max(worst, e / bound)
    return worst


def describe(case, names, ls, need, dt, worst, twin):
    h, w = case.size
    bufs = ", ".join("layer %d %s %d B" % (k, ls[k - 1].kind, ls[k - 1].bytes - 4) for k in case.meant)
    return "%-12s %5dx%-5d %s > 2^%d  kernels %s  device %.2f GiB  %.3f s  worst window err/gate %.3g  banded twin %s" % (
        case.id, h, w, bufs, 32 if case.threshold == fo.TWO32 else 31, ",".join(names), need / fo.GIB, dt, worst, twin)


def skip_unless_free(need):
    free = torch.cuda.mem_get_info()[0]
    if free < need + 2 * fo.GIB:
        pytest.skip("needs %.1f GiB of device memory plus 2 GiB of headroom; %.1f GiB are free" % (need / fo.GIB, free / fo.GIB))


@pytest.mark.parametrize("case", [c for c in fo.CASES if c.entry != "filter"], ids=[c.id for c in fo.CASES if c.entry != "filter"])
def test_far_buffer(gpu, case):
    layers, head = fo.model_arrays(case)
    ms = gpu._ModelSet.from_layers(layers, head=head)
    plan, names, ls = fo.planned(gpu, ms, case)
    need = fo.device_bytes(case, plan, ls)
    print("%s: %.2f GiB of device memory (workspaces %d + %d bytes)" % (case.id, need / fo.GIB, plan.workspace_bytes[0], plan.workspace_bytes[1]))
    assert need <= fo.CAP_BYTES
    skip_unless_free(need)
    h, w = case.size
    up = 2 if case.head else 1
    x = np.stack([rand_plane(h, w, 77 + i) for i in range(case.planes[0])])
    try:
        twin, _ = run(gpu, ms, case, x, band_rows=64)
        assert ms.fill_scratch(0xFFC00000, device=0) > 0
        got, dt = run(gpu, ms, case, x)
        model, n, _ = reference_model(case, layers, head)
        wins = fo.windows(case, ls)
        refs = [fo.window_reference(model, x, n, win, up=up) for win in wins]
        worst = worst_over_gate([got[:, up * y0:up * y1, up * x0:up * x1] for y0, y1, x0, x1 in wins], wins, refs, case.gates, up)
        same = np.array_equal(got.view(np.uint32), twin.view(np.uint32))
        record(describe(case, names, ls, need, dt, worst, "bit-identical" if same else "DIFFERS"))
        bad = fo.check_plane(got, twin, wins, refs, case.gates, up=up)
        assert not bad, "\n".join(bad)
    finally:
        ms.trim()
        torch.cuda.empty_cache()


def test_far_filter(gpu):
    """Model::filter, 128 -> 128 with the MFMA kernel on planar planes: w2xc_launch_repack both ways and the two NHWC buffers of the filter cache, each
    past 2^32.  The planes are drawn on the device (4 GiB of input), windows of them are read back for the reference."""
    case = fo.BY_ID["filter"]
    layers, head = fo.model_arrays(case)
    ms = gpu._ModelSet.from_layers(layers)
    _, names, ls = fo.planned(gpu, ms, case)
    need = fo.device_bytes(case, None, ls)
    print("%s: %.2f GiB of device memory" % (case.id, need / fo.GIB))
    assert need <= fo.CAP_BYTES
    skip_unless_free(need)
    h, w = case.size
    cin, cout = fo.io_of(case)[case.layer]
    d_in = d_out = None
    try:
        g = torch.Generator(device="cuda").manual_seed(78)
        d_in = torch.full((cin, h, w + 3), SENT, dtype=torch.float32, device="cuda")
        for c in range(cin):
            d_in[c, :, :w] = torch.rand((h, w), generator=g, dtype=torch.float32, device="cuda")
        d_out = torch.full((cout, h + 1, w + 5), SENT, dtype=torch.float32, device="cuda")
        opts = gpu.make_opts(device=0, **fo.opts_kw(case))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms.filter_device(case.layer, cin, d_in.data_ptr(), d_in.stride()[:2] + (1,), w, h, d_out.data_ptr(), d_out.stride()[:2] + (1,), stream=stream(), opts=opts)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert (d_out[:, h:, :] == SENT).all().item() and (d_out[:, :, w:] == SENT).all().item(), "floats outside the output planes were written"
        assert (d_in[:, :, w:] == SENT).all().item(), "the input's padding was written"
        assert torch.isfinite(d_out[:, :h, :w]).all().item()
        model, n, _ = reference_model(case, layers, head)
        wins = fo.windows(case, ls)
        shape = (cin, h, w)

        class Planes:
            pass
        planes = Planes()
        planes.shape = shape
        take = lambda ys, xs: d_in[:, torch.from_numpy(ys).cuda()][:, :, torch.from_numpy(xs).cuda()].cpu().numpy()
        refs = [fo.window_reference(model, planes, n, win, take=take) for win in wins]
        crops = [d_out[:, y0:y1, x0:x1].cpu().numpy() for y0, y1, x0, x1 in wins]
        worst = worst_over_gate(crops, wins, refs, case.gates, 1)
        bad = [win for g, win, ref in zip(crops, wins, refs) if not fo.window_ok(g, ref, case.gates)]
        record(describe(case, names, ls, need, dt, worst, "none (no banded form)"))
        assert not bad, bad
    finally:
        del d_in, d_out
        ms.trim()
        torch.cuda.empty_cache()


def test_refused_plane_leaves_the_model_as_it_was(gpu):
    """[1, 32, 64, 1] at 1 398 144 x 4: conv3x3_wino4 would read NHWC rows with 24 in_rs 4 >= 2^32.  The call is refused by the plan (W2XC_ERR_UNSUPPORTED,
    naming the width) before anything is launched -- the output keeps its sentinel -- and the next call on the model gives the bits it gave before."""
    ms = gpu._ModelSet.from_layers(gen_model.synth_layers(list(fo.REFUSED["planes"]), 4100))
    small = rand_plane(40, 50, 5)
    opts = gpu.make_opts(device=0)
    before = ms.convert(small, opts=opts)
    h, w = fo.REFUSED["size"]
    d_in = torch.from_numpy(rand_plane(h, w, 6)).cuda()
    d_out = torch.full((h, w), SENT, dtype=torch.float32, device="cuda")
    with pytest.raises(gpu.W2xcError) as e:
        ms.convert_device(d_in.data_ptr(), 4 * w, w, h, d_out.data_ptr(), 4 * w, stream=stream(), opts=opts)
    torch.cuda.synchronize()
    assert e.value.code == gpu.ERR_UNSUPPORTED and str(w) in str(e.value), e.value
    assert (d_out == SENT).all().item(), "a refused call wrote output"
    with pytest.raises(gpu.W2xcError) as e:
        ms.convert(np.zeros((h, w), np.float32), opts=opts)
    assert e.value.code == gpu.ERR_UNSUPPORTED
    assert np.array_equal(ms.convert(small, opts=opts).view(np.uint32), before.view(np.uint32))
    del d_in, d_out
    ms.trim()
    torch.cuda.empty_cache()
