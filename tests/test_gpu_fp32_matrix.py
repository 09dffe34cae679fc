"""Every instantiation of the fp32 convolution kernels, launched by name through a public call and compared with float64 (tests/fp32_matrix.py has the
case table and says why each size is there; tests/test_fp32_matrix.py shows on the CPU that the table names exactly the kernels the build produces).
One test per (case, size):

* launched kernels -- the call runs under torch's profiler, and the set of fp32 convolution keys it reports equals case.keys exactly;
* float sinks, one image -- against the float64 restatement (upconv_ref.chain_z / upconv_ref.reference, oracle.Oracle.convert_f64 for one plane in and
  out) at the project's fp32 gate: conftest.RTOL / ATOL elementwise and max-norm 1e-4 of the reference range;
* the tighter, measured gate -- a baseline that shares no kernel with the case on the same inputs, both against float64:
      ratio = err(kernel) / max(err(baseline), 1 ulp of the range)
  must stay under RATIO_GATE of the case's family, and the F(4x4) families under the project's stated 4e-5 of the range (test_wino4_f4x4_kernel).
  The baseline is the same call with W2XC_KERNEL_DIRECT.  A head model's head runs upconv4x4_head under every option, so its baseline is
  conv3x3_direct on the 3x3 layers alone (convert_planes_device on the model without its head) and torch's fp32 conv_transpose2d on the CPU for the
  head: never the kernel under test.  The case `direct`, the direct kernel itself, is held to the fp32 gate only;
* uint8 sinks -- the bytes equal saturate(rint(255 v)) of the float-sink result v of the same model on u8 / 255 (the float planes call, composed as
  include/w2xc_hip.h defines the image calls: the bleed for the colour of RGBA images, channel 1 of (A, A, A) for alpha, the 8 variants and their fp32
  mean for TTA), which itself passes the fp32 gate against float64;
* batch forms -- image i has the bits of the single-image call, image 0's single-image result passes the fp32 gate;
* every output buffer has a sentinel rim and odd padding, which must survive.

With W2XC_FP32_MATRIX_ERRORS naming a file, the figures of every float case are appended to it; profiles/fp32_matrix_errors.txt is such a run."""
import os

import numpy as np
import pytest

from conftest import RTOL, ATOL
import fp32_matrix as fm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT, GUARD = -7.25, 0xA5
# twice the worst ratio a family recorded in profiles/fp32_matrix_errors.txt (a change of seed moves fp32 rounding error by about that factor),
# rounded up to one digit.  The worst ratios are those of 1x1 planes, where the direct kernel's single value happens to land within one ulp:
#   family   worst recorded ratio   case, size            err / range   direct / range   (largest err / range of the family at any size)
#   mfma2    13.8                   mfma2_128_32 1x1      1.10e-06      7.95e-08         2.62e-06
#   wino      6.63                  wino_32_128 1x1       8.02e-07      1.21e-07         1.02e-06
#   first     2.83                  rgb_64 1x1            2.41e-07      8.51e-08         3.22e-07
#   wino4     3.16                  w4_prog_128_64 4x4    1.66e-06      5.26e-07         2.13e-06
#   first2    6.47                  first2_pp_64 1x1      5.58e-07      4.55e-08         2.90e-06
#   upconv    1.81                  head_64_3 1x1         2.06e-07      1.14e-07         1.82e-06
# (the case `direct` is the direct kernel itself: the fp32 gate alone.  The baseline of a head model runs no upconv4x4_head: baseline() below.)
# A baseline error is 5e-8 .. 2e-6 of the range (typically 3e-7), so a gate of 4 .. 30 allows some 1e-6 .. 2e-5 of it where the fp32 gate allows 1e-4.
RATIO_GATE = {"mfma2": 30, "wino": 20, "wino4": 7, "first": 6, "first2": 20, "upconv": 4}
F4X4_GATE = 4e-5   # of the range: the project's stated max-norm gate of the F(4x4) kernels on short models (tests/test_gpu_winograd.py)
F4X4_FAMILIES = ("wino4", "first2")
PARAMS = [pytest.param(c, s, id="%s-%s" % (c.id, s)) for c in fm.CASES for s in c.sizes]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


_models = {}


def ms_of(gpu, planes, seed, layers, head):
    """one _ModelSet per (topology, head, seed) for the module"""
    key = (tuple(planes), None if head is None else head[0].shape[1], seed)
    if key not in _models:
        _models[key] = gpu._ModelSet.from_layers(layers, head=head)
    return _models[key]


def model_of(gpu, case, seed, layers, head):
    return ms_of(gpu, case.planes, seed, layers, head)


def stream():
    return torch.cuda.current_stream().cuda_stream


def opts_of(gpu, case, **more):
    return gpu.make_opts(device=0, **dict(case.opts, **more))


# ---- the float calls: xs [n, nin, h, w] -> [n, nout, H, W]; rows 3 floats longer than the input planes and 5 longer than the output planes, one more
#      row per output plane, everything outside the planes a sentinel that must survive ----
def run_float(gpu, ms, entry, xs, opts):
    n, nin, h, w = xs.shape
    up = 2 if entry.startswith("up2x") else 1
    nout = ms.planes(ms.n_layers - 1)[1]
    H, W = h * up, w * up
    d_in = torch.full((n, nin, h, w + 3), SENT, dtype=torch.float32, device="cuda")
    d_in[:, :, :, :w] = torch.from_numpy(np.array(xs, np.float32, order="C")).cuda()   # (a copy: a flipped variant has negative strides)
    d_out = torch.full((n, nout, H + 1, W + 5), SENT, dtype=torch.float32, device="cuda")
    i_is, i_ps, i_rs = (4 * s for s in d_in.stride()[:3])
    o_is, o_ps, o_rs = (4 * s for s in d_out.stride()[:3])
    st = stream()
    if entry == "plane":
        assert n == nin == nout == 1
        ms.convert_device(d_in.data_ptr(), i_rs, w, h, d_out.data_ptr(), o_rs, stream=st, opts=opts)
    elif entry == "planes":
        assert n == 1
        ms.convert_planes_device(nin, d_in.data_ptr(), i_ps, i_rs, w, h, d_out.data_ptr(), o_ps, o_rs, stream=st, opts=opts)
    elif entry == "up2x":
        assert n == 1
        ms.convert_planes_up2x_device(nin, d_in.data_ptr(), i_ps, i_rs, w, h, d_out.data_ptr(), o_ps, o_rs, stream=st, opts=opts)
    elif entry == "plane_batch":
        assert nin == nout == 1
        ms.convert_batch_device(n, d_in.data_ptr(), i_is, i_rs, w, h, d_out.data_ptr(), o_is, o_rs, stream=st, opts=opts)
    elif entry == "planes_batch":
        ms.convert_planes_batch_device(n, nin, d_in.data_ptr(), i_is, i_ps, i_rs, w, h, d_out.data_ptr(), o_is, o_ps, o_rs, stream=st, opts=opts)
    elif entry == "up2x_batch":
        ms.convert_planes_up2x_batch_device(n, nin, d_in.data_ptr(), i_is, i_ps, i_rs, w, h, d_out.data_ptr(), o_is, o_ps, o_rs, stream=st, opts=opts)
    else:
        raise ValueError(entry)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:, :, H:, :] == SENT).all() and (out[:, :, :, W:] == SENT).all(), "floats outside the output planes were written"
    assert (d_in[:, :, :, w:] == SENT).all().item(), "the input's padding was written"
    return np.ascontiguousarray(out[:, :, :H, :W])


# ---- the uint8 calls: imgs [n, h, w, ch] -> [n, H, W, ch]; odd row and image strides, everything outside the pixels a guard byte that must survive ----
def run_u8(gpu, ms, case, imgs, opts):
    n, h, w, ch = imgs.shape
    up = 2 if case.head else 1
    H, W = h * up, w * up
    irs, ors = ch * w + 5, ch * W + 3
    iis, ois = irs * h + 17, ors * H + 29
    src = np.full((n, iis), 0x3C, np.uint8)
    for i in range(n):
        np.lib.stride_tricks.as_strided(src[i], (h, ch * w), (irs, 1))[...] = imgs[i].reshape(h, ch * w)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((n, ois), GUARD, dtype=torch.uint8, device="cuda")
    models = dict(noise=None, scale=ms, iterations=1) if case.head else dict(noise=ms, scale=None, iterations=0)
    if case.entry == "rgb_u8":
        assert n == 1
        gpu.process_image_rgb_u8_device(d_in.data_ptr(), irs, w, h, d_out.data_ptr(), ors, stream=stream(), opts=opts, **models)
    elif case.entry == "rgb_u8_batch":
        f = gpu.process_image_rgb_u8_up2x_batch_device if case.head else gpu.process_image_rgb_u8_batch_device
        f(n, d_in.data_ptr(), iis, irs, w, h, d_out.data_ptr(), ois, ors, stream=stream(), opts=opts, **models)
    else:
        gpu.process_image_rgba_u8_up2x_batch_device(n, d_in.data_ptr(), iis, irs, w, h, d_out.data_ptr(), ois, ors, bleed_passes=-1, stream=stream(), opts=opts,
                                                    tta=case.entry == "rgba_u8_tta", **models)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), src), "the input images were written"
    out = d_out.cpu().numpy()
    got = np.empty((n, H, W, ch), np.uint8)
    for i in range(n):
        rows = np.lib.stride_tricks.as_strided(out[i], (H, ch * W), (ors, 1))
        got[i] = rows.reshape(H, W, ch)
        rows[...] = GUARD
    assert (out == GUARD).all(), "bytes outside the output pixels were written"
    return got


def T(k, x):
    """variant k of test-time augmentation (include/w2xc_hip.h): hflip if k & 1, then vflip if k & 2, then transpose if k & 4"""
    if k & 1:
        x = x[..., :, ::-1]
    if k & 2:
        x = x[..., ::-1, :]
    if k & 4:
        x = np.swapaxes(x, -1, -2)
    return np.ascontiguousarray(x)


def Tinv(k, x):
    if k & 4:
        x = np.swapaxes(x, -1, -2)
    if k & 2:
        x = x[..., ::-1, :]
    if k & 1:
        x = x[..., :, ::-1]
    return np.ascontiguousarray(x)


def float_sink(gpu, ms, case, planes, opts):
    """the float planes call of the case's model on x [3, h, w] -> [3, H, W]; TTA: on the 8 variants, each result transformed back, their fp32 sum in
    the order k = 0..7 times 0.125"""
    entry = "up2x" if case.head else "planes"
    if case.entry != "rgba_u8_tta":
        return run_float(gpu, ms, entry, planes[None], opts)[0]
    vs = [Tinv(k, run_float(gpu, ms, entry, T(k, planes)[None], opts)[0]) for k in range(8)]
    a = vs[0] + vs[1]
    for v in vs[2:]:
        a = a + v
    assert a.dtype == np.float32
    return a * np.float32(0.125)


def bled(gpu, img, passes):
    """the colour of an RGBA image after the bleed (w2xc_bleed_rgba_u8_device): [h, w, 3]"""
    h, w, _ = img.shape
    d_in = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    d_out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    gpu.bleed_rgba_u8_device(d_in.data_ptr(), 4 * w, w, h, passes, d_out.data_ptr(), 3 * w, stream=stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def bytes_of_float_sink(gpu, ms, case, img, opts):
    """saturate(rint(255 v)) of the float-sink results of one image [h, w, 3 or 4] -> ([H, W, 3 or 4], [(v, the float planes it was computed from)])"""
    if img.shape[2] == 3:
        x = fm.float_planes(img)
        v = float_sink(gpu, ms, case, x, opts)
        return fm.to_u8(v).transpose(1, 2, 0), [(v, x)]
    x, xa = fm.float_planes(bled(gpu, img, ms.n_layers)), fm.float_planes(np.repeat(img[:, :, 3:4], 3, axis=2))
    v, a = float_sink(gpu, ms, case, x, opts), float_sink(gpu, ms, case, xa, opts)
    return np.concatenate([fm.to_u8(v).transpose(1, 2, 0), fm.to_u8(a[1])[:, :, None]], axis=2), [(v, x), (a, xa)]


def reference_sink(case, layers, head, x):
    """float64: the model on x [3, h, w]; TTA: the mean of the model on the 8 variants, each transformed back"""
    if case.entry != "rgba_u8_tta":
        return fm.reference(layers, head, x)[0]
    return sum(Tinv(k, fm.reference(layers, head, T(k, x))[0]) for k in range(8)) / 8.0


# ---- gates ----
def errors(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    scale = float(np.abs(ref).max())
    return float(err.max()), scale, float((err / (RTOL * np.abs(ref) + ATOL)).max())


def fp32_gate(got, ref, what):
    err, scale, worst = errors(got, ref)
    line = "%s: max|gpu - ref| / max|ref| = %.3g, worst elementwise err / (1e-4 |ref| + 1e-5) = %.3g" % (what, err / scale, worst)
    print(line)
    assert err / scale <= RTOL and worst <= 1.0, line
    return err, scale


ERRORS_HEADER = """# fp32 kernel matrix on one MI355X: W2XC_FP32_MATRIX_ERRORS=<this file> pytest tests/test_gpu_fp32_matrix.py -m gpu (the file is written anew by every
# session).  Every single-image float case at every size: err = max |kernel - float64|, direct = max |baseline - float64| on the same weights and planes, ulp
# = one float32 ulp of the range, all over the reference's range; ratio = err / max(direct, ulp).  The baseline: the same call with W2XC_KERNEL_DIRECT; for
# head models, whose head has one kernel under every option, conv3x3_direct on the 3x3 layers and torch's fp32 conv_transpose2d on the CPU as the head.
# The case `direct` IS the direct kernel and has no line.  RATIO_GATE of the test is twice the worst ratio of a family here, rounded up to one digit.
# The float64 references: upconv_ref.chain_z / upconv_ref.reference, oracle.Oracle.convert_f64 for one plane in and out.
"""
_recorded = []


def record(line):
    print(line)
    path = os.environ.get("W2XC_FP32_MATRIX_ERRORS")
    if path:
        with open(path, "a" if _recorded else "w") as f:
            f.write(("" if _recorded else ERRORS_HEADER) + line + "\n")
        _recorded.append(line)


def baseline(gpu, case, seed, layers, head, xs):
    """the result of the case's model on xs [1, nin, h, w] by code that shares no kernel with the case: W2XC_KERNEL_DIRECT -- and for a head model, whose
    head runs upconv4x4_head whatever w2xc_opts.kernel says (layer_kind), the 3x3 layers alone as a model of their own through convert_planes_device
    with W2XC_KERNEL_DIRECT on the source with one replicated pixel around it (the library pads by the layer count: together the n + 1 pixels of a head
    model), then the head as torch's fp32 conv_transpose2d on the CPU with the bias narrowed to float as the engine narrows it"""
    direct = gpu.make_opts(device=0, kernel=fm.KERNEL_DIRECT)
    if head is None:
        return run_float(gpu, ms_of(gpu, case.planes, seed, layers, None), "plane" if case.entry == "plane" else "planes", xs, direct)[0]
    z = run_float(gpu, ms_of(gpu, case.planes, seed, layers, None), "planes", np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge"), direct)
    hw, hb = head
    bias = None if hb is None else torch.from_numpy(np.asarray(hb).astype(np.float32))
    with torch.no_grad():
        return torch.nn.functional.conv_transpose2d(torch.from_numpy(z), torch.from_numpy(hw), bias, stride=2, padding=3)[0].numpy()


@pytest.mark.parametrize("case,size", PARAMS)
def test_instantiation(gpu, case, size):
    seed, layers, head, src, ref = fm.conditioned(case.id, size)
    ms = model_of(gpu, case, seed, layers, head)
    opts = opts_of(gpu, case)
    what = "%s %s" % (case.id, size)
    assert [ms.kernel_name(l, opts) for l in range(ms.n_layers)] == list(case.layer_names)
    if size in fm.SECOND_TRIP:
        name, items, grid = fm.focus_launch(case, size)
        assert items > grid, (name, items, grid)
    n = 1 if case.entry == "rgba_u8_tta" else case.batch
    srcs = np.stack([src] + [fm.source_of(case, size, seed, i) for i in range(1, n)])

    # the call, under the profiler
    got = []
    if case.entry in fm.U8_ENTRIES:
        names = fm.kernel_names(lambda: got.append(run_u8(gpu, ms, case, srcs, opts)))
    else:
        names = fm.kernel_names(lambda: got.append(run_float(gpu, ms, case.entry, srcs, opts)))
    got = got[0]
    if not any(fm.is_fp32_conv(k) for k in names):
        pytest.fail("the profiler recorded no kernel of the library: %r" % names[:8])
    launched = fm.launched_keys(names)
    assert launched == set(case.keys), "launched but not in the table: %r; in the table but not launched: %r" % (sorted(launched - case.keys), sorted(case.keys - launched))

    if case.entry in fm.U8_ENTRIES:
        for i in range(n):
            want, parts = bytes_of_float_sink(gpu, ms, case, srcs[i], opts)
            if i == 0:   # (the float sink against float64: the conditioned reference where it is that of these planes, else -- bled colour, alpha, TTA -- its own)
                for j, (v, x) in enumerate(parts):
                    plain = j == 0 and case.entry in ("rgb_u8", "rgb_u8_batch")
                    fp32_gate(v, ref if plain else reference_sink(case, layers, head, x), what + " float sink %d" % j)
                inside = (want > 0) & (want < 255)
                assert inside.any() and (inside.mean() >= 0.05 or want.size <= 16), "a saturated image compares nothing"
            assert got[i].shape == want.shape
            assert np.array_equal(got[i], want), (what, i, int((got[i] != want).sum()))
        return

    single = case.entry if case.entry in fm.FLOAT_SINGLE else case.entry[:-len("_batch")]
    if case.entry in fm.FLOAT_BATCH:
        one = [run_float(gpu, ms, single, srcs[i:i + 1], opts)[0] for i in range(n)]
        fp32_gate(one[0], ref, what + " image 0, single call")
        for i in range(n):
            assert np.array_equal(got[i].view(np.uint32), one[i].view(np.uint32)), (what, "image %d differs from the single-image call" % i)
        return

    err, scale = fp32_gate(got[0], ref, what)
    if case.family == "direct":   # (the direct kernel itself: the fp32 gate is its gate, it has no other baseline than float64)
        return
    err_d, _, _ = errors(baseline(gpu, case, seed, layers, head, srcs), ref)
    ulp = float(np.spacing(np.float32(scale)))
    ratio = err / max(err_d, ulp)
    record("%-18s %-6s family %-7s err/range %.3g direct/range %.3g ulp/range %.3g ratio %.3g" % (case.id, size, case.family, err / scale, err_d / scale, ulp / scale, ratio))
    assert err_d / scale <= RTOL, "the baseline itself"
    if case.family in F4X4_FAMILIES:
        assert err / scale <= F4X4_GATE, (what, err / scale)
    assert ratio <= RATIO_GATE[case.family], (what, ratio, RATIO_GATE[case.family])
