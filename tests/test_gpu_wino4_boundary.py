"""conv3x3_wino4 across an item boundary: a workgroup that walks on from one item to the next carries the input transforms in flight (36 values per wave)
through the epilogue in registers, and the fused last layer exchanges an item's taps through LDS that the next item's first stage reuses.

Every case of tests/fp32_matrix.py that is there for a conv3x3_wino4 instantiation of the one-image kernel -- 32 NHWC / 64 / 128 planes in, 64 / 128 out,
planar, NHWC and fused-last (FUSE7) out as the launchers allow, one PROG launch -- on a 272 x 546 plane: every conv3x3_wino4 layer of the case then has
18 x 18 tiles or more, more items than the 256 workgroups of the persistent grid (asserted from the launchers' arithmetic, fm.launch_shape), its right
edge tiles are ragged (546 = 2 mod 32, and 4 mod 32 one layer further in) and -- the layers' first rows are 3 and 2 rows into a 4 x 4 block -- so are
its top and bottom tile rows.  Each case is compared with

* the same call with W2XC_KERNEL_DIRECT, at the fp32 gate of tests/test_gpu_fp32_matrix.py (conftest.RTOL / ATOL elementwise, max-norm 1e-4 of the range);
* the same call cut into two row bands (w2xc_opts.band_rows = 136): the item boundaries then fall on other items, and the results must have the same bits.

The control is a 12 x 30 plane: one tile per 64-plane block, no workgroup runs a second item.  test_direct_alone_is_inside_the_gate rehearses on the CPU,
for the models of every case, that an fp32 direct convolution alone stays inside the gate against float64: what the GPU comparison measures is then
the kernel under test."""
import numpy as np
import pytest

import fp32_matrix as fm
import test_gpu_fp32_matrix as mx   # run_float (sentinel rims), fp32_gate

torch = pytest.importorskip("torch")

H, W = 272, 546
CONTROL = (12, 30)
BAND_ROWS = 136
IDS = (["w4_pn_%d_%d" % (a, b) for a in fm.WIDE for b in fm.WIDE] + ["w4_nn_32_%d" % c for c in fm.WIDE] + ["w4_np_32_%d" % c for c in fm.WIDE]
       + ["w4_f7_%d_%d" % (a, b) for a in fm.WIDE for b in fm.WIDE] + ["w4_f7_32_%d" % c for c in fm.WIDE]
       + ["w4_pp_%d_%d" % (a, b) for a in fm.WIDE for b in fm.WIDE] + ["w4_prog_128_128"])
CASES = [fm.BY_ID[i] for i in IDS]


def wino4_launches(case, h, w):
    """(items, workgroups) of every conv3x3_wino4 layer of the case on an h x w plane (the whole plane one band)"""
    n = fm.n_layers(case)
    out = []
    for k, name in enumerate(case.layer_names, 1):
        if name == "conv3x3_wino4":
            g = 2 * (n - k)
            out.append(fm.launch_shape(name, case.planes[k], h + g, w + g, py=(-(n - k)) & 3))
    return out


def model_and_source(case, h, w):
    seed = fm.seed_of(case)
    layers, _ = fm.model_arrays(case, seed)
    x = np.random.default_rng(seed + 31 * h + w).random((1, case.planes[0], h, w), dtype=np.float32)
    return seed, layers, x


def test_table():
    """the instantiations the cases stand for, and the grid rule on both planes"""
    keys = set()
    for c in CASES:
        assert c.entry in ("plane", "planes") and c.head is None
        keys |= {k for k in c.keys if k[0] == "conv3x3_wino4"}
        big, small = wino4_launches(c, H, W), wino4_launches(c, *CONTROL)
        assert big and all(items > grid for items, grid in big), (c.id, big)            # every conv3x3_wino4 layer crosses an item boundary
        assert small and all(items <= grid for items, grid in small), (c.id, small)     # ... and none does on the control
    for cin in (32, 64, 128):
        for cout in (64, 128):
            nhwc = cin == 32
            assert fm.w4(cin, cout, False, nhwc) in keys and fm.w4(cin, cout, True, nhwc) in keys and fm.w4(cin, cout, True, nhwc, True) in keys, (cin, cout)
    assert fm.w4(128, 128, True, False, True, True) in keys
    assert H % BAND_ROWS == 0 and BAND_ROWS % 4 == 0 and (W % 32, (W + 2) % 32) == (2, 4)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_direct_alone_is_inside_the_gate(case):
    """CPU: the case's model as an fp32 direct convolution (torch) against float64 on a small plane, at the gate the GPU comparison uses"""
    import upconv_ref as ur
    _, layers, x = model_and_source(case, 20, 36)
    n = len(layers)
    ref = ur.chain_z(layers, x[0], n).numpy()
    with torch.no_grad():
        t = torch.nn.functional.pad(torch.from_numpy(x), (n, n, n, n), mode="replicate")
        for _, nout, wt, b in layers:
            bias = torch.from_numpy((np.zeros(nout) if b is None else np.asarray(b)).astype(np.float32))
            t = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(t, torch.from_numpy(wt.astype(np.float32)), bias), 0.1)
    err, scale = mx.fp32_gate(t[0].numpy(), ref, "%s fp32 direct on the CPU" % case.id)
    assert err / scale <= mx.RTOL / 10, "the reference would use up a tenth of the gate itself"


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(H, W), CONTROL], ids=["boundary", "control"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_item_boundary(gpu, case, size):
    h, w = size
    seed, layers, x = model_and_source(case, h, w)
    ms = mx.ms_of(gpu, case.planes, seed, layers, None)
    opts = mx.opts_of(gpu, case)
    assert [ms.kernel_name(l, opts) for l in range(ms.n_layers)] == list(case.layer_names)
    got = mx.run_float(gpu, ms, case.entry, x, opts)[0]
    want = mx.run_float(gpu, ms, case.entry, x, gpu.make_opts(device=0, kernel=fm.KERNEL_DIRECT))[0]
    mx.fp32_gate(got, want.astype(np.float64), "%s %dx%d against conv3x3_direct" % (case.id, h, w))
    banded = mx.run_float(gpu, ms, case.entry, x, mx.opts_of(gpu, case, band_rows=BAND_ROWS if size == (H, W) else 8))[0]
    differ = got.view(np.uint32) != banded.view(np.uint32)
    assert not differ.any(), "%s: %d values differ between one band and two, first at %r" % (case.id, int(differ.sum()), tuple(np.argwhere(differ)[0]))
