"""GPU tests of the batch entry points (w2xc_convert_batch_device / w2xc_convert_batch): every plane of a batch is BIT-identical to the single-plane
call with the same options, the default fp32 chain really runs one launch per layer per sub-batch, the fallback cases stay bit-identical, nothing
outside an output plane is written, and the host form equals the device form."""
import os
import threading

import numpy as np
import pytest

from conftest import assert_close, rand_plane
from tools import gen_model
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@pytest.fixture(scope="module")
def layers():
    return gen_model.synth_layers(seed=gen_model.SEEDS["noise1"])   # trained-like weights


@pytest.fixture(scope="module")
def ms(gpu, layers):
    return gpu._ModelSet.from_layers(layers)


def planes(n, h, w, seed):
    return np.stack([rand_plane(h, w, seed + i) for i in range(n)])


def single(w2xc, ms, x, nn2x=False, opts=None):
    """the single-plane device call, plane by plane"""
    h, w = x.shape[1:]
    up = 1 if nn2x else 0
    o = opts if opts is not None else w2xc.make_opts(device=0)
    out = np.empty((x.shape[0], h << up, w << up), np.float32)
    st = torch.cuda.current_stream()
    for i in range(x.shape[0]):
        d_in = torch.from_numpy(np.ascontiguousarray(x[i])).cuda()
        d_out = torch.empty((h << up, w << up), dtype=torch.float32, device="cuda")
        f = ms.convert_nn2x_device if nn2x else ms.convert_device
        f(d_in.data_ptr(), w * 4, w, h, d_out.data_ptr(), (w << up) * 4, stream=st.cuda_stream, opts=o)
        st.synchronize()
        out[i] = d_out.cpu().numpy()
    return out


def batch(w2xc, ms, x, nn2x=False, opts=None):
    n, h, w = x.shape
    up = 1 if nn2x else 0
    o = opts if opts is not None else w2xc.make_opts(device=0)
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.empty((n, h << up, w << up), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    ms.convert_batch_device(n, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), (h << up) * (w << up) * 4, (w << up) * 4,
                            nn2x=nn2x, stream=st.cuda_stream, opts=o)
    st.synchronize()
    return d_out.cpu().numpy()


def launches(w2xc, ms, fn):
    ms.profile_reset(0)
    fn()
    torch.cuda.synchronize()
    return ms.profile_read(0)[1]


@pytest.mark.parametrize("nn2x", [False, True])
def test_batch_is_bit_identical_to_single_calls(gpu, ms, nn2x):
    x = planes(5, 256, 256, 100)
    got, want = batch(gpu, ms, x, nn2x), single(gpu, ms, x, nn2x)
    assert float(np.abs(got - want).max()) == 0.0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("hw", [(1, 1), (17, 19), (33, 47), (40, 70), (29, 100)])
@pytest.mark.parametrize("n", [1, 3])
def test_odd_shapes_bit_identical(gpu, ms, hw, n):
    x = planes(n, hw[0], hw[1], 7 * n + hw[0])
    assert np.array_equal(batch(gpu, ms, x), single(gpu, ms, x))


def test_golden_fixtures_batched(gpu):
    """the committed fixtures (the reference's own outputs) through the batch entry point: a batch of the fixture's input and two other planes"""
    for f in sorted(os.listdir(GOLDEN)):
        if not f.endswith(".npz"):
            continue
        g = np.load(os.path.join(GOLDEN, f))
        lay = gen_model.synth_layers([int(v) for v in g["planes"]], int(g["seed"]), init=str(g["init"]) if "init" in g else "he_leaky")
        m = gpu._ModelSet.from_layers(lay)
        x = np.stack([g["input"], g["input"][::-1].copy(), g["input"] * 0.5])
        got = m.convert_batch(x)
        assert_close(got[0], g["output"], f)
        assert np.array_equal(got, single(gpu, m, x)), f


def test_one_launch_per_layer(gpu, ms):
    x = planes(16, 256, 256, 300)
    o = gpu.make_opts(device=0, profile=1)
    per_plane = launches(gpu, ms, lambda: single(gpu, ms, x, opts=o))
    batched = launches(gpu, ms, lambda: batch(gpu, ms, x, opts=o))
    assert per_plane == [0] + [16] * 6, per_plane
    assert batched == [0] + [1] * 6, batched


def test_small_workspace_sub_batches_and_fallback_band(gpu, ms):
    x = planes(6, 256, 256, 400)
    o = gpu.make_opts(device=0, profile=1, workspace_mb=160)
    got = None

    def run():
        nonlocal got
        got = batch(gpu, ms, x, opts=o)
    cnt = launches(gpu, ms, run)
    assert 1 < cnt[1] < 6 and len(set(cnt[1:])) == 1, cnt   # several sub-batches, each one launch per layer
    assert np.array_equal(got, single(gpu, ms, x, opts=o))
    # a plane larger than one band under this budget: the single-plane sequence per image (several bands each)
    y = planes(2, 640, 512, 500)
    o2 = gpu.make_opts(device=0, profile=1, workspace_mb=96)
    got2 = []
    cnt = launches(gpu, ms, lambda: got2.append(batch(gpu, ms, y, opts=o2)))
    assert cnt[1] > 2, cnt
    assert np.array_equal(got2[0], single(gpu, ms, y, opts=o2))


@pytest.mark.parametrize("kw", [dict(precision=2), dict(kernel=1), dict(fusion=1), dict(fusion=5), dict(kernel=4)])
def test_fallback_option_sets_bit_identical(gpu, ms, kw):
    x = planes(3, 40, 52, 600)
    o = gpu.make_opts(device=0, **kw)
    assert np.array_equal(batch(gpu, ms, x, opts=o), single(gpu, ms, x, opts=o))


@pytest.mark.parametrize("nn2x", [False, True])
def test_strided_outputs_guard_untouched(gpu, ms, nn2x):
    n, h, w = 3, 45, 70
    up = 1 if nn2x else 0
    H, W = h << up, w << up
    x = planes(n, h, w, 700)
    rs, rows = W + 13, H + 5                      # 13 guard columns per row, 5 guard rows per plane (2 above, 3 below)
    buf = torch.full((n, rows, rs), float("nan"), dtype=torch.float32, device="cuda")
    d_in = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream()
    ms.convert_batch_device(n, d_in.data_ptr(), h * w * 4, w * 4, w, h, buf.data_ptr() + 2 * rs * 4, rows * rs * 4, rs * 4, nn2x=nn2x,
                            stream=st.cuda_stream, opts=gpu.make_opts(device=0))
    st.synchronize()
    b = buf.cpu().numpy()
    assert np.array_equal(b[:, 2:2 + H, :W], single(gpu, ms, x, nn2x))
    guard = np.ones(b.shape, bool)
    guard[:, 2:2 + H, :W] = False
    assert np.isnan(b[guard]).all()


def test_host_form_equals_device_form(gpu, ms):
    x = planes(9, 96, 80, 800)
    want = batch(gpu, ms, x)
    # pageable list
    assert np.array_equal(ms.convert_batch([x[i] for i in range(len(x))]), want)
    # an (n, h, w) array, device_mask = device 0 only
    assert np.array_equal(ms.convert_batch(x, opts=gpu.make_opts(device_mask=1)), want)
    # page-locked planes in and out: DMA'd in place
    pin_in = torch.from_numpy(x.copy()).pin_memory()
    pin_out = torch.empty((len(x), 96, 80), dtype=torch.float32).pin_memory()
    ms.convert_batch(pin_in.numpy(), out=pin_out.numpy())
    assert np.array_equal(pin_out.numpy(), want)
    # nn2x
    assert np.array_equal(ms.convert_batch(x[:4], nn2x=True), batch(gpu, ms, x[:4], nn2x=True))


def test_two_threads_batching_on_one_model(gpu, ms):
    a, b = planes(6, 128, 96, 900), planes(5, 128, 96, 950)
    want = [ms.convert_batch(a), ms.convert_batch(b)]
    got = [None, None]

    def run(i, x):
        got[i] = ms.convert_batch(x)
    th = [threading.Thread(target=run, args=(0, a)), threading.Thread(target=run, args=(1, b))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_batch_of_64x64_matches_oracle(gpu, ms, layers):
    x = planes(8, 64, 64, 1000)
    got = ms.convert_batch(x)
    ref = orc.Oracle(layers)
    for i in range(len(x)):
        assert_close(got[i], ref.convert(x[i]), "plane %d" % i)


# ---- image offsets at and past 2^32 bytes: the batch forms move only 64-bit scalar bases (image x stride) ---------------------------------------
GIB = 1 << 30


def need_free_memory(need_bytes, what):
    """the one route to a skip in the two tests below: a device with less free memory than the test needs plus 4 GiB (not an MI355X: 288 GB)"""
    free = torch.cuda.mem_get_info()[0]
    if free < need_bytes + 4 * GIB:
        pytest.skip("%s needs %.1f GiB of device memory plus 4 GiB of headroom; %.1f GiB are free" % (what, need_bytes / GIB, free / GIB))


def test_batch_workspace_blocks_beyond_4gib(gpu, ms, layers):
    """ONE sub-batch whose per-image workspace blocks reach past 4 GiB in BOTH workspaces: 256 x 256 planes, as many as put the last image's block of
    the smaller workspace 2^32 + 2^28 bytes in.  Every image has its own seed, so an image offset that wraps at 32 bits lands on ANOTHER image's
    activations.  Bit-identical to the single-plane calls for every image; image 0, the images whose blocks straddle 2^32 in either workspace and
    the last image also against the oracle."""
    h = w = 256
    plan = ms.plan_rows(w, h, opts=gpu.make_opts(device=0))
    assert plan.n_bands == 1 and min(plan.workspace_bytes) > 0
    n = -(-((1 << 32) + (1 << 28)) // int(min(plan.workspace_bytes)))
    blk = [((int(b) + 3) // 4 + 63) // 64 * 64 * 4 for b in plan.workspace_bytes]   # batch_ws_floats: every image's block on a 256-byte boundary
    per = sum(blk)
    mb = 0 if (16384 << 20) // per >= n else (n * per + (1 << 20) - 1) >> 20        # batch_sub_size: all n images in one sub-batch
    assert all((n - 1) * b >= 1 << 32 for b in blk), (n, blk)
    need_free_memory(n * per + 2 * n * h * w * 4, "test_batch_workspace_blocks_beyond_4gib")
    print("n = %d images, workspace blocks %s bytes per image, %.2f GiB of workspace, workspace_mb = %d" % (n, blk, n * per / GIB, mb))
    x = planes(n, h, w, 5000)
    try:
        o = gpu.make_opts(device=0, profile=1, workspace_mb=mb)
        got = []
        cnt = launches(gpu, ms, lambda: got.append(batch(gpu, ms, x, opts=o)))
        got = got[0]
        assert cnt == [0] + [1] * 6, cnt     # one launch per layer: one sub-batch holds all n images
        assert np.isfinite(got).all()
        want = single(gpu, ms, x, opts=gpu.make_opts(device=0, workspace_mb=mb))
        bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
        assert not bad, "images %s differ from the single-plane call (blocks %s bytes)" % (bad, blk)
        ref = orc.Oracle(layers)
        for i in sorted({0, n - 1} | {(1 << 32) // b for b in blk}):
            assert_close(got[i], ref.convert(x[i], njob=8), "image %d" % i)
    finally:
        ms.trim()      # (the module's model: do not leave 13 GiB of workspace to the tests that follow)


@pytest.mark.parametrize("nn2x", [False, True])
def test_batch_plane_strides_beyond_4gib(gpu, ms, nn2x):
    """n = 3 planes of 64 x 80 whose input and output plane strides are 2.2 GiB: plane 1 starts past 2^31 bytes, plane 2 past 2^32.  NaN everywhere
    outside the planes, in the input buffer too.  Bit-identical to the single calls; the guard is still NaN in a window around every output plane."""
    n, h, w = 3, 64, 80
    up = 1 if nn2x else 0
    H, W = h << up, w << up
    stride_f = 590558004            # floats: 2.2 GiB, a multiple of 4 floats
    lead = 4096                     # guard floats in front of plane 0
    need_free_memory(2 * n * stride_f * 4, "test_batch_plane_strides_beyond_4gib")
    x = planes(n, h, w, 6000)
    d_in = d_out = None
    try:
        d_in = torch.full((n * stride_f,), float("nan"), dtype=torch.float32, device="cuda")
        d_out = torch.full((n * stride_f,), float("nan"), dtype=torch.float32, device="cuda")
        for i in range(n):
            d_in[lead + i * stride_f: lead + i * stride_f + h * w] = torch.from_numpy(x[i].ravel()).cuda()
        st = torch.cuda.current_stream()
        ms.convert_batch_device(n, d_in.data_ptr() + lead * 4, stride_f * 4, w * 4, w, h, d_out.data_ptr() + lead * 4, stride_f * 4, W * 4,
                                nn2x=nn2x, stream=st.cuda_stream, opts=gpu.make_opts(device=0))
        st.synchronize()
        want = single(gpu, ms, x, nn2x)
        for i in range(n):
            a = lead + i * stride_f
            win = d_out[a - lead: a + H * W + lead].cpu().numpy()      # the plane and 4096 floats on either side
            assert np.array_equal(win[lead: lead + H * W].reshape(H, W), want[i]), "plane %d" % i
            assert np.isnan(win[:lead]).all() and np.isnan(win[lead + H * W:]).all(), "plane %d: the guard around it was written" % i
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()
