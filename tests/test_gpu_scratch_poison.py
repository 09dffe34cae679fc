"""GPU tests on POISONED scratch memory (run with -m gpu on an MI355X).

The engine's scratch buffers -- the two activation workspaces, Model::filter's planes, the host pipeline's device rows, staging rings and page-locked
band buffers, the image planes -- are allocated once per (model, device), only grow, and are never cleared.  A bit-identity test that runs the same
plane twice through the same addresses therefore cannot see a kernel that reads a pad column, a halo row nobody produced, a tap row past out_h or
the neighbouring image's block: the read finds the previous call's (right) value.  Here every call runs three times, after w2xc_debug_fill_scratch
has filled EVERY scratch buffer with zeros, with quiet NaNs and with 1e30f (a large finite value survives every form LeakyReLU is written in; a NaN
need not pass a min / max / med3 instruction), and the three results must be equal bit for bit: a kernel that reads only what was written cannot see
the fill.  So that three runs cannot be identically wrong, the first is also checked against the CPU oracle (the project's fp32 gate, conftest
.assert_close: rtol 1e-4 + atol 1e-5 and max-norm 1e-4; the 16-bit precisions against their stated bounds of tests/test_gpu_parity.py).

Only DATA is poisoned.  Synchronisation words (job counters, job flags, events) are neither filled nor faked: a wrong value there could only make a
launch wait for ever."""
import numpy as np
import pytest

from conftest import assert_close, ramp_plane, rand_plane, small_layers
from tools import gen_model
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f
PRODUCT = [1, 32, 32, 64, 64, 128, 128, 1]     # the topology of the shipped models


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    assert np.float32(1e30).view(np.uint32) == WORDS[2] and np.isnan(np.uint32(WORDS[1]).view(np.float32))
    return w2xc


@pytest.fixture(scope="module")
def layers():
    return gen_model.synth_layers(seed=gen_model.SEEDS["noise1"])   # trained-like weights, the product topology


@pytest.fixture(scope="module")
def ms(gpu, layers):
    return gpu._ModelSet.from_layers(layers)


@pytest.fixture(scope="module")
def ref(layers):
    return orc.Oracle(layers)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def poisoned_runs(ms, call, plan=None, also=()):
    """call() after each of the three fills of every scratch buffer of `ms` (and of the models in `also`) on device 0: finite and bit-identical"""
    for _ in range(2):         # warm: every buffer this call needs exists at its final size (buffers only grow).  Twice: Model::filter's device
        call()                 # planes ping-pong from call to call, so the second call is the first to size the other one of each pair
    outs, filled = [], []
    for word in WORDS:
        filled.append(ms.fill_scratch(word, 0))
        for other in also:
            assert other.fill_scratch(word, 0) > 0
        outs.append(np.array(call()))
    assert filled[0] > 0 and len(set(filled)) == 1, filled    # something was filled; nothing was reallocated in between
    if plan is not None:
        assert filled[0] >= plan.workspace_bytes[0] + plan.workspace_bytes[1], (filled, list(plan.workspace_bytes))   # the workspaces are among it
    for word, o in zip(WORDS, outs):
        assert np.isfinite(o).all(), "fill %#x: %d non-finite values" % (word, int((~np.isfinite(o)).sum()))
    for word, o in zip(WORDS[1:], outs[1:]):
        diff = bits(o) != bits(outs[0])
        assert not diff.any(), "fill %#x changes %d values, first at %s (max |diff| %g)" % (
            word, int(diff.sum()), tuple(int(v[0]) for v in np.nonzero(diff)), float(np.abs(o.astype(np.float64) - outs[0]).max()))
    return outs[0]


def up2(x):
    return np.repeat(np.repeat(x, 2, 0), 2, 1)


def dev_convert(gpu, ms, x, nn2x=False, **okw):
    """the device-pointer entry points on a resident plane"""
    h, w = x.shape
    up = 1 if nn2x else 0
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.empty((h << up, w << up), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    f = ms.convert_nn2x_device if nn2x else ms.convert_device
    f(d_in.data_ptr(), w * 4, w, h, d_out.data_ptr(), (w << up) * 4, stream=st.cuda_stream, opts=gpu.make_opts(device=0, **okw))
    st.synchronize()
    return d_out.cpu().numpy()


def whole_plan(gpu, ms, x, nn2x=False, **okw):
    return ms.plan_rows(x.shape[1] << int(nn2x), x.shape[0] << int(nn2x), opts=gpu.make_opts(device=0, **okw))


def launches(ms, fn):
    ms.profile_reset(0)
    out = fn()
    torch.cuda.synchronize()
    return out, ms.profile_read(0)[1]


# ---- a. the resident chain, default fp32 -----------------------------------------------------------------------------------------------------------
MODELS_A = [PRODUCT, [1, 32, 32, 64, 64, 1], [1, 32, 64, 128, 64, 1], [1, 32, 128, 128, 1], [1, 64, 128, 1]]
SIZES_A = [
    (1, 1),        # one pixel: every tile is all padding
    (5, 3),        # narrower than one pixel quad, shorter than one 4x4 block
    (16, 32),      # exactly one 32-float planar row, whole blocks: the no-ragged-edge control
    (17, 33),      # one row / one column into the next block and the next 32-float row
    (37, 61),      # w = 1 mod 4
    (40, 62),      # w = 2 mod 4
    (40, 63),      # w = 3 mod 4: the 16-byte quad stores run one float past out_w
    (40, 257),     # one column into a second 256-column gather-job group
    (129, 257),    # one row into a ninth 16-row tile row and the second job group
    (131, 2051),   # more than 64 tiles across: the strip walk, XCD bands of unequal width
    (333, 1000),   # many tile rows, h = 1 mod 4
]
ORACLE_MAX_PIXELS = 350000   # output planes up to this size are also converted by the CPU oracle (every size for the plain call; nn2x up to 129 x 257)


@pytest.mark.parametrize("hw", SIZES_A, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("planes", MODELS_A, ids=lambda p: "-".join(map(str, p)))
def test_resident_chain(gpu, planes, hw):
    lay = small_layers(planes, 40 + len(planes) + planes[-2])
    m, o = gpu._ModelSet.from_layers(lay), orc.Oracle(lay)
    h, w = hw
    for nn2x, x in ((False, rand_plane(h, w, 3 * h + w) - 0.5), (True, ramp_plane(h, w))):   # signed noise; the asymmetric ramp
        got = poisoned_runs(m, lambda: dev_convert(gpu, m, x, nn2x), whole_plan(gpu, m, x, nn2x))
        if got.size <= ORACLE_MAX_PIXELS:
            assert_close(got, o.convert(up2(x) if nn2x else x, njob=8), "%s %dx%d nn2x=%d" % (planes, h, w, nn2x))


@pytest.mark.parametrize("hw", [(40, 63), (129, 257), (333, 1000)], ids=lambda s: "%dx%d" % s)   # ragged quad store; second job group; many bands of a wide plane
@pytest.mark.parametrize("band", ["rows16", "rows100", "small_workspace"])
def test_resident_chain_banded(gpu, ms, ref, band, hw):
    h, w = hw
    x = rand_plane(h, w, 11 + h) - 0.5
    want = ref.convert(x, njob=8)
    if band == "small_workspace":
        kw = dict(workspace_mb=32 if h > 200 else 8 if h > 100 else 1)   # 21, 11 and 10 bands by w2xc_plan_rows
        assert whole_plan(gpu, ms, x, **kw).n_bands >= 3
    else:
        kw = dict(band_rows=int(band[4:]))
    plan = whole_plan(gpu, ms, x, **kw)
    got = poisoned_runs(ms, lambda: dev_convert(gpu, ms, x, **kw), plan)
    assert_close(got, want, "%s %dx%d" % (band, h, w))
    assert np.array_equal(got, dev_convert(gpu, ms, x)), "banding changes the fp32 result"


@pytest.mark.parametrize("halo", ["wide", "minimum"])
def test_row_shards(gpu, ms, ref, halo):
    """w2xc_convert_rows_device: three shards of one plane, each on its own view, with the wide halo (4 rows per layer, default kernels) and with
    the minimum halo under a named kernel"""
    h, w, parts = 131, 257, 3    # shard edges off every block grid (131 = 43 + 44 + 44), one column into the second job group
    x = ramp_plane(h, w) - 3.0
    kw = {} if halo == "wide" else dict(kernel=gpu.KERNEL_WINOGRAD32)
    o = gpu.make_opts(device=0, **kw)
    st = torch.cuda.current_stream()

    def call():
        out = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
        for p in range(parts):
            ra, rb = gpu.shard_rows(h, parts, p)
            y0, y1 = gpu.shard_view(h, ra, rb, (4 if halo == "wide" else 1) * ms.n_layers)
            view = torch.from_numpy(np.ascontiguousarray(x[y0:y1])).cuda()
            ms.convert_rows_device(view.data_ptr(), w * 4, y1 - y0, y0, w, h, ra, rb, out[ra:].data_ptr(), w * 4, stream=st.cuda_stream, opts=o)
        st.synchronize()
        return out.cpu().numpy()
    got = poisoned_runs(ms, call)
    assert_close(got, ref.convert(x, njob=8), "row shards, %s halo" % halo)
    assert np.array_equal(got, dev_convert(gpu, ms, x, **kw)), "the shards do not stitch to the whole-plane call"


# ---- b. every kernel, fusion and precision option ----------------------------------------------------------------------------------------------------
OPTION_SIZES = [(40, 63), (40, 257)]   # w = 3 mod 4 (quad stores past out_w); w = 1 mod 4, one column into the second 256-column job group


@pytest.mark.parametrize("hw", OPTION_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("opt", ["kernel=DIRECT", "kernel=MFMA", "kernel=WINOGRAD32", "kernel=WINOGRAD4", "fusion=OFF", "fusion=FIRST", "fusion=LAST",
                                 "fusion=ON", "fusion=GATHER_LAUNCH", "fusion=PROG"])
def test_kernel_and_fusion_options(gpu, ms, ref, opt, hw):
    field, name = opt.split("=")
    kw = {field: getattr(gpu, field.upper() + "_" + name)}
    h, w = hw
    for nn2x, x in ((False, rand_plane(h, w, 5 * h + w) - 0.5), (True, ramp_plane(h // 2, (w + 1) // 2))):
        got = poisoned_runs(ms, lambda: dev_convert(gpu, ms, x, nn2x, **kw), whole_plan(gpu, ms, x, nn2x, **kw))
        want = ref.convert(up2(x) if nn2x else x, njob=8)
        assert_close(got, want, "%s %dx%d nn2x=%d" % (opt, h, w, nn2x))
        if name == "DIRECT":
            assert np.array_equal(got, want)   # (the reference-ordered kernel: the oracle's bits)


def psnr(a, b, peak=1.0):
    return 10.0 * np.log10(peak * peak / max(float(np.mean((a.astype(np.float64) - b) ** 2)), 1e-30))


def assert_16bit_bound(gpu, mode, got, want, what):
    """the stated accuracy of the 16-bit precisions against the fp32 oracle on [0, 1) planes of the 7-layer topology (tests/test_gpu_parity.py:
    test_bf16_vs_fp32_oracle_accuracy_statement, test_split_vs_fp32_oracle_accuracy_statement)"""
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print("%s %s: max err %.3g, / range %.3g, PSNR %.1f dB" % (mode, what, err, err / scale, psnr(got, want)))
    if mode == "BF16":
        assert err <= 2e-2 and psnr(got, want) >= 45.0, (what, err, psnr(got, want))
    else:
        assert err <= (2e-4 if mode == "BF16X2" else 2e-5) * scale, (what, err, scale)


@pytest.mark.parametrize("mode", ["BF16", "BF16X2", "BF16X3", "FP16X2"])
def test_precision_options(gpu, scale_layers, mode):
    m, o = gpu._ModelSet.from_layers(scale_layers), orc.Oracle(scale_layers)
    kw = dict(precision=getattr(gpu, "PRECISION_" + mode))
    # (96, 128): the plane the stated bounds were written for; then the two ragged widths, signed and as the fused nearest 2x
    x = rand_plane(96, 128, 3)
    got = poisoned_runs(m, lambda: dev_convert(gpu, m, x, **kw), whole_plan(gpu, m, x, **kw))
    assert_16bit_bound(gpu, mode, got, o.convert(x, njob=8), "96x128")
    for (h, w) in OPTION_SIZES:
        y = rand_plane(h, w, 7 * h + w)
        got = poisoned_runs(m, lambda: dev_convert(gpu, m, y, **kw), whole_plan(gpu, m, y, **kw))
        assert_16bit_bound(gpu, mode, got, o.convert(y, njob=8), "%dx%d" % (h, w))
        for nn2x, z in ((False, y - 0.5), (True, ramp_plane(h // 2, (w + 1) // 2))):
            poisoned_runs(m, lambda: dev_convert(gpu, m, z, nn2x, **kw), whole_plan(gpu, m, z, nn2x, **kw))
        poisoned_runs(m, lambda: dev_convert(gpu, m, y - 0.5, band_rows=16, **kw))


# ---- c. the host entry points and every launch strategy of w2xc_rows.cpp -------------------------------------------------------------------------
def host_convert(gpu, ms, x, nn2x=False, pinned=False, **okw):
    o = gpu.make_opts(profile=1, **okw)
    if not pinned:
        return ms.convert_nn2x(x, opts=o) if nn2x else ms.convert(x, opts=o)
    h, w = x.shape
    up = 1 if nn2x else 0
    pin_in = torch.from_numpy(x.copy()).pin_memory()
    pin_out = torch.full((h << up, w << up), float("nan")).pin_memory()
    import ctypes as C
    lib = gpu.lib()
    if nn2x:
        rc = lib.w2xc_convert_plane_nn2x(ms.handle, pin_in.data_ptr(), w * 4, w, h, pin_out.data_ptr(), (w << up) * 4, C.byref(o))
    else:
        rc = lib.w2xc_convert_plane(ms.handle, pin_in.data_ptr(), w * 4, w, h, pin_out.data_ptr(), w * 4, 1, C.byref(o))
    assert rc == 0, gpu.last_error()
    return pin_out.numpy().copy()


def host_case(gpu, ms, ref, x, nn2x=False, pinned=False, **okw):
    """one host call through poisoned_runs, with the launch counts of its last run; == the resident call bit for bit, and the oracle"""
    cnt = []

    def call():
        out, c = launches(ms, lambda: host_convert(gpu, ms, x, nn2x, pinned, **okw))
        cnt[:] = c
        return out
    got = poisoned_runs(ms, call)
    dkw = {k: v for k, v in okw.items() if not k.startswith("host_")}
    assert np.array_equal(got, dev_convert(gpu, ms, x, nn2x, **dkw)), "host != resident"
    if ref is not None:
        assert_close(got, ref.convert(up2(x) if nn2x else x, njob=8), "host %s" % okw)
    return got, cnt


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_prog(gpu, ms, ref, pinned):
    """prog_eligible: a default host call where layer n - 1 has 128 inputs -- ONE launch of layer n - 1, which finishes the last layer itself (no
    gather launch) and writes the rows into pin_band (pageable planes) or into the caller's page-locked plane"""
    n = ms.n_layers
    for nn2x, x in ((False, rand_plane(301, 423, 5) - 0.5), (True, ramp_plane(150, 211))):   # 301 = 1 mod 4 rows, 423 = 3 mod 4 columns, two job groups
        _, cnt = host_case(gpu, ms, ref, x, nn2x, pinned)
        assert cnt[n - 2] == 1 and cnt[n - 1] == 0, cnt


def test_host_prog_64_inputs(gpu):
    """prog_eligible with 64 inputs in layer n - 1"""
    lay = small_layers([1, 32, 32, 64, 64, 1], 61)
    m = gpu._ModelSet.from_layers(lay)
    _, cnt = host_case(gpu, m, orc.Oracle(lay), rand_plane(301, 423, 6) - 0.5)
    assert cnt[m.n_layers - 2] == 1 and cnt[m.n_layers - 1] == 0, cnt


@pytest.mark.parametrize("fusion", ["GATHER_LAUNCH", "OFF"])
def test_host_tail32(gpu, ms, ref, fusion):
    """tail32_eligible: fp32, no PROG, a band of >= 256 rows -- layer n - 1 and the last layer (the gather / conv3x3_last) together in row chunks"""
    n = ms.n_layers
    _, cnt = host_case(gpu, ms, ref, rand_plane(301, 423, 7) - 0.5, fusion=getattr(gpu, "FUSION_" + fusion))
    assert cnt[n - 2] > 1 and cnt[n - 1] > 1, cnt


@pytest.mark.parametrize("mode", ["FP16X2", "BF16X3"])
def test_host_tail16(gpu, scale_layers, mode):
    """tail16_eligible: a 16-bit precision, a band of >= 128 rows -- conv3x3_split of layer n - 1 and its gather together in row chunks"""
    m = gpu._ModelSet.from_layers(scale_layers)
    n = m.n_layers
    x = rand_plane(301, 423, 8)
    got, cnt = host_case(gpu, m, None, x, precision=getattr(gpu, "PRECISION_" + mode))
    assert cnt[n - 2] > 1 and cnt[n - 1] > 1, cnt
    assert_16bit_bound(gpu, mode, got, orc.Oracle(scale_layers).convert(x, njob=8), "host 301x423")
    host_case(gpu, m, None, x - 0.5, precision=getattr(gpu, "PRECISION_" + mode))


def test_host_first_and_last_chunks(gpu, ms, ref):
    """first_chunks_eligible (layer 1, or layers 1 + 2 in one launch, in row chunks behind the upload: 16 KiB slices of a >= 300-row plane) and
    last_chunks_eligible (the last layer in row chunks: where neither prog nor a tail strategy takes layer n - 1)"""
    n = ms.n_layers
    x = rand_plane(301, 423, 9) - 0.5
    _, cnt = host_case(gpu, ms, ref, x, host_chunk_kb=16)                                    # conv3x3_first2_wino4 chunked; then prog
    assert cnt[0] == 0 and cnt[1] > 1 and cnt[n - 2] == 1, cnt
    got, cnt = host_case(gpu, ms, ref, x, host_chunk_kb=16, kernel=gpu.KERNEL_DIRECT)         # conv3x3_direct: layer 1 and the last layer chunked
    assert cnt[0] > 1 and cnt[n - 1] > 1 and cnt[1:n - 1] == [1] * (n - 2), cnt
    assert np.array_equal(got, ref.convert(x, njob=8))
    y = ramp_plane(200, 423)                                                                 # < 256 rows: no tail32 -- the gather in chunks
    _, cnt = host_case(gpu, ms, ref, y, host_chunk_kb=16, fusion=gpu.FUSION_GATHER_LAUNCH)
    assert cnt[1] > 1 and cnt[n - 2] == 1 and cnt[n - 1] > 1, cnt
    _, cnt = host_case(gpu, ms, ref, y, host_chunk_kb=16, fusion=gpu.FUSION_OFF)             # conv3x3_first and conv3x3_last in chunks
    assert cnt[0] > 1 and cnt[n - 2] == 1 and cnt[n - 1] > 1, cnt
    _, cnt = host_case(gpu, ms, ref, ramp_plane(150, 211), nn2x=True, host_chunk_kb=16)
    assert cnt[1] > 1, cnt


@pytest.mark.parametrize("hw", [(1, 1), (17, 33), (40, 63)], ids=lambda s: "%dx%d" % s)   # run_plain: planes too short for any chunked strategy
def test_host_plain(gpu, ms, ref, hw):
    for kw in ({}, dict(fusion=gpu.FUSION_GATHER_LAUNCH), dict(fusion=gpu.FUSION_OFF)):
        _, cnt = host_case(gpu, ms, ref, rand_plane(hw[0], hw[1], 10) - 0.5, **kw)
        assert max(cnt) == 1, cnt
    host_case(gpu, ms, ref, ramp_plane(*hw), pinned=True)


def test_host_several_bands_and_units(gpu, ms, ref):
    """band_rows = 100 on 333 rows: four bands, the upload of band k + 1 prefetched under band k, pin_band alternating; host_units = 3: three
    units with their own halo rows through the one pipe of this device"""
    n = ms.n_layers
    x = rand_plane(333, 260, 12) - 0.5
    assert whole_plan(gpu, ms, x, band_rows=100).n_bands == 4
    _, cnt = host_case(gpu, ms, ref, x, band_rows=100)
    assert cnt[n - 2] == 4 and cnt[n - 1] == 0, cnt
    _, cnt = host_case(gpu, ms, ref, x, band_rows=100, fusion=gpu.FUSION_GATHER_LAUNCH, host_chunk_kb=64)
    assert cnt[n - 1] > 4, cnt
    host_case(gpu, ms, ref, x, band_rows=100, pinned=True)
    # (the units' bands are cut on the whole plane's grid: the resident call it equals is the unbanded one)
    got = poisoned_runs(ms, lambda: host_convert(gpu, ms, x, host_units=3))
    assert np.array_equal(got, dev_convert(gpu, ms, x))
    assert_close(got, ref.convert(x, njob=8), "host_units=3")
    got = poisoned_runs(ms, lambda: host_convert(gpu, ms, x[:150, :131], nn2x=True, host_units=3))
    assert np.array_equal(got, dev_convert(gpu, ms, x[:150, :131], True))


# ---- d. batches ------------------------------------------------------------------------------------------------------------------------------------
def batch_planes(n, h, w, seed):
    return np.stack([(rand_plane(h, w, seed + i) - 0.5) if i % 2 == 0 else ramp_plane(h, w) * (1.0 + 0.25 * i) for i in range(n)])


def dev_batch(gpu, ms, x, nn2x=False, **okw):
    n, h, w = x.shape
    up = 1 if nn2x else 0
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((n, h << up, w << up), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    ms.convert_batch_device(n, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), (h << up) * (w << up) * 4, (w << up) * 4,
                            nn2x=nn2x, stream=st.cuda_stream, opts=gpu.make_opts(device=0, **okw))
    st.synchronize()
    return d_out.cpu().numpy()


def singles(gpu, ms, x, nn2x=False, **okw):
    return np.stack([dev_convert(gpu, ms, x[i], nn2x, **okw) for i in range(len(x))])


@pytest.mark.parametrize("nn2x", [False, True], ids=["plain", "nn2x"])
@pytest.mark.parametrize("hw", [(33, 47), (40, 257), (256, 256)], ids=lambda s: "%dx%d" % s)   # ragged blocks; second job group; the batch benchmark's size
def test_batch_default(gpu, ms, ref, hw, nn2x):
    """n = 5 with defaults: one sub-batch, the neighbouring image's block directly behind every image's in both workspaces"""
    x = batch_planes(5, hw[0], hw[1], 100)
    if nn2x:
        x = x[:, :(hw[0] + 1) // 2, :(hw[1] + 1) // 2]
    cnt = []

    def call():
        out, c = launches(ms, lambda: dev_batch(gpu, ms, x, nn2x, profile=1))
        cnt[:] = c
        return out
    got = poisoned_runs(ms, call)
    assert cnt == [0] + [1] * 6, cnt
    assert np.array_equal(got, singles(gpu, ms, x, nn2x))
    for i in (0, 4):
        assert_close(got[i], ref.convert(up2(x[i]) if nn2x else x[i], njob=8), "image %d" % i)
    host = poisoned_runs(ms, lambda: ms.convert_batch(x, nn2x=nn2x))
    assert np.array_equal(host, got)


def test_batch_sub_batches_3_3_1(gpu, ms, ref):
    """n = 7 under a workspace budget that holds three images: sub-batches of 3 + 3 + 1, the last one on one image's block of a three-image workspace"""
    x = batch_planes(7, 256, 256, 200)
    p = ms.plan_rows(256, 256, opts=gpu.make_opts(device=0))
    per = sum(((int(b) + 3) // 4 + 63) // 64 * 64 * 4 for b in p.workspace_bytes)   # batch_ws_floats: every image's block on a 256-byte boundary
    mb = (3 * per + (1 << 20) - 1) >> 20
    assert 3 * per <= mb << 20 < 4 * per
    cnt = []

    def call():
        out, c = launches(ms, lambda: dev_batch(gpu, ms, x, profile=1, workspace_mb=mb))
        cnt[:] = c
        return out
    got = poisoned_runs(ms, call)
    assert cnt == [0] + [3] * 6, cnt
    assert np.array_equal(got, singles(gpu, ms, x, workspace_mb=mb))
    assert_close(got[6], ref.convert(x[6], njob=8), "image 6")
    host = poisoned_runs(ms, lambda: ms.convert_batch(x, opts=gpu.make_opts(workspace_mb=mb)))
    assert np.array_equal(host, got)


def test_batch_fallbacks(gpu, ms, ref):
    """the single-plane launch sequence per image: an option set the batched chain does not take (fusion = PROG), and planes of several bands"""
    x = batch_planes(3, 40, 257, 300)
    got = poisoned_runs(ms, lambda: dev_batch(gpu, ms, x, fusion=gpu.FUSION_PROG))
    assert np.array_equal(got, singles(gpu, ms, x, fusion=gpu.FUSION_PROG))
    assert_close(got[2], ref.convert(x[2], njob=8), "fusion=PROG, image 2")
    y = batch_planes(2, 640, 512, 400)
    cnt = []

    def call():
        out, c = launches(ms, lambda: dev_batch(gpu, ms, y, profile=1, workspace_mb=96))
        cnt[:] = c
        return out
    got = poisoned_runs(ms, call)
    assert cnt[1] > 2, cnt     # several bands per image
    assert np.array_equal(got, singles(gpu, ms, y, workspace_mb=96))
    assert_close(got[1], ref.convert(y[1], njob=8), "several bands, image 1")


# ---- e. Model::filter ------------------------------------------------------------------------------------------------------------------------------
def filter_dev(gpu, ms, l, x, nhwc_in=False, nhwc_out=False, **okw):
    cin, h, w = x.shape
    cout = ms.planes(l)[1]
    d_in = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0) if nhwc_in else x)).cuda()
    d_out = torch.full((h, w, cout) if nhwc_out else (cout, h, w), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    ms.filter_device(l, cin, d_in.data_ptr(), (1, w * cin, cin) if nhwc_in else (h * w, w, 1), w, h, d_out.data_ptr(),
                     (1, w * cout, cout) if nhwc_out else (h * w, w, 1), stream=st.cuda_stream, opts=gpu.make_opts(device=0, **okw))
    st.synchronize()
    out = d_out.cpu().numpy()
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if nhwc_out else out


@pytest.mark.parametrize("w", [69, 70, 71, 72])   # the ragged planar store of conv3x3_wino4 through fc.pout: w = 1, 2, 3, 0 mod 4
def test_filter_wino4_layer(gpu, w):
    lay = small_layers([64, 64], 17)
    m = gpu._ModelSet.from_layers(lay)
    assert m.kernel_name(0) == "conv3x3_wino4"
    x = np.random.default_rng(w).standard_normal((64, 37, w)).astype(np.float32)
    want = orc.Oracle(lay).filter(0, x)
    got = poisoned_runs(m, lambda: m.filter(0, x))                 # host planes: fc.pin, fc.planar, fc.pad, fc.pout
    assert_close(got, want, "filter 64->64 w=%d" % w)
    dev = poisoned_runs(m, lambda: filter_dev(gpu, m, 0, x))       # device planes
    assert np.array_equal(dev, got)


@pytest.mark.parametrize("cin,cout,opt", [(1, 32, "AUTO"), (128, 1, "AUTO"), (3, 32, "AUTO"), (32, 32, "AUTO"), (64, 128, "MFMA"), (64, 128, "WINOGRAD32"),
                                          (128, 128, "AUTO"), (32, 64, "DIRECT")])
def test_filter_layers(gpu, cin, cout, opt):
    """a first and a last layer, the F(2x2) layer, and the named mid-layer kernels, at a ragged size (37 x 61: w = 1 mod 4)"""
    lay = small_layers([cin, cout], 200 + cin * 7 + cout)
    m = gpu._ModelSet.from_layers(lay)
    kw = dict(kernel=getattr(gpu, "KERNEL_" + opt))
    x = np.random.default_rng(cin + cout).standard_normal((cin, 37, 61)).astype(np.float32)
    want = orc.Oracle(lay).filter(0, x)
    got = poisoned_runs(m, lambda: m.filter(0, x, opts=gpu.make_opts(**kw)))
    assert_close(got, want, "%s %d->%d" % (m.kernel_name(0, gpu.make_opts(**kw)), cin, cout))
    assert np.array_equal(poisoned_runs(m, lambda: filter_dev(gpu, m, 0, x, **kw)), got)


def test_filter_chains(gpu):
    """Model::filter chained by hand: planar host planes (uploaded every call, and with filter_resident -- whose promise the fill withdraws), and
    the NHWC device chain"""
    lay = small_layers([3, 32, 64, 64, 3], 91)
    m, o = gpu._ModelSet.from_layers(lay), orc.Oracle(lay)
    x = np.random.default_rng(3).standard_normal((3, 45, 70)).astype(np.float32)
    want = x
    for l in range(4):
        want = o.filter(l, want, njob=4)

    def host_chain(**kw):
        t = x
        for l in range(4):
            t = m.filter(l, list(t) if kw else t, opts=gpu.make_opts(**kw))
        return t

    def nhwc_chain():
        t = x
        for l in range(4):
            t = filter_dev(gpu, m, l, t, nhwc_in=l > 0, nhwc_out=l < 3)
        return t
    got = poisoned_runs(m, host_chain)
    assert_close(got, want, "host filter chain")
    assert np.array_equal(poisoned_runs(m, lambda: host_chain(filter_resident=1)), got)
    assert np.array_equal(poisoned_runs(m, nhwc_chain), got)
    # the fill between two calls of a resident chain: the second call uploads what it is given
    a = m.filter(0, x, opts=gpu.make_opts(filter_resident=1))
    assert m.fill_scratch(WORDS[2], 0) > 0
    b = m.filter(1, list(a), opts=gpu.make_opts(filter_resident=1))
    assert np.array_equal(b, m.filter(1, a.copy()))


# ---- f. the multi-plane wrapper and the image entry points ----------------------------------------------------------------------------------------
def test_multi_plane_wrapper(gpu):
    """[3, 32, 64, 3]: a last layer that does not store into the caller's planes (workspace + repack)"""
    planes = [3, 32, 64, 3]
    lay = small_layers(planes, 900 + sum(planes))
    n = len(lay)
    m, o = gpu._ModelSet.from_layers(lay), orc.Oracle(lay)
    h, w = 31, 45
    x = np.random.default_rng(8).random((3, h, w), dtype=np.float32) - 0.5
    t = np.pad(x, ((0, 0), (n, n), (n, n)), mode="edge")
    for l in range(n):
        t = o.filter(l, t, njob=4)
    want = t[:, n:n + h, n:n + w]
    st = torch.cuda.current_stream()

    def call():
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
        m.convert_planes_device(3, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_out.data_ptr(), h * w * 4, w * 4, stream=st.cuda_stream, opts=gpu.make_opts(device=0))
        st.synchronize()
        return d_out.cpu().numpy()
    assert_close(poisoned_runs(m, call), want, "planes %s" % planes)


def test_image_entry_points(gpu, noise1_layers, scale_layers):
    """scale2x_image_u8 / process_image_u8 on one odd-sized image (aux, img_io): the oracle's bytes with the reference-ordered kernel, at most
    one LSB off with the fast ones (tests/test_gpu_parity.py: test_scale2x_image_u8_pipeline, test_process_image_modes)"""
    mn, msc = gpu._ModelSet.from_layers(noise1_layers), gpu._ModelSet.from_layers(scale_layers)
    img = np.random.default_rng(5).integers(0, 256, (23, 37, 3), dtype=np.uint8)
    direct = gpu.make_opts(kernel=gpu.KERNEL_DIRECT)
    want = orc.scale2x_image_u8(orc.Oracle(scale_layers), img, 1)
    assert np.array_equal(poisoned_runs(msc, lambda: msc.scale2x_image_u8(img, 1, direct)), want)
    fast = poisoned_runs(msc, lambda: msc.scale2x_image_u8(img, 1))
    diff = np.abs(fast.astype(np.int16) - want.astype(np.int16))
    assert diff.max() <= 1 and (diff != 0).mean() < 0.01, (diff.max(), (diff != 0).mean())
    want = orc.process_image_u8(img, orc.Oracle(noise1_layers), orc.Oracle(scale_layers), 1)
    assert np.array_equal(poisoned_runs(mn, lambda: gpu.process_image_u8(img, mn, msc, 1, direct), also=[msc]), want)
    fast = poisoned_runs(mn, lambda: gpu.process_image_u8(img, mn, msc, 1), also=[msc])
    assert np.abs(fast.astype(np.int16) - want.astype(np.int16)).max() <= 1
