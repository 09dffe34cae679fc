"""GPU tests of the image batch entry points (w2xc_process_image_u8_batch / _batch_device): every image of a batch is BYTE-identical to the
single-image call with the same models, iterations, shrink ratio and options -- all modes, odd sizes, both forms, every option set; the colour /
resize stages and the layers really run once per sub-batch; memory follows the sub-batch size and not n; offsets past 4 GiB; poisoned scratch;
two threads with the models in opposite roles.  Every batch holds DISTINCT random images, so an image-index mix-up cannot hide."""
import threading

import numpy as np
import pytest

from tools import gen_model
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORDS = (0x00000000, 0x7FC00000, 0x7149F2CA)   # zeros, quiet NaN, 1e30f
GIB = 1 << 30


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


@pytest.fixture(scope="module")
def mn(gpu, noise1_layers):
    return gpu._ModelSet.from_layers(noise1_layers)


@pytest.fixture(scope="module")
def msc(gpu, scale_layers):
    return gpu._ModelSet.from_layers(scale_layers)


def images(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def models(mode, mn, msc, it):
    return (mn if "noise" in mode else None), (msc if "scale" in mode and it else None)


def single(gpu, x, noise, scale, it, shrink=0.0, opts=None):
    """the single-image host call, image by image"""
    return np.stack([gpu.process_image_u8(x[i], noise, scale, it, opts, shrink) for i in range(len(x))])


def final_size(h, w, it, shrink):
    H, W = h << it, w << it
    if shrink:
        W, H = int(float(W * shrink)), int(float(H * shrink))
    return H, W


def device_batch(gpu, x, noise, scale, it, shrink=0.0, opts=None, pad_cols=0, pad_rows=0):
    """the device form on resident images; pad_cols = guard bytes behind every row, pad_rows = guard rows between the images (above the first too).
    The guard must come back untouched."""
    n, h, w, _ = x.shape
    H, W = final_size(h, w, it, shrink)
    irs, ors = w * 3 + pad_cols, W * 3 + pad_cols
    src = torch.full((n, h + pad_rows, irs), 0x5A, dtype=torch.uint8)
    src[:, pad_rows:, :w * 3] = torch.from_numpy(x.reshape(n, h, w * 3))
    d_in = src.cuda()
    d_out = torch.full((n, H + pad_rows, ors), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    o = opts if opts is not None else gpu.make_opts(device=0)
    gpu.process_image_u8_batch_device(n, d_in.data_ptr() + pad_rows * irs, (h + pad_rows) * irs, irs, w, h, d_out.data_ptr() + pad_rows * ors,
                                      (H + pad_rows) * ors, ors, noise, scale, it, shrink, stream=st.cuda_stream, opts=o)
    st.synchronize()
    b = d_out.cpu().numpy()
    guard = np.ones(b.shape, bool)
    guard[:, pad_rows:, :W * 3] = False
    assert (b[guard] == 0xA5).all(), "bytes outside the output images were written"
    return b[:, pad_rows:, :W * 3].reshape(n, H, W, 3).copy()


def check_both_forms(gpu, x, noise, scale, it, shrink=0.0, opts=None, what=""):
    want = single(gpu, x, noise, scale, it, shrink, opts)
    got = gpu.process_image_u8_batch(x, noise, scale, it, opts, shrink)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = [i for i in range(len(x)) if not np.array_equal(got[i], want[i])]
    assert not bad, "%s host form: images %s differ from the single call" % (what, bad)
    o = None
    if opts is not None:
        o = type(opts).from_buffer_copy(opts)
        o.device = 0
    gotd = device_batch(gpu, x, noise, scale, it, shrink, o, pad_cols=7, pad_rows=2)
    bad = [i for i in range(len(x)) if not np.array_equal(gotd[i], want[i])]
    assert not bad, "%s device form: images %s differ from the single call" % (what, bad)
    return want


@pytest.mark.parametrize("mode,it,shrink", [("noise", 0, 0.0), ("noise", 0, 0.75), ("scale", 1, 0.0), ("scale", 2, 0.0), ("scale", 1, 0.75),
                                            ("scale", 2, 0.75), ("noise_scale", 1, 0.0), ("noise_scale", 2, 0.0), ("noise_scale", 1, 0.75),
                                            ("noise_scale", 2, 0.75)])
def test_modes_iterations_shrink(gpu, mn, msc, mode, it, shrink):
    x = images(7, 23, 37, 11 + it)
    noise, scale = models(mode, mn, msc, it)
    want = check_both_forms(gpu, x, noise, scale, it, shrink, what="%s it=%d shrink=%g" % (mode, it, shrink))
    assert want.shape[1:3] == final_size(23, 37, it, shrink)
    assert len({want[i].tobytes() for i in range(7)}) == 7     # distinct images give distinct results: an index mix-up cannot pass


@pytest.mark.parametrize("hw", [(23, 37), (1, 1), (300, 5), (256, 256)])
@pytest.mark.parametrize("n", [1, 2, 7, 33])
def test_sizes_and_counts(gpu, mn, msc, hw, n):
    x = images(n, hw[0], hw[1], 100 * n + hw[0])
    check_both_forms(gpu, x, mn, msc, 1, what="%dx%d n=%d" % (hw[1], hw[0], n))


def test_sizes_with_shrink_and_noise_only(gpu, mn, msc):
    check_both_forms(gpu, images(5, 300, 5, 1), None, msc, 1, 0.75, what="5x300 scale shrink")
    check_both_forms(gpu, images(3, 1, 1, 2), mn, None, 0, what="1x1 noise")
    check_both_forms(gpu, images(3, 41, 64, 3), mn, msc, 2, 0.75, what="64x41 noise_scale x3")


def test_host_form_pageable_pinned_mixed_and_roi(gpu, mn, msc):
    n, h, w = 9, 40, 52
    x = images(n, h, w, 77)
    want = single(gpu, x, mn, msc, 1)
    # a list of pageable images
    assert np.array_equal(gpu.process_image_u8_batch([x[i].copy() for i in range(n)], mn, msc, 1), want)
    # page-locked in and out: DMA'd in place
    pin_in = torch.from_numpy(x.copy()).pin_memory()
    pin_out = torch.zeros((n, 2 * h, 2 * w, 3), dtype=torch.uint8).pin_memory()
    res = gpu.process_image_u8_batch(pin_in.numpy(), mn, msc, 1, out=pin_out.numpy())
    assert np.array_equal(pin_out.numpy(), want) and np.shares_memory(res, pin_out.numpy())
    # a mix of both in one call
    mixed = [pin_in.numpy()[i] if i % 2 else x[i].copy() for i in range(n)]
    assert np.array_equal(gpu.process_image_u8_batch(mixed, mn, msc, 1), want)
    # row strides wider than 3 w: ROI views into larger images, input and output
    big = np.full((n, h + 5, w + 9, 3), 0x33, np.uint8)
    big[:, 2:2 + h, 4:4 + w] = x
    roi = big[:, 2:2 + h, 4:4 + w]
    assert roi.strides[1] == (w + 9) * 3
    obig = np.full((n, 2 * h + 3, 2 * w + 6, 3), 0xA5, np.uint8)
    oroi = obig[:, 1:1 + 2 * h, 5:5 + 2 * w]
    gpu.process_image_u8_batch(roi, mn, msc, 1, out=oroi)
    assert np.array_equal(oroi, want)
    guard = np.ones(obig.shape, bool)
    guard[:, 1:1 + 2 * h, 5:5 + 2 * w] = False
    assert (obig[guard] == 0xA5).all()
    # device_mask = device 0 only
    assert np.array_equal(gpu.process_image_u8_batch(x, mn, msc, 1, gpu.make_opts(device_mask=1)), want)


@pytest.mark.parametrize("kw", [dict(precision=1), dict(precision=2), dict(precision=3), dict(precision=4), dict(kernel=1), dict(kernel=2),
                                dict(kernel=4), dict(fusion=1), dict(band_rows=16)])
def test_option_sets_byte_identical(gpu, mn, msc, kw):
    """every precision, W2XC_KERNEL_DIRECT / _MFMA / _WINOGRAD32, W2XC_FUSION_OFF, and a band_rows that cuts every image into several bands (the
    per-image launch sequence inside run_batch)"""
    x = images(3, 48, 64, 600)
    o = gpu.make_opts(**kw)
    if "band_rows" in kw:
        assert msc.plan_rows(128, 96, opts=o).n_bands > 1
    check_both_forms(gpu, x, mn, msc, 1, opts=o, what=str(kw))
    check_both_forms(gpu, x, mn, msc, 1, 0.75, opts=o, what=str(kw) + " shrink")


def launches(ms, fn):
    ms.profile_reset(0)
    fn()
    torch.cuda.synchronize()
    return ms.profile_read(0)[1]


def test_one_launch_per_layer_per_sub_batch(gpu, mn, msc):
    """N images inside one sub-batch on the default fp32 chain: each model's per-layer launch count is that of ONE image"""
    x = images(8, 64, 64, 300)
    o = gpu.make_opts(device=0, profile=1)
    per_model = []
    for n in (1, 8):
        mn.profile_reset(0)
        msc.profile_reset(0)
        device_batch(gpu, x[:n], mn, msc, 2, 0.0, o)
        torch.cuda.synchronize()
        per_model.append((mn.profile_read(0)[1], msc.profile_read(0)[1]))
    assert per_model[0] == per_model[1], per_model
    assert per_model[0][0] == [0] + [1] * 6 and per_model[0][1] == [0] + [2] * 6, per_model   # one noise pass, two scale iterations
    # ... and the single-image call 8 times launches 8 times as often
    mn.profile_reset(0)
    for i in range(8):
        device_batch(gpu, x[i:i + 1], mn, None, 0, 0.0, o)
    assert mn.profile_read(0)[1] == [0] + [8] * 6


def test_small_workspace_sub_batches(gpu, msc):
    """workspace_mb cuts 33 images into several sub-batches (here through the layer chain's own rule, which caps the image sub-batch): the layers
    run once per sub-batch, at least 3 and fewer than 33 times, and the bytes are those of the single calls with the same options"""
    x = images(33, 32, 32, 400)
    o = gpu.make_opts(device=0, profile=1, workspace_mb=48)
    got = []
    cnt = launches(msc, lambda: got.append(device_batch(gpu, x, None, msc, 1, 0.0, o)))
    assert 3 <= cnt[1] < 33 and len(set(cnt[1:])) == 1, cnt
    assert np.array_equal(got[0], single(gpu, x, None, msc, 1, opts=gpu.make_opts(workspace_mb=48)))
    assert np.array_equal(gpu.process_image_u8_batch(x, None, msc, 1, gpu.make_opts(workspace_mb=48)), got[0])


def test_memory_follows_sub_batch_not_n(gpu):
    """A small model (its workspaces are small beside the image planes) under workspace_mb = 8: the header's rule gives S = 8 MiB / (float planes of
    every level + uint8 in and out, per image) = 6 images for 64 x 64 sources and two iterations, so 33 images are 6 sub-batches.  Afterwards all
    scratch memory of the context (w2xc_debug_fill_scratch) is less than the image planes of 33 images alone would be."""
    ms = gpu._ModelSet.from_layers(gen_model.synth_layers([1, 16, 16, 1], 31))
    n, h, w, it = 33, 64, 64, 2
    aux = 4 * (4 * h * w + 3 * 4 * h * w + 3 * 16 * h * w)                  # bytes of float planes per image: level 0 four planes, then three per level
    per = aux + h * w * 3 + 16 * h * w * 3
    S = (8 << 20) // per
    assert S >= 1 and -(-n // S) >= 3, S
    x = images(n, h, w, 500)
    o = gpu.make_opts(device=0, workspace_mb=8)
    got = device_batch(gpu, x, None, ms, it, 0.0, o)
    filled = ms.fill_scratch(0, 0)
    assert 0 < filled < n * aux, (filled, n * aux)
    assert np.array_equal(got, single(gpu, x, None, ms, it, opts=gpu.make_opts(workspace_mb=8)))
    assert np.array_equal(gpu.process_image_u8_batch(x, None, ms, it, gpu.make_opts(workspace_mb=8)), got)
    assert ms.fill_scratch(0, 0) < n * aux      # the host form's staging follows S too
    ms.trim()
    assert ms.fill_scratch(0, 0) == 0           # w2xc_model_trim releases all of it


def test_trim_releases_the_filter_ring(gpu):
    """Model::filter from host planes allocates a page-locked bounce ring that w2xc_debug_fill_scratch counts: w2xc_model_trim, which the header says
    releases Model::filter's buffers, releases it too, so nothing is left to fill.  The next call grows everything again and gives the same planes."""
    ms = gpu._ModelSet.from_layers(gen_model.synth_layers([1, 16, 16, 1], 31))
    planes = [np.random.default_rng(77).random((40, 56), dtype=np.float32)]
    want = ms.filter(0, planes)
    assert ms.fill_scratch(0, 0) >= 2 * (8 << 20)   # (the ring alone: two 8 MiB slots)
    ms.trim()
    assert ms.fill_scratch(0, 0) == 0
    assert np.array_equal(ms.filter(0, planes), want)
    ms.trim()
    assert ms.fill_scratch(0, 0) == 0


def test_batch_against_the_oracle(gpu, mn, msc, noise1_layers, scale_layers):
    """W2XC_KERNEL_DIRECT: the batch output equals the CPU restatement of main.cpp byte for byte, for every image of a batch of distinct images"""
    x = images(3, 20, 28, 9)
    o = gpu.make_opts(kernel=gpu.KERNEL_DIRECT)
    got = gpu.process_image_u8_batch(x, mn, msc, 1, o)
    on, osc = orc.Oracle(noise1_layers), orc.Oracle(scale_layers)
    for i in range(len(x)):
        assert np.array_equal(got[i], orc.process_image_u8(x[i], on, osc, 1)), "image %d" % i
    od = gpu.make_opts(kernel=gpu.KERNEL_DIRECT, device=0)
    gotd = device_batch(gpu, x, None, msc, 1, 0.75, od, pad_cols=3, pad_rows=1)
    for i in range(len(x)):
        assert np.array_equal(gotd[i], orc.process_image_u8(x[i], None, osc, 1, 0.75)), "image %d (shrink)" % i


def test_image_strides_beyond_4gib(gpu, mn, msc):
    """n = 3 images of 24 x 16 whose input and output image strides are 2.2 GiB: image 1 starts past 2^31 bytes, image 2 past 2^32.  A guard value
    everywhere outside the images; byte-identical to the single calls, and the guard around every output image is untouched."""
    n, h, w = 3, 16, 24
    H, W = 2 * h, 2 * w
    stride = 2362232013            # bytes: 2.2 GiB, odd on purpose (uint8 images need no alignment)
    lead = 4096
    need = 2 * ((n - 1) * stride + 2 * lead + H * W * 3)
    free = torch.cuda.mem_get_info()[0]
    if free < need + 4 * GIB:      # (not an MI355X: 288 GB)
        pytest.skip("needs %.1f GiB of device memory plus 4 GiB of headroom; %.1f GiB are free" % (need / GIB, free / GIB))
    x = images(n, h, w, 6000)
    d_in = d_out = None
    try:
        size = (n - 1) * stride + 2 * lead + H * W * 3
        d_in = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda")
        d_out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
        for i in range(n):
            d_in[lead + i * stride: lead + i * stride + h * w * 3] = torch.from_numpy(x[i].ravel()).cuda()
        st = torch.cuda.current_stream()
        gpu.process_image_u8_batch_device(n, d_in.data_ptr() + lead, stride, w * 3, w, h, d_out.data_ptr() + lead, stride, W * 3, mn, msc, 1, 0.0,
                                          stream=st.cuda_stream, opts=gpu.make_opts(device=0))
        st.synchronize()
        want = single(gpu, x, mn, msc, 1)
        for i in range(n):
            a = lead + i * stride
            win = d_out[a - lead: a + H * W * 3 + lead].cpu().numpy()
            assert np.array_equal(win[lead: lead + H * W * 3].reshape(H, W, 3), want[i]), "image %d" % i
            assert (win[:lead] == 0xA5).all() and (win[lead + H * W * 3:] == 0xA5).all(), "image %d: the guard around it was written" % i
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()


def test_plane_loop_past_65535(gpu):
    """n = 33000 images of 1 x 1 in ONE sub-batch: the cubic stage gets 2 n = 66000 planes and the shrink's linear stage 3 n = 99000, both more than the
    65535 rows of workgroups a grid has, so the V planes of the images from 32535 on are the second trip of the kernel's plane loop.  330 distinct images
    tiled 100 times; expected, byte for byte: the same calls on the 330 images (the regime every other test here covers), tiled.
    One sub-batch with the default workspace_mb, nothing set: S = 16384 MiB / (the planes of every level + the uint8 image in and out, per image) is far
    above n, and this model has no batched chain whose own rule could cap it; afterwards the context's scratch holds the planes of all n images."""
    ms = gpu._ModelSet.from_layers(gen_model.synth_layers([1, 16, 16, 1], 31))
    n, pf = 33000, 64                                   # pf = floats of a 1 x 1 or 2 x 2 plane, rounded up to 256 bytes
    x330 = images(330, 1, 1, 65535)
    x = np.tile(x330, (100, 1, 1, 1))
    assert len(x) == n and 2 * n > 65535 and n + 65535 > 2 * n      # (U and V: a second trip of the plane loop, no third)
    for shrink, planes in ((0.5, 4 + 3 + 3), (0.0, 4 + 3)):         # planes per image: level 0 (Y, U, V, the noise pass's Y), level 1, the shrunk level
        per = 4 * pf * planes + 3 + 3 * (1 if shrink else 4)
        assert (16384 << 20) // per >= n
        want = np.tile(device_batch(gpu, x330, None, ms, 1, shrink), (100, 1, 1, 1))
        ms.trim()
        got = device_batch(gpu, x, None, ms, 1, shrink)
        assert got.shape == want.shape == (n,) + final_size(1, 1, 1, shrink) + (3,)
        bad = np.nonzero((got != want).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, "shrink %g: %d images differ from the 330-image call, first %s" % (shrink, bad.size, bad[:8])
        # one sub-batch: the planes of all n images exist at once.  (The layer launch count cannot show it for this model: it has no batched chain, so its
        # layers are launched per image whatever S is -- and for the same reason its conv scratch is one image's, a few KiB, which is what makes the
        # scratch total a statement about the image planes: with S = n / 2 the total would be half of this bound.)
        assert ms.fill_scratch(0, 0) >= n * 4 * pf * planes
    # an index mix-up cannot pass: every channel of the result (channel 0 follows V, channel 2 follows U) takes many values over the 330 images, so planes
    # taken from other images change bytes (this small model's Y is near 0, so many results share a clipped 0: not all 330 are distinct)
    assert all(len(set(want[:330, ..., ch].ravel().tolist())) >= 16 for ch in range(3))


def test_element_loop_past_65536_workgroups(gpu):
    """w2xc_u8_to_yuv_device then w2xc_yuv_to_u8_device on 4100 x 4100 pixels: 16 810 000 elements, more than the 65536 x 256 a grid covers in one trip, so
    the last 32 784 are every workgroup's second trip of the element loop.  All three planes and all bytes against the oracle -- the whole image, not
    windows (the oracle takes well under a second) -- and exactly, as the small-image test of these two entry points compares (test_gpu_parity.py)."""
    h = w = 4100
    assert 65536 * 256 < h * w < 2 * 65536 * 256
    img = images(1, h, w, 4100)[0]
    lib = gpu.lib()
    d_img = torch.from_numpy(img).cuda()
    d_p = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    d_out = torch.full((h, w, 3), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.w2xc_u8_to_yuv_device(d_img.data_ptr(), w * 3, w, h, d_p[0].data_ptr(), d_p[1].data_ptr(), d_p[2].data_ptr(), None) == 0
    assert lib.w2xc_yuv_to_u8_device(d_p[0].data_ptr(), d_p[1].data_ptr(), d_p[2].data_ptr(), w, h, d_out.data_ptr(), w * 3, None) == 0
    torch.cuda.synchronize()
    want = orc.u8_to_yuv(img)
    got = d_p.cpu().numpy()
    for name, g, t in zip("YUV", got, want):
        diff = g != t
        assert not diff.any(), "%s: %d elements differ, first at %s" % (name, int(diff.sum()), tuple(int(i[0]) for i in np.nonzero(diff)))
    diff = d_out.cpu().numpy() != orc.yuv_to_u8(*want)
    assert not diff.any(), "bytes: %d differ, first at %s" % (int(diff.sum()), tuple(int(i[0]) for i in np.nonzero(diff)))


def poisoned_runs(call, sets):
    """call() after each of the three fills of every scratch buffer of the models in `sets` on device 0: byte-identical results"""
    for _ in range(2):         # warm: every buffer this call needs exists at its final size (buffers only grow)
        call()
    outs, filled = [], []
    for word in WORDS:
        filled.append(tuple(ms.fill_scratch(word, 0) for ms in sets))
        outs.append(np.array(call()))
    assert all(f > 0 for f in filled[0]) and len(set(filled)) == 1, filled    # something was filled; nothing was reallocated in between
    for word, o in zip(WORDS[1:], outs[1:]):
        diff = o != outs[0]
        assert not diff.any(), "fill %#x changes %d bytes, first at %s" % (word, int(diff.sum()), tuple(int(v[0]) for v in np.nonzero(diff)))
    return outs[0]


@pytest.mark.parametrize("form", ["host", "device"])
def test_poisoned_scratch(gpu, mn, msc, form):
    x = images(5, 37, 45, 800)
    if form == "host":
        got = poisoned_runs(lambda: gpu.process_image_u8_batch(x, mn, msc, 1, None, 0.75), (mn, msc))
    else:
        got = poisoned_runs(lambda: device_batch(gpu, x, mn, msc, 1, 0.75), (mn, msc))
    assert np.array_equal(got, single(gpu, x, mn, msc, 1, 0.75))


def test_two_threads_models_in_opposite_roles(gpu, noise1_layers, scale_layers):
    """(A as noise, B as scale) and (B as noise, A as scale) at the same time: both contexts are taken together, so neither thread can hold one and
    wait for the other"""
    a, b = gpu._ModelSet.from_layers(noise1_layers), gpu._ModelSet.from_layers(scale_layers)
    x, y = images(6, 40, 32, 900), images(5, 40, 32, 950)
    want = [single(gpu, x, a, b, 1), single(gpu, y, b, a, 1)]
    got = [[], []]
    err = []

    def run(i, imgs, noise, scale):
        try:
            for _ in range(4):
                got[i].append(gpu.process_image_u8_batch(imgs, noise, scale, 1))
        except Exception as e:      # noqa: BLE001  (reported below, on the main thread)
            err.append(e)
    th = [threading.Thread(target=run, args=(0, x, a, b)), threading.Thread(target=run, args=(1, y, b, a))]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not any(t.is_alive() for t in th), "deadlock: a thread did not finish"
    assert not err, err
    for i in range(2):
        assert len(got[i]) == 4 and all(np.array_equal(g, want[i]) for g in got[i])
