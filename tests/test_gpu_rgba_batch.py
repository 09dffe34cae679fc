"""GPU tests of the batch forms of the RGBA call (w2xc_process_image_rgba_u8_batch[_device]) and of the one-launch tiled colour bleed.  Exact comparisons
only: the bleed against bleed_ref (tests/test_rgba_api.py), applied one pass at a time so that every pass count of an image shares one chain of passes;
a batch against the single RGBA calls on its images; the launch counts against the 3-channel batch."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from tools import gen_model
from test_rgba_api import bleed_ref
from test_gpu_rgba import WORDS, CASES, OPTS, gpu, models, layers, opts_of, final_size, dev_bleed   # noqa: F401 (gpu, models: fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

L = 16                                          # W2XC_BLEED_TILED_MAX (w2xc_kernels.h), BLEED_L of k_bleed_tiled: 2..L passes are the tiled kernel's at every image size
PASSES = (1, 2, 14, L, L + 1, 40)               # RgbaBleedFirst alone (1), the tiled kernel (2, 14, L), the pass chain (L + 1, 40)
P_USED = 3


# ---- the inputs ----
def blocks_image(seed, h, w):
    """random bytes, alpha zeroed; five opaque blocks, four single opaque pixels"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    img[:, :, 3] = 0
    for _ in range(5):
        y, x = rng.integers(0, h - 12), rng.integers(0, w - 12)
        bh, bw = rng.integers(3, 12), rng.integers(3, 12)
        img[y:y + bh, x:x + bw, 3] = rng.integers(1, 256)
    for _ in range(4):
        img[rng.integers(0, h), rng.integers(0, w), 3] = 255
    return img


@functools.lru_cache(maxsize=None)
def big(name):
    """multi-tile images for any tile size up to 64"""
    if name == "M1":
        img = blocks_image(31, 150, 137)
    elif name == "M2":
        img = blocks_image(32, 67, 201)
    elif name == "M3":                           # opaque, with transparent rectangles -- one of them on two edges -- and an opaque pixel alone in one
        img = np.random.default_rng(33).integers(0, 256, (150, 137, 4)).astype(np.uint8)
        img[:, :, 3] = 255
        img[20:76, 50:111, 3] = 0
        img[100:150, 0:41, 3] = 0
        img[47, 80, 3] = 255
    else:                                        # one row, one column: a few opaque pixels
        h, w = (1, 201) if name == "1x201" else (150, 1)
        img = np.random.default_rng(34).integers(0, 256, (h, w, 4)).astype(np.uint8)
        img[:, :, 3] = 0
        img.reshape(-1, 4)[[3, 90, 91], 3] = (255, 1, 77)
    img.setflags(write=False)
    return img


def dilate(mask):
    h, w = mask.shape
    p = np.pad(mask, 1)
    return np.any([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)


@functools.lru_cache(maxsize=None)
def chain(name, upto):
    """[(colour, mask) after p passes for p = 0..upto]: bleed_ref one pass at a time -- a pass reads only the image and the mask the pass before left,
    and the mask after a pass is the mask before it, dilated (a pixel is filled iff one of its 3x3 neighbours counted)"""
    img = big(name)
    cur, mask = img.copy(), img[:, :, 3] > 0
    steps = [(cur[:, :, :3].copy(), mask)]
    for _ in range(upto):
        cur[:, :, 3] = np.where(mask, 255, 0)
        cur = bleed_ref(cur, 1)
        mask = dilate(mask)
        steps.append((cur[:, :, :3].copy(), mask))
    return steps


def bled(name, passes):
    return chain(name, 40)[passes][0]


def test_chain_of_single_passes_is_bleed_ref():
    assert np.array_equal(bled("M2", 3), bleed_ref(big("M2"), 3)[:, :, :3])
    assert np.array_equal(bled("M3", 2), bleed_ref(big("M3"), 2)[:, :, :3])
    assert np.array_equal(bled("M1", 14), bleed_ref(big("M1"), 14)[:, :, :3])      # the deepest automatic count, in one piece


# ---- 1. the tiled bleed across tile borders, and the pass chain behind it ----
@pytest.mark.parametrize("name", ["M1", "M2", "M3", "1x201", "150x1"])
def test_tiled_bleed_equals_reference(gpu, name):
    """M1 / M2 as built here: the reached share is 0.362 / 0.417 after 14 passes and 0.889 / 0.906 after 40"""
    img = big(name)
    for passes in PASSES:
        assert np.array_equal(dev_bleed(gpu, img, passes), bled(name, passes)), (name, passes)
    if name in ("M1", "M2"):
        steps = chain(name, 40)
        assert all((steps[p + 1][0] != steps[p][0]).any() for p in range(40)), "every one of the first 40 passes changes pixels"
        share = [float(steps[p][1].mean()) for p in (14, 40)]
        print(name, "reached share after 14 / 40 passes: %.3f / %.3f" % tuple(share))
        want = (0.36, 0.89) if name == "M1" else (0.43, 0.90)
        assert abs(share[0] - want[0]) < 0.02 and abs(share[1] - want[1]) < 0.02, share
        assert not any(steps[p][1].all() for p in PASSES), "some pixels stay out of reach at every tested pass count"


def test_tiled_bleed_aligned_rows(gpu):
    """contiguous rows at a 4-byte-aligned address: the kernel loads a pixel as one 32-bit word (dev_bleed's 4 w + 5 row stride takes the byte loads)"""
    img = big("M1")
    h, w, _ = img.shape
    d_in = torch.from_numpy(img.copy()).cuda()
    assert d_in.data_ptr() % 4 == 0
    st = torch.cuda.current_stream()
    for passes in (2, 14, L):
        d_out = torch.full((h + 1, w * 3), 0xAB, dtype=torch.uint8, device="cuda")
        gpu.bleed_rgba_u8_device(d_in.data_ptr(), w * 4, w, h, passes, d_out.data_ptr(), w * 3, stream=st.cuda_stream)
        st.synchronize()
        b = d_out.cpu().numpy()
        assert (b[h] == 0xAB).all(), "bytes behind the output were written"
        assert np.array_equal(b[:h].reshape(h, w, 3), bled("M1", passes)), passes


# ---- the batch's images: one size, colour and alpha pattern of their own ----
SIZES = {"a": (24, 36), "b": (37, 53)}


@functools.lru_cache(maxsize=None)
def bimages(name, n=3):
    h, w = SIZES[name]
    out = []
    for i in range(n):
        img = np.random.default_rng(700 + 10 * i + (name == "b")).integers(0, 256, (h, w, 4)).astype(np.uint8)
        a = img[:, :, 3]
        a[2 + 3 * i:11 + 3 * i, 3 + 2 * i:12 + 2 * i] = 0        # 9 x 9 inside, elsewhere in every image
        a[h - 5 - i:, w - 7 - 2 * i:] = 0                        # a corner: two edges
        a[(5 * i) % h, :] = 0                                    # a row of its own
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


def ms_of(models, name):
    return models[name] if name else None


def singles(gpu, models, imgs, noise, scale, it, shrink, o, passes=P_USED):
    return np.stack([gpu.process_image_rgba_u8(im, ms_of(models, noise), ms_of(models, scale), it, o, shrink, passes) for im in imgs])


def device_batch(gpu, models, imgs, noise, scale, it, shrink, o, passes=P_USED, pad=False):
    """the device form; pad: ROIs inside larger buffers -- a lead, row strides that are no multiple of 4, image strides with bytes between the images --
    and every byte outside the output ROIs must keep its fill, the inputs must stay as they were"""
    n, (h, w, _) = len(imgs), imgs[0].shape
    H, W = final_size(h, w, it, shrink)
    lead_i, irs, gap_i = (11, w * 4 + 5, 37) if pad else (0, w * 4, 0)
    lead_o, ors, gap_o = (13, W * 4 + 7, 29) if pad else (0, W * 4, 0)
    iis, ois = irs * h + gap_i, ors * H + gap_o
    host = np.full(lead_i + n * iis, 0x5A, np.uint8)
    inside = np.zeros(lead_o + n * ois, bool)
    for i, im in enumerate(imgs):
        rows = host[lead_i + i * iis:lead_i + i * iis + irs * h].reshape(h, irs)
        rows[:, :w * 4] = im.reshape(h, w * 4)
        inside[lead_o + i * ois:lead_o + i * ois + ors * H].reshape(H, ors)[:, :W * 4] = True
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.full((lead_o + n * ois,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    gpu.process_image_rgba_u8_batch_device(n, d_in.data_ptr() + lead_i, iis, irs, w, h, d_out.data_ptr() + lead_o, ois, ors, ms_of(models, noise),
                                           ms_of(models, scale), it, shrink, passes, stream=st.cuda_stream, opts=o if o is not None else gpu.make_opts(device=0))
    st.synchronize()
    b = d_out.cpu().numpy()
    assert (b[~inside] == 0xAB).all(), "bytes outside the output ROIs were written"
    assert np.array_equal(d_in.cpu().numpy(), host), "the inputs were written"
    return b[inside].reshape(n, H, W, 4)


# ---- 2. a batch equals the single calls ----
NOISE_SHRINK = {"y": ("noise_shrink0.6", "yn", None, "b", 0, 0.6), "rgb": ("noise_shrink0.6", "m7", None, "b", 0, 0.6)}
ALL_CASES = {r: CASES[r] + [NOISE_SHRINK[r]] for r in CASES}
EXTRA = [("noise_scale", "direct"), ("scale1", "fusion_off"), ("noise", "fusion_off"), ("scale2", "bands"), ("noise_shrink0.6", "bands")]
ROUTE_CASE_OPT = ([(r, c[0], "default") for r in ("y", "rgb") for c in ALL_CASES[r]] + [(r, c, o) for r in ("y", "rgb") for c, o in EXTRA] +
                  [("y", "noise_scale", "bf16x3"), ("y", "ratio1.5", "bf16x3")])


@pytest.mark.parametrize("route,case,opt", ROUTE_CASE_OPT, ids=["%s-%s-%s" % t for t in ROUTE_CASE_OPT])
def test_batch_equals_single_calls(gpu, models, route, case, opt):
    _, noise, scale, img, it, shrink = [c for c in ALL_CASES[route] if c[0] == case][0]
    imgs = bimages(img)
    o = opts_of(gpu, opt)
    want = singles(gpu, models, imgs, noise, scale, it, shrink, o)
    assert len({want[i].tobytes() for i in range(3)}) == 3 and len({want[i][:, :, 3].tobytes() for i in range(3)}) == 3, "an image-index error would show"
    got = gpu.process_image_rgba_u8_batch(list(imgs), ms_of(models, noise), ms_of(models, scale), it, o, shrink, P_USED)
    assert got.shape == want.shape and np.array_equal(got, want), "host form"
    assert np.array_equal(device_batch(gpu, models, imgs, noise, scale, it, shrink, opts_of(gpu, opt, device=0)), want), "device form"
    assert np.array_equal(gpu.process_image_rgba_u8_batch(list(imgs[:1]), ms_of(models, noise), ms_of(models, scale), it, o, shrink, P_USED), want[:1]), "n = 1"


# ---- 3. ragged sub-batches ----
def launches(ms, fn):
    ms.profile_reset(0)
    fn()
    torch.cuda.synchronize()
    return ms.profile_read(0)[1]


def test_ragged_sub_batches(gpu, models):
    """n = 5 under a workspace_mb that holds the batched layer chain's workspace of 4 planes (and not of 6) at the call's largest level: the header's rule
    gives the chain k = 4 or 5 planes and so the RGBA call S = k // 2 = 2 images -- a Y brings its alpha -- in sub-batches of 2, 2 and 1"""
    imgs = bimages("b", 5)
    h, w = SIZES["b"]
    plan = models["ys"].plan_rows(2 * w, 2 * h)
    per = sum(4 * (((int(b) + 3) // 4 + 63) & ~63) for b in plan.workspace_bytes)
    mb = -(-4 * per >> 20)
    assert per > 0 and ((mb << 20) // per) in (4, 5), (per, mb)
    o = gpu.make_opts(device=0, profile=1, workspace_mb=mb)
    got = []
    cnt = launches(models["ys"], lambda: got.append(device_batch(gpu, models, imgs, None, "ys", 1, 0.0, o)))
    print("workspace_mb", mb, "launches per layer", cnt)
    assert cnt == [0] + [3] * 6, cnt
    assert np.array_equal(got[0], singles(gpu, models, imgs, None, "ys", 1, 0.0, gpu.make_opts(workspace_mb=mb)))
    assert np.array_equal(gpu.process_image_rgba_u8_batch(list(imgs), None, models["ys"], 1, gpu.make_opts(workspace_mb=mb), 0.0, P_USED), got[0])
    one = launches(models["ys"], lambda: got.append(device_batch(gpu, models, imgs, None, "ys", 1, 0.0, gpu.make_opts(device=0, profile=1))))
    assert one == [0] + [1] * 6, one
    assert np.array_equal(got[1], got[0]), "the default workspace: one sub-batch, the same bytes"


# ---- 4. launch counts: alpha rides with Y ----
def test_launch_counts_equal_three_channel_batch(gpu, models):
    """one sub-batch of n = 3 (the device forms: the host forms cut a batch in two to overlap their copies), noise + 2 iterations"""
    n, h, w, it = 3, 64, 64, 2
    x = np.random.default_rng(64).integers(0, 256, (n, h, w, 4)).astype(np.uint8)
    o = gpu.make_opts(device=0, profile=1)
    st = torch.cuda.current_stream()
    counts = {}
    for name, px in (("rgba", 4), ("three", 3)):
        d_in = torch.from_numpy(np.ascontiguousarray(x[:, :, :, :px])).cuda()
        d_out = torch.empty((n, h << it, w << it, px), dtype=torch.uint8, device="cuda")
        args = (n, d_in.data_ptr(), h * w * px, w * px, w, h, d_out.data_ptr(), (h << it) * (w << it) * px, (w << it) * px, models["yn"], models["ys"], it, 0.0)
        for m in ("yn", "ys"):
            models[m].profile_reset(0)
        if px == 4:
            gpu.process_image_rgba_u8_batch_device(*args, -1, stream=st.cuda_stream, opts=o)
        else:
            gpu.process_image_u8_batch_device(*args, stream=st.cuda_stream, opts=o)
        torch.cuda.synchronize()
        counts[name] = [models[m].profile_read(0)[1] for m in ("yn", "ys")]
    print(counts)
    assert counts["three"] == [[0] + [1] * 6, [0] + [2] * 6]
    assert counts["rgba"] == counts["three"]


# ---- 5. the device form's layout ----
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_device_form_layout(gpu, models, route):
    for case in ("noise_scale", "noise", "ratio1.5", "noise_shrink0.6"):
        _, noise, scale, img, it, shrink = [c for c in ALL_CASES[route] if c[0] == case][0]
        imgs = bimages(img)
        want = singles(gpu, models, imgs, noise, scale, it, shrink, None, -1)
        assert np.array_equal(device_batch(gpu, models, imgs, noise, scale, it, shrink, None, -1, pad=True), want), case


# ---- 6. nothing is read that the call did not write ----
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_scratch_independence_and_trim(gpu, models, route):
    for case in ("noise_scale", "noise_shrink0.6"):
        _, noise, scale, img, it, shrink = [c for c in ALL_CASES[route] if c[0] == case][0]
        imgs = list(bimages(img))

        def call():
            return gpu.process_image_rgba_u8_batch(imgs, ms_of(models, noise), ms_of(models, scale), it, None, shrink, L + 1)   # (the pass chain: stamps)
        first = call()
        for word in WORDS:
            for ms in models.values():
                ms.fill_scratch(word)
            assert np.array_equal(call(), first), (case, hex(word))
        for ms in models.values():
            ms.trim()
        assert all(ms.fill_scratch(0) == 0 for ms in models.values()), "trim released every buffer, the RGBA batch's included"
        assert np.array_equal(call(), first), "after trim the next call allocates again"


# ---- 7. multi-tile images through the whole call ----
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_multi_tile_images_through_the_call(gpu, models, route):
    scale = "ys" if route == "y" else "m4"
    auto = len(layers(scale))                    # bleed_passes = -1: the layer count of the scale model
    assert auto <= L
    imgs = [big("M1"), big("M3")]
    got = gpu.process_image_rgba_u8_batch(imgs, None, models[scale], 1, None, 0.0, -1)
    three = gpu.process_image_rgb_u8_batch if route == "rgb" else gpu.process_image_u8_batch
    want = three([np.ascontiguousarray(bled(n, auto)) for n in ("M1", "M3")], None, models[scale], 1, None)
    assert np.array_equal(got[:, :, :, :3], want), "colour = the 3-channel batch on bleed_ref's images"
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i, :, :, 3], gpu.process_image_rgba_u8(im, None, models[scale], 1, None, 0.0, -1)[:, :, 3]), "alpha = the single call's"


# ---- 8. the CLI ----
@pytest.mark.parametrize("route", ["y", "rgb"])
def test_cli_batches_alpha_inputs(gpu, models, route, tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    spec = importlib.util.spec_from_file_location("w2xc_cli", os.path.join(ROOT, "tools", "w2xc_cli.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    scale = "ys" if route == "y" else "m4"
    gen_model.write_json(layers(scale), str(tmp_path / "scale2.0x_model.json"))
    flip = (lambda a: a) if route == "rgb" else (lambda a: np.ascontiguousarray(a[:, :, [2, 1, 0, 3]]))
    srcs = {}
    for name, (h, w), seed in (("p", (20, 16), 1), ("q", (20, 16), 2), ("r", (12, 18), 3)):
        src = np.random.default_rng(seed).integers(1, 256, (h, w, 4)).astype(np.uint8)
        src[:7 - seed, 10 - seed:, 3] = 0                                      # a transparent corner, of its own size in every image
        Image.fromarray(src).save(str(tmp_path / (name + ".png")))
        srcs[name] = src
    assert cli.main(["-i"] + [str(tmp_path / (n + ".png")) for n in srcs] + ["-m", "scale", "--model_dir", str(tmp_path)]) == 0
    for name, src in srcs.items():
        out = Image.open(cli.auto_output_name(str(tmp_path / (name + ".png")), "scale", 1, 2.0))
        assert out.mode == "RGBA"
        want = flip(gpu.process_image_rgba_u8(flip(src), None, models[scale], 1, gpu.make_opts(precision=gpu.PRECISION_FP32)))
        assert np.array_equal(np.asarray(out), want), name
