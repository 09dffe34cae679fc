"""The device calls that take a frame, image or plane stride as a 64-bit byte count, with n = 3 frames 2.2 GiB apart: frame 1 starts past 2^31 bytes, frame 2
past 2^32 -- the luma, chroma, RGB-end and TTA blocks of the YUV and image routes, the batch forms of the RGB, RGBA and head-model image calls, and the YUV frame
calls (both sides far apart, whole and in sub-batches of 2 + 1, so the sub-batch offset is taken at a far stride).

Every comparison is equality of bytes: frame i of the far call against the same call on frame i alone in a compact buffer, the form the block and frame
tests hold to NumPy.  The far buffers hold a guard byte; a frame's window (its rows and the gaps between them) is compared whole, and when the windows have
been wiped every byte of the far buffers must be the guard again -- counted on the device.

Strides follow tests/test_gpu_batch.py and tests/test_gpu_image_batch.py: 2362232013 bytes for bytes (odd on purpose), that plus one for 16-bit words, 590558004
floats for float planes; every case runs again with all strides 2362232016 and 8-byte aligned bases and rows, where the byte kernels choose their wide
instantiations.  Frames are 70 x 38 at 4:2:0, images 24 x 16: more than one tile each way, ragged edges."""
import collections

import numpy as np
import pytest

import stream_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GIB = 1 << 30
STRIDE = {1: 2362232013, 2: 2362232014, 4: 2362232016}     # by the alignment of the samples: bytes, words, floats (590558004 of them)
STRIDE_8 = 2362232016
assert STRIDE_8 == 4 * 590558004 and STRIDE[1] > 1 << 31 and 2 * STRIDE[1] > 1 << 32
LEAD, SUB, SLOTS = 4096, 1 << 20, 4                         # guard in front; a region's windows start SUB apart from the next region's; regions per buffer
SIZE = LEAD + (SLOTS + 1) * SUB + 2 * STRIDE_8
GUARD = {"in": 0x5A, "out": 0xA5}
RIM = 32                                                    # guard bytes around a compact window
N, W, H, IW, IH = 3, 70, 38, 24, 16
CW, CH = 35, 19
LIMITED, BT709, DEPTH = 1, 1, 10
YUV_420, TOPLEFT = 0, 0x30
VARIANTS = ["odd", "aligned"]

View = collections.namedtuple("View", "ptr stride row plane")


@pytest.fixture(scope="module")
def ctx(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return sc.Ctx(w2xc, torch)


@pytest.fixture(scope="module")
def pool():
    """the two far buffers, inputs and outputs, filled with their guards.  The one route to a skip: a device with less free memory than they need plus 4 GiB
    (not an MI355X: 288 GB)"""
    need = 2 * SIZE
    free = torch.cuda.mem_get_info()[0]
    if free < need + 4 * GIB:
        pytest.skip("needs %.1f GiB of device memory plus 4 GiB of headroom; %.1f GiB are free" % (need / GIB, free / GIB))
    bufs = {role: torch.full((SIZE,), g, dtype=torch.uint8, device="cuda") for role, g in GUARD.items()}
    yield bufs
    bufs.clear()
    torch.cuda.empty_cache()


def dirty(buf, guard):
    """how many bytes of a far buffer are not the guard: counted on the device, 1 GiB at a time"""
    total = torch.zeros((), dtype=torch.int64, device="cuda")
    for a in range(0, buf.numel(), GIB):
        total += (buf[a:a + GIB] != guard).sum()
    return int(total)


class Region:
    """n windows of one kind in a far buffer: `planes` planes of `rows` rows of row_bytes bytes; kind: what the input data is ("u8", "rgba", "u16", "f32");
    contiguous: rows that follow each other without a gap (float planes whose call has no row stride)"""

    def __init__(self, name, role, kind, rows, row_bytes, planes=1, contiguous=False):
        self.name, self.role, self.kind, self.rows, self.row_bytes, self.planes, self.contiguous = name, role, kind, rows, row_bytes, planes, contiguous
        self.align = {"u8": 1, "rgba": 1, "u16": 2, "f32": 4}[kind]

    def resolve(self, variant, slot, buf):
        assert slot < SLOTS
        rb, a = self.row_bytes, self.align
        if variant == "aligned":
            self.stride, off = STRIDE_8, 0
            self.row = rb if self.contiguous else (rb + 7) // 8 * 8 + 8
        else:       # an odd base and odd strides for bytes, words two bytes and floats four bytes off an 8-byte boundary
            self.stride, off = STRIDE[a], {1: 13, 2: 2, 4: 4}[a]
            self.row = rb if self.contiguous else rb + {1: 3 - (rb & 1), 2: 2, 4: 4}[a]
        self.plane = self.rows * self.row + (16 if self.planes > 1 else 0)
        self.span = self.planes * self.plane
        assert self.span + 64 < SUB
        self.buf, self.base, self.guard = buf, LEAD + slot * SUB + off, GUARD[self.role]
        assert self.base + (N - 1) * self.stride + self.span + RIM <= buf.numel(), "the last window ends inside the buffer"
        return self

    def far(self):
        return View(self.buf.data_ptr() + self.base, self.stride, self.row, self.plane)

    def window(self, i):
        a = self.base + i * self.stride
        return self.buf[a:a + self.span]

    def data(self, seed):
        """one window of random samples, guard in the gaps"""
        r = np.random.default_rng(seed)
        shape = (self.planes, self.rows, self.row_bytes)
        if self.kind == "f32":
            x = (r.random((self.planes, self.rows, self.row_bytes // 4), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)).view(np.uint8)
        elif self.kind == "u16":
            x = r.integers(0, 1 << DEPTH, (self.planes, self.rows, self.row_bytes // 2)).astype("<u2").view(np.uint8)
        else:
            x = r.integers(0, 256, shape, dtype=np.uint8)
            if self.kind == "rgba":
                x[:, :, 3::4] = np.where(x[:, :, 3::4] & 1, 255, 0)
        win = np.full(self.span, self.guard, np.uint8)
        p, q, c = np.meshgrid(np.arange(self.planes), np.arange(self.rows), np.arange(self.row_bytes), indexing="ij")
        win[p * self.plane + q * self.row + c] = x.reshape(shape)
        return torch.from_numpy(win).cuda()


def compact(regions, windows):
    """a frame alone: every region as one window in a small buffer of its own, guard around it -> (the buffers, the views)"""
    bufs, views = {}, {}
    for r in regions:
        t = torch.full((r.span + 2 * RIM,), r.guard, dtype=torch.uint8, device="cuda")
        if r.role == "in":
            t[RIM:RIM + r.span] = windows[r.name]
        bufs[r.name] = t
        views[r.name] = View(t.data_ptr() + RIM, r.span, r.row, r.plane)
    return bufs, views


def run_far(pool, variant, regions, call, seed):
    """call(n, {name: View}) on the N frames far apart, and on every frame alone"""
    slots = {"in": 0, "out": 0}
    for r in regions:
        r.resolve(variant, slots[r.role], pool[r.role])
        slots[r.role] += 1
    ins, outs = [r for r in regions if r.role == "in"], [r for r in regions if r.role == "out"]
    data = [{r.name: r.data(seed + 10 * i + k) for k, r in enumerate(ins)} for i in range(N)]
    assert all(not torch.equal(data[0][r.name], data[i][r.name]) for r in ins for i in (1, 2)), "every frame has data of its own"
    want = []
    for i in range(N):
        bufs, views = compact(regions, data[i])
        call(1, views)
        torch.cuda.synchronize()
        for r in regions:
            t = bufs[r.name]
            assert (t[:RIM] == r.guard).all() and (t[RIM + r.span:] == r.guard).all(), "frame %d alone: bytes around %s were written" % (i, r.name)
            assert r.role == "out" or torch.equal(t[RIM:RIM + r.span], data[i][r.name]), "frame %d alone: the input %s was written" % (i, r.name)
        want.append({r.name: bufs[r.name][RIM:RIM + r.span] for r in outs})
        assert all(not (want[i][r.name] == r.guard).all() for r in outs), "the call wrote nothing"
    assert all(not torch.equal(want[0][r.name], want[i][r.name]) for r in outs for i in (1, 2)), "every frame has a result of its own"
    try:
        for r in ins:
            for i in range(N):
                r.window(i).copy_(data[i][r.name])
        call(N, {r.name: r.far() for r in regions})
        torch.cuda.synchronize()
        for i in range(N):
            for r in outs:
                got = r.window(i)
                assert torch.equal(got, want[i][r.name]), "frame %d, %s: %d of %d bytes differ from the frame alone" % (
                    i, r.name, int((got != want[i][r.name]).sum()), r.span)
            for r in ins:
                assert torch.equal(r.window(i), data[i][r.name]), "frame %d: the input %s was written" % (i, r.name)
    finally:
        check_guards(pool, regions)


def check_guards(pool, regions):
    """wipe the windows; every byte of both far buffers is the guard again (a buffer that is not is refilled, so the next case starts clean)"""
    for r in regions:
        for i in range(N):
            r.window(i).fill_(r.guard)
    bad = {role: dirty(buf, GUARD[role]) for role, buf in pool.items()}
    for role, cnt in bad.items():
        if cnt:
            pool[role].fill_(GUARD[role])
    assert not any(bad.values()), "bytes outside the frames were written (far buffer: count): %s" % bad


def test_the_strides_put_frames_past_2g_and_4g(pool):
    for a, s in STRIDE.items():
        assert s % a == 0 and LEAD + s > 1 << 31 and LEAD + 2 * s > 1 << 32
    assert STRIDE[1] % 2 == 1 and STRIDE_8 % 8 == 0
    assert all(dirty(buf, GUARD[role]) == 0 for role, buf in pool.items())


# ---- the luma blocks ----
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("to_plane", [True, False], ids=["to_plane", "from_plane"])
def test_luma_blocks(ctx, pool, to_plane, bits, variant):
    k = bits // 8
    regions = [Region("b", "in" if to_plane else "out", "u8" if bits == 8 else "u16", H, k * W),
               Region("p", "out" if to_plane else "in", "f32", 1, 4 * W * H, contiguous=True)]
    extra = () if bits == 8 else (DEPTH, 0)

    def call(n, R):
        b, p = R["b"], R["p"]
        if to_plane:
            getattr(ctx.w, "y%d_to_plane_device" % bits)(b.ptr, n, b.stride, b.row, W, H, LIMITED, *extra, p.ptr, p.stride)
        else:
            getattr(ctx.w, "plane_to_y%d_device" % bits)(p.ptr, n, p.stride, W, H, LIMITED, *extra, b.ptr, b.stride, b.row)
    run_far(pool, variant, regions, call, 100 + bits)


# ---- the chroma blocks ----
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("kind", ["2x", "sited", "resize"])
def test_chroma_blocks(ctx, pool, kind, bits, variant):
    k = bits // 8
    ow, oh = (53, 29) if kind == "resize" else (2 * CW, 2 * CH)
    regions = [Region("s", "in", "u8" if bits == 8 else "u16", CH, k * CW), Region("d", "out", "u8" if bits == 8 else "u16", oh, k * ow)]
    fn = getattr(ctx.w, {"2x": "chroma2x_u%d_device", "sited": "chroma2x_u%d_sited_device", "resize": "chroma_resize_u%d_device"}[kind] % bits)
    tail = {"2x": (), "sited": (TOPLEFT,), "resize": (W, H, 105, 57, 1, 1, TOPLEFT)}[kind]

    def call(n, R):
        s, d = R["s"], R["d"]
        src, dst = (s.ptr, n, s.stride, s.row, 1), (d.ptr, d.stride, d.row, 1)
        if bits == 16:
            src, dst = src + (0, CW, CH, DEPTH), dst + (0,)
        else:
            src = src + (CW, CH)
        fn(*src, *dst, ow, oh, *tail)
    run_far(pool, variant, regions, call, 200 + bits)


# ---- the two ends of the RGB route: the frames and the float planes both far apart ----
def yuv_side(ctx, bits, R, prefix):
    s = ctx.w.YuvPlanes() if bits == 8 else ctx.w.Yuv16Planes()
    y, u, v = (R[prefix + c] for c in "yuv")
    assert (u.stride, u.row) == (v.stride, v.row)
    s.y, s.y_stride, s.y_frame_stride = y.ptr, y.row, y.stride
    s.u, s.v, s.c_stride, s.c_frame_stride, s.c_px = u.ptr, v.ptr, u.row, u.stride, 1
    return s


def yuv_regions(ctx, prefix, role, bits, w, h):
    k, kind = bits // 8, "u8" if bits == 8 else "u16"
    cw, ch = ctx.w.yuv_chroma_size(w, h, YUV_420)
    return [Region(prefix + "y", role, kind, h, k * w), Region(prefix + "u", role, kind, ch, k * cw), Region(prefix + "v", role, kind, ch, k * cw)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("chroma", [YUV_420, YUV_420 | TOPLEFT], ids=["centred", "topleft"])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("to_rgb", [True, False], ids=["to_rgb", "from_rgb"])
def test_rgb_ends(ctx, pool, to_rgb, bits, chroma, variant):
    regions = yuv_regions(ctx, "", "in" if to_rgb else "out", bits, W, H) + [Region("f", "out" if to_rgb else "in", "f32", 1, 4 * W * H, planes=3, contiguous=True)]
    depth = () if bits == 8 else (DEPTH,)

    def call(n, R):
        side, f = yuv_side(ctx, bits, R, ""), R["f"]
        if to_rgb:
            getattr(ctx.w, "yuv%d_to_rgb_device" % bits)(side, n, W, H, chroma, LIMITED, *depth, BT709, f.ptr, f.stride, f.plane)
        else:
            getattr(ctx.w, "rgb_to_yuv%d_device" % bits)(f.ptr, f.stride, f.plane, n, W, H, chroma, LIMITED, *depth, BT709, side)
    run_far(pool, variant, regions, call, 300 + bits)


# ---- the TTA blocks: the images (uint8 forms) or the planes (float forms) far apart, the 8 variants of everything in compact buffers ----
def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "float"])
def test_tta_spread(ctx, pool, u8, variant):
    """ppi planes per far item (3 per uint8 image, 1 per float plane): variant k of item i's plane c lies at plane (k & 3) (ppi N) + ppi i + c"""
    ppi, ps = (3, IW * IH + 5) if u8 else (1, IW * IH + 5)
    src = Region("s", "in", "u8", IH, 3 * IW) if u8 else Region("s", "in", "f32", IH, 4 * IW)
    src.resolve(variant, 0, pool["in"])
    data = [src.data(400 + i) for i in range(N)]

    def spread(n, v):
        out = [torch.full((4 * ppi * n, ps), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
        if u8:
            ctx.w.tta_spread_u8_device(v.ptr, n, v.stride, v.row, 3, 0, 1, IW, IH, out[0].data_ptr(), out[1].data_ptr(), 4 * ps)
        else:
            ctx.w.tta_spread_device(v.ptr, n, v.stride, v.row, IW, IH, out[0].data_ptr(), out[1].data_ptr(), 4 * ps)
        torch.cuda.synchronize()
        return [o.view(4, n, ppi, ps) for o in out]
    try:
        for i in range(N):
            src.window(i).copy_(data[i])
        got = spread(N, src.far())
        for i in range(N):
            _, views = compact([src], {"s": data[i]})
            alone = spread(1, views["s"])
            for g, a, what in zip(got, alone, ("upright", "transposed")):
                assert not torch.isnan(a[..., :IW * IH]).any()
                assert bits_equal(g[:, i], a[:, 0]), "item %d: the %s variants differ from the item alone" % (i, what)
            assert torch.equal(src.window(i), data[i]), "the source was written"
    finally:
        check_guards(pool, [src])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "float"])
def test_tta_gather(ctx, pool, u8, variant):
    ppi, ps = (3 if u8 else 1), IW * IH + 5
    dst = Region("d", "out", "u8", IH, 3 * IW) if u8 else Region("d", "out", "f32", IH, 4 * IW)
    dst.resolve(variant, 0, pool["out"])
    g = torch.Generator(device="cpu").manual_seed(410)
    groups = [(torch.rand((4, N, ppi, ps), generator=g, dtype=torch.float32) * 1.3 - 0.15).cuda() for _ in range(2)]

    def gather(n, up, tr, v):
        if u8:
            ctx.w.tta_gather_u8_device(up.data_ptr(), tr.data_ptr(), 4 * ps, n, 3, 0, 3, IW, IH, v.ptr, v.stride, v.row, 3, 0)
        else:
            ctx.w.tta_gather_device(up.data_ptr(), tr.data_ptr(), 4 * ps, n, IW, IH, v.ptr, v.stride, v.row)
        torch.cuda.synchronize()
    try:
        gather(N, groups[0], groups[1], dst.far())
        for i in range(N):
            bufs, views = compact([dst], {})
            gather(1, *(x[:, i:i + 1].contiguous() for x in groups), views["d"])
            alone = bufs["d"][RIM:RIM + dst.span]
            assert not (alone == dst.guard).all()
            assert torch.equal(dst.window(i), alone), "item %d differs from the item alone" % i
    finally:
        check_guards(pool, [dst])


# ---- the batch forms of the image calls and of the head model's plane call ----
IMAGE_CALLS = [("process_image_rgb_u8_batch_device", ("rn", "rs"), 3), ("process_image_rgba_u8_batch_device", ("rn", "rs"), 4),
               ("process_image_rgb_u8_up2x_batch_device", ("rn", "head"), 3), ("process_image_rgba_u8_up2x_batch_device", ("rn", "head"), 4)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,models,ch", IMAGE_CALLS, ids=[c[0][len("process_image_"):-len("_device")] for c in IMAGE_CALLS])
def test_image_batches(ctx, pool, name, models, ch, variant):
    """noise + scale, one iteration; the RGBA calls with the tiled bleed at its default passes"""
    noise, scale = (ctx.model(m) for m in models)
    regions = [Region("i", "in", "rgba" if ch == 4 else "u8", IH, ch * IW), Region("o", "out", "u8", 2 * IH, ch * 2 * IW)]
    opts = ctx.opts()

    def call(n, R):
        i, o = R["i"], R["o"]
        getattr(ctx.w, name)(n, i.ptr, i.stride, i.row, IW, IH, o.ptr, o.stride, o.row, noise=noise, scale=scale, iterations=1, opts=opts)
    run_far(pool, variant, regions, call, 500 + ch)


@pytest.mark.parametrize("variant", VARIANTS)
def test_head_model_plane_batch(ctx, pool, variant):
    head = ctx.model("head")
    regions = [Region("i", "in", "f32", IH, 4 * IW, planes=3), Region("o", "out", "f32", 2 * IH, 8 * IW, planes=3)]
    opts = ctx.opts()

    def call(n, R):
        i, o = R["i"], R["o"]
        head.convert_planes_up2x_batch_device(n, 3, i.ptr, i.stride, i.plane, i.row, IW, IH, o.ptr, o.stride, o.plane, o.row, opts=opts)
    run_far(pool, variant, regions, call, 600)


# ---- the YUV frame calls: both sides far apart; whole, and in sub-batches of 2 + 1 ----
FRAME_CALLS = [("process_frames_yuv_u8_device", 8, False, False), ("process_frames_yuv_u8_rgb_device", 8, True, False),
               ("process_frames_yuv_u16_sized_device", 16, False, True), ("process_frames_yuv_u8_rgb_sized_device", 8, True, True)]


def frame_opts(ctx, noise, scale, planes, sub2):
    """the default options, or a workspace_mb under which the batched chains of both passes take two frames at a time (w2xc_batch_plan: host arithmetic)"""
    if not sub2:
        assert min(m.batch_plan(planes, W, H, nn2x, ctx.opts())[1] for m, nn2x in ((noise, False), (scale, True))) >= N, "the default: one sub-batch"
        return ctx.opts()
    for mb in range(1, 4096):
        o = ctx.opts(workspace_mb=mb)
        plans = [noise.batch_plan(planes, W, H, False, o), scale.batch_plan(planes, W, H, True, o)]
        if all(b for b, _ in plans) and min(s for _, s in plans) == 2:
            return o
        assert not all(b for b, _ in plans) or min(s for _, s in plans) < 2, "no budget gives a sub-batch of 2"
    raise AssertionError("no budget found")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("sub2", [True, False], ids=["sub2", "whole"])
@pytest.mark.parametrize("name,bits,rgb,sized", FRAME_CALLS, ids=[c[0][len("process_frames_"):-len("_device")] for c in FRAME_CALLS])
def test_frame_calls(ctx, pool, name, bits, rgb, sized, sub2, variant):
    noise, scale = (ctx.model(m) for m in (("rn", "rs") if rgb else ("yn", "ys")))
    ow, oh = (105, 57) if sized else (2 * W, 2 * H)
    regions = yuv_regions(ctx, "i", "in", bits, W, H) + yuv_regions(ctx, "o", "out", bits, ow, oh)
    kw = dict(noise=noise, scale=scale, iterations=1, range=LIMITED, opts=frame_opts(ctx, noise, scale, 3 if rgb else 1, sub2))
    if rgb:
        kw["matrix"] = BT709
    if bits == 16:
        kw["depth"] = DEPTH
    size = (ow, oh) if sized else ()

    def call(n, R):
        getattr(ctx.w, name)(n, W, H, YUV_420, yuv_side(ctx, bits, R, "i"), *size, yuv_side(ctx, bits, R, "o"), **kw)
    run_far(pool, variant, regions, call, 700 + bits)
