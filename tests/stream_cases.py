"""One row per device entry point (every prototype of include/w2xc_hip.h with a `hip_stream` parameter, every callable of the package whose name ends in
`_device`): the Python callable, the C symbol it reaches, and a builder of small arguments that says which device buffers the call reads and which it writes.
tests/test_stream_cases.py holds the table complete without a GPU; tests/test_gpu_stream_order.py runs every row on a caller's non-blocking stream.

A builder returns a Case: `ins` -- (buffer, real content, stale content) per buffer the call reads --, `outs` -- (buffer, its sentinel fill, a check of the rims
or None) per buffer it writes --, and `call(stream)`.  Buffers are whole allocations, rims included, laid out with the block tests' helpers (Lay, Lay16, Side,
Side16, Planes, make_side) and, for float planes, FLay below.  variant 1 of a row is a second call for the same scratch: other data, a smaller size.

Shapes: 17 x 33 planes and images for the model calls (two tile columns, three 8-row tiles), 70 x 38 frames at 4:2:0 with n = 3 for the frame calls, the block
tests' two-tile shapes for the blocks."""
import numpy as np

from tools import gen_model


class _Blocks:
    """the block tests' layout helpers, imported when a builder first asks: those modules (and tests/upconv_ref.py) need torch, the table and its
    completeness check (tests/test_stream_cases.py) do not"""

    def __getattr__(self, name):
        import test_gpu_yuv_blocks as b8
        import test_gpu_yuv16_blocks as b16
        import test_gpu_yuv_rgb_blocks as brgb
        return {"Lay": b8.Lay, "Lay16": b16.Lay16, "Side16": b16.Side16, "to_dev": b16.to_dev, "Planes": brgb.Planes, "make_side": brgb.make_side}[name]


B = _Blocks()
PLANAR = False          # tests/test_gpu_yuv_rgb_blocks.py: two chroma planes

RIM_F = 8
YUV_420, LIMITED, BT709, DEPTH16 = 0, 1, 1, 10
COSITED_X = 0x10
FUSION_PROG = 6

# the models: the 7-layer Y chains of tools/gen_model.py, the three-plane chains of tests/test_gpu_rgb.py and tests/test_gpu_upconv_batch.py, the published
# head topology (tests/upconv_ref.py)
MODEL_ARRAYS = {
    "yn": lambda: (gen_model.synth_layers(seed=gen_model.SEEDS["noise1"]), None),
    "ys": lambda: (gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]), None),
    "rn": lambda: (gen_model.synth_layers([3, 32, 32, 3], 403), None),
    "rs": lambda: (gen_model.synth_layers([3, 32, 64, 64, 3], 302), None),
    "head": lambda: __import__("upconv_ref").head_model(gen_model.TOPOLOGY_UPCONV7, 3, gen_model.SEEDS["upconv7"]),
}


class Ctx:
    """what the builders need: the package, torch, one _ModelSet per name"""

    def __init__(self, w2xc, torch=None):
        self.w, self.torch = w2xc, torch
        self._models = {}

    def model(self, name):
        if name not in self._models:
            layers, head = MODEL_ARRAYS[name]()
            self._models[name] = self.w._ModelSet.from_layers(layers, head=head)
        return self._models[name]

    def opts(self, **kw):
        return self.w.make_opts(device=0, **kw)

    def dev(self, a):
        a = np.ascontiguousarray(a)
        return B.to_dev(a) if a.dtype == np.uint16 else self.torch.from_numpy(a).cuda()


class FLay:
    """float planes in a buffer of NaN with rims: an array of `shape` whose rows, planes and images lie a few floats further apart than they are long (tight:
    contiguous), RIM_F floats in front and behind"""

    def __init__(self, shape, tight=False):
        self.shape = tuple(shape)
        st = [1]
        for k, d in enumerate(reversed(self.shape[1:])):
            st.append(d * st[-1] + (0 if tight else (3, 5, 7, 9)[k]))
        self.strides = tuple(reversed(st))
        self.total = 2 * RIM_F + self.shape[0] * self.strides[0]

    def bytes(self, axis):
        return 4 * self.strides[axis]

    def index(self):
        return RIM_F + sum(g * s for g, s in zip(np.indices(self.shape), self.strides))

    def scatter(self, x):
        buf = np.full(self.total, np.nan, np.float32)
        buf[self.index()] = x
        return buf

    def gather(self, buf):
        idx = self.index()
        rest = np.ones(self.total, bool)
        rest[idx] = False
        assert np.isnan(buf[rest]).all(), "floats outside the planes were written"
        return buf[idx]


class Case:
    def __init__(self, ctx):
        self.ctx, self.ins, self.outs, self.keep, self.call = ctx, [], [], [], None

    def inp(self, real, stale):
        """a buffer the call reads, from two whole host buffers of one layout; -> the device buffer (holding the stale data)"""
        r, s = self.ctx.dev(real), self.ctx.dev(stale)
        self.ins.append((s.clone(), r, s))
        return self.ins[-1][0]

    def out(self, fill, check=None):
        """a buffer the call writes, from its host image before the call; check(host buffer) asserts the rims"""
        f = self.ctx.dev(fill)
        self.outs.append((f.clone(), f, check))
        return self.outs[-1][0]

    def adopt_in(self, buf, real, stale):
        self.ins.append((buf, real, stale))

    def adopt_out(self, buf, check=None):
        self.outs.append((buf, buf.clone(), check))

    # -- the layouts the rows share --
    def floats_in(self, shape, seed, tight=False, lo=0.0, hi=1.0):
        lay = FLay(shape, tight)
        g = [np.random.default_rng(s).random(lay.shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo) for s in (seed, seed + 50)]
        return self.inp(lay.scatter(g[0]), lay.scatter(g[1])).data_ptr() + 4 * RIM_F, lay

    def floats_out(self, shape, tight=False):
        lay = FLay(shape, tight)
        return self.out(np.full(lay.total, np.nan, np.float32), lay.gather).data_ptr() + 4 * RIM_F, lay

    def bytes_in(self, n, rows, cols, seed, px=1, alpha=False):
        lay = B.Lay(n, rows, cols, px)
        g = [np.random.default_rng(s).integers(0, 256, (n, rows, cols), dtype=np.uint8) for s in (seed, seed + 50)]
        if alpha:       # rows of RGBA pixels: half of them transparent
            for a in g:
                a[:, :, 3::4] = np.where(a[:, :, 3::4] & 1, 255, 0)
        return self.inp(lay.scatter(g[0], 0x5A), lay.scatter(g[1], 0x5A)).data_ptr() + lay.off, lay

    def bytes_out(self, n, rows, cols, px=1):
        lay = B.Lay(n, rows, cols, px)
        return self.out(np.full(lay.total, 0xAB, np.uint8), lambda b: lay.gather(b, 0xAB)).data_ptr() + lay.off, lay

    def words_in(self, n, rows, cols, seed, px=1):
        lay = B.Lay16(n, rows, cols, px)
        g = [np.random.default_rng(s).integers(0, 1 << DEPTH16, (n, rows, cols)).astype(np.uint16) for s in (seed, seed + 50)]
        return self.inp(lay.scatter(g[0], 0x5A5A), lay.scatter(g[1], 0x5A5A)).data_ptr() + 2 * lay.off, lay

    def words_out(self, n, rows, cols, px=1):
        lay = B.Lay16(n, rows, cols, px)
        return self.out(np.full(lay.total, 0xABCD, np.uint16), lambda b: lay.gather(b.view(np.uint16))).data_ptr() + 2 * lay.off, lay

    def side_in(self, bits, n, w, h, seed):
        """n frames of w x h at 4:2:0 in a Side / Side16 of the block tests; -> the side"""
        ctx = self.ctx
        side = B.make_side(ctx.w, n, w, h, YUV_420, PLANAR, False) if bits == 8 else B.Side16(ctx.w, n, w, h, YUV_420, "planar", 0, 1)
        images = []
        for s in (seed + 50, seed):
            r = np.random.default_rng(s)
            dt, top = (np.uint8, 256) if bits == 8 else (np.uint16, 1 << DEPTH16)
            Y, U, V = (r.integers(0, top, shp).astype(dt) for shp in ((n, h, w), (n, side.ch, side.cw), (n, side.ch, side.cw)))
            side.upload(Y, U, V) if bits == 8 else side.upload(Y, U, V, DEPTH16)
            images.append([b.clone() for b in [side.by] + side.bc])
        for buf, stale, real in zip([side.by] + side.bc, *images):
            self.adopt_in(buf, real, stale)
        self.keep.append(side)
        return side

    def side_out(self, bits, n, w, h):
        ctx = self.ctx
        side = B.make_side(ctx.w, n, w, h, YUV_420, PLANAR, False) if bits == 8 else B.Side16(ctx.w, n, w, h, YUV_420, "planar", 0, 1)
        lays = [side.ly] + [side.lc] * len(side.bc)
        for buf, lay in zip([side.by] + side.bc, lays):
            self.adopt_out(buf, (lambda b, lay=lay: lay.gather(b, 0xAB)) if bits == 8 else (lambda b, lay=lay: lay.gather(b.view(np.uint16))))
        self.keep.append(side)
        return side


class Row:
    def __init__(self, id, symbol, py, build, family, tta=False, waits=None):
        """py: "name" (module level), "_ModelSet.name", or None for a C symbol the package has no wrapper of; family: "model" / "frame" / "block";
        waits: the source line at which the call waits for the device in the warm state, where it does (None: it must not)"""
        self.id, self.symbol, self.py, self.build, self.family, self.tta, self.waits = id, symbol, py, build, family, tta, waits


def size(v):
    """(h, w) of the model calls: 17 x 33, and for a second call on the same scratch 13 x 29"""
    return (13, 29) if v else (17, 33)


def frame_size(v):
    """(w, h, out_w, out_h of the sized calls)"""
    return (66, 34, 101, 55) if v else (70, 38, 105, 57)


def sub_batch_opts(ctx, model, n_in, w, h, want_sub, nn2x=False):
    """a workspace_mb under which a batch of w x h images runs in sub-batches of want_sub (host arithmetic: w2xc_batch_plan)"""
    for mb in range(1, 4096):
        o = ctx.w.make_opts(device=0, workspace_mb=mb)
        batched, sub = model.batch_plan(n_in, w, h, nn2x, o)
        if batched and sub == want_sub:
            return o
        assert not batched or sub < want_sub, "no budget gives a sub-batch of %d" % want_sub
    raise AssertionError("no budget found")


# ---- model calls on float planes ----
def planes_row(id, symbol, method, model, in_shape, out_shape, call, opts=None, family="model"):
    """in_shape / out_shape: functions of (h, w); call(ms, pi, li, po, lo, w, h, stream, opts)"""
    def build(ctx, v=0):
        h, w = size(v)
        c = Case(ctx)
        ms = ctx.model(model)
        pi, li = c.floats_in(in_shape(h, w), 1000 + 7 * v)
        po, lo = c.floats_out(out_shape(h, w))
        o = opts(ctx, ms, w, h) if opts else ctx.opts()
        c.call = lambda stream: call(ms, pi, li, po, lo, w, h, stream, o)
        c.keep.append(o)
        return c
    return Row(id, symbol, "_ModelSet." + method, build, family)


def _plane_rows():
    one, two = (lambda h, w: (h, w)), (lambda h, w: (2 * h, 2 * w))
    three, three2 = (lambda h, w: (3, h, w)), (lambda h, w: (3, 2 * h, 2 * w))
    batch, batch2 = (lambda h, w: (3, 3, h, w)), (lambda h, w: (3, 3, 2 * h, 2 * w))

    def convert(ms, pi, li, po, lo, w, h, st, o):
        ms.convert_device(pi, li.bytes(0), w, h, po, lo.bytes(0), stream=st, opts=o)

    def planes_call(method, lead=()):
        def call(ms, pi, li, po, lo, w, h, st, o):
            getattr(ms, method)(*lead, 3, pi, li.bytes(0), li.bytes(1), w, h, po, lo.bytes(0), lo.bytes(1), stream=st, opts=o)
        return call

    def batch_call(method, **kw):
        def call(ms, pi, li, po, lo, w, h, st, o):
            getattr(ms, method)(3, pi, li.bytes(0), li.bytes(1), w, h, po, lo.bytes(0), lo.bytes(1), stream=st, opts=o, **kw)
        return call

    def planes_batch_call(method):
        def call(ms, pi, li, po, lo, w, h, st, o):
            getattr(ms, method)(3, 3, pi, li.bytes(0), li.bytes(1), li.bytes(2), w, h, po, lo.bytes(0), lo.bytes(1), lo.bytes(2), stream=st, opts=o)
        return call

    def rows_call(ms, pi, li, po, lo, w, h, st, o):
        ms.convert_rows_device(pi, li.bytes(0), h, 0, w, h, 4, h - 3, po, lo.bytes(0), stream=st, opts=o)

    def filter_call(ms, pi, li, po, lo, w, h, st, o):
        ms.filter_device(1, 32, pi, li.strides, w, h, po, lo.strides, stream=st, opts=o)

    return [
        planes_row("convert", "w2xc_convert_plane_device", "convert_device", "yn", one, one, convert),
        planes_row("convert-banded", "w2xc_convert_plane_device", "convert_device", "yn", one, one, convert, opts=lambda ctx, ms, w, h: ctx.opts(band_rows=8)),
        planes_row("convert-prog", "w2xc_convert_plane_device", "convert_device", "yn", one, one, convert, opts=lambda ctx, ms, w, h: ctx.opts(fusion=FUSION_PROG)),
        planes_row("convert_nn2x", "w2xc_convert_plane_nn2x_device", "convert_nn2x_device", "ys", one, two,
                   lambda ms, pi, li, po, lo, w, h, st, o: ms.convert_nn2x_device(pi, li.bytes(0), w, h, po, lo.bytes(0), stream=st, opts=o)),
        planes_row("convert_rows", "w2xc_convert_rows_device", "convert_rows_device", "yn", one, lambda h, w: (h - 7, w), rows_call),
        planes_row("convert_planes", "w2xc_convert_planes_device", "convert_planes_device", "rn", three, three, planes_call("convert_planes_device")),
        planes_row("convert_planes_nn2x", "w2xc_convert_planes_nn2x_device", "convert_planes_nn2x_device", "rs", three, three2,
                   planes_call("convert_planes_nn2x_device")),
        planes_row("convert_planes_up2x", "w2xc_convert_planes_up2x_device", "convert_planes_up2x_device", "head", three, three2,
                   planes_call("convert_planes_up2x_device")),
        planes_row("convert_planes_tta", "w2xc_convert_planes_tta_device", "convert_planes_tta_device", "rn", three, three,
                   lambda ms, pi, li, po, lo, w, h, st, o: ms.convert_planes_tta_device(3, pi, li.bytes(0), li.bytes(1), w, h, po, lo.bytes(0), lo.bytes(1),
                                                                                        stream=st, opts=o)),
        planes_row("convert_batch", "w2xc_convert_batch_device", "convert_batch_device", "yn", three, three, batch_call("convert_batch_device")),
        planes_row("convert_batch-nn2x", "w2xc_convert_batch_device", "convert_batch_device", "ys", three, three2, batch_call("convert_batch_device", nn2x=True)),
        planes_row("convert_batch-sub2", "w2xc_convert_batch_device", "convert_batch_device", "yn", three, three, batch_call("convert_batch_device"),
                   opts=lambda ctx, ms, w, h: sub_batch_opts(ctx, ms, 1, w, h, 2)),
        planes_row("convert_batch_tta", "w2xc_convert_batch_tta_device", "convert_batch_tta_device", "yn", three, three, batch_call("convert_batch_tta_device")),
        planes_row("convert_planes_batch", "w2xc_convert_planes_batch_device", "convert_planes_batch_device", "rn", batch, batch,
                   planes_batch_call("convert_planes_batch_device")),
        planes_row("convert_planes_up2x_batch", "w2xc_convert_planes_up2x_batch_device", "convert_planes_up2x_batch_device", "head", batch, batch2,
                   planes_batch_call("convert_planes_up2x_batch_device")),
        planes_row("filter", "w2xc_layer_filter_device", "filter_device", "yn", lambda h, w: (32, h, w), lambda h, w: (32, h, w), filter_call),
    ]


# ---- model calls on uint8 images ----
def image_row(id, symbol, py, models, n=None, ch=3, tta=False, call=None, **kw):
    """noise + scale, one iteration; n: a batch of n images; ch: bytes per pixel; call: for the entries with a signature of their own"""
    def build(ctx, v=0):
        h, w = size(v)
        c = Case(ctx)
        noise, scale = (ctx.model(m) if m else None for m in models)
        pi, li = c.bytes_in(n or 1, h, ch * w, 2000 + 7 * v, alpha=(ch == 4))
        po, lo = c.bytes_out(n or 1, 2 * h, ch * 2 * w)
        o = ctx.opts()
        c.keep.append(o)
        if call:
            c.call = lambda stream: call(ctx, noise, scale, pi, li, po, lo, w, h, stream, o)
        else:
            lead = () if n is None else (n,)
            strides = (lambda lay: (lay.row,)) if n is None else (lambda lay: (lay.frame, lay.row))
            extra = dict(kw, tta=True) if tta else kw
            c.call = lambda stream: getattr(ctx.w, py)(*lead, pi, *strides(li), w, h, po, *strides(lo), noise=noise, scale=scale, iterations=1, stream=stream,
                                                        opts=o, **extra)
        return c
    return Row(id, symbol, py, build, "model", tta=tta)


def _image_rows():
    def plain(ctx, noise, scale, pi, li, po, lo, w, h, st, o):
        rc = ctx.w.lib().w2xc_process_image_u8_device(noise.handle, scale.handle, pi, li.row, w, h, po, lo.row, 1, st or None, o)
        if rc != 0:     # (as the package's wrappers: tests/test_gpu_fail_paths.py reads the code)
            raise ctx.w.W2xcError(rc, ctx.w.last_error())

    def scale2x(ctx, noise, scale, pi, li, po, lo, w, h, st, o):
        scale.scale2x_image_u8_device(pi, li.row, w, h, po, lo.row, iterations=1, stream=st, opts=o)

    Y, RGB, HEAD = ("yn", "ys"), ("rn", "rs"), ("rn", "head")
    rows = [image_row("scale2x_image_u8", "w2xc_scale2x_image_u8_device", "_ModelSet.scale2x_image_u8_device", (None, "ys"), call=scale2x),
            image_row("process_image_u8-plain", "w2xc_process_image_u8_device", None, Y, call=plain)]
    for tta in (False, True):
        t, s = ("-tta", "_tta") if tta else ("", "")
        rows += [
            image_row("process_image_u8" + t, "w2xc_process_image_u8%s_device" % (s or "_ex"), "process_image_u8_device", Y, tta=tta),
            image_row("process_image_u8_batch" + t, "w2xc_process_image_u8_batch%s_device" % s, "process_image_u8_batch_device", Y, n=3, tta=tta),
            image_row("process_image_rgb_u8" + t, "w2xc_process_image_rgb_u8%s_device" % (s or "_ex"), "process_image_rgb_u8_device", RGB, tta=tta),
            image_row("process_image_rgb_u8_batch" + t, "w2xc_process_image_rgb_u8_batch%s_device" % s, "process_image_rgb_u8_batch_device", RGB, n=3, tta=tta),
            image_row("process_image_rgb_u8_up2x_batch" + t, "w2xc_process_image_rgb_u8_up2x_batch_device", "process_image_rgb_u8_up2x_batch_device", HEAD, n=3,
                      tta=tta),
            image_row("process_image_rgba_u8" + t, "w2xc_process_image_rgba_u8_batch_tta_device" if tta else "w2xc_process_image_rgba_u8_ex_device",
                      "process_image_rgba_u8_device", Y, ch=4, tta=tta),
            image_row("process_image_rgba_u8_batch" + t, "w2xc_process_image_rgba_u8_batch%s_device" % s, "process_image_rgba_u8_batch_device", RGB, n=3, ch=4,
                      tta=tta),
            image_row("process_image_rgba_u8_up2x_batch" + t, "w2xc_process_image_rgba_u8_up2x_batch%s_device" % s, "process_image_rgba_u8_up2x_batch_device",
                      HEAD, n=3, ch=4, tta=tta),
        ]
    return rows


# ---- YUV frame calls ----
def frame_row(bits, rgb, sized):
    name = "process_frames_yuv_u%d%s%s_device" % (bits, "_rgb" if rgb else "", "_sized" if sized else "")

    def build(ctx, v=0):
        w, h, ow, oh = frame_size(v)
        if not sized:
            ow, oh = 2 * w, 2 * h
        c = Case(ctx)
        noise, scale = (ctx.model(m) for m in (("rn", "rs") if rgb else ("yn", "ys")))
        i, o = c.side_in(bits, 3, w, h, 3000 + 7 * v), c.side_out(bits, 3, ow, oh)
        kw = dict(noise=noise, scale=scale, iterations=1, range=LIMITED, opts=ctx.opts())
        if rgb:
            kw["matrix"] = BT709
        if bits == 16:
            kw["depth"] = DEPTH16
        size_args = (ow, oh) if sized else ()
        c.call = lambda stream: getattr(ctx.w, name)(3, w, h, YUV_420, i.s, *size_args, o.s, stream=stream, **kw)
        return c
    return Row(name[:-7], "w2xc_" + name, name, build, "frame")


# ---- blocks without a model ----
def block(id, symbol, py, build):
    return Row(id, symbol, py, build, "block")


def _luma_rows():
    n, h, w = 3, 37, 53

    def y8_in(ctx, v=0):
        c = Case(ctx)
        pi, li = c.bytes_in(n, h, w, 4000)
        po, lo = c.floats_out((n, h * w))
        c.call = lambda st: ctx.w.y8_to_plane_device(pi, n, li.frame, li.row, w, h, LIMITED, po, lo.bytes(0), stream=st)
        return c

    def y8_out(ctx, v=0):
        c = Case(ctx)
        pi, li = c.floats_in((n, h * w), 4001, lo=-0.25, hi=1.25)
        po, lo = c.bytes_out(n, h, w)
        c.call = lambda st: ctx.w.plane_to_y8_device(pi, n, li.bytes(0), w, h, LIMITED, po, lo.frame, lo.row, stream=st)
        return c

    def y16_in(ctx, v=0):
        c = Case(ctx)
        pi, li = c.words_in(n, h, w, 4002)
        po, lo = c.floats_out((n, h * w))
        c.call = lambda st: ctx.w.y16_to_plane_device(pi, n, 2 * li.frame, 2 * li.row, w, h, LIMITED, DEPTH16, 0, po, lo.bytes(0), stream=st)
        return c

    def y16_out(ctx, v=0):
        c = Case(ctx)
        pi, li = c.floats_in((n, h * w), 4003, lo=-0.25, hi=1.25)
        po, lo = c.words_out(n, h, w)
        c.call = lambda st: ctx.w.plane_to_y16_device(pi, n, li.bytes(0), w, h, LIMITED, DEPTH16, 0, po, 2 * lo.frame, 2 * lo.row, stream=st)
        return c

    return [block("y8_to_plane", "w2xc_y8_to_plane_device", "y8_to_plane_device", y8_in), block("plane_to_y8", "w2xc_plane_to_y8_device", "plane_to_y8_device", y8_out),
            block("y16_to_plane", "w2xc_y16_to_plane_device", "y16_to_plane_device", y16_in),
            block("plane_to_y16", "w2xc_plane_to_y16_device", "plane_to_y16_device", y16_out)]


def _chroma_rows():
    n, ch, cw, oh, ow = 3, 21, 37, 41, 73               # the 2x kernels: the block tests' three planes, an odd cropped output
    W, H, OW, OH = 70, 38, 105, 57                      # the resize kernels: the chroma of a 70 x 38 frame at 4:2:0 for a 105 x 57 one
    rcw, rch, rocw, roch = 35, 19, 53, 29

    def make(bits, kind):
        def build(ctx, v=0):
            c = Case(ctx)
            k = 1 if bits == 8 else 2
            sw, sh, dw, dh = (rcw, rch, rocw, roch) if kind == "resize" else (cw, ch, ow, oh)
            pi, li = (c.bytes_in if bits == 8 else c.words_in)(n, sh, sw, 4100 + bits)
            po, lo = (c.bytes_out if bits == 8 else c.words_out)(n, dh, dw)
            src = (pi, n, k * li.frame, k * li.row, 1) + ((cw, ch) if kind != "resize" else (rcw, rch))
            dst = (po, k * lo.frame, k * lo.row, 1)
            if bits == 16:
                src, dst = src[:5] + (0,) + src[5:] + (DEPTH16,), dst + (0,)
            tail = {"2x": (), "sited": (COSITED_X,), "resize": (W, H, OW, OH, 1, 1, COSITED_X)}[kind]
            fn = getattr(ctx.w, py)
            c.call = lambda st: fn(*src, *dst, dw, dh, *tail, stream=st)
            return c
        py = {"2x": "chroma2x_u%d_device", "sited": "chroma2x_u%d_sited_device", "resize": "chroma_resize_u%d_device"}[kind] % bits
        return block(py[:-7], "w2xc_" + py, py, build)
    return [make(bits, kind) for bits in (8, 16) for kind in ("2x", "sited", "resize")]


def _rgb_end_rows():
    n, w, h = 3, 67, 35

    def make(bits, to_rgb):
        py = ("yuv%d_to_rgb_device" if to_rgb else "rgb_to_yuv%d_device") % bits

        def build(ctx, v=0):
            c = Case(ctx)
            P = B.Planes(n, w, h)
            depth = (DEPTH16,) if bits == 16 else ()
            if to_rgb:
                side = c.side_in(bits, n, w, h, 4200 + bits)
                d = c.out(np.full(P.total, np.nan, np.float32), P.gather)
                c.call = lambda st: getattr(ctx.w, py)(side.s, n, w, h, YUV_420, LIMITED, *depth, BT709, d.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, stream=st)
            else:
                x = [(np.random.default_rng(s).random((n, 3, h, w), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)) for s in (4300 + bits, 4350 + bits)]
                d = c.inp(P.scatter(x[0]), P.scatter(x[1]))
                side = c.side_out(bits, n, w, h)
                c.call = lambda st: getattr(ctx.w, py)(d.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, n, w, h, YUV_420, LIMITED, *depth, BT709, side.s, stream=st)
            return c
        return block(py[:-7], "w2xc_" + py, py, build)
    return [make(bits, to_rgb) for bits in (8, 16) for to_rgb in (True, False)]


def _colour_rows():
    h, w = 19, 67        # more than one 256-thread block, an odd width

    def lib_call(ctx, name, *args):
        rc = getattr(ctx.w.lib(), name)(*args)      # (the argument types are declared: integers pass as pointers)
        if rc != 0:
            raise ctx.w.W2xcError(rc, ctx.w.last_error())

    def u8_to(name, py):
        def build(ctx, v=0):
            c = Case(ctx)
            pi, li = c.bytes_in(1, h, 3 * w, 4400)
            po, lo = c.floats_out((3, h, w), tight=True)
            if py:
                c.call = lambda st: ctx.w.u8_to_rgb_device(pi, li.row, w, h, po, stream=st)
            else:
                c.call = lambda st: lib_call(ctx, name, pi, li.row, w, h, po, po + lo.bytes(0), po + 2 * lo.bytes(0), st or None)
            return c
        return block(name[5:-7], name, py, build)

    def to_u8(name, py):
        def build(ctx, v=0):
            c = Case(ctx)
            pi, li = c.floats_in((3, h, w), 4401, tight=True, lo=-0.2, hi=1.2)
            po, lo = c.bytes_out(1, h, 3 * w)
            if py:
                c.call = lambda st: ctx.w.rgb_to_u8_device(pi, w, h, po, lo.row, stream=st)
            else:
                c.call = lambda st: lib_call(ctx, name, pi, pi + li.bytes(0), pi + 2 * li.bytes(0), w, h, po, lo.row, st or None)
            return c
        return block(name[5:-7], name, py, build)

    def cubic(ctx, v=0):
        c = Case(ctx)
        pi, _ = c.floats_in((h, w), 4402, tight=True)
        po, _ = c.floats_out((2 * h, 2 * w), tight=True)
        c.call = lambda st: lib_call(ctx, "w2xc_resize2x_cubic_device", pi, w, h, po, st or None)
        return c

    def linear(ctx, v=0):
        c = Case(ctx)
        pi, _ = c.floats_in((2 * h, 2 * w), 4403, tight=True)
        po, _ = c.floats_out((29, 101), tight=True)
        c.call = lambda st: ctx.w.resize_linear_device(pi, 2 * w, 2 * h, po, 101, 29, stream=st)
        return c

    def bleed(ctx, v=0):
        c = Case(ctx)
        pi, li = c.bytes_in(1, h, 4 * w, 4404, alpha=True)
        po, lo = c.bytes_out(1, h, 3 * w)
        c.call = lambda st: ctx.w.bleed_rgba_u8_device(pi, li.row, w, h, 3, po, lo.row, stream=st)
        return c

    return [u8_to("w2xc_u8_to_rgb_device", "u8_to_rgb_device"), to_u8("w2xc_rgb_to_u8_device", "rgb_to_u8_device"), u8_to("w2xc_u8_to_yuv_device", None),
            to_u8("w2xc_yuv_to_u8_device", None), block("resize2x_cubic", "w2xc_resize2x_cubic_device", None, cubic),
            block("resize_linear", "w2xc_resize_linear_device", "resize_linear_device", linear),
            block("bleed_rgba_u8", "w2xc_bleed_rgba_u8_device", "bleed_rgba_u8_device", bleed)]


def _tta_rows():
    n, h, w = 3, 19, 37      # more than one tile each way

    def spread(ctx, v=0):
        c = Case(ctx)
        pi, li = c.floats_in((n, h, w), 4500)
        pu, lu = c.floats_out((4 * n, h * w))
        pt, _ = c.floats_out((4 * n, h * w))
        c.call = lambda st: ctx.w.tta_spread_device(pi, n, li.bytes(0), li.bytes(1), w, h, pu, pt, lu.bytes(0), stream=st)
        return c

    def gather(ctx, v=0):
        c = Case(ctx)
        pu, lu = c.floats_in((4 * n, h * w), 4501)
        pt, _ = c.floats_in((4 * n, h * w), 4502)
        po, lo = c.floats_out((n, h, w))
        c.call = lambda st: ctx.w.tta_gather_device(pu, pt, lu.bytes(0), n, w, h, po, lo.bytes(0), lo.bytes(1), stream=st)
        return c

    def spread_u8(ctx, v=0):
        c = Case(ctx)
        pi, li = c.bytes_in(n, h, 3 * w, 4503)
        pu, lu = c.floats_out((4 * 3 * n, h * w))
        pt, _ = c.floats_out((4 * 3 * n, h * w))
        c.call = lambda st: ctx.w.tta_spread_u8_device(pi, n, li.frame, li.row, 3, 0, 1, w, h, pu, pt, lu.bytes(0), stream=st)
        return c

    def gather_u8(ctx, v=0):
        c = Case(ctx)
        pu, lu = c.floats_in((4 * 3 * n, h * w), 4504, lo=-0.2, hi=1.2)
        pt, _ = c.floats_in((4 * 3 * n, h * w), 4505, lo=-0.2, hi=1.2)
        po, lo = c.bytes_out(n, h, 3 * w)
        c.call = lambda st: ctx.w.tta_gather_u8_device(pu, pt, lu.bytes(0), n, 3, 0, 3, w, h, po, lo.frame, lo.row, 3, 0, stream=st)
        return c

    return [block("tta_spread", "w2xc_tta_spread_device", "tta_spread_device", spread), block("tta_gather", "w2xc_tta_gather_device", "tta_gather_device", gather),
            block("tta_spread_u8", "w2xc_tta_spread_u8_device", "tta_spread_u8_device", spread_u8),
            block("tta_gather_u8", "w2xc_tta_gather_u8_device", "tta_gather_u8_device", gather_u8)]


def rows():
    r = (_plane_rows() + _image_rows() + [frame_row(bits, rgb, sized) for sized in (False, True) for bits in (8, 16) for rgb in (False, True)]
         + _luma_rows() + _chroma_rows() + _rgb_end_rows() + _colour_rows() + _tta_rows())
    assert len({x.id for x in r}) == len(r), "row ids are unique"
    return tuple(r)


ROWS = rows()
BY_ID = {r.id: r for r in ROWS}
# the positive control's three rows: a model call, a frame call, a block
CONTROL = ("convert", "process_frames_yuv_u8", "chroma2x_u8")
