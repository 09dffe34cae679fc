#!/usr/bin/env python3
"""tools/w2xc_y4m.py in.y4m out.y4m -m noise|scale|noise_scale --model_dir DIR [--noise_level N] [--range full|limited] [--matrix bt601|bt709|bt2020]
                     [--frames_per_call N] [--siting center|left|topleft|auto] [--size WxH | --scale_ratio R]

An 8-bit YUV4MPEG2 stream through the YUV frame calls.  The route follows the loaded models, as in tools/w2xc_cli.py.  Y models (one plane in, one out) go
through w2xc_process_frames_yuv_u8: luma through the models, chroma enlarged on bytes -- no RGB image, no colour matrix; --matrix is ignored.  Models whose
first layer takes three planes -- three-plane models and the upconv_7 schema, whose scale model enlarges by itself -- go through
w2xc_process_frames_yuv_u8_rgb, by the colour matrix --matrix (default: bt709 for streams of 720 rows and more, bt601 below); a Cmono stream has no colour
to convert and is refused with such models.
The reader and the writer are pure Python (numpy for the planes): colour spaces C420* (C420, C420jpeg, C420mpeg2, C420paldv: all of them
(w + 1) / 2 x (h + 1) / 2 chroma), C422, C444 and Cmono; no C tag means C420jpeg, as the format says.
--siting says where a chroma sample sits (include/w2xc_hip.h, "Chroma siting"): center (the default: JPEG / MPEG-1, whatever the C tag says), left (on the left
luma column: MPEG-2, H.264, HEVC), topleft (on the top-left luma sample: BT.2020 / UHD) -- on the axes the stream's layout subsamples --, or auto, by the C
tag: C420mpeg2 and C422 are left, C420jpeg, C420, no tag and the deeper CxxxpD forms center, and C420paldv is refused: its Cb and Cr sit on different lines,
which no call here corrects.  The C tag is passed on unchanged.
The range is the stream's XCOLORRANGE=FULL|LIMITED where present, otherwise --range (default limited).  Frames go through the host call in groups of
--frames_per_call.  With a scale step the W and H fields are doubled; F (the frame rate) and A (the pixel aspect) are those of the input -- twice the samples
in both directions change neither --, every other header field is passed on as it is.  Interlaced streams (I other than p / ?) are refused: fields would have
to be enlarged separately.
--size WxH and --scale_ratio R name the output size (include/w2xc_hip.h, "Sized YUV frames": the _sized frame calls).  --size: as many 2x steps as reach it
(W2XC_ITERATIONS_AUTO's rule), the last level shrunk linearly, chroma resized in one step; the output is never smaller than the input and at most 16 times it a
side.  --scale_ratio, by the reference's rule: iterations = ceil(log2 R), the output int(W * R) x int(H * R); R = 1 needs a noise model, R < 1 is
refused.  Either needs a scale model where a 2x step is taken (-m scale or noise_scale).  The W and H of the written header follow; without either option the
tool behaves as before.
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAGIC = b"YUV4MPEG2"
# colour-space tag -> the chroma layout's name (the values of w2xc_amd.YUV_*: 420 = 0, 422 = 1, 444 = 2, 400 = 3)
LAYOUTS = {"420": 0, "422": 1, "444": 2, "mono": 3}


MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}   # (the values of w2xc_amd.MATRIX_*)
MONO_RGB = "Cmono stream with models that take R, G and B: a grey frame has no colour to convert -- use Y models (one plane in, one plane out)"


# --siting: the flags or-ed onto the layout (the values of w2xc_amd.CHROMA_COSITED_X / _Y)
COSITED_X, COSITED_Y = 0x10, 0x20
SITINGS = ("center", "left", "topleft", "auto")
PALDV = "C420paldv with --siting auto: its Cb and Cr samples sit on different lines, which no call corrects -- name a siting (center, left or topleft)"


INTERLACED = "interlaced stream (I%s): not supported -- its fields would have to be enlarged separately; deinterlace first"


class Y4mError(ValueError):
    pass


def layout_of(tag):
    """the chroma layout of a C tag's value: 420jpeg / 420mpeg2 / 420paldv / 420 -> 0, 422 -> 1, 444 -> 2, mono -> 3; everything else (10-bit forms such as
    420p10, 444alpha) is refused"""
    if tag in ("420", "420jpeg", "420mpeg2", "420paldv"):
        return LAYOUTS["420"]
    if tag in ("422", "444", "mono"):
        return LAYOUTS[tag]
    raise Y4mError("unsupported colour space C%s (8-bit C420*, C422, C444 and Cmono only; 9- to 16-bit streams: tools/w2xc_y4m16.py)" % tag)


def siting_flags(siting, tag, layout):
    """the siting flags of a stream: --siting, the C tag's value (None: no tag) and its layout -> COSITED_X | COSITED_Y, only on the axes the layout subsamples"""
    if siting == "auto":
        if tag == "420paldv":
            raise Y4mError(PALDV)
        siting = "left" if tag in ("420mpeg2", "422") else "center"
    if siting not in SITINGS:
        raise Y4mError("unknown siting %r" % (siting,))
    flags = 0
    if siting in ("left", "topleft") and layout in (LAYOUTS["420"], LAYOUTS["422"]):
        flags |= COSITED_X
    if siting == "topleft" and layout == LAYOUTS["420"]:
        flags |= COSITED_Y
    return flags


def parse_size(text):
    """'WxH' -> (W, H)"""
    parts = text.lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts) or int(parts[0]) < 1 or int(parts[1]) < 1:
        raise Y4mError("--size wants WxH, two positive integers (got %r)" % (text,))
    return int(parts[0]), int(parts[1])


def auto_iterations(w, h, out_w, out_h):
    """the smallest k with (w << k) >= out_w and (h << k) >= out_h (W2XC_ITERATIONS_AUTO's rule); 5 where four steps do not reach"""
    k = 0
    while k < 5 and ((w << k) < out_w or (h << k) < out_h):
        k += 1
    return k


def output_plan(w, h, size, scale_ratio, has_noise, has_scale):
    """(iterations, (out_w, out_h) or None) of a stream of w x h frames: --size (a string) or --scale_ratio (a float), neither: the tool's old rule -- one 2x
    step with a scale model, none without -- and None, the base frame calls.  What the options cannot mean is a Y4mError"""
    if size is not None and scale_ratio is not None:
        raise Y4mError("--size and --scale_ratio exclude each other")
    if size is None and scale_ratio is None:
        return (1 if has_scale else 0), None
    if size is not None:
        out_w, out_h = parse_size(size)
        if out_w < w or out_h < h:
            raise Y4mError("--size %dx%d is smaller than the stream's %dx%d: the output is never smaller than the input" % (out_w, out_h, w, h))
        iterations = auto_iterations(w, h, out_w, out_h)
        if iterations > 4:
            raise Y4mError("--size %dx%d is more than 16 times the stream's %dx%d a side (four 2x steps at the most)" % (out_w, out_h, w, h))
    else:
        if not (scale_ratio >= 1.0) or scale_ratio > 16.0:
            raise Y4mError("--scale_ratio %g: 1 to 16 (the output is never smaller than the input, four 2x steps at the most)" % scale_ratio)
        iterations = int(math.ceil(math.log2(scale_ratio)))          # main.cpp:107-108
        out_w, out_h = int(w * scale_ratio), int(h * scale_ratio)    # :160-165
    if iterations and not has_scale:
        raise Y4mError("an output of %dx%d from %dx%d takes %d 2x step%s: that needs a scale model (-m scale or noise_scale)"
                       % (out_w, out_h, w, h, iterations, "" if iterations == 1 else "s"))
    if not iterations and not has_noise:
        raise Y4mError("an output of the input's size takes no 2x step: that needs a noise model (-m noise or noise_scale)")
    return iterations, (out_w, out_h)


def chroma_size(w, h, layout):
    if layout == LAYOUTS["mono"]:
        return 0, 0
    return ((w + 1) // 2 if layout != LAYOUTS["444"] else w), ((h + 1) // 2 if layout == LAYOUTS["420"] else h)


class Header:
    """the stream header: width, height, and every other field as (letter, value) in the order given"""

    def __init__(self, w, h, fields):
        self.w, self.h, self.fields = w, h, list(fields)

    def get(self, letter, default=None):
        for k, v in self.fields:
            if k == letter:
                return v
        return default

    @property
    def layout(self):
        return layout_of(self.get("C", "420jpeg"))

    @property
    def interlaced(self):
        return self.get("I", "p") not in ("p", "?")

    def colour_range(self):
        """'full' / 'limited' from an XCOLORRANGE field, None without one"""
        for k, v in self.fields:
            if k == "X" and v.upper().startswith("COLORRANGE="):
                r = v.split("=", 1)[1].lower()
                if r not in ("full", "limited"):
                    raise Y4mError("unknown XCOLORRANGE=%s" % v.split("=", 1)[1])
                return r
        return None

    def scaled(self, iterations):
        """the header of the output: W and H doubled `iterations` times, every other field -- F and A among them -- kept"""
        return Header(self.w << iterations, self.h << iterations, self.fields)

    def sized(self, out_w, out_h):
        """the header of a sized output: W and H as named, every other field kept"""
        return Header(out_w, out_h, self.fields)

    def line(self):
        return b" ".join([MAGIC, b"W%d" % self.w, b"H%d" % self.h] + [("%s%s" % kv).encode("ascii") for kv in self.fields]) + b"\n"


def read_line(f, limit=4096):
    line = bytearray()
    while True:
        b = f.read(1)
        if not b:
            return None if not line else bytes(line)
        if b == b"\n":
            return bytes(line)
        line += b
        if len(line) > limit:
            raise Y4mError("header line longer than %d bytes" % limit)


def read_header(f):
    line = read_line(f)
    if line is None or not line.startswith(MAGIC):
        raise Y4mError("not a YUV4MPEG2 stream")
    w = h = None
    fields = []
    for tok in line[len(MAGIC):].decode("ascii", "replace").split():
        k, v = tok[0], tok[1:]
        if k == "W":
            w = int(v)
        elif k == "H":
            h = int(v)
        else:
            fields.append((k, v))
    if not w or not h or w < 1 or h < 1:
        raise Y4mError("the header gives no frame size")
    return Header(w, h, fields)


def read_frames(f, hdr, count, layout=None, dtype=np.uint8):
    """up to `count` frames: (y, u, v) as (n, h, w) and (n, ch, cw) uint8 arrays (u = v = None for Cmono), n = 0 at the end of the stream.  layout / dtype: the
    chroma layout and the sample type where the caller reads the C tag itself (tools/w2xc_y4m16.py: little-endian 16-bit words)"""
    cw, ch = chroma_size(hdr.w, hdr.h, hdr.layout if layout is None else layout)
    ysz, csz = hdr.w * hdr.h, cw * ch
    unit = np.dtype(dtype).itemsize
    ys, us, vs = [], [], []
    while len(ys) < count:
        line = read_line(f)
        if line is None:
            break
        if not line.startswith(b"FRAME"):
            raise Y4mError("expected a FRAME header, got %r" % line[:16])
        data = f.read((ysz + 2 * csz) * unit)
        if len(data) != (ysz + 2 * csz) * unit:
            raise Y4mError("the stream ends inside a frame")
        a = np.frombuffer(data, dtype)
        ys.append(a[:ysz].reshape(hdr.h, hdr.w))
        if csz:
            us.append(a[ysz:ysz + csz].reshape(ch, cw))
            vs.append(a[ysz + csz:].reshape(ch, cw))
    if not ys:
        return np.empty((0, hdr.h, hdr.w), dtype), None, None
    return np.stack(ys), (np.stack(us) if csz else None), (np.stack(vs) if csz else None)


def write_header(f, hdr):
    f.write(hdr.line())


def write_frames(f, y, u, v):
    for i in range(y.shape[0]):
        f.write(b"FRAME\n")
        f.write(np.ascontiguousarray(y[i]).tobytes())
        if u is not None:
            f.write(np.ascontiguousarray(u[i]).tobytes())
            f.write(np.ascontiguousarray(v[i]).tobytes())


def default_matrix(h):
    """the matrix of a stream that does not say: BT.709 for 720 rows and more, BT.601 below"""
    return "bt709" if h >= 720 else "bt601"


def model_route(noise_planes, scale_planes):
    """'rgb' when the loaded models' first layers take three planes (w2xc_process_frames_yuv_u8_rgb: three-plane models, the upconv_7 schema), 'y' when they
    take one (w2xc_process_frames_yuv_u8); None = no such model.  Models of different kinds or of neither kind are a Y4mError."""
    loaded = [p for p in (noise_planes, scale_planes) if p is not None]
    for p in loaded:
        if p not in (1, 3):
            raise Y4mError("a model whose first layer takes %d planes: only Y models (1 plane) and RGB / upconv models (3 planes) are supported" % p)
    if len(set(loaded)) > 1:
        raise Y4mError("mixed model kinds: use a noise model and a scale model of the same kind")
    return "rgb" if loaded and loaded[0] == 3 else "y"


def check_route(route, layout):
    """what a route cannot take of a stream"""
    if route == "rgb" and layout == LAYOUTS["mono"]:
        raise Y4mError(MONO_RGB)


def build_parser(description="8-bit YUV4MPEG2 streams through waifu2x models on an MI355X: Y models (luma through the CNN, chroma 2x on bytes), or RGB and "
                             "upconv models by a colour matrix"):
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("-m", "--mode", default="noise_scale", choices=["noise", "scale", "noise_scale"])
    ap.add_argument("--noise_level", type=int, default=1, choices=[1, 2])
    ap.add_argument("--model_dir", default="models")
    ap.add_argument("--range", default="limited", choices=["full", "limited"], help="luma range where the stream has no XCOLORRANGE field")
    ap.add_argument("--matrix", default=None, choices=sorted(MATRICES),
                    help="colour matrix for RGB and upconv models (default: bt709 when H >= 720, else bt601); Y models use no matrix and ignore it")
    ap.add_argument("--frames_per_call", type=int, default=8)
    ap.add_argument("--siting", default="center", choices=list(SITINGS),
                    help="where a chroma sample sits: center (JPEG / MPEG-1), left (MPEG-2, H.264, HEVC), topleft (BT.2020 / UHD), or auto: by the C tag")
    ap.add_argument("--size", default=None, metavar="WxH", help="the output frame size: as many 2x steps as reach it, then a linear shrink (never below the input's size)")
    ap.add_argument("--scale_ratio", type=float, default=None, metavar="R",
                    help="the reference's rule: ceil(log2 R) 2x steps, output int(W * R) x int(H * R); R = 1 needs a noise model")
    return ap


def convert_stream(fin, fout, process, iterations, default_range="limited", frames_per_call=8, layout_of_header=None, dtype=np.uint8, size=None):
    """read fin, write fout; process(y, u, v, layout, full_range) -> (Y, U, V) is the frame call.  Returns the number of frames.  layout_of_header / dtype: how
    another tool reads the C tag, and its sample type.  size = (out_w, out_h): the W and H of the written header (default: doubled `iterations` times)"""
    hdr = read_header(fin)
    if hdr.interlaced:
        raise Y4mError(INTERLACED % hdr.get("I"))
    layout = hdr.layout if layout_of_header is None else layout_of_header(hdr)
    full = (hdr.colour_range() or default_range) == "full"
    write_header(fout, hdr.scaled(iterations) if size is None else hdr.sized(*size))
    total = 0
    while True:
        y, u, v = read_frames(fin, hdr, max(1, frames_per_call), layout, dtype)
        if y.shape[0] == 0:
            return total
        write_frames(fout, *process(y, u, v, layout, full))
        total += y.shape[0]


def run_tool(name, args, layout_of_header, make_process, dtype=np.uint8):
    """what both tools do with their parsed arguments: check the stream, load the models, route by their kind, convert.  make_process(w2xc, hdr, noise, scale,
    iterations, route, matrix, flags, size) -> the process callback of convert_stream; flags = the siting flags the frame call gets or-ed onto the layout,
    size = None (the base frame calls, as before) or (out_w, out_h) (--size / --scale_ratio: the _sized calls)"""
    try:
        with open(args.input, "rb") as fin:
            # what the stream itself rules out, before a model is loaded or the output file is created
            hdr = read_header(fin)
            if hdr.interlaced:
                raise Y4mError(INTERLACED % hdr.get("I"))
            layout, _ = layout_of_header(hdr), hdr.colour_range()
            flags = siting_flags(args.siting, hdr.get("C"), layout)
            iterations, size = output_plan(hdr.w, hdr.h, args.size, args.scale_ratio, args.mode in ("noise", "noise_scale"), args.mode in ("scale", "noise_scale"))
            fin.seek(0)
            import __graft_entry__ as graft
            w2xc = graft.load_package()
            noise = scale = None
            if args.mode in ("noise", "noise_scale"):
                noise = w2xc._ModelSet.from_json(os.path.join(args.model_dir, "noise%d_model.json" % args.noise_level))
            if args.mode in ("scale", "noise_scale"):
                scale = w2xc._ModelSet.from_json(os.path.join(args.model_dir, "scale2.0x_model.json"))
            route = model_route(noise.planes(0)[0] if noise else None, scale.planes(0)[0] if scale else None)
            check_route(route, layout)
            matrix = MATRICES[args.matrix or default_matrix(hdr.h)]
            process = make_process(w2xc, hdr, noise, scale if iterations else None, iterations, route, matrix, flags, size)
            with open(args.output, "wb") as fout:
                n = convert_stream(fin, fout, process, iterations, args.range, args.frames_per_call, layout_of_header, dtype, size)
    except Y4mError as e:
        sys.stderr.write("%s: %s\n" % (name, e))
        return 2
    sys.stderr.write("%s: %d frames\n" % (name, n))
    return 0


def main(argv=None):
    def make_process(w2xc, hdr, noise, scale, iterations, route, matrix, flags, size):
        def process(y, u, v, layout, full):
            rng = w2xc.RANGE_FULL if full else w2xc.RANGE_LIMITED
            if size is not None:
                kw = dict(chroma=layout | flags, noise=noise, scale=scale, iterations=iterations, range=rng)
                out = (w2xc.process_frames_yuv_u8_rgb_sized(y, size[0], size[1], u, v, matrix=matrix, **kw) if route == "rgb" else
                       w2xc.process_frames_yuv_u8_sized(y, size[0], size[1], u, v, **kw))
            elif route == "rgb":
                return w2xc.process_frames_yuv_u8_rgb(y, u, v, chroma=layout | flags, noise=noise, scale=scale, iterations=iterations, range=rng, matrix=matrix)
            else:
                out = w2xc.process_frames_yuv_u8(y, u, v, chroma=layout | flags, noise=noise, scale=scale, iterations=iterations, range=rng)
            return out if len(out) == 3 else (out[0], None, None)
        return process
    return run_tool("w2xc_y4m", build_parser().parse_args(argv), lambda hdr: hdr.layout, make_process)


if __name__ == "__main__":
    sys.exit(main())
