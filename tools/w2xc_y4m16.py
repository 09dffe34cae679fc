#!/usr/bin/env python3
"""tools/w2xc_y4m16.py in.y4m out.y4m -m noise|scale|noise_scale --model_dir DIR [--noise_level N] [--range full|limited] [--matrix bt601|bt709|bt2020]
                       [--frames_per_call N] [--siting center|left|topleft|auto] [--size WxH | --scale_ratio R]

A YUV4MPEG2 stream of 9- to 16-bit samples through the 16-bit YUV frame calls (include/w2xc_hip.h, "16-bit YUV frames"): colour spaces C420pD, C422pD and
C444pD with D in 9, 10, 12, 14, 16, and CmonoD.  Samples are little-endian 16-bit words with the value in the low bits (W2XC_PACK_LOW), as the format has them.
The header, line and stream code, the options and the routing by the loaded models are those of tools/w2xc_y4m.py: Y models go through
w2xc_process_frames_yuv_u16, models whose first layer takes three planes through w2xc_process_frames_yuv_u16_rgb by --matrix.  8-bit streams belong to
tools/w2xc_y4m.py and are refused here.  --siting is that tool's: center (the default), left, topleft, or auto -- the CxxxpD tags name no siting, so auto is
center here.  --size and --scale_ratio are that tool's too ("Sized YUV frames": the _sized forms of the 16-bit calls).
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import w2xc_y4m as y4m   # noqa: E402

Y4mError = y4m.Y4mError
DEPTHS = (9, 10, 12, 14, 16)
WORD = np.dtype("<u2")


def format_of(tag):
    """(chroma layout, depth) of a C tag's value: 420pD / 422pD / 444pD / monoD; 8-bit tags and everything else are refused"""
    m = re.fullmatch(r"(420|422|444)p(\d+)|mono(\d+)", tag or "")
    if not m:
        raise Y4mError("unsupported colour space C%s (C420pD, C422pD, C444pD and CmonoD with D in 9, 10, 12, 14, 16 only; 8-bit streams: tools/w2xc_y4m.py)" % tag)
    depth = int(m.group(2) or m.group(3))
    if depth not in DEPTHS:
        raise Y4mError("unsupported sample depth %d in C%s (9, 10, 12, 14 or 16 bits)" % (depth, tag))
    return y4m.LAYOUTS[m.group(1) or "mono"], depth


def header_format(hdr):
    return format_of(hdr.get("C", "420jpeg"))


def header_layout(hdr):
    return header_format(hdr)[0]


def read_frames(f, hdr, count):
    """up to `count` frames: (y, u, v) as (n, h, w) and (n, ch, cw) uint16 arrays of low-packed values (u = v = None for CmonoD)"""
    return y4m.read_frames(f, hdr, count, header_layout(hdr), WORD)


def write_frames(f, y, u, v):
    le = lambda a: None if a is None else np.asarray(a).astype(WORD, copy=False)
    y4m.write_frames(f, le(y), le(u), le(v))


def convert_stream(fin, fout, process, iterations, default_range="limited", frames_per_call=8, size=None):
    """tools/w2xc_y4m.py's convert_stream on words; process(y, u, v, layout, full_range) gets uint16 arrays"""
    def words_out(y, u, v, layout, full):
        Y, U, V = process(y, u, v, layout, full)
        conv = lambda a: None if a is None else np.asarray(a).astype(WORD, copy=False)
        return conv(Y), conv(U), conv(V)
    return y4m.convert_stream(fin, fout, words_out, iterations, default_range, frames_per_call, header_layout, WORD, size)


def main(argv=None):
    def make_process(w2xc, hdr, noise, scale, iterations, route, matrix, flags, size):
        depth = header_format(hdr)[1]

        def process(y, u, v, layout, full):
            rng = w2xc.RANGE_FULL if full else w2xc.RANGE_LIMITED
            kw = dict(chroma=layout | flags, noise=noise, scale=scale, iterations=iterations, range=rng, depth=depth, pack=w2xc.PACK_LOW)
            y, u, v = (None if a is None else a.astype(np.uint16, copy=False) for a in (y, u, v))
            if size is not None:
                out = (w2xc.process_frames_yuv_u16_rgb_sized(y, size[0], size[1], u, v, matrix=matrix, **kw) if route == "rgb" else
                       w2xc.process_frames_yuv_u16_sized(y, size[0], size[1], u, v, **kw))
            elif route == "rgb":
                return w2xc.process_frames_yuv_u16_rgb(y, u, v, matrix=matrix, **kw)
            else:
                out = w2xc.process_frames_yuv_u16(y, u, v, **kw)
            return out if len(out) == 3 else (out[0], None, None)
        return process
    ap = y4m.build_parser("9- to 16-bit YUV4MPEG2 streams (C420pD, C422pD, C444pD, CmonoD) through waifu2x models on an MI355X: Y models (luma through the "
                          "CNN, chroma 2x on words), or RGB and upconv models by a colour matrix")
    return y4m.run_tool("w2xc_y4m16", ap.parse_args(argv), header_layout, make_process, WORD)


if __name__ == "__main__":
    sys.exit(main())
