"""NumPy restatement of "16-bit YUV frames" (include/w2xc_hip.h): the two packings of a value in a 16-bit word, the luma ends, the chroma rule of the Y route
and the two ends of the RGB route for a depth D of 8 .. 16 bits -- every operation in float32, one rounding each, one operation per line, in the order the header
gives; every constant computed in double and rounded once.  Built on tests/yuv_ref.py and tests/yuv_rgb_ref.py: the cubic, chroma at luma resolution, the
matrix constants and the box mean are theirs.  And the grid rules of the new launchers (csrc/w2xc_yuv16.hip, csrc/w2xc_yuv16_rgb.hip)."""
import numpy as np

import yuv_ref as yr
import yuv_rgb_ref as rr
from yuv_ref import F32, FULL, LIMITED, YUV_420, YUV_422, YUV_444, YUV_400, chroma_size, out_chroma_size   # noqa: F401

LOW, HIGH = 0, 1
DEPTHS = tuple(range(8, 17))


def maxval(depth):
    return (1 << depth) - 1


def step(depth):
    """s = 2^(D - 8)"""
    return 1 << (depth - 8)


# ---- words <-> values ----
def unpack(words, depth, pack):
    w = np.asarray(words, np.uint16).astype(np.uint32)
    return (w >> (16 - depth)) if pack == HIGH else (w & maxval(depth))


def pack_words(values, depth, pack):
    v = np.asarray(values).astype(np.uint32)
    assert v.size == 0 or int(v.max()) <= maxval(depth)
    return (v << (16 - depth) if pack == HIGH else v).astype(np.uint16)


def sat(r, depth):
    """clamp(rint(r), 0, M): numpy's rint is half to even; the clip comes first, so values past int32 saturate"""
    return np.clip(np.rint(r), 0, maxval(depth)).astype(np.uint16)


# ---- luma ----
def luma_in(Y, rng, depth):
    """values (not words) -> float32"""
    y = np.asarray(Y).astype(F32)
    if rng == LIMITED:
        y = y - F32(16.0 * step(depth))
        return y * F32(1.0 / (219.0 * step(depth)))
    return y * F32(1.0 / maxval(depth))


def luma_out(y, rng, depth):
    y = np.asarray(y, F32)
    if rng == LIMITED:
        r = y * F32(219.0 * step(depth))
        return sat(r + F32(16.0 * step(depth)), depth)
    return sat(y * F32(float(maxval(depth))), depth)


# ---- chroma of the Y route ----
def chroma2x(C, depth, ow=None, oh=None):
    """chroma values cw x ch -> the leading ow x oh values of the 2x enlargement"""
    C = np.asarray(C)
    ch, cw = C.shape
    c = C.astype(F32) * F32(1.0 / maxval(depth))
    out = sat(yr.resize2x_cubic(c) * F32(float(maxval(depth))), depth)
    return np.ascontiguousarray(out[:(2 * ch if oh is None else oh), :(2 * cw if ow is None else ow)])


# ---- the RGB route ----
def chroma_scale(rng, depth):
    """(k in, scale out, offset) of the chroma of the RGB route"""
    if rng == LIMITED:
        return F32(1.0 / (224.0 * step(depth))), F32(224.0 * step(depth)), F32(128.0 * step(depth))
    return F32(1.0 / maxval(depth)), F32(float(maxval(depth))), F32(128.0 * step(depth))


def chroma_at_luma(C, w, h, layout):
    c = np.asarray(C).astype(F32)
    if layout != YUV_444:
        c = rr._up_axis(c, 1, w)
    if layout == YUV_420:
        c = rr._up_axis(c, 0, h)
    assert c.shape == (h, w) and c.dtype == F32
    return c


def chroma_in(c, rng, depth):
    """(c - 128 s) * k on float32 values"""
    k, _, mid = chroma_scale(rng, depth)
    c = np.asarray(c, F32) - mid
    return c * k


def chroma_out(c, rng, depth):
    """clamp(rint(c * scale + 128 s), 0, M)"""
    _, scale, mid = chroma_scale(rng, depth)
    m = np.asarray(c, F32) * scale
    return sat(m + mid, depth)


def yuv16_to_rgb(Y, U, V, layout, rng, matrix, depth):
    """one frame of values: (h, w) luma and (ch, cw) chroma -> (3, h, w) float32 R, G, B in [0, 1]"""
    k = rr.constants(matrix)
    h, w = Y.shape
    assert U.shape == V.shape == chroma_size(w, h, layout)[::-1]
    y = luma_in(Y, rng, depth)
    cb = chroma_in(chroma_at_luma(U, w, h, layout), rng, depth)
    cr = chroma_in(chroma_at_luma(V, w, h, layout), rng, depth)
    t = k["cRV"] * cr
    R = y + t
    t = k["cBU"] * cb
    B = y + t
    t = k["cGU"] * cb
    G = y - t
    t = k["cGV"] * cr
    G = G - t
    out = np.stack([R, G, B])
    assert out.dtype == F32
    return np.clip(out, F32(0.0), F32(1.0))


def rgb_to_yuv16(rgb, layout, rng, matrix, depth):
    """(3, H, W) float32 planes, unclipped -> (Y, U, V) values of one frame"""
    k = rr.constants(matrix)
    R, G, B = (np.asarray(p, F32) for p in rgb)
    with np.errstate(over="ignore", invalid="ignore"):
        a = k["Kr"] * R
        b = k["Kg"] * G
        c = k["Kb"] * B
        y = a + b
        y = y + c
        cb = B - y
        cb = cb * k["iBU"]
        cr = R - y
        cr = cr * k["iRV"]
        Y = luma_out(y, rng, depth)
        out = [chroma_out(rr._block_mean(c_, layout), rng, depth) for c_ in (cb, cr)]
    assert y.dtype == F32 and cb.dtype == F32
    return Y, out[0], out[1]


# ---- the launches ----
TQX, TQY, GRID_MAX = yr.TQX, yr.TQY, yr.GRID_MAX


def chroma_launch(ow, oh, frames):
    """(tile turns, workgroups) of w2xc_launch_chroma2x_u16: a turn is one tile of ALL planes (U, or U and V) of one frame, quads 0 .. ow // 2 by 0 .. oh // 2"""
    turns = ((ow // 2 + TQX) // TQX) * ((oh // 2 + TQY) // TQY) * frames
    return turns, min(turns, GRID_MAX)


def chroma_load_path(planar, aligned_bytes, v_follows_u):
    """the load path w2xc_launch_chroma2x_u16 and w2xc_launch_yuv16_to_rgb take for chroma: 1 = four samples per 8-byte load (planar planes, every row on an
    8-byte boundary), 2 = a (U, V) pair per 4-byte load (interleaved, v = u + 1 sample, every row on a 4-byte boundary), 0 = sample by sample"""
    if planar:
        return 1 if aligned_bytes % 8 == 0 else 0
    return 2 if v_follows_u and aligned_bytes % 4 == 0 else 0


launch = rr.launch    # w2xc_launch_yuv16_to_rgb / w2xc_launch_rgb_to_yuv16: the tiles of the 8-bit launchers

# more tile turns than workgroups, in few samples: one column of tiles
CHROMA_SECOND_TRIP = dict(cw=17, ch=16 * 2048 + 1, n=1)            # quads 0 .. 17 x 0 .. 32770: 1 x 2049 tiles
RGB_SECOND_TRIP = dict(w=33, h=16 * 1024 + 1, layout=YUV_444, n=1)   # 2 x 1025 tiles of 32 x 16 samples
