"""NumPy restatement of "Sized YUV frames" (include/w2xc_hip.h): chroma from the input plane to the output plane in ONE step, at any luma ratio r <= 1 per axis --
coordinates in float64 (three operations: the sum, the product, the difference), everything behind them in float32, one operation per line, in the order the
header gives.  Built on tests/yuv_ref.py (the cubic's coefficients), tests/yuv16_ref.py (the scale of a depth and the rounding) and tests/yuv_sited_ref.py (the
flag bits and the split of a `chroma` value): nothing of theirs is copied.  And the rules a sized call adds: the output range, ITERATIONS_AUTO, the grid."""
import numpy as np

import yuv_ref as yr
import yuv16_ref as y16
import yuv_sited_ref as sr
from yuv_ref import F32, YUV_420, YUV_422, YUV_444, YUV_400   # noqa: F401

F64 = np.float64
ITERATIONS_AUTO = -1
TX, TY, GRID_MAX = 32, 16, 2048          # a tile of OUTPUT samples; the cap of the grid-stride loop


def auto_iterations(w, h, out_w, out_h):
    """the smallest k with (w << k) >= out_w and (h << k) >= out_h; 5 where four steps do not reach"""
    k = 0
    while k < 5 and ((w << k) < out_w or (h << k) < out_h):
        k += 1
    return k


def size_ok(w, h, out_w, out_h, iterations):
    """the output range of a sized call whose iterations are resolved"""
    return 0 <= iterations <= 4 and w <= out_w <= w << iterations and h <= out_h <= h << iterations


def subsampling(chroma):
    """(sub_x, sub_y) of a layout, flags or not"""
    layout = chroma & 0xF
    return int(layout in (YUV_420, YUV_422)), int(layout == YUV_420)


def offset(subsampled, cosited):
    """o: 0.25 on a co-sited axis, 0.5 on a centred or unsubsampled one"""
    return 0.25 if subsampled and cosited else 0.5


def positions(n_out, luma_in, luma_out, o):
    """per output sample of an axis: (s, t) -- the floor of its source coordinate (int64) and the fraction as float32"""
    r = F64(luma_in) / F64(luma_out)
    m = np.arange(n_out).astype(F64)
    pos = m + F64(o)
    pos = pos * r
    pos = pos - F64(o)
    s = np.floor(pos)
    t = pos - s
    return s.astype(np.int64), t.astype(F32)


def _axis(n_in, n_out, luma_in, luma_out, o):
    """the four clamped taps and the four coefficients of every output sample of an axis"""
    s, t = positions(n_out, luma_in, luma_out, o)
    c = yr.cubic_coeffs(t)
    taps = [np.clip(s - 1 + k, 0, n_in - 1) for k in range(4)]
    return taps, c


def resize_cubic(x, ow, oh, w, h, out_w, out_h, ox, oy):
    """a float32 plane -> ow x oh: the horizontal pass of every source row, then the vertical pass, each sum from tap 0 to tap 3"""
    x = np.asarray(x, F32)
    ch, cw = x.shape
    xs, kx = _axis(cw, ow, w, out_w, ox)
    rows = x[:, xs[0]] * kx[0]
    for k in (1, 2, 3):
        rows = rows + x[:, xs[k]] * kx[k]
    ys, ky = _axis(ch, oh, h, out_h, oy)
    out = rows[ys[0]] * ky[0][:, None]
    for k in (1, 2, 3):
        out = out + rows[ys[k]] * ky[k][:, None]
    assert out.dtype == F32
    return out


def chroma_resize(C, ow, oh, w, h, out_w, out_h, sub_x=1, sub_y=1, cosited=0, depth=8):
    """chroma values cw x ch -> ow x oh values (uint8 for a uint8 plane at depth 8, else uint16): the block w2xc_chroma_resize_u8_device / _u16_device"""
    C = np.asarray(C)
    M = y16.maxval(depth)
    c = C.astype(F32) * F32(1.0 / M)
    up = resize_cubic(c, ow, oh, w, h, out_w, out_h, offset(sub_x, cosited & sr.COSITED_X), offset(sub_y, cosited & sr.COSITED_Y))
    out = y16.sat(up * F32(float(M)), depth)
    return np.ascontiguousarray(out.astype(np.uint8) if depth == 8 and C.dtype == np.uint8 else out)


def frame_chroma(C, w, h, out_w, out_h, chroma, depth=8):
    """one chroma plane of a w x h frame -> that of the out_w x out_h frame, `chroma` the interface's value (layout | siting flags)"""
    ocw, och = sr.chroma_size(out_w, out_h, chroma)
    sx, sy = subsampling(chroma)
    return chroma_resize(C, ocw, och, w, h, out_w, out_h, sx, sy, chroma & 0x30, depth)


def launch(ow, oh, per_tile):
    """(turns, workgroups) of the resize launchers: per_tile = frames x planes on bytes, frames on words"""
    turns = ((ow + TX - 1) // TX) * ((oh + TY - 1) // TY) * per_tile
    return turns, min(turns, GRID_MAX)


# the GPU tests' second trip of the grid-stride loop: a thin tall plane of 1 x 2049 tiles for 2048 workgroups
SECOND_TRIP = dict(ow=17, oh=16 * 2048 + 1, n=1)
