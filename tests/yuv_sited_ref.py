"""NumPy restatement of "Chroma siting" (include/w2xc_hip.h): the bicubic 2x of chroma, chroma at luma resolution and chroma from R, G, B for chroma that is
co-sited with luma along x and / or y -- every operation in float32, one rounding each, one operation per line, in the order the header gives.  Built on
tests/yuv_ref.py, tests/yuv_rgb_ref.py and tests/yuv16_ref.py: the cubic's coefficients, the centred axes, the matrix constants, the scales and the roundings are
theirs.  A `chroma` value here is the interface's: a layout with the flags or-ed on.  The two ends of the RGB route are written once, for a depth (8: the calls
on bytes, whose constants the 16-bit expressions give at D = 8)."""
import numpy as np

import yuv_ref as yr
import yuv_rgb_ref as rr
import yuv16_ref as y16
from yuv_ref import F32, YUV_420, YUV_422, YUV_444, YUV_400

COSITED_X, COSITED_Y = 0x10, 0x20
YUV_420_LEFT, YUV_420_TOPLEFT, YUV_422_LEFT = YUV_420 | COSITED_X, YUV_420 | COSITED_X | COSITED_Y, YUV_422 | COSITED_X
SITED_LAYOUTS = (YUV_420_LEFT, YUV_420_TOPLEFT, YUV_422_LEFT)
SITED_IDS = {YUV_420_LEFT: "420left", YUV_420_TOPLEFT: "420topleft", YUV_422_LEFT: "422left", YUV_420 | COSITED_Y: "420top"}
ALL_SITED = SITED_LAYOUTS + (YUV_420 | COSITED_Y,)      # every flagged value the interface accepts


def split(chroma):
    """(layout, co-sited x, co-sited y)"""
    return chroma & 0xF, bool(chroma & COSITED_X), bool(chroma & COSITED_Y)


def accepted(chroma):
    """the interface's rule: only the two flag bits on a layout 0 .. 3, and a flag only on an axis the layout subsamples"""
    if chroma < 0 or chroma & ~0x3F or (chroma & 0xF) > YUV_400:
        return False
    layout, cx, cy = split(chroma)
    return (not cx or layout in (YUV_420, YUV_422)) and (not cy or layout == YUV_420)


def chroma_size(w, h, chroma):
    return yr.chroma_size(w, h, chroma & 0xF)


# ---- Y route: the bicubic 2x ----
def _axis(n, cosited):
    """per output index of a 2x axis over n source samples: the four clamped taps and the four coefficients"""
    if not cosited:
        return yr._axis(n)
    m = np.arange(2 * n)
    f = m.astype(F32) * F32(0.5)
    f = f - F32(0.125)
    s = np.floor(f)
    t = f - s                                    # 0.375 for odd m, 0.875 for even m, exactly
    s = s.astype(np.int64)
    c = yr.cubic_coeffs(t)
    taps = [np.clip(s - 1 + k, 0, n - 1) for k in range(4)]
    return taps, c


def resize2x_cubic(x, cx, cy):
    """yr.resize2x_cubic with the co-sited axes' positions: the horizontal pass of every source row, then the vertical pass, each sum from tap 0 to tap 3"""
    x = np.asarray(x, F32)
    h, w = x.shape
    xs, kx = _axis(w, cx)
    rows = x[:, xs[0]] * kx[0]
    for k in (1, 2, 3):
        rows = rows + x[:, xs[k]] * kx[k]
    ys, ky = _axis(h, cy)
    out = rows[ys[0]] * ky[0][:, None]
    for k in (1, 2, 3):
        out = out + rows[ys[k]] * ky[k][:, None]
    assert out.dtype == F32
    return out


def chroma2x(C, cosited, depth=8, ow=None, oh=None):
    """chroma values cw x ch -> the leading ow x oh values of the 2x enlargement; cosited = the flag bits"""
    C = np.asarray(C)
    ch, cw = C.shape
    M = y16.maxval(depth)
    c = C.astype(F32) * F32(1.0 / M)
    up = resize2x_cubic(c, bool(cosited & COSITED_X), bool(cosited & COSITED_Y))
    out = y16.sat(up * F32(float(M)), depth)
    out = out.astype(np.uint8) if depth == 8 and C.dtype == np.uint8 else out
    return np.ascontiguousarray(out[:(2 * ch if oh is None else oh), :(2 * cw if ow is None else ow)])


# ---- RGB route, in: chroma at luma resolution ----
def _up_axis(C, axis, n_out, cosited):
    if not cosited:
        return rr._up_axis(C, axis, n_out)
    n = C.shape[axis]
    x = np.arange(n_out)
    j = x >> 1
    jn = np.minimum(j + 1, n - 1)
    here = np.take(C, j, axis=axis)
    a = F32(0.5) * here
    b = F32(0.5) * np.take(C, jn, axis=axis)
    mid = a + b
    odd = (x & 1).astype(bool).reshape([-1 if k == axis else 1 for k in range(C.ndim)])
    return np.where(odd, mid, here)


def chroma_at_luma(C, w, h, chroma):
    """a chroma plane of values -> float32 values at the w x h luma samples: horizontally first, then vertically on the row results"""
    layout, cx, cy = split(chroma)
    c = np.asarray(C).astype(F32)
    if layout != YUV_444:
        c = _up_axis(c, 1, w, cx)
    if layout == YUV_420:
        c = _up_axis(c, 0, h, cy)
    assert c.shape == (h, w) and c.dtype == F32
    return c


# ---- RGB route, out: chroma from cb, cr at luma resolution ----
def _down_axis(c, axis, cosited):
    """a subsampled axis: co-sited, (l + r) * 0.25 + m * 0.5 around luma 2k with the neighbours clamped; centred, (a + b) * 0.5 of the block, the last sample
    replicated at an odd edge"""
    n = c.shape[axis]
    k = np.arange((n + 1) // 2)
    if cosited:
        l = np.take(c, np.maximum(2 * k - 1, 0), axis=axis)
        m = np.take(c, 2 * k, axis=axis)
        r = np.take(c, np.minimum(2 * k + 1, n - 1), axis=axis)
        s = l + r
        s = s * F32(0.25)
        m = m * F32(0.5)
        return s + m
    a = np.take(c, 2 * k, axis=axis)
    b = np.take(c, np.minimum(2 * k + 1, n - 1), axis=axis)
    s = a + b
    return s * F32(0.5)


def chroma_down(c, chroma):
    """cb or cr at luma resolution -> the chroma plane: both axes centred is the box mean of rr._block_mean; otherwise horizontally first, then vertically"""
    layout, cx, cy = split(chroma)
    c = np.asarray(c, F32)
    if not cx and not cy:
        return rr._block_mean(c, layout)
    c = _down_axis(c, 1, cx)
    if layout == YUV_420:
        c = _down_axis(c, 0, cy)
    assert c.dtype == F32
    return c


# ---- the two ends, for a depth ----
def yuv_to_rgb(Y, U, V, chroma, rng, matrix, depth=8):
    """one frame of values: (h, w) luma and (ch, cw) chroma -> (3, h, w) float32 R, G, B in [0, 1]"""
    k = rr.constants(matrix)
    h, w = Y.shape
    assert U.shape == V.shape == chroma_size(w, h, chroma)[::-1]
    y = y16.luma_in(Y, rng, depth)
    cb = y16.chroma_in(chroma_at_luma(U, w, h, chroma), rng, depth)
    cr = y16.chroma_in(chroma_at_luma(V, w, h, chroma), rng, depth)
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


def rgb_to_yuv(rgb, chroma, rng, matrix, depth=8):
    """(3, H, W) float32 planes, unclipped -> (Y, U, V) values of one frame (uint16; at depth 8 they fit bytes)"""
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
        Y = y16.luma_out(y, rng, depth)
        out = [y16.chroma_out(chroma_down(c_, chroma), rng, depth) for c_ in (cb, cr)]
    assert y.dtype == F32 and cb.dtype == F32
    return Y, out[0], out[1]


# ---- the GPU tests' "second trip" of the RGB route on a subsampled layout: 2 x 1025 tiles of 32 x 16 chroma samples for 2048 workgroups ----
RGB_SECOND_TRIP = dict(w=66, h=2 * (16 * 1024 + 1), n=1)
