"""NumPy restatement of "YUV frames through RGB models" (include/w2xc_hip.h): the constants of a colour matrix, chroma at luma resolution, bytes -> R, G, B
planes and planes -> bytes -- every operation in float32, one rounding each, one operation per line, in the order the header gives.  And the grid rule of the
two kernels' launchers (w2xc_launch_yuv8_to_rgb / w2xc_launch_rgb_to_yuv8, csrc/w2xc_yuv_rgb.hip), as tests/yuv_ref.py mirrors the chroma kernel's."""
import numpy as np

from yuv_ref import F32, FULL, LIMITED, YUV_420, YUV_422, YUV_444, chroma_size, luma_in, sat_u8

BT601, BT709, BT2020 = 0, 1, 2
MATRICES = (BT601, BT709, BT2020)
LAYOUTS = (YUV_420, YUV_422, YUV_444)
WEIGHTS = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722), BT2020: (0.2627, 0.0593)}


def constants64(matrix):
    """the header's expressions, in double"""
    Kr, Kb = WEIGHTS[matrix]
    Kg = 1.0 - Kr - Kb
    cRV = 2.0 * (1.0 - Kr)
    cBU = 2.0 * (1.0 - Kb)
    cGV = Kr * cRV / Kg
    cGU = Kb * cBU / Kg
    iRV = 1.0 / cRV
    iBU = 1.0 / cBU
    return dict(Kr=Kr, Kg=Kg, Kb=Kb, cRV=cRV, cBU=cBU, cGV=cGV, cGU=cGU, iRV=iRV, iBU=iBU)


def constants(matrix):
    """... each rounded once to float"""
    return {k: F32(v) for k, v in constants64(matrix).items()}


def _up_axis(C, axis, n_out):
    """0.75 C[j] + 0.25 C[j'] along `axis` for the luma indices 0 .. n_out - 1: j = x >> 1, j' = j + 1 for odd x, j - 1 for even x, clamped into the plane"""
    n = C.shape[axis]
    x = np.arange(n_out)
    j = x >> 1
    jj = np.clip(np.where(x & 1, j + 1, j - 1), 0, n - 1)
    near = np.take(C, j, axis=axis)
    far = np.take(C, jj, axis=axis)
    a = F32(0.75) * near
    b = F32(0.25) * far
    return a + b


def chroma_at_luma(C, w, h, layout):
    """a chroma plane of bytes -> float32 values at the w x h luma samples: horizontally first, then vertically on the row results"""
    c = np.asarray(C, np.uint8).astype(F32)
    if layout != YUV_444:
        c = _up_axis(c, 1, w)
    if layout == YUV_420:
        c = _up_axis(c, 0, h)
    assert c.shape == (h, w) and c.dtype == F32
    return c


def yuv8_to_rgb(Y, U, V, layout, rng, matrix):
    """one frame: (h, w) luma bytes and (ch, cw) chroma bytes -> (3, h, w) float32 R, G, B in [0, 1]"""
    k = constants(matrix)
    h, w = Y.shape
    assert U.shape == V.shape == chroma_size(w, h, layout)[::-1]
    y = luma_in(Y, rng)
    kc = F32(1.0 / 224.0) if rng == LIMITED else F32(1.0 / 255.0)
    cb = chroma_at_luma(U, w, h, layout) - F32(128.0)
    cb = cb * kc
    cr = chroma_at_luma(V, w, h, layout) - F32(128.0)
    cr = cr * kc
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


def _block_mean(c, layout):
    """the box mean of chroma over a luma block, the block's last column / row replicated at an odd edge"""
    h, w = c.shape
    if layout == YUV_444:
        return c
    if w & 1:
        c = np.concatenate([c, c[:, -1:]], axis=1)
    if layout == YUV_422:
        s = c[:, 0::2] + c[:, 1::2]
        return s * F32(0.5)
    if h & 1:
        c = np.concatenate([c, c[-1:, :]], axis=0)
    top = c[0::2, 0::2] + c[0::2, 1::2]
    bot = c[1::2, 0::2] + c[1::2, 1::2]
    s = top + bot
    return s * F32(0.25)


def rgb_to_yuv8(rgb, layout, rng, matrix):
    """(3, H, W) float32 planes, unclipped -> (Y, U, V) bytes of one frame"""
    k = constants(matrix)
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
        if rng == LIMITED:
            Y = y * F32(219.0)
            Y = sat_u8(Y + F32(16.0))
        else:
            Y = sat_u8(y * F32(255.0))
        cs = F32(224.0) if rng == LIMITED else F32(255.0)
        out = []
        for ch in (cb, cr):
            m = _block_mean(ch, layout)
            m = m * cs
            out.append(sat_u8(m + F32(128.0)))
    assert y.dtype == F32 and cb.dtype == F32
    return Y, out[0], out[1]


# ---- the launch of both kernels: tiles of TCX x TCY chroma samples of one frame, at most GRID_MAX workgroups ----
TCX, TCY, GRID_MAX = 32, 16, 2048


def launch(w, h, layout, n):
    """(tile turns, workgroups) of w2xc_launch_yuv8_to_rgb / w2xc_launch_rgb_to_yuv8 for n frames of w x h"""
    cw, ch = chroma_size(w, h, layout)
    turns = ((cw + TCX - 1) // TCX) * ((ch + TCY - 1) // TCY) * n
    return turns, min(turns, GRID_MAX)


# the narrow, tall frame of the GPU tests' "second trip": more tiles than workgroups, a few tens of MB of float planes
SECOND_TRIP = dict(w=131, h=22081, layout=YUV_420, n=1)   # 3 x 691 tiles
