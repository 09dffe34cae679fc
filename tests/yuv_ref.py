"""NumPy restatement of the YUV frame arithmetic of include/w2xc_hip.h ("YUV frames"): the two luma ends, the chroma sizes and the chroma rule -- every
operation in float32, one rounding each, in the order the header gives.  tests/test_yuv_api.py holds it against the oracle's cubic primitive where
tests/test_oracle_color.py pins that; the GPU tests use it beside their composed routes.  And the grid rule of the chroma kernel's launcher
(w2xc_launch_chroma2x_u8, csrc/w2xc_yuv.hip), as tests/fp32_matrix.py mirrors the convolution launchers'."""
import numpy as np

F32 = np.float32
YUV_420, YUV_422, YUV_444, YUV_400 = 0, 1, 2, 3
LAYOUTS = (YUV_420, YUV_422, YUV_444, YUV_400)
FULL, LIMITED = 0, 1


def chroma_size(w, h, layout):
    """(cw, ch) of a w x h frame"""
    if layout == YUV_400:
        return 0, 0
    return (w if layout == YUV_444 else (w + 1) // 2), ((h + 1) // 2 if layout == YUV_420 else h)


def out_chroma_size(w, h, layout):
    """the chroma size of the 2w x 2h frame: the leading part of the 2cw x 2ch enlargement that is kept"""
    return chroma_size(2 * w, 2 * h, layout)


def luma_in(Y, rng):
    y = np.asarray(Y, np.uint8).astype(F32)
    return (y - F32(16.0)) * F32(1.0 / 219.0) if rng == LIMITED else y * F32(1.0 / 255.0)


def sat_u8(r):
    """saturate(rint(r)): numpy's rint is half to even; the clip comes first, so values past int32 saturate"""
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def luma_out(y, rng):
    y = np.asarray(y, F32)
    return sat_u8(y * F32(219.0) + F32(16.0)) if rng == LIMITED else sat_u8(y * F32(255.0))


def cubic_coeffs(t):
    """Keys' cubic, A = -0.75, the expressions of cubic_coeffs (csrc/w2xc_px.h) on float32 arrays"""
    t = np.asarray(t, F32)
    A, one = F32(-0.75), F32(1.0)
    c0 = ((A * (t + one) - F32(5) * A) * (t + one) + F32(8) * A) * (t + one) - F32(4) * A
    c1 = ((A + F32(2)) * t - (A + F32(3))) * t * t + one
    c2 = ((A + F32(2)) * (one - t) - (A + F32(3))) * (one - t) * (one - t) + one
    c3 = one - c0 - c1 - c2
    return [c0, c1, c2, c3]


def _axis(n):
    """per output index of a 2x axis over n source samples: the four clamped taps and the four coefficients"""
    d = np.arange(2 * n)
    f = ((d + 0.5) * 0.5 - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    c = cubic_coeffs(f - s.astype(F32))
    taps = [np.clip(s - 1 + k, 0, n - 1) for k in range(4)]
    return taps, c


def resize2x_cubic(x):
    """Resize2xCubic: the horizontal pass of every source row, then the vertical pass, each sum from tap 0 to tap 3"""
    x = np.asarray(x, F32)
    h, w = x.shape
    xs, cx = _axis(w)
    rows = x[:, xs[0]] * cx[0]
    for k in (1, 2, 3):
        rows = rows + x[:, xs[k]] * cx[k]
    ys, cy = _axis(h)
    out = rows[ys[0]] * cy[0][:, None]
    for k in (1, 2, 3):
        out = out + rows[ys[k]] * cy[k][:, None]
    return out


def chroma2x(C, ow=None, oh=None):
    """chroma bytes cw x ch -> the leading ow x oh bytes of the 2x enlargement"""
    C = np.asarray(C, np.uint8)
    ch, cw = C.shape
    out = sat_u8(resize2x_cubic(C.astype(F32) * F32(1.0 / 255.0)) * F32(255.0))
    return np.ascontiguousarray(out[:(2 * ch if oh is None else oh), :(2 * cw if ow is None else ow)])


# ---- the chroma kernel's launch: tiles of TQX x TQY quads (a quad = 2 x 2 outputs), at most GRID_MAX workgroups ----
TQX, TQY, GRID_MAX = 32, 16, 2048


def chroma_launch(ow, oh, planes):
    """(tile turns, workgroups) of w2xc_launch_chroma2x_u8 for `planes` planes of ow x oh outputs: quads 0 .. ow // 2 by 0 .. oh // 2"""
    turns = ((ow // 2 + TQX) // TQX) * ((oh // 2 + TQY) // TQY) * planes
    return turns, min(turns, GRID_MAX)


# ---- YUV4MPEG2 streams for the tool's tests ----
def y4m_stream(w, h, tag, n, seed, extra=b"F30000:1001 Ip A1:1"):
    """(bytes, [(y, u, v)]) of a generated stream; tag = the C field's value or None for none"""
    layout = {None: YUV_420, "420": YUV_420, "420jpeg": YUV_420, "420mpeg2": YUV_420, "420paldv": YUV_420, "422": YUV_422, "444": YUV_444, "mono": YUV_400}[tag]
    cw, ch = chroma_size(w, h, layout)
    rng = np.random.default_rng(seed)
    head = b"YUV4MPEG2 W%d H%d %s" % (w, h, extra) + (b" C" + tag.encode() if tag else b"") + b"\n"
    frames, body = [], b""
    for _ in range(n):
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        u = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        v = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        frames.append((y, u, v))
        body += b"FRAME\n" + y.tobytes() + u.tobytes() + v.tobytes()
    return head + body, frames
