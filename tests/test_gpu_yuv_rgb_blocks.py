"""GPU tests of the two ends of YUV frames through RGB models (csrc/w2xc_yuv_rgb.hip through w2xc_yuv8_to_rgb_device and w2xc_rgb_to_yuv8_device).  Every
comparison is equality of float bits or of bytes with the NumPy restatement of include/w2xc_hip.h (tests/yuv_rgb_ref.py: float32, one operation per line).
Every buffer has a sentinel rim -- in front, behind, between rows, planes and frames, and with 2-byte samples between the samples -- that must be intact."""
import numpy as np
import pytest

import yuv_ref as yr
import yuv_rgb_ref as rr
from test_gpu_yuv_blocks import Lay, same_bits, stream
from test_gpu_yuv_frames import Side

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RIM_F = 8   # floats in front of and behind the float planes: they stay NaN
LAYOUT_IDS = {yr.YUV_420: "420", yr.YUV_422: "422", yr.YUV_444: "444"}
# the byte sides: planar / NV12 (v = u + 1) / NV21 (u = v + 1: with a colour matrix the order of U and V shows), each on the dword path (everything aligned,
# and the float planes' rows on 8-byte boundaries where the width is even: the 8-byte accesses) and on the byte path (odd base, odd strides)
PLANAR, NV12, NV21 = False, True, "nv21"
SIDES = [(PLANAR, True), (PLANAR, False), (NV12, True), (NV12, False), (NV21, True), (NV21, False)]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


class Side21(Side):
    """NV21: the two interleaved planes with V first -- u = v + 1"""

    def __init__(self, gpu, n, w, h, layout, aligned=False):
        super().__init__(gpu, n, w, h, layout, True, aligned)
        self.s.u, self.s.v = self.s.v, self.s.u
        assert self.s.u == self.s.v + 1

    def upload(self, Y, U, V):
        return super().upload(Y, V, U)

    def download(self):
        Y, first, second = super().download()
        return Y, second, first


def make_side(gpu, n, w, h, layout, kind, aligned):
    return Side21(gpu, n, w, h, layout, aligned) if kind == NV21 else Side(gpu, n, w, h, layout, bool(kind), aligned)


class Planes:
    """the 3 n float planes of n frames in a buffer with rims: planes of w * h floats ps apart, frames `img` apart, neither a round number -- odd numbers of
    floats, or (even) even ones: every row of an even width then starts on an 8-byte boundary"""

    def __init__(self, n, w, h, even=False):
        self.n, self.w, self.h = n, w, h
        self.ps = w * h + 3 + (even and (w * h + 3) % 2)
        self.img = 3 * self.ps + 7 + (even and (3 * self.ps + 7) % 2)
        self.total = 2 * RIM_F + n * self.img

    def index(self):
        f, p, q = np.meshgrid(np.arange(self.n), np.arange(3), np.arange(self.w * self.h), indexing="ij")
        return (RIM_F + f * self.img + p * self.ps + q).reshape(self.n, 3, self.h, self.w)

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


def to_rgb(gpu, Y, U, V, layout, rng, matrix, nv12=False, aligned=False):
    n, h, w = Y.shape
    side = make_side(gpu, n, w, h, layout, nv12, aligned).upload(Y, U, V)
    P = Planes(n, w, h, aligned)
    d = torch.full((P.total,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.yuv8_to_rgb_device(side.s, n, w, h, layout, rng, matrix, d.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, stream=stream().cuda_stream)
    stream().synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(side.download(), (Y, U, V))), "the frames were written"
    return P.gather(d.cpu().numpy())


def from_rgb(gpu, x, layout, rng, matrix, nv12=False, aligned=False):
    n, _, h, w = x.shape
    P = Planes(n, w, h, aligned)
    d = torch.from_numpy(P.scatter(x)).cuda()
    side = make_side(gpu, n, w, h, layout, nv12, aligned)
    gpu.rgb_to_yuv8_device(d.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, n, w, h, layout, rng, matrix, side.s, stream=stream().cuda_stream)
    stream().synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint32), P.scatter(x).view(np.uint32)), "the planes were written"
    return side.download()   # (checks the rims)


def ref_to_rgb(Y, U, V, layout, rng, matrix):
    return np.stack([rr.yuv8_to_rgb(Y[i], U[i], V[i], layout, rng, matrix) for i in range(Y.shape[0])])


def ref_from_rgb(x, layout, rng, matrix):
    out = [rr.rgb_to_yuv8(x[i], layout, rng, matrix) for i in range(x.shape[0])]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def frames(n, w, h, layout, seed):
    g = np.random.default_rng(seed)
    cw, ch = yr.chroma_size(w, h, layout)
    return g.integers(0, 256, (n, h, w), dtype=np.uint8), g.integers(0, 256, (n, ch, cw), dtype=np.uint8), g.integers(0, 256, (n, ch, cw), dtype=np.uint8)


def planes(n, w, h, seed):
    """R, G, B around and beyond [0, 1]"""
    return (np.random.default_rng(seed).random((n, 3, h, w), dtype=np.float32) * np.float32(1.3) - np.float32(0.15)).astype(np.float32)


def same_bytes(got, want):
    for name, a, b in zip("YUV", got, want):
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %d of %d bytes differ" % (name, int((a != b).sum()), a.size)
    return True


CONFIGS = [(m, r, l) for m in rr.MATRICES for r in (yr.FULL, yr.LIMITED) for l in rr.LAYOUTS]
CONFIG_IDS = ["%s-%s-%s" % (("bt601", "bt709", "bt2020")[m], ("full", "limited")[r], LAYOUT_IDS[l]) for m, r, l in CONFIGS]
# (w, h): the smallest, odd sizes with a cut block at both edges, more than one tile either way in every layout -- with an odd and with an even width
SMALL = [(1, 1), (2, 2), (3, 5), (67, 35), (66, 35)]


@pytest.mark.parametrize("matrix,rng,layout", CONFIGS, ids=CONFIG_IDS)
def test_yuv8_to_rgb(gpu, matrix, rng, layout):
    for w, h in SMALL:
        Y, U, V = frames(3, w, h, layout, 7 * w + h)
        want = ref_to_rgb(Y, U, V, layout, rng, matrix)
        if w * h > 1000:
            assert want.min() == 0.0 and want.max() == 1.0, "random frames clamp on both sides"
        for nv12, aligned in SIDES:
            assert same_bits(to_rgb(gpu, Y, U, V, layout, rng, matrix, nv12, aligned), want), (w, h, nv12, aligned)


@pytest.mark.parametrize("matrix,rng,layout", CONFIGS, ids=CONFIG_IDS)
def test_rgb_to_yuv8(gpu, matrix, rng, layout):
    for w, h in SMALL:
        x = planes(3, w, h, 11 * w + h)
        want = ref_from_rgb(x, layout, rng, matrix)
        for nv12, aligned in SIDES:
            assert same_bytes(from_rgb(gpu, x, layout, rng, matrix, nv12, aligned), want), (w, h, nv12, aligned)


def edge_sizes(layout):
    """one below, at and one above a tile edge in both directions, in luma samples"""
    tw = rr.TCX * (1 if layout == yr.YUV_444 else 2)
    th = rr.TCY * (2 if layout == yr.YUV_420 else 1)
    return [(w, h) for w in (tw - 1, tw, tw + 1) for h in (th - 1, th, th + 1)]


@pytest.mark.parametrize("layout", rr.LAYOUTS, ids=list(LAYOUT_IDS.values()))
def test_tile_edges(gpu, layout):
    for w, h in edge_sizes(layout):
        Y, U, V = frames(1, w, h, layout, w + 100 * h)
        want = ref_to_rgb(Y, U, V, layout, yr.LIMITED, rr.BT709)
        x = planes(1, w, h, w + 100 * h)
        back = ref_from_rgb(x, layout, yr.LIMITED, rr.BT709)
        for nv12, aligned in ((PLANAR, True), (NV12, False), (NV21, True)):
            assert same_bits(to_rgb(gpu, Y, U, V, layout, yr.LIMITED, rr.BT709, nv12, aligned), want), (w, h, nv12)
            assert same_bytes(from_rgb(gpu, x, layout, yr.LIMITED, rr.BT709, nv12, aligned), back), (w, h, nv12)


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("matrix", rr.MATRICES, ids=["bt601", "bt709", "bt2020"])
def test_all_luma_values_and_extreme_frames(gpu, matrix, rng):
    """all 256 luma values against several chroma pairs (a frame per pair, 4:4:4: no neighbour mixes in), and constant frames of extreme values in every
    layout: inputs that clamp on both sides"""
    pairs = [(128, 128), (0, 0), (255, 255), (0, 255), (255, 0), (16, 240), (240, 16), (100, 200)]
    Y = np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, 16, 16), (len(pairs), 16, 16)).copy()
    U = np.stack([np.full((16, 16), u, np.uint8) for u, _ in pairs])
    V = np.stack([np.full((16, 16), v, np.uint8) for _, v in pairs])
    want = ref_to_rgb(Y, U, V, yr.YUV_444, rng, matrix)
    assert (want == 0.0).any() and (want == 1.0).any()
    assert same_bits(to_rgb(gpu, Y, U, V, yr.YUV_444, rng, matrix, False, True), want)
    y0 = np.clip(yr.luma_in(Y[0], rng), np.float32(0), np.float32(1))
    assert all(same_bits(want[0, c], y0) for c in range(3)), "neutral chroma: R = G = B = y"
    for layout in rr.LAYOUTS:
        cw, ch = yr.chroma_size(5, 3, layout)
        for yv, uv, vv in ((0, 0, 0), (255, 255, 255), (16, 240, 16)):
            Yc, Uc, Vc = np.full((1, 3, 5), yv, np.uint8), np.full((1, ch, cw), uv, np.uint8), np.full((1, ch, cw), vv, np.uint8)
            want = ref_to_rgb(Yc, Uc, Vc, layout, rng, matrix)
            assert (want.reshape(3, -1) == want.reshape(3, -1)[:, :1]).all(), "a constant frame gives constant planes"
            assert same_bits(to_rgb(gpu, Yc, Uc, Vc, layout, rng, matrix), want)


def tie_planes(matrix, rng):
    """R planes (G = B = 0, so y' = Kr * R in one rounding) whose luma product lands on k + 0.5 exactly: 255 y' = k + 0.5 for full range, y' * 219 = k + 0.5 - 16
    for limited range (the sum with 16 is then exact).  Returns (R values, the k of each)."""
    Kr = rr.constants(matrix)["Kr"]
    scale, off = (np.float32(219.0), 16.0) if rng == yr.LIMITED else (np.float32(255.0), 0.0)
    vals, ks = [], []
    for k in range(int(off), 255):
        target = np.float32(k + 0.5 - off)
        guess = np.float32((k + 0.5 - off) / float(scale) / float(Kr))
        cand = guess + np.arange(-400, 401, dtype=np.float32) * np.spacing(guess)
        y = Kr * cand
        hit = np.nonzero(y * scale == target)[0]
        if hit.size:
            vals.append(cand[hit[0]])
            ks.append(k)
    return np.array(vals, np.float32), np.array(ks)


@pytest.mark.parametrize("rng", [yr.FULL, yr.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("matrix", rr.MATRICES, ids=["bt601", "bt709", "bt2020"])
def test_rounding_ties_and_saturation(gpu, matrix, rng):
    R, ks = tie_planes(matrix, rng)
    assert R.size >= 32, "ties constructed: %d" % R.size
    x = np.zeros((1, 3, 1, R.size), np.float32)
    x[0, 0, 0] = R
    got = from_rgb(gpu, x, yr.YUV_444, rng, matrix)
    assert same_bytes(got, ref_from_rgb(x, yr.YUV_444, rng, matrix))
    assert np.array_equal(got[0][0, 0], (2 * np.round((ks + 0.5) / 2)).astype(np.uint8)), "half to even"
    # far beyond [0, 1]: every byte saturates, in every layout, and the rounding is the restatement's
    big = np.array([-1e30, -3.0, -0.2, 0.0, 1.0, 1.2, 3.0, 1e30], np.float32)
    x = np.stack(np.meshgrid(big, big, big, indexing="ij")).reshape(1, 3, 16, 32)
    for layout in rr.LAYOUTS:
        got = from_rgb(gpu, x, layout, rng, matrix)
        assert same_bytes(got, ref_from_rgb(x, layout, rng, matrix))
        assert got[0].min() == 0 and got[0].max() == 255 and got[1].min() == 0 and got[1].max() == 255 and got[2].min() == 0 and got[2].max() == 255


def test_more_tiles_than_workgroups(gpu):
    """a narrow, tall frame: the grid-stride loop of both kernels takes a second trip (tests/test_yuv_rgb_api.py holds the shape to the launchers' rule)"""
    w, h, layout, n = (rr.SECOND_TRIP[k] for k in ("w", "h", "layout", "n"))
    turns, grid = rr.launch(w, h, layout, n)
    assert turns > grid
    Y, U, V = frames(n, w, h, layout, 5)
    assert same_bits(to_rgb(gpu, Y, U, V, layout, yr.LIMITED, rr.BT709, False, True), ref_to_rgb(Y, U, V, layout, yr.LIMITED, rr.BT709))
    x = planes(n, w, h, 6)
    assert same_bytes(from_rgb(gpu, x, layout, yr.LIMITED, rr.BT709, True, False), ref_from_rgb(x, layout, yr.LIMITED, rr.BT709))


@pytest.mark.parametrize("layout", rr.LAYOUTS, ids=list(LAYOUT_IDS.values()))
def test_two_byte_samples_of_separate_planes(gpu, layout):
    """c_px = 2 with U and V in two buffers of their own: the bytes between a plane's samples are another plane's and keep their values"""
    n, w, h = 2, 35, 19
    cw, ch = yr.chroma_size(w, h, layout)
    x = planes(n, w, h, 77)
    want = ref_from_rgb(x, layout, yr.FULL, rr.BT601)
    P = Planes(n, w, h)
    d = torch.from_numpy(P.scatter(x)).cuda()
    ly, lc = Lay(n, h, w, 1, False), Lay(n, ch, cw, 2, False)
    before = [np.random.default_rng(s).integers(0, 256, lc.total, dtype=np.uint8) for s in (1, 2)]
    by = torch.full((ly.total,), 0xAB, dtype=torch.uint8, device="cuda")
    bc = [torch.from_numpy(b).cuda() for b in before]
    s = gpu.YuvPlanes()
    s.y, s.y_stride, s.y_frame_stride = by.data_ptr() + ly.off, ly.row, ly.frame
    s.u, s.v, s.c_stride, s.c_frame_stride, s.c_px = bc[0].data_ptr() + lc.off, bc[1].data_ptr() + lc.off, lc.row, lc.frame, 2
    gpu.rgb_to_yuv8_device(d.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, n, w, h, layout, yr.FULL, rr.BT601, s, stream=stream().cuda_stream)
    stream().synchronize()
    assert np.array_equal(ly.gather(by.cpu().numpy(), 0xAB), want[0])
    idx = lc.index()
    for b, old, wanted in zip(bc, before, want[1:]):
        now = b.cpu().numpy()
        assert np.array_equal(now[idx], wanted)
        rest = np.ones(lc.total, bool)
        rest[idx] = False
        assert np.array_equal(now[rest], old[rest]), "bytes between the samples were written"
    # ... and read from such planes: the same floats as from planar ones
    Y, U, V = frames(n, w, h, layout, 78)
    for b, Pl in zip(bc, (U, V)):
        b.copy_(torch.from_numpy(lc.scatter(Pl, "random")))
    by.copy_(torch.from_numpy(ly.scatter(Y, 0xAB)))
    o = torch.full((P.total,), float("nan"), dtype=torch.float32, device="cuda")
    gpu.yuv8_to_rgb_device(s, n, w, h, layout, yr.FULL, rr.BT601, o.data_ptr() + 4 * RIM_F, 4 * P.img, 4 * P.ps, stream=stream().cuda_stream)
    stream().synchronize()
    assert same_bits(P.gather(o.cpu().numpy()), ref_to_rgb(Y, U, V, layout, yr.FULL, rr.BT601))
