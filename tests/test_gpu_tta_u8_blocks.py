"""GPU tests of the TTA building blocks with a uint8 image at their outer side (revision 0.4.1.6.3: w2xc_tta_spread_u8_device, w2xc_tta_gather_u8_device;
kernels in w2xc_tta_u8.hip).  Every comparison is EQUALITY of bits / bytes against the blocks that existed: w2xc_u8_to_rgb_device + w2xc_tta_spread_device
for the spread, w2xc_tta_gather_device + w2xc_rgb_to_u8_device for the gather, with torch for the channel selection and the merge into the pixels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 32
SENTINEL = 0xA5
# one pixel; a tile edge + 1 both ways; one tile; several tiles on both axes; one row / one column below a tile
SIZES = [(1, 1), (17, 33), (33, 17), (32, 32), (40, 70), (31, 1), (1, 31)]
SIZE_IDS = ["%dx%d" % s for s in SIZES]
# (px_bytes, ch0, ch_step) the engine uses: the bled 3-byte image, the colour of RGBA pixels, the grey image (A, A, A) of RGBA pixels
SPREADS = [(3, 0, 1), (4, 0, 1), (4, 3, 0)]
# (planes_per_image, first_plane, n_ch, byte0) into 4-byte pixels: colour, alpha out of a 3-plane result, alpha out of a one-plane result; and the packed
# 3-byte image of the building block's own definition
GATHERS = [(3, 0, 3, 4, 0), (3, 1, 1, 4, 3), (1, 0, 1, 4, 3), (3, 0, 3, 3, 0)]
# the second trips of the kernels' two grid-stride loops (at most 65536 tiles, 65535 images per launch)
SECOND_TRIPS = [((1, TILE * 65536 + 1), 1), ((1, 1), 65537)]
SECOND_TRIP_IDS = ["%dx%d-n%d" % (s + (n,)) for s, n in SECOND_TRIPS]


@pytest.fixture(scope="module")
def gpu(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return w2xc


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view(torch.int32)


def u8_images(n, h, w, px, seed, lead=0, pad=0):
    """n images in one device buffer: `lead` bytes in front (lead = 1: no row starts on a 4-byte boundary where the row stride is even), rows px w + pad
    bytes apart, an image stride with a few bytes more.  -> (buffer, pointer of image 0, image stride, row stride, the pixels [n, h, w, px] as a view)"""
    rs = px * w + pad
    ims = rs * h + 2 * pad
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = torch.randint(0, 256, (lead + n * ims,), dtype=torch.uint8, generator=g).cuda()
    view = torch.as_strided(buf, (n, h, w, px), (ims, rs, px, 1), lead)
    return buf, buf.data_ptr() + lead, ims, rs, view


def check_spread(gpu, hw, n, px, ch0, step, lead=0, pad=0):
    h, w = hw
    ps = w * h + 5
    buf, p, ims, rs, pix = u8_images(n, h, w, px, 7 * h + 3 * w + n + px + ch0, lead, pad)
    before = buf.clone()
    # the definition: the selected bytes as a packed 3-byte image (torch), u8 / 255 per image, the float spread on 3 n planes
    sel = torch.stack([pix[..., ch0 + c * step] for c in range(3)], dim=-1).contiguous()
    planes = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    if n <= 4:
        for i in range(n):
            gpu.u8_to_rgb_device(sel[i].data_ptr(), 3 * w, w, h, planes[i].data_ptr(), stream=stream())
    else:   # (many one-pixel images: the same expression, (float)byte * (float)(1.0 / 255.0), in torch)
        planes.copy_(sel.permute(0, 3, 1, 2).to(torch.float32) * np.float32(1.0 / 255.0))
    want = [torch.full((4 * 3 * n * ps,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    gpu.tta_spread_device(planes.data_ptr(), 3 * n, w * h * 4, w * 4, w, h, want[0].data_ptr(), want[1].data_ptr(), ps * 4, stream=stream())
    got = [torch.full((4 * 3 * n * ps,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    gpu.tta_spread_u8_device(p, n, ims, rs, px, ch0, step, w, h, got[0].data_ptr(), got[1].data_ptr(), ps * 4, stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(got[0]), bits(want[0])), "upright variants (the floats behind a plane's last element included)"
    assert torch.equal(bits(got[1]), bits(want[1])), "transposed variants"
    assert torch.equal(buf, before), "the source was written"
    if n <= 4 and h * w > 1:
        assert not torch.isnan(got[0].view(4 * 3 * n, ps)[:, :w * h]).any()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("sel", SPREADS, ids=["px%d-ch%d-step%d" % s for s in SPREADS])
@pytest.mark.parametrize("hw", SIZES, ids=SIZE_IDS)
def test_spread_u8_bit_for_bit(gpu, hw, sel, n):
    check_spread(gpu, hw, n, *sel)                      # packed: 4-byte pixels on 4-byte boundaries
    check_spread(gpu, hw, n, *sel, lead=1, pad=3)       # no pixel and no row start on a 4-byte boundary


@pytest.mark.parametrize("sel", SPREADS[1:], ids=["px%d-ch%d-step%d" % s for s in SPREADS[1:]])
def test_spread_u8_aligned_pixels_unaligned_strides(gpu, sel):
    """4-byte pixels whose first one is aligned while the row stride (or, n > 1, the image stride) is not: the word path must not be taken"""
    check_spread(gpu, (17, 33), 1, *sel, pad=1)
    check_spread(gpu, (17, 33), 3, *sel, pad=2)         # rows of 4 w + 2, images of 17 (4 w + 2) + 4: even strides, not multiples of 4


@pytest.mark.parametrize("hw,n", SECOND_TRIPS, ids=SECOND_TRIP_IDS)
def test_spread_u8_second_trips(gpu, hw, n):
    check_spread(gpu, hw, n, 4, 0, 1)
    check_spread(gpu, hw, n, 4, 3, 0, lead=1)


def result_planes(m, h, w, seed):
    """8 m result planes as the two group buffers [4 m, ps]: mixed magnitudes across the eight variants (a reordered sum rounds differently), means at
    the rounding ties (k + 0.5) / 255, below 0, above 1"""
    ps = w * h + 5
    g = torch.Generator(device="cpu").manual_seed(seed)
    up = torch.full((4 * m, ps), float("nan"), dtype=torch.float32)
    tr = torch.full((4 * m, ps), float("nan"), dtype=torch.float32)
    for buf in (up, tr):
        v = torch.rand((4 * m, w * h), generator=g, dtype=torch.float32) * 1.5 - 0.25                      # below 0 and above 1 among them
        v += torch.randn((4 * m, w * h), generator=g, dtype=torch.float32) * 10.0 ** torch.randint(-6, 0, (4 * m, w * h), generator=g).float()
        buf[:, :w * h] = v
    q = w * h
    # every third element of every plane (planes of three elements and more): the variants hold v, v, 2 v, 0, 4 v, 0, 0, 0, so every partial sum of the
    # definition's order is v times a power of two and the mean is v exactly.  Element (y, x) of the upright plane is element tta_at(k, y, x) of variant k:
    # the planes are filled through the index maps of the definition
    if q < 3:
        return up.cuda(), tr.cuda(), ps
    ys, xs = np.divmod(np.arange(q), w)
    tie = ((np.arange(q) * 7 % 256) + 0.5) / 255.0
    tie[::5] = -0.3
    tie[1::5] = 1.7
    pick = np.arange(q) % 3 == 0
    for k in range(8):
        xx = w - 1 - xs if k & 1 else xs
        yy = h - 1 - ys if k & 2 else ys
        at = xx * h + yy if k & 4 else yy * w + xx
        buf = up if k < 4 else tr
        rows = buf[(k & 3) * m:(k & 3) * m + m]
        rows[:, torch.from_numpy(at[pick])] = torch.from_numpy(tie[pick].astype(np.float32)) * (1.0, 1.0, 2.0, 0.0, 4.0, 0.0, 0.0, 0.0)[k]
    return up.cuda(), tr.cuda(), ps


def gather_reference(gpu, up, tr, ps, n, ppi, first, nch, h, w):
    """[n, h, w, nch] bytes: the float gather on all ppi n planes, torch for the plane selection, w2xc_rgb_to_u8_device for the rounding"""
    m = ppi * n
    mean = torch.full((m, h, w), float("nan"), dtype=torch.float32, device="cuda")
    gpu.tta_gather_device(up.data_ptr(), tr.data_ptr(), ps * 4, m, w, h, mean.data_ptr(), w * h * 4, w * 4, stream=stream())
    mean = mean.view(n, ppi, h, w)
    sel = torch.stack([mean[:, first + min(c, nch - 1)] for c in range(3)], dim=1).contiguous()     # (a one-channel selection: three times that plane)
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    if n <= 4:
        for i in range(n):
            gpu.rgb_to_u8_device(sel[i].data_ptr(), w, h, u8[i].data_ptr(), 3 * w, stream=stream())
    else:   # (many one-pixel images: saturate(rint(255 x)), half to even, in torch)
        u8.copy_(torch.clamp(torch.round(sel.permute(0, 2, 3, 1) * np.float32(255.0)), 0, 255).to(torch.uint8))
    return u8[..., :nch]


def run_gather(gpu, up, tr, ps, n, ppi, first, nch, px, byte0, h, w, dst=None, lead=0, pad=0):
    rs = px * w + pad
    ims = rs * h + 2 * pad
    if dst is None:
        dst = torch.full((lead + n * ims,), SENTINEL, dtype=torch.uint8, device="cuda")
    gpu.tta_gather_u8_device(up.data_ptr(), tr.data_ptr(), ps * 4, n, ppi, first, nch, w, h, dst.data_ptr() + lead, ims, rs, px, byte0, stream=stream())
    return dst, torch.as_strided(dst, (n, h, w, px), (ims, rs, px, 1), lead)


def check_gather(gpu, hw, n, ppi, first, nch, px, byte0, lead=0, pad=0):
    h, w = hw
    up, tr, ps = result_planes(ppi * n, h, w, 11 * h + 5 * w + n + ppi + first)
    ref = gather_reference(gpu, up, tr, ps, n, ppi, first, nch, h, w)
    rs = px * w + pad
    want = torch.full((lead + n * (rs * h + 2 * pad),), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.as_strided(want, (n, h, w, px), (rs * h + 2 * pad, rs, px, 1), lead)[..., byte0:byte0 + nch] = ref
    got, _ = run_gather(gpu, up, tr, ps, n, ppi, first, nch, px, byte0, h, w, lead=lead, pad=pad)
    torch.cuda.synchronize()
    assert torch.equal(got, want), "the named bytes, and the sentinel in every other byte: the pixel's other bytes, row padding, between the images"
    return ref


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("sel", GATHERS, ids=["ppi%d-first%d-nch%d-px%d-byte%d" % s for s in GATHERS])
@pytest.mark.parametrize("hw", SIZES, ids=SIZE_IDS)
def test_gather_u8_byte_for_byte(gpu, hw, sel, n):
    ref = check_gather(gpu, hw, n, *sel)
    check_gather(gpu, hw, n, *sel, lead=1, pad=3)
    if hw == (40, 70) and sel[2] == 3:   # the inputs hold what they are meant to: bytes from both saturations and from ties
        ref = ref.cpu().numpy()
        assert (ref == 0).any() and (ref == 255).any() and ((ref > 0) & (ref < 255)).any()


def test_gather_u8_inputs_tell_ties_and_the_order_of_the_sum(gpu):
    """the reference itself: at the tie elements the mean is (k + 0.5) / 255 exactly and rounds half to even; elsewhere a reordered sum gives other floats"""
    h, w, m = 40, 70, 3
    up, tr, ps = result_planes(m, h, w, 5)
    mean = torch.empty((m, h, w), dtype=torch.float32, device="cuda")
    gpu.tta_gather_device(up.data_ptr(), tr.data_ptr(), ps * 4, m, w, h, mean.data_ptr(), w * h * 4, w * 4, stream=stream())
    torch.cuda.synchronize()
    mean = mean.cpu().numpy().reshape(m, -1)
    q = np.arange(w * h)
    k = q * 7 % 256
    ties = (q % 3 == 0) & (q % 5 > 1)
    assert np.array_equal(mean[:, ties], np.broadcast_to(((k[ties] + 0.5) / 255.0).astype(np.float32), (m, ties.sum())))
    prod = mean[:, ties] * np.float32(255.0)
    assert (prod == np.floor(prod) + 0.5).mean() > 0.5, "most tie values must still be ties after the fp32 product with 255"
    u, t = up.cpu().numpy()[:, :w * h], tr.cpu().numpy()[:, :w * h]
    assert np.abs(u).max() / np.abs(u[u != 0]).min() > 1e3 and not np.array_equal(u[:m], t[:m])


def test_two_gathers_into_the_same_pixels_in_either_order(gpu):
    h, w, n = 40, 70, 2
    up3, tr3, ps = result_planes(3 * n, h, w, 21)
    up1, tr1, _ = result_planes(n, h, w, 22)
    colour = gather_reference(gpu, up3, tr3, ps, n, 3, 0, 3, h, w)
    for alpha_from in ("three planes", "one plane"):
        a = (up3, tr3, ps, n, 3, 1, 1) if alpha_from == "three planes" else (up1, tr1, ps, n, 1, 0, 1)
        alpha = gather_reference(gpu, *a, h, w)
        want = torch.cat([colour, alpha], dim=-1)
        first, px1 = run_gather(gpu, up3, tr3, ps, n, 3, 0, 3, 4, 0, h, w, pad=3)
        run_gather(gpu, *a, 4, 3, h, w, dst=first, pad=3)
        second, px2 = run_gather(gpu, *a, 4, 3, h, w, pad=3)
        run_gather(gpu, up3, tr3, ps, n, 3, 0, 3, 4, 0, h, w, dst=second, pad=3)
        torch.cuda.synchronize()
        assert torch.equal(px1, want) and torch.equal(px2, want), alpha_from
        assert torch.equal(first, second), alpha_from


@pytest.mark.parametrize("hw,n", SECOND_TRIPS, ids=SECOND_TRIP_IDS)
def test_gather_u8_second_trips(gpu, hw, n):
    check_gather(gpu, hw, n, 3, 0, 3, 4, 0)
    check_gather(gpu, hw, n, 3, 1, 1, 4, 3, lead=1)
