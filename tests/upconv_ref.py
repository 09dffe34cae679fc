"""What the upconv head model tests share: seeded head models (tools/gen_model.py: He-scaled 3x3 layers, head weights N(0, 1 / (4 C))), the torch float64
restatement of the whole model -- replicate pad by the layer count, conv2d + LeakyReLU(0.1) per 3x3 layer, conv_transpose2d(stride 2, padding 3), no
activation behind it -- and the explicit index formula of include/w2xc_hip.h ("upconv head models") that the restatement is checked against."""
import numpy as np
import torch
import torch.nn.functional as F

from tools import gen_model

PUBLISHED = gen_model.TOPOLOGY_UPCONV7   # 3-16-32-64-128-128-256, head 256 -> 3


def head_model(planes, nout, seed, bias=True):
    """(layers, (W[c,o,4,4], bias or None))"""
    return gen_model.synth_layers(planes, seed), gen_model.synth_head(planes[-1], nout, seed, bias)


def _bias64(b, nout):
    # the engine narrows the double bias to float (cv::add's scalar rule); the reference adds that float
    b = np.zeros(nout) if b is None else np.asarray(b)
    return torch.from_numpy(b.astype(np.float32).astype(np.float64))


def chain_z(layers, x, n):
    """z = valid CNN over `layers` of x [nin, H, W] replicate-padded by n pixels, float64: [C, H + 2 (n - len(layers)), ...]"""
    t = F.pad(torch.from_numpy(np.asarray(x, np.float64))[None], (n, n, n, n), mode="replicate")
    for _, nout, w, b in layers:
        t = F.leaky_relu(F.conv2d(t, torch.from_numpy(w.astype(np.float64)), _bias64(b, nout)), 0.1)
    return t[0]


def reference(layers, head, x):
    """the whole head model on x [nin, H, W] in float64 -> [nout, 2H, 2W]"""
    hw, hb = head
    z = chain_z(layers, x, len(layers) + 1)
    return F.conv_transpose2d(z[None], torch.from_numpy(hw.astype(np.float64)), _bias64(hb, hw.shape[1]), stride=2, padding=3)[0].numpy()


def head_formula(z, hw, hb):
    """out[o][Y][X] = bias[o] + sum_c sum_{r, s: (Y + 3 - r), (X + 3 - s) even} Wt[c][o][r][s] z[c][(Y + 3 - r) / 2][(X + 3 - s) / 2], index by index"""
    z = np.asarray(z, np.float64)
    C, zh, zw = z.shape
    H, W = zh - 2, zw - 2
    nout = hw.shape[1]
    out = np.zeros((nout, 2 * H, 2 * W))
    taps = np.zeros((2 * H, 2 * W), int)
    for r in range(4):
        for s in range(4):
            Y = np.array([y for y in range(2 * H) if (y + 3 - r) % 2 == 0])
            X = np.array([x for x in range(2 * W) if (x + 3 - s) % 2 == 0])
            zy, zx = (Y + 3 - r) // 2, (X + 3 - s) // 2
            assert zy.min() >= 0 and zy.max() < zh and zx.min() >= 0 and zx.max() < zw   # all indices lie inside z
            out[:, Y[:, None], X[None, :]] += np.einsum("co,cyx->oyx", hw[:, :, r, s].astype(np.float64), z[:, zy[:, None], zx[None, :]])
            taps[Y[:, None], X[None, :]] += 1
    assert (taps == 4).all()   # exactly 2 x 2 taps per plane reach a pixel
    b = np.zeros(nout) if hb is None else np.asarray(hb).astype(np.float32).astype(np.float64)
    return out + b[:, None, None]


def ramp_planes(n, h, w):
    """n asymmetric positive planes (x, y and the plane distinguishable)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return np.stack([(0.05 + 0.013 * x + 0.029 * y + 0.0007 * x * y + 0.01 * p * (x + 1)).astype(np.float32) for p in range(n)])
