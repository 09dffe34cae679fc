"""Emulation of the 16-bit precisions for tests (TEST INFRASTRUCTURE): W2XC_PRECISION_BF16 / BF16X2 / BF16X3 /
FP16X2 are ONE pipeline (csrc/w2xc_split.hip) with 1, 2, 3 bf16 terms or 2 fp16 terms per value.  The emulation follows
the engine's dataflow layer by layer -- which kernel kind runs a layer and what its output is stored as is decided by
split_dataflow(), a Python mirror of layer_kind / fuse_first / fuse_last / out_terms_of in csrc/w2xc_select.cpp -- and
accumulates in float64 (the GPU accumulates in fp32 in MFMA order: the tests' bounds are for that difference alone).

An activation is split into 16-bit terms (one term = rounded, RNE) only where the layer that READS it is a split mid
layer, the second half of the fused first two layers, or a last layer computed inside the epilogue of the mid layer
before it; everything else -- the first layer, a plain last layer, and whatever those read and write -- is fp32."""
import numpy as np
import torch
import torch.nn.functional as F

# w2xc_opts.fusion (include/w2xc_hip.h)
FUSION_AUTO, FUSION_OFF, FUSION_ON, FUSION_FIRST, FUSION_LAST, FUSION_GATHER_LAUNCH, FUSION_PROG = 0, 1, 2, 3, 4, 5, 6

# mode -> (16-bit terms per value, fp16 terms?)
MODES = {"bf16": (1, False), "bf16x2": (2, False), "bf16x3": (3, False), "fp16x2": (2, True)}

PRODUCTS = {1: [(0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 3: [(1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)]}   # (activation term, weight term)

_MID = (32, 64, 128)
# kernel names as w2xc_layer_kernel_name reports them
K_FIRST, K_FIRST_SPLIT, K_FUSED_AWAY, K_FIRST2_SPLIT = "conv3x3_first", "conv3x3_first_split", "(in_next_layer)", "conv3x3_first2_split"
K_MID_SPLIT, K_LAST, K_LAST_GATHER = "conv3x3_split", "conv3x3_last", "conv3x3_last_gather"
SPLIT_CONSUMERS = (K_MID_SPLIT, K_FIRST2_SPLIT, K_LAST_GATHER)   # the kernels that read 16-bit terms


def _pick(cin, cout):   # w2xc_pick_kernel (csrc/w2xc_pack.cpp)
    if cin in _MID and cout in _MID:
        return "mfma"
    if cin in (1, 3) and cout in _MID:
        return "first"
    if cin in _MID and cout in (1, 3):
        return "last"
    return "direct"


def split_dataflow(planes, mode, fusion=FUSION_AUTO):
    """planes = [n_in, planes after layer 1, ..., planes after layer n]; mode = a key of MODES (or its term count, bf16).
    Returns per layer (kernel_name, cin, cout, out_terms): the kernel that w2xc_layer_kernel_name names and the
    out_terms of its output as out_terms_of (csrc/w2xc_select.cpp) answers them -- T = 16-bit term planes for a split mid
    layer behind it, 9 = the partial tap planes of the last layer computed in this layer's epilogue, 0 = fp32 (also for
    a layer 1 that runs inside conv3x3_first2_split: its activations never reach memory; the kernel keeps them as T terms).
    ValueError where the engine has no kernel for a layer (it refuses such a model with W2XC_ERR_UNSUPPORTED)."""
    T = MODES[mode][0] if mode in MODES else int(mode)
    io = list(zip(planes[:-1], planes[1:]))
    n = len(io)
    first_on = fusion not in (FUSION_OFF, FUSION_LAST)
    last_on = fusion not in (FUSION_OFF, FUSION_FIRST)
    # fuse_last: a one-plane last layer behind a mid layer that is not layer 1
    fuse_last = (last_on and n >= 3 and io[n - 1][1] == 1 and _pick(io[n - 1][0], 1) == "last" and _pick(*io[n - 2]) == "mfma" and n - 2 > 0)
    # fuse_first: layers 1 (1 -> 32) and 2 (a mid layer) in one kernel, unless layer 2 would have to carry the fused last layer
    fuse_first = (first_on and n >= 3 and io[0] == (1, 32) and _pick(*io[1]) == "mfma" and not (n == 3 and fuse_last))

    def kind(l):
        cin, cout = io[l]
        if l <= 1 and fuse_first:
            return K_FUSED_AWAY if l == 0 else K_FIRST2_SPLIT
        k = _pick(cin, cout)
        if k == "mfma" and l > 0:
            return K_MID_SPLIT
        if k == "first" and l == 0:
            return K_FIRST_SPLIT if (n > 1 and _pick(*io[1]) == "mfma") else K_FIRST
        if k == "last" and l == n - 1 and l > 0:
            return K_LAST_GATHER if fuse_last else K_LAST
        raise ValueError("16-bit precision modes: layer %d (%d->%d) has no kernel" % (l + 1, cin, cout))

    def out_terms(l):
        if l + 1 >= n:
            return 0
        if l == n - 2 and fuse_last:
            return 9
        return T if kind(l + 1) == K_MID_SPLIT else 0

    return [(kind(l), io[l][0], io[l][1], out_terms(l)) for l in range(n)]


def _split(t, terms, dtype=torch.bfloat16):
    """fp32 tensor -> list of `terms` 16-bit-valued float64 tensors: a0 = rnd(a), a1 = rnd(a - a0), ... (RNE)."""
    r = t.to(torch.float32)
    out = []
    for _ in range(terms):
        h = r.to(dtype).to(torch.float32)
        out.append(h.to(torch.float64))
        r = r - h          # exact in fp32
    return out


def convert_split_emulated(layers, plane, terms, n_in=1, fp16=False, fusion=FUSION_AUTO, accumulate="float64", trace=None):
    """Dataflow of the 16-bit pipeline (terms = 1, 2, 3) under the call's w2xc_opts.fusion, per layer as split_dataflow()
    names it: the first layer and a plain last layer are fp32 convolutions of fp32 activations with fp32 weights; a split
    mid layer (also as the second half of conv3x3_first2_split) and a last layer fused into the mid layer before it
    (conv3x3_last_gather finishes it) sum PRODUCTS[terms] of the 16-bit terms of their fp32 input and of their weights.
    fp16=True (W2XC_PRECISION_FP16X2): fp16 terms, split activations clamped to +-65504, weights scaled by the power of two that
    puts max|w| into [2^14, 2^15) and the sum scaled back.  Every layer's accumulator is cast to fp32 and LeakyReLU
    follows in fp32, as in the kernels.  accumulate="float64" sums exactly (to float64); "float32" runs the
    same dataflow with torch float32 convolutions: one more fp32 summation order, the yardstick for what two fp32 orders
    may differ by.  `plane` is (h, w) or (n_in, h, w); returns all output planes.  `trace`: a list that receives max |input| of
    every layer (the scale of what the layer sums: a test can tell an output that is a near-cancellation from it)."""
    assert accumulate in ("float64", "float32")
    acc_t = torch.float64 if accumulate == "float64" else torch.float32
    n = len(layers)
    dt = torch.float16 if fp16 else torch.bfloat16
    flow = split_dataflow([layers[0][0]] + [l[1] for l in layers], terms, fusion)
    x = np.ascontiguousarray(plane, dtype=np.float32)
    t = torch.from_numpy(x).reshape(1, n_in, x.shape[-2], x.shape[-1])
    t = F.pad(t.to(torch.float64), (n, n, n, n), mode="replicate").to(torch.float32)
    for (kernel, _, _, _), (nin, nout, w, b) in zip(flow, layers):
        bias = torch.from_numpy(b.astype(np.float32)).to(acc_t)
        if trace is not None:
            trace.append(float(t.abs().max()))
        wt = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        if kernel in SPLIT_CONSUMERS:
            scale = 1.0
            if fp16:
                mx = float(np.abs(w).max())
                scale = float(2.0 ** (15 - np.frexp(np.float32(mx))[1])) if mx > 0 else 1.0
                t = t.clamp(-65504.0, 65504.0)
            xs, ws = _split(t, terms, dt), _split(wt * np.float32(scale), terms, dt)
            acc = None
            if accumulate == "float64":
                # conv is linear: the products of one activation term share a convolution with the (exact) float64 sum of their weight terms
                for ta in range(terms):
                    wsum = sum(ws[tb] for (pa, tb) in PRODUCTS[terms] if pa == ta)
                    p = F.conv2d(xs[ta], wsum)
                    acc = p if acc is None else acc + p
            else:
                for (ta, tb) in PRODUCTS[terms]:
                    p = F.conv2d(xs[ta].to(acc_t), ws[tb].to(acc_t))
                    acc = p if acc is None else acc + p
            y = acc / scale + bias.view(1, -1, 1, 1)
        else:
            y = F.conv2d(t.to(acc_t), wt.to(acc_t), bias)
        y = y.to(torch.float32)                       # the accumulator is fp32
        t = torch.where(y > 0, y, np.float32(0.1) * y)
    return t[0].numpy()


def convert_mode_emulated(layers, plane, mode, n_in=1, fusion=FUSION_AUTO, accumulate="float64", trace=None):
    terms, fp16 = MODES[mode]
    return convert_split_emulated(layers, plane, terms, n_in=n_in, fp16=fp16, fusion=fusion, accumulate=accumulate, trace=trace)


def convert_bf16_emulated(layers, plane):
    """W2XC_PRECISION_BF16, default fusion: the one-term case of convert_split_emulated."""
    return convert_split_emulated(layers, plane, 1)[0]
