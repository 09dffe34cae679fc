// w2xc_upconv.hip -- upconv4x4_head: the head of an upconv model, a 4x4 stride-2 padding-3 transposed convolution from C NHWC planes of (h + 2) x (w + 2)
// pixels to NOUT planes of 2h x 2w (the definition: include/w2xc_hip.h, "upconv head models").  The sibling of conv3x3_last (w2xc_kernels.hip), "taps as N":
//   per pixel q of the haloed source tile   G[q][n] = sum_c z[q][c] * Wt[c][o][r][s],  n = (4 r + s) * NOUT + o,  N = 16 NOUT = NOUT whole 16-column blocks,
//   on v_mfma_f32_16x16x4_f32 (M = 16 pixels, K = 4).  A comes straight from global memory: lane (i = lane & 15, kk = lane >> 4) loads channels
//   16 s4 + 4 kk .. + 3 of pixel i as one dwordx4; MFMA j of group s4 contracts the channels {16 s4 + 4 kk + j}.  B = the w2xc_upconv_pack image, kept in LDS
//   (at C = 256 it would be 192 registers a lane).
//   Then output pixel (2 y + py, 2 x + px) of the tile sums its four taps out of G in LDS -- r = 1 - py, 3 - py and s = 1 - px, 3 - px, the z pixel
//   (y + (py + 3 - r) / 2, x + (px + 3 - s) / 2) of the view whose row 0 / column 0 is z row y0 / z column 0 (off_y, off_x as for every layer) -- in the
//   order r ascending, s ascending, starting from 0.0f; the bias is added last and NO activation follows.  Every fp32 operation is separate
//   (-ffp-contract=off), so the float and the uint8 form, and every band, give one pixel the same bits.
// Workgroup = 4 waves, tile = 8 x 32 source pixels = 16 x 64 output pixels; a workgroup walks a run of consecutive tiles (w2xc_upconv_grid workgroups).
// The body is w2xc_upconv_body.inc, shared with the batch form upconv4x4_head_batch below (an object of its own: -DW2XC_UPCONV_BATCH).
#include "w2xc_kernels.h"
#include "w2xc_device.h"
#include "w2xc_launch.hpp"

// U8 (W2XC_K_UPCONV_U8): the sink is an interleaved uint8 image as for conv3x3_last<U8> -- d.out points at bytes, out_rs / out_ps / out_cs are byte
// strides (row stride, 3 or 4, 1) -- and the epilogue stores saturate(rint(255 v)), one byte store per value.  out_ps = 4: the colour bytes of RGBA pixels
// (the RGBA call for head models), the fourth byte is never touched.
// The alpha head (W2XC_K_UPCONV_A_U8, <CIN, 1, true>): ONE plane into byte d.out[0] of pixels out_ps = 3 or 4 bytes apart, on the image packed from channel 1
// of a three-plane head (w2xc_upconv_pack_alpha) with bias[1].  A column's MFMA chain does not depend on its neighbours and the tap sum is per plane: the
// byte has the bits of channel 1 of the three-plane launch, at a third of its matrix work and of its LDS.
// W2XC_K_UPCONV_A is that head with the float sink (<CIN, 1, false>, the instantiation of one-plane head models): the same image and bias[1], ONE float plane
// at d.out with the bits of plane 1 of the three-plane launch -- the last alpha pass of the RGBA TTA call, whose mean is taken before the rounding.
// the sink a kind may have: float planes (pixels one float apart); three uint8 channels one byte apart in pixels of 3 or 4 bytes; the alpha head's one byte
static bool w2xc_upconv_sink_ok(W2xcKernelKind kind, const W2xcConvDesc &d)
{
    switch (kind) {
    case W2XC_K_UPCONV: return d.out_ps == 1;
    case W2XC_K_UPCONV_A: return d.cout == 1 && d.out_ps == 1;   // (the alpha head with the float sink: <CIN, 1, false>)
    case W2XC_K_UPCONV_U8: return d.cout == 3 && (d.out_ps == 3 || d.out_ps == 4) && d.out_cs == 1;
    case W2XC_K_UPCONV_A_U8: return d.cout == 1 && (d.out_ps == 3 || d.out_ps == 4);
    default: return false;
    }
}

template <int CIN, int NOUT, bool U8>
__global__ void __launch_bounds__(256) upconv4x4_head(W2xcConvDesc d, int tiles_x, int ntiles)
{
#define UPB_ONLY(...)
#define UPB_SEL(b_, s_) s_
#define UPB_IN d.in
#define UPB_OUT d.out
#include "w2xc_upconv_body.inc"
#undef UPB_OUT
#undef UPB_IN
#undef UPB_SEL
#undef UPB_ONLY
}

// batch form (w2xc_convert_planes_up2x_batch_device, the head-model image batch and its TTA pass): bd.batch images of `ntiles` tiles each, image i's NHWC planes
// bd.in_bs floats behind image 0's, its output bd.out_bs floats (U8: bytes) behind image 0's.  The one-image body with the batch hooks on: per tile the same
// loads, MFMAs, tap sums and stores -- a pixel has the bits of the single launch.  An object of its own (W2XC_UPCONV_BATCH), like every batch form.
#ifdef W2XC_UPCONV_BATCH
template <int CIN, int NOUT, bool U8>
__global__ void __launch_bounds__(256) upconv4x4_head_batch(W2xcConvDesc d, int tiles_x, int ntiles, W2xcBatchDesc bd)
{
#define UPB_ONLY(...) __VA_ARGS__
#define UPB_SEL(b_, s_) b_
#define UPB_IN (d.in + (long long)img * bd.in_bs)
#define UPB_OUT (U8 ? reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(d.out) + (long long)img * bd.out_bs) : d.out + (long long)img * bd.out_bs)
#include "w2xc_upconv_body.inc"
#undef UPB_OUT
#undef UPB_IN
#undef UPB_SEL
#undef UPB_ONLY
}

template <int CIN, int NOUT, bool U8>
static hipError_t launch_upconv_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    const long long tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + 7) / 8;
    if (tiles_x * tiles_y * b.batch > 0x7fffffffll) return hipErrorInvalidValue;
    const int ntiles = (int)(tiles_x * tiles_y);
    b.items = ntiles;
    constexpr size_t lds_bytes = ((size_t)22 * 16 * ((16 * NOUT) | 1) + (size_t)16 * NOUT * CIN) * sizeof(float);   // G + the weight image
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    auto kern = upconv4x4_head_batch<CIN, NOUT, U8>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_upconv_grid(ntiles * b.batch)), dim3(256), lds_bytes, stream, d, (int)tiles_x, ntiles, b);
    return hipGetLastError();
}

// d = the single-image descriptor of w2xc_launch_upconv (its checks apply unchanged), b.in_bs = the image stride of the NHWC planes in floats (a multiple of 4:
// 16-byte loads), b.out_bs = that of the output: floats, or -- W2XC_K_UPCONV_U8 -- bytes
hipError_t w2xc_launch_upconv_batch(W2xcKernelKind kind, const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0 || b.batch == 0) return hipSuccess;
    if (b.batch < 0 || b.in_bs < 0 || b.out_bs < 0 || (b.in_bs & 3) != 0) return hipErrorInvalidValue;
    if (d.in_shift != 0 || d.in_ps != d.cin || d.in_cs != 1 || (d.in_rs & 3) != 0 || (((size_t)d.in) & 15) != 0) return hipErrorInvalidValue;
    if (d.in_h < 1 || d.in_w < 1) return hipErrorInvalidValue;
    const bool u8 = kind != W2XC_K_UPCONV && kind != W2XC_K_UPCONV_A;
    if (!w2xc_upconv_sink_ok(kind, d)) return hipErrorInvalidValue;
    switch (d.cin * 10 + d.cout) {
#define W2XC_UPCONV_CASE(C)                                                                                        \
    case C * 10 + 1: return u8 ? launch_upconv_batch<C, 1, true>(d, b, stream) : launch_upconv_batch<C, 1, false>(d, b, stream); \
    case C * 10 + 3: return u8 ? launch_upconv_batch<C, 3, true>(d, b, stream) : launch_upconv_batch<C, 3, false>(d, b, stream);
        W2XC_UPCONV_CASE(32)
        W2XC_UPCONV_CASE(64)
        W2XC_UPCONV_CASE(128)
        W2XC_UPCONV_CASE(256)
#undef W2XC_UPCONV_CASE
    default: return hipErrorInvalidValue;
    }
}
#else

template <int CIN, int NOUT, bool U8>
static hipError_t launch_upconv(const W2xcConvDesc &d, hipStream_t stream)
{
    const long long tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + 7) / 8;
    if (tiles_x * tiles_y > 0x7fffffffll) return hipErrorInvalidValue;
    const int ntiles = (int)(tiles_x * tiles_y);
    constexpr size_t lds_bytes = ((size_t)22 * 16 * ((16 * NOUT) | 1) + (size_t)16 * NOUT * CIN) * sizeof(float);   // G + the weight image
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    auto kern = upconv4x4_head<CIN, NOUT, U8>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_upconv_grid(ntiles)), dim3(256), lds_bytes, stream, d, (int)tiles_x, ntiles);
    return hipGetLastError();
}

// d.in = the NHWC view of z (in_ps = cin, in_cs = 1, 16-byte aligned pixels), d.out_h x d.out_w = the SOURCE pixels of the launch: it writes
// 2 out_h x 2 out_w output pixels per plane at d.out (out_rs = the row stride of the doubled image); d.wpk = the w2xc_upconv_pack image
hipError_t w2xc_launch_upconv(W2xcKernelKind kind, const W2xcConvDesc &d, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0) return hipSuccess;
    if (d.in_shift != 0 || d.in_ps != d.cin || d.in_cs != 1 || (d.in_rs & 3) != 0 || (((size_t)d.in) & 15) != 0) return hipErrorInvalidValue;
    if (d.in_h < 1 || d.in_w < 1) return hipErrorInvalidValue;
    const bool u8 = kind != W2XC_K_UPCONV && kind != W2XC_K_UPCONV_A;
    if (!w2xc_upconv_sink_ok(kind, d)) return hipErrorInvalidValue;
    switch (d.cin * 10 + d.cout) {
#define W2XC_UPCONV_CASE(C)                                                                                  \
    case C * 10 + 1: return u8 ? launch_upconv<C, 1, true>(d, stream) : launch_upconv<C, 1, false>(d, stream); \
    case C * 10 + 3: return u8 ? launch_upconv<C, 3, true>(d, stream) : launch_upconv<C, 3, false>(d, stream);
        W2XC_UPCONV_CASE(32)
        W2XC_UPCONV_CASE(64)
        W2XC_UPCONV_CASE(128)
        W2XC_UPCONV_CASE(256)
#undef W2XC_UPCONV_CASE
    default: return hipErrorInvalidValue;
    }
}
#endif
