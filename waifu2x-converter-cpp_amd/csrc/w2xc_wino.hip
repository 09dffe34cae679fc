// w2xc_wino.hip -- conv3x3_wino: the 3x3 x Cin x Cout contraction of Model::filterWorker
// (/root/reference/src/modelHandler.cpp:117-159) as Winograd F(2x2, 3x3) on the fp32 MFMA of gfx950.
//
// CDNA4's fp32 MFMA runs at the fp32 VECTOR rate (157 TFLOP/s): layers 2..6 of the 7-layer model are bound by it and
// conv3x3_mfma2 already holds 92 % of it.  What is left is doing fewer multiplies: for a 2x2 block of outputs
//
//     Y = A^T [ (G g G^T) (.) (B^T d B) ] A            g = 3x3 taps, d = 4x4 input patch, (.) = element-wise
//
// needs 16 multiplies per (output plane, input plane) instead of 36 -- 2.25x fewer MFMAs -- and everything else is
// additions in fp32 (all transform coefficients are 0, +-1, +-1/2: exact), so this is still fp32 arithmetic with a
// different summation order (measured against the CPU oracle in tests/: same 1e-4 gate as conv3x3_mfma2).
// The 16 "positions" xi of the transformed domain are 16 independent GEMMs  M_xi[o][t] = sum_c U_xi[o][c] V_xi[c][t]
// (t = 2x2 output block), each on v_mfma_f32_32x32x2_f32 with U = weights as the A operand and V as the B operand:
// lane (t, kk) TRANSFORMS ITS OWN PATCH in registers (32 additions per 16 MFMAs) -- V never exists in memory --
// and owns the 16 x 16 accumulators of its block column (256 AGPRs, all of them).
//
//   Workgroup  4 waves (one per SIMD, 512 registers), persistent, one per CU.  Work item = (16 rows x 32 pixels of output,
//              one block of 32 output planes); the Cout/32 items of a pixel tile are neighbours in the list, so they
//              run at the same time on CUs of one XCD and share the input tile in that XCD's L2.
//   Wave w     rows 4w .. 4w+3 of the tile = 2 x 16 blocks of 2x2 = the 32 columns of its MFMAs.
//   Stage      one 16-channel slice of the input: lane half kk works on channels 8kk .. 8kk+7 of the slice, two per
//              k-group (one ds_read_b64 per patch pixel), 8 steps of 16 MFMAs (one per xi) = 128 MFMAs = 8192 cycles.
//   LDS        A[2] x 40 KiB: the 18 x 34 pixel halo tile of a slice, 64 B per pixel, by LDS-DMA.  Pixels of a row are
//              stored even columns first, then odd ones, and the four 16-byte chunks of a pixel are XOR-swizzled with
//              bits 2..3 of the pixel index, so the 32 lanes that read patch element (r, c) of horizontally adjacent
//              blocks (2 pixels apart) spread over the banks.
//              B[2] x 32 KiB: U of one (plane block, slice) in fragment order [k-group][step][xi/4][lane][xi%4].
//              + 10 KiB: the per-lane source offsets of the 10 tile pieces a wave transfers per slice (registers are the scarce
//              resource: 256 accumulators + ~200 VGPRs), + the bias vector.
//   Epilogue   output transform (24 additions per plane), bias, LeakyReLU, 16-byte NHWC stores.
//   Banding    the 2x2 blocks sit on EVEN rows of the layer's whole output (W2xcConvDesc::wino_py): results do not depend on the band origin.
// Measured (round 2, 2160x3840, profiles/): 128->128 10.4 ms vs 16.9 ms for conv3x3_mfma2 -- 235 TFLOP/s of algorithmic FLOPs, 1.5x the
// MFMA roofline of a direct convolution, 2/3 of the MFMA peak on the multiplies it really issues; what the rest is, DESIGN.md 3.
// Kernel and launcher only: w2xc_wino_supported and the weight image (w2xc_wino_pack) are in w2xc_pack.cpp.
#include "w2xc_kernels.h"
#include "w2xc_device.h"
#include "w2xc_launch.hpp"

#include <type_traits>

typedef float f32x2v __attribute__((ext_vector_type(2)));

// Two objects (make -j): the single-image instantiations, and -- W2XC_WINO_BATCH -- the batch forms
#ifndef W2XC_WINO_BATCH
template <int CIN, int COUT>
__global__ void __launch_bounds__(256, 1) conv3x3_wino(W2xcConvDesc d, int tiles_x, int nitems)
{
#define WNB_ONLY(...)
#define WNB_SEL(b_, s_) s_
#define WNB_OUT d.out
#include "w2xc_wino_body.inc"
#undef WNB_OUT
#undef WNB_SEL
#undef WNB_ONLY
}

// ------------------------------------------------------------------------------------------------
// host side (w2xc_wino_supported and the packer w2xc_wino_pack: w2xc_pack.cpp)
// ------------------------------------------------------------------------------------------------
template <int CIN, int COUT>
static hipError_t launch_wino(const W2xcConvDesc &d, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 1) + 15) / 16;
    const int nitems = tiles_x * tiles_y * (COUT / 32);
    constexpr size_t lds_bytes = 2 * (size_t)(4 * 10 * 1024) + 2 * (size_t)(32 * 1024) + 10 * 1024 + COUT * 4;   // tile + U ring + the DMA offset table + bias
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    auto kern = conv3x3_wino<CIN, COUT>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(nitems)), dim3(256), lds_bytes, stream, d, tiles_x, nitems);
    return hipGetLastError();
}

// d.wpk = w2xc_wino_pack image; NHWC fp32 in / out like W2XC_K_MFMA
hipError_t w2xc_launch_wino(const W2xcConvDesc &d, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0) return hipSuccess;
    if (d.in_ps != d.cin || d.in_cs != 1 || d.out_ps != d.cout || d.out_cs != 1 || d.in_shift != 0) return hipErrorInvalidValue;
    if ((d.in_rs & 3) != 0 || (d.out_rs & 3) != 0) return hipErrorInvalidValue;   // 16-byte accesses
    switch (d.cin * 1000 + d.cout) {
    case 32032:  return launch_wino<32, 32>(d, stream);
    case 32064:  return launch_wino<32, 64>(d, stream);
    case 32128:  return launch_wino<32, 128>(d, stream);
    case 64032:  return launch_wino<64, 32>(d, stream);
    case 128032: return launch_wino<128, 32>(d, stream);
    case 64064:  return launch_wino<64, 64>(d, stream);
    case 64128:  return launch_wino<64, 128>(d, stream);
    case 128064: return launch_wino<128, 64>(d, stream);
    case 128128: return launch_wino<128, 128>(d, stream);
    default: return hipErrorInvalidValue;
    }
}

#else   // W2XC_WINO_BATCH
// batch form (w2xc_convert_planes_batch_device, the batched image calls): NHWC in and out, bd.batch images of bd.items items
template <int CIN, int COUT>
__global__ void __launch_bounds__(256, 1) conv3x3_wino_batch(W2xcConvDesc d, int tiles_x, int nitems, W2xcBatchDesc bd)
{
#define WNB_ONLY(...) __VA_ARGS__
#define WNB_SEL(b_, s_) b_
#define WNB_OUT (d.out + (long long)(item / bd.items) * bd.out_bs)
#include "w2xc_wino_body.inc"
#undef WNB_OUT
#undef WNB_SEL
#undef WNB_ONLY
}

template <int CIN, int COUT>
static hipError_t launch_wino_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 1) + 15) / 16;
    const long long items = (long long)tiles_x * tiles_y * (COUT / 32);
    if (items * b.batch >= (1ll << 31)) return hipErrorInvalidValue;
    b.items = (int)items;
    const int nitems = (int)(items * b.batch);
    constexpr size_t lds_bytes = 2 * (size_t)(4 * 10 * 1024) + 2 * (size_t)(32 * 1024) + 10 * 1024 + COUT * 4;   // tile + U ring + the DMA offset table + bias
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    auto kern = conv3x3_wino_batch<CIN, COUT>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(nitems)), dim3(256), lds_bytes, stream, d, tiles_x, nitems, b);
    return hipGetLastError();
}

// d = the single-image descriptor (the checks of w2xc_launch_wino apply to it unchanged), b.in_bs / b.out_bs = image strides in floats (multiples of 4:
// every image's pixels keep the 16-byte alignment of image 0's); the shapes w2xc_wino_batch_supported names
hipError_t w2xc_launch_wino_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0 || b.batch == 0) return hipSuccess;
    if (b.batch < 0 || b.in_bs < 0 || b.out_bs < 0 || (b.in_bs & 3) != 0 || (b.out_bs & 3) != 0) return hipErrorInvalidValue;
    if (d.in_ps != d.cin || d.in_cs != 1 || d.out_ps != d.cout || d.out_cs != 1 || d.in_shift != 0) return hipErrorInvalidValue;
    if ((d.in_rs & 3) != 0 || (d.out_rs & 3) != 0) return hipErrorInvalidValue;   // 16-byte accesses
    if (!w2xc_wino_batch_supported(d.cin, d.cout)) return hipErrorInvalidValue;
    switch (d.cin * 1000 + d.cout) {
    case 32032:  return launch_wino_batch<32, 32>(d, b, stream);
    case 64032:  return launch_wino_batch<64, 32>(d, b, stream);
    case 128032: return launch_wino_batch<128, 32>(d, b, stream);
    default: return hipErrorInvalidValue;
    }
}
#endif   // W2XC_WINO_BATCH
