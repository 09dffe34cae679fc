// w2xc_first2_wino4.hip -- conv3x3_first2_wino4: layers 1 (ONE plane -> 32) and 2 (32 -> 32) of convertWithModelsBasic's loop
// (/root/reference/src/convertRoutine.cpp:66-76) in ONE launch: layer 1's activations never reach HBM (N3).  Layer 2 -- the 3x3 x 32 x 32
// contraction of Model::filterWorker (/root/reference/src/modelHandler.cpp:117-159) -- runs as Winograd F(4x4, 3x3) on v_mfma_f32_16x16x4_f32 with its
// weights STATIONARY IN REGISTERS; layer 1 (9 multiplies per value) is computed on the fly, per Winograd patch, from a tile of the source plane.
//
//   With 32 input planes the transformed weights of a 32-output-plane layer are 36 x 32 x 32 floats = 144 KiB = 144 registers per lane of a
//   four-wave workgroup: they are loaded ONCE per workgroup and never move again (conv3x3_wino4 streams its U through LDS for every tile: 36 KiB per
//   4-channel stage, its largest cost beside the MFMAs).  What is left per tile is what depends on the pixels.
//
//   Workgroup   4 waves, two workgroups per CU (two waves per SIMD, 256 registers each; 74 KiB of LDS each).  Wave g owns the positions
//               xi in [9 g, 9 g + 9) of the transformed domain (xi = 6 i + j) for all 32 output planes and all 32 channels:
//               U[9][2 plane tiles][8 k-steps] = 144 registers in MFMA A-fragment order (lane = 16 k + plane).
//   Tile        16 blocks of 4x4 = 8 rows x 32 pixels of output (2 x 8 blocks); persistent workgroups walk an XCD-chunked tile list in strips.
//   S           the tile's 12 x 38 source pixels into LDS: replicate padding (copyMakeBorder, convertRoutine.cpp:35,96) and the nearest-2x
//               (main.cpp:132-140, in_shift) folded into the addresses, exactly as conv3x3_first does.
//   T           per lane two patches (block, channel c) and (block, c + 16): the 6 x 6 layer-1 activations leaky(b1[c] + sum w1[c][tap] src) as a
//               bias-first fma chain in tap order over an 8 x 8 window (rolling three rows), then V = B^T d B, written to LDS in B-fragment order
//               V[xi][k-step / 4][lane = 16 k + block][k-step % 4]: wave g handles the channels = g mod 4 with a lane map of its own (conflict-free dword writes).
//   G           36 x (32 planes x 16 blocks x 32 channels) GEMMs: per wave 9 xi x 2 plane tiles x 8 k-steps = 144 MFMAs, one ds_read_b128 per
//               (xi, four k-steps); every V value is read by exactly one wave.
//   X           the accumulators change owner through LDS (over V): M[xi][plane pair][lane = 16 (plane quad) + block] as 8-byte pairs.
//   O           output transform Y = A^T M A, bias, LeakyReLU: two (plane, block) pairs per lane, stores as 16-byte pixel quads of a plane row
//               (eight lanes = one 128-byte line), spread between the arithmetic (a burst of stores costs the wave their issue and the wait for their data registers back to back; the memory pipeline's FIFOs never fill).
//   The phases of a tile run one after the other between workgroup barriers; the second workgroup of the CU is in another phase.  MFMA and VALU
//   share the SIMD's issue time on this hardware (an fp32 MFMA and a VALU instruction of two waves do not run side by side), so the kernel's
//   time is the SUM of its matrix and vector work: what fusion buys is layer 1's HBM round trip (1.07 GB written and read again) and every
//   global load of layer 2 -- measured, the unfused form of this kernel lost as much to its patch loads as it gained (profiles/r5_sweeps.log).
//   Edges       source rows / columns clamped (replicate) in the tile fill; patch columns >= layer 2's input width are zeroed (they only reach
//               outputs >= out_w), rows beyond it are layer-1 values of clamped source rows (they only reach outputs >= out_h).  Blocks sit on
//               rows = 0 mod 4 of layer 2's whole output (W2xcConvDesc::wino_py): banding-invariant on run_rows' four-rows-per-layer geometry.
// Kernels and launchers only: w2xc_first2_wino4_supported and the weight image (w2xc_first2_wino4_pack) are in w2xc_pack.cpp.
#include "w2xc_kernels.h"
#include "w2xc_device.h"
#include "w2xc_launch.hpp"
#include "w2xc_wino4_math.h"

#ifndef W4S_ABL
#define W4S_ABL 0   // timing-only ablations (wrong results): 1 no input transform arithmetic | 2 no layer-1 arithmetic | 4 no MFMAs | 8 no output transform | 16 no stores
#endif
#ifdef W4S_TIMING
// tools/ubench/first2_wino4_timing.hip: s_memtime stamps of workgroup 0, wave 0: [tile * 8 + k], k = 0 tile start, 1 source tile in LDS, 2 T done, 3 barrier, 4 G done, 5 barrier + X done, 6 barrier, 7 O done
__device__ unsigned long long w4s_stamps[4096];
#define W4S_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0 && 8 * tn + (k) < 4096) w4s_stamps[8 * tn + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define W4S_STAMP(k) do { } while (0)
#endif

// d.in / in_* / in_h / in_w / off_* / in_shift: LAYER 1's input plane (off = layer 1's offsets + layer 2's); d.w1pk / d.bias1: layer 1's W2XC_K_FIRST
// image and bias; d.wpk / d.bias / d.out* / out_h / out_w / wino_py: layer 2
#ifndef W2XC_FIRST2_BATCH
#define W2XC_FIRST2_BATCH 0   // 1: this object holds the batch form (conv3x3_first2_wino4_batch) and its launcher instead of the one-image kernel
#endif
#if !W2XC_FIRST2_BATCH
__global__ void __launch_bounds__(256, 2) conv3x3_first2_wino4(W2xcConvDesc d, int tiles_x, int ntiles)
{
#define W4B_ONLY(...)
#define W4B_SEL(b_, s_) s_
#include "w2xc_first2_wino4_body.inc"
#undef W4B_SEL
#undef W4B_ONLY
}
#else
// batch form (w2xc_convert_batch*): bd.batch images of bd.items tiles
__global__ void __launch_bounds__(256, 2) conv3x3_first2_wino4_batch(W2xcConvDesc d, int tiles_x, int ntiles, W2xcBatchDesc bd)
{
#define W4B_ONLY(...) __VA_ARGS__
#define W4B_SEL(b_, s_) b_
#include "w2xc_first2_wino4_body.inc"
#undef W4B_SEL
#undef W4B_ONLY
}
#endif

// ------------------------------------------------------------------------------------------------
// host side (w2xc_first2_wino4_supported and the packer w2xc_first2_wino4_pack: w2xc_pack.cpp)
// ------------------------------------------------------------------------------------------------
#if !W2XC_FIRST2_BATCH
// d.in .. in_shift: layer 1's one-plane input (any row stride; in_h / in_w in UPSCALED coordinates when in_shift = 1), off_y / off_x = layer 1's offsets
// plus layer 2's; d.w1pk / d.bias1 = layer 1's W2XC_K_FIRST image / bias; d.wpk = w2xc_first2_wino4_pack image, d.bias, planar fp32 out (out_ps = 1,
// 16-byte aligned rows of >= roundup4(out_w) floats), d.out_h / out_w / wino_py = layer 2's region
hipError_t w2xc_launch_first2_wino4(const W2xcConvDesc &d, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0) return hipSuccess;
    if (d.cin != 32 || d.cout != 32 || !d.w1pk || !d.bias1 || d.in_ps != 1 || d.in_shift < 0 || d.in_shift > 1 || d.out_terms != 0) return hipErrorInvalidValue;
    if (d.out_ps != 1 || (d.out_rs & 3) != 0 || (d.out_cs & 3) != 0 || (((size_t)d.out) & 15) != 0 || d.out_rs < ((d.out_w + 3) & ~3)) return hipErrorInvalidValue;
    // 32-bit lane offsets: 12 plane strides + a row of THIS launch's region + a pixel -- the largest one a lane forms, whatever the relation of the strides
    if (12ll * d.out_cs * 4 + ((long long)d.out_h + 8) * d.out_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 3) + 7) / 8;
    const int ntiles = tiles_x * tiles_y;
    constexpr size_t lds_bytes = 36 * 2 * 64 * 16 + 12 * 40 * 4 + 32 * 12 * 4;   // V (then M over it): 72 KiB; the source tile; layer 1's weights
    auto kern = conv3x3_first2_wino4;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(ntiles, 2)), dim3(256), lds_bytes, stream, d, tiles_x, ntiles);
    return hipGetLastError();
}
#endif

// the checks of w2xc_launch_first2_wino4 on the single-image descriptor d (d.out / d.in of image 0), and the image strides in floats (b.out_bs: a multiple
// of 4, every image's planes keep the 16-byte alignment of image 0's)
#if W2XC_FIRST2_BATCH
hipError_t w2xc_launch_first2_wino4_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0 || b.batch == 0) return hipSuccess;
    if (b.batch < 0 || b.in_bs < 0 || b.out_bs < 0 || (b.out_bs & 3) != 0) return hipErrorInvalidValue;
    if (d.cin != 32 || d.cout != 32 || !d.w1pk || !d.bias1 || d.in_ps != 1 || d.in_shift < 0 || d.in_shift > 1 || d.out_terms != 0) return hipErrorInvalidValue;
    if (d.out_ps != 1 || (d.out_rs & 3) != 0 || (d.out_cs & 3) != 0 || (((size_t)d.out) & 15) != 0 || d.out_rs < ((d.out_w + 3) & ~3)) return hipErrorInvalidValue;
    if (12ll * d.out_cs * 4 + ((long long)d.out_h + 8) * d.out_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 3) + 7) / 8;
    const long long items = (long long)tiles_x * tiles_y;
    if (items * b.batch >= (1ll << 31)) return hipErrorInvalidValue;
    b.items = (int)items;
    const int ntiles = (int)(items * b.batch);
    constexpr size_t lds_bytes = 36 * 2 * 64 * 16 + 12 * 40 * 4 + 32 * 12 * 4;   // V (then M over it): 72 KiB; the source tile; layer 1's weights
    auto kern = conv3x3_first2_wino4_batch;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(ntiles, 2)), dim3(256), lds_bytes, stream, d, tiles_x, ntiles, b);
    return hipGetLastError();
}
#endif
