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
#include "w2xc_kernels.h"
#include "w2xc_device.h"
#include "w2xc_launch.hpp"

// U8 (W2XC_K_UPCONV_U8): the sink is an interleaved uint8 image as for conv3x3_last<U8> -- d.out points at bytes, out_rs / out_ps / out_cs are byte
// strides (row stride, NOUT, 1) -- and the epilogue stores saturate(rint(255 v)), one byte store per value.
template <int CIN, int NOUT, bool U8>
__global__ void __launch_bounds__(256) upconv4x4_head(W2xcConvDesc d, int tiles_x, int ntiles)
{
    constexpr int ROWS = 8, HW = 34, HH = ROWS + 2, NPIX = HH * HW;
    constexpr int NBLK = (NPIX + 15) / 16;
    constexpr int N = 16 * NOUT, NB16 = NOUT;
    constexpr int GS = N | 1;                  // odd LDS row stride
    constexpr int S4 = CIN / 16;
    extern __shared__ float lds[];
    float *G = lds;                            // [NBLK * 16][GS]
    float *Wl = lds + NBLK * 16 * GS;          // [S4 * 4][NB16][64]: the weight image as packed

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kk = lane >> 4, i = lane & 15;

    for (int e = threadIdx.x; e < S4 * 4 * NB16 * 64; e += 256) Wl[e] = d.wpk[e];
    float bo[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; o++) bo[o] = d.bias[o];
    __syncthreads();

    // the 16 channels-of-four of pixel block `blk` of tile `tile` (clamped: only pixels of the tile's overhang, which no kept output reads, ever clamp)
    auto blk_load = [&](int tile, int blk, f32x4 (&v)[S4]) {
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        int q = blk * 16 + i;
        q = q < NPIX ? q : NPIX - 1;
        const int py = q / HW, px = q - py * HW;
        const int gy = clampi(tile_y * ROWS + py + d.off_y, 0, d.in_h - 1);
        const int gx = clampi(tile_x * 32 + px + d.off_x, 0, d.in_w - 1);
        const f32x4 *src = reinterpret_cast<const f32x4 *>(d.in + (long long)gy * d.in_rs + (long long)gx * CIN) + kk;
#pragma unroll
        for (int s4 = 0; s4 < S4; s4++) v[s4] = src[s4 * 4];
    };

    // this workgroup's run of consecutive tiles; runs that follow each other share an XCD (their tiles share halo pixels in its L2)
    const int nwg = gridDim.x, per = (ntiles + nwg - 1) / nwg;
    const int tile_first = xcd_remap(blockIdx.x, nwg) * per;
    const int tile_end = tile_first + per < ntiles ? tile_first + per : ntiles;
    f32x4 av[S4];
    if (tile_first < tile_end) blk_load(tile_first, wave, av);
    for (int tile = tile_first; tile < tile_end; tile++) {
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const int oy0 = tile_y * ROWS, ox0 = tile_x * 32;
        for (int blk = wave; blk < NBLK; blk += 4) {
            // the next block's loads (this tile's, or the first of the next tile) fly under this block's MFMAs
            f32x4 nv[S4];
            const bool more = blk + 4 < NBLK;
            const bool next_tile = !more && tile + 1 < tile_end;
            if (more) blk_load(tile, blk + 4, nv);
            else if (next_tile) blk_load(tile + 1, wave, nv);
            f32x4 acc[NB16];
#pragma unroll
            for (int nb = 0; nb < NB16; nb++) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s4 = 0; s4 < S4; s4++)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int nb = 0; nb < NB16; nb++)
                        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4][j], Wl[((s4 * 4 + j) * NB16 + nb) * 64 + lane], acc[nb], 0, 0, 0);
            // C/D map of the 16x16 MFMA: column = lane & 15 (n), row = 4 (lane >> 4) + r (pixel in block)
#pragma unroll
            for (int nb = 0; nb < NB16; nb++)
#pragma unroll
                for (int r = 0; r < 4; r++) G[(blk * 16 + kk * 4 + r) * GS + nb * 16 + i] = acc[nb][r];
            if (more || next_tile) {
#pragma unroll
                for (int s4 = 0; s4 < S4; s4++) av[s4] = nv[s4];
            }
        }
        __syncthreads();

        for (int p = threadIdx.x; p < 2 * ROWS * 64; p += 256) {
            const int yl = p >> 6, xl = p & 63;
            const int iy = yl >> 1, py = yl & 1, ix = xl >> 1, px = xl & 1;
            const int y = oy0 + iy, x = ox0 + ix;
            if (y >= d.out_h || x >= d.out_w) continue;
#pragma unroll
            for (int o = 0; o < NOUT; o++) {
                float v = 0.0f;
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const int r = 1 - py + 2 * a, s = 1 - px + 2 * b;
                        const int zy = iy + ((py + 3 - r) >> 1), zx = ix + ((px + 3 - s) >> 1);
                        v += G[(zy * HW + zx) * GS + (4 * r + s) * NOUT + o];
                    }
                v += bo[o];
                const long long at = (long long)o * d.out_cs + (long long)(2 * y + py) * d.out_rs + (long long)(2 * x + px) * d.out_ps;
                if constexpr (U8) reinterpret_cast<unsigned char *>(d.out)[at] = (unsigned char)clampi(__float2int_rn(v * 255.0f), 0, 255);
                else d.out[at] = v;
            }
        }
        __syncthreads();                                 // (G is rewritten by the next tile)
    }
}

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
    const bool u8 = kind == W2XC_K_UPCONV_U8;
    if (u8 ? (d.cout != 3 || d.out_ps != 3 || d.out_cs != 1) : d.out_ps != 1) return hipErrorInvalidValue;
    switch (d.cin * 10 + d.cout) {
#define W2XC_UPCONV_CASE(C)                                                                                  \
    case C * 10 + 1: return u8 ? hipErrorInvalidValue : launch_upconv<C, 1, false>(d, stream);              \
    case C * 10 + 3: return u8 ? launch_upconv<C, 3, true>(d, stream) : launch_upconv<C, 3, false>(d, stream);
        W2XC_UPCONV_CASE(32)
        W2XC_UPCONV_CASE(64)
        W2XC_UPCONV_CASE(128)
        W2XC_UPCONV_CASE(256)
#undef W2XC_UPCONV_CASE
    default: return hipErrorInvalidValue;
    }
}
