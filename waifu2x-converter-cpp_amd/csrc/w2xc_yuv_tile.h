// w2xc_yuv_tile.h -- what the six tile kernels of the YUV frame calls share across the two sample widths (k_chroma2x_u8 / _u16 in w2xc_yuv.hip / w2xc_yuv16.hip,
// k_yuv8_to_rgb / k_yuv16_to_rgb and k_rgb_to_yuv8 / k_rgb_to_yuv16 in w2xc_yuv_rgb.hip / w2xc_yuv16_rgb.hip): ONE definition each of the tile geometry, the
// launch grid, and in the four kernels of the RGB route a turn's tile and what a thread does between its tile in LDS (or its block of float planes) and the
// values it rounds -- the 16-bit arithmetic IS the 8-bit arithmetic on other constants.  Per width, in the kernels' own files: the loaders, the LDS layout of
// luma, the roundings and the stores.
// Four pieces that both widths also have stay written out in the kernels, where they cost nothing: the row store of the to-RGB kernels, the load of a block into
// YCC p[][], and the tile decode, taps and two passes of the bicubic 2x -- as functions here the first three took registers above the parent's, and the taps
// and the horizontal pass changed the code of every k_chroma2x instantiation, one of them measurably (profiles/yuv_shared_isa_compare.txt, yuv_shared_bench.json).
// Every file that includes it is built with -ffp-contract=off.
#pragma once
#include "w2xc_kernels.h"
#include "w2xc_host_geom.hpp"   // YuvTileGrid and the two grid rules
#include "w2xc_yuv_px.h"   // lerp31, clamp01, YCC

// ---- the tile of the bicubic 2x: CH_TQX x CH_TQY quads, their source pixels in LDS as floats, rows of CH_LD words ----
#define CH_TQX W2XC_CHROMA_TQX
#define CH_TQY W2XC_CHROMA_TQY
#define CH_SW (CH_TQX + 3)
#define CH_SH (CH_TQY + 3)
#define CH_LD (CH_SW + 2)
static_assert(CH_TQX == 32 && CH_TQY == 16 && (CH_LD & 1) == 1 && CH_SW <= CH_LD, "256 threads = 32 x 8 quads, two quad rows per thread");

// ---- the tile of the RGB route: YR_TCX x YR_TCY chroma samples (YR_YLD, the LDS row of luma, is each file's own: bytes or words) ----
#define YR_TCX W2XC_YUVRGB_TCX
#define YR_TCY W2XC_YUVRGB_TCY
#define YR_LD (YR_TCX + 3)          // words per LDS row of chroma: the tile, a halo sample at either side, one word of padding -- an odd count
static_assert(YR_TCX == 32 && YR_TCY == 16 && (YR_LD & 1) == 1, "256 threads = 32 x 8 chroma samples, two rows per thread");

// ---- host ----
// (The launch grid is plain integers and lives in w2xc_host_geom.hpp -- chroma2x_tile_grid, yuv_rgb_tile_grid --, where tests/cpp/host_geom_test.cpp checks it.)
using w2xc_eng::YuvTileGrid;
// the byte alignment every row of a plane of n frames shares (W2xcU8Planes, W2xcU16Planes: strides in samples)
template <class Planes> static inline size_t rows_align(const Planes &p, int n)
{
    return reinterpret_cast<size_t>(p.p) | (size_t)p.row * sizeof(*p.p) | (n > 1 ? (size_t)p.frame * sizeof(*p.p) : 0);
}

// ---- device: a turn's frame, returned, and the first chroma sample of its tile ----
static __device__ __forceinline__ long long yuv_tile_at(long long turn, long long tiles, int tiles_x, int tx, int ty, int *x0, int *y0)
{
    const long long f = turn / tiles, t = turn - f * tiles;
    *y0 = (int)(t / tiles_x) * ty;
    *x0 = (int)(t % tiles_x) * tx;
    return f;
}

// ---- device: samples -> R, G, B ----
// A thread's U or V at the luma samples of its block, from S = its own sample in an LDS tile of rows of ld words with a halo along each subsampled axis:
// horizontally first, on the rows the vertical step needs, then vertically on the two row results
template <bool SX, bool SY> static __device__ __forceinline__ void chroma_at_luma(const float *S, int ld, float (&cu)[1 + SY][1 + SX])
{
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;
    float hz[1 + 2 * HY][1 + HX];   // rows cy - 1, cy, cy + 1 (SY) or cy alone
#pragma unroll
    for (int r = 0; r < 1 + 2 * HY; r++) {
        const float *R = S + (r - HY) * ld;
        if (SX) { hz[r][0] = lerp31(R[0], R[-1]); hz[r][HX] = lerp31(R[0], R[1]); }
        else hz[r][0] = R[0];
    }
#pragma unroll
    for (int q = 0; q < 1 + HX; q++) {
        if (SY) { cu[0][q] = lerp31(hz[HY][q], hz[0][q]); cu[HY][q] = lerp31(hz[HY][q], hz[2 * HY][q]); }
        else cu[0][q] = hz[0][q];
    }
}
// pixel q of a row from y', cb, cr: the matrix, the clamp to the models' domain
template <int N> static __device__ __forceinline__ void rgb_px(const W2xcYuvToRgb &m, float y, float cb, float cr, float (&px)[3][N], int q)
{
    const float R = y + m.cRV * cr;
    const float B = y + m.cBU * cb;
    const float G = (y - m.cGU * cb) - m.cGV * cr;
    px[0][q] = clamp01(R);
    px[1][q] = clamp01(G);
    px[2][q] = clamp01(B);
}

// ---- device: R, G, B -> y', cb, cr of a thread's block ----
// the box mean of cb and of cr over the block
template <bool SX, bool SY> static __device__ __forceinline__ void chroma_mean(const YCC (&p)[1 + SY][1 + SX], float *cb, float *cr)
{
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;
    if (SX && SY) {
        *cb = ((p[0][0].cb + p[0][HX].cb) + (p[HY][0].cb + p[HY][HX].cb)) * 0.25f;
        *cr = ((p[0][0].cr + p[0][HX].cr) + (p[HY][0].cr + p[HY][HX].cr)) * 0.25f;
    } else if (SX) {
        *cb = (p[0][0].cb + p[0][HX].cb) * 0.5f;
        *cr = (p[0][0].cr + p[0][HX].cr) * 0.5f;
    } else { *cb = p[0][0].cb; *cr = p[0][0].cr; }
}
