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
// ... with chroma co-sited along x (CX) and / or y (CY): at luma 2k the sample C[k] itself, at 2k + 1 lerp11(C[k], C[k + 1]) -- the halo's sample below / to the right,
// clamped into the plane as the tile's loader clamps it; an axis that is centred or not subsampled is chroma_at_luma's.  Horizontally first, then vertically
template <bool SX, bool SY, bool CX, bool CY> static __device__ __forceinline__ void chroma_at_luma_sited(const float *S, int ld, float (&cu)[1 + SY][1 + SX])
{
    static_assert((SX || !CX) && (SY || !CY), "a co-sited axis is a subsampled one");
    if (!CX && !CY) { chroma_at_luma<SX, SY>(S, ld, cu); return; }
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;
    constexpr int R0 = (SY && !CY) ? -1 : 0, NR = SY ? (CY ? 2 : 3) : 1;   // the rows the vertical step needs: cy - 1 .. cy + 1, cy and cy + 1, or cy alone
    float hz[NR][1 + HX];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const float *R = S + (R0 + r) * ld;
        if (CX) { hz[r][0] = R[0]; hz[r][HX] = lerp11(R[0], R[1]); }
        else if (SX) { hz[r][0] = lerp31(R[0], R[-1]); hz[r][HX] = lerp31(R[0], R[1]); }
        else hz[r][0] = R[0];
    }
#pragma unroll
    for (int q = 0; q < 1 + HX; q++) {
        if (CY) { cu[0][q] = hz[0][q]; cu[HY][q] = lerp11(hz[0][q], hz[NR - 1][q]); }
        else if (SY) { cu[0][q] = lerp31(hz[NR / 2][q], hz[0][q]); cu[HY][q] = lerp31(hz[NR / 2][q], hz[NR - 1][q]); }
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

// ---- device: R, G, B -> chroma co-sited with luma (w2xc_rgb_to_yuv8_body.inc, w2xc_rgb_to_yuv16_body.inc) ----
// y', cb, cr of the pixel (X, Y) of a frame's float planes
static __device__ __forceinline__ YCC ycc_at(const W2xcRgbToYuv &m, const float *s, long long ps, int w, int Y, int X)
{
    const float *e = s + (long long)Y * w + X;
    return to_ycc(m, e[0], e[ps], e[2 * ps]);
}
// The horizontal pass of luma row Y for the chroma sample of lane lx of a tile that starts at chroma column cx0: p0 and p1 are the thread's pixels of that row,
// luma columns 2 cx and 2 cx + 1 (clamped).  CX: mean121 around column 2 cx; its left neighbour, column 2 cx - 1, is p1 of the lane below in the wave's 32-lane
// half -- every lane of the half calls this together --, for lane 0 a pixel converted from memory, at the plane's left edge the thread's own p0.  Centred: the mean
// of the two
template <bool CX>
static __device__ __forceinline__ void row_chroma(const W2xcRgbToYuv &m, const float *s, long long ps, int w, int Y, int cx0, int lx, const YCC &p0, const YCC &p1,
                                                  float *cb, float *cr)
{
    if (!CX) {
        *cb = (p0.cb + p1.cb) * 0.5f;
        *cr = (p0.cr + p1.cr) * 0.5f;
        return;
    }
    float lb = __shfl_up(p1.cb, 1, 32), lr = __shfl_up(p1.cr, 1, 32);
    const bool edge = lx == 0 && cx0 == 0;
    lb = edge ? p0.cb : lb;
    lr = edge ? p0.cr : lr;
    if (lx == 0 && cx0 > 0) {
        const YCC e = ycc_at(m, s, ps, w, Y, 2 * cx0 - 1);
        lb = e.cb; lr = e.cr;
    }
    *cb = mean121(lb, p0.cb, p1.cb);
    *cr = mean121(lr, p0.cr, p1.cr);
}
// ... of the luma row above a tile that starts at chroma row cy0, for the threads of tile row 0 (one 32-lane half of a wave, together): the pixels of row 2 cy0 - 1
// at the columns of chroma sample bx are converted from memory; at the plane's top edge the row clamps to the block's own first row, whose result the caller hands in
template <bool CX>
static __device__ __forceinline__ void top_row_chroma(const W2xcRgbToYuv &m, const float *s, long long ps, int w, int cx0, int cy0, int bx, int lx, float own_cb,
                                                      float own_cr, float *cb, float *cr)
{
    if (cy0 == 0) { *cb = own_cb; *cr = own_cr; return; }
    const int Y = 2 * cy0 - 1;
    const YCC p0 = ycc_at(m, s, ps, w, Y, min(2 * bx, w - 1)), p1 = ycc_at(m, s, ps, w, Y, min(2 * bx + 1, w - 1));
    row_chroma<CX>(m, s, ps, w, Y, cx0, lx, p0, p1, cb, cr);
}
