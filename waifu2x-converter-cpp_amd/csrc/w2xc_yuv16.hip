// w2xc_yuv16.hip -- 16-bit YUV frames (include/w2xc_hip.h, "16-bit YUV frames": w2xc_process_frames_yuv_u16[_device] and their building blocks): luma words to the
// float plane the models take and back, and the 2x enlargement of chroma on words.  A word holds a value of `depth` bits (8 .. 16) in its low or its high bits.
// No colour matrix anywhere.  Built with -ffp-contract=off like w2xc_yuv.hip: every product and sum below is its own fp32 operation.
//   Y16ToPlane / PlaneToY16   two stages on the per-pixel skeleton (w2xc_px.h), batch forms
//   ChromaCopy16              chroma values as they are (a call without a 2x step), from either sample stride and packing to either
//   k_chroma2x_u16            words in, words out: Resize2xCubic (w2xc_color.hip) on (float)C * (float)(1.0 / M), then saturate(rint(c * M)), without a float plane
//                             of chroma in memory
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi
#include "w2xc_px.h"       // k_px, launch_px, row_col, cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum, u16_value, to_u16, luma_u16, u16_scale
#include "w2xc_yuv_tile.h" // the tile of the bicubic 2x, the launch grid, rows_align

// luma word -> y: full range (float)Y * (float)(1.0 / M), limited range ((float)Y - 16 s) * (float)(1.0 / (219 s)).  Frame i's plane at dst + i * ps floats
struct Y16ToPlane {
    const unsigned short *src;
    long long frame, row;
    int w, limited, rshift;
    unsigned max;
    float off, scale;
    float *dst;
    long long ps;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const float Y = (float)u16_value(src[img * frame + at.r * row + at.c], rshift, max);
        dst[img * ps + q] = limited ? (Y - off) * scale : Y * scale;
    }
};
hipError_t w2xc_launch_y16_to_plane(W2xcU16Planes src, int w, int h, int range, int depth, float *dst, long long ps, int n, hipStream_t st)
{
    if (depth < 8 || depth > 16 || !src.p || !dst || w < 1 || h < 1 || n < 1) return hipErrorInvalidValue;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    return launch_px(Y16ToPlane{src.p, src.frame, src.row, w, range != 0, src.pack ? 16 - depth : 0, (unsigned)k.max, k.y_off, k.y_in, dst, ps}, (long long)w * h, n, st);
}

// y -> luma word: saturate(rint(y * M)), or saturate(rint(y * (219 s) + 16 s)) for limited range, half to even, the product and the sum unfused
struct PlaneToY16 {
    const float *src;
    long long ps;
    int w, limited, lshift, max;
    float scale, off;
    unsigned short *dst;
    long long frame, row;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const float y = src[img * ps + q];
        dst[img * frame + at.r * row + at.c] = (unsigned short)(luma_u16(y, limited, scale, off, max) << lshift);
    }
};
hipError_t w2xc_launch_plane_to_y16(const float *src, long long ps, int w, int h, int range, int depth, W2xcU16Planes dst, int n, hipStream_t st)
{
    if (depth < 8 || depth > 16 || !src || !dst.p || w < 1 || h < 1 || n < 1) return hipErrorInvalidValue;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    return launch_px(PlaneToY16{src, ps, w, range != 0, dst.pack ? 16 - depth : 0, k.max, k.y_out, k.y_off, dst.p, dst.frame, dst.row}, (long long)w * h, n, st);
}

// plane p of the launch: npl planes per frame (U, or U and V), frame p / npl; the value is repacked where the two sides differ in packing
struct ChromaCopy16 {
    const unsigned short *su, *sv;
    long long sframe, srow;
    int spx, cw, npl, rshift;
    unsigned max;
    unsigned short *du, *dv;
    long long dframe, drow;
    int dpx, lshift;
    __device__ __forceinline__ void operator()(int p, long long q) const
    {
        const RowCol at = row_col(q, cw);
        const int f = p / npl, v = p - f * npl;
        const unsigned c = u16_value((v ? sv : su)[f * sframe + at.r * srow + (long long)at.c * spx], rshift, max);
        (v ? dv : du)[f * dframe + at.r * drow + (long long)at.c * dpx] = (unsigned short)(c << lshift);
    }
};
hipError_t w2xc_launch_chroma_copy_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int depth, int n, hipStream_t st)
{
    if (depth < 8 || depth > 16 || !su.p || !du.p || (sv != nullptr) != (dv != nullptr) || cw < 1 || ch < 1 || n < 1) return hipErrorInvalidValue;
    const int npl = sv ? 2 : 1;
    return launch_px(ChromaCopy16{su.p, sv, su.frame, su.row, su.px, cw, npl, su.pack ? 16 - depth : 0, (1u << depth) - 1u, du.p, dv, du.frame, du.row, du.px,
                                  du.pack ? 16 - depth : 0},
                     (long long)cw * ch, n * npl, st);
}

// ---- the bicubic 2x of chroma, words to words ----
// The quads, the tile of CH_TQX x CH_TQY quads and its source pixels in LDS as floats are those of k_chroma2x_u8 (w2xc_yuv.hip), rows of CH_LD words: a wave's
// 32-lane halves read 32 consecutive words of a row.  A TURN here is one tile of ALL planes of one frame (npl = 1: U alone, 2: U and V), each plane's source
// tile in its own LDS array: a thread then holds the U and the V of its samples, and where the output interleaves them it stores both as one dword.
// LOAD 1: planar planes (spx = 1) whose rows start on 8-byte boundaries: an aligned group of four source samples inside the row is ONE 8-byte load by one thread.
// LOAD 2: interleaved planes, sv = su + 1 (P010), rows on 4-byte boundaries: ONE 4-byte load per LDS position fetches the sample's (U, V) pair for both tiles.
// LOAD 0: sample by sample (the clamped rim of LOAD 1 too).
// Stores: a thread writes only its own samples, as 16-bit stores, or -- pair: du and dv interleave as dv = du + 1 and the rows start on 4-byte boundaries -- its
// (U, V) pair as ONE 32-bit store.  Never a read-modify-write of a word that is another thread's or another plane's.
template <int LOAD>
__global__ void __launch_bounds__(256) k_chroma2x_u16(const unsigned short *su, const unsigned short *sv, long long sframe, long long srow, int spx, int cw, int ch,
                                                      int rshift, int max, unsigned short *du, unsigned short *dv, long long dframe, long long drow, int dpx,
                                                      int lshift, int pair, int ow, int oh, int npl, float inv_max, float fmax, int tiles_x, long long tiles,
                                                      long long turns)
{
    __shared__ float tile[2][CH_SH * CH_LD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    float c25[4], c75[4];
    cubic_coeffs(0.25f, c25);
    cubic_coeffs(0.75f, c75);
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of the planes of one frame
        const long long f = turn / tiles, t = turn - f * tiles;
        const int qy0 = (int)(t / tiles_x) * CH_TQY, qx0 = (int)(t % tiles_x) * CH_TQX;
        const int gx0 = qx0 - 2, gy0 = qy0 - 2;   // the source pixel of LDS word (0, 0)
        __syncthreads();   // (the tiles of the loop's previous turn have been read)
        if (LOAD == 2) {
            const unsigned short *s = su + f * sframe;
            for (int i = threadIdx.x; i < CH_SH * CH_SW; i += 256) {
                const int r = i / CH_SW, c = i - r * CH_SW;
                const unsigned w2 = *reinterpret_cast<const unsigned *>(s + clampi(gy0 + r, 0, ch - 1) * srow + (long long)clampi(gx0 + c, 0, cw - 1) * 2);
                tile[0][r * CH_LD + c] = (float)u16_value(w2 & 0xFFFFu, rshift, max) * inv_max;
                tile[1][r * CH_LD + c] = (float)u16_value(w2 >> 16, rshift, max) * inv_max;
            }
        } else {
            for (int v = 0; v < npl; v++) {
                const unsigned short *s = (v ? sv : su) + f * sframe;
                float *T = tile[v];
                if (LOAD == 1) {
                    // column groups of four source pixels from gx0 - 2 (a multiple of 4) on: ten cover the CH_SW columns
                    for (int i = threadIdx.x; i < CH_SH * 10; i += 256) {
                        const int r = i / 10, g = i - r * 10;
                        const int gx4 = gx0 - 2 + 4 * g;
                        const unsigned short *row = s + clampi(gy0 + r, 0, ch - 1) * srow;
                        unsigned b[4];
                        if (gx4 >= 0 && gx4 + 3 < cw) {
                            const uint2 w4 = *reinterpret_cast<const uint2 *>(row + gx4);
                            b[0] = w4.x & 0xFFFFu; b[1] = w4.x >> 16; b[2] = w4.y & 0xFFFFu; b[3] = w4.y >> 16;
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; k++) b[k] = row[clampi(gx4 + k, 0, cw - 1)];
                        }
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int c = 4 * g - 2 + k;
                            if (c >= 0 && c < CH_SW) T[r * CH_LD + c] = (float)u16_value(b[k], rshift, max) * inv_max;
                        }
                    }
                } else {
                    for (int i = threadIdx.x; i < CH_SH * CH_SW; i += 256) {
                        const int r = i / CH_SW, c = i - r * CH_SW;
                        T[r * CH_LD + c] = (float)u16_value(s[clampi(gy0 + r, 0, ch - 1) * srow + (long long)clampi(gx0 + c, 0, cw - 1) * spx], rshift, max) * inv_max;
                    }
                }
            }
        }
        __syncthreads();
        const int qx = qx0 + lx, X0 = 2 * qx - 1;   // the quad's columns X0 (t = 0.25) and X0 + 1 (t = 0.75)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int qr = ly + j * (CH_TQY / 2), Y0 = 2 * (qy0 + qr) - 1;   // rows Y0 (t = 0.25) and Y0 + 1 (t = 0.75)
            if (X0 >= ow || Y0 >= oh) continue;
            unsigned o[2][4] = {};   // per plane: (Y0, X0), (Y0, X0 + 1), (Y0 + 1, X0), (Y0 + 1, X0 + 1), packed words
#pragma unroll
            for (int v = 0; v < 2; v++) {
                if (v >= npl) continue;
                float r25[4], r75[4];   // the horizontal pass of the four rows, for either column
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float *S = tile[v] + (qr + k) * CH_LD + lx;
                    r25[k] = chroma_row_sum(S, c25);
                    r75[k] = chroma_row_sum(S, c75);
                }
                o[v][0] = to_u16(chroma_row_sum(r25, c25), fmax, max) << lshift;
                o[v][1] = to_u16(chroma_row_sum(r75, c25), fmax, max) << lshift;
                o[v][2] = to_u16(chroma_row_sum(r25, c75), fmax, max) << lshift;
                o[v][3] = to_u16(chroma_row_sum(r75, c75), fmax, max) << lshift;
            }
            const long long at = f * dframe + Y0 * drow + (long long)X0 * dpx;
            const bool ok[4] = {Y0 >= 0 && X0 >= 0, Y0 >= 0 && X0 + 1 < ow, Y0 + 1 < oh && X0 >= 0, Y0 + 1 < oh && X0 + 1 < ow};
            const long long off[4] = {0, dpx, drow, drow + dpx};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!ok[k]) continue;
                if (pair) *reinterpret_cast<unsigned *>(du + at + off[k]) = o[0][k] | (o[1][k] << 16);
                else {
                    du[at + off[k]] = (unsigned short)o[0][k];
                    if (npl == 2) dv[at + off[k]] = (unsigned short)o[1][k];
                }
            }
        }
    }
}

hipError_t w2xc_launch_chroma2x_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int ow, int oh, int depth, int n,
                                    hipStream_t st)
{
    if (cw < 1 || ch < 1 || ow < 1 || oh < 1 || ow > 2 * (long long)cw || oh > 2 * (long long)ch || n < 1 || (su.px != 1 && su.px != 2) || (du.px != 1 && du.px != 2) ||
        !su.p || !du.p || (sv != nullptr) != (dv != nullptr) || depth < 8 || depth > 16)
        return hipErrorInvalidValue;
    const int npl = sv ? 2 : 1;
    const YuvTileGrid g = w2xc_eng::chroma2x_tile_grid(ow, oh, n, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX);   // a turn: one tile of ALL planes of a frame
    const size_t salign = rows_align(su, n), dalign = rows_align(du, n);
    int load = 0;
    if (su.px == 1 && ((salign | (sv ? reinterpret_cast<size_t>(sv) : 0)) & 7) == 0) load = 1;
    else if (su.px == 2 && sv == su.p + 1 && (salign & 3) == 0) load = 2;
    const int pair = du.px == 2 && dv == du.p + 1 && (dalign & 3) == 0;
    const W2xcU16Scale k = u16_scale(depth, 0);
    const int rshift = su.pack ? 16 - depth : 0, lshift = du.pack ? 16 - depth : 0;
    const auto kernel = load == 2 ? k_chroma2x_u16<2> : load == 1 ? k_chroma2x_u16<1> : k_chroma2x_u16<0>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, su.p, sv, su.frame, su.row, su.px, cw, ch, rshift, k.max, du.p, dv, du.frame, du.row, du.px, lshift, pair,
                       ow, oh, npl, k.inv_max, k.fmax, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
