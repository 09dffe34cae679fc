// w2xc_yuv16_sized.hip -- chroma words of a SIZED frame call (include/w2xc_hip.h, "Sized YUV frames": w2xc_chroma_resize_u16_device and the Y route of
// w2xc_process_frames_yuv_u16_sized*): k_chroma_resize_u8 (w2xc_yuv_sized.hip: the positions, the window, its origin, the two passes) on 16-bit words.
// Built with -ffp-contract=off like w2xc_yuv16.hip.  An object of its own: the instantiations of w2xc_yuv16.o and w2xc_yuv16_sited.o stay what they are.
//   k_chroma_resize_u16<LOAD>   c = (float)C * (float)(1.0 / M), the bicubic at pos = (m + o) * r - o per axis, clamp(rint(c * M), 0, M)
// A turn is a tile of CR_TX x CR_TY OUTPUT samples of ALL planes of one frame (npl = 1: U alone, 2: U and V), each plane's source window in its own LDS array, as
// in k_chroma2x_u16: a thread holds the U and the V of its samples and, where the output interleaves them, stores both as one dword.
// Loaders and stores are k_chroma2x_u16's: LOAD 1 (planar rows on 8-byte boundaries) one 8-byte load per aligned group of four source samples inside the row;
// LOAD 2 (sv = su + 1, rows on 4-byte boundaries: P010) one 4-byte load per LDS position for the (U, V) pair; LOAD 0 sample by sample.  A thread writes only its
// own samples, as 16-bit stores or -- pair -- its (U, V) pair as ONE 32-bit store; never a read-modify-write.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi
#include "w2xc_px.h"       // cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum, u16_value, to_u16, u16_scale
#include "w2xc_yuv_tile.h" // CH_SW, CH_SH, CH_LD; w2xc_host_geom.hpp: chroma_resize_pos / _floor / _origin, chroma_resize_tile_grid
#include "w2xc_yuv_launch.h" // chroma_prologue_u16: the checks, load paths, pair store, shifts and scales of the 2x launcher

#define CR_TX W2XC_CHROMA_RESIZE_TX
#define CR_TY W2XC_CHROMA_RESIZE_TY
static_assert(CR_TX == 32 && CR_TY == 16 && CR_TX + 3 == CH_SW && CR_TY + 3 == CH_SH, "256 threads = 32 columns x 8 rows, two rows per thread; the 2x kernels' window");

using w2xc_eng::chroma_resize_floor;
using w2xc_eng::chroma_resize_origin;
using w2xc_eng::chroma_resize_pos;

template <int LOAD>
__global__ void __launch_bounds__(256) k_chroma_resize_u16(const unsigned short *su, const unsigned short *sv, long long sframe, long long srow, int spx, int cw, int ch,
                                                           int rshift, int max, unsigned short *du, unsigned short *dv, long long dframe, long long drow, int dpx,
                                                           int lshift, int pair, int ow, int oh, int npl, float inv_max, float fmax, double rx, double ox, double ry,
                                                           double oy, int tiles_x, long long tiles, long long turns)
{
    __shared__ float tile[2][CH_SH * CH_LD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of the planes of one frame
        const long long f = turn / tiles, t = turn - f * tiles;
        const int y0 = (int)(t / tiles_x) * CR_TY, x0 = (int)(t % tiles_x) * CR_TX;
        const int gx0 = chroma_resize_origin(x0, rx, ox), gy0 = chroma_resize_origin(y0, ry, oy);   // the source sample of LDS word (0, 0)
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
                    // column groups of four source samples from the multiple of 4 at or below gx0 on: ten cover the CH_SW columns
                    const int ga = gx0 & ~3, off = gx0 - ga;
                    for (int i = threadIdx.x; i < CH_SH * 10; i += 256) {
                        const int r = i / 10, g = i - r * 10;
                        const int gx4 = ga + 4 * g;
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
                            const int c = 4 * g - off + k;
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
        // the thread's column: its position, its four coefficients, and the LDS column of its first tap
        const int X = x0 + lx;
        const double px = chroma_resize_pos(X, rx, ox);
        const int sx = chroma_resize_floor(px);
        float cx[4];
        cubic_coeffs((float)(px - (double)sx), cx);
        const int c0 = sx - 1 - gx0;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int Y = y0 + ly + j * (CR_TY / 2);
            if (X >= ow || Y >= oh) continue;
            const double py = chroma_resize_pos(Y, ry, oy);
            const int sy = chroma_resize_floor(py);
            float cy[4];
            cubic_coeffs((float)(py - (double)sy), cy);
            const int at0 = (sy - 1 - gy0) * CH_LD + c0;
            unsigned o[2] = {};   // per plane: the packed word
#pragma unroll
            for (int v = 0; v < 2; v++) {
                if (v >= npl) continue;
                float rr[4];   // the horizontal pass of the four rows
#pragma unroll
                for (int k = 0; k < 4; k++) rr[k] = chroma_row_sum(tile[v] + at0 + k * CH_LD, cx);
                o[v] = to_u16(chroma_row_sum(rr, cy), fmax, max) << lshift;
            }
            const long long at = f * dframe + Y * drow + (long long)X * dpx;
            if (pair) *reinterpret_cast<unsigned *>(du + at) = o[0] | (o[1] << 16);
            else {
                du[at] = (unsigned short)o[0];
                if (npl == 2) dv[at] = (unsigned short)o[1];
            }
        }
    }
}

// The planes su (and sv: nullptr = one plane per frame) of cw x ch samples of n frames -> ow x oh samples at du (and dv), by the two axes' r and o (chroma_axis,
// w2xc_host_geom.hpp: 0 < r <= 1, o 0.5 or 0.25); the packings are su's and du's.  One launch; the loads are clamped into cw x ch whatever the axes say.
hipError_t w2xc_launch_chroma_resize_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int ow, int oh, int depth,
                                         double rx, double ox, double ry, double oy, int n, hipStream_t st)
{
    ChromaU16 c;
    if (!chroma_prologue_u16(su, sv, cw, ch, du, dv, ow, oh, depth, n, &c) || !(rx > 0.0 && rx <= 1.0) || !(ry > 0.0 && ry <= 1.0) || (ox != 0.5 && ox != 0.25) ||
        (oy != 0.5 && oy != 0.25))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::chroma_resize_tile_grid(ow, oh, n, CR_TX, CR_TY, W2XC_CHROMA_GRID_MAX);   // a turn: one tile of ALL planes of a frame
    const auto kernel = c.load == 2 ? k_chroma_resize_u16<2> : c.load == 1 ? k_chroma_resize_u16<1> : k_chroma_resize_u16<0>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, su.p, sv, su.frame, su.row, su.px, cw, ch, c.rshift, c.k.max, du.p, dv, du.frame, du.row, du.px, c.lshift,
                       c.pair, ow, oh, c.npl, c.k.inv_max, c.k.fmax, rx, ox, ry, oy, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
