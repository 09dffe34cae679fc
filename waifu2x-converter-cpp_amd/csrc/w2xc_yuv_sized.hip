// w2xc_yuv_sized.hip -- chroma bytes of a SIZED frame call (include/w2xc_hip.h, "Sized YUV frames": w2xc_chroma_resize_u8_device and the Y route of
// w2xc_process_frames_yuv_u8_sized*): the bicubic of k_chroma2x_u8 at ANY ratio r <= 1 per axis, in one step from the input plane to the output plane.
// Built with -ffp-contract=off like w2xc_yuv.hip.  An object of its own: the instantiations of w2xc_yuv.o and w2xc_yuv_sited.o stay what they are.
//   k_chroma_resize_u8<DW>   output sample m of an axis reads pos = (m + o) * r - o (double: chroma_resize_pos, w2xc_host_geom.hpp), s = floor(pos),
//                            t = (float)(pos - s), the taps s - 1 .. s + 2 clamped, cubic_coeffs(t), chroma_row_sum horizontally then vertically, to_u8
// A turn is a tile of CR_TX x CR_TY OUTPUT samples of one plane of one frame; 256 threads = 32 x 8 take one column and two rows each, CR_TY / 2 apart.  With
// r <= 1 the floors of 32 consecutive outputs span at most 32 source samples, so the tile's source window with its taps is at most CH_SW x CH_SH = 35 x 19: the
// window k_chroma2x_u8 stages, as floats in LDS, rows of CH_LD = 37 words.  Its origin is computed per tile (chroma_resize_origin) where the 2x kernel has
// 2 q0 - 2.  A 32-lane half of a wave shares its row and reads, per tap, words that step by 0 or 1 from lane to lane: at most 32 consecutive words, equal
// addresses broadcast, no bank conflict for any row length; the two halves of a wave (ds_read_b32 banks them apart) read rows 0 or 1 apart.  The odd pitch
// keeps the dword loader's column-strided writes where k_chroma2x_u8 has them.
// Loaders and stores are k_chroma2x_u8's: DW (planar rows on 4-byte boundaries) one dword load per aligned group of four source samples inside the row, else a
// byte load per LDS word; each thread stores its own bytes, never a read-modify-write.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8
#include "w2xc_px.h"       // cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum
#include "w2xc_yuv_tile.h" // CH_SW, CH_SH, CH_LD; w2xc_host_geom.hpp: chroma_resize_pos / _floor / _origin, chroma_resize_tile_grid
#include "w2xc_yuv_launch.h" // chroma_prologue_u8: the checks and the load path of the 2x launcher

#define CR_TX W2XC_CHROMA_RESIZE_TX
#define CR_TY W2XC_CHROMA_RESIZE_TY
static_assert(CR_TX == 32 && CR_TY == 16 && CR_TX + 3 == CH_SW && CR_TY + 3 == CH_SH, "256 threads = 32 columns x 8 rows, two rows per thread; the 2x kernels' window");

using w2xc_eng::chroma_resize_floor;
using w2xc_eng::chroma_resize_origin;
using w2xc_eng::chroma_resize_pos;

template <bool DW>
__global__ void __launch_bounds__(256) k_chroma_resize_u8(const unsigned char *su, const unsigned char *sv, long long sframe, long long srow, int spx, int cw, int ch,
                                                          unsigned char *du, unsigned char *dv, long long dframe, long long drow, int dpx, int ow, int oh, int npl,
                                                          double rx, double ox, double ry, double oy, int tiles_x, long long tiles, long long turns)
{
    __shared__ float tile[CH_SH * CH_LD];
    const float s255 = (float)(1.0 / 255.0);
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of one plane of one frame
        const long long p = turn / tiles, t = turn - p * tiles;
        const long long f = p / npl;
        const int v = (int)(p - f * npl);
        const unsigned char *s = (v ? sv : su) + f * sframe;
        unsigned char *d = (v ? dv : du) + f * dframe;
        const int y0 = (int)(t / tiles_x) * CR_TY, x0 = (int)(t % tiles_x) * CR_TX;
        const int gx0 = chroma_resize_origin(x0, rx, ox), gy0 = chroma_resize_origin(y0, ry, oy);   // the source sample of LDS word (0, 0)
        __syncthreads();   // (the tile of the loop's previous turn has been read)
        if (DW) {
            // column groups of four source samples from the multiple of 4 at or below gx0 on: ten cover the CH_SW columns
            const int ga = gx0 & ~3, off = gx0 - ga;
            for (int i = threadIdx.x; i < CH_SH * 10; i += 256) {
                const int r = i / 10, g = i - r * 10;
                const int gx4 = ga + 4 * g;
                const unsigned char *row = s + clampi(gy0 + r, 0, ch - 1) * srow;
                unsigned b[4];
                if (gx4 >= 0 && gx4 + 3 < cw) {
                    const unsigned w4 = *reinterpret_cast<const unsigned *>(row + gx4);
                    b[0] = w4 & 255u; b[1] = (w4 >> 8) & 255u; b[2] = (w4 >> 16) & 255u; b[3] = w4 >> 24;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) b[k] = row[clampi(gx4 + k, 0, cw - 1)];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int c = 4 * g - off + k;
                    if (c >= 0 && c < CH_SW) tile[r * CH_LD + c] = (float)b[k] * s255;
                }
            }
        } else {
            for (int i = threadIdx.x; i < CH_SH * CH_SW; i += 256) {
                const int r = i / CH_SW, c = i - r * CH_SW;
                tile[r * CH_LD + c] = (float)s[clampi(gy0 + r, 0, ch - 1) * srow + (long long)clampi(gx0 + c, 0, cw - 1) * spx] * s255;
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
            const float *S = tile + (sy - 1 - gy0) * CH_LD + c0;
            float rr[4];   // the horizontal pass of the four rows
#pragma unroll
            for (int k = 0; k < 4; k++) rr[k] = chroma_row_sum(S + k * CH_LD, cx);
            d[Y * drow + (long long)X * dpx] = to_u8(chroma_row_sum(rr, cy));
        }
    }
}

// The planes su (and sv: nullptr = one plane per frame) of cw x ch samples of n frames -> ow x oh samples at du (and dv), by the two axes' r and o (chroma_axis,
// w2xc_host_geom.hpp: 0 < r <= 1, o 0.5 or 0.25).  One launch; the loads are clamped into cw x ch whatever the axes say.
hipError_t w2xc_launch_chroma_resize_u8(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, unsigned char *dv, int ow, int oh,
                                        double rx, double ox, double ry, double oy, int n, hipStream_t st)
{
    int npl;
    bool dw;
    if (!chroma_prologue_u8(su, sv, cw, ch, du, dv, ow, oh, n, &npl, &dw) || !(rx > 0.0 && rx <= 1.0) || !(ry > 0.0 && ry <= 1.0) || (ox != 0.5 && ox != 0.25) ||
        (oy != 0.5 && oy != 0.25))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::chroma_resize_tile_grid(ow, oh, (long long)n * npl, CR_TX, CR_TY, W2XC_CHROMA_GRID_MAX);   // a turn: one tile of ONE plane
    hipLaunchKernelGGL(dw ? k_chroma_resize_u8<true> : k_chroma_resize_u8<false>, dim3(g.grid), dim3(256), 0, st, su.p, sv, su.frame, su.row, su.px, cw, ch, du.p, dv,
                       du.frame, du.row, du.px, ow, oh, npl, rx, ox, ry, oy, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
