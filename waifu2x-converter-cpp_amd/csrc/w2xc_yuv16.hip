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
#include "w2xc_yuv_tile.h" // the tile of the bicubic 2x, the launch grid
#include "w2xc_yuv_launch.h" // the kernel's parameter list, the co-sited instantiations, chroma_prologue_u16

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
__global__ void __launch_bounds__(256) k_chroma2x_u16(W2XC_CHROMA2X_U16_PARAMS)
{
    constexpr bool CX = false, CY = false;   // centred along both axes (the co-sited forms: w2xc_yuv16_sited.hip)
#include "w2xc_chroma2x_u16_body.inc"
}

// cosited: 0 = centred chroma, or W2XC_CHROMA_COSITED_X | _Y -- the same grid, load paths and pair store, the kernel from w2xc_yuv16_sited.hip
hipError_t w2xc_launch_chroma2x_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int ow, int oh, int depth,
                                    int cosited, int n, hipStream_t st)
{
    ChromaU16 c;
    if (!chroma_prologue_u16(su, sv, cw, ch, du, dv, ow, oh, depth, n, &c) || ow > 2 * (long long)cw || oh > 2 * (long long)ch || !cosited_ok(cosited))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::chroma2x_tile_grid(ow, oh, n, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX);   // a turn: one tile of ALL planes of a frame
    const Chroma2xU16Kernel kernel = cosited       ? chroma2x_u16_sited_kernel(c.load, cosited & W2XC_CHROMA_COSITED_X, cosited & W2XC_CHROMA_COSITED_Y)
                                     : c.load == 2 ? k_chroma2x_u16<2>
                                     : c.load == 1 ? k_chroma2x_u16<1>
                                                   : k_chroma2x_u16<0>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, su.p, sv, su.frame, su.row, su.px, cw, ch, c.rshift, c.k.max, du.p, dv, du.frame, du.row, du.px, c.lshift,
                       c.pair, ow, oh, c.npl, c.k.inv_max, c.k.fmax, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
