// w2xc_yuv.hip -- YUV frames (include/w2xc_hip.h, "YUV frames": w2xc_process_frames_yuv_u8[_device] and their building blocks): luma bytes to the float
// plane the models take and back, and the 2x enlargement of chroma on bytes.  No colour matrix anywhere.  Built with -ffp-contract=off like w2xc_color.hip:
// every product and sum below is its own fp32 operation.
//   Y8ToPlane / PlaneToY8   two stages on the per-pixel skeleton (w2xc_px.h), batch forms, the range a stage member
//   ChromaCopy              chroma bytes as they are (a call without a 2x step), from either sample stride to either
//   k_chroma2x_u8           bytes in, bytes out: Resize2xCubic (w2xc_color.hip) on (float)byte * (float)(1.0 / 255.0), then to_u8, without a float plane of
//                           chroma in memory
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8
#include "w2xc_px.h"       // k_px, launch_px, row_col, cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum, luma_u8
#include "w2xc_yuv_tile.h" // the tile of the bicubic 2x, the launch grid
#include "w2xc_yuv_launch.h" // the kernel's parameter list, the co-sited instantiations, chroma_prologue_u8

// luma byte -> y: full range (float)Y * (float)(1.0 / 255.0), limited range ((float)Y - 16) * (float)(1.0 / 219.0).  Frame i's plane at dst + i * ps floats
struct Y8ToPlane {
    const unsigned char *src;
    long long frame, row;
    int w, limited;
    float *dst;
    long long ps;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const float Y = (float)src[img * frame + at.r * row + at.c];
        dst[img * ps + q] = limited ? (Y - 16.0f) * (float)(1.0 / 219.0) : Y * (float)(1.0 / 255.0);
    }
};
hipError_t w2xc_launch_y8_to_plane(W2xcU8Planes src, int w, int h, int range, float *dst, long long ps, int n, hipStream_t st)
{
    return launch_px(Y8ToPlane{src.p, src.frame, src.row, w, range != 0, dst, ps}, (long long)w * h, n, st);
}

// y -> luma byte (luma_u8)
struct PlaneToY8 {
    const float *src;
    long long ps;
    int w, limited;
    unsigned char *dst;
    long long frame, row;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const float y = src[img * ps + q];
        dst[img * frame + at.r * row + at.c] = luma_u8(y, limited);
    }
};
hipError_t w2xc_launch_plane_to_y8(const float *src, long long ps, int w, int h, int range, W2xcU8Planes dst, int n, hipStream_t st)
{
    return launch_px(PlaneToY8{src, ps, w, range != 0, dst.p, dst.frame, dst.row}, (long long)w * h, n, st);
}

// plane p of the launch: npl planes per frame (U, or U and V), frame p / npl
struct ChromaCopy {
    const unsigned char *su, *sv;
    long long sframe, srow;
    int spx, cw, npl;
    unsigned char *du, *dv;
    long long dframe, drow;
    int dpx;
    __device__ __forceinline__ void operator()(int p, long long q) const
    {
        const RowCol at = row_col(q, cw);
        const int f = p / npl, v = p - f * npl;
        (v ? dv : du)[f * dframe + at.r * drow + (long long)at.c * dpx] = (v ? sv : su)[f * sframe + at.r * srow + (long long)at.c * spx];
    }
};
hipError_t w2xc_launch_chroma_copy_u8(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, unsigned char *dv, int n, hipStream_t st)
{
    const int npl = sv ? 2 : 1;
    return launch_px(ChromaCopy{su.p, sv, su.frame, su.row, su.px, cw, npl, du.p, dv, du.frame, du.row, du.px}, (long long)cw * ch, n * npl, st);
}

// ---- the bicubic 2x of chroma, bytes to bytes ----
// Resize2xCubic reads, for output column X, fx = (X + 0.5) * 0.5 - 0.5, sx = floor(fx), t = fx - sx and the taps sx - 1 .. sx + 2 clamped into the plane.  The
// two columns 2 sx + 1 (t = 0.25) and 2 sx + 2 (t = 0.75) share sx and so their taps; the same holds for rows.  A QUAD (qx, qy) is those 2 x 2 outputs of the
// source pixel (sx, sy) = (qx - 1, qy - 1): columns 2 qx - 1 and 2 qx, rows 2 qy - 1 and 2 qy, all from ONE 4 x 4 neighbourhood.  Quad 0 has only its second
// column / row inside the plane (sx = -1: output 0, every tap clamped to 0 or 1), the last quad of an uncropped plane only its first.
// A tile is TQX x TQY quads of one plane of one frame; a workgroup of 256 threads = 32 x 8 takes two quads per thread, TQY / 2 quad rows apart.  The source
// pixels the tile reads -- its TQX x TQY source pixels, one more to the left and above, two more to the right and below, coordinates clamped as the taps are --
// are fetched once, converted to c = (float)byte * (float)(1.0 / 255.0) and kept in LDS as floats, rows of CH_LD words: a wave's 32-lane halves read 32
// consecutive words of a row (conflict-free for any row length; the odd length keeps the dword loader's column-strided writes off each other's banks).
// DW: the source planes are planar (px = 1) and every row starts on a 4-byte boundary: an aligned group of four source pixels that lies inside the row is one
// dword load by one thread; everything else (the clamped rim, px = 2) one byte load per LDS word.
// Stores: the thread's own bytes, one byte store each -- a quad's two columns start on an odd column, and with px = 2 the other plane's bytes lie between
// them --, never a read-modify-write of a byte that is another thread's.
template <bool DW>
__global__ void __launch_bounds__(256) k_chroma2x_u8(W2XC_CHROMA2X_U8_PARAMS)
{
    constexpr bool CX = false, CY = false;   // centred along both axes (the co-sited forms: w2xc_yuv_sited.hip)
#include "w2xc_chroma2x_u8_body.inc"
}

// cosited: 0 = centred chroma, or W2XC_CHROMA_COSITED_X | _Y -- the same grid and load path, the kernel from w2xc_yuv_sited.hip
hipError_t w2xc_launch_chroma2x_u8(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, unsigned char *dv, int ow, int oh, int cosited, int n,
                                   hipStream_t st)
{
    int npl;
    bool dw;
    if (!chroma_prologue_u8(su, sv, cw, ch, du, dv, ow, oh, n, &npl, &dw) || ow > 2 * (long long)cw || oh > 2 * (long long)ch || !cosited_ok(cosited))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::chroma2x_tile_grid(ow, oh, (long long)n * npl, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX);   // a turn: one tile of ONE plane
    const Chroma2xU8Kernel kernel = cosited ? chroma2x_u8_sited_kernel(dw, cosited & W2XC_CHROMA_COSITED_X, cosited & W2XC_CHROMA_COSITED_Y)
                                    : dw    ? k_chroma2x_u8<true>
                                            : k_chroma2x_u8<false>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, su.p, sv, su.frame, su.row, su.px, cw, ch, du.p, dv, du.frame, du.row, du.px, ow, oh, npl, g.tiles_x,
                       g.tiles, g.turns);
    return hipGetLastError();
}
