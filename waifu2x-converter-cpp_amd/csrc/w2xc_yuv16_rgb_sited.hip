// w2xc_yuv16_rgb_sited.hip -- the two ends of 16-bit YUV frames through RGB models for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h,
// "Chroma siting": w2xc_yuv16_to_rgb_device / w2xc_rgb_to_yuv16_device and the RGB route of the 16-bit frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built
// with -ffp-contract=off like w2xc_yuv16_rgb.hip.
//   k_yuv16_to_rgb_sited<CM, SX, SY, CX, CY>   k_yuv16_to_rgb's body (w2xc_yuv16_to_rgb_body.inc): chroma at luma 2k is C[k], at 2k + 1 the mean of C[k] and C[k + 1]
//   k_rgb_to_yuv16_sited<SX, SY, CX, CY>       k_rgb_to_yuv16's body (w2xc_rgb_to_yuv16_body.inc): chroma k is the 1-2-1 mean around luma 2k, exchanged as in
//                                              k_rgb_to_yuv8_sited
// CX / CY only on a subsampled axis: 4:2:0 x, y or both; 4:2:2 x.  An object of its own: the instantiations of w2xc_yuv16_rgb.o stay what they are.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi
#include "w2xc_yuv_px.h"   // u16_value, to_u16, luma_u16, mean121, the constants of a matrix and of a depth, sited_layout
#include "w2xc_yuv_tile.h" // the tile (YR_*), rows_align, yuv_tile_at, chroma_at_luma_sited, rgb_px, chroma_mean, row_chroma, top_row_chroma

#define YR_YLD (2 * YR_TCX + 2)     // 16-bit words per LDS row of luma, as in w2xc_yuv16_rgb.hip
static_assert((YR_YLD & 1) == 0 && ((YR_YLD / 2) & 1) == 1, "a luma row in LDS is whole dwords, an odd count of them");

template <int CM, bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_yuv16_to_rgb_sited(const unsigned short *__restrict__ sy, long long yframe, long long yrow, int yv, int yshift,
                                                            const unsigned short *__restrict__ su, const unsigned short *__restrict__ sv, long long cframe,
                                                            long long crow, int spx, int cshift, int max, int w, int h, int cw, int ch, float y0, float ky, float c0,
                                                            float kc, W2xcYuvToRgb m, float *__restrict__ rgb, long long is, long long ps, int v2, int tiles_x,
                                                            long long tiles, long long turns)
{
    static_assert(CX || CY, "the centred kernel is k_yuv16_to_rgb");
#include "w2xc_yuv16_to_rgb_body.inc"
}

template <bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_rgb_to_yuv16_sited(const float *__restrict__ rgb, long long is, long long ps, int v2, int w, int h, int cw, int ch, int limited,
                                                            int max, float ys, float y0, float cs, float c0, W2xcRgbToYuv m, unsigned short *__restrict__ dy,
                                                            long long yframe, long long yrow, int y32, int yshift, unsigned short *__restrict__ du,
                                                            unsigned short *__restrict__ dv, long long cframe, long long crow, int dpx, int uv32, int cshift,
                                                            int tiles_x, long long tiles, long long turns)
{
    static_assert(CX || CY, "the centred kernel is k_rgb_to_yuv16");
#include "w2xc_rgb_to_yuv16_body.inc"
}

// the instantiation of K for a layout and its flags (sited_layout has let only these four through)
#define W2XC_SITED_KERNEL(K, layout, cx, cy) \
    ((layout) == 1 ? K(true, false, true, false) : (cx) && (cy) ? K(true, true, true, true) : (cx) ? K(true, true, true, false) : K(true, true, false, true))

// chroma = the layout with W2XC_CHROMA_COSITED_* or-ed on; everything else as w2xc_launch_yuv16_to_rgb, whose grid, load paths and stores these are
hipError_t w2xc_launch_yuv16_to_rgb_sited(W2xcU16Planes y, W2xcU16Planes u, const unsigned short *v, int w, int h, int chroma, int range, int matrix, int depth,
                                          float *rgb, long long is, long long ps, int n, hipStream_t st)
{
    W2xcYuvToRgb m;
    int cw, ch, layout;
    bool cx, cy;
    if (!sited_layout(chroma, &layout, &cx, &cy) || !matrix_to_rgb(matrix, &m) || !frame_geometry(w, h, layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb ||
        y.px != 1 || (u.px != 1 && u.px != 2) || depth < 8 || depth > 16)
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int yv = (rows_align(y, n) & 7) == 0;
    int cm = 0;
    if (u.px == 1 && ((rows_align(u, n) | reinterpret_cast<size_t>(v)) & 7) == 0) cm = 1;
    else if (u.px == 2 && v == u.p + 1 && (rows_align(u, n) & 3) == 0) cm = 2;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    const int v2 = rows_8_aligned(rgb, is, ps, w, n), yshift = y.pack ? 16 - depth : 0, cshift = u.pack ? 16 - depth : 0;
#define W2XC_TO_RGB16(SX, SY, CX, CY) \
    (cm == 2 ? k_yuv16_to_rgb_sited<2, SX, SY, CX, CY> : cm == 1 ? k_yuv16_to_rgb_sited<1, SX, SY, CX, CY> : k_yuv16_to_rgb_sited<0, SX, SY, CX, CY>)
    const auto kernel = W2XC_SITED_KERNEL(W2XC_TO_RGB16, layout, cx, cy);
#undef W2XC_TO_RGB16
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, y.p, y.frame, y.row, yv, yshift, u.p, v, u.frame, u.row, u.px, cshift, k.max, w, h, cw, ch, k.y_off, k.y_in,
                       k.c_mid, k.c_in, m, rgb, is, ps, v2, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}

hipError_t w2xc_launch_rgb_to_yuv16_sited(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, int depth, W2xcU16Planes y,
                                          W2xcU16Planes u, unsigned short *v, int n, hipStream_t st)
{
    W2xcRgbToYuv m;
    int cw, ch, layout;
    bool cx, cy;
    if (!sited_layout(chroma, &layout, &cx, &cy) || !matrix_from_rgb(matrix, &m) || !frame_geometry(w, h, layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb ||
        y.px != 1 || (u.px != 1 && u.px != 2) || depth < 8 || depth > 16)
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int y32 = (rows_align(y, n) & 3) == 0;
    const int uv32 = u.px == 2 && v == u.p + 1 && (rows_align(u, n) & 3) == 0;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n), yshift = y.pack ? 16 - depth : 0, cshift = u.pack ? 16 - depth : 0;
#define W2XC_FROM_RGB16(SX, SY, CX, CY) k_rgb_to_yuv16_sited<SX, SY, CX, CY>
    const auto kernel = W2XC_SITED_KERNEL(W2XC_FROM_RGB16, layout, cx, cy);
#undef W2XC_FROM_RGB16
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, rgb, is, ps, v2, w, h, cw, ch, limited, k.max, k.y_out, k.y_off, k.c_out, k.c_mid, m, y.p, y.frame, y.row,
                       y32, yshift, u.p, v, u.frame, u.row, u.px, uv32, cshift, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
