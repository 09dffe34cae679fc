// w2xc_yuv_rgb_sited.hip -- the two ends of YUV frames through RGB models for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h, "Chroma
// siting": w2xc_yuv8_to_rgb_device / w2xc_rgb_to_yuv8_device and the RGB route of the frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built with
// -ffp-contract=off like w2xc_yuv_rgb.hip.
//   k_yuv8_to_rgb_sited<DW, SX, SY, CX, CY>   k_yuv8_to_rgb's body (w2xc_yuv8_to_rgb_body.inc): chroma at luma 2k is C[k], at 2k + 1 the mean of C[k] and C[k + 1]
//   k_rgb_to_yuv8_sited<SX, SY, CX, CY>       k_rgb_to_yuv8's body (w2xc_rgb_to_yuv8_body.inc): chroma k is the 1-2-1 mean around luma 2k; the neighbour column comes
//                                             from the lane below, the neighbour row from 4 KB of LDS, the tile's own left column and top row from memory
// CX / CY only on a subsampled axis: 4:2:0 x, y or both; 4:2:2 x.  An object of its own: the instantiations of w2xc_yuv_rgb.o stay what they are.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8
#include "w2xc_yuv_px.h"   // luma_u8, chroma_u8, mean121, the constants of a matrix, sited_layout
#include "w2xc_yuv_tile.h" // the tile (YR_*), rows_align, yuv_tile_at, chroma_at_luma_sited, rgb_px, chroma_mean, row_chroma, top_row_chroma

#define YR_YLD (2 * YR_TCX + 4)     // bytes per LDS row of luma, as in w2xc_yuv_rgb.hip
static_assert((YR_YLD & 3) == 0, "a luma row in LDS is whole dwords");

template <bool DW, bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_yuv8_to_rgb_sited(const unsigned char *__restrict__ sy, long long yframe, long long yrow, const unsigned char *__restrict__ su,
                                                           const unsigned char *__restrict__ sv, long long cframe, long long crow, int spx, int w, int h, int cw, int ch,
                                                           int limited, W2xcYuvToRgb m, float *__restrict__ rgb, long long is, long long ps, int v2, int tiles_x,
                                                           long long tiles, long long turns)
{
    static_assert(CX || CY, "the centred kernel is k_yuv8_to_rgb");
#include "w2xc_yuv8_to_rgb_body.inc"
}

template <bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_rgb_to_yuv8_sited(const float *__restrict__ rgb, long long is, long long ps, int v2, int w, int h, int cw, int ch, int limited,
                                                           W2xcRgbToYuv m, unsigned char *__restrict__ dy, long long yframe, long long yrow, int y16,
                                                           unsigned char *__restrict__ du, unsigned char *__restrict__ dv, long long cframe, long long crow, int dpx,
                                                           int tiles_x, long long tiles, long long turns)
{
    static_assert(CX || CY, "the centred kernel is k_rgb_to_yuv8");
#include "w2xc_rgb_to_yuv8_body.inc"
}

// the instantiation of K for a layout and its flags (sited_layout has let only these four through)
#define W2XC_SITED_KERNEL(K, layout, cx, cy) \
    ((layout) == 1 ? K(true, false, true, false) : (cx) && (cy) ? K(true, true, true, true) : (cx) ? K(true, true, true, false) : K(true, true, false, true))

// chroma = the layout with W2XC_CHROMA_COSITED_* or-ed on; everything else as w2xc_launch_yuv8_to_rgb, whose grid, load paths and stores these are
hipError_t w2xc_launch_yuv8_to_rgb_sited(W2xcU8Planes y, W2xcU8Planes u, const unsigned char *v, int w, int h, int chroma, int range, int matrix, float *rgb,
                                         long long is, long long ps, int n, hipStream_t st)
{
    W2xcYuvToRgb m;
    int cw, ch, layout;
    bool cx, cy;
    if (!sited_layout(chroma, &layout, &cx, &cy) || !matrix_to_rgb(matrix, &m) || !frame_geometry(w, h, layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb ||
        y.px != 1 || (u.px != 1 && u.px != 2))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    size_t align = rows_align(y, n);
    if (u.px == 1) align |= rows_align(u, n) | reinterpret_cast<size_t>(v);
    const bool dw = (align & 3) == 0;
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n);
#define W2XC_TO_RGB(SX, SY, CX, CY) (dw ? k_yuv8_to_rgb_sited<true, SX, SY, CX, CY> : k_yuv8_to_rgb_sited<false, SX, SY, CX, CY>)
    const auto kernel = W2XC_SITED_KERNEL(W2XC_TO_RGB, layout, cx, cy);
#undef W2XC_TO_RGB
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, y.p, y.frame, y.row, u.p, v, u.frame, u.row, u.px, w, h, cw, ch, limited, m, rgb, is, ps, v2,
                       g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}

hipError_t w2xc_launch_rgb_to_yuv8_sited(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, W2xcU8Planes y, W2xcU8Planes u,
                                         unsigned char *v, int n, hipStream_t st)
{
    W2xcRgbToYuv m;
    int cw, ch, layout;
    bool cx, cy;
    if (!sited_layout(chroma, &layout, &cx, &cy) || !matrix_from_rgb(matrix, &m) || !frame_geometry(w, h, layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb ||
        y.px != 1 || (u.px != 1 && u.px != 2))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int y16 = (rows_align(y, n) & 1) == 0;
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n);
#define W2XC_FROM_RGB(SX, SY, CX, CY) k_rgb_to_yuv8_sited<SX, SY, CX, CY>
    const auto kernel = W2XC_SITED_KERNEL(W2XC_FROM_RGB, layout, cx, cy);
#undef W2XC_FROM_RGB
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, rgb, is, ps, v2, w, h, cw, ch, limited, m, y.p, y.frame, y.row, y16, u.p, v, u.frame, u.row, u.px,
                       g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
