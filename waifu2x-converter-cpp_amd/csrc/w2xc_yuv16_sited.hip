// w2xc_yuv16_sited.hip -- the bicubic 2x of chroma words for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h, "Chroma siting":
// w2xc_chroma2x_u16_sited_device and the Y route of the 16-bit frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built with -ffp-contract=off like w2xc_yuv16.hip.
//   k_chroma2x_u16_sited<LOAD, CX, CY>   k_chroma2x_u16's body (w2xc_chroma2x_u16_body.inc) with t = 0.375 / 0.875 instead of 0.25 / 0.75 on the co-sited axes
// An object of its own: the instantiations of w2xc_yuv16.o stay what they are.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi
#include "w2xc_px.h"       // cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum, u16_value, to_u16, u16_scale
#include "w2xc_yuv_tile.h" // the tile of the bicubic 2x, the launch grid, rows_align

template <int LOAD, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_chroma2x_u16_sited(const unsigned short *su, const unsigned short *sv, long long sframe, long long srow, int spx, int cw,
                                                            int ch, int rshift, int max, unsigned short *du, unsigned short *dv, long long dframe, long long drow,
                                                            int dpx, int lshift, int pair, int ow, int oh, int npl, float inv_max, float fmax, int tiles_x,
                                                            long long tiles, long long turns)
{
    static_assert(CX || CY, "the centred kernel is k_chroma2x_u16");
#include "w2xc_chroma2x_u16_body.inc"
}

// cosited: W2XC_CHROMA_COSITED_X | _Y, at least one of them; everything else as w2xc_launch_chroma2x_u16, whose grid, load paths and pair store these are
hipError_t w2xc_launch_chroma2x_u16_sited(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int ow, int oh, int depth,
                                          int cosited, int n, hipStream_t st)
{
    if (cw < 1 || ch < 1 || ow < 1 || oh < 1 || ow > 2 * (long long)cw || oh > 2 * (long long)ch || n < 1 || (su.px != 1 && su.px != 2) || (du.px != 1 && du.px != 2) ||
        !su.p || !du.p || (sv != nullptr) != (dv != nullptr) || depth < 8 || depth > 16 || !cosited || (cosited & ~(W2XC_CHROMA_COSITED_X | W2XC_CHROMA_COSITED_Y)))
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
    const bool cx = cosited & W2XC_CHROMA_COSITED_X, cy = cosited & W2XC_CHROMA_COSITED_Y;
#define W2XC_C2X16(CX, CY) (load == 2 ? k_chroma2x_u16_sited<2, CX, CY> : load == 1 ? k_chroma2x_u16_sited<1, CX, CY> : k_chroma2x_u16_sited<0, CX, CY>)
    const auto kernel = cx && cy ? W2XC_C2X16(true, true) : cx ? W2XC_C2X16(true, false) : W2XC_C2X16(false, true);
#undef W2XC_C2X16
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, su.p, sv, su.frame, su.row, su.px, cw, ch, rshift, k.max, du.p, dv, du.frame, du.row, du.px, lshift, pair,
                       ow, oh, npl, k.inv_max, k.fmax, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
