// w2xc_yuv_sited.hip -- the bicubic 2x of chroma bytes for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h, "Chroma siting":
// w2xc_chroma2x_u8_sited_device and the Y route of the frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built with -ffp-contract=off like w2xc_yuv.hip.
//   k_chroma2x_u8_sited<DW, CX, CY>   k_chroma2x_u8's body (w2xc_chroma2x_u8_body.inc) with t = 0.375 / 0.875 instead of 0.25 / 0.75 on the co-sited axes: output m sits
//                                     on output luma 2m, which is source chroma coordinate m / 2 - 0.125, so outputs 2q - 1 and 2q still share the source pixel q - 1
// An object of its own: the instantiations of w2xc_yuv.o stay what they are.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8
#include "w2xc_px.h"       // cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum
#include "w2xc_yuv_tile.h" // the tile of the bicubic 2x, the launch grid, rows_align

template <bool DW, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_chroma2x_u8_sited(const unsigned char *su, const unsigned char *sv, long long sframe, long long srow, int spx, int cw, int ch,
                                                           unsigned char *du, unsigned char *dv, long long dframe, long long drow, int dpx, int ow, int oh, int npl,
                                                           int tiles_x, long long tiles, long long turns)
{
    static_assert(CX || CY, "the centred kernel is k_chroma2x_u8");
#include "w2xc_chroma2x_u8_body.inc"
}

// cosited: W2XC_CHROMA_COSITED_X | _Y, at least one of them; everything else as w2xc_launch_chroma2x_u8, whose grid and load path these are
hipError_t w2xc_launch_chroma2x_u8_sited(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, unsigned char *dv, int ow, int oh, int cosited, int n,
                                         hipStream_t st)
{
    if (cw < 1 || ch < 1 || ow < 1 || oh < 1 || ow > 2 * (long long)cw || oh > 2 * (long long)ch || n < 1 || (su.px != 1 && su.px != 2) || (du.px != 1 && du.px != 2) ||
        !su.p || !du.p || (sv != nullptr) != (dv != nullptr) || !cosited || (cosited & ~(W2XC_CHROMA_COSITED_X | W2XC_CHROMA_COSITED_Y)))
        return hipErrorInvalidValue;
    const int npl = sv ? 2 : 1;
    const YuvTileGrid g = w2xc_eng::chroma2x_tile_grid(ow, oh, (long long)n * npl, CH_TQX, CH_TQY, W2XC_CHROMA_GRID_MAX);   // a turn: one tile of ONE plane
    const bool dw = su.px == 1 && ((rows_align(su, n) | (sv ? reinterpret_cast<size_t>(sv) : 0)) & 3) == 0;
    const bool cx = cosited & W2XC_CHROMA_COSITED_X, cy = cosited & W2XC_CHROMA_COSITED_Y;
#define W2XC_C2X(CX, CY) (dw ? k_chroma2x_u8_sited<true, CX, CY> : k_chroma2x_u8_sited<false, CX, CY>)
    const auto kernel = cx && cy ? W2XC_C2X(true, true) : cx ? W2XC_C2X(true, false) : W2XC_C2X(false, true);
#undef W2XC_C2X
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, su.p, sv, su.frame, su.row, su.px, cw, ch, du.p, dv, du.frame, du.row, du.px, ow, oh, npl, g.tiles_x,
                       g.tiles, g.turns);
    return hipGetLastError();
}
