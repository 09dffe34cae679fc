// w2xc_yuv_sited.hip -- the bicubic 2x of chroma bytes for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h, "Chroma siting":
// w2xc_chroma2x_u8_sited_device and the Y route of the frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built with -ffp-contract=off like w2xc_yuv.hip.
//   k_chroma2x_u8_sited<DW, CX, CY>   k_chroma2x_u8's body (w2xc_chroma2x_u8_body.inc) with t = 0.375 / 0.875 instead of 0.25 / 0.75 on the co-sited axes: output m sits
//                                     on output luma 2m, which is source chroma coordinate m / 2 - 0.125, so outputs 2q - 1 and 2q still share the source pixel q - 1
// An object of its own: the instantiations of w2xc_yuv.o stay what they are.  No launcher here: w2xc_launch_chroma2x_u8 (w2xc_yuv.hip) decides the siting by its
// `cosited` argument and takes the kernel from chroma2x_u8_sited_kernel below.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8
#include "w2xc_px.h"       // cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum
#include "w2xc_yuv_tile.h" // the tile of the bicubic 2x
#include "w2xc_yuv_launch.h" // the kernel's parameter list, the selector's declaration

template <bool DW, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_chroma2x_u8_sited(W2XC_CHROMA2X_U8_PARAMS)
{
    static_assert(CX || CY, "the centred kernel is k_chroma2x_u8");
#include "w2xc_chroma2x_u8_body.inc"
}

// the instantiation for a load path and the flags, at least one of them: w2xc_launch_chroma2x_u8 (w2xc_yuv.hip) launches it
Chroma2xU8Kernel chroma2x_u8_sited_kernel(bool dw, bool cx, bool cy)
{
#define W2XC_C2X(CX, CY) (dw ? k_chroma2x_u8_sited<true, CX, CY> : k_chroma2x_u8_sited<false, CX, CY>)
    return cx && cy ? W2XC_C2X(true, true) : cx ? W2XC_C2X(true, false) : W2XC_C2X(false, true);
#undef W2XC_C2X
}
