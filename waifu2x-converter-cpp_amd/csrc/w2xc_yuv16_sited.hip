// w2xc_yuv16_sited.hip -- the bicubic 2x of chroma words for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h, "Chroma siting":
// w2xc_chroma2x_u16_sited_device and the Y route of the 16-bit frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built with -ffp-contract=off like w2xc_yuv16.hip.
//   k_chroma2x_u16_sited<LOAD, CX, CY>   k_chroma2x_u16's body (w2xc_chroma2x_u16_body.inc) with t = 0.375 / 0.875 instead of 0.25 / 0.75 on the co-sited axes
// An object of its own: the instantiations of w2xc_yuv16.o stay what they are.  No launcher here: w2xc_launch_chroma2x_u16 (w2xc_yuv16.hip) decides the siting by
// its `cosited` argument and takes the kernel from chroma2x_u16_sited_kernel below.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi
#include "w2xc_px.h"       // cubic_coeffs
#include "w2xc_yuv_px.h"   // chroma_row_sum, u16_value, to_u16
#include "w2xc_yuv_tile.h" // the tile of the bicubic 2x
#include "w2xc_yuv_launch.h" // the kernel's parameter list, the selector's declaration

template <int LOAD, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_chroma2x_u16_sited(W2XC_CHROMA2X_U16_PARAMS)
{
    static_assert(CX || CY, "the centred kernel is k_chroma2x_u16");
#include "w2xc_chroma2x_u16_body.inc"
}

// the instantiation for a load path and the flags, at least one of them: w2xc_launch_chroma2x_u16 (w2xc_yuv16.hip) launches it
Chroma2xU16Kernel chroma2x_u16_sited_kernel(int load, bool cx, bool cy)
{
#define W2XC_C2X16(CX, CY) (load == 2 ? k_chroma2x_u16_sited<2, CX, CY> : load == 1 ? k_chroma2x_u16_sited<1, CX, CY> : k_chroma2x_u16_sited<0, CX, CY>)
    return cx && cy ? W2XC_C2X16(true, true) : cx ? W2XC_C2X16(true, false) : W2XC_C2X16(false, true);
#undef W2XC_C2X16
}
