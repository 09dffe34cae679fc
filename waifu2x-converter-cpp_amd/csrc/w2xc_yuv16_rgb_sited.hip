// w2xc_yuv16_rgb_sited.hip -- the two ends of 16-bit YUV frames through RGB models for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h,
// "Chroma siting": w2xc_yuv16_to_rgb_device / w2xc_rgb_to_yuv16_device and the RGB route of the 16-bit frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built
// with -ffp-contract=off like w2xc_yuv16_rgb.hip.
//   k_yuv16_to_rgb_sited<CM, SX, SY, CX, CY>   k_yuv16_to_rgb's body (w2xc_yuv16_to_rgb_body.inc): chroma at luma 2k is C[k], at 2k + 1 the mean of C[k] and C[k + 1]
//   k_rgb_to_yuv16_sited<SX, SY, CX, CY>       k_rgb_to_yuv16's body (w2xc_rgb_to_yuv16_body.inc): chroma k is the 1-2-1 mean around luma 2k, exchanged as in
//                                              k_rgb_to_yuv8_sited
// CX / CY only on a subsampled axis: 4:2:0 x, y or both; 4:2:2 x.  An object of its own: the instantiations of w2xc_yuv16_rgb.o stay what they are.  No launcher
// here: w2xc_launch_yuv16_to_rgb / w2xc_launch_rgb_to_yuv16 (w2xc_yuv16_rgb.hip) read the flags in their `chroma` and take the kernel from the two selectors below.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi
#include "w2xc_yuv_px.h"   // u16_value, to_u16, luma_u16, mean121
#include "w2xc_yuv_tile.h" // the tile (YR_*), yuv_tile_at, chroma_at_luma_sited, rgb_px, chroma_mean, row_chroma, top_row_chroma
#include "w2xc_yuv_launch.h" // the kernels' parameter lists, the selectors' declarations, W2XC_SITED_KERNEL

#define YR_YLD (2 * YR_TCX + 2)     // 16-bit words per LDS row of luma, as in w2xc_yuv16_rgb.hip
static_assert((YR_YLD & 1) == 0 && ((YR_YLD / 2) & 1) == 1, "a luma row in LDS is whole dwords, an odd count of them");

template <int CM, bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_yuv16_to_rgb_sited(W2XC_YUV16_TO_RGB_PARAMS)
{
    static_assert(CX || CY, "the centred kernel is k_yuv16_to_rgb");
#include "w2xc_yuv16_to_rgb_body.inc"
}

template <bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_rgb_to_yuv16_sited(W2XC_RGB_TO_YUV16_PARAMS)
{
    static_assert(CX || CY, "the centred kernel is k_rgb_to_yuv16");
#include "w2xc_rgb_to_yuv16_body.inc"
}

// the instantiations for a load path, a layout and its flags -- one of the four pairs chroma_layout lets through with a flag: the launchers of w2xc_yuv16_rgb.hip
// launch them
Yuv16ToRgbKernel yuv16_to_rgb_sited_kernel(int cm, int layout, bool cx, bool cy)
{
#define W2XC_TO_RGB16(SX, SY, CX, CY) \
    (cm == 2 ? k_yuv16_to_rgb_sited<2, SX, SY, CX, CY> : cm == 1 ? k_yuv16_to_rgb_sited<1, SX, SY, CX, CY> : k_yuv16_to_rgb_sited<0, SX, SY, CX, CY>)
    return W2XC_SITED_KERNEL(W2XC_TO_RGB16, layout, cx, cy);
#undef W2XC_TO_RGB16
}

RgbToYuv16Kernel rgb_to_yuv16_sited_kernel(int layout, bool cx, bool cy)
{
#define W2XC_FROM_RGB16(SX, SY, CX, CY) k_rgb_to_yuv16_sited<SX, SY, CX, CY>
    return W2XC_SITED_KERNEL(W2XC_FROM_RGB16, layout, cx, cy);
#undef W2XC_FROM_RGB16
}
