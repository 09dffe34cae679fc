// w2xc_yuv_rgb_sited.hip -- the two ends of YUV frames through RGB models for chroma that is CO-SITED with luma along x and / or y (include/w2xc_hip.h, "Chroma
// siting": w2xc_yuv8_to_rgb_device / w2xc_rgb_to_yuv8_device and the RGB route of the frame calls with W2XC_CHROMA_COSITED_* in `chroma`).  Built with
// -ffp-contract=off like w2xc_yuv_rgb.hip.
//   k_yuv8_to_rgb_sited<DW, SX, SY, CX, CY>   k_yuv8_to_rgb's body (w2xc_yuv8_to_rgb_body.inc): chroma at luma 2k is C[k], at 2k + 1 the mean of C[k] and C[k + 1]
//   k_rgb_to_yuv8_sited<SX, SY, CX, CY>       k_rgb_to_yuv8's body (w2xc_rgb_to_yuv8_body.inc): chroma k is the 1-2-1 mean around luma 2k; the neighbour column comes
//                                             from the lane below, the neighbour row from 4 KB of LDS, the tile's own left column and top row from memory
// CX / CY only on a subsampled axis: 4:2:0 x, y or both; 4:2:2 x.  An object of its own: the instantiations of w2xc_yuv_rgb.o stay what they are.  No launcher
// here: w2xc_launch_yuv8_to_rgb / w2xc_launch_rgb_to_yuv8 (w2xc_yuv_rgb.hip) read the flags in their `chroma` and take the kernel from the two selectors below.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8
#include "w2xc_yuv_px.h"   // luma_u8, chroma_u8, mean121
#include "w2xc_yuv_tile.h" // the tile (YR_*), yuv_tile_at, chroma_at_luma_sited, rgb_px, chroma_mean, row_chroma, top_row_chroma
#include "w2xc_yuv_launch.h" // the kernels' parameter lists, the selectors' declarations, W2XC_SITED_KERNEL

#define YR_YLD (2 * YR_TCX + 4)     // bytes per LDS row of luma, as in w2xc_yuv_rgb.hip
static_assert((YR_YLD & 3) == 0, "a luma row in LDS is whole dwords");

template <bool DW, bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_yuv8_to_rgb_sited(W2XC_YUV8_TO_RGB_PARAMS)
{
    static_assert(CX || CY, "the centred kernel is k_yuv8_to_rgb");
#include "w2xc_yuv8_to_rgb_body.inc"
}

template <bool SX, bool SY, bool CX, bool CY>
__global__ void __launch_bounds__(256) k_rgb_to_yuv8_sited(W2XC_RGB_TO_YUV8_PARAMS)
{
    static_assert(CX || CY, "the centred kernel is k_rgb_to_yuv8");
#include "w2xc_rgb_to_yuv8_body.inc"
}

// the instantiations for a load path, a layout and its flags -- one of the four pairs chroma_layout lets through with a flag: the launchers of w2xc_yuv_rgb.hip
// launch them
Yuv8ToRgbKernel yuv8_to_rgb_sited_kernel(bool dw, int layout, bool cx, bool cy)
{
#define W2XC_TO_RGB(SX, SY, CX, CY) (dw ? k_yuv8_to_rgb_sited<true, SX, SY, CX, CY> : k_yuv8_to_rgb_sited<false, SX, SY, CX, CY>)
    return W2XC_SITED_KERNEL(W2XC_TO_RGB, layout, cx, cy);
#undef W2XC_TO_RGB
}

RgbToYuv8Kernel rgb_to_yuv8_sited_kernel(int layout, bool cx, bool cy)
{
#define W2XC_FROM_RGB(SX, SY, CX, CY) k_rgb_to_yuv8_sited<SX, SY, CX, CY>
    return W2XC_SITED_KERNEL(W2XC_FROM_RGB, layout, cx, cy);
#undef W2XC_FROM_RGB
}
