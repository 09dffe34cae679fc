// w2xc_px.h -- the per-pixel skeleton of the stages around the CNN, shared by w2xc_color.hip (the colour stages) and w2xc_yuv.hip (the YUV frame stages):
// every stage is ONE struct of pointers, strides and sizes whose operator()(img, q) computes output element q of image / plane img; the one kernel template
// k_px holds the loops over both, and launch_px the grid and the launch.  A stage is its kernel's by-value argument: img comes from blockIdx.y -- uniform per
// workgroup -- and moves only the stage's 64-bit base pointers by img x stride.  One image is n = 1.
// And the coefficients of the bicubic 2x (Resize2xCubic in w2xc_color.hip, k_chroma2x_u8 in w2xc_yuv.hip): ONE definition.
// Device code only; every file that includes it is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

// blockIdx.y strides over the n images / planes (more than 65535 take further trips), blockIdx.x x 256 threads over the `total` elements of each.
// (Every stage has a batch form: the register cost of the loop nest for the stages that once ran one image only is in profiles/color_stage_resources.txt.)
template <class Stage> __global__ void __launch_bounds__(256) k_px(Stage s, long long total, int n)
{
    for (int img = blockIdx.y; img < n; img += gridDim.y)
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) s(img, q);
}

template <class Stage> static hipError_t launch_px(const Stage &s, long long total, int n, hipStream_t st)
{
    const long long b = (total + 255) / 256;
    const dim3 grid((unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b)), (unsigned)(n > 65535 ? 65535 : n));
    hipLaunchKernelGGL((k_px<Stage>), grid, dim3(256), 0, st, s, total, n);
    return hipGetLastError();
}

// element q of rows of w: its row and column
struct RowCol { int r, c; };
static __device__ __forceinline__ RowCol row_col(long long q, int w)
{
    const int r = (int)(q / w);
    return {r, (int)(q - (long long)r * w)};
}

static __device__ __forceinline__ void cubic_coeffs(float t, float *c)   // Keys cubic, A = -0.75 (OpenCV interpolateCubic)
{
    const float A = -0.75f;
    c[0] = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A;
    c[1] = ((A + 2) * t - (A + 3)) * t * t + 1;
    c[2] = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}
