// w2xc_tta_px.h -- the per-element arithmetic the TTA kernels (w2xc_tta.hip: float planes; w2xc_tta_u8.hip: uint8 images at either end) and the colour
// stages (w2xc_color.hip, w2xc_yuv.hip) share: ONE definition each of where an element lies in a variant, of the gather's sum and of the float -> uint8 rounding.
// Device code only; every file that includes it is built with -ffp-contract=off.
#pragma once

#define TTA_T 32
#define TTA_LD (TTA_T + 1)

// where element (y, x) of the upright h x w plane lies in variant k: upright variants have rows of w, transposed ones rows of h
static __device__ __forceinline__ long long tta_at(int k, int y, int x, int w, int h)
{
    const int xx = (k & 1) ? w - 1 - x : x, yy = (k & 2) ? h - 1 - y : y;
    return (k & 4) ? (long long)xx * h + yy : (long long)yy * w + xx;
}

// element (y, x) of the result from its eight variants' values
static __device__ __forceinline__ float tta_gather_px(const float v[8])
{
    float a = v[0] + v[1];
    a = a + v[2];
    a = a + v[3];
    a = a + v[4];
    a = a + v[5];
    a = a + v[6];
    a = a + v[7];
    return a * 0.125f;
}

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// convertTo(CV_8U, 255) = saturate(cvRound(x * 255)): round half to even
static __device__ __forceinline__ unsigned char to_u8(float x) { return (unsigned char)clampi(__float2int_rn(x * 255.0f), 0, 255); }
