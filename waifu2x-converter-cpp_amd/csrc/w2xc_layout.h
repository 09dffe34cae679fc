// w2xc_layout.h -- the constants a kernel and the packer of its weight image (w2xc_pack.cpp) must agree on.  No HIP header: the kernels include it
// under hipcc, the packers under any C++17 compiler.
#pragma once

#ifdef __HIP__
#define W2XC_HD __host__ __device__
#else
#define W2XC_HD
#endif

// conv3x3_direct: output planes per thread = the padding unit of its weight image [cin][9][cout padded]
constexpr int DIRECT_CG = 8;
static constexpr W2XC_HD int direct_cout_pad(int cout) { return (cout + DIRECT_CG - 1) / DIRECT_CG * DIRECT_CG; }

// MFMA fragment geometry: a wave is 64 lanes; a 32x32 tile is lane = 32 k + row, a 16x16 tile lane = 16 k + row
constexpr int W2XC_WAVE = 64;
// positions xi of the transformed domain = independent GEMMs per block: F(2x2,3x3) on 4x4 patches, F(4x4,3x3) on 6x6 patches
constexpr int W2XC_WINO_XI = 16, W2XC_WINO4_XI = 36;

// conv3x3_wino4: position (i, j) of the transformed domain in the fragment order: the column halves j < 3 / j >= 3 as the xi ranges [0, 18) / [18, 36)
static constexpr W2XC_HD int xi_of(int i, int j) { return j < 3 ? 3 * i + j : 18 + 3 * i + (j - 3); }
