// w2xc_yuv_px.h -- the per-sample arithmetic of the YUV frame kernels that does not depend on the sample width: ONE definition each for the kernels on bytes
// (w2xc_yuv.hip, w2xc_yuv_rgb.hip) and those on 16-bit words (w2xc_yuv16.hip, w2xc_yuv16_rgb.hip) -- the tap sum of the bicubic 2x, chroma at luma resolution,
// the clamp to the models' domain, R, G, B -> y', cb, cr, y' -> a luma sample, the constants of a colour matrix, and the 16-bit sample format (depth, packing) as a
// kernel takes it.  (What the tile kernels share beyond one sample -- geometry, grid, a thread's block -- is w2xc_yuv_tile.h.)
// Every file that includes it is built with -ffp-contract=off.
#pragma once
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8

// the four taps of one row of the neighbourhood, summed in Resize2xCubic's order
static __device__ __forceinline__ float chroma_row_sum(const float *S, const float *c)
{
    float a = S[0] * c[0];
    a = a + S[1] * c[1];
    a = a + S[2] * c[2];
    a = a + S[3] * c[3];
    return a;
}

// 0.75 C[j] + 0.25 C[j']: on samples as floats every operation is exact (multiples of 1/4 and then of 1/16 below 2^16: 20 bits)
static __device__ __forceinline__ float lerp31(float near, float far)
{
    const float a = 0.75f * near;
    const float b = 0.25f * far;
    return a + b;
}

// co-sited chroma (include/w2xc_hip.h, "Chroma siting"): the value halfway between two samples, 0.5 C[j] + 0.5 C[j + 1] -- exact on samples as floats
static __device__ __forceinline__ float lerp11(float a, float b)
{
    const float x = 0.5f * a;
    const float y = 0.5f * b;
    return x + y;
}
// ... and the 1-2-1 mean around a luma sample m with its neighbours l and r: the sum, two exact scalings, one sum
static __device__ __forceinline__ float mean121(float l, float m, float r)
{
    const float a = (l + r) * 0.25f;
    const float b = m * 0.5f;
    return a + b;
}

static __device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

struct YCC { float y, cb, cr; };
static __device__ __forceinline__ YCC to_ycc(const W2xcRgbToYuv &m, float R, float G, float B)
{
    const float a = m.Kr * R;
    const float b = m.Kg * G;
    const float c = m.Kb * B;
    YCC o;
    o.y = (a + b) + c;
    o.cb = (B - o.y) * m.iBU;
    o.cr = (R - o.y) * m.iRV;
    return o;
}

// ---- 16-bit samples: a value of `depth` bits in a 16-bit word, in its low bits (pack 0) or its high bits (pack 1) ----
// word -> value: (word >> rshift) & max (LOW: the high bits are masked; HIGH: the low bits are shifted out)
static __device__ __forceinline__ unsigned u16_value(unsigned word, int rshift, unsigned max) { return (word >> rshift) & max; }
// saturate(rint(x * scale + offset)) to [0, max], half to even, the product and the sum two operations; __float2int_rn saturates, so the clamp holds past int32
static __device__ __forceinline__ unsigned to_u16(float x, float scale, float offset, int max) { return (unsigned)clampi(__float2int_rn(x * scale + offset), 0, max); }
// ... without an offset: saturate(rint(x * scale))
static __device__ __forceinline__ unsigned to_u16(float x, float scale, int max) { return (unsigned)clampi(__float2int_rn(x * scale), 0, max); }

// ---- y -> a luma sample, in the stages of the Y route and in the kernels of the RGB route alike ----
// byte: full range to_u8, limited range saturate(rint(y * 219 + 16)), half to even, the product and the sum unfused
static __device__ __forceinline__ unsigned char luma_u8(float y, int limited)
{
    return limited ? (unsigned char)clampi(__float2int_rn(y * 219.0f + 16.0f), 0, 255) : to_u8(y);
}
// cb or cr -> a chroma byte of the RGB route: saturate(rint(c * scale + 128))
static __device__ __forceinline__ unsigned char chroma_u8(float c, float scale) { return (unsigned char)clampi(__float2int_rn(c * scale + 128.0f), 0, 255); }
// value of a word: saturate(rint(y * M)), or saturate(rint(y * (219 s) + 16 s)) for limited range
static __device__ __forceinline__ unsigned luma_u16(float y, int limited, float scale, float off, int max)
{
    return limited ? to_u16(y, scale, off, max) : to_u16(y, scale, max);
}

// ---- host: the constants of a matrix, doubles from the two luma weights, each rounded once to float (the header lists the expressions) ----
static inline bool matrix_weights(int matrix, double *Kr, double *Kb)
{
    switch (matrix) {
    case 0: *Kr = 0.299; *Kb = 0.114; return true;      // W2XC_MATRIX_BT601
    case 1: *Kr = 0.2126; *Kb = 0.0722; return true;    // W2XC_MATRIX_BT709
    case 2: *Kr = 0.2627; *Kb = 0.0593; return true;    // W2XC_MATRIX_BT2020
    }
    return false;
}
static inline bool matrix_to_rgb(int matrix, W2xcYuvToRgb *m)
{
    double Kr, Kb;
    if (!matrix_weights(matrix, &Kr, &Kb)) return false;
    const double Kg = 1.0 - Kr - Kb, cRV = 2.0 * (1.0 - Kr), cBU = 2.0 * (1.0 - Kb);
    *m = {(float)cRV, (float)cBU, (float)(Kr * cRV / Kg), (float)(Kb * cBU / Kg)};
    return true;
}
static inline bool matrix_from_rgb(int matrix, W2xcRgbToYuv *m)
{
    double Kr, Kb;
    if (!matrix_weights(matrix, &Kr, &Kb)) return false;
    const double Kg = 1.0 - Kr - Kb, cRV = 2.0 * (1.0 - Kr), cBU = 2.0 * (1.0 - Kb);
    *m = {(float)Kr, (float)Kg, (float)Kb, (float)(1.0 / cBU), (float)(1.0 / cRV)};
    return true;
}

// every row of every float plane starts on an 8-byte boundary: a thread's two adjacent pixels are one 8-byte access
static inline int rows_8_aligned(const float *rgb, long long is, long long ps, int w, int n)
{
    return ((reinterpret_cast<size_t>(rgb) & 7) == 0 && (w & 1) == 0 && (ps & 1) == 0 && (n == 1 || (is & 1) == 0)) ? 1 : 0;
}

// a `chroma` value of the RGB route as the interface takes it: the layout (4:2:0, 4:2:2, 4:4:4) with the siting flags W2XC_CHROMA_COSITED_X 0x10 / _Y 0x20 or-ed
// on, or with none.  False for another bit, another layout, or a flag on an axis the layout does not subsample (the interface's rule, check_chroma_range in
// w2xc_image_yuv.cpp, refuses the same with a message): a launcher that decodes its `chroma` here honours every flag it accepts
struct ChromaLayout {
    int layout;
    bool cx, cy;
};
static inline bool chroma_layout(int chroma, ChromaLayout *c)
{
    if (chroma < 0 || (chroma & ~0x3F)) return false;
    *c = {chroma & 0xF, (chroma & 0x10) != 0, (chroma & 0x20) != 0};
    return c->layout == 0 || (c->layout == 1 && !c->cy) || (c->layout == 2 && !c->cx && !c->cy);
}
// the chroma planes of a w x h frame of that layout (the siting does not change a size)
static inline bool frame_geometry(int w, int h, int layout, int *cw, int *ch)
{
    if (w < 1 || h < 1 || layout < 0 || layout > 2) return false;
    *cw = layout != 2 ? (w + 1) / 2 : w;
    *ch = layout == 0 ? (h + 1) / 2 : h;
    return true;
}

// the scales and offsets of a depth (D bits, s = 2^(D - 8), M = 2^D - 1) and a range, computed in double and rounded once to float
struct W2xcU16Scale {
    int max;                 // M
    float y_off, y_in;       // luma in:  ((float)Y - y_off) * y_in      (full range: y_off = 0, Y * y_in)
    float y_out;             // luma out: y * y_out + y_off
    float c_mid, c_in;       // chroma of the RGB route in: (c - c_mid) * c_in;  out: c * c_out + c_mid
    float c_out;
    float inv_max, fmax;     // chroma of the Y route: (float)C * inv_max, c * fmax
};
static inline W2xcU16Scale u16_scale(int depth, int limited)
{
    const double s = (double)(1 << (depth - 8)), M = (double)((1 << depth) - 1);
    W2xcU16Scale k;
    k.max = (1 << depth) - 1;
    k.y_off = limited ? (float)(16.0 * s) : 0.0f;
    k.y_in = limited ? (float)(1.0 / (219.0 * s)) : (float)(1.0 / M);
    k.y_out = limited ? (float)(219.0 * s) : (float)M;
    k.c_mid = (float)(128.0 * s);
    k.c_in = limited ? (float)(1.0 / (224.0 * s)) : (float)(1.0 / M);
    k.c_out = limited ? (float)(224.0 * s) : (float)M;
    k.inv_max = (float)(1.0 / M);
    k.fmax = (float)M;
    return k;
}
