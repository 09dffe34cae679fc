// w2xc_yuv_launch.h -- the host side of the YUV tile kernels that more than one kernel file needs.  Each of the six tile kernels has ONE launcher, in the file of
// its centred instantiations (w2xc_yuv.hip, w2xc_yuv16.hip, w2xc_yuv_rgb.hip, w2xc_yuv16_rgb.hip): it checks its arguments and computes grid, load path and
// constants once, then launches a centred instantiation where no siting flag is set and otherwise the co-sited one that the selector of the *_sited.hip file
// hands it -- the host stub of a __global__ function is an ordinary function inside the one library, so its pointer launches from any file.
//   the parameter list of each kernel, written once for the centred definition, the co-sited one and the pointer type
//   the selectors of the co-sited instantiations
//   the chroma prologue of a sample width: what the 2x launcher and the resize launcher (w2xc_yuv_sized.hip, w2xc_yuv16_sized.hip) check and decide alike
#pragma once
#include "w2xc_kernels.h"
#include "w2xc_yuv_px.h"   // u16_scale
#include "w2xc_yuv_tile.h" // rows_align

// ---- the kernels' parameter lists ----
#define W2XC_CHROMA2X_U8_PARAMS                                                                                                                                    \
    const unsigned char *su, const unsigned char *sv, long long sframe, long long srow, int spx, int cw, int ch, unsigned char *du, unsigned char *dv,           \
        long long dframe, long long drow, int dpx, int ow, int oh, int npl, int tiles_x, long long tiles, long long turns
#define W2XC_CHROMA2X_U16_PARAMS                                                                                                                                   \
    const unsigned short *su, const unsigned short *sv, long long sframe, long long srow, int spx, int cw, int ch, int rshift, int max, unsigned short *du,       \
        unsigned short *dv, long long dframe, long long drow, int dpx, int lshift, int pair, int ow, int oh, int npl, float inv_max, float fmax, int tiles_x,     \
        long long tiles, long long turns
#define W2XC_YUV8_TO_RGB_PARAMS                                                                                                                                    \
    const unsigned char *__restrict__ sy, long long yframe, long long yrow, const unsigned char *__restrict__ su, const unsigned char *__restrict__ sv,           \
        long long cframe, long long crow, int spx, int w, int h, int cw, int ch, int limited, W2xcYuvToRgb m, float *__restrict__ rgb, long long is, long long ps, \
        int v2, int tiles_x, long long tiles, long long turns
#define W2XC_RGB_TO_YUV8_PARAMS                                                                                                                                    \
    const float *__restrict__ rgb, long long is, long long ps, int v2, int w, int h, int cw, int ch, int limited, W2xcRgbToYuv m, unsigned char *__restrict__ dy, \
        long long yframe, long long yrow, int y16, unsigned char *__restrict__ du, unsigned char *__restrict__ dv, long long cframe, long long crow, int dpx,     \
        int tiles_x, long long tiles, long long turns
#define W2XC_YUV16_TO_RGB_PARAMS                                                                                                                                   \
    const unsigned short *__restrict__ sy, long long yframe, long long yrow, int yv, int yshift, const unsigned short *__restrict__ su,                           \
        const unsigned short *__restrict__ sv, long long cframe, long long crow, int spx, int cshift, int max, int w, int h, int cw, int ch, float y0, float ky,  \
        float c0, float kc, W2xcYuvToRgb m, float *__restrict__ rgb, long long is, long long ps, int v2, int tiles_x, long long tiles, long long turns
#define W2XC_RGB_TO_YUV16_PARAMS                                                                                                                                   \
    const float *__restrict__ rgb, long long is, long long ps, int v2, int w, int h, int cw, int ch, int limited, int max, float ys, float y0, float cs, float c0, \
        W2xcRgbToYuv m, unsigned short *__restrict__ dy, long long yframe, long long yrow, int y32, int yshift, unsigned short *__restrict__ du,                  \
        unsigned short *__restrict__ dv, long long cframe, long long crow, int dpx, int uv32, int cshift, int tiles_x, long long tiles, long long turns

using Chroma2xU8Kernel = void (*)(W2XC_CHROMA2X_U8_PARAMS);
using Chroma2xU16Kernel = void (*)(W2XC_CHROMA2X_U16_PARAMS);
using Yuv8ToRgbKernel = void (*)(W2XC_YUV8_TO_RGB_PARAMS);
using RgbToYuv8Kernel = void (*)(W2XC_RGB_TO_YUV8_PARAMS);
using Yuv16ToRgbKernel = void (*)(W2XC_YUV16_TO_RGB_PARAMS);
using RgbToYuv16Kernel = void (*)(W2XC_RGB_TO_YUV16_PARAMS);

// ---- the co-sited instantiations (the *_sited.hip files): cx || cy; dw / load / cm is the launcher's load path; the RGB route's layout and flags are a pair
// chroma_layout (w2xc_yuv_px.h) has let through -- 4:2:0 with x, y or both, 4:2:2 with x ----
Chroma2xU8Kernel chroma2x_u8_sited_kernel(bool dw, bool cx, bool cy);
Chroma2xU16Kernel chroma2x_u16_sited_kernel(int load, bool cx, bool cy);
Yuv8ToRgbKernel yuv8_to_rgb_sited_kernel(bool dw, int layout, bool cx, bool cy);
RgbToYuv8Kernel rgb_to_yuv8_sited_kernel(int layout, bool cx, bool cy);
Yuv16ToRgbKernel yuv16_to_rgb_sited_kernel(int cm, int layout, bool cx, bool cy);
RgbToYuv16Kernel rgb_to_yuv16_sited_kernel(int layout, bool cx, bool cy);
// the instantiation of K(SX, SY, CX, CY) for such a pair
#define W2XC_SITED_KERNEL(K, layout, cx, cy) \
    ((layout) == 1 ? K(true, false, true, false) : (cx) && (cy) ? K(true, true, true, true) : (cx) ? K(true, true, true, false) : K(true, true, false, true))

// ---- the chroma prologue: the planes su (and sv: nullptr = one plane per frame) of cw x ch samples of n frames -> ow x oh samples at du (and dv) ----
// false: an argument no chroma launcher takes (each adds its own: the 2x bound, the axes of the resize)
template <class Planes, class Sample>
static inline bool chroma_args(const Planes &su, const Sample *sv, int cw, int ch, const Planes &du, const Sample *dv, int ow, int oh, int n)
{
    return cw >= 1 && ch >= 1 && ow >= 1 && oh >= 1 && n >= 1 && (su.px == 1 || su.px == 2) && (du.px == 1 || du.px == 2) && su.p && du.p &&
           (sv != nullptr) == (dv != nullptr);
}
// bytes.  dw: planar source planes whose rows start on 4-byte boundaries -- the dword loader
static inline bool chroma_prologue_u8(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, const unsigned char *dv, int ow, int oh, int n, int *npl,
                                bool *dw)
{
    if (!chroma_args(su, sv, cw, ch, du, dv, ow, oh, n)) return false;
    *npl = sv ? 2 : 1;
    *dw = su.px == 1 && ((rows_align(su, n) | (sv ? reinterpret_cast<size_t>(sv) : 0)) & 3) == 0;
    return true;
}
// words.  load 1: planar source planes whose rows start on 8-byte boundaries; 2: sv = su + 1 and rows on 4-byte boundaries; 0: sample by sample.  pair: dv = du + 1
// and rows on 4-byte boundaries -- a (U, V) pair is one 32-bit store.  The shifts of the two sides' packings and the scales of the depth
struct ChromaU16 {
    int npl, load, pair, rshift, lshift;
    W2xcU16Scale k;
};
static inline bool chroma_prologue_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, const unsigned short *dv, int ow, int oh, int depth, int n,
                                ChromaU16 *c)
{
    if (!chroma_args(su, sv, cw, ch, du, dv, ow, oh, n) || depth < 8 || depth > 16) return false;
    const size_t salign = rows_align(su, n), dalign = rows_align(du, n);
    c->npl = sv ? 2 : 1;
    c->load = 0;
    if (su.px == 1 && ((salign | (sv ? reinterpret_cast<size_t>(sv) : 0)) & 7) == 0) c->load = 1;
    else if (su.px == 2 && sv == su.p + 1 && (salign & 3) == 0) c->load = 2;
    c->pair = du.px == 2 && dv == du.p + 1 && (dalign & 3) == 0;
    c->rshift = su.pack ? 16 - depth : 0;
    c->lshift = du.pack ? 16 - depth : 0;
    c->k = u16_scale(depth, 0);
    return true;
}
// `cosited` of the 2x launchers: 0 or W2XC_CHROMA_COSITED_X | _Y
static inline bool cosited_ok(int cosited) { return (cosited & ~(W2XC_CHROMA_COSITED_X | W2XC_CHROMA_COSITED_Y)) == 0; }
