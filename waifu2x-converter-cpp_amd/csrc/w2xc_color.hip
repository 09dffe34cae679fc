// w2xc_color.hip -- row N2 of SURVEY.md 8f: the colour front/back end and the U/V resize of the reference
// CLI's scale loop (/root/reference/src/main.cpp:74-76,136,144,171-172), so that the whole scale phase of
// one image runs device-resident.  All kernels are HBM-streaming (a few bytes per pixel) and keep
// OpenCV's float evaluation order with unfused mul/add (the file is built with -ffp-contract=off).
// Every stage is ONE struct on the per-pixel skeleton of w2xc_px.h: k_px holds the loops over images and elements, launch_px the grid and the launch.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8: shared with w2xc_tta_u8.hip
#include "w2xc_px.h"       // k_px, launch_px, row_col, cubic_coeffs: shared with w2xc_yuv.hip

// main.cpp:75-76 (+ cv::split): convertTo(CV_32F, 1/255) and COLOR_RGB2YUV on the channels AS GIVEN
// (the reference feeds imread's BGR order, Q3): Y = .299 c0 + .587 c1 + .114 c2, U = (c2-Y)*.492+.5, V = (c0-Y)*.877+.5
// n images, image i at src + i * img_stride bytes; its planes at y / u / v + i * ps floats
struct U8ToYuv {
    const unsigned char *src;
    long long img_stride, stride;
    int w;
    float *y, *u, *v;
    long long ps;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const float s = (float)(1.0 / 255.0);
        const RowCol at = row_col(q, w);
        const unsigned char *p = src + img * img_stride + at.r * stride + (long long)at.c * 3;
        const float c0 = (float)p[0] * s, c1 = (float)p[1] * s, c2 = (float)p[2] * s;
        float Y = c0 * 0.299f;
        Y = Y + c1 * 0.587f;
        Y = Y + c2 * 0.114f;
        const long long o = img * ps + q;
        y[o] = Y;
        u[o] = (c2 - Y) * 0.492f + 0.5f;
        v[o] = (c0 - Y) * 0.877f + 0.5f;
    }
};
hipError_t w2xc_launch_u8_to_yuv_batch(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *y, float *u, float *v,
                                       long long ps, int n, hipStream_t st)
{
    return launch_px(U8ToYuv{src, (long long)img_stride, (long long)stride, w, y, u, v, ps}, (long long)w * h, n, st);
}
hipError_t w2xc_launch_u8_to_yuv(const unsigned char *src, size_t stride, int w, int h, float *y, float *u, float *v, hipStream_t st)
{
    return w2xc_launch_u8_to_yuv_batch(src, 0, stride, w, h, y, u, v, 0, 1, st);
}

// main.cpp:171-172 (+ cv::merge): COLOR_YUV2RGB and convertTo(CV_8U, 255)
// n images: planes of image i at y / u / v + i * ps floats, its pixels at dst + i * img_stride bytes
struct YuvToU8 {
    const float *y, *u, *v;
    long long ps;
    int w;
    unsigned char *dst;
    long long img_stride, stride;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const long long o = img * ps + q;
        const float Y = y[o], U = u[o] - 0.5f, V = v[o] - 0.5f;
        float ch[3];
        ch[2] = Y + U * 2.032f;
        ch[1] = (Y + U * -0.395f) + V * -0.581f;
        ch[0] = Y + V * 1.140f;
        unsigned char *p = dst + img * img_stride + at.r * stride + (long long)at.c * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = to_u8(ch[k]);
    }
};
hipError_t w2xc_launch_yuv_to_u8_batch(const float *y, const float *u, const float *v, long long ps, int w, int h, unsigned char *dst, size_t img_stride,
                                       size_t stride, int n, hipStream_t st)
{
    return launch_px(YuvToU8{y, u, v, ps, w, dst, (long long)img_stride, (long long)stride}, (long long)w * h, n, st);
}
hipError_t w2xc_launch_yuv_to_u8(const float *y, const float *u, const float *v, int w, int h, unsigned char *dst, size_t stride, hipStream_t st)
{
    return w2xc_launch_yuv_to_u8_batch(y, u, v, 0, w, h, dst, 0, stride, 1, st);
}

// The RGB image pipeline (w2xc_process_image_rgb_u8*; no counterpart in v1 of the reference): x = u8 / 255 on the three channels as given, and
// back out = saturate(rint(255 x)) -- the two expressions of U8ToYuv / YuvToU8 without the colour matrix, and the ones the uint8 forms of
// conv3x3_first / conv3x3_last (w2xc_kernels.hip) evaluate in their load / store.  Three planar float planes p0 / p1 / p2, those of image i `is` floats on.
struct U8ToRgb {
    const unsigned char *src;
    long long img_stride, stride;
    int w;
    float *p0, *p1, *p2;
    long long is;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const float s = (float)(1.0 / 255.0);
        const RowCol at = row_col(q, w);
        const unsigned char *p = src + img * img_stride + at.r * stride + (long long)at.c * 3;
        const long long o = img * is + q;
        p0[o] = (float)p[0] * s;
        p1[o] = (float)p[1] * s;
        p2[o] = (float)p[2] * s;
    }
};
// the three planes of image i at planes + i * is + {0, 1, 2} * ps floats
hipError_t w2xc_launch_u8_to_rgb_batch(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *planes, long long ps, long long is,
                                       int n, hipStream_t st)
{
    return launch_px(U8ToRgb{src, (long long)img_stride, (long long)stride, w, planes, planes + ps, planes + 2 * ps, is}, (long long)w * h, n, st);
}
hipError_t w2xc_launch_u8_to_rgb(const unsigned char *src, size_t stride, int w, int h, float *p0, float *p1, float *p2, hipStream_t st)
{
    return launch_px(U8ToRgb{src, 0, (long long)stride, w, p0, p1, p2, 0}, (long long)w * h, 1, st);
}

struct RgbToU8 {
    const float *p0, *p1, *p2;
    long long is;
    int w;
    unsigned char *dst;
    long long img_stride, stride;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const long long o = img * is + q;
        unsigned char *p = dst + img * img_stride + at.r * stride + (long long)at.c * 3;
        p[0] = to_u8(p0[o]);
        p[1] = to_u8(p1[o]);
        p[2] = to_u8(p2[o]);
    }
};
hipError_t w2xc_launch_rgb_to_u8_batch(const float *planes, long long ps, long long is, int w, int h, unsigned char *dst, size_t img_stride, size_t stride,
                                       int n, hipStream_t st)
{
    return launch_px(RgbToU8{planes, planes + ps, planes + 2 * ps, is, w, dst, (long long)img_stride, (long long)stride}, (long long)w * h, n, st);
}
hipError_t w2xc_launch_rgb_to_u8(const float *p0, const float *p1, const float *p2, int w, int h, unsigned char *dst, size_t stride, hipStream_t st)
{
    return launch_px(RgbToU8{p0, p1, p2, 0, w, dst, 0, (long long)stride}, (long long)w * h, 1, st);
}

// main.cpp:144 on one plane: cv::resize(2x, INTER_CUBIC): horizontal pass to float, then vertical pass,
// taps sx-1..sx+2 clipped to the image.  One thread per output pixel (4 x 4 source taps from L2/L1).
// n planes (the U and the V planes of a sub-batch, adjacent): plane p at src + p * sps, its 2x plane at dst + p * dps (floats)
struct Resize2xCubic {
    const float *src;
    long long sps;
    int w, h;
    float *dst;
    long long dps;
    __device__ __forceinline__ void operator()(int p, long long q) const
    {
        const float *s = src + p * sps;
        const RowCol d = row_col(q, 2 * w);
        const int dy = d.r, dx = d.c;
        const float fx = (float)((dx + 0.5) * 0.5 - 0.5), fy = (float)((dy + 0.5) * 0.5 - 0.5);
        const int sx = (int)floorf(fx), sy = (int)floorf(fy);
        float cx[4], cy[4];
        cubic_coeffs(fx - sx, cx);
        cubic_coeffs(fy - sy, cy);
        int xs[4];
#pragma unroll
        for (int k = 0; k < 4; k++) xs[k] = clampi(sx - 1 + k, 0, w - 1);
        float rowv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float *S = s + (long long)clampi(sy - 1 + j, 0, h - 1) * w;
            float a = S[xs[0]] * cx[0];
            a = a + S[xs[1]] * cx[1];
            a = a + S[xs[2]] * cx[2];
            a = a + S[xs[3]] * cx[3];
            rowv[j] = a;
        }
        float a = rowv[0] * cy[0];
        a = a + rowv[1] * cy[1];
        a = a + rowv[2] * cy[2];
        a = a + rowv[3] * cy[3];
        dst[p * dps + q] = a;
    }
};
hipError_t w2xc_launch_resize2x_cubic_batch(const float *src, long long sps, int w, int h, float *dst, long long dps, int n, hipStream_t st)
{
    return launch_px(Resize2xCubic{src, sps, w, h, dst, dps}, 4LL * w * h, n, st);
}
hipError_t w2xc_launch_resize2x_cubic(const float *src, int w, int h, float *dst, hipStream_t st) { return w2xc_launch_resize2x_cubic_batch(src, 0, w, h, dst, 0, 1, st); }

// main.cpp:158-167 on one plane: cv::resize(Size(dw, dh), INTER_LINEAR): half-pixel centres, the two taps
// clipped to the image, horizontal pass to float then vertical pass (no antialiasing, like OpenCV).
// n planes (Y, U and V of a sub-batch): the first ny planes at src_y + p * sps (the Y planes: after a noise pass they do not adjoin U), plane p >= ny at
// src_uv + (p - ny) * sps; destination plane p at dst + p * dps (floats)
struct ResizeLinear {
    const float *src_y, *src_uv;
    int ny;
    long long sps;
    int sw, sh;
    float *dst;
    long long dps;
    int dw;
    double scale_x, scale_y;
    __device__ __forceinline__ void operator()(int p, long long q) const
    {
        const float *src = p < ny ? src_y + p * sps : src_uv + (p - ny) * sps;
        const RowCol d = row_col(q, dw);
        const int dy = d.r, dx = d.c;
        float fx = (float)((dx + 0.5) * scale_x - 0.5), fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sx = (int)floorf(fx), sy = (int)floorf(fy);
        fx -= sx;
        fy -= sy;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        if (sy < 0) { fy = 0; sy = 0; }
        if (sy >= sh - 1) { fy = 0; sy = sh - 1; }
        const int sx1 = sx + 1 < sw ? sx + 1 : sw - 1, sy1 = sy + 1 < sh ? sy + 1 : sh - 1;
        const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
        const float *R0 = src + (long long)sy * sw, *R1 = src + (long long)sy1 * sw;
        float h0 = R0[sx] * a0;
        h0 = h0 + R0[sx1] * a1;
        float h1 = R1[sx] * a0;
        h1 = h1 + R1[sx1] * a1;
        float a = h0 * b0;
        a = a + h1 * b1;
        dst[p * dps + q] = a;
    }
};
hipError_t w2xc_launch_resize_linear_batch(const float *src_y, const float *src_uv, int ny, long long sps, int sw, int sh, float *dst, long long dps, int dw,
                                           int dh, int n, hipStream_t st)
{
    return launch_px(ResizeLinear{src_y, src_uv, ny, sps, sw, sh, dst, dps, dw, (double)sw / dw, (double)sh / dh}, (long long)dw * dh, n, st);
}
hipError_t w2xc_launch_resize_linear(const float *src, int sw, int sh, float *dst, int dw, int dh, hipStream_t st)
{
    return w2xc_launch_resize_linear_batch(src, src, 1, 0, sw, sh, dst, 0, dw, dh, 1, st);
}

// ---- RGBA images (w2xc_process_image_rgba_u8*; no counterpart in v1 of the reference): n images per launch, one image is n = 1 ----
// Colour bleed: a transparent pixel (alpha == 0) beside opaque ones takes the rounded mean of its opaque 3x3 neighbours, (2 sum + n) / (2 n) per channel,
// and counts as opaque in the next pass; P passes carry the colour P pixels into the transparent region.  The passes are defined as a ping-pong (a pass
// reads only what the pass before left); they run IN PLACE on the packed 3-channel image, exactly, because a pixel filled in pass k (its stamp: 0 = opaque in
// the source, k = filled in pass k, BLEED_FAR = not reached) reads only neighbours whose stamp is below k, and those are written by no thread of pass k; a
// neighbour's stamp that is being set to k reads as BLEED_FAR or as k, neither of them below k.
// Two forms: 2 to W2XC_BLEED_TILED_MAX passes run in ONE launch, a workgroup per tile with the passes between LDS words (k_bleed_tiled); more passes are the
// chain RgbaBleedFirst, RgbaBleedPass x (P - 1) on a 16-bit stamp plane in memory, and one pass is RgbaBleedFirst alone, without stamps.  The bytes are the same.
#define BLEED_FAR 0xFFFFu

// which neighbours count: the opaque pixels of the RGBA source (pass 1), the pixels stamped below k (pass k)
struct AlphaSet {
    const unsigned char *src;
    long long stride;
    __device__ __forceinline__ bool operator()(int rr, int cc) const { return src[rr * stride + (long long)cc * 4 + 3] != 0; }
};
struct StampBelow {
    const unsigned short *stamp;
    int w;
    unsigned k;
    __device__ __forceinline__ bool operator()(int rr, int cc) const { return stamp[(long long)rr * w + cc] < k; }
};

// the 3x3 neighbours of (r, c) inside the w x h image for which counts(row, column) holds: how many, and the sums of their three channels (px bytes per pixel)
struct BleedSum {
    int n, s0, s1, s2;
    __device__ __forceinline__ int mean(int s) const { return (2 * s + n) / (2 * n); }
};
template <class Counts> static __device__ __forceinline__ BleedSum bleed_sum(const unsigned char *img, long long stride, int px, int w, int h, int r, int c, Counts counts)
{
    BleedSum b = {0, 0, 0, 0};
    for (int dy = -1; dy <= 1; dy++) {
        const int rr = r + dy;
        if (rr < 0 || rr >= h) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int cc = c + dx;
            if (cc < 0 || cc >= w || !counts(rr, cc)) continue;
            const unsigned char *nb = img + rr * stride + (long long)cc * px;
            b.n++; b.s0 += nb[0]; b.s1 += nb[1]; b.s2 += nb[2];
        }
    }
    return b;
}

// writes pixel q of the packed image, its stamp (where there is a stamp plane: the plain repack, first_pass = 0, needs none), and -- with first_pass --
// pass 1, read from the RGBA source's own alpha.  Image i: src + i * img_stride, dst + i * dst_img_stride bytes, stamp + i * stamp_stride words
struct RgbaBleedFirst {
    const unsigned char *src;
    long long img_stride, stride;
    int w, h, first_pass;
    unsigned char *dst;
    long long dst_img_stride, dst_stride;
    unsigned short *stamp;
    long long stamp_stride;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const unsigned char *s = src + img * img_stride;
        const unsigned char *p = s + at.r * stride + (long long)at.c * 4;
        int o0 = p[0], o1 = p[1], o2 = p[2];
        unsigned st = p[3] ? 0u : BLEED_FAR;
        if (st && first_pass) {
            const BleedSum b = bleed_sum(s, stride, 4, w, h, at.r, at.c, AlphaSet{s, stride});
            if (b.n) { o0 = b.mean(b.s0); o1 = b.mean(b.s1); o2 = b.mean(b.s2); st = 1u; }
        }
        unsigned char *d = dst + img * dst_img_stride + at.r * dst_stride + (long long)at.c * 3;
        d[0] = (unsigned char)o0; d[1] = (unsigned char)o1; d[2] = (unsigned char)o2;
        if (stamp) stamp[img * stamp_stride + q] = (unsigned short)st;
    }
};

// pass k >= 2, in place (see above)
struct RgbaBleedPass {
    unsigned char *img;
    long long img_stride, stride;
    int w, h;
    unsigned k;
    unsigned short *stamp;
    long long stamp_stride;
    __device__ __forceinline__ void operator()(int i, long long q) const
    {
        unsigned short *sp = stamp + i * stamp_stride;
        if (sp[q] != BLEED_FAR) return;
        unsigned char *im = img + i * img_stride;
        const RowCol at = row_col(q, w);
        const BleedSum b = bleed_sum(im, stride, 3, w, h, at.r, at.c, StampBelow{sp, w, k});
        if (!b.n) return;
        unsigned char *d = im + at.r * stride + (long long)at.c * 3;
        d[0] = (unsigned char)b.mean(b.s0);
        d[1] = (unsigned char)b.mean(b.s1);
        d[2] = (unsigned char)b.mean(b.s2);
        sp[q] = (unsigned short)k;
    }
};

// The tiled form: all P <= BLEED_L passes of one BLEED_T x BLEED_T tile of one image in one workgroup.  The tile and a halo of P pixels live in LDS as one
// 32-bit word per pixel -- the three colour bytes and, on top, an 8-bit stamp: 0 = opaque in the source, k = filled in pass k, TILE_FAR = not reached,
// TILE_OUT = outside the image (never a neighbour, never filled) -- in rows of BLEED_R words, so the lanes of a wave read consecutive banks.
// The halo suffices: a pixel filled in pass k depends only on pixels within Chebyshev distance k, so a region pixel at distance d from the tile has to be
// right through pass P - d only, and its (P - d)-neighbourhood lies inside the region: pass k covers the rows and columns [k, R - k) of the region's R =
// T + 2 P, and reads [k - 1, R - k + 1).  In place for the reason above, between LDS words: a pass reads only neighbours stamped below k, which no thread of
// pass k writes, and a word that is being written reads as the old one (TILE_FAR) or the new one (k), neither below k.
// A pass that fills nothing in its part of the region ends the tile's passes -- then no later pass can fill anything there (a pixel still TILE_FAR has no
// neighbour stamped below k, and none was stamped k) -- and so does a tile without a transparent pixel; both are decisions of the whole workgroup.
#define BLEED_T 32
#define BLEED_L W2XC_BLEED_TILED_MAX
#define BLEED_R (BLEED_T + 2 * BLEED_L)
#define TILE_FAR 0xFEu
#define TILE_OUT 0xFFu
static_assert(BLEED_L >= 14 && BLEED_L <= 253 && BLEED_R == 64 && BLEED_R * BLEED_R * 4 <= 64 * 1024, "the tile region: 64 x 64 words, 256 threads = 4 rows");

// BleedSum::mean, (2 s + n) / (2 n), for n = 1..8 neighbours and s <= 255 n without a division: x / d = (x * ceil(2^16 / d)) >> 16 exactly while x * (d ceil(2^16 / d)
// - 2^16) < 2^16, and x <= 4088, d <= 16 gives at most 4088 * 15.  The eight multipliers, 16 bits each.
static __device__ __forceinline__ unsigned tile_mean(unsigned s, unsigned n)
{
    const unsigned long long m = n <= 4 ? 0x20002aab40008000ull : 0x1000124a1556199aull;
    return ((2 * s + n) * ((unsigned)(m >> (16 * ((n - 1) & 3))) & 0xFFFFu)) >> 16;
}

// blockIdx.x strides over the tiles of an image, blockIdx.y over the n images (k_px's loops); thread t = column t & 63 of the region, in rows that depend on t >> 6
__global__ void __launch_bounds__(256) k_bleed_tiled(const unsigned char *src, long long img_stride, long long stride, int w, int h, int passes,
                                                     unsigned char *dst, long long dst_img_stride, long long dst_stride, int tiles_x, long long tiles, int n)
{
    __shared__ unsigned px[BLEED_R * BLEED_R];
    __shared__ int live[BLEED_L + 1];   // [0]: the tile holds a transparent pixel; [k]: pass k filled a pixel
    const int P = passes, R = BLEED_T + 2 * P;
    const int tx = threadIdx.x & (BLEED_R - 1), ty = threadIdx.x >> 6;
    for (int img = blockIdx.y; img < n; img += gridDim.y) {
        const unsigned char *s = src + img * img_stride;
        unsigned char *d = dst + img * dst_img_stride;
        const bool words = ((reinterpret_cast<unsigned long long>(s) | (unsigned long long)stride) & 3) == 0;   // (uniform: 4-byte pixels as one load)
        for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const int y0 = (int)(tile / tiles_x) * BLEED_T, x0 = (int)(tile % tiles_x) * BLEED_T;
            if (threadIdx.x <= BLEED_L) live[threadIdx.x] = 0;
            __syncthreads();   // (also: the tile before has left the LDS words)
            const int gx = x0 - P + tx;
            if (tx < R) for (int ry = ty; ry < R; ry += 4) {
                const int gy = y0 - P + ry;
                unsigned v = TILE_OUT << 24;
                if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                    const unsigned char *p = s + gy * stride + (long long)gx * 4;
                    if (words) v = *reinterpret_cast<const unsigned *>(p);
                    else v = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
                    v = (v & 0xFFFFFFu) | (v >> 24 ? 0u : TILE_FAR << 24);
                    if (v >> 24 && tx >= P && tx < P + BLEED_T && ry >= P && ry < P + BLEED_T) live[0] = 1;
                }
                px[ry * BLEED_R + tx] = v;
            }
            __syncthreads();
            if (live[0]) for (int k = 1; k <= P; k++) {
                // a thread walks its column down a quarter of the pass's rows with the 3 x 3 window in registers: three words a row, and the row below is
                // on its way while this one is summed.  A word read before another thread restamped it reads as TILE_FAR: not below k either way.
                const int rows = (R - 2 * k + 3) >> 2, r0 = k + ty * rows, r1 = r0 + rows < R - k ? r0 + rows : R - k;
                if (tx >= k && tx < R - k && r0 < r1) {
                    const unsigned *col = px + tx;
                    unsigned a0 = col[(r0 - 1) * BLEED_R - 1], a1 = col[(r0 - 1) * BLEED_R], a2 = col[(r0 - 1) * BLEED_R + 1];
                    unsigned b0 = col[r0 * BLEED_R - 1], b1 = col[r0 * BLEED_R], b2 = col[r0 * BLEED_R + 1];
                    for (int ry = r0; ry < r1; ry++) {
                        const unsigned c0 = col[(ry + 1) * BLEED_R - 1], c1 = col[(ry + 1) * BLEED_R], c2 = col[(ry + 1) * BLEED_R + 1];
                        if (b1 >> 24 == TILE_FAR) {
                            const unsigned nb[8] = {a0, a1, a2, b0, b2, c0, c1, c2};
                            unsigned cnt = 0;
#pragma unroll
                            for (int j = 0; j < 8; j++) cnt += nb[j] >> 24 < (unsigned)k ? 1u : 0u;
                            if (cnt) {   // (on this pass's front)
                                unsigned s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
                                for (int j = 0; j < 8; j++) {
                                    const unsigned v = nb[j] >> 24 < (unsigned)k ? nb[j] : 0u;
                                    s0 += v & 255; s1 += v >> 8 & 255; s2 += v >> 16 & 255;
                                }
                                px[ry * BLEED_R + tx] = tile_mean(s0, cnt) | tile_mean(s1, cnt) << 8 | tile_mean(s2, cnt) << 16 | (unsigned)k << 24;
                                live[k] = 1;
                            }
                        }
                        a0 = b0; a1 = b1; a2 = b2; b0 = c0; b1 = c1; b2 = c2;
                    }
                }
                __syncthreads();
                if (!live[k]) break;
            }
            // the tile's pixels: 8 rows of 32 per trip
            const int cx = threadIdx.x & (BLEED_T - 1);
            if (x0 + cx < w) for (int cy = threadIdx.x >> 5; cy < BLEED_T && y0 + cy < h; cy += 8) {
                const unsigned v = px[(P + cy) * BLEED_R + P + cx];
                unsigned char *o = d + (y0 + cy) * dst_stride + (long long)(x0 + cx) * 3;
                o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
            }
        }
    }
}

// n RGBA images (image i at src + i * img_stride bytes) -> the packed 3-channel images dst + i * dst_img_stride after `passes` bleed passes (<= 65534).
// w2xc_bleed_stamps(passes): stamp = n planes of w * h 16-bit words of scratch, stamp_stride words apart; otherwise no stamp is read or written.
hipError_t w2xc_launch_rgba_bleed(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, int passes, unsigned char *dst, size_t dst_img_stride,
                                  size_t dst_stride, unsigned short *stamp, size_t stamp_stride, int n, hipStream_t st)
{
    const long long total = (long long)w * h;
    if (passes <= 1)   // the plain repack; one pass, which reads the source alone: already one launch, and without LDS and barriers the faster one
        return launch_px(RgbaBleedFirst{src, (long long)img_stride, (long long)stride, w, h, passes, dst, (long long)dst_img_stride, (long long)dst_stride, nullptr, 0}, total, n, st);
    if (passes <= W2XC_BLEED_TILED_MAX) {
        const int tiles_x = (w + BLEED_T - 1) / BLEED_T;
        const long long tiles = (long long)tiles_x * ((h + BLEED_T - 1) / BLEED_T);
        const dim3 grid((unsigned)(tiles > (1 << 20) ? (1 << 20) : tiles), (unsigned)(n > 65535 ? 65535 : n));
        hipLaunchKernelGGL(k_bleed_tiled, grid, dim3(256), 0, st, src, (long long)img_stride, (long long)stride, w, h, passes, dst, (long long)dst_img_stride,
                           (long long)dst_stride, tiles_x, tiles, n);
        return hipGetLastError();
    }
    // every pass is launched, whatever an earlier launch reported; the first error is the call's
    hipError_t e = launch_px(RgbaBleedFirst{src, (long long)img_stride, (long long)stride, w, h, 1, dst, (long long)dst_img_stride, (long long)dst_stride, stamp,
                                            (long long)stamp_stride}, total, n, st);
    for (int k = 2; k <= passes; k++) {
        const hipError_t ek = launch_px(RgbaBleedPass{dst, (long long)dst_img_stride, (long long)dst_stride, w, h, (unsigned)k, stamp, (long long)stamp_stride}, total, n, st);
        if (e == hipSuccess) e = ek;
    }
    return e;
}

// alpha byte -> a = u8 / 255 (the Y route: the planes that ride with Y through the scale model); image i's plane at a + i * ps floats
struct AlphaToPlane {
    const unsigned char *src;
    long long img_stride, stride;
    int w;
    float *a;
    long long ps;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        a[img * ps + q] = (float)src[img * img_stride + at.r * stride + (long long)at.c * 4 + 3] * (float)(1.0 / 255.0);
    }
};
hipError_t w2xc_launch_alpha_to_plane(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *a, long long ps, int n, hipStream_t st)
{
    return launch_px(AlphaToPlane{src, (long long)img_stride, (long long)stride, w, a, ps}, (long long)w * h, n, st);
}

// alpha byte -> the packed 3-channel image (A, A, A) (the RGB route: alpha goes through the RGB pipeline as a grey image)
struct AlphaToGrey {
    const unsigned char *src;
    long long img_stride, stride;
    int w;
    unsigned char *dst;
    long long dst_img_stride, dst_stride;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        const unsigned char a = src[img * img_stride + at.r * stride + (long long)at.c * 4 + 3];
        unsigned char *d = dst + img * dst_img_stride + at.r * dst_stride + (long long)at.c * 3;
        d[0] = a; d[1] = a; d[2] = a;
    }
};
hipError_t w2xc_launch_alpha_to_grey(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, unsigned char *dst, size_t dst_img_stride,
                                     size_t dst_stride, int n, hipStream_t st)
{
    return launch_px(AlphaToGrey{src, (long long)img_stride, (long long)stride, w, dst, (long long)dst_img_stride, (long long)dst_stride}, (long long)w * h, n, st);
}

// the merge: a packed 3-channel result + alpha -> the caller's 4-byte pixels.  Alpha is a float plane (saturate(rint(255 a)), the expression of YuvToU8;
// image i's at a + i * ps floats) or a byte of an image with a_px bytes per pixel (the RGBA source: 4; the grey result of the RGB route: 3).
static __device__ __forceinline__ void merge_rgba_px(const unsigned char *rgb, long long rgb_stride, unsigned char a, RowCol at, unsigned char *dst, long long stride)
{
    const unsigned char *s = rgb + at.r * rgb_stride + (long long)at.c * 3;
    unsigned char *d = dst + at.r * stride + (long long)at.c * 4;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = a;
}
struct MergeRgbaF32 {
    const unsigned char *rgb;
    long long rgb_img_stride, rgb_stride;
    const float *a;
    long long ps;
    int w;
    unsigned char *dst;
    long long img_stride, stride;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        merge_rgba_px(rgb + img * rgb_img_stride, rgb_stride, to_u8(a[img * ps + q]), row_col(q, w), dst + img * img_stride, stride);
    }
};
struct MergeRgbaU8 {
    const unsigned char *rgb;
    long long rgb_img_stride, rgb_stride;
    const unsigned char *a;
    long long a_img_stride, a_stride;
    int a_px, w;
    unsigned char *dst;
    long long img_stride, stride;
    __device__ __forceinline__ void operator()(int img, long long q) const
    {
        const RowCol at = row_col(q, w);
        merge_rgba_px(rgb + img * rgb_img_stride, rgb_stride, a[img * a_img_stride + at.r * a_stride + (long long)at.c * a_px], at, dst + img * img_stride, stride);
    }
};
hipError_t w2xc_launch_merge_rgba(const unsigned char *rgb, size_t rgb_img_stride, size_t rgb_stride, const float *a, long long ps, int w, int h,
                                  unsigned char *dst, size_t img_stride, size_t stride, int n, hipStream_t st)
{
    return launch_px(MergeRgbaF32{rgb, (long long)rgb_img_stride, (long long)rgb_stride, a, ps, w, dst, (long long)img_stride, (long long)stride}, (long long)w * h, n, st);
}
hipError_t w2xc_launch_merge_rgba_u8(const unsigned char *rgb, size_t rgb_img_stride, size_t rgb_stride, const unsigned char *a, size_t a_img_stride, size_t a_stride,
                                     int a_px, int w, int h, unsigned char *dst, size_t img_stride, size_t stride, int n, hipStream_t st)
{
    return launch_px(MergeRgbaU8{rgb, (long long)rgb_img_stride, (long long)rgb_stride, a, (long long)a_img_stride, (long long)a_stride, a_px, w, dst,
                                 (long long)img_stride, (long long)stride}, (long long)w * h, n, st);
}
