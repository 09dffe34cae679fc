// w2xc_color.hip -- row N2 of SURVEY.md 8f: the colour front/back end and the U/V resize of the reference
// CLI's scale loop (/root/reference/src/main.cpp:74-76,136,144,171-172), so that the whole scale phase of
// one image runs device-resident.  All kernels are HBM-streaming (a few bytes per pixel) and keep
// OpenCV's float evaluation order with unfused mul/add (the file is built with -ffp-contract=off).
// Every stage is ONE __device__ body per output element (*_px).  The YUV and resize stages have a batch kernel only (one image: n = 1): it takes its
// image / plane from blockIdx.y -- uniform per workgroup -- and moves only the 64-bit base pointers by image x stride.
#include "w2xc_kernels.h"

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// main.cpp:75-76 (+ cv::split): convertTo(CV_32F, 1/255) and COLOR_RGB2YUV on the channels AS GIVEN
// (the reference feeds imread's BGR order, Q3): Y = .299 c0 + .587 c1 + .114 c2, U = (c2-Y)*.492+.5, V = (c0-Y)*.877+.5
static __device__ __forceinline__ void u8_to_yuv_px(const unsigned char *src, long long stride, int w, long long q, float *y, float *u, float *v)
{
    const float s = (float)(1.0 / 255.0);
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    const unsigned char *p = src + r * stride + (long long)c * 3;
    const float c0 = (float)p[0] * s, c1 = (float)p[1] * s, c2 = (float)p[2] * s;
    float Y = c0 * 0.299f;
    Y = Y + c1 * 0.587f;
    Y = Y + c2 * 0.114f;
    y[q] = Y;
    u[q] = (c2 - Y) * 0.492f + 0.5f;
    v[q] = (c0 - Y) * 0.877f + 0.5f;
}

// n images, image i at src + i * img_stride bytes; its planes at y / u / v + i * ps floats
__global__ void __launch_bounds__(256) k_u8_to_yuv_batch(const unsigned char *src, long long img_stride, long long stride, int w, int h, float *y, float *u,
                                                         float *v, long long ps, int n)
{
    const long long total = (long long)w * h;
    for (int img = blockIdx.y; img < n; img += gridDim.y) {
        const unsigned char *s = src + img * img_stride;
        float *yi = y + img * ps, *ui = u + img * ps, *vi = v + img * ps;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) u8_to_yuv_px(s, stride, w, q, yi, ui, vi);
    }
}

// main.cpp:171-172 (+ cv::merge): COLOR_YUV2RGB and convertTo(CV_8U, 255) = saturate(cvRound(v*255))
static __device__ __forceinline__ void yuv_to_u8_px(const float *y, const float *u, const float *v, int w, long long q, unsigned char *dst, long long stride)
{
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    const float Y = y[q], U = u[q] - 0.5f, V = v[q] - 0.5f;
    float ch[3];
    ch[2] = Y + U * 2.032f;
    ch[1] = (Y + U * -0.395f) + V * -0.581f;
    ch[0] = Y + V * 1.140f;
    unsigned char *p = dst + r * stride + (long long)c * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = (unsigned char)clampi(__float2int_rn(ch[k] * 255.0f), 0, 255);   // round half to even
}

// n images: planes of image i at y / u / v + i * ps floats, its pixels at dst + i * img_stride bytes
__global__ void __launch_bounds__(256) k_yuv_to_u8_batch(const float *y, const float *u, const float *v, long long ps, int w, int h, unsigned char *dst,
                                                         long long img_stride, long long stride, int n)
{
    const long long total = (long long)w * h;
    for (int img = blockIdx.y; img < n; img += gridDim.y) {
        const float *yi = y + img * ps, *ui = u + img * ps, *vi = v + img * ps;
        unsigned char *d = dst + img * img_stride;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) yuv_to_u8_px(yi, ui, vi, w, q, d, stride);
    }
}

// The RGB image pipeline (w2xc_process_image_rgb_u8*; no counterpart in v1 of the reference): x = u8 / 255 on the three channels as given, and
// back out = saturate(rint(255 x)) -- the two expressions of u8_to_yuv_px / yuv_to_u8_px without the colour matrix, and the ones the uint8 forms of
// conv3x3_first / conv3x3_last (w2xc_kernels.hip) evaluate in their load / store.  Three planar float planes p0 / p1 / p2.
static __device__ __forceinline__ void u8_to_rgb_px(const unsigned char *src, long long stride, int w, long long q, float *p0, float *p1, float *p2)
{
    const float s = (float)(1.0 / 255.0);
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    const unsigned char *p = src + r * stride + (long long)c * 3;
    p0[q] = (float)p[0] * s;
    p1[q] = (float)p[1] * s;
    p2[q] = (float)p[2] * s;
}

__global__ void __launch_bounds__(256) k_u8_to_rgb(const unsigned char *src, long long stride, int w, int h, float *p0, float *p1, float *p2)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) u8_to_rgb_px(src, stride, w, q, p0, p1, p2);
}

// n images, image i at src + i * img_stride bytes; its three planes at planes + i * is + {0, 1, 2} * ps floats
__global__ void __launch_bounds__(256) k_u8_to_rgb_batch(const unsigned char *src, long long img_stride, long long stride, int w, int h, float *planes,
                                                         long long ps, long long is, int n)
{
    const long long total = (long long)w * h;
    for (int img = blockIdx.y; img < n; img += gridDim.y) {
        const unsigned char *s = src + img * img_stride;
        float *p0 = planes + img * is;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) u8_to_rgb_px(s, stride, w, q, p0, p0 + ps, p0 + 2 * ps);
    }
}

static __device__ __forceinline__ void rgb_to_u8_px(const float *p0, const float *p1, const float *p2, int w, long long q, unsigned char *dst, long long stride)
{
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    unsigned char *p = dst + r * stride + (long long)c * 3;
    p[0] = (unsigned char)clampi(__float2int_rn(p0[q] * 255.0f), 0, 255);   // round half to even
    p[1] = (unsigned char)clampi(__float2int_rn(p1[q] * 255.0f), 0, 255);
    p[2] = (unsigned char)clampi(__float2int_rn(p2[q] * 255.0f), 0, 255);
}

__global__ void __launch_bounds__(256) k_rgb_to_u8(const float *p0, const float *p1, const float *p2, int w, int h, unsigned char *dst, long long stride)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) rgb_to_u8_px(p0, p1, p2, w, q, dst, stride);
}

__global__ void __launch_bounds__(256) k_rgb_to_u8_batch(const float *planes, long long ps, long long is, int w, int h, unsigned char *dst, long long img_stride,
                                                         long long stride, int n)
{
    const long long total = (long long)w * h;
    for (int img = blockIdx.y; img < n; img += gridDim.y) {
        const float *p0 = planes + img * is;
        unsigned char *d = dst + img * img_stride;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) rgb_to_u8_px(p0, p0 + ps, p0 + 2 * ps, w, q, d, stride);
    }
}

static __device__ __forceinline__ void cubic_coeffs(float t, float *c)   // Keys cubic, A = -0.75 (OpenCV interpolateCubic)
{
    const float A = -0.75f;
    c[0] = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A;
    c[1] = ((A + 2) * t - (A + 3)) * t * t + 1;
    c[2] = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// main.cpp:144 on one plane: cv::resize(2x, INTER_CUBIC): horizontal pass to float, then vertical pass,
// taps sx-1..sx+2 clipped to the image.  One thread per output pixel (4 x 4 source taps from L2/L1).
static __device__ __forceinline__ void resize2x_cubic_px(const float *src, int w, int h, long long q, float *dst)
{
    const int W = 2 * w;
    const int dy = (int)(q / W), dx = (int)(q - (long long)dy * W);
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
        const float *S = src + (long long)clampi(sy - 1 + j, 0, h - 1) * w;
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
    dst[q] = a;
}

// n planes (the U and the V planes of a sub-batch, adjacent): plane p at src + p * sps, its 2x plane at dst + p * dps (floats)
__global__ void __launch_bounds__(256) k_resize2x_cubic_batch(const float *src, long long sps, int w, int h, float *dst, long long dps, int n)
{
    const long long total = 4LL * w * h;
    for (int p = blockIdx.y; p < n; p += gridDim.y) {
        const float *s = src + p * sps;
        float *d = dst + p * dps;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) resize2x_cubic_px(s, w, h, q, d);
    }
}

// main.cpp:158-167 on one plane: cv::resize(Size(dw, dh), INTER_LINEAR): half-pixel centres, the two taps
// clipped to the image, horizontal pass to float then vertical pass (no antialiasing, like OpenCV).
static __device__ __forceinline__ void resize_linear_px(const float *src, int sw, int sh, long long q, float *dst, int dw, double scale_x, double scale_y)
{
    const int dy = (int)(q / dw), dx = (int)(q - (long long)dy * dw);
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
    dst[q] = a;
}

// n planes (Y, U and V of a sub-batch): the first ny planes at src_y + p * sps (the Y planes: after a noise pass they do not adjoin U), plane p >= ny at
// src_uv + (p - ny) * sps; destination plane p at dst + p * dps (floats)
__global__ void __launch_bounds__(256) k_resize_linear_batch(const float *src_y, const float *src_uv, int ny, long long sps, int sw, int sh, float *dst,
                                                             long long dps, int dw, int dh, double scale_x, double scale_y, int n)
{
    const long long total = (long long)dw * dh;
    for (int p = blockIdx.y; p < n; p += gridDim.y) {
        const float *s = p < ny ? src_y + p * sps : src_uv + (p - ny) * sps;
        float *d = dst + p * dps;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) resize_linear_px(s, sw, sh, q, d, dw, scale_x, scale_y);
    }
}

// ---- RGBA images (w2xc_process_image_rgba_u8*; no counterpart in v1 of the reference) ----
// Colour bleed: a transparent pixel (alpha == 0) beside opaque ones takes the rounded mean of its opaque 3x3 neighbours, (2 sum + n) / (2 n) per channel,
// and counts as opaque in the next pass; P passes carry the colour P pixels into the transparent region.  The passes are defined as a ping-pong (a pass
// reads only what the pass before left); they run IN PLACE on the packed 3-channel image, exactly, because a pixel filled in pass k (its stamp: 0 = opaque in
// the source, k = filled in pass k, BLEED_FAR = not reached) reads only neighbours whose stamp is below k, and those are written by no thread of pass k; a
// neighbour's stamp that is being set to k reads as BLEED_FAR or as k, neither of them below k.
#define BLEED_FAR 0xFFFFu

// writes pixel q of the packed image, its stamp, and -- with first_pass -- pass 1, read from the RGBA source's own alpha
static __device__ __forceinline__ void rgba_bleed_first_px(const unsigned char *src, long long stride, int w, int h, long long q, int first_pass,
                                                           unsigned char *dst, long long dst_stride, unsigned short *stamp)
{
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    const unsigned char *p = src + r * stride + (long long)c * 4;
    int o0 = p[0], o1 = p[1], o2 = p[2];
    unsigned s = p[3] ? 0u : BLEED_FAR;
    if (s && first_pass) {
        int n = 0, s0 = 0, s1 = 0, s2 = 0;
        for (int dy = -1; dy <= 1; dy++) {
            const int rr = r + dy;
            if (rr < 0 || rr >= h) continue;
            for (int dx = -1; dx <= 1; dx++) {
                const int cc = c + dx;
                if (cc < 0 || cc >= w) continue;
                const unsigned char *nb = src + rr * stride + (long long)cc * 4;
                if (nb[3]) { n++; s0 += nb[0]; s1 += nb[1]; s2 += nb[2]; }
            }
        }
        if (n) { o0 = (2 * s0 + n) / (2 * n); o1 = (2 * s1 + n) / (2 * n); o2 = (2 * s2 + n) / (2 * n); s = 1u; }
    }
    unsigned char *d = dst + r * dst_stride + (long long)c * 3;
    d[0] = (unsigned char)o0; d[1] = (unsigned char)o1; d[2] = (unsigned char)o2;
    stamp[q] = (unsigned short)s;
}

__global__ void __launch_bounds__(256) k_rgba_bleed_first(const unsigned char *src, long long stride, int w, int h, int first_pass, unsigned char *dst,
                                                          long long dst_stride, unsigned short *stamp)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256)
        rgba_bleed_first_px(src, stride, w, h, q, first_pass, dst, dst_stride, stamp);
}

// pass k >= 2, in place (see above)
static __device__ __forceinline__ void rgba_bleed_pass_px(unsigned char *img, long long stride, int w, int h, long long q, unsigned k, unsigned short *stamp)
{
    if (stamp[q] != BLEED_FAR) return;
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    int n = 0, s0 = 0, s1 = 0, s2 = 0;
    for (int dy = -1; dy <= 1; dy++) {
        const int rr = r + dy;
        if (rr < 0 || rr >= h) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int cc = c + dx;
            if (cc < 0 || cc >= w) continue;
            if (stamp[(long long)rr * w + cc] < k) {
                const unsigned char *nb = img + rr * stride + (long long)cc * 3;
                n++; s0 += nb[0]; s1 += nb[1]; s2 += nb[2];
            }
        }
    }
    if (!n) return;
    unsigned char *d = img + r * stride + (long long)c * 3;
    d[0] = (unsigned char)((2 * s0 + n) / (2 * n));
    d[1] = (unsigned char)((2 * s1 + n) / (2 * n));
    d[2] = (unsigned char)((2 * s2 + n) / (2 * n));
    stamp[q] = (unsigned short)k;
}

__global__ void __launch_bounds__(256) k_rgba_bleed_pass(unsigned char *img, long long stride, int w, int h, unsigned k, unsigned short *stamp)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) rgba_bleed_pass_px(img, stride, w, h, q, k, stamp);
}

// alpha byte -> a = u8 / 255 (the Y route: the plane that rides with Y through the scale model)
static __device__ __forceinline__ void alpha_to_plane_px(const unsigned char *src, long long stride, int w, long long q, float *a)
{
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    a[q] = (float)src[r * stride + (long long)c * 4 + 3] * (float)(1.0 / 255.0);
}

__global__ void __launch_bounds__(256) k_alpha_to_plane(const unsigned char *src, long long stride, int w, int h, float *a)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) alpha_to_plane_px(src, stride, w, q, a);
}

// alpha byte -> the packed 3-channel image (A, A, A) (the RGB route: alpha goes through the RGB pipeline as a grey image)
static __device__ __forceinline__ void alpha_to_grey_px(const unsigned char *src, long long stride, int w, long long q, unsigned char *dst, long long dst_stride)
{
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    const unsigned char a = src[r * stride + (long long)c * 4 + 3];
    unsigned char *d = dst + r * dst_stride + (long long)c * 3;
    d[0] = a; d[1] = a; d[2] = a;
}

__global__ void __launch_bounds__(256) k_alpha_to_grey(const unsigned char *src, long long stride, int w, int h, unsigned char *dst, long long dst_stride)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) alpha_to_grey_px(src, stride, w, q, dst, dst_stride);
}

// the merge: a packed 3-channel result + alpha -> the caller's 4-byte pixels.  Alpha is a float plane (saturate(rint(255 a)), the expression of yuv_to_u8_px)
// or a byte of an image with a_px bytes per pixel (the RGBA source: 4; the grey result of the RGB route: 3).
static __device__ __forceinline__ void merge_rgba_px(const unsigned char *rgb, long long rgb_stride, unsigned char a, int w, long long q, unsigned char *dst,
                                                     long long stride)
{
    const int r = (int)(q / w), c = (int)(q - (long long)r * w);
    const unsigned char *s = rgb + r * rgb_stride + (long long)c * 3;
    unsigned char *d = dst + r * stride + (long long)c * 4;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = a;
}

__global__ void __launch_bounds__(256) k_merge_rgba_f32(const unsigned char *rgb, long long rgb_stride, const float *a, int w, int h, unsigned char *dst, long long stride)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256)
        merge_rgba_px(rgb, rgb_stride, (unsigned char)clampi(__float2int_rn(a[q] * 255.0f), 0, 255), w, q, dst, stride);   // round half to even
}

__global__ void __launch_bounds__(256) k_merge_rgba_u8(const unsigned char *rgb, long long rgb_stride, const unsigned char *a, long long a_stride, int a_px,
                                                       int w, int h, unsigned char *dst, long long stride)
{
    const long long total = (long long)w * h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        const int r = (int)(q / w), c = (int)(q - (long long)r * w);
        merge_rgba_px(rgb, rgb_stride, a[r * a_stride + (long long)c * a_px], w, q, dst, stride);
    }
}

static unsigned grid_for(long long total)
{
    long long b = (total + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

// ---- batch forms: grid.y = images / planes (a grid-stride loop inside the kernel covers more than 65535) ----
static dim3 grid_batch(long long total, int n) { return dim3(grid_for(total), (unsigned)(n > 65535 ? 65535 : n)); }

hipError_t w2xc_launch_u8_to_yuv_batch(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *y, float *u, float *v,
                                       long long ps, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_u8_to_yuv_batch, grid_batch((long long)w * h, n), dim3(256), 0, st, src, (long long)img_stride, (long long)stride, w, h, y, u, v, ps, n);
    return hipGetLastError();
}
hipError_t w2xc_launch_yuv_to_u8_batch(const float *y, const float *u, const float *v, long long ps, int w, int h, unsigned char *dst, size_t img_stride,
                                       size_t stride, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_yuv_to_u8_batch, grid_batch((long long)w * h, n), dim3(256), 0, st, y, u, v, ps, w, h, dst, (long long)img_stride, (long long)stride, n);
    return hipGetLastError();
}
hipError_t w2xc_launch_resize2x_cubic_batch(const float *src, long long sps, int w, int h, float *dst, long long dps, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_resize2x_cubic_batch, grid_batch(4LL * w * h, n), dim3(256), 0, st, src, sps, w, h, dst, dps, n);
    return hipGetLastError();
}
hipError_t w2xc_launch_resize_linear_batch(const float *src_y, const float *src_uv, int ny, long long sps, int sw, int sh, float *dst, long long dps, int dw,
                                           int dh, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_resize_linear_batch, grid_batch((long long)dw * dh, n), dim3(256), 0, st, src_y, src_uv, ny, sps, sw, sh, dst, dps, dw, dh,
                       (double)sw / dw, (double)sh / dh, n);
    return hipGetLastError();
}

// one image / one plane: the batch launch with n = 1
hipError_t w2xc_launch_u8_to_yuv(const unsigned char *src, size_t stride, int w, int h, float *y, float *u, float *v, hipStream_t st)
{
    return w2xc_launch_u8_to_yuv_batch(src, 0, stride, w, h, y, u, v, 0, 1, st);
}
hipError_t w2xc_launch_yuv_to_u8(const float *y, const float *u, const float *v, int w, int h, unsigned char *dst, size_t stride, hipStream_t st)
{
    return w2xc_launch_yuv_to_u8_batch(y, u, v, 0, w, h, dst, 0, stride, 1, st);
}
hipError_t w2xc_launch_resize2x_cubic(const float *src, int w, int h, float *dst, hipStream_t st) { return w2xc_launch_resize2x_cubic_batch(src, 0, w, h, dst, 0, 1, st); }
hipError_t w2xc_launch_resize_linear(const float *src, int sw, int sh, float *dst, int dw, int dh, hipStream_t st)
{
    return w2xc_launch_resize_linear_batch(src, src, 1, 0, sw, sh, dst, 0, dw, dh, 1, st);
}

// ---- the RGB pipeline's colour stages ----
hipError_t w2xc_launch_u8_to_rgb(const unsigned char *src, size_t stride, int w, int h, float *p0, float *p1, float *p2, hipStream_t st)
{
    hipLaunchKernelGGL(k_u8_to_rgb, dim3(grid_for((long long)w * h)), dim3(256), 0, st, src, (long long)stride, w, h, p0, p1, p2);
    return hipGetLastError();
}
hipError_t w2xc_launch_rgb_to_u8(const float *p0, const float *p1, const float *p2, int w, int h, unsigned char *dst, size_t stride, hipStream_t st)
{
    hipLaunchKernelGGL(k_rgb_to_u8, dim3(grid_for((long long)w * h)), dim3(256), 0, st, p0, p1, p2, w, h, dst, (long long)stride);
    return hipGetLastError();
}
hipError_t w2xc_launch_u8_to_rgb_batch(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *planes, long long ps, long long is,
                                       int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_u8_to_rgb_batch, grid_batch((long long)w * h, n), dim3(256), 0, st, src, (long long)img_stride, (long long)stride, w, h, planes, ps, is, n);
    return hipGetLastError();
}
hipError_t w2xc_launch_rgb_to_u8_batch(const float *planes, long long ps, long long is, int w, int h, unsigned char *dst, size_t img_stride, size_t stride,
                                       int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_rgb_to_u8_batch, grid_batch((long long)w * h, n), dim3(256), 0, st, planes, ps, is, w, h, dst, (long long)img_stride, (long long)stride, n);
    return hipGetLastError();
}

// ---- RGBA images ----
// d_in -> the packed 3-channel image dst after `passes` bleed passes (<= 65534); stamp = w * h 16-bit words of scratch
hipError_t w2xc_launch_rgba_bleed(const unsigned char *src, size_t stride, int w, int h, int passes, unsigned char *dst, size_t dst_stride, unsigned short *stamp,
                                  hipStream_t st)
{
    const dim3 grid(grid_for((long long)w * h));
    hipLaunchKernelGGL(k_rgba_bleed_first, grid, dim3(256), 0, st, src, (long long)stride, w, h, passes > 0 ? 1 : 0, dst, (long long)dst_stride, stamp);
    for (int k = 2; k <= passes; k++) hipLaunchKernelGGL(k_rgba_bleed_pass, grid, dim3(256), 0, st, dst, (long long)dst_stride, w, h, (unsigned)k, stamp);
    return hipGetLastError();
}
hipError_t w2xc_launch_alpha_to_plane(const unsigned char *src, size_t stride, int w, int h, float *a, hipStream_t st)
{
    hipLaunchKernelGGL(k_alpha_to_plane, dim3(grid_for((long long)w * h)), dim3(256), 0, st, src, (long long)stride, w, h, a);
    return hipGetLastError();
}
hipError_t w2xc_launch_alpha_to_grey(const unsigned char *src, size_t stride, int w, int h, unsigned char *dst, size_t dst_stride, hipStream_t st)
{
    hipLaunchKernelGGL(k_alpha_to_grey, dim3(grid_for((long long)w * h)), dim3(256), 0, st, src, (long long)stride, w, h, dst, (long long)dst_stride);
    return hipGetLastError();
}
hipError_t w2xc_launch_merge_rgba(const unsigned char *rgb, size_t rgb_stride, const float *a, int w, int h, unsigned char *dst, size_t stride, hipStream_t st)
{
    hipLaunchKernelGGL(k_merge_rgba_f32, dim3(grid_for((long long)w * h)), dim3(256), 0, st, rgb, (long long)rgb_stride, a, w, h, dst, (long long)stride);
    return hipGetLastError();
}
hipError_t w2xc_launch_merge_rgba_u8(const unsigned char *rgb, size_t rgb_stride, const unsigned char *a, size_t a_stride, int a_px, int w, int h,
                                     unsigned char *dst, size_t stride, hipStream_t st)
{
    hipLaunchKernelGGL(k_merge_rgba_u8, dim3(grid_for((long long)w * h)), dim3(256), 0, st, rgb, (long long)rgb_stride, a, (long long)a_stride, a_px, w, h, dst,
                       (long long)stride);
    return hipGetLastError();
}
