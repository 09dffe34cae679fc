// w2xc_tta_u8.hip -- the TTA spread and gather with the uint8 image at their outer side (include/w2xc_hip.h, "TTA": w2xc_tta_spread_u8_device /
// w2xc_tta_gather_u8_device; the RGBA TTA calls run their RGB and head routes through them).
//   spread  n interleaved uint8 images -> the 8 variants of their 3 n planes: the floats and the layout of U8ToRgb (w2xc_color.hip) followed by k_tta_spread
//           on 3 n planes -- plane 3 i + c = (float)byte[ch0 + c * ch_step] * (float)(1.0 / 255.0) -- without the float copy of the source.  (ch0, ch_step) =
//           (0, 1): the colour of RGB / RGBA pixels; (3, 0) on 4-byte pixels: the grey image (A, A, A) without building it: one conversion, three stores.
//   gather  8 m result planes (m = ppi n) -> bytes byte0 .. byte0 + n_ch - 1 of the px-byte pixels of n images: to_u8 of k_tta_gather's sum for the planes
//           ppi i + first .. + n_ch - 1 of image i.  Nothing else is written -- BYTE stores, never a read-modify-write of a pixel: the colour gather and the
//           alpha gather of one image are two launches that may run in either order.
// The structure is w2xc_tta.hip's: TTA_T x TTA_T tiles of the upright plane, 256 threads as 32 x 8, four rows per thread, the upright half through registers,
// the transposed half through LDS tiles of TTA_LD-word rows (conflict-free on both sides); per element the shared bodies of w2xc_tta_px.h.  blockIdx.y --
// uniform per workgroup -- counts (image, channel) pairs, so that one image of a few tiles still fills the device (the grey spread: images, its three planes
// are one conversion), with a grid-stride loop past 65535; the tile comes from blockIdx.x with one past 65536.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"

// the selected byte of channel c of one pixel (ch_step = 0: of every channel).  DW: the pixel is an aligned 4-byte word, fetched as one
template <bool DW> static __device__ __forceinline__ unsigned ttau8_load_px(const unsigned char *p, int at)
{
    if (DW) return (*reinterpret_cast<const unsigned *>(p) >> (8 * at)) & 255u;
    return (unsigned)p[at];
}

// n images (image i at src + i * sis bytes, rows srs bytes apart, pixels px bytes) -> the 8 variants of their 3 n planes.  DW: every pixel of every image is
// an aligned 4-byte word (the launcher looks at the pointer and the strides).  A workgroup's turn is one channel of one image -- with ch_step = 0 one image:
// the one fetch, the one conversion and the one LDS tile serve its three planes.
template <bool DW>
__global__ void __launch_bounds__(256) k_ttau8_spread(const unsigned char *src, long long sis, long long srs, int px, int ch0, int ch_step, int w, int h,
                                                      float *up, float *tr, long long ps, int n)
{
    __shared__ float tile[TTA_T * TTA_LD];
    const float s255 = (float)(1.0 / 255.0);
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int tx = (w + TTA_T - 1) / TTA_T;
    const long long tiles = (long long)tx * ((h + TTA_T - 1) / TTA_T);
    const long long ks = 3ll * n * ps;   // from variant k of a plane to its variant k + 1
    const int per = ch_step ? 3 : 1, planes = 3 / per;   // turns per image, planes per turn
    for (long long pi = blockIdx.y; pi < (long long)n * per; pi += gridDim.y) {
        const long long i = pi / per;
        const int c0 = (int)(pi % per);
        const unsigned char *s = src + i * sis;
        for (long long q = blockIdx.x; q < tiles; q += gridDim.x) {
            const int y0 = (int)(q / tx) * TTA_T, x0 = (int)(q % tx) * TTA_T;
            float v[TTA_T / 8];
            __syncthreads();   // (the tile of the loop's previous turn has been read)
#pragma unroll
            for (int j = 0; j < TTA_T; j += 8) {
                const int y = y0 + ly + j, x = x0 + lx;
                v[j / 8] = y < h && x < w ? (float)ttau8_load_px<DW>(s + y * srs + (long long)x * px, ch0 + c0 * ch_step) * s255 : 0.0f;
                tile[(ly + j) * TTA_LD + lx] = v[j / 8];
            }
            __syncthreads();
#pragma unroll 1
            for (int c = c0; c < c0 + planes; c++) {
                float *u = up + (3 * i + c) * ps, *t = tr + (3 * i + c) * ps;
#pragma unroll
                for (int j = 0; j < TTA_T; j += 8) {
                    const int y = y0 + ly + j, x = x0 + lx;
                    if (y < h && x < w) {
#pragma unroll
                        for (int k = 0; k < 4; k++) u[k * ks + tta_at(k, y, x, w, h)] = v[j / 8];
                    }
                }
#pragma unroll
                for (int j = 0; j < TTA_T; j += 8) {
                    const int y = y0 + lx, x = x0 + ly + j;   // lanes run along y: along the rows of the transposed planes
                    if (y < h && x < w) {
                        const float vt = tile[lx * TTA_LD + ly + j];
#pragma unroll
                        for (int k = 4; k < 8; k++) t[(k - 4) * ks + tta_at(k, y, x, w, h)] = vt;
                    }
                }
            }
        }
    }
}

// 8 m result planes of the upright size w x h (m = ppi n; transposed ones: h x w) -> bytes byte0 .. byte0 + nch - 1 of the pixels of n images (image i at
// dst + i * dis bytes, rows drs bytes apart, pixels px bytes): channel c from plane ppi i + first + c
__global__ void __launch_bounds__(256) k_ttau8_gather(const float *up, const float *tr, long long ps, int w, int h, unsigned char *dst, long long dis,
                                                      long long drs, int px, int byte0, int nch, int ppi, int first, int n)
{
    __shared__ float tile[4 * TTA_T * TTA_LD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int tx = (w + TTA_T - 1) / TTA_T;
    const long long tiles = (long long)tx * ((h + TTA_T - 1) / TTA_T);
    const long long ks = (long long)ppi * n * ps;   // from variant k of a plane to its variant k + 1
    for (long long pi = blockIdx.y; pi < (long long)n * nch; pi += gridDim.y) {   // a turn: one channel of one image
        const long long i = pi / nch;
        const int c = (int)(pi % nch);
        unsigned char *d = dst + i * dis + byte0 + c;
        const long long p = (ppi * i + first + c) * ps;
        const float *u = up + p, *t = tr + p;
        for (long long q = blockIdx.x; q < tiles; q += gridDim.x) {
            const int y0 = (int)(q / tx) * TTA_T, x0 = (int)(q % tx) * TTA_T;
            __syncthreads();   // (the tiles of the loop's previous turn have been read)
#pragma unroll
            for (int j = 0; j < TTA_T; j += 8) {
                const int y = y0 + lx, x = x0 + ly + j;   // along the rows of the transposed planes
                if (y < h && x < w) {
#pragma unroll
                    for (int k = 4; k < 8; k++) tile[(k - 4) * TTA_T * TTA_LD + lx * TTA_LD + ly + j] = t[(k - 4) * ks + tta_at(k, y, x, w, h)];
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < TTA_T; j += 8) {
                const int y = y0 + ly + j, x = x0 + lx;
                if (y < h && x < w) {
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 4; k++) v[k] = u[k * ks + tta_at(k, y, x, w, h)];
#pragma unroll
                    for (int k = 4; k < 8; k++) v[k] = tile[(k - 4) * TTA_T * TTA_LD + (ly + j) * TTA_LD + lx];
                    d[y * drs + (long long)x * px] = to_u8(tta_gather_px(v));   // one byte store: the pixel's other bytes are not this launch's
                }
            }
        }
    }
}

static dim3 ttau8_grid(int w, int h, long long turns)
{
    const long long tiles = (long long)((w + TTA_T - 1) / TTA_T) * ((h + TTA_T - 1) / TTA_T);
    return dim3((unsigned)(tiles > 65536 ? 65536 : tiles), (unsigned)(turns > 65535 ? 65535 : turns));
}

hipError_t w2xc_launch_tta_spread_u8(const unsigned char *src, size_t img_stride, size_t stride, int px, int ch0, int ch_step, int w, int h, float *up,
                                     float *tr, long long ps, int n, hipStream_t st)
{
    if ((px != 3 && px != 4) || ch0 < 0 || ch_step < 0 || ch0 + 2 * ch_step >= px || w < 1 || h < 1 || n < 1) return hipErrorInvalidValue;
    const bool dw = px == 4 && ((reinterpret_cast<size_t>(src) | stride | (n > 1 ? img_stride : 0)) & 3) == 0;
    hipLaunchKernelGGL(dw ? k_ttau8_spread<true> : k_ttau8_spread<false>, ttau8_grid(w, h, (long long)n * (ch_step ? 3 : 1)), dim3(256), 0, st, src,
                       (long long)img_stride, (long long)stride, px, ch0, ch_step, w, h, up, tr, ps, n);
    return hipGetLastError();
}

hipError_t w2xc_launch_tta_gather_u8(const float *up, const float *tr, long long ps, int w, int h, unsigned char *dst, size_t img_stride, size_t stride, int px,
                                     int byte0, int n_ch, int planes_per_image, int first_plane, int n, hipStream_t st)
{
    if ((px != 3 && px != 4) || byte0 < 0 || n_ch < 1 || byte0 + n_ch > px || first_plane < 0 || first_plane + n_ch > planes_per_image || w < 1 || h < 1 || n < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ttau8_gather, ttau8_grid(w, h, (long long)n * n_ch), dim3(256), 0, st, up, tr, ps, w, h, dst, (long long)img_stride, (long long)stride, px,
                       byte0, n_ch, planes_per_image, first_plane, n);
    return hipGetLastError();
}
