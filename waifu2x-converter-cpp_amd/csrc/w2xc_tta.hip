// w2xc_tta.hip -- test-time augmentation (include/w2xc_hip.h, "TTA"): the dihedral spread in front of a CNN pass and the gather behind it.
//   T_k, k = 0..7: horizontal flip if k & 1, then vertical flip if k & 2, then transpose if k & 4.  Variants 0..3 of an h x w plane are h x w ("upright"),
//   variants 4..7 are w x h ("transposed").  spread writes T_k(x) for all k from ONE read of x; gather reads the 8 results r_k and writes
//   (((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125f with v_k = T_k^-1(r_k), in that order (the file is built with -ffp-contract=off).
// Layout of the variant planes (contiguous rows, planes ps floats apart): upright (k, i) at up + (k n + i) ps, transposed (k, i) at tr + ((k - 4) n + i) ps.
// Both kernels work on TTA_T x TTA_T tiles of the upright plane, 256 threads as 32 x 8, four rows per thread.  The upright half moves through registers.  The
// transposed half goes through LDS tiles of TTA_T rows of TTA_T + 1 floats: a thread's global accesses then run along the rows of BOTH the upright and the
// transposed planes (a wave covers two 128-byte row segments), and both LDS sides are conflict-free -- ds_write_b32 / ds_read_b32 bank by (address / 4) % 32
// within a 32-lane half: a row access is 32 consecutive words, a column access has stride 33 = 1 mod 32.
// One __device__ body per output element (*_px); the plane comes from blockIdx.y -- uniform per workgroup -- with a grid-stride loop past 65535.
#include "w2xc_kernels.h"

#include "w2xc_tta_px.h"   // TTA_T, TTA_LD, tta_at, tta_gather_px: shared with w2xc_tta_u8.hip

// the four upright variants of source element (y, x)
static __device__ __forceinline__ void tta_spread_up_px(float v, int y, int x, int w, int h, float *up, long long ks)
{
#pragma unroll
    for (int k = 0; k < 4; k++) up[k * ks + tta_at(k, y, x, w, h)] = v;
}

// the four transposed variants of source element (y, x)
static __device__ __forceinline__ void tta_spread_tr_px(float v, int y, int x, int w, int h, float *tr, long long ks)
{
#pragma unroll
    for (int k = 4; k < 8; k++) tr[(k - 4) * ks + tta_at(k, y, x, w, h)] = v;
}

// n source planes (plane i at src + i * sps, rows srs floats apart) -> 8 n variant planes
__global__ void __launch_bounds__(256) k_tta_spread(const float *src, long long sps, long long srs, int w, int h, float *up, float *tr, long long ps, int n)
{
    __shared__ float tile[TTA_T * TTA_LD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int tx = (w + TTA_T - 1) / TTA_T;
    const long long tiles = (long long)tx * ((h + TTA_T - 1) / TTA_T);
    const long long ks = (long long)n * ps;   // from variant k of a plane to its variant k + 1
    for (int p = blockIdx.y; p < n; p += gridDim.y) {
        const float *s = src + p * sps;
        float *u = up + p * ps, *t = tr + p * ps;
        for (long long q = blockIdx.x; q < tiles; q += gridDim.x) {
            const int y0 = (int)(q / tx) * TTA_T, x0 = (int)(q % tx) * TTA_T;
            __syncthreads();   // (the tile of the loop's previous turn has been read)
#pragma unroll
            for (int j = 0; j < TTA_T; j += 8) {
                const int y = y0 + ly + j, x = x0 + lx;
                if (y < h && x < w) {
                    const float v = s[y * srs + x];
                    tile[(ly + j) * TTA_LD + lx] = v;
                    tta_spread_up_px(v, y, x, w, h, u, ks);
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < TTA_T; j += 8) {
                const int y = y0 + lx, x = x0 + ly + j;   // lanes run along y: along the rows of the transposed planes
                if (y < h && x < w) tta_spread_tr_px(tile[lx * TTA_LD + ly + j], y, x, w, h, t, ks);
            }
        }
    }
}

// 8 n result planes of the upright size w x h (transposed ones: h x w) -> n planes (plane i at dst + i * dps, rows drs floats apart)
__global__ void __launch_bounds__(256) k_tta_gather(const float *up, const float *tr, long long ps, int w, int h, float *dst, long long dps, long long drs, int n)
{
    __shared__ float tile[4 * TTA_T * TTA_LD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int tx = (w + TTA_T - 1) / TTA_T;
    const long long tiles = (long long)tx * ((h + TTA_T - 1) / TTA_T);
    const long long ks = (long long)n * ps;
    for (int p = blockIdx.y; p < n; p += gridDim.y) {
        const float *u = up + p * ps, *t = tr + p * ps;
        float *d = dst + p * dps;
        for (long long q = blockIdx.x; q < tiles; q += gridDim.x) {
            const int y0 = (int)(q / tx) * TTA_T, x0 = (int)(q % tx) * TTA_T;
            __syncthreads();
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
                    d[y * drs + x] = tta_gather_px(v);
                }
            }
        }
    }
}

static dim3 tta_grid(int w, int h, int n)
{
    const long long tiles = (long long)((w + TTA_T - 1) / TTA_T) * ((h + TTA_T - 1) / TTA_T);
    return dim3((unsigned)(tiles > 65536 ? 65536 : tiles), (unsigned)(n > 65535 ? 65535 : n));
}

hipError_t w2xc_launch_tta_spread(const float *src, long long sps, long long srs, int w, int h, float *up, float *tr, long long ps, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_tta_spread, tta_grid(w, h, n), dim3(256), 0, st, src, sps, srs, w, h, up, tr, ps, n);
    return hipGetLastError();
}

hipError_t w2xc_launch_tta_gather(const float *up, const float *tr, long long ps, int w, int h, float *dst, long long dps, long long drs, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_tta_gather, tta_grid(w, h, n), dim3(256), 0, st, up, tr, ps, w, h, dst, dps, drs, n);
    return hipGetLastError();
}
