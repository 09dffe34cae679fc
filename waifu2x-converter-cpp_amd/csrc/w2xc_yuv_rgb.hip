// w2xc_yuv_rgb.hip -- the two ends of YUV frames through RGB models (include/w2xc_hip.h, "YUV frames through RGB models": w2xc_process_frames_yuv_u8_rgb[_device],
// w2xc_yuv8_to_rgb_device, w2xc_rgb_to_yuv8_device): Y, U and V bytes of n frames -> three float planes R, G, B per frame by a colour matrix the caller names, and
// three float planes -> the bytes of a frame.  Built with -ffp-contract=off like w2xc_yuv.hip: every product and sum below is its own fp32 operation, in the
// order the header writes it.
//   k_yuv8_to_rgb<DW, SX, SY>   chroma enlarged to luma resolution (0.75 / 0.25, centred siting) from an LDS tile, the matrix, the clamp to [0, 1]
//   k_rgb_to_yuv8<SX, SY>       the matrix the other way, the box mean of chroma over a luma block, the roundings to bytes
// SX / SY: chroma is subsampled along x / y (4:2:0 both, 4:2:2 SX alone, 4:4:4 neither).
// Both kernels share one tiling: a tile is YR_TCX x YR_TCY CHROMA samples of one frame -- so (SX ? 2 : 1) YR_TCX x (SY ? 2 : 1) YR_TCY luma samples --, a workgroup of
// 256 threads = 32 x 8 takes two chroma samples per thread, YR_TCY / 2 rows apart, and with each its block of luma samples (2 x 2, 2 x 1 or 1 x 1).  Tiles of
// all frames are the turns of one grid-stride loop over at most W2XC_YUVRGB_GRID_MAX workgroups; the frame index moves only the 64-bit bases.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi, to_u8
#include "w2xc_yuv_px.h"   // luma_u8, the constants of a matrix
#include "w2xc_yuv_tile.h" // the tile (YR_*), rows_align, yuv_tile_at, chroma_at_luma, rgb_px, chroma_mean

#define YR_YLD (2 * YR_TCX + 4)     // bytes per LDS row of luma: the widest tile and one dword of padding
static_assert((YR_YLD & 3) == 0, "a luma row in LDS is whole dwords");

// ---- bytes -> R, G, B ----
// The chroma tile with a one-sample halo along each subsampled axis (coordinates clamped into the plane, as the taps are) is fetched once for U and once for V
// and kept in LDS as the bytes' values in floats; the luma tile is kept as bytes.  DW: luma rows start on 4-byte boundaries, and so do the rows of planar
// chroma: an aligned group of four samples inside the row is one dword load by one thread; the rim, and interleaved chroma (spx = 2), go byte by byte.
// Stores: a thread's two pixels of a row are adjacent; v2 (every row of every plane starts on an 8-byte boundary: w, ps, is even) makes them ONE 8-byte store per
// plane, a wave's stores a contiguous run of the row; otherwise two float stores.
template <bool DW, bool SX, bool SY>
__global__ void __launch_bounds__(256) k_yuv8_to_rgb(const unsigned char *__restrict__ sy, long long yframe, long long yrow, const unsigned char *__restrict__ su,
                                                     const unsigned char *__restrict__ sv, long long cframe, long long crow, int spx, int w, int h, int cw, int ch,
                                                     int limited, W2xcYuvToRgb m, float *__restrict__ rgb, long long is, long long ps, int v2, int tiles_x,
                                                     long long tiles, long long turns)
{
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;          // the halo
    constexpr int SW = YR_TCX + 2 * HX, SH = YR_TCY + 2 * HY;   // the chroma tile in LDS
    constexpr int LW = YR_TCX << HX, LH = YR_TCY << HY;       // the luma tile
    __shared__ float ctile[2][(YR_TCY + 2) * YR_LD];
    __shared__ __attribute__((aligned(4))) unsigned char ytile[2 * YR_TCY * YR_YLD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float ky = limited ? (float)(1.0 / 219.0) : (float)(1.0 / 255.0), kc = limited ? (float)(1.0 / 224.0) : (float)(1.0 / 255.0);
    const float y0 = limited ? 16.0f : 0.0f;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of one frame
        int cx0, cy0;
        const long long f = yuv_tile_at(turn, tiles, tiles_x, YR_TCX, YR_TCY, &cx0, &cy0);
        const int X0 = cx0 << HX, Y0 = cy0 << HY;   // the tile's first luma sample
        const unsigned char *fy = sy + f * yframe;
        __syncthreads();   // (the tiles of the loop's previous turn have been read)
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const unsigned char *s = (v ? sv : su) + f * cframe;
            float *tile = ctile[v];
            if (DW && spx == 1) {
                // column groups of four samples from cx0 - 4 HX (a multiple of 4) on
                constexpr int NG = YR_TCX / 4 + 2 * HX;
                for (int i = threadIdx.x; i < SH * NG; i += 256) {
                    const int r = i / NG, g = i - r * NG;
                    const int gx4 = cx0 - 4 * HX + 4 * g;
                    const unsigned char *row = s + clampi(cy0 - HY + r, 0, ch - 1) * crow;
                    unsigned b[4];
                    if (gx4 >= 0 && gx4 + 3 < cw) {
                        const unsigned w4 = *reinterpret_cast<const unsigned *>(row + gx4);
                        b[0] = w4 & 255u; b[1] = (w4 >> 8) & 255u; b[2] = (w4 >> 16) & 255u; b[3] = w4 >> 24;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) b[k] = row[clampi(gx4 + k, 0, cw - 1)];
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int c = 4 * g - 3 * HX + k;
                        if (c >= 0 && c < SW) tile[r * YR_LD + c] = (float)b[k];
                    }
                }
            } else {
                for (int i = threadIdx.x; i < SH * SW; i += 256) {
                    const int r = i / SW, c = i - r * SW;
                    tile[r * YR_LD + c] = (float)s[clampi(cy0 - HY + r, 0, ch - 1) * crow + (long long)clampi(cx0 - HX + c, 0, cw - 1) * spx];
                }
            }
        }
        // luma: rows Y0 .. Y0 + LH - 1, columns X0 .. X0 + LW - 1 where they lie in the plane (nothing else of the tile is read below)
        if (DW) {
            constexpr int NG = LW / 4;
            for (int i = threadIdx.x; i < LH * NG; i += 256) {
                const int r = i / NG, g = i - r * NG;
                const int x4 = X0 + 4 * g;
                if (Y0 + r >= h || x4 >= w) continue;
                const unsigned char *row = fy + (Y0 + r) * yrow;
                unsigned w4;
                if (x4 + 3 < w) w4 = *reinterpret_cast<const unsigned *>(row + x4);
                else {
                    w4 = row[x4];
                    if (x4 + 1 < w) w4 |= (unsigned)row[x4 + 1] << 8;
                    if (x4 + 2 < w) w4 |= (unsigned)row[x4 + 2] << 16;
                }
                *reinterpret_cast<unsigned *>(ytile + r * YR_YLD + 4 * g) = w4;
            }
        } else {
            for (int i = threadIdx.x; i < LH * LW; i += 256) {
                const int r = i / LW, c = i - r * LW;
                if (Y0 + r < h && X0 + c < w) ytile[r * YR_YLD + c] = fy[(Y0 + r) * yrow + X0 + c];
            }
        }
        __syncthreads();
        float *o = rgb + f * is;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int tr = ly + j * (YR_TCY / 2), cx = cx0 + lx, cy = cy0 + tr;
            if (cx >= cw || cy >= ch) continue;
            float cu[2][1 + HY][1 + HX];   // U and V at the block's luma samples, from the thread's own sample
#pragma unroll
            for (int v = 0; v < 2; v++) chroma_at_luma<SX, SY>(ctile[v] + (tr + HY) * YR_LD + lx + HX, YR_LD, cu[v]);
#pragma unroll
            for (int r = 0; r < 1 + HY; r++) {
                const int Y = (cy << HY) + r;
                if (Y >= h) continue;
                float px[3][1 + HX];   // R, G, B of the row's pixels
#pragma unroll
                for (int q = 0; q < 1 + HX; q++) {
                    const float y = ((float)ytile[((tr << HY) + r) * YR_YLD + (lx << HX) + q] - y0) * ky;
                    rgb_px(m, y, (cu[0][r][q] - 128.0f) * kc, (cu[1][r][q] - 128.0f) * kc, px, q);
                }
                const int X = cx << HX;
                float *d = o + (long long)Y * w + X;
                if (SX && v2) {   // (w is even: the second pixel lies in the row)
#pragma unroll
                    for (int p = 0; p < 3; p++) *reinterpret_cast<float2 *>(d + p * ps) = make_float2(px[p][0], px[p][HX]);
                } else {
#pragma unroll
                    for (int p = 0; p < 3; p++) {
                        d[p * ps] = px[p][0];
                        if (SX && X + 1 < w) d[p * ps + 1] = px[p][HX];
                    }
                }
            }
        }
    }
}

hipError_t w2xc_launch_yuv8_to_rgb(W2xcU8Planes y, W2xcU8Planes u, const unsigned char *v, int w, int h, int chroma, int range, int matrix, float *rgb, long long is,
                                   long long ps, int n, hipStream_t st)
{
    W2xcYuvToRgb m;
    int cw, ch;
    if (!matrix_to_rgb(matrix, &m) || !frame_geometry(w, h, chroma, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 || (u.px != 1 && u.px != 2))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    size_t align = rows_align(y, n);
    if (u.px == 1) align |= rows_align(u, n) | reinterpret_cast<size_t>(v);
    const bool dw = (align & 3) == 0;
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n);
#define W2XC_TO_RGB(SX, SY) (dw ? k_yuv8_to_rgb<true, SX, SY> : k_yuv8_to_rgb<false, SX, SY>)
    const auto kernel = chroma == 0 ? W2XC_TO_RGB(true, true) : chroma == 1 ? W2XC_TO_RGB(true, false) : W2XC_TO_RGB(false, false);
#undef W2XC_TO_RGB
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, y.p, y.frame, y.row, u.p, v, u.frame, u.row, u.px, w, h, cw, ch, limited, m, rgb, is, ps, v2,
                       g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}

// ---- R, G, B -> bytes ----
// A thread reads its block of the three planes (a block cut by an odd edge replicates its last column / row), computes the block's luma bytes and its one U
// and one V byte, and stores only to its own samples: byte stores, or -- Y16: every luma row starts on an even address -- one 16-bit store for the two luma
// bytes of a row where both lie in the plane.  Never a read-modify-write: with dpx = 2 the bytes between a plane's samples are the other plane's.
// Loads: v2 (every row of every float plane starts on an 8-byte boundary) fetches a thread's two adjacent pixels of a row as ONE 8-byte load per plane.
static __device__ __forceinline__ unsigned char chroma_u8(float c, float scale) { return (unsigned char)clampi(__float2int_rn(c * scale + 128.0f), 0, 255); }

template <bool SX, bool SY>
__global__ void __launch_bounds__(256) k_rgb_to_yuv8(const float *__restrict__ rgb, long long is, long long ps, int v2, int w, int h, int cw, int ch, int limited,
                                                     W2xcRgbToYuv m, unsigned char *__restrict__ dy, long long yframe, long long yrow, int y16,
                                                     unsigned char *__restrict__ du, unsigned char *__restrict__ dv, long long cframe, long long crow, int dpx,
                                                     int tiles_x, long long tiles, long long turns)
{
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float cs = limited ? 224.0f : 255.0f;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {
        int cx0, cy0;
        const long long f = yuv_tile_at(turn, tiles, tiles_x, YR_TCX, YR_TCY, &cx0, &cy0);
        const float *s = rgb + f * is;
        unsigned char *oy = dy + f * yframe;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int cx = cx0 + lx, cy = cy0 + ly + j * (YR_TCY / 2);
            if (cx >= cw || cy >= ch) continue;
            YCC p[1 + HY][1 + HX];
#pragma unroll
            for (int r = 0; r < 1 + HY; r++) {
                const int Y = min((cy << HY) + r, h - 1);
                if (SX && v2) {   // (w is even: no block is cut at the right edge)
                    const float *e = s + (long long)Y * w + (cx << HX);
                    const float2 R = *reinterpret_cast<const float2 *>(e), G = *reinterpret_cast<const float2 *>(e + ps), B = *reinterpret_cast<const float2 *>(e + 2 * ps);
                    p[r][0] = to_ycc(m, R.x, G.x, B.x);
                    p[r][HX] = to_ycc(m, R.y, G.y, B.y);
                    continue;
                }
#pragma unroll
                for (int q = 0; q < 1 + HX; q++) {
                    const int X = min((cx << HX) + q, w - 1);
                    const float *e = s + (long long)Y * w + X;
                    p[r][q] = to_ycc(m, e[0], e[ps], e[2 * ps]);
                }
            }
#pragma unroll
            for (int r = 0; r < 1 + HY; r++) {
                const int Y = (cy << HY) + r, X = cx << HX;
                if (Y >= h) continue;
                unsigned char *d = oy + Y * yrow + X;
                const unsigned b0 = luma_u8(p[r][0].y, limited);
                if (SX && X + 1 < w) {
                    const unsigned b1 = luma_u8(p[r][HX].y, limited);
                    if (y16) *reinterpret_cast<unsigned short *>(d) = (unsigned short)(b0 | (b1 << 8));
                    else { d[0] = (unsigned char)b0; d[1] = (unsigned char)b1; }
                } else d[0] = (unsigned char)b0;
            }
            float cb, cr;
            chroma_mean<SX, SY>(p, &cb, &cr);
            const long long at = f * cframe + cy * crow + (long long)cx * dpx;
            du[at] = chroma_u8(cb, cs);
            dv[at] = chroma_u8(cr, cs);
        }
    }
}

hipError_t w2xc_launch_rgb_to_yuv8(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, W2xcU8Planes y, W2xcU8Planes u,
                                   unsigned char *v, int n, hipStream_t st)
{
    W2xcRgbToYuv m;
    int cw, ch;
    if (!matrix_from_rgb(matrix, &m) || !frame_geometry(w, h, chroma, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 || (u.px != 1 && u.px != 2))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int y16 = (rows_align(y, n) & 1) == 0;
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n);
    const auto kernel = chroma == 0 ? k_rgb_to_yuv8<true, true> : chroma == 1 ? k_rgb_to_yuv8<true, false> : k_rgb_to_yuv8<false, false>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, rgb, is, ps, v2, w, h, cw, ch, limited, m, y.p, y.frame, y.row, y16, u.p, v, u.frame, u.row, u.px,
                       g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
