// w2xc_yuv16_rgb.hip -- the two ends of 16-bit YUV frames through RGB models (include/w2xc_hip.h, "16-bit YUV frames": w2xc_process_frames_yuv_u16_rgb[_device],
// w2xc_yuv16_to_rgb_device, w2xc_rgb_to_yuv16_device): Y, U and V words of n frames -- a value of `depth` bits in the low or the high bits of each -- -> three float
// planes R, G, B per frame by a colour matrix the caller names, and three float planes -> the words of a frame.  Built with -ffp-contract=off like
// w2xc_yuv_rgb.hip: every product and sum below is its own fp32 operation, in the order the header writes it.
//   k_yuv16_to_rgb<CM, SX, SY>   chroma enlarged to luma resolution (0.75 / 0.25, centred siting) from an LDS tile, the matrix, the clamp to [0, 1]
//   k_rgb_to_yuv16<SX, SY>       the matrix the other way, the box mean of chroma over a luma block, the roundings to words
// SX / SY: chroma is subsampled along x / y (4:2:0 both, 4:2:2 SX alone, 4:4:4 neither).  The tiling is that of w2xc_yuv_rgb.hip: a tile is YR_TCX x YR_TCY CHROMA
// samples of one frame, a workgroup of 256 threads = 32 x 8 takes two chroma samples per thread, YR_TCY / 2 rows apart, and with each its block of luma samples;
// tiles of all frames are the turns of one grid-stride loop over at most W2XC_YUVRGB_GRID_MAX workgroups; the frame index moves only the 64-bit bases.
#include "w2xc_kernels.h"
#include "w2xc_tta_px.h"   // clampi
#include "w2xc_yuv_px.h"   // u16_value, to_u16, luma_u16, the constants of a matrix and of a depth
#include "w2xc_yuv_tile.h" // the tile (YR_*), rows_align, yuv_tile_at, chroma_at_luma, rgb_px, chroma_mean

#define YR_YLD (2 * YR_TCX + 2)     // 16-bit words per LDS row of luma: the widest tile and one dword of padding -- 33 dwords, an odd count
static_assert((YR_YLD & 1) == 0 && ((YR_YLD / 2) & 1) == 1, "a luma row in LDS is whole dwords, an odd count of them");

// ---- words -> R, G, B ----
// The chroma tiles with a one-sample halo along each subsampled axis (coordinates clamped into the plane, as the taps are) are kept in LDS as the samples' values
// in floats; the luma tile is kept as the samples' words.
//   CM 1: planar chroma whose rows start on 8-byte boundaries: an aligned group of four samples inside the row is ONE 8-byte load by one thread, the rim sample
//         by sample;
//   CM 2: interleaved chroma, sv = su + 1 (P010), rows on 4-byte boundaries: ONE pass of 4-byte loads, a sample's (U, V) pair each, fills BOTH tiles;
//   CM 0: sample by sample.
//   yv:   luma rows start on 8-byte boundaries: an aligned group of four samples inside the row is one 8-byte load.
// Stores: a thread's two pixels of a row are adjacent; v2 (every row of every plane starts on an 8-byte boundary: w, ps, is even) makes them ONE 8-byte store per
// plane; otherwise two float stores.
template <int CM, bool SX, bool SY>
__global__ void __launch_bounds__(256) k_yuv16_to_rgb(const unsigned short *__restrict__ sy, long long yframe, long long yrow, int yv, int yshift,
                                                      const unsigned short *__restrict__ su, const unsigned short *__restrict__ sv, long long cframe, long long crow,
                                                      int spx, int cshift, int max, int w, int h, int cw, int ch, float y0, float ky, float c0, float kc,
                                                      W2xcYuvToRgb m, float *__restrict__ rgb, long long is, long long ps, int v2, int tiles_x, long long tiles,
                                                      long long turns)
{
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;          // the halo
    constexpr int SW = YR_TCX + 2 * HX, SH = YR_TCY + 2 * HY;   // the chroma tile in LDS
    constexpr int LW = YR_TCX << HX, LH = YR_TCY << HY;       // the luma tile
    __shared__ float ctile[2][(YR_TCY + 2) * YR_LD];
    __shared__ __attribute__((aligned(4))) unsigned short ytile[2 * YR_TCY * YR_YLD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of one frame
        int cx0, cy0;
        const long long f = yuv_tile_at(turn, tiles, tiles_x, YR_TCX, YR_TCY, &cx0, &cy0);
        const int X0 = cx0 << HX, Y0 = cy0 << HY;   // the tile's first luma sample
        const unsigned short *fy = sy + f * yframe;
        // yv: the thread's groups of four luma samples go into registers first, so that their loads are in flight with those of the chroma tiles
        constexpr int NGY = LW / 4, NJ = (LH * NGY + 255) / 256;
        uint2 yw[NJ];
        if (yv) {
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int i = threadIdx.x + 256 * j, r = i / NGY, g = i - r * NGY;
                const int x4 = X0 + 4 * g;
                yw[j] = make_uint2(0u, 0u);
                if (i >= LH * NGY || Y0 + r >= h || x4 >= w) continue;
                const unsigned short *row = fy + (Y0 + r) * yrow;
                if (x4 + 3 < w) yw[j] = *reinterpret_cast<const uint2 *>(row + x4);
                else {
                    yw[j].x = row[x4];
                    if (x4 + 1 < w) yw[j].x |= (unsigned)row[x4 + 1] << 16;
                    if (x4 + 2 < w) yw[j].y = row[x4 + 2];
                }
            }
        }
        __syncthreads();   // (the tiles of the loop's previous turn have been read)
        if (CM == 2) {
            const unsigned short *s = su + f * cframe;
            for (int i = threadIdx.x; i < SH * SW; i += 256) {
                const int r = i / SW, c = i - r * SW;
                const unsigned w2 = *reinterpret_cast<const unsigned *>(s + clampi(cy0 - HY + r, 0, ch - 1) * crow + (long long)clampi(cx0 - HX + c, 0, cw - 1) * 2);
                ctile[0][r * YR_LD + c] = (float)u16_value(w2 & 0xFFFFu, cshift, max);
                ctile[1][r * YR_LD + c] = (float)u16_value(w2 >> 16, cshift, max);
            }
        } else if (CM == 1) {
            // column groups of four samples from cx0 - 4 HX (a multiple of 4) on; a thread fetches a group of U and the same group of V: two loads in flight
            constexpr int NG = YR_TCX / 4 + 2 * HX;
            const unsigned short *s0 = su + f * cframe, *s1 = sv + f * cframe;
            for (int i = threadIdx.x; i < SH * NG; i += 256) {
                const int r = i / NG, g = i - r * NG;
                const int gx4 = cx0 - 4 * HX + 4 * g;
                const long long at = clampi(cy0 - HY + r, 0, ch - 1) * crow;
                unsigned b[2][4];
                if (gx4 >= 0 && gx4 + 3 < cw) {
                    const uint2 u4 = *reinterpret_cast<const uint2 *>(s0 + at + gx4), v4 = *reinterpret_cast<const uint2 *>(s1 + at + gx4);
                    b[0][0] = u4.x & 0xFFFFu; b[0][1] = u4.x >> 16; b[0][2] = u4.y & 0xFFFFu; b[0][3] = u4.y >> 16;
                    b[1][0] = v4.x & 0xFFFFu; b[1][1] = v4.x >> 16; b[1][2] = v4.y & 0xFFFFu; b[1][3] = v4.y >> 16;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const long long e = at + clampi(gx4 + k, 0, cw - 1);
                        b[0][k] = s0[e];
                        b[1][k] = s1[e];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int c = 4 * g - 3 * HX + k;
                    if (c >= 0 && c < SW) {
                        ctile[0][r * YR_LD + c] = (float)u16_value(b[0][k], cshift, max);
                        ctile[1][r * YR_LD + c] = (float)u16_value(b[1][k], cshift, max);
                    }
                }
            }
        } else {
            for (int i = threadIdx.x; i < SH * SW; i += 256) {
                const int r = i / SW, c = i - r * SW;
                const long long at = clampi(cy0 - HY + r, 0, ch - 1) * crow + (long long)clampi(cx0 - HX + c, 0, cw - 1) * spx;
                ctile[0][r * YR_LD + c] = (float)u16_value((su + f * cframe)[at], cshift, max);
                ctile[1][r * YR_LD + c] = (float)u16_value((sv + f * cframe)[at], cshift, max);
            }
        }
        // luma: rows Y0 .. Y0 + LH - 1, columns X0 .. X0 + LW - 1 where they lie in the plane (nothing else of the tile is read below)
        if (yv) {   // (the groups were fetched ahead of the chroma tiles; a group outside the plane is zeros that nothing reads)
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int i = threadIdx.x + 256 * j, r = i / NGY, g = i - r * NGY;
                if (i >= LH * NGY) continue;
                unsigned *d = reinterpret_cast<unsigned *>(ytile + r * YR_YLD + 4 * g);
                d[0] = yw[j].x;
                d[1] = yw[j].y;
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
                    const float y = ((float)u16_value(ytile[((tr << HY) + r) * YR_YLD + (lx << HX) + q], yshift, max) - y0) * ky;
                    rgb_px(m, y, (cu[0][r][q] - c0) * kc, (cu[1][r][q] - c0) * kc, px, q);
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

hipError_t w2xc_launch_yuv16_to_rgb(W2xcU16Planes y, W2xcU16Planes u, const unsigned short *v, int w, int h, int chroma, int range, int matrix, int depth, float *rgb,
                                    long long is, long long ps, int n, hipStream_t st)
{
    W2xcYuvToRgb m;
    int cw, ch;
    if (!matrix_to_rgb(matrix, &m) || !frame_geometry(w, h, chroma, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 || (u.px != 1 && u.px != 2) ||
        depth < 8 || depth > 16)
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int yv = (rows_align(y, n) & 7) == 0;
    int cm = 0;
    if (u.px == 1 && ((rows_align(u, n) | reinterpret_cast<size_t>(v)) & 7) == 0) cm = 1;
    else if (u.px == 2 && v == u.p + 1 && (rows_align(u, n) & 3) == 0) cm = 2;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    const int v2 = rows_8_aligned(rgb, is, ps, w, n), yshift = y.pack ? 16 - depth : 0, cshift = u.pack ? 16 - depth : 0;
#define W2XC_TO_RGB16(SX, SY) (cm == 2 ? k_yuv16_to_rgb<2, SX, SY> : cm == 1 ? k_yuv16_to_rgb<1, SX, SY> : k_yuv16_to_rgb<0, SX, SY>)
    const auto kernel = chroma == 0 ? W2XC_TO_RGB16(true, true) : chroma == 1 ? W2XC_TO_RGB16(true, false) : W2XC_TO_RGB16(false, false);
#undef W2XC_TO_RGB16
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, y.p, y.frame, y.row, yv, yshift, u.p, v, u.frame, u.row, u.px, cshift, k.max, w, h, cw, ch, k.y_off, k.y_in,
                       k.c_mid, k.c_in, m, rgb, is, ps, v2, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}

// ---- R, G, B -> words ----
// A thread reads its block of the three planes (a block cut by an odd edge replicates its last column / row), computes the block's luma words and its one U
// and one V word, and stores only to its own samples: 16-bit stores, or -- y32: every luma row starts on a 4-byte boundary -- one 32-bit store for the two luma
// words of a row where both lie in the plane, and -- uv32: dv = du + 1 and the chroma rows start on 4-byte boundaries -- one 32-bit store for the (U, V) pair.
// Never a read-modify-write: with dpx = 2 and planes that do not interleave, the words between a plane's samples are another plane's.  No LDS.
// Loads: v2 (every row of every float plane starts on an 8-byte boundary) fetches a thread's two adjacent pixels of a row as ONE 8-byte load per plane.
template <bool SX, bool SY>
__global__ void __launch_bounds__(256) k_rgb_to_yuv16(const float *__restrict__ rgb, long long is, long long ps, int v2, int w, int h, int cw, int ch, int limited,
                                                      int max, float ys, float y0, float cs, float c0, W2xcRgbToYuv m, unsigned short *__restrict__ dy,
                                                      long long yframe, long long yrow, int y32, int yshift, unsigned short *__restrict__ du,
                                                      unsigned short *__restrict__ dv, long long cframe, long long crow, int dpx, int uv32, int cshift, int tiles_x,
                                                      long long tiles, long long turns)
{
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {
        int cx0, cy0;
        const long long f = yuv_tile_at(turn, tiles, tiles_x, YR_TCX, YR_TCY, &cx0, &cy0);
        const float *s = rgb + f * is;
        unsigned short *oy = dy + f * yframe;
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
                unsigned short *d = oy + Y * yrow + X;
                const unsigned b0 = luma_u16(p[r][0].y, limited, ys, y0, max) << yshift;
                if (SX && X + 1 < w) {
                    const unsigned b1 = luma_u16(p[r][HX].y, limited, ys, y0, max) << yshift;
                    if (y32) *reinterpret_cast<unsigned *>(d) = b0 | (b1 << 16);
                    else { d[0] = (unsigned short)b0; d[1] = (unsigned short)b1; }
                } else d[0] = (unsigned short)b0;
            }
            float cb, cr;
            chroma_mean<SX, SY>(p, &cb, &cr);
            const long long at = f * cframe + cy * crow + (long long)cx * dpx;
            const unsigned U = to_u16(cb, cs, c0, max) << cshift, V = to_u16(cr, cs, c0, max) << cshift;
            if (uv32) *reinterpret_cast<unsigned *>(du + at) = U | (V << 16);
            else {
                du[at] = (unsigned short)U;
                dv[at] = (unsigned short)V;
            }
        }
    }
}

hipError_t w2xc_launch_rgb_to_yuv16(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, int depth, W2xcU16Planes y,
                                    W2xcU16Planes u, unsigned short *v, int n, hipStream_t st)
{
    W2xcRgbToYuv m;
    int cw, ch;
    if (!matrix_from_rgb(matrix, &m) || !frame_geometry(w, h, chroma, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 || (u.px != 1 && u.px != 2) ||
        depth < 8 || depth > 16)
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int y32 = (rows_align(y, n) & 3) == 0;
    const int uv32 = u.px == 2 && v == u.p + 1 && (rows_align(u, n) & 3) == 0;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n), yshift = y.pack ? 16 - depth : 0, cshift = u.pack ? 16 - depth : 0;
    const auto kernel = chroma == 0 ? k_rgb_to_yuv16<true, true> : chroma == 1 ? k_rgb_to_yuv16<true, false> : k_rgb_to_yuv16<false, false>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, rgb, is, ps, v2, w, h, cw, ch, limited, k.max, k.y_out, k.y_off, k.c_out, k.c_mid, m, y.p, y.frame, y.row,
                       y32, yshift, u.p, v, u.frame, u.row, u.px, uv32, cshift, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
