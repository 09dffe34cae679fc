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
#include "w2xc_yuv_launch.h" // the kernels' parameter lists, the co-sited instantiations

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
__global__ void __launch_bounds__(256) k_yuv16_to_rgb(W2XC_YUV16_TO_RGB_PARAMS)
{
    constexpr bool CX = false, CY = false;   // centred siting (the co-sited forms: w2xc_yuv16_rgb_sited.hip)
#include "w2xc_yuv16_to_rgb_body.inc"
}

// chroma: the layout with W2XC_CHROMA_COSITED_* or-ed on, or with none -- the same grid, load paths and stores, with a flag the kernel from w2xc_yuv16_rgb_sited.hip
hipError_t w2xc_launch_yuv16_to_rgb(W2xcU16Planes y, W2xcU16Planes u, const unsigned short *v, int w, int h, int chroma, int range, int matrix, int depth, float *rgb,
                                    long long is, long long ps, int n, hipStream_t st)
{
    W2xcYuvToRgb m;
    ChromaLayout c;
    int cw, ch;
    if (!matrix_to_rgb(matrix, &m) || !chroma_layout(chroma, &c) || !frame_geometry(w, h, c.layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 ||
        (u.px != 1 && u.px != 2) || depth < 8 || depth > 16)
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int yv = (rows_align(y, n) & 7) == 0;
    int cm = 0;
    if (u.px == 1 && ((rows_align(u, n) | reinterpret_cast<size_t>(v)) & 7) == 0) cm = 1;
    else if (u.px == 2 && v == u.p + 1 && (rows_align(u, n) & 3) == 0) cm = 2;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    const int v2 = rows_8_aligned(rgb, is, ps, w, n), yshift = y.pack ? 16 - depth : 0, cshift = u.pack ? 16 - depth : 0;
#define W2XC_TO_RGB16(SX, SY) (cm == 2 ? k_yuv16_to_rgb<2, SX, SY> : cm == 1 ? k_yuv16_to_rgb<1, SX, SY> : k_yuv16_to_rgb<0, SX, SY>)
    const Yuv16ToRgbKernel kernel = c.cx || c.cy    ? yuv16_to_rgb_sited_kernel(cm, c.layout, c.cx, c.cy)
                                    : c.layout == 0 ? W2XC_TO_RGB16(true, true)
                                    : c.layout == 1 ? W2XC_TO_RGB16(true, false)
                                                    : W2XC_TO_RGB16(false, false);
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
__global__ void __launch_bounds__(256) k_rgb_to_yuv16(W2XC_RGB_TO_YUV16_PARAMS)
{
    constexpr bool CX = false, CY = false;   // centred siting (the co-sited forms: w2xc_yuv16_rgb_sited.hip)
#include "w2xc_rgb_to_yuv16_body.inc"
}

hipError_t w2xc_launch_rgb_to_yuv16(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, int depth, W2xcU16Planes y,
                                    W2xcU16Planes u, unsigned short *v, int n, hipStream_t st)
{
    W2xcRgbToYuv m;
    ChromaLayout c;
    int cw, ch;
    if (!matrix_from_rgb(matrix, &m) || !chroma_layout(chroma, &c) || !frame_geometry(w, h, c.layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 ||
        (u.px != 1 && u.px != 2) || depth < 8 || depth > 16)
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int y32 = (rows_align(y, n) & 3) == 0;
    const int uv32 = u.px == 2 && v == u.p + 1 && (rows_align(u, n) & 3) == 0;
    const W2xcU16Scale k = u16_scale(depth, range != 0);
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n), yshift = y.pack ? 16 - depth : 0, cshift = u.pack ? 16 - depth : 0;
    const RgbToYuv16Kernel kernel = c.cx || c.cy    ? rgb_to_yuv16_sited_kernel(c.layout, c.cx, c.cy)
                                    : c.layout == 0 ? k_rgb_to_yuv16<true, true>
                                    : c.layout == 1 ? k_rgb_to_yuv16<true, false>
                                                    : k_rgb_to_yuv16<false, false>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, rgb, is, ps, v2, w, h, cw, ch, limited, k.max, k.y_out, k.y_off, k.c_out, k.c_mid, m, y.p, y.frame, y.row,
                       y32, yshift, u.p, v, u.frame, u.row, u.px, uv32, cshift, g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
