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
#include "w2xc_yuv_launch.h" // the kernels' parameter lists, the co-sited instantiations

#define YR_YLD (2 * YR_TCX + 4)     // bytes per LDS row of luma: the widest tile and one dword of padding
static_assert((YR_YLD & 3) == 0, "a luma row in LDS is whole dwords");

// ---- bytes -> R, G, B ----
// The chroma tile with a one-sample halo along each subsampled axis (coordinates clamped into the plane, as the taps are) is fetched once for U and once for V
// and kept in LDS as the bytes' values in floats; the luma tile is kept as bytes.  DW: luma rows start on 4-byte boundaries, and so do the rows of planar
// chroma: an aligned group of four samples inside the row is one dword load by one thread; the rim, and interleaved chroma (spx = 2), go byte by byte.
// Stores: a thread's two pixels of a row are adjacent; v2 (every row of every plane starts on an 8-byte boundary: w, ps, is even) makes them ONE 8-byte store per
// plane, a wave's stores a contiguous run of the row; otherwise two float stores.
template <bool DW, bool SX, bool SY>
__global__ void __launch_bounds__(256) k_yuv8_to_rgb(W2XC_YUV8_TO_RGB_PARAMS)
{
    constexpr bool CX = false, CY = false;   // centred siting (the co-sited forms: w2xc_yuv_rgb_sited.hip)
#include "w2xc_yuv8_to_rgb_body.inc"
}

// chroma: the layout with W2XC_CHROMA_COSITED_* or-ed on, or with none -- the same grid, load paths and stores, with a flag the kernel from w2xc_yuv_rgb_sited.hip
hipError_t w2xc_launch_yuv8_to_rgb(W2xcU8Planes y, W2xcU8Planes u, const unsigned char *v, int w, int h, int chroma, int range, int matrix, float *rgb, long long is,
                                   long long ps, int n, hipStream_t st)
{
    W2xcYuvToRgb m;
    ChromaLayout c;
    int cw, ch;
    if (!matrix_to_rgb(matrix, &m) || !chroma_layout(chroma, &c) || !frame_geometry(w, h, c.layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 ||
        (u.px != 1 && u.px != 2))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    size_t align = rows_align(y, n);
    if (u.px == 1) align |= rows_align(u, n) | reinterpret_cast<size_t>(v);
    const bool dw = (align & 3) == 0;
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n);
#define W2XC_TO_RGB(SX, SY) (dw ? k_yuv8_to_rgb<true, SX, SY> : k_yuv8_to_rgb<false, SX, SY>)
    const Yuv8ToRgbKernel kernel = c.cx || c.cy    ? yuv8_to_rgb_sited_kernel(dw, c.layout, c.cx, c.cy)
                                   : c.layout == 0 ? W2XC_TO_RGB(true, true)
                                   : c.layout == 1 ? W2XC_TO_RGB(true, false)
                                                   : W2XC_TO_RGB(false, false);
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
// (chroma_u8, the rounding of cb and cr to a byte: w2xc_yuv_px.h)

template <bool SX, bool SY>
__global__ void __launch_bounds__(256) k_rgb_to_yuv8(W2XC_RGB_TO_YUV8_PARAMS)
{
    constexpr bool CX = false, CY = false;   // centred siting (the co-sited forms: w2xc_yuv_rgb_sited.hip)
#include "w2xc_rgb_to_yuv8_body.inc"
}

hipError_t w2xc_launch_rgb_to_yuv8(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, W2xcU8Planes y, W2xcU8Planes u,
                                   unsigned char *v, int n, hipStream_t st)
{
    W2xcRgbToYuv m;
    ChromaLayout c;
    int cw, ch;
    if (!matrix_from_rgb(matrix, &m) || !chroma_layout(chroma, &c) || !frame_geometry(w, h, c.layout, &cw, &ch) || n < 1 || !y.p || !u.p || !v || !rgb || y.px != 1 ||
        (u.px != 1 && u.px != 2))
        return hipErrorInvalidValue;
    const YuvTileGrid g = w2xc_eng::yuv_rgb_tile_grid(cw, ch, n, YR_TCX, YR_TCY, W2XC_YUVRGB_GRID_MAX);
    const int y16 = (rows_align(y, n) & 1) == 0;
    const int limited = range != 0, v2 = rows_8_aligned(rgb, is, ps, w, n);
    const RgbToYuv8Kernel kernel = c.cx || c.cy    ? rgb_to_yuv8_sited_kernel(c.layout, c.cx, c.cy)
                                   : c.layout == 0 ? k_rgb_to_yuv8<true, true>
                                   : c.layout == 1 ? k_rgb_to_yuv8<true, false>
                                                   : k_rgb_to_yuv8<false, false>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(256), 0, st, rgb, is, ps, v2, w, h, cw, ch, limited, m, y.p, y.frame, y.row, y16, u.p, v, u.frame, u.row, u.px,
                       g.tiles_x, g.tiles, g.turns);
    return hipGetLastError();
}
