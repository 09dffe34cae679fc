// w2xc_host_geom.hpp -- the integers of the host side of the engine (w2xc_host_pipeline.cpp, the image units w2xc_image*.cpp): which rows a unit converts and
// reads, the staging chunk sizes, which output rows finished tile rows cover, the job flags' epoch test, how a batch is cut into sub-batches, the float planes
// of the image pipelines, where the RGBA call's uint8 images lie (w2xc_image_rgba.cpp), the planes of a YUV frame and their device mirror (w2xc_image_yuv.cpp).
// No HIP header: tests/cpp/host_geom_test.cpp builds it with g++ and checks what the consumers of these numbers need.
#pragma once
#include "../../include/w2xc_hip.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace w2xc_eng {

typedef std::pair<int, int> RowSpan;   // rows [first, second)

// contiguous share of the output rows [row_begin, row_end) for unit t of nd: independent, no exchange
inline RowSpan unit_rows(int row_begin, int row_end, int t, int nd)
{
    const int R = row_end - row_begin;
    return {row_begin + (int)((long long)R * t / nd), row_begin + (int)((long long)R * (t + 1) / nd)};
}

// source rows that cover output rows [ra - hs, rb + hs) (clipped to the H output rows) of a conversion that doubles `up` times, in source coordinates
inline RowSpan src_rows(int ra, int rb, int hs, int up, int H) { return {std::max(0, ra - hs) >> up, (std::min(H, rb + hs) + up) >> up}; }

// view rows (source coordinates, relative to sy0) a band of output rows that ends at y1 reads; overlapping planes: every row of the view (svh)
inline int band_src_end(int y1, int hs, int up, int H, int sy0, bool overlap, int svh)
{
    return overlap ? svh : ((std::min(H, y1 + hs) + up) >> up) - sy0;
}

// staging granularity, whole rows: input slices of ~2 MiB; output chunks of at most ~8 MiB tapering to 1/16 of that (multiples of the 8-row tiles of the
// last-layer kernels).  w2xc_opts.host_chunk_kb overrides the maximum (test aid).
struct HostChunks { int in_rows, out_rows, out_min; };
inline HostChunks host_chunks(int host_chunk_kb, size_t in_row, size_t out_row)
{
    const size_t chunk_max = host_chunk_kb > 0 ? (size_t)host_chunk_kb << 10 : (size_t)8 << 20;
    HostChunks c;
    c.in_rows = (int)std::max<size_t>(1, std::min<size_t>(chunk_max, (size_t)2 << 20) / in_row);
    c.out_rows = (int)std::max<size_t>(8, (chunk_max / out_row) & ~(size_t)7);
    c.out_min = (int)std::max<size_t>(8, (chunk_max / 16 / out_row) & ~(size_t)7);
    return c;
}

// output rows of layer 1 per chunk while the band's input is still arriving in slices of in_chunk_rows source rows
inline int layer1_chunk(int in_chunk_rows, int up) { return std::max(8, ((in_chunk_rows << up) + 7) & ~7); }

// the call's first chunks are an eighth, a quarter, a half of a slice (the chunk that starts at output row c0): the first launch starts ~30 us into the call
// instead of behind the first 2 MiB; later chunks are whole slices, every launch of the persistent kernel has a ramp
inline int taper_chunk(int c0, int full)
{
    return c0 < full / 8 ? full / 8 : c0 < full / 8 + full / 4 ? full / 4 : c0 < full / 8 + full / 4 + full / 2 ? full / 2 : full;
}

// conv3x3_wino4 PROG: job row jr holds the band's rows [16 jr - first, 16 jr - first + 16) clipped to its R rows; what tile rows [jr, ready) cover (empty: second <= first)
inline RowSpan tile_rows_span(int jr, int ready, int first, int R) { return {std::max(0, 16 * jr - first), std::min(R, 16 * ready - first)}; }

// a job flag holds the epoch of the band whose job stored it last; epochs count up from 1 per band buffer and the comparison is signed, so the flags start
// over (zeroed, epoch 0) once the epoch has reached PROG_EPOCH_LAST
constexpr unsigned PROG_EPOCH_LAST = 0x7FFFFFFFu;
inline bool flag_reached(unsigned flag, unsigned epoch) { return (int)(flag - epoch) >= 0; }

// images per sub-batch of a host batch of n images on ndev devices: at most `sub`, and at least two sub-batches per device where there are images enough
// (uploads, launches and downloads then have something to overlap with)
inline int batch_stripe_sub(int sub, int n, int ndev) { return std::min(sub, std::max(1, (n + 2 * ndev - 1) / (2 * ndev))); }
// the sub-batches ([first image, count), in order) striped over the devices; share.size() = the devices that get any
inline std::vector<std::vector<std::pair<int, int>>> batch_stripes(int n, int sub, int ndev)
{
    const int nsub = (n + sub - 1) / sub;
    const int nd = std::min(ndev, nsub);
    std::vector<std::vector<std::pair<int, int>>> share(nd);
    for (int j = 0; j < nsub; j++) share[j % nd].push_back({j * sub, std::min(sub, n - j * sub)});
    return share;
}

// final size of the image pipeline: (w << iterations) x (h << iterations), then the optional shrink of main.cpp:158-167
inline void final_size(int w, int h, int iterations, double shrink, int *fw, int *fh)
{
    *fw = w << iterations;
    *fh = h << iterations;
    if (shrink > 0.0) {
        *fw = static_cast<int>(static_cast<double>(*fw * shrink));   // :160-165
        *fh = static_cast<int>(static_cast<double>(*fh * shrink));
    }
}

// float planes of ONE image over all levels of the Y image pipeline, every plane on a 256-byte boundary: per level Y, U and V, on level 0 a second Y for
// the noise pass; with alpha (one image: the RGBA call) every Y has an alpha plane behind it
inline size_t plane_floats(int w, int h) { return ((size_t)w * h + 63) & ~(size_t)63; }
// test-time augmentation: the variant planes of one pass on one plane -- 8 at the pass's input level, 8 at its output level -- and the most a pass of an image
// call needs of them per plane that goes through the CNN (every pass reuses them: the last scale iteration is the largest; without one, the noise pass)
inline size_t tta_pass_floats(int w, int h, int up) { return 8 * (plane_floats(w, h) + plane_floats(w << up, h << up)); }
inline size_t tta_variant_floats(int w, int h, int iterations)
{
    return iterations > 0 ? tta_pass_floats(w << (iterations - 1), h << (iterations - 1), 1) : tta_pass_floats(w, h, 0);
}
// (tta: the Y planes go through the CNN -- one per image, with alpha its alpha plane beside it in the scale passes)
inline size_t image_aux_floats(int w, int h, int iterations, double shrink, bool alpha = false, bool tta = false)
{
    const size_t ya = alpha ? 2 : 1;
    size_t need = (2 * ya + 2) * plane_floats(w, h);
    if (tta) need += ya * tta_variant_floats(w, h, iterations);
    for (int i = 1; i <= iterations; i++) need += (ya + 2) * plane_floats(w << i, h << i);
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    if (shrink > 0.0) need += (ya + 2) * plane_floats(fw, fh);
    return need;
}


inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// ---- RGBA images (w2xc_image_rgba.cpp) ----
// what ONE image of the call takes: bytes of each of its uint8 images (a multiple of 256; 0 = the call has none), and its float planes
struct RgbaImageBytes {
    size_t bled = 0, stamp = 0, res = 0, grey = 0, ares = 0;
    size_t floats = 0;
};
// where those lie for sub-batches of at most cap images: byte offsets, in this order; head = where the float planes start, bytes = where they end
struct RgbaLayout {
    size_t bled, stamp, res, grey, ares, head, bytes;
    RgbaLayout(const RgbaImageBytes &R, size_t cap)
    {
        size_t at = 0;
        const auto take = [&](size_t img) { const size_t a = at; at += cap * img; return a; };
        bled = take(R.bled); stamp = take(R.stamp); res = take(R.res); grey = take(R.grey); ares = take(R.ares);
        head = at;
        bytes = at + cap * R.floats * sizeof(float);
    }
};

// ---- YUV frames (w2xc_image_yuv.cpp) ----
// the chroma planes of a w x h frame (include/w2xc_hip.h; yuv_chroma_size of __init__.py is its mirror): 0 x 0 for W2XC_YUV_400
struct ChromaSize { int cw, ch; };
inline ChromaSize yuv_chroma_size(int w, int h, int chroma)
{
    if (chroma == W2XC_YUV_400) return {0, 0};
    return {chroma != W2XC_YUV_444 ? (w + 1) / 2 : w, chroma == W2XC_YUV_420 ? (h + 1) / 2 : h};
}
// bytes from the first to behind the last sample of a chroma row of cw samples, px samples apart, of bps bytes each (1: bytes; 2: 16-bit words)
inline size_t chroma_row_bytes(int cw, int px, int bps = 1) { return ((size_t)px * (cw - 1) + 1) * bps; }
// the float planes of one frame of the Y call: two luma planes per level; a sized call ("Sized YUV frames") whose output out_w x out_h is not the last level
// has one more, the shrunk plane (out_w = 0: the output is the last level)
inline size_t yuv_aux_floats(int w, int h, int iterations, int out_w = 0, int out_h = 0)
{
    size_t need = 2 * plane_floats(w, h);
    for (int i = 1; i <= iterations; i++) need += 2 * plane_floats(w << i, h << i);
    if (out_w && (out_w != w << iterations || out_h != h << iterations)) need += plane_floats(out_w, out_h);
    return need;
}
// ... of the call through RGB models: three per level, the noise pass's output included, and the three shrunk planes of a sized call
inline size_t yuv_rgb_aux_floats(bool noise, int w, int h, int iterations, int out_w = 0, int out_h = 0)
{
    size_t need = (noise ? 2 : 1) * plane_floats(w, h);
    for (int i = 1; i <= iterations; i++) need += plane_floats(w << i, h << i);
    if (out_w && (out_w != w << iterations || out_h != h << iterations)) need += plane_floats(out_w, out_h);
    return 3 * need;
}
// the bytes of one frame's planes: w x h luma, two planes of cw x ch chroma, bps bytes per sample
inline size_t yuv_frame_bytes(int w, int h, int cw, int ch, int bps = 1) { return ((size_t)w * h + 2 * (size_t)cw * ch) * bps; }

// The device copy of one side of a host frame call for sub-batches of at most cap frames, as byte offsets from its start: luma rows w samples apart; chroma as
// the caller has it -- planar planes (c_px = 1), or the two interleaved planes (c_px = 2; u_first: U is the lower sample, NV12 / P010) as ONE plane of rows of
// 2 cw samples --, every frame of luma and of chroma on a 256-byte boundary.  bps = bytes per sample.  bytes = what it takes: the end of the last plane's share.
struct YuvMirrorLayout {
    size_t y_stride = 0, y_frame_stride = 0;
    bool pair = false;
    size_t c_copy_row = 0;   // bytes of a chroma row the copies move (both interleaved planes at once; 0: no chroma)
    size_t c_stride = 0, c_frame_stride = 0, u = 0, v = 0;
    size_t bytes = 0;
};
inline YuvMirrorLayout yuv_mirror_layout(int c_px, bool u_first, int cap, int w, int h, int cw, int ch, int bps = 1)
{
    YuvMirrorLayout m;
    m.y_stride = (size_t)w * bps;
    m.y_frame_stride = align256((size_t)w * h * bps);
    m.bytes = m.y_frame_stride * cap;
    if (cw) {
        m.pair = c_px == 2;
        m.c_copy_row = (m.pair ? 2 * (size_t)cw : (size_t)cw) * bps;
        m.c_stride = m.c_copy_row;
        const size_t plane = align256(m.c_copy_row * ch), c0 = m.bytes;
        m.c_frame_stride = m.pair ? plane : 2 * plane;
        if (m.pair) { m.u = c0 + (u_first ? 0 : bps); m.v = c0 + (u_first ? bps : 0); }
        else { m.u = c0; m.v = c0 + plane; }
        m.bytes += m.c_frame_stride * cap;
    }
    return m;
}

// ---- the launch grid of the six YUV tile kernels (w2xc_yuv_tile.h gives the tile sizes and the caps of w2xc_kernels.h) ----
// Tiles of all frames -- or planes: per_tile turns per tile -- are the turns of one grid-stride loop over at most `cap` workgroups
struct YuvTileGrid {
    int tiles_x;
    long long tiles, turns;
    unsigned grid;
};
inline YuvTileGrid yuv_tile_grid(int tiles_x, int tiles_y, long long per_tile, long long cap)
{
    const long long tiles = (long long)tiles_x * tiles_y, turns = tiles * per_tile;
    return {tiles_x, tiles, turns, (unsigned)(turns > cap ? cap : turns)};
}
// the bicubic 2x of chroma: quads 0 .. ow / 2 and 0 .. oh / 2 hold the ow x oh outputs, tqx x tqy quads a tile
inline YuvTileGrid chroma2x_tile_grid(int ow, int oh, long long per_tile, int tqx, int tqy, long long cap)
{
    return yuv_tile_grid((ow / 2 + tqx) / tqx, (oh / 2 + tqy) / tqy, per_tile, cap);
}
// the two ends of the RGB route: cw x ch chroma samples, tcx x tcy of them a tile, a turn per tile and frame
inline YuvTileGrid yuv_rgb_tile_grid(int cw, int ch, int n, int tcx, int tcy, long long cap)
{
    return yuv_tile_grid((cw + tcx - 1) / tcx, (ch + tcy - 1) / tcy, n, cap);
}


// ---- the chroma of a sized frame call ("Sized YUV frames": k_chroma_resize_u8 / _u16, w2xc_yuv_sized.hip / w2xc_yuv16_sized.hip) ----
// (these few are the kernels' own arithmetic too: host and device where a HIP compiler reads them, plain C++ elsewhere)
#if defined(__HIP__)
#define W2XC_GEOM_HD __host__ __device__
#else
#define W2XC_GEOM_HD
#endif
// W2XC_ITERATIONS_AUTO: the smallest k with (w << k) >= out_w and (h << k) >= out_h; 5 where 4 steps do not reach (the range check refuses it)
inline int sized_auto_iterations(int w, int h, int out_w, int out_h)
{
    int k = 0;
    while (k < 5 && (((long long)w << k) < out_w || ((long long)h << k) < out_h)) k++;
    return k;
}
// One axis of the resize: r = (double)luma_in / luma_out, the LUMA ratio (<= 1: the output is never smaller than the input), and o, the offset of a chroma
// sample against its coordinate: 0.5 on a centred or unsubsampled axis, 0.25 on a co-sited one.  Output sample m reads source coordinate
// pos = (m + o) * r - o: three double operations in this order; s = floor(pos), t = (float)(pos - s), taps s - 1 .. s + 2 clamped into the plane.
struct ChromaAxis { double r, o; };
inline ChromaAxis chroma_axis(int luma_in, int luma_out, bool subsampled, bool cosited) { return {(double)luma_in / (double)luma_out, subsampled && cosited ? 0.25 : 0.5}; }
W2XC_GEOM_HD inline double chroma_resize_pos(int m, double r, double o)
{
    const double a = (double)m + o;
    const double b = a * r;
    return b - o;
}
W2XC_GEOM_HD inline int chroma_resize_floor(double pos) { return (int)floor(pos); }
// A tile of outputs that starts at m0 keeps its source window in LDS from source sample chroma_resize_origin(m0) on: the first tap of its first output.
// With r <= 1 the floors of `len` consecutive outputs span at most `len` source samples, so the window with its taps is at most len + 3 wide (32 -> 35, 16 -> 19:
// the window of the 2x kernels); tests/cpp/yuv_sized_geom_test.cpp holds that bound over a sweep of ratios and sizes.
W2XC_GEOM_HD inline int chroma_resize_origin(int m0, double r, double o) { return chroma_resize_floor(chroma_resize_pos(m0, r, o)) - 1; }
// the launch grid: tiles of tx x ty OUTPUT samples, per_tile turns per tile (frames, or frames x planes)
inline YuvTileGrid chroma_resize_tile_grid(int ow, int oh, long long per_tile, int tx, int ty, long long cap)
{
    return yuv_tile_grid((ow + tx - 1) / tx, (oh + ty - 1) / ty, per_tile, cap);
}

}  // namespace w2xc_eng
