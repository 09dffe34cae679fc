// w2xc_kernels.h -- launch interface between the engine (w2xc_rows.cpp, see w2xc_engine.hpp) and the gfx950
// kernels (w2xc_kernels.hip).  One "layer launch" computes
//     out(y,x,o) = leaky( bias[o] + sum_{i,r,c} W[o][i][r][c] * in(clamp(y+r+off_y), clamp(x+c+off_x), i) )
// which is Model::filterWorker (/root/reference/src/modelHandler.cpp:117-159) on one haloed
// band: off = 0 gives the shrinking "valid" conv used inside convertWithModels,
// off = -1 with out dims == in dims gives the same-size BORDER_REPLICATE conv of Model::filter,
// off = -n_layers on layer 1 folds cv::copyMakeBorder (convertRoutine.cpp:35,96) into the load.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "w2xc_pack.hpp"   // W2xcKernelKind, the shape predicates and the weight packers (host code without HIP)

struct W2xcConvDesc {
    const float *in;
    float *out;
    const float *wpk;    // weights packed for the chosen kernel
    const float *bias;   // float[cout]  ((float)double, modelHandler.cpp:147 via cv::add scalar rule)
    int cin, cout;
    // element (y,x,c) lives at base[y*rs + x*ps + c*cs] (units: floats)
    long long in_rs, in_ps, in_cs;
    long long out_rs, out_ps, out_cs;
    int in_h, in_w;      // extent of the input view (clamp bounds)
    int out_h, out_w;    // region to compute
    int off_y, off_x;
    // W2XC_K_FIRST_U8 / W2XC_K_LAST_U8 (the RGB image pipeline): `in` / `out` points at the BYTES of an interleaved uint8 image and in_* / out_* are byte
    // strides (row stride, 3, 1); the kernels convert in their load / store (conv3x3_first / conv3x3_last, U8).
    // N1 (nearest-neighbour 2x of main.cpp:132-140 folded into the load): in_h/in_w and all offsets are
    // in UPSCALED coordinates, memory is addressed at (y >> in_shift, x >> in_shift).  0 or 1; only the
    // first-layer kernels (conv3x3_first, conv3x3_direct) honour it.
    int in_shift;
    // split kernels (w2xc_split.hip): an activation tensor is `terms` 16-bit (bf16 / fp16) term planes, each channel-group
    // blocked: element (t, c, y, x) at t*ts + (c / G)*gs + y*rs + x*G + c % G  (ELEMENTS; G = 16).
    // out_terms = 0 stores plain fp32 NHWC.
    int terms, out_terms;
    long long in_ts, out_ts, in_gs, out_gs;
    int fmt;             // 0 = bf16 terms, 1 = fp16 terms (W2XC_PRECISION_FP16X2)
    float acc_scale;     // fp16: 1 / (power-of-two weight scale of this layer), applied to the accumulators
    // out_terms = 9: the LAST layer (cout = 1) is computed inside this layer's epilogue; `out` receives its partial sums
    // G[half][tap][y][x] fp32 (out_ts = half stride, out_gs = tap-plane stride, out_rs = row stride, in floats) and
    // W2XC_K_LAST_GATHER adds halves and taps (in = G, in_ts / in_gs / in_rs as written, `halves` halves).
    // W2XC_K_FIRST2_SPLIT (layers 1 + 2 in one kernel): `in` / in_* / off_* / in_shift describe LAYER 1's input plane,
    // wpk / bias / acc_scale / terms / fmt / out_* layer 2; layer 1's own weights (W2XC_K_FIRST image) and bias:
    const float *w1pk;
    const float *bias1;
    const void *w7pk;    // last layer's weights as MFMA A fragments (w2xc_split_pack_last)
    float g_scale;       // fp16: 1 / (power-of-two scale of the last layer's weights)
    int halves;
    // conv3x3_wino: 0 / 1 = the 2x2 output blocks start at row -wino_py of this launch's region, so that they sit on EVEN rows of the
    // layer's whole output whatever row the band starts at -- a pixel's arithmetic then does not depend on the banding.
    int wino_py;
    // conv3x3_wino4 with out_terms = 9 and prog_cnt != NULL (PROG): the launch finishes the fused one-plane last layer itself, in row order -- g_out = that
    // layer's output rows (g_h x g_w, row stride g_out_rs floats), output row y reads the partial tap rows y + g_off .. y + g_off + 2 of `out`, g_bias its
    // bias; prog_cnt = w2xc_wino4_prog_counters() job counters (zeroed by the launcher on the stream).
    unsigned *prog_cnt;
    float *g_out;
    const float *g_bias;
    long long g_out_rs;
    int g_h, g_w, g_off;
    // ... with prog_flags != NULL (page-locked HOST memory, one word per job = (tile row, group of 8 tile columns), w2xc_wino4_prog_jobs()) every finished job
    // stores prog_epoch there at system scope behind its output rows: the host pipeline's drainer ships rows while the launch is still running
    unsigned *prog_flags;
    unsigned prog_epoch;
};

// Batch launches (w2xc_convert_batch*): `batch` images of identical geometry, each described by the W2xcConvDesc of the single-image launch; image i's
// input / output start in_bs / out_bs floats after image 0's (for a fused-last producer out_bs is one image's block of tap planes).  `items` = the
// single-image launch's item (first2: tile) count: the batch kernels walk batch x items items, image-major, and add i * stride to their 64-bit scalar
// bases only -- every 32-bit lane offset and every range check of the single-image launcher stays per image.  (A struct of its own rather than fields
// appended to W2xcConvDesc: that struct is the by-value argument of every existing kernel, and growing it would move their kernel-argument offsets.)
// The uint8 forms (W2XC_K_FIRST_U8 / W2XC_K_LAST_U8): the descriptor's strides on the uint8 side are BYTES, and so is that side's image stride -- in_bs of
// conv3x3_first_batch<U8>, out_bs of conv3x3_last_batch<U8>; the other side (a workspace of floats) stays in floats.
struct W2xcBatchDesc {
    int batch;
    int items;
    long long in_bs, out_bs;
};

// Enqueue one layer on `stream`.  Returns hipSuccess or the launch error.
hipError_t w2xc_launch_conv(W2xcKernelKind kind, const W2xcConvDesc &d, hipStream_t stream);

// Winograd F(2x2, 3x3) on the fp32 MFMA (w2xc_wino.hip): the same layer as W2XC_K_MFMA (NHWC fp32 in / out) with 2.25x fewer MFMAs,
// for the shapes w2xc_wino_supported() names; d.wpk = the w2xc_wino_pack image (16 * cin * cout floats).
hipError_t w2xc_launch_wino(const W2xcConvDesc &d, hipStream_t stream);
// Winograd F(4x4,3x3) on PLANAR activations (w2xc_wino4.hip): in_ps = 1 / in_cs = plane stride; out planar (out_ps = 1) or NHWC (out_cs = 1, out_ps = cout);
// d.wpk = the w2xc_wino4_pack image (36 * cin * cout floats), d.wino_py = first output row mod 4, off_x a non-negative multiple of 4
// d.out_terms = 9: the one-plane LAST layer in conv3x3_wino4's epilogue; d.w7pk = w2xc_wino4_pack_last image, `out` = partial tap planes
// G[64-plane block][tap][y][x] (out_ts / out_gs / out_rs), finished by W2XC_K_LAST_GATHER with halves = cout / 64
hipError_t w2xc_launch_wino4(const W2xcConvDesc &d, hipStream_t stream);
// layers 1 + 2 of the fp32 path in one launch (w2xc_first2_wino4.hip): `in` / in_* / in_h / in_w / in_shift describe LAYER 1's one-plane input, off_y / off_x =
// layer 1's offsets + layer 2's, w1pk / bias1 = layer 1's W2XC_K_FIRST image and bias; wpk = the w2xc_first2_wino4_pack image (36 * 32 * 32 floats), bias,
// planar out, out_h / out_w / wino_py (first output row mod 4) = layer 2's region
hipError_t w2xc_launch_first2_wino4(const W2xcConvDesc &d, hipStream_t stream);
// batch forms (bit-identical per image to the launches above; b.items is set by the launcher): conv3x3_wino4_batch (planar in, planar out or FUSE7, no
// PROG; the layers w2xc_wino4_batch_supported names), conv3x3_first2_wino4_batch, conv3x3_last_gather_x4_batch.
hipError_t w2xc_launch_wino4_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
hipError_t w2xc_launch_first2_wino4_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
hipError_t w2xc_launch_last_gather_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
// ... and of the multi-plane (RGB) chains: conv3x3_first_batch / conv3x3_last_batch (kind = W2XC_K_FIRST / _FIRST_U8 with three planes in, W2XC_K_LAST / _LAST_U8
// with three planes out; w2xc_conv_batch.hip), conv3x3_wino_batch (w2xc_wino_batch_supported), and through w2xc_launch_wino4_batch the layouts
// w2xc_wino4_batch_layout_supported names (conv3x3_wino4_batch_l: 32 NHWC planes in and / or NHWC out)
hipError_t w2xc_launch_conv_batch(W2xcKernelKind kind, const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
hipError_t w2xc_launch_wino_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);

// split kernels (w2xc_split.hip); d.wpk = the w2xc_split_pack image (W2XC_K_FIRST_SPLIT: the W2XC_K_FIRST image)
hipError_t w2xc_launch_split_mid(const W2xcConvDesc &d, hipStream_t stream);
hipError_t w2xc_launch_split_first(const W2xcConvDesc &d, hipStream_t stream);
hipError_t w2xc_launch_first2_split(const W2xcConvDesc &d, hipStream_t stream);
// last layer fused into a two-term mid layer (d.w7pk = the w2xc_split_pack_last image)
hipError_t w2xc_launch_last_gather(const W2xcConvDesc &d, hipStream_t stream);

// the head of an upconv model (w2xc_upconv.hip; kind = W2XC_K_UPCONV / W2XC_K_UPCONV_U8): `in` = the NHWC view of z (in_ps = cin in {32, 64, 128, 256}), off_y / off_x
// = the view's row / column of z row y0 / column 0, out_h x out_w = the SOURCE pixels; writes 2 out_h x 2 out_w pixels of cout in {1, 3} planes (planar
// floats, or -- U8 -- an interleaved uint8 image with byte strides), out_rs = the row stride of the doubled image; d.wpk = the w2xc_upconv_pack image
hipError_t w2xc_launch_upconv(W2xcKernelKind kind, const W2xcConvDesc &d, hipStream_t stream);
// conv3x3_wino4 128 -> 256 planes, planar in, NHWC out (the layer in front of the head of the published upconv_7 topology; an object of its own)
hipError_t w2xc_launch_wino4_wide(const W2xcConvDesc &d, hipStream_t stream);
// their batch forms (bit-identical per image): upconv4x4_head_batch -- b.in_bs floats between the images' NHWC planes, b.out_bs floats (U8: bytes) between
// their outputs --, and conv3x3_wino4_batch_l<128, 256> through w2xc_launch_wino4_batch (w2xc_wino4_batch_layout_supported)
hipError_t w2xc_launch_upconv_batch(W2xcKernelKind kind, const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);

// strided element copy (planar <-> NHWC repack at the Model::filter boundary)
hipError_t w2xc_launch_repack(const float *src, long long s_rs, long long s_ps, long long s_cs,
                              float *dst, long long d_rs, long long d_ps, long long d_cs,
                              int h, int w, int c, hipStream_t stream);

// replicate-padded planar copy (Model::filter's BORDER_REPLICATE made explicit for conv3x3_wino4): dst is (h + 2 pad) x (w + 2 pad) per plane
hipError_t w2xc_launch_pad_planar(const float *src, long long s_rs, long long s_ps, long long s_cs, float *dst, long long d_rs, long long d_cs,
                                  int h, int w, int c, int pad, hipStream_t stream);

// N2 (w2xc_color.hip): colour front/back end and U/V bicubic of the CLI scale loop (main.cpp:74-76,144,171-172).  One kernel per stage (k_px<Stage>): every
// one-image launcher here is its batch launch with n = 1.
hipError_t w2xc_launch_u8_to_yuv(const unsigned char *src, size_t stride, int w, int h, float *y, float *u, float *v, hipStream_t st);
hipError_t w2xc_launch_yuv_to_u8(const float *y, const float *u, const float *v, int w, int h, unsigned char *dst, size_t stride, hipStream_t st);
hipError_t w2xc_launch_resize2x_cubic(const float *src, int w, int h, float *dst, hipStream_t st);
hipError_t w2xc_launch_resize_linear(const float *src, int sw, int sh, float *dst, int dw, int dh, hipStream_t st);
// their batch forms (w2xc_process_image_u8_batch*), one launch for a sub-batch of n images: image i at src / dst + i * img_stride BYTES, the float planes
// of image (plane) i at base + i * ps FLOATS.  The image index moves only the 64-bit bases: per output element the arithmetic does not depend on n.
hipError_t w2xc_launch_u8_to_yuv_batch(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *y, float *u, float *v,
                                       long long ps, int n, hipStream_t st);
hipError_t w2xc_launch_yuv_to_u8_batch(const float *y, const float *u, const float *v, long long ps, int w, int h, unsigned char *dst, size_t img_stride,
                                       size_t stride, int n, hipStream_t st);
// the RGB pipeline (w2xc_process_image_rgb_u8*): uint8 / 255 on the three channels as given <-> three planar float planes, saturate(rint(255 x)) back.
// Batch forms: the three planes of image i at planes + i * is + {0, 1, 2} * ps FLOATS.
hipError_t w2xc_launch_u8_to_rgb(const unsigned char *src, size_t stride, int w, int h, float *p0, float *p1, float *p2, hipStream_t st);
hipError_t w2xc_launch_rgb_to_u8(const float *p0, const float *p1, const float *p2, int w, int h, unsigned char *dst, size_t stride, hipStream_t st);
hipError_t w2xc_launch_u8_to_rgb_batch(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *planes, long long ps, long long is,
                                       int n, hipStream_t st);
hipError_t w2xc_launch_rgb_to_u8_batch(const float *planes, long long ps, long long is, int w, int h, unsigned char *dst, size_t img_stride, size_t stride,
                                       int n, hipStream_t st);
// n planes src + p * sps -> dst + p * dps (the U and V planes of a sub-batch adjoin: n = 2 x images)
hipError_t w2xc_launch_resize2x_cubic_batch(const float *src, long long sps, int w, int h, float *dst, long long dps, int n, hipStream_t st);
// n planes (Y, U, V of a sub-batch: n = 3 x images): plane p < ny at src_y + p * sps, the others at src_uv + (p - ny) * sps; -> dst + p * dps
hipError_t w2xc_launch_resize_linear_batch(const float *src_y, const float *src_uv, int ny, long long sps, int sw, int sh, float *dst, long long dps, int dw,
                                           int dh, int n, hipStream_t st);
// RGBA images (w2xc_process_image_rgba_u8*), n images of one size per launch (image i at a byte pointer + i * its image stride, its float plane at a +
// i * ps floats): the colour bleed under transparent pixels -- `passes` <= 65534 passes from the RGBA images src into the packed 3-channel images dst; up to
// W2XC_BLEED_TILED_MAX passes are one launch (one pass: RgbaBleedFirst alone; more: the tiled kernel) and touch no stamp (nullptr will do), more run in place on dst with stamp = n planes of w * h 16-bit words of
// scratch, stamp_stride words apart, written before they are read -- alpha -> a float plane (u8 / 255) or a packed grey image (A, A, A), and the merge of
// a packed 3-channel result with alpha -- a float plane (saturate(rint(255 a))) or a byte a_px apart in rows a_stride apart -- into 4-byte pixels.
#define W2XC_BLEED_TILED_MAX 16
inline bool w2xc_bleed_stamps(int passes) { return passes > W2XC_BLEED_TILED_MAX; }   // (the pass chain alone has stamps)
hipError_t w2xc_launch_rgba_bleed(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, int passes, unsigned char *dst, size_t dst_img_stride,
                                  size_t dst_stride, unsigned short *stamp, size_t stamp_stride, int n, hipStream_t st);
hipError_t w2xc_launch_alpha_to_plane(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, float *a, long long ps, int n, hipStream_t st);
hipError_t w2xc_launch_alpha_to_grey(const unsigned char *src, size_t img_stride, size_t stride, int w, int h, unsigned char *dst, size_t dst_img_stride,
                                     size_t dst_stride, int n, hipStream_t st);
hipError_t w2xc_launch_merge_rgba(const unsigned char *rgb, size_t rgb_img_stride, size_t rgb_stride, const float *a, long long ps, int w, int h,
                                  unsigned char *dst, size_t img_stride, size_t stride, int n, hipStream_t st);
hipError_t w2xc_launch_merge_rgba_u8(const unsigned char *rgb, size_t rgb_img_stride, size_t rgb_stride, const unsigned char *a, size_t a_img_stride, size_t a_stride,
                                     int a_px, int w, int h, unsigned char *dst, size_t img_stride, size_t stride, int n, hipStream_t st);

// test-time augmentation (w2xc_tta.hip): T_k, k = 0..7 = horizontal flip if k & 1, then vertical flip if k & 2, then transpose if k & 4.  Variant planes have
// contiguous rows and lie ps floats apart: upright (k, i) at up + (k n + i) ps, transposed (k, i) at tr + ((k - 4) n + i) ps.
// spread: n source planes of w x h (plane i at src + i * sps, rows srs floats apart) -> their 8 n variants.
// gather: 8 n result planes (upright ones w x h) -> n planes (plane i at dst + i * dps, rows drs apart): the fp32 sum of T_k^-1 in the order k = 0..7, * 0.125f.
hipError_t w2xc_launch_tta_spread(const float *src, long long sps, long long srs, int w, int h, float *up, float *tr, long long ps, int n, hipStream_t st);
hipError_t w2xc_launch_tta_gather(const float *up, const float *tr, long long ps, int w, int h, float *dst, long long dps, long long drs, int n, hipStream_t st);
// ... with the uint8 image at the outer side (w2xc_tta_u8.hip).  spread_u8: n interleaved images (image i at src + i * img_stride BYTES, rows `stride` bytes
// apart, pixels px = 3 or 4 bytes) -> the 8 variants of their 3 n planes, plane 3 i + c = byte ch0 + c * ch_step of each pixel / 255 (ch_step = 0: three times
// the same byte).  gather_u8: 8 m result planes, m = planes_per_image * n -> byte byte0 + c, c < n_ch, of each pixel of image i = to_u8 of the gather's sum
// for plane planes_per_image * i + first_plane + c; byte stores, nothing else is written.
hipError_t w2xc_launch_tta_spread_u8(const unsigned char *src, size_t img_stride, size_t stride, int px, int ch0, int ch_step, int w, int h, float *up,
                                     float *tr, long long ps, int n, hipStream_t st);
hipError_t w2xc_launch_tta_gather_u8(const float *up, const float *tr, long long ps, int w, int h, unsigned char *dst, size_t img_stride, size_t stride, int px,
                                     int byte0, int n_ch, int planes_per_image, int first_plane, int n, hipStream_t st);

// ---- YUV frames (w2xc_yuv.hip; the arithmetic: include/w2xc_hip.h, "YUV frames") ----
// One plane of each of n frames, in bytes: frame i's at p + i * frame bytes, rows `row` bytes apart, samples px bytes apart (1 = planar, 2 = one of two interleaved
// planes: NV12's U at p, V at p + 1).
struct W2xcU8Planes {
    unsigned char *p;
    long long frame, row;
    int px;
};
// luma bytes -> float planes with contiguous rows, plane i at dst + i * ps floats, and back; range = W2XC_RANGE_*
hipError_t w2xc_launch_y8_to_plane(W2xcU8Planes src, int w, int h, int range, float *dst, long long ps, int n, hipStream_t st);
hipError_t w2xc_launch_plane_to_y8(const float *src, long long ps, int w, int h, int range, W2xcU8Planes dst, int n, hipStream_t st);
// the bicubic 2x of chroma on bytes: the planes su (and sv: nullptr = one plane per frame) of cw x ch samples of n frames -> the leading ow x oh samples
// (ow <= 2 cw, oh <= 2 ch) of their enlargements at du (and dv); bytes of Resize2xCubic + to_u8 on (float)byte * (float)(1.0 / 255.0).  One launch.
// cosited: 0 = chroma centred between luma samples, or W2XC_CHROMA_COSITED_X | W2XC_CHROMA_COSITED_Y for chroma that sits ON luma column / row 2k
// (include/w2xc_hip.h, "Chroma siting": the instantiations of w2xc_yuv_sited.hip, the same grid and load path); any other bit is hipErrorInvalidValue
hipError_t w2xc_launch_chroma2x_u8(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, unsigned char *dv, int ow, int oh, int cosited, int n,
                                   hipStream_t st);
// ... and chroma bytes as they are (no 2x step): cw x ch samples per plane
hipError_t w2xc_launch_chroma_copy_u8(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, unsigned char *dv, int n, hipStream_t st);
// the grid rule of w2xc_launch_chroma2x_u8 / _u16 (chroma2x_tile_grid, w2xc_host_geom.hpp): tiles of W2XC_CHROMA_TQX x
// W2XC_CHROMA_TQY output quads, at most W2XC_CHROMA_GRID_MAX workgroups
#define W2XC_CHROMA_TQX 32
#define W2XC_CHROMA_TQY 16
#define W2XC_CHROMA_GRID_MAX 2048

// ---- YUV frames through RGB models (w2xc_yuv_rgb.hip; the arithmetic: include/w2xc_hip.h, "YUV frames through RGB models") ----
// The constants of a colour matrix as the kernels take them: doubles from the two luma weights, each rounded once to float (by the launchers).
struct W2xcYuvToRgb { float cRV, cBU, cGV, cGU; };
struct W2xcRgbToYuv { float Kr, Kg, Kb, iBU, iRV; };
// n frames (luma y: px = 1; chroma u and v: one W2xcU8Planes geometry for both, px = 1 or 2) -> their 3 n float planes with contiguous rows of w: frame i's R, G
// and B at rgb + i * is + {0, 1, 2} * ps FLOATS; chroma = W2XC_YUV_420 / _422 / _444 with W2XC_CHROMA_COSITED_* or-ed on as the interface takes it (a flag picks
// the instantiations of w2xc_yuv_rgb_sited.hip, the same grid, load paths and stores; a flag on an axis the layout does not subsample is hipErrorInvalidValue:
// chroma_layout, w2xc_yuv_px.h), range = W2XC_RANGE_*, matrix = W2XC_MATRIX_*.  One launch.
hipError_t w2xc_launch_yuv8_to_rgb(W2xcU8Planes y, W2xcU8Planes u, const unsigned char *v, int w, int h, int chroma, int range, int matrix, float *rgb, long long is,
                                   long long ps, int n, hipStream_t st);
// ... and back: 3 n float planes of w x h -> the bytes of n frames.  One launch; only the frames' own samples are written.
hipError_t w2xc_launch_rgb_to_yuv8(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, W2xcU8Planes y, W2xcU8Planes u,
                                   unsigned char *v, int n, hipStream_t st);
// the grid rule of these launchers and their 16-bit twins (yuv_rgb_tile_grid, w2xc_host_geom.hpp): tiles of W2XC_YUVRGB_TCX x
// W2XC_YUVRGB_TCY chroma samples of one frame, at most W2XC_YUVRGB_GRID_MAX workgroups
#define W2XC_YUVRGB_TCX 32
#define W2XC_YUVRGB_TCY 16
#define W2XC_YUVRGB_GRID_MAX 2048

// ---- 16-bit YUV frames (w2xc_yuv16.hip, w2xc_yuv16_rgb.hip; the arithmetic: include/w2xc_hip.h, "16-bit YUV frames") ----
// One plane of each of n frames, in 16-bit words that hold a value of `depth` bits: frame i's at p + i * frame WORDS, rows `row` words apart, samples px words
// apart (1 = planar, 2 = one of two interleaved planes: P010's U at p, V at p + 1); pack = W2XC_PACK_LOW (0: the value in the low bits) / W2XC_PACK_HIGH (1).
struct W2xcU16Planes {
    unsigned short *p;
    long long frame, row;
    int px, pack;
};
// the launchers of the sections above on words: the same arguments -- `cosited` and the flags in `chroma` too: the instantiations of w2xc_yuv16_sited.hip and
// w2xc_yuv16_rgb_sited.hip -- and `depth` (8 .. 16); the chroma launchers take the two sides' packings from su / du
hipError_t w2xc_launch_y16_to_plane(W2xcU16Planes src, int w, int h, int range, int depth, float *dst, long long ps, int n, hipStream_t st);
hipError_t w2xc_launch_plane_to_y16(const float *src, long long ps, int w, int h, int range, int depth, W2xcU16Planes dst, int n, hipStream_t st);
// (a turn of k_chroma2x_u16 is one tile of ALL planes of one frame -- U, or U and V: tiles x n turns, at most W2XC_CHROMA_GRID_MAX workgroups)
hipError_t w2xc_launch_chroma2x_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int ow, int oh, int depth,
                                    int cosited, int n, hipStream_t st);
hipError_t w2xc_launch_chroma_copy_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int depth, int n, hipStream_t st);
hipError_t w2xc_launch_yuv16_to_rgb(W2xcU16Planes y, W2xcU16Planes u, const unsigned short *v, int w, int h, int chroma, int range, int matrix, int depth, float *rgb,
                                    long long is, long long ps, int n, hipStream_t st);
hipError_t w2xc_launch_rgb_to_yuv16(const float *rgb, long long is, long long ps, int w, int h, int chroma, int range, int matrix, int depth, W2xcU16Planes y,
                                    W2xcU16Planes u, unsigned short *v, int n, hipStream_t st);

// ---- chroma of the sized frame calls (w2xc_yuv_sized.hip, w2xc_yuv16_sized.hip; include/w2xc_hip.h, "Sized YUV frames") ----
// The bicubic of the 2x launchers at any ratio r <= 1 per axis, in one launch from the input planes to the output planes: output sample m of an axis reads
// pos = (m + o) * r - o, with r the LUMA ratio of the axis and o = 0.5 (centred or not subsampled) or 0.25 (co-sited) -- chroma_axis, w2xc_host_geom.hpp.
// cw x ch -> ow x oh, any sizes >= 1 (reads are clamped into the plane); tiles of W2XC_CHROMA_RESIZE_TX x W2XC_CHROMA_RESIZE_TY OUTPUT samples
// (chroma_resize_tile_grid), at most W2XC_CHROMA_GRID_MAX workgroups; a turn is one plane's tile on bytes, all planes' tile of a frame on words.
#define W2XC_CHROMA_RESIZE_TX 32
#define W2XC_CHROMA_RESIZE_TY 16
hipError_t w2xc_launch_chroma_resize_u8(W2xcU8Planes su, const unsigned char *sv, int cw, int ch, W2xcU8Planes du, unsigned char *dv, int ow, int oh, double rx, double ox,
                                        double ry, double oy, int n, hipStream_t st);
hipError_t w2xc_launch_chroma_resize_u16(W2xcU16Planes su, const unsigned short *sv, int cw, int ch, W2xcU16Planes du, unsigned short *dv, int ow, int oh, int depth,
                                         double rx, double ox, double ry, double oy, int n, hipStream_t st);
