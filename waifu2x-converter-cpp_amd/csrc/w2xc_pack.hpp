// w2xc_pack.hpp -- which kernel a layer gets, and the weight image each kernel reads (w2xc_pack.cpp).  Plain C++: no HIP, nothing here touches the GPU.
// Every packer takes w as [cout][cin][3][3] (index o*cin+i, modelHandler.cpp:102); the image layouts are stated at the packers and must match the
// fragment addressing of the kernel named there (shared constants: w2xc_layout.h).  tests/cpp/pack_test.cpp checks them on the CPU.
#pragma once
#include <stddef.h>

enum W2xcKernelKind {
    W2XC_K_DIRECT = 0,   // any shape, any strides, reference summation order (VALU)
    W2XC_K_MFMA = 1,     // cin, cout in {32,64,128}; NHWC in/out; fp32 MFMA implicit GEMM
    W2XC_K_FIRST = 2,    // cin <= 3 -> cout multiple of 32: planar in, NHWC out, fp32 MFMA (K = 9*cin)
    W2XC_K_LAST = 3,     // cin multiple of 32 -> cout <= 3: NHWC in, planar out, taps-as-N fp32 MFMA
    // W2XC_PRECISION_BF16X2 / BF16X3 (and BF16 through the same pipeline): fp32 values carried as d.terms bf16 terms
    W2XC_K_MID_SPLIT = 7,      // cin, cout in {32,64,128}: term planes in, term planes (or fp32 when out_terms = 0) out
    W2XC_K_FIRST_SPLIT = 8,    // W2XC_K_FIRST storing d.out_terms term planes
    W2XC_K_LAST_GATHER = 9,    // sums the partial G planes of a fused W2XC_K_MID_SPLIT (out_terms = 9) into the output plane
    W2XC_K_FIRST2_SPLIT = 10,  // layers 1 (1 -> 32) and 2 (32 -> {32,64,128}) in one kernel; launched in layer 2's slot
    W2XC_K_FUSED_AWAY = 11,    // layer 1 when W2XC_K_FIRST2_SPLIT / W2XC_K_FIRST2_WINO4 computes it: no launch
    W2XC_K_FIRST2_WINO4 = 12,  // fp32: layers 1 (1 -> 32) and 2 (32 -> 32, Winograd F(4x4,3x3)) in one kernel (w2xc_first2_wino4.hip); launched in layer 2's slot
    // the RGB image pipeline (w2xc_process_image_rgb_u8*): never what w2xc_pick_kernel / resolve_chain answer -- run_rows puts them in place of W2XC_K_FIRST /
    // W2XC_K_LAST for the layer that touches the caller's uint8 image; both read the weight image of the kind they stand in for
    W2XC_K_FIRST_U8 = 13,      // W2XC_K_FIRST (3 -> {32,64,128}) reading an interleaved uint8 image: d.in = bytes, in_rs / in_ps / in_cs = row stride in bytes / 3 / 1
    W2XC_K_LAST_U8 = 14,       // W2XC_K_LAST ({32,64,128} -> 3) writing one: d.out = bytes, out_rs / out_ps / out_cs likewise
    // the head of an upconv model (w2xc_upconv.hip): {32,64,128,256} NHWC planes in -> {1,3} planes out at twice the size, 4x4 stride-2 transposed convolution;
    // never what w2xc_pick_kernel answers (a head is a property of the model, not of a plane count) -- pick_kind puts it in place for the head layer
    W2XC_K_UPCONV = 15,        // planar float planes out
    W2XC_K_UPCONV_U8 = 16,     // three interleaved uint8 channels out (as W2XC_K_LAST_U8), pixels 3 or 4 bytes apart
    W2XC_K_UPCONV_A_U8 = 17,   // the alpha head: channel 1 of a three-plane head alone, one uint8 per pixel (the w2xc_upconv_pack_alpha image, bias[1])
    W2XC_K_UPCONV_A = 18,      // the alpha head with the float sink: channel 1 of a three-plane head as one float plane (the alpha pass of the RGBA TTA call)
};

// Which kernel kind the fast path has for a (cin, cout) layer; W2XC_K_DIRECT when none.
W2xcKernelKind w2xc_pick_kernel(int cin, int cout);
const char *w2xc_kernel_name(W2xcKernelKind kind, int cin, int cout);

// Size in floats of the packed weight image for `kind`, and the packer.
size_t w2xc_packed_weight_floats(W2xcKernelKind kind, int cin, int cout);
void w2xc_pack_weights(W2xcKernelKind kind, int cin, int cout, const float *w, float *dst);

// conv3x3_wino (Winograd F(2x2,3x3), w2xc_wino.hip): the shapes it exists for, and its image (16 * cin * cout floats)
bool w2xc_wino_supported(int cin, int cout);
size_t w2xc_wino_packed_floats(int cin, int cout);
void w2xc_wino_pack(int cin, int cout, const float *w, float *dst);

// conv3x3_wino4 (Winograd F(4x4,3x3), w2xc_wino4.hip): its image is 36 * cin * cout floats
bool w2xc_wino4_supported(int cin, int cout);
void w2xc_wino4_pack(int cin, int cout, const float *w, float *dst);
// d.out_terms = 9: the one-plane LAST layer in conv3x3_wino4's epilogue reads the w2xc_wino4_pack_last image
size_t w2xc_wino4_pack_last_floats(int cin);
void w2xc_wino4_pack_last(int cin, const float *w, float *dst);
// PROG (the fused launch finishes the last layer itself): the shapes, its counter words, and its job grid: tile rows (16 rows each, the first one
// starting wino_py rows above the region) x groups of 8 tile columns (256 pixels)
bool w2xc_wino4_prog_supported(int cin, int cout);
size_t w2xc_wino4_prog_counters(int out_w, int out_h, int wino_py);
void w2xc_wino4_prog_jobs(int out_w, int out_h, int wino_py, int *tile_rows, int *groups);
// a batch instantiation (conv3x3_wino4_batch) exists for this layer
bool w2xc_wino4_batch_supported(int cin, int cout, bool fused_last);
// ... and the layouts of the multi-plane (RGB) chains, no fused last layer: 32 NHWC planes in (the layer behind conv3x3_first / conv3x3_wino) -> 64 / 128
// planes, planar or NHWC out; 64 / 128 planar planes in -> NHWC out (the layer in front of conv3x3_last).  Planar in and out: the predicate above.
bool w2xc_wino4_batch_layout_supported(int cin, int cout, bool in_nhwc, bool out_planar);
// conv3x3_wino_batch: the layers W2XC_KERNEL_AUTO sends to conv3x3_wino ({32, 64, 128} -> 32 planes)
bool w2xc_wino_batch_supported(int cin, int cout);

// conv3x3_first2_wino4 (w2xc_first2_wino4.hip): layer 2's image is 36 * 32 * 32 floats
bool w2xc_first2_wino4_supported(int cin1, int cout1, int cout2);
void w2xc_first2_wino4_pack(const float *w, float *dst);

// split kernels (w2xc_split.hip).  Packed weights of a mid layer: `terms` 16-bit terms of every weight in
// fragment order; W2XC_K_FIRST_SPLIT uses the W2XC_K_FIRST image.
int w2xc_split_kg(int terms, int cin);
size_t w2xc_split_packed_bytes(int cin, int cout, int terms);
float w2xc_split_pack(int cin, int cout, int terms, int fmt, const float *w, void *dst);   // returns the weight scale (1 for bf16)
// last layer fused into a two-term mid layer
int w2xc_split_halves(int terms, int cin, int cout);
size_t w2xc_split_pack_last_bytes(int cin, int terms);   // terms = 2 (one- and two-term modes) or 3
float w2xc_split_pack_last(int cin, int terms, int fmt, const float *w, void *dst);

// upconv4x4_head (w2xc_upconv.hip), the head of an upconv model: w is [cin][nout][4][4] (torch's layout of nn.SpatialFullConvolution); the image is
// 16 * nout * cin floats.  Tiles of 8 x 32 source pixels; the launch has w2xc_upconv_grid(tiles) workgroups, each walking tiles grid-stride.
bool w2xc_upconv_supported(int cin, int nout);
size_t w2xc_upconv_packed_floats(int cin, int nout);
void w2xc_upconv_pack(int cin, int nout, const float *w, float *dst);
// the alpha head's image: w2xc_upconv_pack(cin, 1, .) on channel 1 of a three-plane head, Wt[:, 1] -- 16 * cin floats; column 4 r + s of it is column
// (4 r + s) * 3 + 1 of the three-plane image
void w2xc_upconv_pack_alpha(int cin, const float *w, float *dst);
int w2xc_upconv_grid(int ntiles);
// a 3x3 layer of a head model with fewer than 32 planes on a side, zero-padded to cin_p x cout_p planes: dst[o][i][3][3] = w[o][i] for o < cout, i < cin, else 0
void w2xc_pad_layer(int cin, int cout, int cin_p, int cout_p, const float *w, float *dst);
// ... and the head's weights with zero input planes behind the model's: dst[c][nout][4][4], c < cin_p
void w2xc_pad_head(int cin, int nout, int cin_p, const float *w, float *dst);
