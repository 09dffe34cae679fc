/*
 * w2xc_hip.h -- C ABI of libw2xc_hip.so, the MI355X (gfx950) engine for the one hot path of
 * WL-Amigo/waifu2x-converter-cpp v1:
 *
 *     w2xc::convertWithModels -> Model::filter -> Model::filterWorker
 *     (/root/reference/src/convertRoutine.cpp:21-169, src/modelHandler.cpp:26-72,117-159)
 *
 * Plain pointers and sizes only: this is what a cgo/JNI/ctypes/C++ binding of the reference's
 * API for this path binds to.  include/w2xc/modelHandler.hpp and convertRoutine.hpp re-expose the
 * reference's exact C++ signatures (w2xc::Model, w2xc::modelUtility, w2xc::convertWithModels) on
 * top of these entry points; INTEGRATION.md shows the swap.
 *
 * Every function returns W2XC_OK (0) or a negative W2XC_ERR_* code; w2xc_last_error() holds a
 * message for the calling thread.  There is NO CPU fallback: if no HIP device is usable the
 * compute calls fail with W2XC_ERR_HIP.
 */
#ifndef W2XC_HIP_H_
#define W2XC_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2XC_OK               0
#define W2XC_ERR_IO          -1   /* model file could not be opened (modelHandler.cpp:175-179)      */
#define W2XC_ERR_JSON        -2   /* JSON parse / schema error       (modelHandler.cpp:181-187)      */
#define W2XC_ERR_ARG         -3   /* bad argument (null pointer, non-positive size, bad stride ...) */
#define W2XC_ERR_PLANES      -4   /* number of input planes mismatch (modelHandler.cpp:29-35)        */
#define W2XC_ERR_HIP         -5   /* HIP runtime error / no device                                   */
#define W2XC_ERR_UNSUPPORTED -6   /* kernel size != 3 (hpp:52-58 only demands square; see Q8)        */
#define W2XC_ERR_NOMEM       -7   /* an allocation failed: host, page-locked or device memory, weights included */

/* One loaded model file == the reference's std::vector<std::unique_ptr<w2xc::Model>>
 * (one w2xc::Model per conv layer, modelHandler.hpp:24-90). */
typedef struct w2xc_model w2xc_model;

#define W2XC_PRECISION_FP32 0   /* fp32 throughout on the fp32 MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2): Winograd F(4x4,3x3) for the layers
                                 * with 64 / 128 output planes (conv3x3_wino4), F(2x2,3x3) for 32 output planes (conv3x3_wino); per call
                                 * w2xc_opts.kernel = W2XC_KERNEL_MFMA selects the exact-f32 fma chains of conv3x3_mfma2 instead.
                                 * rtol 1e-4 vs the reference either way                                                       */
#define W2XC_PRECISION_BF16 1   /* w2xc_convert_* only: activations BETWEEN layers are bf16 (RNE), layers
                                 * 2..n-1 use bf16 weights on v_mfma_f32_32x32x16_bf16 with fp32
                                 * accumulate, bias and LeakyReLU; the first layer stays fp32, a one-plane
                                 * last layer is fused into layer n-1's epilogue as one more bf16 layer.
                                 * Not the reference's arithmetic: tolerance in DESIGN.md 4.          */
#define W2XC_PRECISION_BF16X2 2 /* w2xc_convert_* only: split products.  Every fp32 activation / weight of layers
                                 * 2..n-1 is carried as the sum of 2 bf16 terms (hi + lo, ~16 mantissa bits)
                                 * and each product is 3 bf16 MFMA products accumulated in fp32.          */
#define W2XC_PRECISION_BF16X3 3 /* as above with 3 terms (~24 mantissa bits) and 6 products: the error level
                                 * of an fp32 FMA chain at 2.7x the fp32 MFMA rate of CDNA4.  First / last
                                 * layer arithmetic stays fp32 MFMA in both.  Tolerances in DESIGN.md 4.   */
#define W2XC_PRECISION_FP16X2 4 /* split into 2 fp16 terms (~22 mantissa bits), 3 products on the fp16 MFMA: the
                                 * speed of BF16X2 at nearly the accuracy of BF16X3.  fp16 has 5 exponent bits:
                                 * weights are pre-scaled per layer by a power of two (exact), activations of
                                 * layers 1..n-2 saturate at +-65504 and carry 2^-25 ABSOLUTE precision below
                                 * 2^-3 -- meant for image planes in [0, 1].                   */

#define W2XC_KERNEL_AUTO    0   /* the fast kernel of each layer shape; for the fp32 layers with 32 / 64 / 128 planes in and out that is
                                 * W2XC_KERNEL_WINOGRAD4.  On a row-band view WITHOUT the wide halo below (w2xc_convert_rows_device /
                                 * w2xc_convert_plane_rows) it is REFUSED with W2XC_ERR_ARG: the kernel (and with it the rounding)
                                 * never changes silently with the view; such a caller passes the wide view or names a kernel.
                                 * No environment switches: the choice is the caller's, per call.                            */
#define W2XC_KERNEL_DIRECT  1   /* every layer: reference-ordered direct conv on VALU (bit-exact vs the oracle)             */
#define W2XC_KERNEL_MFMA    2   /* mid layers: direct implicit GEMM, a k-ordered fp32 fma chain on v_mfma_f32_32x32x2_f32
                                 * (conv3x3_mfma2) -- the closest MFMA analogue of modelHandler.cpp:134-145                */
#define W2XC_KERNEL_WINOGRAD 3  /* = W2XC_KERNEL_WINOGRAD32 (the value is kept for callers compiled against rounds 3 / 4, whose own
                                 * F(2x2) kernel on 16x16x4 tiles, conv3x3_wino16, was retired in round 5)                  */
#define W2XC_KERNEL_WINOGRAD32 4 /* mid layers: Winograd F(2x2,3x3) on v_mfma_f32_32x32x2_f32 (conv3x3_wino), fp32 throughout;
                                 * banding-invariant on minimum-halo row views; the last layer is its own launch             */
#define W2XC_KERNEL_WINOGRAD4 5 /* mid layers with >= 64 output planes: Winograd F(4x4,3x3) (conv3x3_wino4) on planar activations, fp32
                                 * throughout: 2.25 multiplies per output instead of 4, interpolation points 0, +-3/4, +-3/2 (error against the
                                 * fp64 truth 1.6-1.9x the CPU oracle's own, 0.2-0.3 of the rtol 1e-4 gate on whole frames:
                                 * tests/test_gpu_configs.py).  What W2XC_KERNEL_AUTO picks; asked for explicitly it also runs on row-band
                                 * views with the minimum halo, where its results depend on the banding at rounding level          */

typedef struct w2xc_opts {
    int      struct_size;     /* sizeof(w2xc_opts): ABI versioning                                   */
    int      precision;       /* W2XC_PRECISION_*  (opts == NULL: the process defaults, w2xc_set_default_opts)  */
    int      kernel;          /* W2XC_KERNEL_*                                                       */
    int      device;          /* device-pointer entry points: HIP device ordinal, -1 = current      */
    unsigned device_mask;     /* host-pointer entry points: bit i = use device i; 0 = all devices   */
    int      band_rows;       /* output rows per band (tile height); 0 = derive from workspace_mb   */
    int      workspace_mb;    /* activation workspace budget per device in MiB; 0 = default (16384) */
    int      profile;         /* 1 = bracket every layer launch with hipEvents (see below)          */
    int      verbose;         /* 1 = print the reference's progress lines (convertRoutine.cpp:67)   */
    int      filter_resident; /* w2xc_layer_filter: 1 = when the input planes are exactly the planes the previous
                               * w2xc_layer_filter call on this model wrote (same pointers, count, size) the caller
                               * promises they are unmodified, and the copy still on the device is used instead of
                               * uploading them again (chained Model::filter, test.cpp:72-85).  opts == NULL: the
                               * process defaults (w2xc_set_default_opts).  Default 0: every call uploads what it is given. */
    int      fusion;          /* W2XC_FUSION_*: cross-layer fusion on the fp32 path -- convertRoutine.cpp:66-76's loop collapsed by two launches:
                               * (a) the one-plane last layer inside the epilogue of the layer before it (the default kernel conv3x3_wino4
                               *     carries it; conv3x3_last_gather finishes), (b) layers 1 (1 -> 32) and 2 (32 -> 32) in one launch,
                               *     conv3x3_first2_wino4: layer 1's activations never reach HBM.  W2XC_FUSION_AUTO = both on where the
                               *     model's shapes allow (a fusion whose kernel cannot address the plane is given up, never an error),
                               *     W2XC_FUSION_OFF runs every layer as its own launch, W2XC_FUSION_FIRST / _LAST allow only (b) / only (a),
                               *     W2XC_FUSION_ON = both, and W2XC_ERR_UNSUPPORTED where AUTO would give one up.  Results stay inside the
                               *     fp32 gate either way (fused vs unfused <= 4e-6 of the output range, tests/test_gpu_winograd.py).
                               * The 16-bit modes have the same two fusions (conv3x3_first2_split, conv3x3_split + gather) under the same switch. */
    int      host_units;      /* host-pointer entry points, test aid: cut the rows into this many units, round-robin over the selected
                               * devices, so a one-GPU box runs the multi-device arithmetic; 0 = one unit per device              */
    int      host_chunk_kb;   /* host-pointer entry points, test aid: maximum size of a staged output chunk in KiB; 0 = 8192     */
    int      host_numa;       /* host-pointer entry points: 0 = a unit's feeder / drainer threads and pinned rings are placed on the CPU
                               * node its device hangs off (multi-socket hosts), 1 = the caller's affinity is left alone            */
} w2xc_opts;                  /* (verbose: bit 0 = the reference's progress lines, bit 1 = the host pipeline's phase timestamps on stderr) */

#define W2XC_FUSION_AUTO  0
#define W2XC_FUSION_OFF   1
#define W2XC_FUSION_ON    2
#define W2XC_FUSION_FIRST 3   /* only layers 1 + 2 in one launch */
#define W2XC_FUSION_LAST  4   /* only the last layer inside the epilogue of the layer before it */
/* Round 6: where the fused last layer is FINISHED.  The host-pointer entry points let the launch of layer n - 1 finish it itself, in row order
 * (conv3x3_wino4 PROG: its gather jobs write the output rows straight into page-locked host memory and flag them, so rows leave for the caller's plane
 * while the launch is still running); the device-pointer entry points follow it with a conv3x3_last_gather launch (0.2 ms faster when nothing waits
 * for rows).  Both are the same sum in the same order: BIT-identical.  For A/B runs and tests: */
#define W2XC_FUSION_GATHER_LAUNCH 5   /* as AUTO, but the gather launch in every entry point (the form of rounds 4 / 5) */
#define W2XC_FUSION_PROG          6   /* as AUTO, but finished inside the producing launch in every entry point        */

/* Fill *o with defaults (fp32, auto kernels, current device, all devices, auto banding).  Writes sizeof(w2xc_opts) bytes of THIS header's
 * struct: a binary compiled against an older, shorter w2xc_opts must call w2xc_opts_init_sized with ITS sizeof (or be rebuilt) --
 * the ABI version string (w2xc_version) changes whenever the struct grows. */
void w2xc_opts_init(w2xc_opts *o);
/* The same for a caller that knows only the first `struct_size` bytes of w2xc_opts (an older header): nothing past them is written, and
 * o->struct_size is set to it, which is what every entry point honours when it reads the options back. */
void w2xc_opts_init_sized(w2xc_opts *o, size_t struct_size);
/* What `opts == NULL` means for this process (the C++ adapter behind the reference's unmodified callers passes no options).  Initially:
 * w2xc_opts_init's defaults with precision from the environment variable W2XC_PRECISION (fp32 | fp16x2 | bf16x3 | bf16x2 | bf16) and
 * filter_resident from W2XC_FILTER_RESIDENT (0 | 1) -- the only two environment variables the library reads, once, here.  Passing a
 * struct replaces the defaults; passing NULL re-reads the environment.  Thread-safe; calls already running keep what they resolved. */
int w2xc_set_default_opts(const w2xc_opts *defaults);

/* ---- model container (modelHandler.hpp:24-90, modelHandler.cpp:74-115,170-197) ------------- */

/* == modelUtility::generateModelFromJSON (modelHandler.cpp:170-197).  The file is a JSON array of
 * {kW,kH,nInputPlane,nOutputPlane,bias[nOut],weight[nOut][nIn][kH][kW]} objects
 * (appendix/waifu2x-nocuda/export_model_nocuda.lua:12-19).  Numbers are parsed with strtod and
 * weights narrowed double->float exactly like modelHandler.cpp:95-97; biases stay double. */
int w2xc_model_load_json(const char *path, w2xc_model **out);

/* Same container from arrays: weight[l] is [nout][nin][3][3] floats (index o*nin+i, :102),
 * bias[l] is nout doubles.  Data is copied. */
int w2xc_model_from_arrays(int n_layers, const int *nin, const int *nout,
                           const float *const *weight, const double *const *bias, w2xc_model **out);

/* ---- upconv head models (revision 0.4.1.6; their batch and TTA forms: 0.4.1.6.1; their RGBA form: 0.4.1.6.2) ----
 * The upconv_7 family of later upstream versions: the model does the 2x enlargement itself, in its last layer, so nothing is enlarged in front of it.  v1
 * of the reference has no such path; the arithmetic is defined here.
 *   model:  a HEAD MODEL is n - 1 >= 1 ordinary 3x3 layers followed by one head layer: C planes in, nout in {1, 3} planes out, a 4x4 kernel, stride 2,
 *           padding 3 (a transposed convolution).  The published topology is 3 -> 16 -> 32 -> 64 -> 128 -> 128 -> 256, head 256 -> 3.
 *   head:   with z the C input planes of (H + 2) x (W + 2) pixels, output row Y in [0, 2H) and column X in [0, 2W):
 *               out[o][Y][X] = bias[o] + sum_c sum_{r, s in 0..3, (Y + 3 - r) and (X + 3 - s) even} Wt[c][o][r][s] * z[c][(Y + 3 - r) / 2][(X + 3 - s) / 2]
 *           all in fp32, the bias narrowed double -> float as elsewhere in the engine.  Exactly 2 x 2 taps per plane contribute to a pixel and all their
 *           indices lie inside z.  This is torch.nn.functional.conv_transpose2d(z, Wt, bias, stride=2, padding=3).
 *           NO activation follows the head: it is the network's linear output upstream (a deliberate departure from quirk Q1; the uint8 result is the
 *           same either way, since 0.1 x keeps the sign and saturates to 0).
 *   order:  per output pixel and plane o the sum is taken taps outer, planes inner, bias last:  v = 0;  for r ascending, for s ascending (the two r and the
 *           two s of the pixel's parity):  v += T(r, s);  v += (float)bias[o],  where T(r, s) = sum_c Wt[c][o][r][s] * z[c][..] is one fp32 MFMA accumulation
 *           chain from 0 over the planes in k-order: step (g, j), g = 0 .. C / 16 - 1, j = 0 .. 3, contracts the planes {16 g + 4 k + j, k = 0 .. 3}
 *           (v_mfma_f32_16x16x4_f32).  Every pixel of every band and of both output forms (float planes, uint8) is this one sequence: same bits.
 *   whole:  z = the valid CNN (LeakyReLU(0.1) behind every 3x3 layer) over layers 1 .. n - 1 of the source replicate-padded by n pixels -- pad = layer
 *           count, as convertRoutine.cpp:33-35 -- so n - 1 valid layers leave a one-pixel rim: z has (H + 2) x (W + 2) pixels, the result exactly 2H x 2W.
 *   JSON:   the LAST array element is the head when kW == kH == 4, dW == dH == 2, padW == padH == 3 and class_name, if present, is
 *           "nn.SpatialFullConvolution"; its weight is [nInputPlane][nOutputPlane][4][4] (torch's layout for that module), its bias may be absent and then
 *           counts as zeros (upstream builds the head with :noBias()).  Unknown keys on the 3x3 layers are ignored as before; every other non-3x3 layer, or
 *           a head anywhere but last, is refused as before (W2XC_ERR_UNSUPPORTED; a head that gives neither 1 nor 3 planes likewise).
 *   planes: on the fast path plane counts below 32 BETWEEN the layers of a head model are zero-padded to 32 when the model is built (zero weights and zero
 *           bias for the added output planes, zero weights for the added input planes of the next layer: exact zeros that add exact zeros), so that
 *           3 -> 16 -> 32 runs as conv3x3_first 3 -> 32 and a 32 -> 32 layer; w2xc_model_nin / _nout / _get_layer answer what the model declares.  The head
 *           has a kernel for C in {32, 64, 128, 256} (after padding); other counts, and the 16-bit precisions, are W2XC_ERR_UNSUPPORTED.  Models
 *           without a head are untouched.
 *   calls:  w2xc_convert_planes_up2x_device and w2xc_process_image_rgb_u8_ex[_device] (a head model as scale_model) run a head model.  EVERY other entry
 *           point given one returns W2XC_ERR_UNSUPPORTED from its argument checks, before a device is touched: the Y route, w2xc_convert_plane*,
 *           w2xc_convert_planes[_nn2x]_device, the batch, TTA and RGBA calls (w2xc_process_image_rgba_u8_ex* / _batch*), w2xc_layer_filter*;
 *           w2xc_batch_plan answers "not batched".
 *   batch:  (0.4.1.6.1) the batch and TTA forms of a head model are entry points of their own, below: w2xc_convert_planes_up2x_batch_device and
 *           w2xc_process_image_rgb_u8_up2x_batch[_device]; w2xc_batch_plan plans them with nn2x = 2.  The calls above go on refusing a head model.
 *           (0.4.1.6.2) So is the RGBA form, single image and batch in one: w2xc_process_image_rgba_u8_up2x_batch[_device], at the RGBA calls below.
 *   RGBA:   (0.4.1.6.2) image i of w2xc_process_image_rgba_u8_up2x_batch[_device] has the bytes of this composition of public calls:
 *             1. bled = w2xc_bleed_rgba_u8_device(rgba_i, P); for bleed_passes < 0, P = the sum of w2xc_model_layers of the models given (the head counts
 *                as a layer); P is clipped to max(w, h) - 1.
 *             2. colour = w2xc_process_image_rgb_u8_ex_device(noise_model, scale_model, bled, iterations, shrink_ratio, opts).
 *             3. alpha, iterations >= 1: channel 1 of w2xc_process_image_rgb_u8_ex_device(NULL, scale_model, (A, A, A), iterations, shrink_ratio, opts);
 *                iterations == 0: as in w2xc_process_image_rgba_u8_ex, the bytes as they are or the INTER_LINEAR shrink.  Alpha never sees the noise model.
 *           Where the first and the last layer have their uint8 kernels (fp32, the fast kernels, w2xc_opts.fusion other than W2XC_FUSION_OFF, no shrink)
 *           the colour pass's head writes bytes 0 .. 2 of the output pixels, layer 1 of the alpha pass reads the alpha bytes of the input pixels, and the
 *           alpha pass ends in the ALPHA HEAD: the head's channel 1 alone, on a weight image packed from Wt[:, 1] and bias[1], written to byte 3.  A
 *           column's MFMA chain does not depend on its neighbours and the tap sum is per plane, so the byte has the bits of channel 1 of the full head.
 *           Neither the grey image (A, A, A), nor a 3-channel result of either pass, nor a merge exists then.  Everywhere else the passes run around
 *           float planes and the colour stages, with the same bytes.
 * w2xc_model_add_upconv_head appends the head to a model from w2xc_model_from_arrays: weight is [nin][nout][4][4] with nin = the last 3x3 layer's output
 * planes, bias nout doubles or NULL (zeros).  It must come before the model's first use on a device and only once: otherwise W2XC_ERR_ARG.
 * w2xc_model_layers / _nin / _nout count the head as the last layer; w2xc_model_get_layer gives its weight as [nin][nout][4][4]. */
int w2xc_model_add_upconv_head(w2xc_model *m, int nout, const float *weight, const double *bias);
int w2xc_model_has_head(const w2xc_model *m);   /* 1 / 0 */

void w2xc_model_free(w2xc_model *m);
/* Release what grew with the largest plane converted so far -- activation workspaces, the host pipeline's device rows and
 * pinned rings, Model::filter's buffers -- on every device the model has run on.  Weights, streams and events stay; the
 * next call re-grows what it needs.  For a long-lived process after an unusually large image (a 16384^2 plane leaves
 * 17 GiB of workspace and 1.3 GiB of plane copies behind).  Not to be called concurrently with a conversion on `m`. */
int  w2xc_model_trim(w2xc_model *m);
int  w2xc_model_layers(const w2xc_model *m);             /* models.size()                          */
int  w2xc_model_nin(const w2xc_model *m, int layer);     /* Model::getNInputPlanes  (:18-20)        */
int  w2xc_model_nout(const w2xc_model *m, int layer);    /* Model::getNOutputPlanes (:22-24)        */
/* copy out one layer's weights ([nout][nin][3][3]) and biases; either pointer may be NULL.
 * Backs Model::printWeightMatrix / printBiases (:229-242). */
int  w2xc_model_get_layer(const w2xc_model *m, int layer, float *weight, double *bias);

/* ---- modelUtility singleton knobs (modelHandler.hpp:92-113, .cpp:199-224) ------------------- */
int  w2xc_set_jobs(int n);                    /* setNumberOfJobs: rejects n < 1 (:199-203)          */
int  w2xc_get_jobs(void);                     /* default 4 (hpp:99)                                 */
int  w2xc_set_block_size(int w, int h);       /* setBlockSize: rejects negatives (:209-213)         */
int  w2xc_set_block_size_exp2(int exp);       /* setBlockSizeExp2Square (:215-220)                  */
void w2xc_get_block_size(int *w, int *h);     /* default 512x512 (hpp:99)                           */

/* ---- the hot path --------------------------------------------------------------------------- */

/* == w2xc::convertWithModels(inputPlane, outputPlane, models, blockSplitting)
 * (convertRoutine.cpp:21-51).  `in`/`out` are HOST pointers to h rows of w floats, strides in
 * bytes (a cv::Mat ROI's step).  out(y,x) = valid-conv CNN(replicate_pad(in, n_layers))(y,x):
 * identical math per output pixel to both the unsplit path (:32-46) and the 512/498 block walk
 * (:84-169), so `block_splitting` and the singleton block size do not change results and the
 * engine bands the plane by its own workspace budget.  No clipping (Q2).  Uses every device in
 * opts->device_mask: row bands are striped over devices, one host thread per device, no
 * inter-device traffic.  opts may be NULL.
 * Host pipeline (per model and device, created once and kept): three HIP streams (H2D, layers, D2H), device copies of
 * this device's rows, and rings of pinned staging slots.  The caller's pageable planes are copied into / out of the
 * slots by modelUtility's nJob host threads (w2xc_set_jobs) while the DMA engines and the kernels run: the upload of
 * band k+1 and the download + stitch of the previous rows overlap the layers of band k; the last layer is launched in
 * ~2 MiB row chunks so its rows leave while the rest is still computed.  Planes that are already page-locked
 * (hipHostMalloc / hipHostRegister) are DMA'd in place.  The call returns when `out` is complete. */
int w2xc_convert_plane(w2xc_model *m, const float *in, size_t in_stride_bytes, int w, int h,
                       float *out, size_t out_stride_bytes, int block_splitting,
                       const w2xc_opts *opts);

/* Same contract with DEVICE pointers on device opts->device, enqueued on `hip_stream`
 * (a hipStream_t; NULL = the null stream) and NOT synchronised on return.  Input and output
 * stay resident in HBM: this is what bench.py times.  The enqueued kernels use the model's per-device
 * activation workspace, so asynchronous calls on the same (model, device) must share one stream (or be
 * serialised by the caller); different models or devices are independent. */
int w2xc_convert_plane_device(w2xc_model *m, const float *d_in, size_t in_stride_bytes, int w, int h,
                              float *d_out, size_t out_stride_bytes, void *hip_stream,
                              const w2xc_opts *opts);

/* Row-band form for sharding ONE plane over several processes / GPUs (the reference's block walk,
 * convertRoutine.cpp:114-165, made parallel): computes output rows [row_begin, row_end) of the
 * plane_h x w conversion.  `d_view` holds plane rows [view_y0, view_y0 + view_h) and must cover
 * [row_begin - n_layers, row_end + n_layers) clipped to the plane; `d_out` points at output row
 * row_begin.  Device pointers, asynchronous on `hip_stream`, no exchange between bands.
 * Bands stitch BIT-identically with the whole-plane call when the view holds the WIDE halo,
 * [row_begin - 4 n_layers, row_end + 4 n_layers) clipped: the default F(4x4) mid-layer kernel works on 4x4 blocks
 * and needs every band region to end on a block row, four rows of halo per layer.  On a view with only the minimum
 * halo W2XC_KERNEL_AUTO is refused (W2XC_ERR_ARG) -- the rounding never changes silently with the view; a named kernel
 * (W2XC_KERNEL_WINOGRAD32 / _WINOGRAD / _MFMA / _DIRECT: banding-invariant there) runs on it.                        */
int w2xc_convert_rows_device(w2xc_model *m, const float *d_view, size_t view_stride_bytes, int view_h,
                             int view_y0, int w, int plane_h, int row_begin, int row_end, float *d_out,
                             size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts);

/* Multi-plane generalisation (BASELINE.json configs[4]: a 3 -> 128 -> ... -> 3 model).  The reference
 * can only reach such a model by chaining Model::filter by hand (convertWithModels pushes one plane,
 * convertRoutine.cpp:63-64, and returns only outputPlanes[0], :78); this runs the same wrapper --
 * replicate pad by the layer count, all layers, crop -- on n_in_planes planar DEVICE planes and writes
 * ALL planes of the last layer, planar.  With one input plane and a one-plane last layer it equals
 * w2xc_convert_plane_device.  fp32 only. */
int w2xc_convert_planes_device(w2xc_model *m, int n_in_planes, const float *d_in, size_t in_plane_stride_bytes,
                               size_t in_stride_bytes, int w, int h, float *d_out, size_t out_plane_stride_bytes,
                               size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts);

/* ... with the nearest-neighbour 2x of w2xc_convert_plane_nn2x_device folded into layer 1: (w, h) is the SOURCE size, the n_in_planes input planes are
 * h rows of w floats, the output planes 2h x 2w.  Result == w2xc_convert_planes_device on the explicitly upscaled planes, bit for bit. */
int w2xc_convert_planes_nn2x_device(w2xc_model *m, int n_in_planes, const float *d_in, size_t in_plane_stride_bytes,
                                    size_t in_stride_bytes, int w, int h, float *d_out, size_t out_plane_stride_bytes,
                                    size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts);

/* N1: the scale loop of the CLI -- cv::resize(INTER_NEAREST, 2x) of the luma plane
 * (main.cpp:132-140) followed by convertWithModels (:148) -- as ONE call.  `in` is the h x w plane
 * BEFORE the resize, `out` is 2h x 2w.  The nearest-neighbour upscale is folded into layer 1's load
 * (source pixel (y>>1, x>>1)), so the 4x larger plane is never materialised nor copied over PCIe.
 * Result == w2xc_convert_plane on the explicitly upscaled plane. */
int w2xc_convert_plane_nn2x(w2xc_model *m, const float *in, size_t in_stride_bytes, int w, int h,
                            float *out, size_t out_stride_bytes, const w2xc_opts *opts);
int w2xc_convert_plane_nn2x_device(w2xc_model *m, const float *d_in, size_t in_stride_bytes, int w, int h,
                                   float *d_out, size_t out_stride_bytes, void *hip_stream,
                                   const w2xc_opts *opts);

/* An upconv head model ("upconv head models" above) on float planes: n_in_planes planar planes of w x h in, ALL planes of the head out at 2w x 2h -- the raw
 * head output, no clip (quirk Q2), no enlargement in front.  Arguments as w2xc_convert_planes_device, the output planes 2w x 2h (W2XC_ERR_ARG as
 * there; sizes at most 2^28 a side); a model without a head is W2XC_ERR_ARG.  w2xc_opts.band_rows counts SOURCE rows (a band of b source rows gives 2b output rows), memory follows
 * w2xc_opts.workspace_mb as for every call, and a banded run gives the bits of the unbanded one.  Asynchronous on hip_stream. */
int w2xc_convert_planes_up2x_device(w2xc_model *m, int n_in_planes, const float *d_in, size_t in_plane_stride_bytes,
                                    size_t in_stride_bytes, int w, int h, float *d_out, size_t out_plane_stride_bytes,
                                    size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts);

/* (0.4.1.6.1) The batch form of w2xc_convert_planes_up2x_device: n images of n_in_planes planes of w x h, image i's planes in_image_stride_bytes behind
 * image 0's, ALL planes of the head out at 2w x 2h, image i's out_image_stride_bytes behind image 0's.  Arguments as w2xc_convert_planes_batch_device
 * without nn2x; its checks too (n < 1, null pointers, bad sizes and strides, images that overlap: W2XC_ERR_ARG; a plane count the model does not take:
 * W2XC_ERR_PLANES), a model without a head is W2XC_ERR_ARG, a 16-bit precision W2XC_ERR_UNSUPPORTED; no device is touched by a refused call.  Image i is
 * BIT-identical to w2xc_convert_planes_up2x_device on image i for every option set.  A three-plane head model under the default options (fp32,
 * W2XC_KERNEL_AUTO, one band) runs ONE launch per layer for a sub-batch of as many images as w2xc_opts.workspace_mb holds -- conv3x3_first_batch,
 * conv3x3_wino_batch / conv3x3_wino4_batch[_l] (the 128 -> 256 layer among them), upconv4x4_head_batch --; everything else (a one-plane head model,
 * named kernels, images of more than one band) runs the single-image launch sequence per image.  w2xc_batch_plan(m, n_in_planes, w, h, 2, ...) answers
 * which, and the sub-batch size (a model without a head: W2XC_ERR_ARG).  Asynchronous on hip_stream. */
int w2xc_convert_planes_up2x_batch_device(w2xc_model *m, int n, int n_in_planes, const float *d_in, size_t in_image_stride_bytes,
                                          size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h, float *d_out,
                                          size_t out_image_stride_bytes, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream,
                                          const w2xc_opts *opts);

/* (0.4.1.6.1) n RGB images of one size with an upconv head model as scale_model (it must be one: otherwise W2XC_ERR_ARG; noise_model is an ordinary RGB
 * model or NULL, a head model there is W2XC_ERR_UNSUPPORTED).  Arguments, checks and the host form's overlap of sub-batches as
 * w2xc_process_image_rgb_u8_batch_tta[_device]; tta must be 0 or 1 (W2XC_ERR_ARG).
 *   tta = 0: image i has the bytes of w2xc_process_image_rgb_u8_ex[_device] on image i; a scale pass of S >= 2 images is one launch per layer where the
 *            chain has batch kernels (above), the uint8-fused first and last layers included.
 *   tta = 1: (n >= 1; n = 1 is the single-image TTA form) every pass is its TTA pass in the arithmetic of "test-time augmentation": spread at source
 *            resolution, the head model on the 8 variants -- the images of ONE head batch where w == h, else 4 + 4 --, gather at 2x.  Image i has the bytes
 *            of w2xc_u8_to_rgb_device, w2xc_tta_spread_device, w2xc_convert_planes_up2x_device on each variant, w2xc_tta_gather_device, w2xc_rgb_to_u8_device.
 * Not built: the Y route and 16-bit precisions for head models (W2XC_ERR_UNSUPPORTED / W2XC_ERR_PLANES as for the single-image call), multi-device
 * striping of the device forms.  (The RGBA form, 0.4.1.6.2: w2xc_process_image_rgba_u8_up2x_batch[_device].) */
int w2xc_process_image_rgb_u8_up2x_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                                size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                                size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                                void *hip_stream, const w2xc_opts *opts, int tta);
int w2xc_process_image_rgb_u8_up2x_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                         int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                         const w2xc_opts *opts, int tta);

/* Batches: n planes of ONE size in one call (sprite sheets, icon sets, thumbnails, dataset crops, short clips).  (w, h) is the SOURCE size, the
 * output planes are (w << nn2x) x (h << nn2x) (nn2x = 1: the nearest-neighbour 2x of w2xc_convert_plane_nn2x folded into layer 1).  out[i] is
 * BIT-identical to w2xc_convert_plane[_nn2x][_device] on in[i] with the same opts, for every option set.  With the default fp32 chain (fp32,
 * W2XC_KERNEL_AUTO, a one-plane model whose layers 1 + 2, mid layers and fused last layer run conv3x3_first2_wino4 / conv3x3_wino4 / the gather, an
 * image that fits one band) a sub-batch of images -- as many as w2xc_opts.workspace_mb holds -- is ONE launch per layer, the kernels walking the
 * items of all its images; every other case (16-bit precisions, named kernels, other fusion settings, planes larger than one band) runs the
 * single-plane launch sequence per image, with no host synchronisation in between.  n < 1, null pointers, non-positive sizes, short strides and
 * output planes that overlap each other or an input plane return W2XC_ERR_ARG, a model that does not take one plane to one plane
 * W2XC_ERR_PLANES, before any device is touched.
 * Device form: plane i starts i * *_plane_stride_bytes after d_in / d_out, on device opts->device, enqueued on `hip_stream` and NOT synchronised
 * (as w2xc_convert_plane_device: asynchronous calls on one (model, device) share one stream).
 * Host form: in[i] / out[i] are host planes; sub-batches are striped over opts->device_mask and run through the model's per-device host pipeline --
 * the upload of sub-batch k + 1, the layers of sub-batch k and the download of sub-batch k - 1 overlap; pageable planes are staged by modelUtility's
 * nJob threads through pinned slots, page-locked ones are DMA'd in place.  Returns when every out[i] is complete. */
int w2xc_convert_batch_device(w2xc_model *m, int n, int nn2x, const float *d_in, size_t in_plane_stride_bytes,
                              size_t in_stride_bytes, int w, int h, float *d_out, size_t out_plane_stride_bytes,
                              size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts);
int w2xc_convert_batch(w2xc_model *m, int n, int nn2x, const float *const *in, size_t in_stride_bytes, int w, int h,
                       float *const *out, size_t out_stride_bytes, const w2xc_opts *opts);

/* (revision 0.4.1.5) The multi-plane sibling of w2xc_convert_batch_device: n IMAGES of one size, each n_in_planes planar planes in and ALL planes of the
 * model's last layer out (w2xc_convert_planes[_nn2x]_device for n images; RGB models: 3 in, 3 out).  Image i starts i * *_image_stride_bytes after d_in /
 * d_out, its planes *_plane_stride_bytes apart, their rows *_stride_bytes apart; (w, h) is the SOURCE size, the output planes are (w << nn2x) x
 * (h << nn2x).  Image i is BIT-identical to w2xc_convert_planes[_nn2x]_device on it with the same opts, for every option set.  Where the batched chain
 * applies -- fp32, W2XC_KERNEL_AUTO, w2xc_opts.fusion other than W2XC_FUSION_PROG, an image that fits one band, and a three-plane model whose layers run
 * conv3x3_first / conv3x3_wino ({32, 64, 128} -> 32) / conv3x3_wino4 / conv3x3_last (3 -> {32, 64, 128} -> ... -> 3), or the one-plane chain of
 * w2xc_convert_batch_device -- a sub-batch of images, as many as w2xc_opts.workspace_mb holds, is ONE launch per layer; every other case runs the
 * single-image launch sequence per image, with no host synchronisation in between.  w2xc_batch_plan tells which.  Enqueued on `hip_stream`, not synchronised.
 * Errors, before any device is touched: those of w2xc_convert_batch_device and w2xc_convert_planes_device (n < 1, nn2x other than 0 / 1, null pointers,
 * sizes, row strides short or no multiple of 4, plane strides short or no multiple of 4: W2XC_ERR_ARG); image strides that are no multiple of 4, output
 * images that overlap each other or the input images: W2XC_ERR_ARG; a model whose first layer does not take n_in_planes planes: W2XC_ERR_PLANES. */
int w2xc_convert_planes_batch_device(w2xc_model *m, int n, int nn2x, int n_in_planes, const float *d_in, size_t in_image_stride_bytes,
                                     size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h, float *d_out,
                                     size_t out_image_stride_bytes, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream,
                                     const w2xc_opts *opts);
/* (revision 0.4.1.5) Pure host arithmetic, no device: how a batch of w x h images of n_in_planes planes (nn2x: converted at twice the size) runs with these
 * options -- *batched = 1 where a sub-batch is one launch per layer (the conditions above; a one-plane model is planned as w2xc_convert_batch_device
 * runs it), 0 where every image takes the single-image launch sequence; *sub_batch = images per sub-batch under w2xc_opts.workspace_mb (>= 1; 1 when
 * not batched).  The image calls on RGB models (w2xc_process_image_rgb_u8_batch*, the RGB route of the RGBA calls, TTA passes) batch their passes under
 * the same conditions.  W2XC_ERR_ARG for null pointers, nn2x other than 0 / 1 / 2 and bad sizes; the errors of the options and W2XC_ERR_PLANES as the call.
 * (0.4.1.6.1) nn2x = 2 plans w2xc_convert_planes_up2x_batch_device: an upconv head model on its w x h source (a model without a head: W2XC_ERR_ARG).  With
 * nn2x = 0 / 1 a head model is answered "not batched", (0, 1), as before: the calls those values plan refuse it. */
int w2xc_batch_plan(const w2xc_model *m, int n_in_planes, int w, int h, int nn2x, const w2xc_opts *opts, int *batched, int *sub_batch);

/* One UNIT of the tile farm from host memory (the reference's block walk, convertRoutine.cpp:114-165, made parallel across
 * processes): output rows [row_begin, row_end) of the conversion of a w x h source plane (nn2x = 1: of its nearest-
 * neighbour 2x, main.cpp:132-140, so the output plane is 2w x 2h and row numbers are in OUTPUT coordinates).
 * `in_view` points at source row view_y0 and holds view_h rows, which must cover every source row the range reads
 * (rows [row_begin - n_layers, row_end + n_layers) of the plane, halved for nn2x, clipped -- 4 n_layers instead of n_layers
 * for units that stitch bit-identically with the whole-plane call, see w2xc_convert_rows_device); `out` points at output row
 * row_begin.  Same pinned-staged, overlapped pipeline and device_mask semantics as w2xc_convert_plane; units never
 * exchange data, so N processes each calling this with their own row range ARE the multi-GPU farm (host-side gather only). */
int w2xc_convert_plane_rows(w2xc_model *m, const float *in_view, size_t in_stride_bytes, int view_y0, int view_h, int w, int h,
                            int nn2x, int row_begin, int row_end, float *out, size_t out_stride_bytes, const w2xc_opts *opts);

/* N2: the whole SCALE PHASE of the CLI for one image, device-resident:
 *   convertTo(CV_32F, 1/255) + cvtColor(COLOR_RGB2YUV) on the three channels as given  (main.cpp:75-76)
 *   `iterations` times: Y <- convertWithModels(resize(Y, 2x, INTER_NEAREST)),
 *                       U, V <- resize(2x, INTER_CUBIC)                                  (main.cpp:126-156)
 *   cvtColor(COLOR_YUV2RGB) + convertTo(CV_8U, 255)  (the only clip, Q2)                 (main.cpp:171-172)
 * `in` is h rows of w interleaved 3-channel uint8 pixels, `out` is (h << iterations) rows of (w << iterations).
 * The image stays float YUV between iterations, exactly like the reference.  The *_device form takes device
 * pointers and is asynchronous on `hip_stream`; the host form uses opts->device (default: current). */
int w2xc_scale2x_image_u8_device(w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w, int h,
                                 unsigned char *d_out, size_t out_stride_bytes, int iterations, void *hip_stream,
                                 const w2xc_opts *opts);
int w2xc_scale2x_image_u8(w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                          unsigned char *out, size_t out_stride_bytes, int iterations, const w2xc_opts *opts);
/* All three processing modes of the CLI (main.cpp:46-48, -m noise | scale | noise_scale) on one uint8 image:
 * an optional noise model is applied to Y first (main.cpp:83-98), then `iterations` 2x steps with the scale
 * model.  noise_model or scale_model may be NULL (iterations must be 0 without a scale model). */
int w2xc_process_image_u8_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in,
                                 size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_stride_bytes,
                                 int iterations, void *hip_stream, const w2xc_opts *opts);
int w2xc_process_image_u8(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes,
                          int w, int h, unsigned char *out, size_t out_stride_bytes, int iterations, const w2xc_opts *opts);
/* ... plus the final INTER_LINEAR shrink the CLI applies for scale ratios that are not powers of two
 * (main.cpp:107-114,158-167): shrink_ratio in (0,1) resizes the float YUV image to
 * int((w << iterations) * shrink_ratio) x int((h << iterations) * shrink_ratio) before the conversion back to
 * uint8; 0 = no shrink. */
int w2xc_process_image_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in,
                                    size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_stride_bytes,
                                    int iterations, double shrink_ratio, void *hip_stream, const w2xc_opts *opts);
int w2xc_process_image_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes,
                             int w, int h, unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                             const w2xc_opts *opts);
/* Batches: n uint8 images of ONE source size w x h in one call -- the batch forms of w2xc_process_image_u8_ex[_device], for the callers
 * w2xc_convert_batch names, who hold images and not luma planes.  Every image is 3-channel interleaved uint8 as in the single-image call; the
 * output images have its final size, (w << iterations) x (h << iterations), then the optional shrink.
 * out[i] is BYTE-identical to w2xc_process_image_u8_ex[_device] on in[i] with the same models, iterations, shrink_ratio and opts, for every
 * option set (precisions, named kernels, fusion settings, band_rows, workspace_mb).
 * A sub-batch of S images is ONE launch per colour / resize stage (uint8 -> YUV; the bicubic 2x of all U and V planes; the shrink of all Y, U
 * and V planes; YUV -> uint8) and one w2xc_convert_batch_device-style pass per model pass on its S luma planes: one launch per layer on the
 * default fp32 chain, the single-plane launch sequence per image otherwise.  S = as many images as w2xc_opts.workspace_mb (0 = 16384 MiB)
 * holds of the pipeline's own memory per image -- the float Y / U / V planes of every level plus the uint8 image in and out -- but no more than
 * the sub-batch the batched layer chain takes at the call's largest level (its workspace rule, see w2xc_convert_batch), and never less than 1.
 * The pipeline's memory grows with S, not with n.
 * n < 1, null pointers (a null in[i] / out[i] too), non-positive sizes, iterations outside 0..4, a shrink_ratio outside [0, 1), a shrink that
 * leaves an empty image, row strides below 3 x width, output images that overlap each other or an input image, and a model / iteration
 * combination the single-image call refuses return W2XC_ERR_ARG; a model that does not take one plane to one plane W2XC_ERR_PLANES -- all
 * before any device is touched.
 * Device form: image i starts i * *_image_stride_bytes after d_in / d_out (64-bit offsets, no alignment asked), on device opts->device;
 * enqueued on `hip_stream` and NOT synchronised (asynchronous calls that share a (model, device) share one stream).
 * Host form: in[i] / out[i] are host images; sub-batches are striped over opts->device_mask and run through the per-device host pipeline of
 * w2xc_convert_batch -- the upload of sub-batch k + 1, the launches of sub-batch k and the download of sub-batch k - 1 overlap; pageable
 * images are staged by modelUtility's nJob threads through pinned slots, page-locked ones are DMA'd in place.  Returns when every out[i] is
 * complete; without a device W2XC_ERR_HIP.  Both models' contexts are locked together for the call, as in the single-image call. */
int w2xc_process_image_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                       size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                       size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                       void *hip_stream, const w2xc_opts *opts);
int w2xc_process_image_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in,
                                size_t in_stride_bytes, int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations,
                                double shrink_ratio, const w2xc_opts *opts);
/* RGB models: the same four calls for models that take the three colour planes and return three (3 -> 32 -> ... -> 3, the form most published
 * waifu2x weights have).  v1 of the reference has no such path (its CLI converts Y only); the arithmetic is that of later upstream versions:
 *   x = u8 / 255 on the three channels AS GIVEN (no colour matrix, no channel swap);
 *   with a noise model x <- CNN(x), all three output planes; `iterations` times x <- CNN(nearest2x(x));
 *   shrink_ratio in (0,1): INTER_LINEAR on each of the three planes;   out = saturate(rint(255 x))  (the only clip).
 * Between passes the image is three float planes.  With W2XC_PRECISION_FP32 and w2xc_opts.fusion other than W2XC_FUSION_OFF the first layer of the
 * call's first pass reads the uint8 image itself and the last layer of its last pass (no shrink behind it) writes the uint8 result itself, where those
 * layers have the kernels for it (3 -> 32 / 64 / 128, 32 / 64 / 128 -> 3; not W2XC_KERNEL_DIRECT): the float copy of the source and of the result --
 * 4^iterations as many pixels -- then never exists in device memory.  Every other case runs colour kernels around float planes: the same float
 * operations in the same order, so the same bytes.
 * Arguments, argument errors (W2XC_ERR_ARG), sub-batch sizing by w2xc_opts.workspace_mb, the host forms' pipeline and the byte-identity of a batch's
 * images with the single-image call are those of w2xc_process_image_u8_ex* / _batch* above; in addition the single-image device form refuses an output
 * that overlaps the input.  noise_model / scale_model: NULL or a model whose first layer takes 3 planes and whose last layer gives 3 -- anything else,
 * a Y model beside an RGB one included, is W2XC_ERR_PLANES.  All of that before a device is touched; without a device W2XC_ERR_HIP.
 * An upconv head model as scale_model (w2xc_process_image_rgb_u8_ex[_device] only; the noise model stays a same-size RGB model): an iteration is then ONE
 * pass of the head model on the image as it is, x <- upconv(x), instead of CNN(nearest2x(x)); the shrink and the final uint8 step stay.  With fp32 and
 * fusion other than OFF layer 1 reads the uint8 image and the head writes the uint8 result; with fusion OFF the same bytes through float planes.
 * RGB chains have no batch kernels: a sub-batch runs the single-image launch sequence per image, with no host synchronisation in between (the colour
 * kernels and the shrink, where they run, are one launch per sub-batch). */
int w2xc_process_image_rgb_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w,
                                        int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                        void *hip_stream, const w2xc_opts *opts);
int w2xc_process_image_rgb_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                 unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts);
int w2xc_process_image_rgb_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                           size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                           size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                           void *hip_stream, const w2xc_opts *opts);
int w2xc_process_image_rgb_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                    int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                    const w2xc_opts *opts);
/* RGBA images: the image calls above for an image with an alpha channel.  v1 of the reference has no such path (main.cpp reads IMREAD_COLOR); like later
 * upstream versions, alpha goes through the SCALE model and the colour is first extended ("bled") under the transparent pixels, so that the CNN does not
 * pull the colour that happens to lie under alpha == 0 -- usually black -- into the visible edge.  The arithmetic is defined here:
 *   in:    h rows of w pixels of 4 interleaved bytes, rows in_stride_bytes >= 4 w apart: three colour channels in the order the 3-channel call of the route
 *          expects, alpha last.   out: (w << iterations) x (h << iterations), then the optional shrink -- the size of the 3-channel calls -- 4 bytes per
 *          pixel, rows out_stride_bytes >= 4 W apart; bytes of an output row behind 4 W are not written.
 *   route: the models choose it.  First layer takes 1 plane (and the last gives 1): the Y pipeline, w2xc_process_image_u8_ex*; 3 planes in and 3 out: the
 *          RGB pipeline, w2xc_process_image_rgb_u8_ex*; a Y model beside an RGB one, or any other plane count: W2XC_ERR_PLANES.
 *   bleed: on bytes, in integers.  mask = alpha > 0.  P times, each pass reading only the image and the mask the pass before left: a pixel with mask 0 that
 *          has n > 0 pixels with mask 1 among the in-bounds pixels of its 3x3 window becomes, per channel, (2 sum + n) / (2 n) in integer division (sum =
 *          those neighbours' bytes: their mean, half rounded up), and its mask becomes 1.  Every other pixel keeps its bytes, pixels never reached too.
 *          P = bleed_passes: < 0 = automatic -- the layer count of the noise model, if given, plus that of the scale model, if given: the CNN's reach at
 *          source resolution; 0 = off; > 0 = that many (passes beyond max(w, h) - 1 change nothing and are not run; more than 65534 that would be run:
 *          W2XC_ERR_ARG).  With no transparent pixel the bleed is the identity.
 *   colour: byte for byte what the 3-channel call of the route gives on the bled 3-channel image with the same models, iterations, shrink_ratio and opts.
 *          It is not clipped or zeroed by alpha afterwards.
 *   alpha: never sees the noise model.  iterations == 0: the alpha bytes are copied -- or, with a shrink_ratio (the output is then smaller than the
 *          input), on both routes a = (float)byte * (float)(1.0 / 255.0), the shrink's INTER_LINEAR, out = saturate(rint(255 a)).  Y route: a = (float)byte * (float)(1.0 / 255.0); per iteration
 *          a <- CNN_scale(nearest2x(a)), what w2xc_convert_plane_nn2x_device does; the shrink's INTER_LINEAR; out = saturate(rint(255 a)), half to even.
 *          Y and alpha run as ONE batch of two planes per iteration (w2xc_convert_batch_device's launches where they apply: the launch count of the
 *          3-channel call; the per-plane sequence with the same bits where not).  RGB route: channel 1 of w2xc_process_image_rgb_u8_ex_device(NULL,
 *          scale_model, ...) with the same iterations, shrink_ratio and opts on the image (A, A, A).
 * No step depends on the data: an all-255 alpha is processed like any other (callers that know their image is opaque use the 3-channel calls), and the
 * device form is asynchronous on hip_stream like the other device forms.  The host form runs on w2xc_opts.device: blocking 2-D copies around the device
 * sequence.  W2XC_ERR_ARG -- before any device is touched -- for everything the 3-channel call of the route refuses, for row strides below 4 * width
 * and for an output that overlaps the input; without a device W2XC_ERR_HIP.  The merge into 4-byte pixels is one pass of its own over the result. */
int w2xc_process_image_rgba_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w, int h,
                                         unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                         void *hip_stream, const w2xc_opts *opts);
int w2xc_process_image_rgba_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                  unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes, const w2xc_opts *opts);
/* n RGBA images of one size in ONE call (revision 0.4.1.3): what w2xc_process_image_u8_batch* is to w2xc_process_image_u8_ex*.  Nothing new is defined: the
 * route, the bleed, the colour and the alpha are the single call's, and
 * out[i] is BYTE-identical to w2xc_process_image_rgba_u8_ex[_device] on in[i] with the same models, iterations, shrink_ratio, bleed_passes and opts, for
 * every option set (precisions, named kernels, fusion settings, band_rows, workspace_mb).
 * A sub-batch of S images is ONE launch per colour stage (the bleed, alpha -> plane / grey image, the merge) and the 3-channel batch of the route around
 * them.  Y route: the Y group of a scale pass is 2 S planes, the S Y planes and their S alpha planes, one w2xc_convert_batch_device-style pass; the noise
 * pass runs on the S Y planes alone.  RGB route: the colour pass and the alpha pass are the RGB batch's, the single-image launch sequence per image.
 * iterations == 0: the alpha bytes of all S images are copied, or resized by the shrink, in one launch each.  S = as many images as
 * w2xc_opts.workspace_mb (0 = 16384 MiB) holds of the call's memory per image -- the float planes, alpha's among them, the uint8 images between the
 * stages, the 4-byte image in and out -- on the Y route at most half the sub-batch the batched layer chain takes at the call's largest level (a Y brings
 * its alpha), and never less than 1.  Memory grows with S, not with n.
 * n < 1, null pointers (a null in[i] / out[i] too), row strides below 4 x width, output images that overlap each other or an input image, and everything
 * the single RGBA call refuses return W2XC_ERR_ARG; a Y model beside an RGB one, or any other plane count, W2XC_ERR_PLANES -- all before any device is
 * touched; without a device W2XC_ERR_HIP.
 * Device form: image i starts i * *_image_stride_bytes after d_in / d_out (64-bit offsets, no alignment asked), on device opts->device; asynchronous on
 * hip_stream.  Host form: sub-batches are striped over opts->device_mask through the per-device host pipeline of w2xc_process_image_u8_batch; n = 1 is
 * the single call on the first device of the mask.  Returns when every out[i] is complete. */
int w2xc_process_image_rgba_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                            size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes, size_t out_stride_bytes,
                                            int iterations, double shrink_ratio, int bleed_passes, void *hip_stream, const w2xc_opts *opts);
int w2xc_process_image_rgba_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w, int h,
                                     unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                     const w2xc_opts *opts);
/* (0.4.1.6.2) n >= 1 RGBA images of one size with an upconv head model as scale_model: the result is defined under "upconv head models", RGBA.  n = 1 is the
 * single-image form, bands included (w2xc_opts.band_rows; a banded run gives the bytes of the unbanded one).  Arguments as
 * w2xc_process_image_rgba_u8_batch[_device]; there is no tta argument here: the TTA form is w2xc_process_image_rgba_u8_up2x_batch_tta[_device] below (0.4.1.6.3).
 * A sub-batch of S >= 2 images runs the colour pass and the alpha pass as one launch per layer each where the chain has batch kernels -- the uint8 forms
 * above included: upconv4x4_head_batch on 4-byte pixels, the alpha head's batch form, conv3x3_first_batch on the alpha bytes --, S = 1 the single-image
 * launches.  The host form overlaps sub-batches like w2xc_process_image_rgba_u8_batch.
 * Refused before a device is touched: what w2xc_process_image_rgb_u8_up2x_batch* refuses -- a scale model without a head (also with iterations == 0)
 * W2XC_ERR_ARG, a head model as noise model and the 16-bit precisions W2XC_ERR_UNSUPPORTED, a model that is not three planes in and three out
 * W2XC_ERR_PLANES -- and what the RGBA batch calls refuse, with their codes: row strides below 4 x width, n < 1, null pointers, outputs that overlap each
 * other or an input, more than 65534 effective bleed passes, an extent above 2^28.
 * Not built: the Y route, split precisions, multi-device striping of the device form, and the colour and alpha images of a sub-batch as ONE batch of
 * 2 S through the 3x3 layers (they share weights; layer 1 and the head differ). */
int w2xc_process_image_rgba_u8_up2x_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                                 size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes,
                                                 size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes, void *hip_stream,
                                                 const w2xc_opts *opts);
int w2xc_process_image_rgba_u8_up2x_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                          int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                          const w2xc_opts *opts);
/* (0.4.1.6.3) The RGBA calls under test-time augmentation (the arithmetic: "Test-time augmentation" below): the arguments of
 * w2xc_process_image_rgba_u8_batch[_device] (Y and RGB models; a head model is refused as there) and of w2xc_process_image_rgba_u8_up2x_batch[_device] (a head
 * model as scale model) and `int tta` behind them.  n >= 1; n = 1 is the single-image form, bands included.  tta = 0 is exactly the call without the argument,
 * anything but 0 and 1 W2XC_ERR_ARG.  Each refuses, with the same codes and before any device is touched, everything its sibling without tta refuses; without
 * a device W2XC_ERR_HIP.  The device forms are asynchronous on hip_stream, the host forms overlap sub-batches as their siblings do.  Image i of a batch is
 * byte-identical to the n = 1 call on image i, for every option set.
 * With tta = 1 the result is, byte for byte, this composition of calls that exist without it:
 *   bleed   unchanged: w2xc_bleed_rgba_u8_device with the same automatic pass count (TTA changes no layer count).
 *   colour  the 3-channel TTA call of the route on the bled image, same models, iterations, shrink_ratio and opts: w2xc_process_image_u8_tta_device(..., 1)
 *           for Y models, w2xc_process_image_rgb_u8_tta_device(..., 1) for RGB models, w2xc_process_image_rgb_u8_up2x_batch_device(n = 1, ..., tta = 1) for a
 *           head model as scale model.
 *   alpha   never sees the noise model, and goes through TTA only where it goes through the CNN.  iterations == 0: the bytes are copied, or linearly shrunk,
 *           as without TTA.  Y route: a = (float)byte * (float)(1.0 / 255.0); per iteration one TTA pass of the scale model with the nearest-2x fold
 *           (w2xc_convert_batch_tta_device(scale, 1, nn2x = 1, ...)); the shrink's INTER_LINEAR; saturate(rint(255 a)).  RGB route: channel 1 of the
 *           scale-only 3-channel TTA call on the image (A, A, A); head route: the same through the up2x TTA call.
 * How it runs.  Y route: alpha rides with Y -- the scale pass's variants are 16 S planes in one batch where w == h, two of 8 S otherwise; the noise pass runs
 * on the S Y planes alone.  RGB and head routes, w2xc_opts.fusion other than W2XC_FUSION_OFF: the first spread of the colour sequence reads the bled uint8
 * image and that of the alpha sequence the caller's alpha bytes (w2xc_tta_spread_u8_device's kernel: no float copy of the source, no grey image), and where the
 * last pass is a scale pass with no shrink behind it the colour gather writes bytes 0 .. 2 and the alpha gather byte 3 of the caller's pixels
 * (w2xc_tta_gather_u8_device's kernel: no final float planes, no intermediate uint8 results, no merge launch).  These ends do not depend on precision or kernel
 * choice.  On the head route the last alpha pass runs the one-plane alpha head with its float sink (the bits of channel 1 of the full head), so its gather
 * reads 8 planes per image instead of 24; for RGB models without a head it runs the full chain and the gather selects channel 1.  Every other case --
 * W2XC_FUSION_OFF, a shrink, iterations == 0, the levels between two passes -- runs the stages of the calls above around float planes.  The variant planes of
 * the larger of the two sequences count into the per-image bytes that size a sub-batch under w2xc_opts.workspace_mb.
 * Not built: fused uint8 ends for the opaque TTA calls and for the Y route, a one-plane last layer for RGB models without a head, colour and alpha as one
 * batch of 2 S through the 3x3 layers, 16-bit precisions for head models, multi-device striping of the device forms. */
int w2xc_process_image_rgba_u8_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                                size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes,
                                                size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes, void *hip_stream,
                                                const w2xc_opts *opts, int tta);
int w2xc_process_image_rgba_u8_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                         int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                         const w2xc_opts *opts, int tta);
int w2xc_process_image_rgba_u8_up2x_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                                     size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                                     size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                                     int bleed_passes, void *hip_stream, const w2xc_opts *opts, int tta);
int w2xc_process_image_rgba_u8_up2x_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                              int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                              int bleed_passes, const w2xc_opts *opts, int tta);
/* Test-time augmentation (TTA): every CNN pass runs on the 8 flips and transposes of its input, each result is transformed back and the 8 are averaged --
 * the quality option later upstream versions of the converter have as --tta (v1 of the reference has none); 8x the CNN work.  The arithmetic is defined here:
 *   T_k, k = 0..7, on a plane x of h rows x w columns applies, in this order: the horizontal flip (x[:, ::-1]) if k & 1, the vertical flip (x[::-1, :]) if
 *          k & 2, the transpose if k & 4.  T_k^-1 undoes them in the reverse order.  Variants 0..3 are h x w ("upright"), variants 4..7 are w x h ("transposed").
 *   One TTA pass of a model, plane-wise for a model of several planes:
 *          v_k = T_k^-1( CNN( T_k(x) ) ),  k = 0..7
 *          out = (((((((v_0 + v_1) + v_2) + v_3) + v_4) + v_5) + v_6) + v_7) * 0.125f
 *          in fp32, in exactly this order, nothing contracted.  CNN = what the call without TTA runs with the same options: w2xc_convert_plane[_nn2x]_device for
 *          a one-plane model (the variants of one size go through w2xc_convert_batch_device's launches -- one batch of 8 n planes where w == h, two of 4 n
 *          otherwise -- whose planes are bit-identical to the single call), w2xc_convert_planes[_nn2x]_device for a model of several planes (the single-image
 *          launch sequence per variant).  Nearest-2x commutes with every T_k: a scale pass transforms the SOURCE, runs with the 2x folded into layer 1 as
 *          always and transforms back at 2x; the 2x float source never exists.
 *   Image calls: TTA replaces every CNN pass of the route by its TTA pass -- the noise pass and every scale iteration; Y on the Y route, all three planes on the
 *          RGB route.  Everything else is the call without TTA: the colour conversion, the bicubic U / V, the shrink, the final rounding; the image stays float
 *          between passes.  On the RGB route the first / last layer does NOT read / write the uint8 image itself under TTA (the mean is taken before the
 *          rounding): the colour kernels run around float planes.
 * Memory: the variant planes of the largest pass -- 8 planes at its input level, 8 at its output level per plane that goes through the CNN -- live with the
 * image planes in the model's context (released by w2xc_model_trim, filled by w2xc_debug_fill_scratch), count into the per-image bytes that size a sub-batch
 * under w2xc_opts.workspace_mb, and are reused by every pass.
 *
 * Plane calls.  w2xc_convert_batch_tta_device: one TTA pass on each of n planes, the arguments and errors of w2xc_convert_batch_device (one plane in, one plane
 * out).  w2xc_convert_planes_tta_device: one TTA pass of a model of n_in_planes planes, the arguments and errors of w2xc_convert_planes_device (nn2x = 0) /
 * w2xc_convert_planes_nn2x_device (nn2x = 1); nn2x outside {0, 1} and a plane count the model does not take are refused before a device is touched.  Both are
 * asynchronous on hip_stream, on device opts->device. */
int w2xc_convert_batch_tta_device(w2xc_model *m, int n, int nn2x, const float *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h,
                                  float *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts);
int w2xc_convert_planes_tta_device(w2xc_model *m, int n_in_planes, int nn2x, const float *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w,
                                   int h, float *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts);
/* Image calls: each takes the arguments of the call it is named after -- w2xc_process_image_u8_ex[_device], w2xc_process_image_u8_batch[_device] and their
 * rgb forms -- and `int tta` behind them: 0 = exactly that call, 1 = TTA, anything else W2XC_ERR_ARG.  Argument and model errors are those of that call (on the
 * Y route a model that does not take one plane to one plane is W2XC_ERR_PLANES already here), before a device is touched; without a device W2XC_ERR_HIP.  The
 * device forms are asynchronous.  A batch's images are byte-identical to the single-image TTA call.  The TTA forms of the RGBA calls (0.4.1.6.3) are
 * w2xc_process_image_rgba_u8_batch_tta[_device] and w2xc_process_image_rgba_u8_up2x_batch_tta[_device], above. */
int w2xc_process_image_u8_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w, int h,
                                     unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio, void *hip_stream,
                                     const w2xc_opts *opts, int tta);
int w2xc_process_image_u8_tta(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                              unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts, int tta);
int w2xc_process_image_u8_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                           size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes,
                                           size_t out_stride_bytes, int iterations, double shrink_ratio, void *hip_stream, const w2xc_opts *opts, int tta);
int w2xc_process_image_u8_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                    int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts,
                                    int tta);
int w2xc_process_image_rgb_u8_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w, int h,
                                         unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio, void *hip_stream,
                                         const w2xc_opts *opts, int tta);
int w2xc_process_image_rgb_u8_tta(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                  unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts, int tta);
int w2xc_process_image_rgb_u8_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                               size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                               size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                               void *hip_stream, const w2xc_opts *opts, int tta);
int w2xc_process_image_rgb_u8_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                        int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                        const w2xc_opts *opts, int tta);
/* TTA's building blocks, without a model, on the current device, asynchronous on hip_stream.  Variant planes have contiguous rows (w floats upright, h floats
 * transposed) and lie variant_plane_stride_bytes >= 4 w h apart: T_k of plane i at d_up + (k n + i) strides for k = 0..3, at d_tr + ((k - 4) n + i) strides for
 * k = 4..7 -- two groups of 4 n planes that must not overlap each other or the n planes on the other side.
 * spread: n source planes of w x h (rows src_stride_bytes apart, planes src_plane_stride_bytes apart) -> their 8 n variants.
 * gather: 8 n result planes in that layout, the upright ones w x h -> n planes of w x h: the sum above.  Bytes of a row behind 4 w are not written. */
int w2xc_tta_spread_device(const float *d_src, int n, size_t src_plane_stride_bytes, size_t src_stride_bytes, int w, int h, float *d_up, float *d_tr,
                           size_t variant_plane_stride_bytes, void *hip_stream);
int w2xc_tta_gather_device(const float *d_up, const float *d_tr, size_t variant_plane_stride_bytes, int n, int w, int h, float *d_dst,
                           size_t dst_plane_stride_bytes, size_t dst_stride_bytes, void *hip_stream);
/* (0.4.1.6.3) The two blocks with an interleaved uint8 image at their outer side -- what the RGBA TTA calls run on their RGB and head routes.
 * spread_u8: n images of w x h (pixels px_bytes = 3 or 4 bytes, rows stride_bytes >= px_bytes w apart, images image_stride_bytes apart) -> the 8 variants of
 *   their 3 n planes, in exactly the layout and with exactly the floats of w2xc_u8_to_rgb_device followed by w2xc_tta_spread_device with 3 n planes: source
 *   plane 3 i + c, c = 0 .. 2, is (float)byte * (float)(1.0 / 255.0) of byte ch0 + c * ch_step of each pixel of image i.  (ch0, ch_step) = (0, 1): the colour
 *   of RGB or RGBA pixels; (3, 0) with 4-byte pixels: the grey image (A, A, A) without building it.
 * gather_u8: 8 m result planes in the gather's layout, m = planes_per_image * n, the upright ones w x h -> for image i and c in [0, n_ch), byte byte0 + c of
 *   each px_bytes-wide pixel = saturate(rint(255 x)) (half to even, as w2xc_rgb_to_u8_device) of w2xc_tta_gather_device's sum x for plane
 *   planes_per_image * i + first_plane + c.  Bytes not named are not written -- byte stores, no pixel is read --, nor are bytes of a row behind px_bytes * w: two
 *   gathers into different bytes of the same pixels may be in flight in either order.  (3, 0, 3) into bytes 0 .. 2: colour; (3, 1, 1) or (1, 0, 1) into byte 3: alpha.
 * W2XC_ERR_ARG before a device is touched: null pointers, n < 1, sizes < 1, strides below a row (an image stride below an image where n > 1), a variant plane
 * stride below 4 w h or no multiple of 4, px_bytes outside {3, 4}, a selected byte outside the pixel (ch0, ch_step < 0 or ch0 + 2 ch_step >= px_bytes; byte0 < 0,
 * n_ch < 1 or byte0 + n_ch > px_bytes), selected planes outside the image (first_plane < 0 or first_plane + n_ch > planes_per_image), variant groups that overlap
 * each other, the source or the destination. */
int w2xc_tta_spread_u8_device(const unsigned char *d_src, int n, size_t image_stride_bytes, size_t stride_bytes, int px_bytes, int ch0, int ch_step, int w, int h,
                              float *d_up, float *d_tr, size_t variant_plane_stride_bytes, void *hip_stream);
int w2xc_tta_gather_u8_device(const float *d_up, const float *d_tr, size_t variant_plane_stride_bytes, int n, int planes_per_image, int first_plane, int n_ch,
                              int w, int h, unsigned char *d_dst, size_t image_stride_bytes, size_t stride_bytes, int px_bytes, int byte0, void *hip_stream);

/* ---- YUV frames (revision 0.4.1.7) ----------------------------------------------------------------
 * Frames that are Y, U and V already -- what a video decoder, a y4m / raw-yuv pipeline or a grey scan holds -- through Y models: luma through the CNN, chroma
 * enlarged on bytes (the reference's pipeline, SURVEY Q9, without the RGB image it starts from).  NO colour matrix is involved anywhere: Y is the frame's
 * own luma, not OpenCV's full-range BT.601 Y of an RGB image.  v1 of the reference has no such entry point; the arithmetic is defined here.
 *   frame:   a luma plane of w x h bytes and, by `chroma`, two chroma planes of cw x ch bytes:
 *              W2XC_YUV_420: cw = (w + 1) / 2, ch = (h + 1) / 2      W2XC_YUV_422: cw = (w + 1) / 2, ch = h
 *              W2XC_YUV_444: cw = w, ch = h                          W2XC_YUV_400: no chroma, the chroma pointers are ignored
 *            n frames are one w2xc_yuv_planes per side: frame i's luma at y + i * y_frame_stride, rows y_stride bytes apart; its chroma at u / v +
 *            i * c_frame_stride, rows c_stride apart, samples c_px bytes apart -- 1: planar; 2: two interleaved planes, NV12 is v = u + 1 (NV21: u = v + 1).
 *            A row of luma is w bytes, a row of chroma c_px * (cw - 1) + 1 bytes from its plane's pointer.
 *   luma in: (float)Y the byte as a float.  W2XC_RANGE_FULL: y = (float)Y * (float)(1.0 / 255.0); W2XC_RANGE_LIMITED: y = ((float)Y - 16.0f) * (float)(1.0 / 219.0).
 *   models:  with a noise model y <- CNN_noise(y); then, `iterations` (0 or 1) times, y <- CNN_scale(nearest2x(y)) -- exactly the passes
 *            w2xc_convert_batch_device runs with nn2x = 0 / 1 on the luma planes of a sub-batch: one launch per layer on the default chain, and bands,
 *            precisions, named kernels and fusion settings as there.
 *   luma out: full range saturate(rint(255 y)), half to even, as w2xc_rgb_to_u8_device; limited range saturate(rint(y * 219.0f + 16.0f)), the product and the sum
 *            two fp32 operations.
 *   chroma:  iterations = 1: c = (float)C * (float)(1.0 / 255.0), the 2x enlargement of w2xc_resize2x_cubic_device -- its taps, clamping, coefficient
 *            expressions and summation order --, saturate(rint(255 c)).  The output plane is the leading (2 w + 1) / 2 x (2 h + 1) / 2 samples of the 2 cw x 2 ch
 *            enlargement (4:2:2: (2 w + 1) / 2 x 2 h; 4:4:4: all of it): the chroma size of a frame of 2 w x 2 h.  `range` does not touch chroma.
 *            iterations = 0: the chroma bytes are copied.
 *            The enlargement treats a chroma sample as CENTRED on its block of luma samples (JPEG / MPEG-1 siting); left-sited chroma (MPEG-2, H.264 and
 *            later: the sample sits on the block's left column) is not corrected, and comes out a quarter of an output chroma sample to the right.
 *   refused, before a device is touched: a model that is not one plane to one plane W2XC_ERR_PLANES; an upconv head model W2XC_ERR_UNSUPPORTED; neither model
 *            given, iterations outside 0 .. 1, iterations = 1 without a scale model, iterations = 0 without a noise model, n < 1, null pointers (the chroma
 *            pointers too, unless W2XC_YUV_400), non-positive sizes or more than 2^22 a side, row strides below the row's bytes, frame strides below a plane
 *            where n > 1, c_px not 1 or 2, an unknown chroma / range, output planes that overlap each other or an input plane: W2XC_ERR_ARG.
 * Device form: device pointers on device opts->device, enqueued on hip_stream and NOT synchronised (asynchronous calls that share a (model, device) share one
 * stream).  Frames run in sub-batches of S: as many as w2xc_opts.workspace_mb (0 = 16384 MiB) holds of the pipeline's own memory per frame -- two float luma
 * planes per level, and the frame's bytes in and out -- but no more than the sub-batch the batched layer chain takes at the call's largest level, and never
 * less than 1.  A sub-batch is one launch of each luma stage, the passes on its S luma planes, and ONE launch of the chroma kernel for its 2 S chroma
 * planes (bytes in, bytes out: no float plane of chroma exists).  The float planes live in the model's context.
 * Host form: the same with host planes; per sub-batch the planes are uploaded, the device sequence runs and the result is downloaded, on the first device of
 * opts->device_mask, with blocking copies around it; returns when every output plane is complete.  Host planes with c_px = 2 must be the two interleaved
 * planes of one buffer, v = u + 1 (NV12) or u = v + 1 (NV21): anything else is W2XC_ERR_ARG here.  Without a device W2XC_ERR_HIP.
 * Left out: RGB and head models on YUV frames (they need a colour matrix chosen by the caller), 10 / 16-bit samples, TTA, more than one 2x step, the shrink,
 * chroma siting correction, a submit / wait pair that overlaps frames across calls, overlapped host sub-batches, multi-device striping.
 * (Samples of 9 to 16 bits in 16-bit words now live in w2xc_process_frames_yuv_u16*: "16-bit YUV frames" below.)
 * (An output size, several 2x steps and the shrink now live in the _sized forms of these calls: "Sized YUV frames" below.) */
#define W2XC_YUV_420 0
#define W2XC_YUV_422 1
#define W2XC_YUV_444 2
#define W2XC_YUV_400 3
#define W2XC_RANGE_FULL    0
#define W2XC_RANGE_LIMITED 1
typedef struct w2xc_yuv_planes {   /* one side of a call: n frames */
    unsigned char *y;  size_t y_stride,  y_frame_stride;     /* bytes */
    unsigned char *u, *v; size_t c_stride, c_frame_stride;    /* bytes; NV12: v = u + 1, c_px = 2 */
    int c_px;
} w2xc_yuv_planes;
int w2xc_process_frames_yuv_u8_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range,
                                      const w2xc_yuv_planes *d_in, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u8(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *in,
                               const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts);
/* Its building blocks, without a model, on the current device, asynchronous on hip_stream; n planes each, plane i frame_stride_bytes / plane_stride_bytes on.
 * y8_to_plane: "luma in" on n byte planes of w x h (rows stride_bytes apart) -> n float planes with contiguous rows, plane_stride_bytes (a multiple of 4,
 *   at least 4 w h) apart.   plane_to_y8: "luma out", the other way.  Bytes of a row behind w are not written.
 * chroma2x_u8: "chroma" with iterations = 1 on n byte planes of cw x ch samples, src_px bytes apart -> the leading ow x oh samples (1 <= ow <= 2 cw, 1 <= oh <=
 *   2 ch) of their enlargements, dst_px bytes apart.  Only the bytes of those samples are written, each with a byte store: with dst_px = 2 the bytes between them
 *   are another plane's, and two calls may fill the two planes in either order.
 * W2XC_ERR_ARG: null pointers, n < 1, sizes below 1 or above 2^22, strides below a row (a frame / plane stride below a plane where n > 1), an unknown range,
 * src_px / dst_px not 1 or 2, an output size outside the enlargement, source and destination that overlap. */
int w2xc_y8_to_plane_device(const unsigned char *d_src, int n, size_t frame_stride_bytes, size_t stride_bytes, int w, int h, int range, float *d_dst,
                            size_t plane_stride_bytes, void *hip_stream);
int w2xc_plane_to_y8_device(const float *d_src, int n, size_t plane_stride_bytes, int w, int h, int range, unsigned char *d_dst, size_t frame_stride_bytes,
                            size_t stride_bytes, void *hip_stream);
int w2xc_chroma2x_u8_device(const unsigned char *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int cw, int ch,
                            unsigned char *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int ow, int oh, void *hip_stream);

/* ---- YUV frames through RGB models (revision 0.4.1.8) ---------------------------------------------
 * The frames of the section above through the models that take R, G and B: three-plane models (3 -> ... -> 3, the form most published weights have) and upconv
 * head models.  The caller names the colour matrix; the call converts the frames' bytes to three float planes per frame, runs the passes of
 * w2xc_process_image_rgb_u8* on them and converts back -- one colour matrix each way and one rounding to bytes, where the route over an RGB byte image has two
 * of each.  w2xc_process_frames_yuv_u8* itself goes on refusing these models.  v1 of the reference has no such entry point; the arithmetic is defined here.
 * Every kernel file involved is built with -ffp-contract=off: every expression below is a sequence of single fp32 operations in the order written.
 *   constants: computed in double from the two luma weights of `matrix`, then rounded ONCE to float:
 *              W2XC_MATRIX_BT601: Kr = 0.299, Kb = 0.114    W2XC_MATRIX_BT709: Kr = 0.2126, Kb = 0.0722    W2XC_MATRIX_BT2020 (non-constant luminance): Kr = 0.2627,
 *              Kb = 0.0593;   Kg = 1.0 - Kr - Kb;   cRV = 2.0 * (1.0 - Kr);   cBU = 2.0 * (1.0 - Kb);   cGV = Kr * cRV / Kg;   cGU = Kb * cBU / Kg;
 *              iRV = 1.0 / cRV;   iBU = 1.0 / cBU.
 *   frame:     w2xc_yuv_planes, c_px 1 or 2, NV12 and NV21, the chroma sizes (w + 1) / 2 and so on and W2XC_YUV_420 / _422 / _444 as above.  W2XC_YUV_400 is
 *              W2XC_ERR_ARG here: a grey frame belongs to the Y call.
 *   samples in: luma as above: y = (float)Y * (float)(1.0 / 255.0), or ((float)Y - 16.0f) * (float)(1.0 / 219.0) for W2XC_RANGE_LIMITED.  Chroma: cb = (u - 128.0f) * k
 *              and cr = (v - 128.0f) * k with k = (float)(1.0 / 255.0) for full and (float)(1.0 / 224.0) for limited range, u and v the chroma AT THE LUMA SAMPLE:
 *   chroma at luma resolution: a chroma sample is CENTRED on its block of luma samples, the siting the chroma kernel above assumes (left-sited chroma stays
 *              uncorrected).  Along a subsampled axis luma index x reads the chroma samples j = x >> 1 and j' = (x odd ? j + 1 : j - 1), clamped into the plane,
 *              and the value is 0.75f * C[j] + 0.25f * C[j'] on the bytes as floats -- horizontally first, then vertically on the two row results; along an axis
 *              that is not subsampled the sample is read as it is.  The - 128 and the scale come after this.  On bytes every one of these operations is exact in
 *              fp32 (multiples of 1 / 4, then of 1 / 16, below 256): the order is a convention, not a rounding choice.
 *   to RGB:    R = y + cRV * cr;   B = y + cBU * cb;   G = (y - cGU * cb) - cGV * cr;   each clamped to [0, 1], the models' domain (and what the byte image of
 *              the old route did).  Three float planes R, G, B per frame.
 *   passes:    those of w2xc_process_image_rgb_u8* between its two ends: with a noise model x <- CNN_noise(x); then `iterations` (0 or 1) times x <-
 *              CNN_scale(nearest2x(x)) with the 2x folded into layer 1 -- or, for an upconv head model, the model's own 2x.  The planes between and after the
 *              passes are unclipped.
 *   from RGB:  (W x H planes, unclipped)  y' = (Kr * R + Kg * G) + Kb * B;   cb = (B - y') * iBU;   cr = (R - y') * iRV.
 *              Luma byte: saturate(rint(255 y')), or saturate(rint(y' * 219.0f + 16.0f)) for limited range; half to even.
 *              Chroma of a subsampled layout is the box mean over the luma block before the rounding: ((a + b) + (c + d)) * 0.25f for 4:2:0 (a, b the upper row
 *              from left to right, c, d the lower), (a + b) * 0.5f for 4:2:2; a block cut by an odd edge replicates its last column / row.
 *              Chroma byte: saturate(rint(c * 255.0f + 128.0f)), or saturate(rint(c * 224.0f + 128.0f)) for limited range.
 *   refused, before a device is touched: a model that is not three planes to three planes W2XC_ERR_PLANES; a head model as noise model, and the options
 *              w2xc_convert_planes[_up2x]_batch_device refuse (an unknown precision; any 16-bit precision with a head model): W2XC_ERR_UNSUPPORTED; everything the
 *              Y call refuses as W2XC_ERR_ARG, an unknown `matrix` and W2XC_YUV_400: W2XC_ERR_ARG.
 * The frame call is DEFINED as this route, by bytes, for every option set the route accepts: w2xc_yuv8_to_rgb_device -> w2xc_convert_planes_batch_device with
 * nn2x = 0 (the noise pass) -> w2xc_convert_planes_batch_device with nn2x = 1, or w2xc_convert_planes_up2x_batch_device for a head model (the scale pass) ->
 * w2xc_rgb_to_yuv8_device.  Device form, host form and the sub-batch rule as above; the pipeline's own memory per frame is three float planes per level (the
 * noise pass's output included) and the frame's bytes in and out.  A sub-batch is ONE launch of each end and the passes between: S >= 2 frames one launch per
 * layer where the chain has batch kernels, one frame the single-image sequence, bands included.
 * Left out: left-sited chroma, 10 / 16-bit samples, TTA, the shrink, more than one 2x step, uint8-fused first and last layers (the float RGB planes exist in
 * memory), multi-device striping, overlapped host sub-batches, a submit / wait pair.
 * (Samples of 9 to 16 bits in 16-bit words now live in w2xc_process_frames_yuv_u16_rgb*: "16-bit YUV frames" below.)
 * (An output size, several 2x steps and the shrink now live in the _sized forms of these calls: "Sized YUV frames" below.) */
#define W2XC_MATRIX_BT601  0
#define W2XC_MATRIX_BT709  1
#define W2XC_MATRIX_BT2020 2
int w2xc_process_frames_yuv_u8_rgb_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                          const w2xc_yuv_planes *d_in, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u8_rgb(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                   const w2xc_yuv_planes *in, const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts);
/* Its two ends, without a model, on the current device, asynchronous on hip_stream.  Frame i's planes R, G, B have contiguous rows of w floats and lie at d_rgb +
 * i * image_stride_bytes + {0, 1, 2} * plane_stride_bytes.
 * yuv8_to_rgb: "samples in", "chroma at luma resolution" and "to RGB" on n frames -> their 3 n float planes.
 * rgb_to_yuv8: "from RGB" on 3 n float planes of w x h -> n frames.  Only the frames' own samples are written: with c_px = 2 and u, v that do not interleave,
 *   the bytes between a plane's samples are left as they are.
 * W2XC_ERR_ARG: null pointers, n < 1, sizes below 1 or above 2^22, what the frame call refuses of a w2xc_yuv_planes, strides that are no multiples of 4 / a plane
 * stride below a plane / an image stride below three planes where n > 1, an unknown chroma / range / matrix, W2XC_YUV_400, written planes that overlap each other
 * or a plane that is read. */
int w2xc_yuv8_to_rgb_device(const w2xc_yuv_planes *d_src, int n, int w, int h, int chroma, int range, int matrix, float *d_rgb, size_t image_stride_bytes,
                            size_t plane_stride_bytes, void *hip_stream);
int w2xc_rgb_to_yuv8_device(const float *d_rgb, size_t image_stride_bytes, size_t plane_stride_bytes, int n, int w, int h, int chroma, int range, int matrix,
                            const w2xc_yuv_planes *d_dst, void *hip_stream);

/* ---- 16-bit YUV frames (revision 0.4.1.9) -----------------------------------------------------------
 * The frames of the two sections above with samples of 8 to 16 bits in 16-bit little-endian words: what yuv420p10le / y4m C420p10 files and the P010 / P012 /
 * P016 surfaces of hardware decoders hold.  Only the two ends differ: the float pipeline between them is the one of the 8-bit calls.  v1 of the reference has
 * no such entry point; the arithmetic is defined here.  Every kernel file involved is built with -ffp-contract=off: every expression below is a sequence of
 * single fp32 operations in the order written; every constant is computed in double and rounded ONCE to float.
 *   sample:   a word holding a value of `depth` bits, 8 <= depth <= 16.  D = depth, s = 2^(D - 8), M = 2^D - 1.
 *              W2XC_PACK_LOW  (0): the value in the low bits (yuv420p10le, y4m C420p10).  Read: word & M.  Write: the value, the high bits zero.
 *              W2XC_PACK_HIGH (1): the value in the high bits (P010, P012, P016).  Read: word >> (16 - D), the low bits are ignored.  Write: value << (16 - D),
 *              the low bits zero.  At D = 16 the two are the same.
 *   frame:    w2xc_yuv16_planes is w2xc_yuv_planes with unsigned short pointers -- 2-byte aligned; strides in BYTES and even; c_px counts SAMPLES: 1 planar, 2
 *              interleaved, P010 is v = u + 1 (one sample on) -- and one more field, `pack`: the two sides of a call may differ in packing as they may in c_px.
 *              `depth` is an argument of the call, the same on both sides.  Chroma sizes and W2XC_YUV_420 / _422 / _444 / _400 as for the 8-bit calls.
 *   Everything is the 8-bit definition with 255 -> M, 16 -> 16 s, 219 -> 219 s, 224 -> 224 s, 128 -> 128 s:
 *   luma in:  W2XC_RANGE_FULL: y = (float)Y * (float)(1.0 / M);  W2XC_RANGE_LIMITED: y = ((float)Y - 16 s) * (float)(1.0 / (219 s)).
 *   luma out: full range clamp(rint(y * M), 0, M), half to even; limited range clamp(rint(y * (219 s) + 16 s), 0, M), the product and the sum two operations.  The
 *              clamp holds past the int32 range.
 *   chroma, Y route (iterations = 1): c = (float)C * (float)(1.0 / M), the 2x enlargement of w2xc_resize2x_cubic_device -- its taps, clamping, coefficient
 *              expressions and summation order --, clamp(rint(c * M), 0, M), cropped to the chroma size of a 2 w x 2 h frame.  iterations = 0: the values are
 *              copied, repacked where the two sides differ in `pack`.
 *   RGB route, in: chroma at luma resolution is 0.75f * C[j] + 0.25f * C[j'] with j, j', the clamping and the horizontal-then-vertical order of "YUV frames
 *              through RGB models"; the values are multiples of 1 / 16 below 2^16 (20 bits), so the arithmetic is still exact in fp32 and the order a convention.
 *              cb = (u - 128 s) * k and cr = (v - 128 s) * k with k = (float)(1.0 / M) for full and (float)(1.0 / (224 s)) for limited range.  The matrix
 *              constants, R, G, B and the clamp to [0, 1] as there.
 *   RGB route, out: y', cb, cr and the box mean over the luma block as there.  Luma word: "luma out" above.  Chroma word: clamp(rint(c * M + 128 s), 0, M) for
 *              full range, clamp(rint(c * (224 s) + 128 s), 0, M) for limited range.
 *   With D = 8 every constant is the 8-bit call's constant ((float)(1.0 / (219 * 1)) is (float)(1.0 / 219.0)): a frame of bytes widened to low-packed words
 *   gives, word for byte, the 8-bit call's output.  For every D every value 0 .. M returns unchanged through luma in -> luma out, and through the chroma scale and
 *   offset of the RGB route, in both ranges (tests/test_yuv16_api.py).
 * w2xc_process_frames_yuv_u16[_device]: Y models, W2XC_YUV_400 included, iterations 0 or 1 -- DEFINED, by words, as w2xc_y16_to_plane_device ->
 *   w2xc_convert_batch_device (nn2x = 0, then 1) -> w2xc_plane_to_y16_device, and w2xc_chroma2x_u16_device per chroma plane.
 * w2xc_process_frames_yuv_u16_rgb[_device]: three-plane models, or an upconv head model as scale model, by `matrix` -- DEFINED as w2xc_yuv16_to_rgb_device ->
 *   w2xc_convert_planes_batch_device / w2xc_convert_planes_up2x_batch_device -> w2xc_rgb_to_yuv16_device.
 * Sub-batches, bands at S = 1, precisions, named kernels, fusion settings, the device and the host form are those of the 8-bit calls, with two bytes per sample
 * in the per-frame memory; a sub-batch of S frames is one launch of each end and the passes between.  Host planes with c_px = 2 must be the two planes of one
 * buffer, v = u +- 1 sample.
 * Refused, before a device is touched: everything the corresponding 8-bit call refuses, with its code; and W2XC_ERR_ARG for a depth outside 8 .. 16, a pack that
 * is not 0 or 1, an odd pointer, an odd row or frame stride, a stride below the row's bytes counted at 2 bytes per sample.
 * Left out: different depths on the two sides (8-bit in with 16-bit out included), left-sited chroma, TTA, the shrink, more than one 2x step, big-endian words,
 * packed 10-bit formats such as v210, uint16-fused first and last layers, multi-device striping, overlapped host sub-batches, a submit / wait pair.
 * (An output size, several 2x steps and the shrink now live in the _sized forms of these calls: "Sized YUV frames" below.) */
#define W2XC_PACK_LOW  0
#define W2XC_PACK_HIGH 1
typedef struct w2xc_yuv16_planes {   /* one side of a call: n frames */
    unsigned short *y;  size_t y_stride,  y_frame_stride;     /* bytes, even */
    unsigned short *u, *v; size_t c_stride, c_frame_stride;    /* bytes, even; P010: v = u + 1, c_px = 2 */
    int c_px;                                                  /* samples */
    int pack;                                                  /* W2XC_PACK_* */
} w2xc_yuv16_planes;
int w2xc_process_frames_yuv_u16_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth,
                                       const w2xc_yuv16_planes *d_in, const w2xc_yuv16_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u16(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth,
                                const w2xc_yuv16_planes *in, const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u16_rgb_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                           const w2xc_yuv16_planes *d_in, const w2xc_yuv16_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u16_rgb(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                    const w2xc_yuv16_planes *in, const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts);
/* The building blocks, as those of the 8-bit sections with `depth` behind `range` and `pack` behind `depth`: strides in bytes (even), src_px / dst_px in samples.
 * chroma2x_u16 writes only the words of its own samples: with dst_px = 2 two calls may fill the two planes in either order.
 * W2XC_ERR_ARG: what the 8-bit blocks refuse, a depth outside 8 .. 16, a pack that is not 0 or 1, odd pointers or strides. */
int w2xc_y16_to_plane_device(const unsigned short *d_src, int n, size_t frame_stride_bytes, size_t stride_bytes, int w, int h, int range, int depth, int pack,
                             float *d_dst, size_t plane_stride_bytes, void *hip_stream);
int w2xc_plane_to_y16_device(const float *d_src, int n, size_t plane_stride_bytes, int w, int h, int range, int depth, int pack, unsigned short *d_dst,
                             size_t frame_stride_bytes, size_t stride_bytes, void *hip_stream);
int w2xc_chroma2x_u16_device(const unsigned short *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw, int ch,
                             int depth, unsigned short *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack, int ow, int oh,
                             void *hip_stream);
int w2xc_yuv16_to_rgb_device(const w2xc_yuv16_planes *d_src, int n, int w, int h, int chroma, int range, int depth, int matrix, float *d_rgb,
                             size_t image_stride_bytes, size_t plane_stride_bytes, void *hip_stream);
int w2xc_rgb_to_yuv16_device(const float *d_rgb, size_t image_stride_bytes, size_t plane_stride_bytes, int n, int w, int h, int chroma, int range, int depth,
                             int matrix, const w2xc_yuv16_planes *d_dst, void *hip_stream);

/* ---- Chroma siting (revision 0.4.1.10) ----------------------------------------------------------------
 * The three sections above treat a chroma sample as CENTRED on its block of luma samples (JPEG / MPEG-1).  Most decoded video is not: 4:2:0 from MPEG-2, H.264
 * and HEVC is co-sited with the LEFT luma column, BT.2020 / UHD material with the TOP-LEFT luma sample, 4:2:2 with the left column almost everywhere (y4m:
 * C420mpeg2 against C420jpeg).  Two flag bits or-ed onto the layout value say so, per axis; no frame call gains an argument:
 *   W2XC_CHROMA_COSITED_X  along x chroma sample k sits ON luma column 2k         W2XC_CHROMA_COSITED_Y  along y chroma sample k sits ON luma row 2k
 *   W2XC_YUV_420_LEFT, W2XC_YUV_420_TOPLEFT, W2XC_YUV_422_LEFT: the three combinations in use.
 * The layout is chroma & 0xF, the flags chroma & 0x30; chroma sizes do not depend on the flags.  One siting applies to both sides of a call.
 * Accepted by all eight frame calls (w2xc_process_frames_yuv_u8[_rgb][_device], w2xc_process_frames_yuv_u16[_rgb][_device]) and by the four ends of the RGB
 * route (w2xc_yuv8_to_rgb_device, w2xc_rgb_to_yuv8_device, w2xc_yuv16_to_rgb_device, w2xc_rgb_to_yuv16_device).  Refused as W2XC_ERR_ARG, before a device is
 * touched: a negative value, any other bit, a layout outside 0 .. 3, and a flag on an axis the layout does not subsample -- any flag with W2XC_YUV_444 or
 * W2XC_YUV_400, W2XC_CHROMA_COSITED_Y with W2XC_YUV_422.  With no flag every call gives, byte for byte, what it gave before this revision.
 * The arithmetic, per axis; an axis that is centred or not subsampled is exactly what the sections above define.  Single fp32 operations in the order written
 * (-ffp-contract=off), for bytes and for words of any depth alike:
 *   Y route, the bicubic 2x of chroma on a co-sited axis: the luma 2x is pixel-centred, output luma X sits at source luma (X + 0.5) / 2 - 0.5; source chroma k sits on
 *              source luma 2k, output chroma m on output luma 2m, which is source chroma coordinate m / 2 - 0.125.  So sx = floor(m / 2 - 0.125) and t = 0.375 for odd
 *              m, 0.875 for even m; the taps are sx - 1 .. sx + 2, clamped, the coefficients cubic_coeffs(t), the tap sum that of the centred enlargement --
 *              horizontally, then vertically --, then its rounding.  Outputs 2q - 1 and 2q share sx = q - 1: the centred enlargement with (0.25, 0.75) replaced
 *              by (0.375, 0.875) on that axis and nothing else -- not the clamping, the crop to the leading (2 w + 1) / 2 samples, nor column 0.  iterations = 0:
 *              the samples are copied, as before.
 *   RGB route, chroma at luma resolution on a co-sited axis: luma index x reads j = x >> 1; even x: C[j]; odd x: 0.5f * C[j] + 0.5f * C[min(j + 1, last)] -- both
 *              exact in fp32 at every depth.  Horizontally first, then vertically on the row results.
 *   RGB route, from R, G, B, on a co-sited axis: chroma sample k is the 1-2-1 mean around luma 2k: with l = P[max(2k - 1, 0)], m = P[2k], r = P[min(2k + 1, last)] of
 *              cb (and of cr), (l + r) * 0.25f + m * 0.5f -- the sum, two exact scalings, one sum.  Horizontally first, on every luma row the vertical step needs
 *              (a centred subsampled x axis: (a + b) * 0.5f of the block's two columns, the last replicated at an odd edge); then a co-sited y axis applies the
 *              same expression to rows 2k - 1, 2k, 2k + 1 (clamped), a centred subsampled y axis (top + bottom) * 0.5f to the block's two rows, an odd edge
 *              replicating the last row, and an axis not subsampled passes through.  Both axes centred: the box mean ((a + b) + (c + d)) * 0.25f, unchanged.
 *              The roundings to bytes and words are unchanged.
 * The frame calls stay DEFINED as their composed routes of public calls, the same `chroma` value handed to both ends; the Y route uses
 * w2xc_chroma2x_u8_sited_device / w2xc_chroma2x_u16_sited_device per chroma plane, with the flags.  Those two are this revision's only new entry points (their
 * presence marks it; w2xc_opts and w2xc_version() are unchanged): w2xc_chroma2x_u8_device / _u16_device with `cosited` behind `oh` -- any combination of the two
 * flag bits, anything else W2XC_ERR_ARG; cosited = 0 is the centred block, byte for byte.
 * Left out: per-plane sitings (PAL-DV 4:2:0, whose Cb and Cr sit on different lines), different sitings on the two sides of a call, TTA, the shrink, more than one
 * 2x step.
 * (An output size, several 2x steps and the shrink now live in the _sized forms of these calls: "Sized YUV frames" below.) */
#define W2XC_CHROMA_COSITED_X 0x10   /* along x a chroma sample sits ON luma column 2k (left-sited)   */
#define W2XC_CHROMA_COSITED_Y 0x20   /* along y a chroma sample sits ON luma row 2k (top-sited)        */
#define W2XC_YUV_420_LEFT    (W2XC_YUV_420 | W2XC_CHROMA_COSITED_X)                         /* MPEG-2, H.264, HEVC default */
#define W2XC_YUV_420_TOPLEFT (W2XC_YUV_420 | W2XC_CHROMA_COSITED_X | W2XC_CHROMA_COSITED_Y) /* BT.2020 / UHD               */
#define W2XC_YUV_422_LEFT    (W2XC_YUV_422 | W2XC_CHROMA_COSITED_X)
int w2xc_chroma2x_u8_sited_device(const unsigned char *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int cw, int ch,
                                  unsigned char *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int ow, int oh, int cosited,
                                  void *hip_stream);
int w2xc_chroma2x_u16_sited_device(const unsigned short *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw,
                                   int ch, int depth, unsigned short *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack,
                                   int ow, int oh, int cosited, void *hip_stream);

/* ---- Sized YUV frames (revision 0.4.1.11) --------------------------------------------------------------
 * The eight frame calls above leave a frame at its own size or at exactly twice it.  Their _sized forms take an output size and up to four 2x steps: 720p ->
 * 1080p (1.5x), 540p -> 2160p (4x), DVD 720 x 480 -> 1920 x 1080 (2.67x by 2.25x).  Each is its base call with `out_w, out_h` in front of the output planes;
 * w2xc_opts and w2xc_version() are unchanged, the new symbols mark the revision, and every older entry point keeps its arguments, its refusals and its bytes.
 *   iterations: 0 .. 4, as in the image calls, or W2XC_ITERATIONS_AUTO (-1): the smallest k with (w << k) >= out_w and (h << k) >= out_h.
 *   output size: with W = w << iterations and H = h << iterations, w <= out_w <= W and h <= out_h <= H, the two axes independent: the output is never smaller than
 *              the input, and with iterations = 0 it has the input's size.  The output chroma planes have the chroma size of an out_w x out_h frame, by the rule
 *              of "YUV frames".
 *   refused, before a device is touched: everything the base call refuses, with its code, except that iterations 2 .. 4 and AUTO are legal; an output size
 *              outside those ranges (AUTO that four steps do not reach included) W2XC_ERR_ARG; iterations >= 1 without a scale model, a head model as noise
 *              model, as before.
 * The arithmetic.  Every expression is a sequence of single fp32 operations in the order given, in files built with -ffp-contract=off; coordinates are computed
 * in double, as w2xc_resize_linear_device computes its own.
 *   luma, Y route: "luma in" of the base call; the noise pass; `iterations` times y <- CNN_scale(nearest2x(y)), which is w2xc_convert_batch_device with nn2x = 1,
 *              unclipped between the passes; where (out_w, out_h) != (W, H), exactly w2xc_resize_linear_device from W x H to out_w x out_h; "luma out" of the
 *              base call.
 *   RGB route: w2xc_yuv8_to_rgb_device / w2xc_yuv16_to_rgb_device at w x h; the passes of w2xc_process_image_rgb_u8* for that many iterations (a head model
 *              enlarges by itself, as there); w2xc_resize_linear_device on each of the three planes; w2xc_rgb_to_yuv8_device / w2xc_rgb_to_yuv16_device at
 *              out_w x out_h.  The same `chroma` value, siting flags included, goes to both ends.
 *   chroma, Y route: ONE step from the input plane to the output plane -- chroma does not pass the CNN, so it gains nothing from being resampled once per 2x step
 *              and rounded to samples in between.  Per axis r = (double)w / out_w ((double)h / out_h in y), the LUMA ratio, not a quotient of chroma sizes: odd
 *              sizes stay aligned with luma.  o = 0.5 on a centred or unsubsampled axis, 0.25 on a co-sited one.  For output chroma sample m, in double:
 *              pos = (m + o) * r - o -- the sum, the product, the difference --, s = floor(pos), t = (float)(pos - s); the taps s - 1 .. s + 2 clamped into the
 *              plane; the coefficients cubic_coeffs(t) of w2xc_resize2x_cubic_device; the values (float)C * (float)(1.0 / 255.0) ((float)(1.0 / M) for words); the
 *              tap sum of the 2x enlargement, horizontally then vertically; saturate(rint(255 c)), or clamp(rint(c * M), 0, M) for words.
 *              At r = 0.5 this IS the existing enlargement, for every m, column 0 and the crop included: centred t = 0.25 for odd m and 0.75 for even m,
 *              co-sited 0.375 / 0.875, in both s = q - 1 for m = 2q - 1 and m = 2q (every double operation above is exact there).  At r = 1, pos = m, t = 0
 *              and cubic_coeffs(0) is exactly (0, 1, 0, 0): the plane is copied.
 * The frame calls are DEFINED, by bytes and words, as these composed routes of public calls, for every option set the routes accept (fusion settings, precisions,
 * named kernels, a cutting band_rows at S = 1); the Y route uses w2xc_chroma_resize_u8_device / _u16_device per chroma plane.  With iterations <= 1 and (out_w,
 * out_h) = (W, H) a sized call gives, byte for byte, what the base call gives: the engine runs the chroma copy where the output has the input's size and the
 * bicubic 2x kernels at exactly twice it, the resize kernels everywhere else.  Sub-batches (the per-frame memory has the float planes of every level and of the
 * shrunk one), bands at S = 1, the lock, the stream rules, the host form and device_mask are those of the base calls; a sub-batch is ONE chroma launch and, where
 * the output is not the last level, ONE launch of the linear stage for its luma (or 3 S RGB) planes.
 * The two blocks: w2xc_chroma2x_u8_sited_device / _u16_sited_device with the luma sizes of both sides (w, h, out_w, out_h: they give the ratios; out_w >= w and
 * out_h >= h) and the layout's two subsampling flags (sub_x, sub_y, 0 or 1: with `cosited` they give o; a siting flag on an axis that is not subsampled is
 * W2XC_ERR_ARG) behind `oh`.  Any cw x ch -> ow x oh with ow, oh >= 1: the 2x blocks' bound on ow and oh is gone, their other refusals stay.  They always run
 * the resize kernels (tiles of 32 x 16 output samples, the source window of at most 35 x 19 samples in LDS as floats), at r = 1 and r = 0.5 too.
 * Left out: output smaller than the input, antialiasing in the linear shrink (OpenCV has none either), a fused luma shrink-and-quantise kernel (the shrunk float
 * plane exists in memory), a shrink fused into the from-RGB kernels, TTA, different depths or sitings on the two sides, multi-device striping, a submit / wait
 * pair. */
#define W2XC_ITERATIONS_AUTO (-1)
int w2xc_process_frames_yuv_u8_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range,
                                            const w2xc_yuv_planes *d_in, int out_w, int out_h, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream,
                                            const w2xc_opts *opts);
int w2xc_process_frames_yuv_u8_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *in,
                                     int out_w, int out_h, const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u8_rgb_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                                const w2xc_yuv_planes *d_in, int out_w, int out_h, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream,
                                                const w2xc_opts *opts);
int w2xc_process_frames_yuv_u8_rgb_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                         const w2xc_yuv_planes *in, int out_w, int out_h, const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u16_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth,
                                             const w2xc_yuv16_planes *d_in, int out_w, int out_h, const w2xc_yuv16_planes *d_out, int iterations, void *hip_stream,
                                             const w2xc_opts *opts);
int w2xc_process_frames_yuv_u16_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth,
                                      const w2xc_yuv16_planes *in, int out_w, int out_h, const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u16_rgb_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                                 const w2xc_yuv16_planes *d_in, int out_w, int out_h, const w2xc_yuv16_planes *d_out, int iterations,
                                                 void *hip_stream, const w2xc_opts *opts);
int w2xc_process_frames_yuv_u16_rgb_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                          const w2xc_yuv16_planes *in, int out_w, int out_h, const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts);
int w2xc_chroma_resize_u8_device(const unsigned char *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int cw, int ch,
                                 unsigned char *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int ow, int oh, int w, int h, int out_w,
                                 int out_h, int sub_x, int sub_y, int cosited, void *hip_stream);
int w2xc_chroma_resize_u16_device(const unsigned short *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw,
                                  int ch, int depth, unsigned short *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack,
                                  int ow, int oh, int w, int h, int out_w, int out_h, int sub_x, int sub_y, int cosited, void *hip_stream);

/* the building blocks on contiguous float planes (device pointers): main.cpp:144 on one plane, :75-76, :171-172 */
int w2xc_resize2x_cubic_device(const float *d_src, int w, int h, float *d_dst, void *hip_stream);
/* main.cpp:158-167 on one plane (revision 0.4.1.4): cv::resize(Size(dw, dh), INTER_LINEAR) of the contiguous sw x sh plane d_src into the contiguous
 * dw x dh plane d_dst, any sizes >= 1 (the image calls only shrink).  Output (dx, dy) reads fx = float((dx + 0.5) * (double)sw / dw - 0.5), sx =
 * floor(fx), fx -= sx; sx < 0 or sx >= sw - 1 clamps sx into the row with fx = 0, the second tap is min(sx + 1, sw - 1); the same in y.  Rows first,
 * h = S[sx] * (1 - fx) + S[sx + 1] * fx for the two rows, then h0 * (1 - fy) + h1 * fy, all in unfused fp32; no antialiasing, like OpenCV.
 * W2XC_ERR_ARG for a null pointer or a size below 1.  Asynchronous on hip_stream, on the current device. */
int w2xc_resize_linear_device(const float *d_src, int sw, int sh, float *d_dst, int dw, int dh, void *hip_stream);
int w2xc_u8_to_yuv_device(const unsigned char *d_in, size_t in_stride_bytes, int w, int h, float *d_y, float *d_u,
                          float *d_v, void *hip_stream);
int w2xc_yuv_to_u8_device(const float *d_y, const float *d_u, const float *d_v, int w, int h, unsigned char *d_out,
                          size_t out_stride_bytes, void *hip_stream);

/* ... and the RGB pipeline's: u8 / 255 into three contiguous w x h float planes, saturate(rint(255 x)) back */
int w2xc_u8_to_rgb_device(const unsigned char *d_in, size_t in_stride_bytes, int w, int h, float *d_c0, float *d_c1, float *d_c2, void *hip_stream);
int w2xc_rgb_to_u8_device(const float *d_c0, const float *d_c1, const float *d_c2, int w, int h, unsigned char *d_out, size_t out_stride_bytes,
                          void *hip_stream);

/* ... and the RGBA call's: the colour bleed alone.  `passes` (>= 0) passes of the bleed above on the w x h RGBA image d_in; d_out_rgb receives the packed
 * 3-channel image (rows out_stride_bytes >= 3 w apart, bytes behind 3 w untouched; it must not overlap d_in).  Asynchronous on hip_stream, on the current
 * device.  Up to 16 effective passes run in one launch and need no scratch.  More run as one launch per pass, and as the call has no model, their scratch
 * (2 bytes per pixel of the largest such image so far) is one buffer per device, shared by all callers and kept until
 * w2xc_bleed_rgba_u8_trim -- calls on different streams that may run at the same time are the caller's to order, as with the calls of one model.
 * w2xc_bleed_rgba_u8_trim waits for every device that holds such a buffer and releases it (what w2xc_model_trim is to a model's buffers). */
int w2xc_bleed_rgba_u8_device(const unsigned char *d_in, size_t in_stride_bytes, int w, int h, int passes, unsigned char *d_out_rgb,
                              size_t out_stride_bytes, void *hip_stream);
int w2xc_bleed_rgba_u8_trim(void);

/* == Model::filter(inputPlanes, outputPlanes) for layer `layer` (modelHandler.cpp:26-72):
 * n_in_planes host planes of h x w floats in, nout planes out, SAME size, per-layer
 * BORDER_REPLICATE (:141-142), bias, LeakyReLU(0.1) (:147-152).  Returns W2XC_ERR_PLANES when
 * n_in_planes != nInputPlanes (the reference returns false, :29-35). */
int w2xc_layer_filter(w2xc_model *m, int layer, int n_in_planes, const float *const *in_planes,
                      size_t in_stride_bytes, int w, int h, float *const *out_planes,
                      size_t out_stride_bytes, const w2xc_opts *opts);

/* The same layer on DEVICE data with arbitrary element strides (in floats): element (plane c, row y, pixel x) is at
 * base[c*plane_stride + y*row_stride + x*pixel_stride] -- planar planes (pixel_stride 1) as Model::filter has them, or
 * NHWC (plane_stride 1, pixel_stride = plane count, 16-byte aligned), which the MFMA kernels use directly so a chain
 * of calls that hands NHWC from layer to layer never repacks.  Asynchronous on `hip_stream`. */
int w2xc_layer_filter_device(w2xc_model *m, int layer, int n_in_planes, const float *d_in, long long in_plane_stride,
                             long long in_row_stride, long long in_pixel_stride, int w, int h, float *d_out,
                             long long out_plane_stride, long long out_row_stride, long long out_pixel_stride,
                             void *hip_stream, const w2xc_opts *opts);

/* ---- measurement / introspection ------------------------------------------------------------ */

/* With opts->profile = 1 every layer launch of the device entry point is bracketed by hipEvents
 * on the launch stream.  After the stream has been synchronised, this returns for each layer the
 * SUM of its launch durations (ms) and the number of launches since the last reset. */
int  w2xc_profile_read(w2xc_model *m, int device, float *layer_ms, int *layer_launches, int n_layers);
void w2xc_profile_reset(w2xc_model *m, int device);
/* name of the kernel the engine picks for a layer (for matching rocprofv3 kernel traces) */
const char *w2xc_layer_kernel_name(const w2xc_model *m, int layer, const w2xc_opts *opts);

/* The band geometry a w2xc_convert_rows_device call with these arguments would run with, computed on the host (no device needed, nothing is
 * allocated or launched): halo rows per layer (1, or 4 = the banding-invariant geometry of the default F(4x4) kernel), output rows per band,
 * number of bands, bytes of the two activation workspaces, and whether the two cross-layer fusions are in effect.  Fails exactly where the
 * conversion would refuse its arguments (W2XC_ERR_ARG for W2XC_KERNEL_AUTO on a minimum-halo view, W2XC_ERR_PLANES ...). */
typedef struct w2xc_row_plan {
    int struct_size;
    int n_layers;
    int halo_rows_per_layer;
    int band_rows;
    int n_bands;
    int fused_first, fused_last;
    unsigned long long workspace_bytes[2];
} w2xc_row_plan;
int w2xc_plan_rows(const w2xc_model *m, int w, int view_y0, int view_h, int plane_h, int row_begin, int row_end, const w2xc_opts *opts,
                   w2xc_row_plan *plan);
/* plane rows [*top, *bottom) that layer `layer` (1 .. n_layers) computes for the band of output rows [y0, y1) under `plan`
 * (negative rows / rows >= plane_h + ...: the replicate padding of convertRoutine.cpp:35 seen from that layer).
 * An upconv head model: every row here is a SOURCE row (w, plane_h, row_begin / row_end of w2xc_plan_rows are the source's), the head is layer n_layers and
 * its region [y0, y1) stands for the output rows [2 y0, 2 y1); it reads z rows [y0, y1 + 2) -- z row i is plane row i - 1 of layer n - 1, whose region
 * [y0 - 1, y1 + 1) on the one-row-per-layer geometry (a superset on the four-row one) is exactly those. */
int w2xc_plan_region(const w2xc_row_plan *plan, int plane_h, int layer, int y0, int y1, int *top, int *bottom);

/* Test aid.  Fills every grow-only scratch buffer the (model, device) context owns with the
 * 32-bit word `word` and returns the number of bytes filled in *bytes (0 when the context does
 * not exist yet: it is not created).  Synchronises the device before and after.
 * Filled, each allocation whole: the two activation workspaces, Model::filter's device planes and bounce ring, the host pipeline's device rows,
 * staging rings and page-locked band buffers, the image pipeline's planes -- data only.  Weights, biases and every synchronisation word (job counters
 * and flags, events) are left alone.  What w2xc_opts.filter_resident promises is gone afterwards.  A conversion that follows must give the result it
 * gives on fresh memory for every `word`: tests/test_gpu_scratch_poison.py.  device = -1: the current device.  Not to be called concurrently with
 * asynchronous work of the caller on this (model, device) that has not been synchronised. */
int w2xc_debug_fill_scratch(w2xc_model *m, int device, unsigned word, unsigned long long *bytes);

/* Test aid (0.4.1.12).  Makes ONE later event of `kind` fail on the host, in place of the runtime call it stands for -- nothing faulty reaches the device:
 *   W2XC_DEBUG_FAIL_ALLOC   a grow-only buffer that has to grow (the allocation behind the drain and the release of the old buffer; a buffer that is
 *                           large enough is no event) and the allocation of a weight image            -> the call returns W2XC_ERR_NOMEM
 *   W2XC_DEBUG_FAIL_COPY    the upload of a weight image (with the model's first use on a device, and of the lazily packed images with the first
 *                           call that runs their kernel)                                                  -> W2XC_ERR_HIP
 *   W2XC_DEBUG_FAIL_LAUNCH  the launch of a model layer (every conv / upconv launch of every entry point; not the colour, YUV, TTA and resize
 *                           stages, not copies, streams or events): nothing is launched               -> W2XC_ERR_HIP
 * nth >= 1: the nth event of that kind from now on, in the whole process, fails once; the seam is then disarmed.  nth = 0 disarms.  Returns the number
 * of events of that kind since the previous call with that kind (0 for the first): a caller counts a call's events between two calls with nth = 0.
 * An unknown kind or a negative nth returns -1 and arms nothing.  Costs one relaxed load per event in a process that never calls it; reads no
 * environment variable.  What a caller may assume after the non-zero return: INTEGRATION.md "After an error"; tests/test_gpu_fail_paths.py. */
#define W2XC_DEBUG_FAIL_ALLOC  1
#define W2XC_DEBUG_FAIL_COPY   2
#define W2XC_DEBUG_FAIL_LAUNCH 3
long long w2xc_debug_fail_nth(int kind, long long nth);

int w2xc_device_count(void);          /* hipGetDeviceCount, 0 when no device / no driver           */
const char *w2xc_last_error(void);    /* thread-local message of the last failing call             */
const char *w2xc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* W2XC_HIP_H_ */
