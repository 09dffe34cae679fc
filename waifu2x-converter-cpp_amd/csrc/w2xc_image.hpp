// w2xc_image.hpp -- what the image units w2xc_image*.cpp share (internal; the map: w2xc_engine.hpp).  What is fixed for a call travels as an ImageCall, the uint8
// images as U8Images views.  Things one unit uses alone stay in that unit's anonymous namespace; the integers of all of them are w2xc_host_geom.hpp's.
#pragma once
#include "w2xc_engine.hpp"
#include "w2xc_host_geom.hpp"

namespace w2xc_eng {
// These functions were file-local before the units were split.  Hidden visibility keeps them out of the library's dynamic symbols, so that what it exports
// stays the C ABI of include/w2xc_hip.h and the w2xc_eng names it exported before; they are called between the image units only.
#pragma GCC visibility push(hidden)

// the Y / U / V planes of both image pipelines live in the owning context's aux buffer, behind `skip` bytes (a multiple of 256) that are the caller's: the
// RGBA call keeps its uint8 images there.  (A buffer that grows loses its content: whoever owns such bytes reserves the whole call's need first.)
inline int reserve_aux(DevCtx *c, size_t skip, size_t floats) { return c->aux.reserve(skip + floats * sizeof(float), "the image planes"); }
inline float *aux_planes(DevCtx *c, size_t skip) { return reinterpret_cast<float *>(c->aux.as<unsigned char>() + skip); }

// What is fixed for one image call: the models and (once a device is open) their contexts, the source size and the passes, the final size, stream, options.
struct ImageCall {
    w2xc_model *mn, *msc;
    CallCtx ctx;
    int w, h, iterations;
    double shrink;
    int fw = 0, fh = 0;   // final_size: set by check_image_size, which refuses the arguments it cannot be computed from
    hipStream_t st;
    w2xc_opts o;
    // who runs a CNN pass of the Y pipeline: run_rows (the single-image calls: bands for large images) or run_batch (everything else)
    bool rows = false;
    // test-time augmentation (the *_tta entry points): every CNN pass of the route is its TTA pass (tta_pass).  tta_arg = the caller's int as given:
    // check_process_args refuses anything but 0 and 1
    int tta_arg;
    bool tta;
    // w2xc_process_image_rgb_u8_up2x_batch[_device] and w2xc_process_image_rgba_u8_up2x_batch[_device]: the scale model is an upconv head model (and must be
    // one), also under TTA
    bool up2x = false;
    // the RGBA TTA calls, RGB and head routes, w2xc_opts.fusion other than W2XC_FUSION_OFF (check_rgba_call sets it): the first spread of a sequence reads the
    // uint8 image itself, the gather behind a last scale pass without a shrink writes the caller's pixels (w2xc_tta_u8.hip; rgb_plan)
    bool tta_u8 = false;
    ImageCall(w2xc_model *noise, w2xc_model *scale, int w_, int h_, int iterations_, double shrink_, void *hip_stream, const w2xc_opts *opts, int tta_ = 0)
        : mn(noise), msc(scale), w(w_), h(h_), iterations(iterations_), shrink(shrink_), st((hipStream_t)hip_stream), o(resolve_opts(opts)), tta_arg(tta_),
          tta(tta_ == 1) {}
};

// uint8 images of one size: image i at p + i * img bytes, its rows `row` bytes apart
template <class T> struct U8Images {
    T *p;
    size_t img, row;
};
typedef U8Images<const unsigned char> U8In;
typedef U8Images<unsigned char> U8Out;

// ---- test-time augmentation: one TTA pass of a model (the arithmetic: include/w2xc_hip.h) ----
// spread -> the CNN on the 8 variants -> gather, for `runs` CNN runs per variant of nin planes in and nout planes out each: `src` = the runs * nin source
// planes, `dst` = the runs * nout result planes.  `var` holds tta_pass_floats(w, h, up) floats per source plane and per result plane's share
// (8 (ni ps + no PS) in all): the input variants -- the upright group, the transposed group directly behind it -- then the output variants likewise.
// rows = false (nin = nout = 1): the one-plane chain, run_batch on all variants of one size -- ONE batch of 8 where w == h, where the transposed group
// continues the upright one.  rows = true: the multi-plane form, run_batch_planes on the variants of one size as images of nin planes (8 runs of them where
// w == h, else 4 runs + 4 runs) -- one launch per layer where the model's chain has batch kernels, the single-image run_rows sequence per variant and run elsewhere.
// Nearest-2x commutes with every T_k: a scale pass (up = 1) spreads at source resolution and gathers at 2x.  So does an upconv head model's pass (head: up = 0,
// nothing is folded into layer 1, and the model itself gives the 2x planes): its variants are the images of a head batch.
struct TtaPass {
    w2xc_model *m;
    DevCtx *cm;
    int up, nin, nout;
    bool rows;
    bool head = false;
    bool head_a = false;   // head, nout = 1: the head launches compute channel 1 alone, as one float plane (ROWS_F32_DST_A)
};
// The uint8 ends of a pass (nin = 3; `runs` = images): src -- the spread reads n interleaved images itself, `src` of tta_pass is not used; dst -- the gather
// writes n_ch bytes of each pixel, from the result planes first .. first + n_ch - 1 of each image, `dst` of tta_pass is not used.
struct TtaU8 {
    const unsigned char *src = nullptr;
    size_t src_img = 0, src_row = 0;
    int px = 3, ch0 = 0, ch_step = 1;
    unsigned char *dst = nullptr;   // (the first byte the gather writes: byte0 is in the pointer)
    size_t dst_img = 0, dst_row = 0;
    int dpx = 4, n_ch = 3, first = 0;
};
int tta_pass(const TtaPass &t, int runs, PlanesIn src, int w, int h, PlanesOut dst, float *var, hipStream_t st, const w2xc_opts &o, const TtaU8 *u8 = nullptr);

// The alpha planes that ride with Y (the Y route of w2xc_process_image_rgba_u8*): a = u8 / 255 of the S RGBA images `src`, through every scale iteration as
// the second half of a run_batch of 2 S planes -- the S alpha planes directly behind the S Y planes that feed the iteration -- and through the shrink; never
// through the noise model.  plane = where the call left image 0's (the final size), image i's ps floats on.  Only with iterations >= 1.
struct AlphaRide {
    U8In src;
    float *plane;
    long long ps;
};
// the Y pipeline and the RGB pipeline for a sub-batch of S images (S <= cap, the call's sub-batch size); skip: the float planes start that many bytes into the aux buffer
int process_y_device(const ImageCall &c, int S, int cap, U8In in, U8Out out, size_t skip = 0, AlphaRide *al = nullptr);
int process_rgb_device(const ImageCall &c, int S, int cap, U8In in, U8Out out, size_t skip = 0, int ends = 0);

// What one image needs of float planes, and whether the call's first / last layer takes the uint8 image itself (the chain's u8_source / u8_sink: then the
// float copy of the source / of the result -- 4^iterations as many pixels -- does not exist):
struct RgbPlan {
    bool src_u8 = false, dst_u8 = false;
    size_t floats = 0;
    size_t var = 0;   // TTA: floats of the levels' planes, behind which the variant planes of a pass lie (three planes' worth per image)
};
RgbPlan rgb_plan(const ImageCall &c);

// The planes of a level of the sub-batch: image i's three at p + i * 3 ps, w x h each, ps floats apart
struct RgbLevel {
    float *p;
    int w, h;
    long long ps;
};
int rgb_passes(const ImageCall &c, const RgbPlan &R, int S, int cap, U8In in, U8Out out, int ends, float **base_io, float *var, RgbLevel *L);

// the plan of a call and what the entry points refuse before any device is touched (w2xc_image.cpp)
enum PlanKind { PLAN_Y, PLAN_RGB };
int plan_image_call(PlanKind kind, const ImageCall &c, int *sub, size_t per_image = 0, int ya = 1, const char *call = "w2xc_process_image_rgb_u8*");
int check_y_models(const ImageCall &c);
int check_process_args(const ImageCall &c, bool head_ok = false);
int check_image_size(ImageCall &c, size_t in_stride, size_t out_stride, int px = 3);
int check_image_extent(const ImageCall &c);

// ---- the call forms, written once: a family brings its checks and ONE callable that enqueues a sub-batch of S images (S <= cap) on the call's contexts ----
// (a reference to the caller's callable, which outlives the call: no allocation, one indirect call per sub-batch)
class SubBatchRef {
    const void *f_;
    int (*call_)(const void *, const ImageCall &, int, int, U8In, U8Out);
public:
    template <class F> SubBatchRef(const F &f)
        : f_(&f), call_([](const void *p, const ImageCall &c, int S, int cap, U8In in, U8Out out) { return (*static_cast<const F *>(p))(c, S, cap, in, out); }) {}
    int operator()(const ImageCall &c, int S, int cap, U8In in, U8Out out) const { return call_(f_, c, S, cap, in, out); }
};
// One host image of px-byte pixels on device `dev`, synchronously (a single image has nothing to overlap with): the call's contexts opened and locked, c.rows set,
// blocking copies around what `enqueue` puts on the null stream
int host_single_form(ImageCall &c, int px, U8In in, U8Out out, int dev, SubBatchRef enqueue);
// n host images behind the family's argument checks: sub-batches of at most `sub` through batch_host_run; n = 1: host_single_form on the first device of the mask
int host_batch_form(ImageCall &c, int n, const unsigned char *const *in, size_t in_stride, unsigned char *const *out, size_t out_stride, int px, int sub,
                    SubBatchRef enqueue);
// n device images: what a batch of px-byte images refuses of its pointers' ranges (c.fw / c.fh are set) ...
int check_device_batch_overlap(const ImageCall &c, int n, U8In in, U8Out out, int px);
// ... and the sub-batch loop, the call's contexts on w2xc_opts.device opened and locked around it
int device_batch_form(ImageCall &c, int n, int sub, U8In in, U8Out out, SubBatchRef enqueue);
// run(first, S) for the sub-batches [first, first + S) of n items, at most `sub` each
template <class F> int for_sub_batches(int n, int sub, F run)
{
    for (int b0 = 0; b0 < n; b0 += sub)
        if (int rc = run(b0, std::min(sub, n - b0))) return rc;
    return W2XC_OK;
}

#pragma GCC visibility pop
}  // namespace w2xc_eng
