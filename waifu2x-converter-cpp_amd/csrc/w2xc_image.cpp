// w2xc_image.cpp -- N2: the CLI's image pipeline around the plane conversion -- uint8 BGR -> float YUV, the noise /
// scale passes on Y, bicubic U/V, the final shrink, YUV -> uint8 (main.cpp:74-76,83-98,126-172).
// And the same surface for RGB models (3 planes in, 3 out; w2xc_process_image_rgb_u8*): no chroma side path, every pass a CNN pass on all three planes,
// the first and the last layer of the call reading / writing the uint8 image themselves where their kernels can (no counterpart in v1).
// One pipeline per route -- process_y_device, process_rgb_device -- for S images of one size: the single-image calls, the batches and the RGBA call
// (process_rgba_device, around either) all run these two.  What is fixed for a call travels as an ImageCall, the uint8 images as U8Images views.
// And frames that are Y, U and V already (w2xc_process_frames_yuv_u8*): process_yuv_device, the Y pipeline without its colour stages -- and, through RGB and
// head models by a colour matrix the caller names (w2xc_process_frames_yuv_u8_rgb*), process_yuv_rgb_device: the passes of the RGB pipeline between two kernels.
#include "w2xc_engine.hpp"
#include "w2xc_host_geom.hpp"

namespace w2xc_eng {

namespace {

// the Y / U / V planes of both image pipelines live in the owning context's aux buffer, behind `skip` bytes (a multiple of 256) that are the caller's: the
// RGBA call keeps its uint8 images there.  (A buffer that grows loses its content: whoever owns such bytes reserves the whole call's need first.)
int reserve_aux(DevCtx *c, size_t skip, size_t floats) { return c->aux.reserve(skip + floats * sizeof(float), "the image planes"); }
float *aux_planes(DevCtx *c, size_t skip) { return reinterpret_cast<float *>(c->aux.as<unsigned char>() + skip); }
size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// What is fixed for one image call: the models and (once a device is open) their contexts, the source size and the passes, the final size, stream, options.
struct ImageCall {
    w2xc_model *mn, *msc;
    CallCtx ctx;
    int w, h, iterations;
    double shrink;
    int fw = 0, fh = 0;   // final_size: set by check_image_args, which refuses the arguments it cannot be computed from
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
int tta_pass(const TtaPass &t, int runs, PlanesIn src, int w, int h, PlanesOut dst, float *var, hipStream_t st, const w2xc_opts &o, const TtaU8 *u8 = nullptr)
{
    const int sc = t.head ? 1 : t.up;   // the pass's enlargement
    const int W = w << sc, H = h << sc, ni = runs * t.nin, no = runs * t.nout;
    const long long ps = (long long)plane_floats(w, h), PS = (long long)plane_floats(W, H);
    // the four groups of variant planes: 4 ni upright and 4 ni transposed (h x w) in, 4 no and 4 no out
    const PlanesOut in_up{var, (size_t)w, ps}, in_tr{in_up.p + 4 * (size_t)ni * ps, (size_t)h, ps};
    const PlanesOut out_up{in_tr.p + 4 * (size_t)ni * ps, (size_t)W, PS}, out_tr{out_up.p + 4 * (size_t)no * PS, (size_t)H, PS};
    if (u8 && u8->src) HIP_TRY(w2xc_launch_tta_spread_u8(u8->src, u8->src_img, u8->src_row, u8->px, u8->ch0, u8->ch_step, w, h, in_up.p, in_tr.p, ps, runs, st));
    else HIP_TRY(w2xc_launch_tta_spread(src.p, src.ps, (long long)src.rs, w, h, in_up.p, in_tr.p, ps, ni, st));
    if (!t.rows) {
        if (w == h) {
            if (int rc = run_batch(t.m, t.cm, 8 * ni, t.up, in_up, w, h, out_up, st, o)) return rc;
        } else {
            if (int rc = run_batch(t.m, t.cm, 4 * ni, t.up, in_up, w, h, out_up, st, o)) return rc;
            if (int rc = run_batch(t.m, t.cm, 4 * ni, t.up, in_tr, h, w, out_tr, st, o)) return rc;
        }
    } else {
        // variant (k, run r) is "image" (k & 3) runs + r of its group: nin planes ps apart in, nout planes PS apart out.  Where the model's chain has batch
        // kernels (batch_eligible) a group is ONE run_batch_planes launch sequence, otherwise that call is the single-image run_rows sequence per variant and run
        const auto group = [&](int nv, const PlanesOut &in, int vw, int vh, const PlanesOut &out) {
            const BatchIO io = {in, t.nin * ps, t.nin, out, t.nout * PS, t.head_a ? ROWS_F32_DST_A : 0};
            return run_batch_planes(t.m, t.cm, nv * runs, t.up, io, vw, vh, st, o);
        };
        if (w == h) {
            if (int rc = group(8, in_up, w, h, out_up)) return rc;
        } else {
            if (int rc = group(4, in_up, w, h, out_up)) return rc;
            if (int rc = group(4, in_tr, h, w, out_tr)) return rc;
        }
    }
    if (u8 && u8->dst) HIP_TRY(w2xc_launch_tta_gather_u8(out_up.p, out_tr.p, PS, W, H, u8->dst, u8->dst_img, u8->dst_row, u8->dpx, 0, u8->n_ch, t.nout, u8->first, runs, st));
    else HIP_TRY(w2xc_launch_tta_gather(out_up.p, out_tr.p, PS, W, H, dst.p, dst.ps, (long long)dst.rs, no, st));
    return W2XC_OK;
}

// uint8 images of one size: image i at p + i * img bytes, its rows `row` bytes apart
template <class T> struct U8Images {
    T *p;
    size_t img, row;
};
typedef U8Images<const unsigned char> U8In;
typedef U8Images<unsigned char> U8Out;

// The alpha planes that ride with Y (the Y route of w2xc_process_image_rgba_u8*): a = u8 / 255 of the S RGBA images `src`, through every scale iteration as
// the second half of a run_batch of 2 S planes -- the S alpha planes directly behind the S Y planes that feed the iteration -- and through the shrink; never
// through the noise model.  plane = where the call left image 0's (the final size), image i's ps floats on.  Only with iterations >= 1.
struct AlphaRide {
    U8In src;
    float *plane;
    long long ps;
};

// The Y pipeline for a sub-batch of S images (S <= cap, the call's sub-batch size: the planes are sized by cap, not by the call's n): noise (optional,
// main.cpp:83-98) then `iterations` 2x scale steps (main.cpp:126-156), the shrink, the colour stages around them.  Every plane lies on a plane_floats
// boundary, ps floats from the next; a level holds the Y group (S Y planes, with alpha S alpha planes behind them), S U planes, S V planes, level 0 also
// the Y group of the noise pass (image_aux_floats).  So the Y planes go to run_batch as they lie, U and V are 2 S adjacent planes for the bicubic launch, all of them the
// planes of the one shrink launch.  One launch per colour / resize stage.
int process_y_device(const ImageCall &c, int S, int cap, U8In in, U8Out out, size_t skip = 0, AlphaRide *al = nullptr)
{
    DevCtx *own = c.ctx.owner();
    const size_t ya = al ? 2 : 1, ny = ya * S;   // planes a Y takes (itself and its alpha), planes of the Y group
    if (int rc = reserve_aux(own, skip, image_aux_floats(c.w, c.h, c.iterations, c.shrink, al != nullptr, c.tta) * (size_t)cap)) return rc;
    // (TTA: the variant planes of a pass lie behind the planes of every level, cap images' worth; every pass reuses them)
    float *var = aux_planes(own, skip) + image_aux_floats(c.w, c.h, c.iterations, c.shrink, al != nullptr) * (size_t)cap;
    // One CNN pass on Y: the noise pass (up = 0) on the S Y planes alone -- alpha never goes through the noise model; beside an alpha plane ONE Y
    // plane is the single call's run_rows -- a scale pass (up = 1) on the whole Y group.  Per plane the bits of the single call either way (run_batch).
    const auto pass = [&](int up, const float *src, long long sps, int w, int h, float *dst, long long dps) {
        const bool noise = up == 0;
        w2xc_model *m = noise ? c.mn : c.msc;
        DevCtx *cm = noise ? c.ctx.cn : c.ctx.cs;
        const int nw = w << up, nh = h << up;   // (up = 1: INTER_NEAREST 2x folded into layer 1, :136-140, + convertWithModels, :148)
        const int np = noise ? S : (int)ny;
        const PlanesIn in{src, (size_t)w, sps};
        const PlanesOut out{dst, (size_t)nw, dps};
        if (c.tta) return tta_pass(TtaPass{m, cm, up, 1, 1, false}, np, in, w, h, out, var, c.st, c.o);
        return c.rows || (noise && al && S == 1) ? run_rows(m, cm, RowsCall::whole(in.plane(0), 1, nw, nh, out.plane(0), up), c.st, c.o)
                                       : run_batch(m, cm, np, up, in, w, h, out, c.st, c.o);
    };
    float *base = aux_planes(own, skip);
    int cw = c.w, ch = c.h;
    long long ps = (long long)plane_floats(cw, ch);
    float *y = base, *u = y + ny * ps, *v = u + (size_t)S * ps, *yn = v + (size_t)S * ps;
    base += (2 * ya + 2) * (size_t)cap * ps;
    HIP_TRY(w2xc_launch_u8_to_yuv_batch(in.p, in.img, in.row, cw, ch, y, u, v, ps, S, c.st));                // :75-76
    if (al) HIP_TRY(w2xc_launch_alpha_to_plane(al->src.p, al->src.img, al->src.row, cw, ch, (c.mn ? yn : y) + (size_t)S * ps, ps, S, c.st));
    if (c.mn) {                                                                                             // :91-98
        if (int rc = pass(0, y, ps, cw, ch, yn, ps)) return rc;
        y = yn;
    }
    for (int it = 0; it < c.iterations; it++) {
        const int nw = cw * 2, nh = ch * 2;
        const long long ps2 = (long long)plane_floats(nw, nh);
        float *y2 = base, *u2 = y2 + ny * ps2;
        base += (ya + 2) * (size_t)cap * ps2;
        if (int rc = pass(1, y, ps, cw, ch, y2, ps2)) return rc;                                         // :136-148
        HIP_TRY(w2xc_launch_resize2x_cubic_batch(u, ps, cw, ch, u2, ps2, 2 * S, c.st));                      // :144-146 (v = u + S ps, v2 = u2 + S ps2)
        y = y2; u = u2; cw = nw; ch = nh; ps = ps2;
    }
    if (c.shrink > 0.0) {                                                                                   // :158-167
        const long long pss = (long long)plane_floats(c.fw, c.fh);
        // (the Y source is a base of its own: after a noise pass the Y group does not adjoin U)
        HIP_TRY(w2xc_launch_resize_linear_batch(y, u, (int)ny, ps, cw, ch, base, pss, c.fw, c.fh, (int)ny + 2 * S, c.st));
        y = base; u = y + ny * pss; cw = c.fw; ch = c.fh; ps = pss;
    }
    HIP_TRY(w2xc_launch_yuv_to_u8_batch(y, u, u + (size_t)S * ps, ps, cw, ch, out.p, out.img, out.row, S, c.st));   // :171-172
    if (al) { al->plane = y + (size_t)S * ps; al->ps = ps; }
    return W2XC_OK;
}

// ---- RGB models (w2xc_process_image_rgb_u8*) ----
// x = u8 / 255 on the three channels as given; with a noise model x <- CNN(x); per iteration x <- CNN(nearest2x(x)), the 2x folded into layer 1; an optional
// INTER_LINEAR shrink per plane; out = saturate(rint(255 x)).  Between passes the image is three float planes, unclipped, like Y in the pipeline above.
// What one image needs of float planes, and whether the call's first / last layer takes the uint8 image itself (u8_source_layer / u8_sink_layer: then the
// float copy of the source / of the result -- 4^iterations as many pixels -- does not exist):
struct RgbPlan {
    bool src_u8 = false, dst_u8 = false;
    size_t floats = 0;
    size_t var = 0;   // TTA: floats of the levels' planes, behind which the variant planes of a pass lie (three planes' worth per image)
};
RgbPlan rgb_plan(const ImageCall &c)
{
    RgbPlan R;
    const int passes = (c.mn ? 1 : 0) + c.iterations;
    // (TTA: the mean is taken before the rounding, so no LAYER takes the uint8 image; the RGBA TTA calls have the spread and the gather take it -- whatever
    // the precision and the kernels -- the gather where the last pass is a scale pass with nothing behind it)
    R.src_u8 = c.tta ? c.tta_u8 : u8_source_layer(c.mn ? c.mn : c.msc, c.o);
    R.dst_u8 = c.tta ? c.tta_u8 && c.shrink == 0.0 && c.iterations > 0 : c.shrink == 0.0 && u8_sink_layer(c.iterations > 0 ? c.msc : c.mn, c.o);
    if (!R.src_u8) R.floats += 3 * plane_floats(c.w, c.h);
    for (int p = 1; p <= passes; p++) {
        const int lvl = p - (c.mn ? 1 : 0);   // the pass's output level: the noise pass stays on level 0
        if (p < passes || !R.dst_u8) R.floats += 3 * plane_floats(c.w << lvl, c.h << lvl);
    }
    if (c.shrink > 0.0) R.floats += 3 * plane_floats(c.fw, c.fh);
    R.var = R.floats;
    if (c.tta) R.floats += 3 * tta_variant_floats(c.w, c.h, c.iterations);
    return R;
}

// The planes of a level of the sub-batch: image i's three at p + i * 3 ps, w x h each, ps floats apart
struct RgbLevel {
    float *p;
    int w, h;
    long long ps;
};
// The CNN passes of the call -- the noise pass, then `iterations` scale passes -- on a sub-batch, what process_rgb_device and process_yuv_rgb_device (YUV frames
// through RGB models) share.  *L: in, the planes the first pass reads (p = nullptr: the image is still the caller's uint8 source `in`); out, the planes behind
// the last pass -- p = nullptr again where that pass wrote the uint8 image `out` itself (R.dst_u8): nothing is left to do.  *base = the next free float of the
// call's planes, var = the variant planes of a TTA pass.
int rgb_passes(const ImageCall &c, const RgbPlan &R, int S, int cap, U8In in, U8Out out, int ends, float **base_io, float *var, RgbLevel *L)
{
    const long long in_cs = (ends & ROWS_U8_SRC_A) ? 0 : 1;   // (bytes between the channels of a source pixel)
    float *base = *base_io, *cur = L->p;
    int cw = L->w, ch = L->h;
    long long ps = L->ps;
    const int passes = (c.mn ? 1 : 0) + c.iterations;
    for (int p = 1; p <= passes; p++) {
        const bool noise = c.mn && p == 1;
        w2xc_model *m = noise ? c.mn : c.msc;
        DevCtx *cm = noise ? c.ctx.cn : c.ctx.cs;
        const bool head = m->has_head();   // (the scale model of the single-image call and of the up2x batch: the pass enlarges by itself, nothing is folded into layer 1)
        const int up = noise || head ? 0 : 1, nw = cw << (noise ? 0 : 1), nh = ch << (noise ? 0 : 1);
        const long long ps2 = (long long)plane_floats(nw, nh);
        const bool from_u8 = cur == nullptr, to_u8 = p == passes && R.dst_u8;
        const int u8 = (from_u8 ? ROWS_U8_SRC | (ends & ROWS_U8_SRC_A) : 0) | (to_u8 ? ROWS_U8_DST | (ends & (ROWS_U8_DST_PX4 | ROWS_U8_DST_A)) : 0);
        float *nxt = nullptr;
        if (!to_u8) { nxt = base; base += 3 * (size_t)cap * ps2; }
        if (c.tta) {
            // (from_u8 / to_u8: the RGBA TTA calls.  ends as without TTA, but ROWS_U8_SRC_A: `in` is the RGBA image itself, alpha is byte 3 of its pixels;
            // ROWS_U8_DST_A: `out` points at byte 3, which gets channel 1 -- from a head the one plane its alpha launches compute)
            TtaU8 u;
            if (from_u8) { u.src = in.p; u.src_img = in.img; u.src_row = in.row; }
            if (from_u8 && (ends & ROWS_U8_SRC_A)) { u.px = 4; u.ch0 = 3; u.ch_step = 0; }
            const bool one = to_u8 && (ends & ROWS_U8_DST_A), head_a = one && head;
            if (to_u8) { u.dst = out.p; u.dst_img = out.img; u.dst_row = out.row; u.n_ch = one ? 1 : 3; u.first = one && !head_a ? 1 : 0; }
            const TtaPass t{m, cm, up, 3, head_a ? 1 : 3, true, head, head_a};
            if (int rc = tta_pass(t, S, {cur, (size_t)cw, ps}, cw, ch, {nxt, (size_t)nw, ps2}, var, c.st, c.o, &u)) return rc;
        } else if (S >= 2) {
            // ONE run_batch_planes for the sub-batch (one launch per layer where the chain has batch kernels): image i's three planes 3 ps on, or -- the uint8
            // forms -- the caller's images themselves: strides in bytes
            const BatchIO io = {from_u8 ? PlanesIn{reinterpret_cast<const float *>(in.p), in.row, in_cs} : PlanesIn{cur, (size_t)cw, ps}, from_u8 ? (long long)in.img : 3 * ps, 3,
                                to_u8 ? PlanesOut{reinterpret_cast<float *>(out.p), out.row, 1} : PlanesOut{nxt, (size_t)nw, ps2}, to_u8 ? (long long)out.img : 3 * ps2, u8};
            if (int rc = run_batch_planes(m, cm, S, up, io, cw, ch, c.st, c.o)) return rc;
        } else for (int i = 0; i < S; i++) {   // (a sub-batch of one: the single-image call, bands included)
            // image i's three planes, or -- the uint8 forms -- the caller's image itself: strides in bytes (Planes, w2xc_engine.hpp)
            const PlanesIn src = from_u8 ? PlanesIn{reinterpret_cast<const float *>(in.p + (size_t)i * in.img), in.row, in_cs} : PlanesIn{cur + (size_t)i * 3 * ps, (size_t)cw, ps};
            const PlanesOut dst = to_u8 ? PlanesOut{reinterpret_cast<float *>(out.p + (size_t)i * out.img), out.row, 1} : PlanesOut{nxt + (size_t)i * 3 * ps2, (size_t)nw, ps2};
            int rc = run_rows(m, cm, RowsCall::whole(src, 3, head ? cw : nw, head ? ch : nh, dst, up, u8), c.st, c.o);
            if (rc) return rc;
        }
        if (to_u8) { L->p = nullptr; return W2XC_OK; }
        cur = nxt; cw = nw; ch = nh; ps = ps2;
    }
    *base_io = base;
    *L = {cur, cw, ch, ps};
    return W2XC_OK;
}

// A sub-batch of S images (S <= cap; the planes are sized by cap): per level the three planes of image i lie at level + i * 3 ps, ps floats apart.  The
// colour stages and the shrink are one launch for the sub-batch, and so is every layer of a pass of S >= 2 images where the model's chain has batch kernels
// (run_batch_planes; elsewhere it is the single-image launch sequence per image, enqueued back to back).  A single image is a sub-batch of one: run_rows.
// (skip: the float planes start that many bytes into the aux buffer -- reserve_aux)
// ends (the RGBA call for head models; ROWS_U8_SRC_A / ROWS_U8_DST_PX4 / ROWS_U8_DST_A of w2xc_engine.hpp): `in` is the alpha byte of RGBA pixels, `out` byte 0
// -- the alpha head: byte 3 -- of RGBA pixels.  Only where the call's first / last layer takes the uint8 image itself (rgb_plan: the caller asks it first).
int process_rgb_device(const ImageCall &c, int S, int cap, U8In in, U8Out out, size_t skip = 0, int ends = 0)
{
    DevCtx *own = c.ctx.owner();
    const RgbPlan R = rgb_plan(c);
    if (((ends & ROWS_U8_SRC_A) && !R.src_u8) || ((ends & (ROWS_U8_DST_PX4 | ROWS_U8_DST_A)) && !R.dst_u8))
        return fail(W2XC_ERR_ARG, "internal error: RGBA pixels for a pass that runs around float planes");
    float *base = nullptr;
    if (R.floats) {
        if (int rc = reserve_aux(own, skip, R.floats * (size_t)cap)) return rc;
        base = aux_planes(own, skip);
    }
    float *var = base + R.var * (size_t)cap;
    RgbLevel L = {nullptr, c.w, c.h, (long long)plane_floats(c.w, c.h)};   // (p = nullptr: the image is still the caller's uint8 source)
    if (!R.src_u8) {
        L.p = base;
        base += 3 * (size_t)cap * L.ps;
        HIP_TRY(w2xc_launch_u8_to_rgb_batch(in.p, in.img, in.row, L.w, L.h, L.p, L.ps, 3 * L.ps, S, c.st));
    }
    if (int rc = rgb_passes(c, R, S, cap, in, out, ends, &base, var, &L)) return rc;
    if (!L.p) return W2XC_OK;   // (the last pass wrote the caller's image)
    float *cur = L.p;
    int cw = L.w, ch = L.h;
    long long ps = L.ps;
    if (c.shrink > 0.0) {
        const long long pss = (long long)plane_floats(c.fw, c.fh);
        HIP_TRY(w2xc_launch_resize_linear_batch(cur, cur, 3 * S, ps, cw, ch, base, pss, c.fw, c.fh, 3 * S, c.st));   // (the 3 S planes of a level are ps apart)
        cur = base; cw = c.fw; ch = c.fh; ps = pss;
    }
    HIP_TRY(w2xc_launch_rgb_to_u8_batch(cur, ps, 3 * ps, cw, ch, out.p, out.img, out.row, S, c.st));
    return W2XC_OK;
}

int process_sub_batch(bool rgb, const ImageCall &c, int S, int cap, U8In in, U8Out out)
{
    return rgb ? process_rgb_device(c, S, cap, in, out) : process_y_device(c, S, cap, in, out);
}

// ---- the plan of a call: host arithmetic only, before any device is touched ----
// The options' errors (plan_rows) of the noise pass and of the largest scale pass, and *sub = images per sub-batch of a batch: as many as
// w2xc_opts.workspace_mb holds of the pipeline's own memory per image (the float planes of every level + the uint8 image in and out), at least 1.
//   PLAN_RGB  first: each model takes three planes and gives three (a Y model beside an RGB one fails here too)
//   both      at most the sub-batch run_batch / run_batch_planes takes at the LARGEST level where a batched chain applies (more images would only be cut again
//             there, and the planes of a larger sub-batch would be memory without a launch saved)
// The RGBA call gives its own bytes per image (per_image; 0 = the 3-channel call's, above) and ya = 2 on the Y route: a Y brings its alpha plane, so a
// sub-batch run_batch takes whole holds half as many images.
enum PlanKind { PLAN_Y, PLAN_RGB };
int plan_image_call(PlanKind kind, const ImageCall &c, int *sub, size_t per_image = 0, int ya = 1, const char *call = "w2xc_process_image_rgb_u8*")
{
    const bool rgb = kind == PLAN_RGB;
    const w2xc_model *pass[2] = {c.mn, c.msc};
    if (rgb) for (const w2xc_model *m : pass) {
        if (!m) continue;
        if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
        if (m->layers[0].nin != 3 || m->layers.back().nout != 3)
            return fail(W2XC_ERR_PLANES, "%s: three planes in and three planes out (the model takes %d and gives %d)", call, m->layers[0].nin,
                        m->layers.back().nout);
    }
    size_t k = 65535;
    pass[1] = c.iterations > 0 ? c.msc : nullptr;
    for (int i = 0; i < 2; i++) {
        if (!pass[i]) continue;
        int W = i ? c.w << c.iterations : c.w, H = i ? c.h << c.iterations : c.h;   // (the last scale iteration: the largest planes of the call)
        if (i && pass[i]->has_head()) { W >>= 1; H >>= 1; }   // (an upconv head model is planned on its source)
        RowPlan P;
        if (int rc = plan_rows(pass[i], c.o, W, H, 0, 0, H, H, rgb ? 3 : 1, rgb, &P)) return rc;
        if (batch_eligible(pass[i], P)) {
            size_t img_f[2];
            batch_ws_floats(P, img_f);
            k = std::min<size_t>(k, (size_t)batch_sub_size(P.o, img_f));
        }
    }
    const size_t budget = (size_t)(c.o.workspace_mb > 0 ? c.o.workspace_mb : 16384) << 20;
    const size_t floats = rgb ? rgb_plan(c).floats : image_aux_floats(c.w, c.h, c.iterations, c.shrink, false, c.tta);
    const size_t per = per_image ? per_image : floats * 4 + (size_t)c.w * 3 * c.h + (size_t)c.fw * 3 * c.fh;
    *sub = (int)std::max<size_t>(std::min(k / ya, budget / per), 1);
    return W2XC_OK;
}

// the Y route through run_batch -- the batch forms, the alpha ride, the variants of a TTA pass -- asks one plane in and one out of each model
int check_y_models(const ImageCall &c)
{
    if (c.mn) if (int rc = check_batch_model(c.mn)) return rc;
    if (c.msc) if (int rc = check_batch_model(c.msc)) return rc;
    return W2XC_OK;
}

// head_ok: the call is w2xc_process_image_rgb_u8_ex[_device], which takes an upconv head model as its scale model; every other image call refuses one
int check_process_args(const ImageCall &c, bool head_ok = false)
{
    if (c.tta_arg != 0 && c.tta_arg != 1) return fail(W2XC_ERR_ARG, "tta must be 0 or 1 (got %d)", c.tta_arg);
    if (int rc = refuse_head(c.mn, "the noise model of an image call")) return rc;
    if (c.up2x) {
        if (!c.msc || !c.msc->has_head()) return fail(W2XC_ERR_ARG, "w2xc_process_image_rgb[a]_u8_up2x_batch*: the scale model must be an upconv head model");
    } else if (!(head_ok && !c.tta)) if (int rc = refuse_head(c.msc, "this image call")) return rc;
    if (!c.mn && !c.msc) return fail(W2XC_ERR_ARG, "need a noise model, a scale model or both");
    if (c.iterations > 0 && !c.msc) return fail(W2XC_ERR_ARG, "scale iterations need a scale model");
    if (!c.mn && c.iterations == 0) return fail(W2XC_ERR_ARG, "nothing to do (no noise model, 0 iterations)");
    return W2XC_OK;
}

// the sizes and row strides of an image call (px bytes per pixel); sets the call's final size (behind check_process_args: one model is there)
int check_image_size(ImageCall &c, size_t in_stride, size_t out_stride, int px = 3)
{
    if (c.w <= 0 || c.h <= 0 || c.iterations < 0 || c.iterations > 4) return fail(W2XC_ERR_ARG, "bad image size / iteration count");
    if (c.shrink < 0.0 || c.shrink >= 1.0) return fail(W2XC_ERR_ARG, "shrink_ratio must be 0 (none) or in (0,1)");
    final_size(c.w, c.h, c.iterations, c.shrink, &c.fw, &c.fh);
    if (c.fw < 1 || c.fh < 1) return fail(W2XC_ERR_ARG, "shrink_ratio leaves an empty image");
    if (in_stride < (size_t)c.w * px || out_stride < (size_t)c.fw * px) return fail(W2XC_ERR_ARG, "row strides must be >= %d*width bytes", px);
    return W2XC_OK;
}
// ... and the two pointers of a single image (a batch checks its own)
int check_image_args(ImageCall &c, const void *in, size_t in_stride, const void *out, size_t out_stride, int px = 3)
{
    if (!in || !out) return fail(W2XC_ERR_ARG, "null argument");
    return check_image_size(c, in_stride, out_stride, px);
}

// the largest level of the call, (w << iterations) x (h << iterations), is at most 2^28 a side (what the plans and the layouts above compute with)
int check_image_extent(const ImageCall &c)
{
    if (c.w > (1 << 28) >> c.iterations || c.h > (1 << 28) >> c.iterations) return fail(W2XC_ERR_ARG, "image too large");
    return W2XC_OK;
}

// One host image on the call's open device, synchronously (a single image has nothing to overlap with): blocking copies of the px-byte pixels around what
// `enqueue(device image in, device image out)` puts on the null stream.  The device copies live in the owning context and are kept between calls -- no
// hipMalloc / hipFree per image.
template <class F> int host_round_trip(const ImageCall &c, int px, U8In in, U8Out out, F enqueue)
{
    DevCtx *own = c.ctx.owner();
    const size_t rs = (size_t)c.w * px, RS = (size_t)c.fw * px, in_bytes = align256(rs * c.h);
    if (int rc = own->img_io.reserve(in_bytes + RS * c.fh, "the image")) return rc;
    unsigned char *d_in = own->img_io.as<unsigned char>(), *d_out = d_in + in_bytes;
    HIP_TRY(hipMemcpy2D(d_in, rs, in.p, in.row, rs, c.h, hipMemcpyHostToDevice));
    if (int rc = enqueue(U8In{d_in, 0, rs}, U8Out{d_out, 0, RS})) { hipDeviceSynchronize(); return rc; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(out.p, out.row, d_out, RS, RS, c.fh, hipMemcpyDeviceToHost));
    return W2XC_OK;
}

// w2xc_process_image_[rgb_]u8_ex on device `dev`, and a host batch of one image
int image_host_single(bool rgb, ImageCall &c, U8In in, U8Out out, int dev)
{
    LockedCtx lc;
    if (int rc = lc.open(c.mn, c.msc, dev)) return rc;
    c.ctx = lc;
    c.rows = true;
    return host_round_trip(c, 3, in, out, [&](U8In d_in, U8Out d_out) { return process_sub_batch(rgb, c, 1, 1, d_in, d_out); });
}

// what both batch forms refuse before any device is touched (the image pointers are the caller's: checked there)
int check_image_batch_args(bool rgb, ImageCall &c, int n, size_t in_stride, size_t out_stride)
{
    if (n < 1) return fail(W2XC_ERR_ARG, "batch of %d images", n);
    int rc = check_process_args(c);
    if (rc) return rc;
    if ((rc = check_image_size(c, in_stride, out_stride))) return rc;
    if ((rc = check_image_extent(c))) return rc;
    return rgb ? W2XC_OK : check_y_models(c);   // (RGB: the models' plane form is plan_image_call's, behind the caller's pointer checks)
}

// ---- RGBA images (w2xc_process_image_rgba_u8*) ----
// bleed -> the 3-channel pipeline of the route on the bled images -> alpha through the scale model -> merge, for a sub-batch of S
// images; the single call is a sub-batch of one.  The call's uint8 images live at the head of the owning context's aux buffer, cap images each at
// 256-byte-aligned image strides, the pipelines' float planes behind them:
//   bled   the packed 3-channel images after the bleed      stamp  the bleed's pass stamps (16 bits per pixel; only the pass chain has them)
//   res    the packed 3-channel results of the colour call  grey / ares (RGB route, iterations >= 1)  alpha as the images (A, A, A), and their results
// A head model as scale model (w2xc_process_image_rgba_u8_up2x_batch*; RGB route, iterations >= 1) runs the same sequence, fused at either end where the layer
// at that end has the uint8 kernel (rgb_plan):
//   fuse_src  layer 1 of the alpha pass reads the caller's alpha bytes itself: no grey images, no AlphaToGrey launch
//   fuse_dst  the colour pass's head writes bytes 0 .. 2 of the caller's output pixels and the alpha pass's head -- the alpha head, channel 1 alone -- byte 3:
//             no res and ares images, no merge launch
// Under TTA (w2xc_process_image_rgba_u8[_up2x]_batch_tta*; c.tta) every CNN pass of the sequence is its TTA pass.  Y route: the alpha planes ride in the scale
// pass's tta_pass.  RGB and head routes, c.tta_u8: the same two flags, for every model, now the spread's and the gather's (w2xc_tta_u8.hip) -- fuse_src: the
// alpha sequence's first spread reads the caller's alpha bytes (and the colour sequence's the bled image: rgb_plan); fuse_dst: the gathers behind the last scale
// pass write the caller's pixels, the alpha one from channel 1 (a head: from the one plane its alpha launches compute, ROWS_F32_DST_A).
struct RgbaPlan {
    bool rgb = false;
    bool fuse_src = false, fuse_dst = false;
    int passes = 0;          // bleed passes that can change a pixel: no pixel is farther than max(w, h) - 1 from an opaque one
    int sub = 1;             // images per sub-batch (plan_image_call)
    size_t bled = 0, stamp = 0, res = 0, grey = 0, ares = 0;   // bytes per image of each (a multiple of 256; 0 = the call has none)
    size_t floats = 0;       // float planes per image
};
// where those lie for sub-batches of at most cap images: byte offsets; head = where the float planes start
struct RgbaLayout {
    size_t bled, stamp, res, grey, ares, head, bytes;
    RgbaLayout(const RgbaPlan &R, size_t cap)
    {
        size_t at = 0;
        const auto take = [&](size_t img) { const size_t a = at; at += cap * img; return a; };
        bled = take(R.bled); stamp = take(R.stamp); res = take(R.res); grey = take(R.grey); ares = take(R.ares);
        head = at;
        bytes = at + cap * R.floats * sizeof(float);
    }
};

// the scale-only call on the same image: what alpha goes through on the RGB route
ImageCall alpha_call(const ImageCall &c)
{
    ImageCall a = c;
    a.mn = nullptr;
    a.ctx.cn = nullptr;
    return a;
}

// The route (the models choose it), everything the 3-channel call of the route refuses, and the plan -- host arithmetic only.
int plan_rgba(const ImageCall &c, int bleed_passes, RgbaPlan *R)
{
    const w2xc_model *first = c.mn ? c.mn : c.msc;
    if (first->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    if (int rc = check_image_extent(c)) return rc;
    R->rgb = c.up2x || first->layers[0].nin == 3;   // (the head call has the RGB route only: a one-plane head model is refused as the 3-channel call refuses it)
    if (!R->rgb) if (int rc = check_y_models(c)) return rc;
    if (int rc = plan_image_call(R->rgb ? PLAN_RGB : PLAN_Y, c, &R->sub)) return rc;   // (the models' and the options' errors, before the models are asked anything)
    long long P = bleed_passes;
    if (P < 0) P = (long long)(c.mn ? c.mn->layers.size() : 0) + (long long)(c.msc ? c.msc->layers.size() : 0);   // the CNN's reach at source resolution
    P = std::min<long long>(P, std::max(c.w, c.h) - 1);
    if (P > 65534) return fail(W2XC_ERR_ARG, "more than 65534 effective bleed passes");
    R->passes = (int)P;
    R->bled = align256((size_t)c.w * 3 * c.h);
    if (w2xc_bleed_stamps((int)P)) R->stamp = align256((size_t)c.w * 2 * c.h);
    const bool ride = c.iterations > 0;   // alpha goes through the scale model
    if (R->rgb && ride && (c.msc->has_head() || c.tta)) {   // (under TTA the ends are the spread's and the gather's: every model)
        R->fuse_src = rgb_plan(alpha_call(c)).src_u8;
        R->fuse_dst = rgb_plan(c).dst_u8;   // (the colour pass and the alpha pass end in the same layer under the same options)
    }
    if (!R->fuse_dst) R->res = align256((size_t)c.fw * 3 * c.fh);
    if (R->rgb) {
        R->floats = rgb_plan(c).floats;
        if (ride) {
            if (!R->fuse_src) R->grey = align256((size_t)c.w * 3 * c.h);
            if (!R->fuse_dst) R->ares = align256((size_t)c.fw * 3 * c.fh);
            R->floats = std::max(R->floats, rgb_plan(alpha_call(c)).floats);
        }
    } else R->floats = image_aux_floats(c.w, c.h, c.iterations, c.shrink, ride, c.tta);
    if (!ride && c.shrink > 0.0) R->floats = std::max(R->floats, plane_floats(c.w, c.h) + plane_floats(c.fw, c.fh));   // alpha as a plane and its shrunk plane
    // what one image takes: the float planes, alpha's among them, the uint8 images above, the 4-byte image in and out
    const size_t per = R->floats * sizeof(float) + R->bled + R->stamp + R->res + R->grey + R->ares + (size_t)c.w * 4 * c.h + (size_t)c.fw * 4 * c.fh;
    return plan_image_call(R->rgb ? PLAN_RGB : PLAN_Y, c, &R->sub, per, !R->rgb && ride ? 2 : 1);
}

// a sub-batch of S images (S <= cap, the call's sub-batch size).  c.rows: the single call -- where Y runs alone (no scale pass) its pass is run_rows
int process_rgba_device(const RgbaPlan &R, const ImageCall &c, int S, int cap, U8In in, U8Out out)
{
    DevCtx *own = c.ctx.owner();
    const RgbaLayout L(R, (size_t)cap);
    if (int rc = own->aux.reserve(L.bytes, "the RGBA images and their planes")) return rc;   // (all of it first: a buffer that grows loses its content)
    unsigned char *a8 = own->aux.as<unsigned char>();
    const int w = c.w, h = c.h, W = c.fw, H = c.fh;
    const size_t rs = (size_t)w * 3, RS = (size_t)W * 3;
    const U8In bled{a8 + L.bled, R.bled, rs};
    const U8Out res{a8 + L.res, R.res, RS};
    HIP_TRY(w2xc_launch_rgba_bleed(in.p, in.img, in.row, w, h, R.passes, a8 + L.bled, R.bled, rs, reinterpret_cast<unsigned short *>(a8 + L.stamp), R.stamp / 2, S, c.st));
    if (R.rgb) {
        // (fuse_dst, a head model: the colour bytes go into the caller's pixels as the head computes them)
        if (int rc = process_rgb_device(c, S, cap, bled, R.fuse_dst ? out : res, L.head, R.fuse_dst ? ROWS_U8_DST_PX4 : 0)) return rc;
        if (c.iterations > 0) {   // alpha = channel 1 of the scale-only call on (A, A, A)
            // fuse_src: layer 1 reads the alpha bytes where they are; fuse_dst: the alpha head computes channel 1 alone, into byte 3 of the caller's pixels
            U8In grey{c.tta ? in.p : in.p + 3, in.img, in.row};   // (TTA: the spread selects the byte)
            if (!R.fuse_src) {
                HIP_TRY(w2xc_launch_alpha_to_grey(in.p, in.img, in.row, w, h, a8 + L.grey, R.grey, rs, S, c.st));
                grey = U8In{a8 + L.grey, R.grey, rs};
            }
            const U8Out ares = R.fuse_dst ? U8Out{out.p + 3, out.img, out.row} : U8Out{a8 + L.ares, R.ares, RS};
            const int ends = (R.fuse_src ? ROWS_U8_SRC_A : 0) | (R.fuse_dst ? ROWS_U8_DST_PX4 | ROWS_U8_DST_A : 0);
            if (int rc = process_rgb_device(alpha_call(c), S, cap, grey, ares, L.head, ends)) return rc;
            if (!R.fuse_dst) HIP_TRY(w2xc_launch_merge_rgba_u8(res.p, res.img, RS, a8 + L.ares + 1, R.ares, RS, 3, W, H, out.p, out.img, out.row, S, c.st));
            return W2XC_OK;
        }
    } else {   // with a scale pass alpha rides with Y (run_batch's passes); without one the 3-channel call as it is: the single image through run_rows
        AlphaRide al = {in, nullptr, 0};
        ImageCall y = c;
        y.rows = c.rows && c.iterations == 0;
        if (int rc = process_y_device(y, S, cap, bled, res, L.head, c.iterations > 0 ? &al : nullptr)) return rc;
        if (c.iterations > 0) {
            HIP_TRY(w2xc_launch_merge_rgba(res.p, res.img, RS, al.plane, al.ps, W, H, out.p, out.img, out.row, S, c.st));
            return W2XC_OK;
        }
    }
    if (c.shrink > 0.0) {
        // no scale pass but a shrink (both routes): a = u8 / 255, INTER_LINEAR like every other plane, rounded in the merge.  The pipeline's float planes
        // are free again: its result is the uint8 images `res`, and everything here follows it on the stream.
        const long long ps = (long long)plane_floats(w, h), pss = (long long)plane_floats(W, H);
        float *a0 = aux_planes(own, L.head), *a1 = a0 + (size_t)cap * ps;
        HIP_TRY(w2xc_launch_alpha_to_plane(in.p, in.img, in.row, w, h, a0, ps, S, c.st));
        HIP_TRY(w2xc_launch_resize_linear_batch(a0, a0, S, ps, w, h, a1, pss, W, H, S, c.st));
        HIP_TRY(w2xc_launch_merge_rgba(res.p, res.img, RS, a1, pss, W, H, out.p, out.img, out.row, S, c.st));
        return W2XC_OK;
    }
    // same size: the alpha bytes as they are
    HIP_TRY(w2xc_launch_merge_rgba_u8(res.p, res.img, RS, in.p + 3, in.img, in.row, 4, W, H, out.p, out.img, out.row, S, c.st));
    return W2XC_OK;
}

// what every form of the RGBA call refuses before any device is touched (the image pointers are the caller's: checked there)
int check_rgba_call(ImageCall &c, size_t in_stride, size_t out_stride, int bleed_passes, RgbaPlan *R)
{
    int rc = check_process_args(c);
    if (rc) return rc;
    if ((rc = check_image_size(c, in_stride, out_stride, 4))) return rc;
    c.tta_u8 = c.tta && c.o.fusion != W2XC_FUSION_OFF;
    return plan_rgba(c, bleed_passes, R);
}
int check_rgba_single(ImageCall &c, U8In in, U8Out out, int bleed_passes, RgbaPlan *R)
{
    int rc = check_process_args(c);
    if (rc || (rc = check_image_args(c, in.p, in.row, out.p, out.row, 4))) return rc;
    if (ranges_overlap(in.p, image_extent(c.h, in.row, c.w, 4), out.p, image_extent(c.fh, out.row, c.fw, 4)))
        return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
    c.tta_u8 = c.tta && c.o.fusion != W2XC_FUSION_OFF;
    return plan_rgba(c, bleed_passes, R);
}

int rgba_ex_device(ImageCall c, U8In in, U8Out out, int bleed_passes)
{
    RgbaPlan R;
    LockedCtx lc;
    int rc = check_rgba_single(c, in, out, bleed_passes, &R);
    if (rc || (rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    c.rows = true;
    return process_rgba_device(R, c, 1, 1, in, out);
}

// one host image on device `dev`, synchronously: w2xc_process_image_rgba_u8_ex (w2xc_opts.device), and a host batch of one image
int rgba_host_single(const RgbaPlan &R, ImageCall &c, U8In in, U8Out out, int dev)
{
    LockedCtx lc;
    if (int rc = lc.open(c.mn, c.msc, dev)) return rc;
    c.ctx = lc;
    c.rows = true;
    return host_round_trip(c, 4, in, out, [&](U8In d_in, U8Out d_out) { return process_rgba_device(R, c, 1, 1, d_in, d_out); });
}

int rgba_ex_host(ImageCall c, U8In in, U8Out out, int bleed_passes)
{
    RgbaPlan R;
    if (int rc = check_rgba_single(c, in, out, bleed_passes, &R)) return rc;
    if (w2xc_device_count() <= 0) return fail(W2XC_ERR_HIP, "no HIP device available (libw2xc_hip has no CPU fallback)");
    return rgba_host_single(R, c, in, out, c.o.device);
}

// ---- batches of RGBA images: image i byte for byte the single call's ----
int rgba_batch_device(ImageCall c, int n, U8In in, U8Out out, int bleed_passes)
{
    if (n < 1) return fail(W2XC_ERR_ARG, "batch of %d images", n);
    if (!in.p || !out.p) return fail(W2XC_ERR_ARG, "null argument");
    RgbaPlan R;
    int rc = check_rgba_call(c, in.row, out.row, bleed_passes, &R);
    if (rc) return rc;
    const size_t in_ext = image_extent(c.h, in.row, c.w, 4), out_ext = image_extent(c.fh, out.row, c.fw, 4);
    if (n > 1 && out.img < out_ext)
        return fail(W2XC_ERR_ARG, "output images overlap each other (image stride %zu < %zu bytes)", out.img, out_ext);
    if (ranges_overlap(in.p, (size_t)(n - 1) * in.img + in_ext, out.p, (size_t)(n - 1) * out.img + out_ext))
        return fail(W2XC_ERR_ARG, "output images overlap the input images");
    const int sub = std::min(R.sub, n);
    LockedCtx lc;
    if ((rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    c.rows = n == 1;   // (a batch of one is the single call, bands included)
    for (int b0 = 0; b0 < n; b0 += sub) {
        rc = process_rgba_device(R, c, std::min(sub, n - b0), sub, U8In{in.p + (size_t)b0 * in.img, in.img, in.row},
                                 U8Out{out.p + (size_t)b0 * out.img, out.img, out.row});
        if (rc) return rc;
    }
    return W2XC_OK;
}

int rgba_batch_host(ImageCall c, int n, const unsigned char *const *in, size_t in_stride, unsigned char *const *out, size_t out_stride, int bleed_passes)
{
    if (n < 1) return fail(W2XC_ERR_ARG, "batch of %d images", n);
    if (!in || !out) return fail(W2XC_ERR_ARG, "null argument");
    RgbaPlan R;
    int rc = check_rgba_call(c, in_stride, out_stride, bleed_passes, &R);
    if (rc) return rc;
    rc = check_batch_host_ptrs(n, (const void *const *)in, image_extent(c.h, in_stride, c.w, 4), (void *const *)out, image_extent(c.fh, out_stride, c.fw, 4));
    if (rc) return rc;
    if (n == 1) {   // nothing to overlap: the synchronous single-image sequence, on the first device of the mask
        std::vector<int> devs;
        if ((rc = host_devices(c.o, &devs))) return rc;
        return rgba_host_single(R, c, U8In{in[0], 0, in_stride}, U8Out{out[0], 0, out_stride}, devs[0]);
    }
    HostBatch b;
    b.n = n;
    b.in = (const void *const *)in; b.out = (void *const *)out;
    b.in_stride = in_stride; b.out_stride = out_stride;
    b.in_row = (size_t)c.w * 4; b.out_row = (size_t)c.fw * 4;
    b.in_rows = c.h; b.out_rows = c.fh;
    b.in_img = align256(b.in_row * c.h); b.out_img = align256(b.out_row * c.fh);
    b.acquire = [&](int dev, std::unique_lock<std::mutex> &l1, std::unique_lock<std::mutex> &l2, HostPipe **pipe) -> int {
        CallCtx ic;
        int r = call_contexts(c.mn, c.msc, dev, &ic, &l1, &l2);
        if (r) return r;
        *pipe = &ic.owner()->pipe;
        return W2XC_OK;
    };
    b.run = [&](int dev, int cnt, const void *din, void *dout, hipStream_t st, int max_sub) -> int {
        ImageCall d = c;   // (this device's share of the call: its contexts, locked by acquire, and the pipeline's stream)
        d.st = st;
        int r = call_contexts(c.mn, c.msc, dev, &d.ctx);
        if (r) return r;
        return process_rgba_device(R, d, cnt, max_sub, U8In{(const unsigned char *)din, b.in_img, b.in_row}, U8Out{(unsigned char *)dout, b.out_img, b.out_row});
    };
    return batch_host_run(b, c.o, R.sub);
}

// w2xc_bleed_rgba_u8_device has no model and so no context: its pass stamps (2 bytes per pixel, written before they are read) live in one buffer per device,
// kept like a context's buffers until w2xc_bleed_rgba_u8_trim releases them; the lock covers the enqueue, as a context's does.
struct BleedScratch {
    std::mutex mu;
    std::map<int, Scratch> stamp;
};
BleedScratch &bleed_scratch()
{
    static BleedScratch *b = new BleedScratch;   // (never destroyed: at exit the HIP runtime may be gone before a static's destructor runs)
    return *b;
}

// ---- the four forms of the image call, for Y models (rgb = false: w2xc_process_image_u8*) and RGB models (w2xc_process_image_rgb_u8*) ----
int image_ex_device(bool rgb, ImageCall c, U8In in, U8Out out)
{
    int rc = check_process_args(c, rgb);
    if (rc) return rc;
    if ((rc = check_image_args(c, in.p, in.row, out.p, out.row))) return rc;
    if (rgb) {
        // (the first layer may read the source while bands of the result are already written: the two must not share memory)
        int sub;
        if (ranges_overlap(in.p, image_extent(c.h, in.row, c.w, 3), out.p, image_extent(c.fh, out.row, c.fw, 3)))
            return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
        if ((rc = plan_image_call(PLAN_RGB, c, &sub))) return rc;
    }
    if (!rgb && c.tta && (rc = check_y_models(c))) return rc;
    LockedCtx lc;
    if ((rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    c.rows = true;
    return process_sub_batch(rgb, c, 1, 1, in, out);
}

int image_ex_host(bool rgb, ImageCall c, U8In in, U8Out out)
{
    int rc = check_process_args(c, rgb);
    if (rc) return rc;
    if ((rc = check_image_args(c, in.p, in.row, out.p, out.row))) return rc;
    int sub;
    if (rgb && (rc = plan_image_call(PLAN_RGB, c, &sub))) return rc;
    if (!rgb && c.tta && (rc = check_y_models(c))) return rc;
    if (w2xc_device_count() <= 0) return fail(W2XC_ERR_HIP, "no HIP device available (libw2xc_hip has no CPU fallback)");
    return image_host_single(rgb, c, in, out, c.o.device);
}

int image_batch_device(bool rgb, ImageCall c, int n, U8In in, U8Out out)
{
    int rc = check_image_batch_args(rgb, c, n, in.row, out.row);
    if (rc) return rc;
    if (!in.p || !out.p) return fail(W2XC_ERR_ARG, "null argument");
    const size_t in_ext = image_extent(c.h, in.row, c.w, 3), out_ext = image_extent(c.fh, out.row, c.fw, 3);
    if (n > 1 && out.img < out_ext)
        return fail(W2XC_ERR_ARG, "output images overlap each other (image stride %zu < %zu bytes)", out.img, out_ext);
    if (ranges_overlap(in.p, (size_t)(n - 1) * in.img + in_ext, out.p, (size_t)(n - 1) * out.img + out_ext))
        return fail(W2XC_ERR_ARG, "output images overlap the input images");
    int sub = 1;
    if ((rc = plan_image_call(rgb ? PLAN_RGB : PLAN_Y, c, &sub))) return rc;
    sub = std::min(sub, n);
    LockedCtx lc;
    if ((rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    for (int b0 = 0; b0 < n; b0 += sub) {
        rc = process_sub_batch(rgb, c, std::min(sub, n - b0), sub, U8In{in.p + (size_t)b0 * in.img, in.img, in.row},
                               U8Out{out.p + (size_t)b0 * out.img, out.img, out.row});
        if (rc) return rc;
    }
    return W2XC_OK;
}

int image_batch_host(bool rgb, ImageCall c, int n, const unsigned char *const *in, size_t in_stride, unsigned char *const *out, size_t out_stride)
{
    int rc = check_image_batch_args(rgb, c, n, in_stride, out_stride);
    if (rc) return rc;
    if (!in || !out) return fail(W2XC_ERR_ARG, "null argument");
    rc = check_batch_host_ptrs(n, (const void *const *)in, image_extent(c.h, in_stride, c.w, 3), (void *const *)out, image_extent(c.fh, out_stride, c.fw, 3));
    if (rc) return rc;
    int sub = 1;
    if ((rgb || n > 1) && (rc = plan_image_call(rgb ? PLAN_RGB : PLAN_Y, c, &sub))) return rc;
    if (n == 1) {   // nothing to overlap: the synchronous single-image sequence, on the first device of the mask
        std::vector<int> devs;
        if ((rc = host_devices(c.o, &devs))) return rc;
        return image_host_single(rgb, c, U8In{in[0], 0, in_stride}, U8Out{out[0], 0, out_stride}, devs[0]);
    }
    HostBatch b;
    b.n = n;
    b.in = (const void *const *)in; b.out = (void *const *)out;
    b.in_stride = in_stride; b.out_stride = out_stride;
    b.in_row = (size_t)c.w * 3; b.out_row = (size_t)c.fw * 3;
    b.in_rows = c.h; b.out_rows = c.fh;
    b.in_img = align256(b.in_row * c.h); b.out_img = align256(b.out_row * c.fh);
    // both models' contexts, locked together for this device's share of the call; the pipeline is the owning context's
    b.acquire = [&](int dev, std::unique_lock<std::mutex> &l1, std::unique_lock<std::mutex> &l2, HostPipe **pipe) -> int {
        CallCtx ic;
        int r = call_contexts(c.mn, c.msc, dev, &ic, &l1, &l2);
        if (r) return r;
        *pipe = &ic.owner()->pipe;
        return W2XC_OK;
    };
    b.run = [&](int dev, int cnt, const void *din, void *dout, hipStream_t st, int max_sub) -> int {
        ImageCall d = c;   // (this device's share of the call: its contexts, locked by acquire, and the pipeline's stream)
        d.st = st;
        int r = call_contexts(c.mn, c.msc, dev, &d.ctx);
        if (r) return r;
        return process_sub_batch(rgb, d, cnt, max_sub, U8In{(const unsigned char *)din, b.in_img, b.in_row}, U8Out{(unsigned char *)dout, b.out_img, b.out_row});
    };
    return batch_host_run(b, c.o, sub);
}

// ---- YUV frames (w2xc_process_frames_yuv_u8*; the arithmetic: include/w2xc_hip.h) ----
// Luma through the models as the planes of run_batch, chroma from bytes to bytes in one launch: no colour matrix, no float plane of chroma.
struct YuvGeom {
    int chroma, range;
    bool rgb = false;       // the frames go through RGB / head models (w2xc_process_frames_yuv_u8_rgb*): process_yuv_rgb_device
    int matrix = 0;         // ... by this colour matrix (W2XC_MATRIX_*)
    int cw = 0, ch = 0;     // the chroma planes of a w x h frame (0 x 0: W2XC_YUV_400)
    int ocw = 0, och = 0;   // ... of the call's output frame
    int W = 0, H = 0;       // the output frame
};
size_t chroma_row_bytes(int cw, int px) { return (size_t)px * (cw - 1) + 1; }
// the float planes of one frame: two luma planes per level
size_t yuv_aux_floats(int w, int h, int iterations) { return 2 * plane_floats(w, h) + (iterations ? 2 * plane_floats(2 * w, 2 * h) : 0); }
// the bytes of one frame's planes: w x h luma, two planes of cw x ch chroma
size_t yuv_frame_bytes(int w, int h, int cw, int ch) { return (size_t)w * h + 2 * (size_t)cw * ch; }

// one side's planes from frame b0 on
w2xc_yuv_planes yuv_from(const w2xc_yuv_planes &s, size_t b0, bool chroma)
{
    w2xc_yuv_planes t = s;
    t.y += b0 * s.y_frame_stride;
    if (chroma) { t.u += b0 * s.c_frame_stride; t.v += b0 * s.c_frame_stride; }
    return t;
}

// n frames of w x h luma and cw x ch chroma on one side: pointers, strides, c_px; its byte ranges go to iv tagged `tag` (check_batch_overlap)
int check_yuv_side(const w2xc_yuv_planes *s, int n, int w, int h, int cw, int ch, int tag, std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> &iv)
{
    if (!s || !s->y) return fail(W2XC_ERR_ARG, "null argument");
    const size_t y_ext = image_extent(h, s->y_stride, w, 1);
    if (s->y_stride < (size_t)w || (n > 1 && s->y_frame_stride < y_ext)) return fail(W2XC_ERR_ARG, "luma: row stride below the row's bytes / frame stride below a plane");
    for (int i = 0; i < n; i++) iv.push_back({{(uintptr_t)s->y + i * s->y_frame_stride, (uintptr_t)s->y + i * s->y_frame_stride + y_ext}, tag});
    if (!cw) return W2XC_OK;
    if (!s->u || !s->v) return fail(W2XC_ERR_ARG, "null argument");
    if (s->c_px != 1 && s->c_px != 2) return fail(W2XC_ERR_ARG, "c_px must be 1 (planar) or 2 (interleaved), got %d", s->c_px);
    const size_t row = chroma_row_bytes(cw, s->c_px), c_ext = (size_t)(ch - 1) * s->c_stride + row;
    if (s->c_stride < row || (n > 1 && s->c_frame_stride < c_ext)) return fail(W2XC_ERR_ARG, "chroma: row stride below the row's bytes / frame stride below a plane");
    // two interleaved planes (NV12: v = u + 1) are one range of bytes, two planes otherwise
    const uintptr_t u = (uintptr_t)s->u, v = (uintptr_t)s->v;
    const bool pair = s->c_px == 2 && (v == u + 1 || u == v + 1);
    for (int i = 0; i < n; i++) {
        const uintptr_t off = i * s->c_frame_stride;
        if (pair) iv.push_back({{std::min(u, v) + off, std::min(u, v) + off + c_ext + 1}, tag});
        else { iv.push_back({{u + off, u + off + c_ext}, tag}); iv.push_back({{v + off, v + off + c_ext}, tag}); }
    }
    return W2XC_OK;
}

// the float planes of one frame on the RGB route: three per level, the noise pass's output included
size_t yuv_rgb_aux_floats(const ImageCall &c)
{
    return 3 * ((c.mn ? 2 : 1) * plane_floats(c.w, c.h) + (c.iterations ? plane_floats(2 * c.w, 2 * c.h) : 0));
}

// the precisions of the RGB route: those w2xc_convert_planes[_up2x]_batch_device take (the models' plane form is plan_image_call's check)
int check_yuv_rgb_precision(const ImageCall &c)
{
    if (c.o.precision != W2XC_PRECISION_FP32 && split_terms(c.o) == 0)
        return fail(W2XC_ERR_UNSUPPORTED, "w2xc_process_frames_yuv_u8_rgb* supports W2XC_PRECISION_FP32 / BF16X2 / BF16X3 / FP16X2");
    if (c.iterations > 0 && c.msc && c.msc->has_head() && c.o.precision != W2XC_PRECISION_FP32)
        return fail(W2XC_ERR_UNSUPPORTED, "16-bit precision modes: not available for a model with an upconv head (W2XC_PRECISION_FP32 only)");
    return W2XC_OK;
}

// everything both forms refuse, before a device is touched; *g = the geometry, *sub = frames per sub-batch.  rgb: the call is w2xc_process_frames_yuv_u8_rgb*
// -- RGB models, or an upconv head model as scale model, and a colour matrix; a grey frame (W2XC_YUV_400) belongs to the Y call
int check_yuv_call(ImageCall &c, bool rgb, int n, int chroma, int range, int matrix, const w2xc_yuv_planes *in, const w2xc_yuv_planes *out, YuvGeom *g, int *sub)
{
    int rc = check_process_args(c, rgb);
    if (rc || (rc = rgb ? check_yuv_rgb_precision(c) : check_y_models(c))) return rc;
    if (c.iterations < 0 || c.iterations > 1) return fail(W2XC_ERR_ARG, "iterations must be 0 or 1 (got %d)", c.iterations);
    if (n < 1 || n > (1 << 20)) return fail(W2XC_ERR_ARG, "batch of %d frames", n);
    if (c.w <= 0 || c.h <= 0 || c.w > (1 << 22) || c.h > (1 << 22)) return fail(W2XC_ERR_ARG, "bad frame size");
    if (chroma < W2XC_YUV_420 || chroma > W2XC_YUV_400) return fail(W2XC_ERR_ARG, "unknown chroma layout %d", chroma);
    if (range != W2XC_RANGE_FULL && range != W2XC_RANGE_LIMITED) return fail(W2XC_ERR_ARG, "unknown range %d", range);
    if (rgb && chroma == W2XC_YUV_400) return fail(W2XC_ERR_ARG, "a frame without chroma (W2XC_YUV_400) belongs to w2xc_process_frames_yuv_u8*");
    if (rgb && (matrix < W2XC_MATRIX_BT601 || matrix > W2XC_MATRIX_BT2020)) return fail(W2XC_ERR_ARG, "unknown colour matrix %d", matrix);
    g->chroma = chroma; g->range = range; g->rgb = rgb; g->matrix = matrix;
    g->W = c.w << c.iterations; g->H = c.h << c.iterations;
    if (chroma != W2XC_YUV_400) {
        const bool half_x = chroma != W2XC_YUV_444, half_y = chroma == W2XC_YUV_420;
        g->cw = half_x ? (c.w + 1) / 2 : c.w;     g->ch = half_y ? (c.h + 1) / 2 : c.h;
        g->ocw = half_x ? (g->W + 1) / 2 : g->W;  g->och = half_y ? (g->H + 1) / 2 : g->H;
    }
    std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> iv;
    if ((rc = check_yuv_side(in, n, c.w, c.h, g->cw, g->ch, 0, iv)) || (rc = check_yuv_side(out, n, g->W, g->H, g->ocw, g->och, 1, iv))) return rc;
    if ((rc = check_batch_overlap(iv))) return rc;
    c.fw = g->W; c.fh = g->H;
    const size_t per = (rgb ? yuv_rgb_aux_floats(c) : yuv_aux_floats(c.w, c.h, c.iterations)) * sizeof(float) + yuv_frame_bytes(c.w, c.h, g->cw, g->ch) +
                       yuv_frame_bytes(g->W, g->H, g->ocw, g->och);
    return plan_image_call(rgb ? PLAN_RGB : PLAN_Y, c, sub, per, 1, "w2xc_process_frames_yuv_u8_rgb*");
}

W2xcU8Planes chroma_planes(const w2xc_yuv_planes &s) { return {s.u, (long long)s.c_frame_stride, (long long)s.c_stride, s.c_px}; }

// A sub-batch of S frames (S <= cap, the call's sub-batch size: the planes are sized by cap): luma bytes -> planes, the noise pass, the scale pass with the
// nearest-2x folded into layer 1 -- run_batch, so bands, precisions, named kernels and fusion settings are those of w2xc_convert_batch_device --, planes ->
// luma bytes; chroma in ONE launch, bytes to bytes.
int process_yuv_device(const ImageCall &c, const YuvGeom &g, int S, int cap, const w2xc_yuv_planes &in, const w2xc_yuv_planes &out)
{
    DevCtx *own = c.ctx.owner();
    if (int rc = reserve_aux(own, 0, yuv_aux_floats(c.w, c.h, c.iterations) * (size_t)cap)) return rc;
    float *base = aux_planes(own, 0);
    long long ps = (long long)plane_floats(c.w, c.h);
    float *y = base, *yn = y + (size_t)cap * ps;
    base += 2 * (size_t)cap * ps;
    HIP_TRY(w2xc_launch_y8_to_plane({in.y, (long long)in.y_frame_stride, (long long)in.y_stride, 1}, c.w, c.h, g.range, y, ps, S, c.st));
    if (c.mn) {
        if (int rc = run_batch(c.mn, c.ctx.cn, S, 0, {y, (size_t)c.w, ps}, c.w, c.h, {yn, (size_t)c.w, ps}, c.st, c.o)) return rc;
        y = yn;
    }
    if (c.iterations) {
        const long long ps2 = (long long)plane_floats(g.W, g.H);
        if (int rc = run_batch(c.msc, c.ctx.cs, S, 1, {y, (size_t)c.w, ps}, c.w, c.h, {base, (size_t)g.W, ps2}, c.st, c.o)) return rc;
        y = base; ps = ps2;
    }
    HIP_TRY(w2xc_launch_plane_to_y8(y, ps, g.W, g.H, g.range, {out.y, (long long)out.y_frame_stride, (long long)out.y_stride, 1}, S, c.st));
    if (!g.cw) return W2XC_OK;
    if (c.iterations) HIP_TRY(w2xc_launch_chroma2x_u8(chroma_planes(in), in.v, g.cw, g.ch, chroma_planes(out), out.v, g.ocw, g.och, S, c.st));
    else HIP_TRY(w2xc_launch_chroma_copy_u8(chroma_planes(in), in.v, g.cw, g.ch, chroma_planes(out), out.v, S, c.st));
    return W2XC_OK;
}

// YUV frames through RGB models, a sub-batch of S frames: ONE launch from the frames' bytes to three float planes per frame (k_yuv8_to_rgb), the passes of
// process_rgb_device with float planes at both ends (rgb_passes: S >= 2 one run_batch_planes per pass, S = 1 run_rows, so bands work; a head model's pass
// enlarges by itself), ONE launch from the planes to the bytes of the output frames (k_rgb_to_yuv8).
int process_yuv_rgb_device(const ImageCall &c, const YuvGeom &g, int S, int cap, const w2xc_yuv_planes &in, const w2xc_yuv_planes &out)
{
    DevCtx *own = c.ctx.owner();
    RgbPlan R;   // (float planes at both ends: no layer takes a uint8 image)
    R.floats = yuv_rgb_aux_floats(c);
    if (int rc = reserve_aux(own, 0, R.floats * (size_t)cap)) return rc;
    float *base = aux_planes(own, 0);
    RgbLevel L = {base, c.w, c.h, (long long)plane_floats(c.w, c.h)};
    base += 3 * (size_t)cap * L.ps;
    HIP_TRY(w2xc_launch_yuv8_to_rgb({in.y, (long long)in.y_frame_stride, (long long)in.y_stride, 1}, chroma_planes(in), in.v, c.w, c.h, g.chroma, g.range, g.matrix,
                                    L.p, 3 * L.ps, L.ps, S, c.st));
    if (int rc = rgb_passes(c, R, S, cap, U8In{nullptr, 0, 0}, U8Out{nullptr, 0, 0}, 0, &base, nullptr, &L)) return rc;
    HIP_TRY(w2xc_launch_rgb_to_yuv8(L.p, 3 * L.ps, L.ps, L.w, L.h, g.chroma, g.range, g.matrix, {out.y, (long long)out.y_frame_stride, (long long)out.y_stride, 1},
                                    chroma_planes(out), out.v, S, c.st));
    return W2XC_OK;
}

int process_yuv_sub_batch(const ImageCall &c, const YuvGeom &g, int S, int cap, const w2xc_yuv_planes &in, const w2xc_yuv_planes &out)
{
    return g.rgb ? process_yuv_rgb_device(c, g, S, cap, in, out) : process_yuv_device(c, g, S, cap, in, out);
}

// rgb: w2xc_process_frames_yuv_u8_rgb* (RGB and head models by the colour matrix `matrix`); otherwise the Y call, which has no matrix
int frames_yuv_device(ImageCall c, bool rgb, int n, int chroma, int range, int matrix, const w2xc_yuv_planes *in, const w2xc_yuv_planes *out)
{
    YuvGeom g;
    int sub = 1;
    int rc = check_yuv_call(c, rgb, n, chroma, range, matrix, in, out, &g, &sub);
    if (rc) return rc;
    sub = std::min(sub, n);
    LockedCtx lc;
    if ((rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    for (int b0 = 0; b0 < n; b0 += sub)
        if ((rc = process_yuv_sub_batch(c, g, std::min(sub, n - b0), sub, yuv_from(*in, b0, g.cw != 0), yuv_from(*out, b0, g.cw != 0)))) return rc;
    return W2XC_OK;
}

// The device copy of one side of a host call for sub-batches of at most cap frames, at `at` in the image buffer: luma rows w bytes apart; chroma as the caller
// has it -- planar planes, or the two interleaved planes as one plane of 2 cw-byte rows --, every frame on a 256-byte boundary.  *bytes = what it takes.
struct YuvMirror {
    w2xc_yuv_planes d;
    size_t c_copy_row = 0;   // bytes of a chroma row the copies move (both interleaved planes at once)
    bool pair = false;
};
YuvMirror yuv_mirror(const w2xc_yuv_planes &host, unsigned char *at, int cap, int w, int h, int cw, int ch, size_t *bytes)
{
    YuvMirror m;
    m.d = host;
    m.d.y = at;
    m.d.y_stride = (size_t)w;
    m.d.y_frame_stride = align256((size_t)w * h);
    size_t used = m.d.y_frame_stride * cap;
    if (cw) {
        m.pair = host.c_px == 2;
        m.c_copy_row = m.pair ? 2 * (size_t)cw : (size_t)cw;
        m.d.c_stride = m.c_copy_row;
        const size_t plane = align256(m.c_copy_row * ch);
        m.d.c_frame_stride = m.pair ? plane : 2 * plane;
        unsigned char *c0 = at + used;
        if (m.pair) { m.d.u = c0 + (host.u < host.v ? 0 : 1); m.d.v = c0 + (host.u < host.v ? 1 : 0); }
        else { m.d.u = c0; m.d.v = c0 + plane; }
        used += m.d.c_frame_stride * cap;
    }
    *bytes = used;
    return m;
}
// frames [b0, b0 + S) of the host side <-> the mirror's first S frames, blocking
int yuv_copy(const YuvMirror &m, const w2xc_yuv_planes &host, size_t b0, int S, int w, int h, int ch, bool upload)
{
    const hipMemcpyKind kind = upload ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    const auto copy = [&](unsigned char *dev, size_t dev_row, unsigned char *hst, size_t hst_row, size_t row, int rows) {
        return upload ? hipMemcpy2D(dev, dev_row, hst, hst_row, row, rows, kind) : hipMemcpy2D(hst, hst_row, dev, dev_row, row, rows, kind);
    };
    for (int i = 0; i < S; i++) {
        HIP_TRY(copy(m.d.y + i * m.d.y_frame_stride, m.d.y_stride, host.y + (b0 + i) * host.y_frame_stride, host.y_stride, (size_t)w, h));
        if (!m.c_copy_row) continue;
        const size_t hoff = (b0 + i) * host.c_frame_stride, doff = i * m.d.c_frame_stride;
        if (m.pair) HIP_TRY(copy(std::min(m.d.u, m.d.v) + doff, m.d.c_stride, std::min(host.u, host.v) + hoff, host.c_stride, m.c_copy_row, ch));
        else {
            HIP_TRY(copy(m.d.u + doff, m.d.c_stride, host.u + hoff, host.c_stride, m.c_copy_row, ch));
            HIP_TRY(copy(m.d.v + doff, m.d.c_stride, host.v + hoff, host.c_stride, m.c_copy_row, ch));
        }
    }
    return W2XC_OK;
}

int frames_yuv_host(ImageCall c, bool rgb, int n, int chroma, int range, int matrix, const w2xc_yuv_planes *in, const w2xc_yuv_planes *out)
{
    YuvGeom g;
    int sub = 1;
    int rc = check_yuv_call(c, rgb, n, chroma, range, matrix, in, out, &g, &sub);
    if (rc) return rc;
    if (g.cw) for (const w2xc_yuv_planes *s : {in, out})
        if (s->c_px == 2 && s->v != s->u + 1 && s->u != s->v + 1)
            return fail(W2XC_ERR_ARG, "host planes with c_px = 2: the two chroma planes must interleave (NV12: v = u + 1; NV21: u = v + 1)");
    sub = std::min(sub, n);
    std::vector<int> devs;
    if ((rc = host_devices(c.o, &devs))) return rc;
    LockedCtx lc;
    if ((rc = lc.open(c.mn, c.msc, devs[0]))) return rc;
    c.ctx = lc;
    c.st = nullptr;
    DevCtx *own = c.ctx.owner();
    size_t in_bytes = 0, out_bytes = 0;
    yuv_mirror(*in, nullptr, sub, c.w, c.h, g.cw, g.ch, &in_bytes);
    yuv_mirror(*out, nullptr, sub, g.W, g.H, g.ocw, g.och, &out_bytes);
    if ((rc = own->img_io.reserve(in_bytes + out_bytes, "the frames"))) return rc;
    unsigned char *dev = own->img_io.as<unsigned char>();
    const YuvMirror mi = yuv_mirror(*in, dev, sub, c.w, c.h, g.cw, g.ch, &in_bytes), mo = yuv_mirror(*out, dev + in_bytes, sub, g.W, g.H, g.ocw, g.och, &out_bytes);
    for (int b0 = 0; b0 < n; b0 += sub) {
        const int S = std::min(sub, n - b0);
        if ((rc = yuv_copy(mi, *in, b0, S, c.w, c.h, g.ch, true))) return rc;
        if ((rc = process_yuv_sub_batch(c, g, S, sub, mi.d, mo.d))) { hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipDeviceSynchronize());
        if ((rc = yuv_copy(mo, *out, b0, S, g.W, g.H, g.och, false))) return rc;
    }
    return W2XC_OK;
}

}  // namespace

}  // namespace w2xc_eng

using namespace w2xc_eng;

extern "C" {

int w2xc_process_image_u8_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                    int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                    void *hip_stream, const w2xc_opts *opts, int tta)
try {
    return image_ex_device(false, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts, tta), U8In{d_in, 0, in_stride_bytes},
                           U8Out{d_out, 0, out_stride_bytes});
} W2XC_CATCH_ALL

int w2xc_process_image_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                    int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                    void *hip_stream, const w2xc_opts *opts)
{
    return w2xc_process_image_u8_tta_device(noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, hip_stream, opts, 0);
}

int w2xc_process_image_u8_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                 int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, void *hip_stream,
                                 const w2xc_opts *opts)
{
    return w2xc_process_image_u8_ex_device(noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, 0.0,
                                           hip_stream, opts);
}

int w2xc_process_image_u8_tta(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                             unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts, int tta)
try {
    return image_ex_host(false, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts, tta), U8In{in, 0, in_stride_bytes},
                         U8Out{out, 0, out_stride_bytes});
} W2XC_CATCH_ALL

int w2xc_process_image_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                             unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
{
    return w2xc_process_image_u8_tta(noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts, 0);
}

int w2xc_process_image_u8(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                          unsigned char *out, size_t out_stride_bytes, int iterations, const w2xc_opts *opts)
{
    return w2xc_process_image_u8_ex(noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, 0.0, opts);
}

// ---- batches of same-size images ----------------------------------------------------------------
int w2xc_process_image_u8_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                       size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes,
                                       size_t out_stride_bytes, int iterations, double shrink_ratio, void *hip_stream, const w2xc_opts *opts, int tta)
try {
    return image_batch_device(false, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts, tta), n,
                              U8In{d_in, in_image_stride_bytes, in_stride_bytes}, U8Out{d_out, out_image_stride_bytes, out_stride_bytes});
} W2XC_CATCH_ALL

int w2xc_process_image_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                       size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes,
                                       size_t out_stride_bytes, int iterations, double shrink_ratio, void *hip_stream, const w2xc_opts *opts)
{
    return w2xc_process_image_u8_batch_tta_device(noise_model, scale_model, n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes, out_stride_bytes, iterations, shrink_ratio, hip_stream, opts, 0);
}

int w2xc_process_image_u8_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts, int tta)
try {
    return image_batch_host(false, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts, tta), n, in, in_stride_bytes, out,
                            out_stride_bytes);
} W2XC_CATCH_ALL

int w2xc_process_image_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
{
    return w2xc_process_image_u8_batch_tta(noise_model, scale_model, n, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts, 0);
}

// ---- RGB models: the same four forms ---------------------------------------------------------------
int w2xc_process_image_rgb_u8_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                        int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                        void *hip_stream, const w2xc_opts *opts, int tta)
try {
    return image_ex_device(true, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts, tta), U8In{d_in, 0, in_stride_bytes},
                           U8Out{d_out, 0, out_stride_bytes});
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                        int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                        void *hip_stream, const w2xc_opts *opts)
{
    return w2xc_process_image_rgb_u8_tta_device(noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, hip_stream, opts, 0);
}

int w2xc_process_image_rgb_u8_tta(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                 unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts, int tta)
try {
    return image_ex_host(true, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts, tta), U8In{in, 0, in_stride_bytes},
                         U8Out{out, 0, out_stride_bytes});
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                 unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
{
    return w2xc_process_image_rgb_u8_tta(noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts, 0);
}

int w2xc_process_image_rgb_u8_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                           size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                           size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                           void *hip_stream, const w2xc_opts *opts, int tta)
try {
    return image_batch_device(true, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts, tta), n,
                              U8In{d_in, in_image_stride_bytes, in_stride_bytes}, U8Out{d_out, out_image_stride_bytes, out_stride_bytes});
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                           size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                           size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                           void *hip_stream, const w2xc_opts *opts)
{
    return w2xc_process_image_rgb_u8_batch_tta_device(noise_model, scale_model, n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes, out_stride_bytes, iterations, shrink_ratio, hip_stream, opts, 0);
}

int w2xc_process_image_rgb_u8_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                    int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                    const w2xc_opts *opts, int tta)
try {
    return image_batch_host(true, ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts, tta), n, in, in_stride_bytes, out,
                            out_stride_bytes);
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                    int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                    const w2xc_opts *opts)
{
    return w2xc_process_image_rgb_u8_batch_tta(noise_model, scale_model, n, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts, 0);
}

// ---- upconv head models as scale model: the batch forms, with and without TTA (n = 1 with tta = 1: the single-image TTA form) ----
int w2xc_process_image_rgb_u8_up2x_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                                size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                                size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                                void *hip_stream, const w2xc_opts *opts, int tta)
try {
    ImageCall c(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts, tta);
    c.up2x = true;
    return image_batch_device(true, c, n, U8In{d_in, in_image_stride_bytes, in_stride_bytes}, U8Out{d_out, out_image_stride_bytes, out_stride_bytes});
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_up2x_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                         int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                         const w2xc_opts *opts, int tta)
try {
    ImageCall c(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts, tta);
    c.up2x = true;
    return image_batch_host(true, c, n, in, in_stride_bytes, out, out_stride_bytes);
} W2XC_CATCH_ALL

// ---- RGBA images: alpha through the scale model, colour bled under the transparent pixels ----------
int w2xc_process_image_rgba_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w, int h,
                                         unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                         void *hip_stream, const w2xc_opts *opts)
try {
    return rgba_ex_device(ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts), U8In{d_in, 0, in_stride_bytes},
                          U8Out{d_out, 0, out_stride_bytes}, bleed_passes);
} W2XC_CATCH_ALL

int w2xc_process_image_rgba_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                  unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes, const w2xc_opts *opts)
try {
    return rgba_ex_host(ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts), U8In{in, 0, in_stride_bytes},
                        U8Out{out, 0, out_stride_bytes}, bleed_passes);
} W2XC_CATCH_ALL

int w2xc_process_image_rgba_u8_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                                size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes, size_t out_stride_bytes,
                                                int iterations, double shrink_ratio, int bleed_passes, void *hip_stream, const w2xc_opts *opts, int tta)
try {
    return rgba_batch_device(ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts, tta), n,
                             U8In{d_in, in_image_stride_bytes, in_stride_bytes}, U8Out{d_out, out_image_stride_bytes, out_stride_bytes}, bleed_passes);
} W2XC_CATCH_ALL

int w2xc_process_image_rgba_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                            size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes, size_t out_stride_bytes,
                                            int iterations, double shrink_ratio, int bleed_passes, void *hip_stream, const w2xc_opts *opts)
{
    return w2xc_process_image_rgba_u8_batch_tta_device(noise_model, scale_model, n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes,
                                                       out_stride_bytes, iterations, shrink_ratio, bleed_passes, hip_stream, opts, 0);
}

int w2xc_process_image_rgba_u8_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                         int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                         const w2xc_opts *opts, int tta)
try {
    return rgba_batch_host(ImageCall(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts, tta), n, in, in_stride_bytes, out, out_stride_bytes,
                           bleed_passes);
} W2XC_CATCH_ALL

int w2xc_process_image_rgba_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w, int h,
                                     unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                     const w2xc_opts *opts)
{
    return w2xc_process_image_rgba_u8_batch_tta(noise_model, scale_model, n, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, bleed_passes,
                                                opts, 0);
}

// ---- ... with an upconv head model as scale model (n = 1: the single-image form, bands included) ----
int w2xc_process_image_rgba_u8_up2x_batch_tta_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                                     size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                                     size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                                     int bleed_passes, void *hip_stream, const w2xc_opts *opts, int tta)
try {
    ImageCall c(noise_model, scale_model, w, h, iterations, shrink_ratio, hip_stream, opts, tta);
    c.up2x = true;
    return rgba_batch_device(c, n, U8In{d_in, in_image_stride_bytes, in_stride_bytes}, U8Out{d_out, out_image_stride_bytes, out_stride_bytes}, bleed_passes);
} W2XC_CATCH_ALL

int w2xc_process_image_rgba_u8_up2x_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                                 size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes,
                                                 size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes, void *hip_stream,
                                                 const w2xc_opts *opts)
{
    return w2xc_process_image_rgba_u8_up2x_batch_tta_device(noise_model, scale_model, n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out,
                                                            out_image_stride_bytes, out_stride_bytes, iterations, shrink_ratio, bleed_passes, hip_stream, opts, 0);
}

int w2xc_process_image_rgba_u8_up2x_batch_tta(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                              int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                              int bleed_passes, const w2xc_opts *opts, int tta)
try {
    ImageCall c(noise_model, scale_model, w, h, iterations, shrink_ratio, nullptr, opts, tta);
    c.up2x = true;
    return rgba_batch_host(c, n, in, in_stride_bytes, out, out_stride_bytes, bleed_passes);
} W2XC_CATCH_ALL

int w2xc_process_image_rgba_u8_up2x_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                          int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                          const w2xc_opts *opts)
{
    return w2xc_process_image_rgba_u8_up2x_batch_tta(noise_model, scale_model, n, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio,
                                                     bleed_passes, opts, 0);
}

// ---- YUV frames: luma through the models, chroma 2x on bytes ----
int w2xc_process_frames_yuv_u8_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *d_in,
                                      const w2xc_yuv_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts)
try {
    return frames_yuv_device(ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), false, n, chroma, range, 0, d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u8(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *in,
                               const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv_host(ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), false, n, chroma, range, 0, in, out);
} W2XC_CATCH_ALL

// ---- YUV frames through RGB and head models, by a colour matrix ----
int w2xc_process_frames_yuv_u8_rgb_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                          const w2xc_yuv_planes *d_in, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts)
try {
    return frames_yuv_device(ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), true, n, chroma, range, matrix, d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u8_rgb(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix, const w2xc_yuv_planes *in,
                                   const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv_host(ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), true, n, chroma, range, matrix, in, out);
} W2XC_CATCH_ALL

// what the two blocks refuse: the frames' side as check_yuv_side refuses it, the 3 n float planes, and the two sides overlapping
static int check_yuv_rgb_block_args(const w2xc_yuv_planes *f, bool f_is_out, int n, int w, int h, int chroma, int range, int matrix, const float *rgb,
                                    size_t image_stride_bytes, size_t plane_stride_bytes)
{
    if (!f || !rgb) return fail(W2XC_ERR_ARG, "null argument");
    if (n < 1 || n > (1 << 20) || w <= 0 || h <= 0 || w > (1 << 22) || h > (1 << 22)) return fail(W2XC_ERR_ARG, "bad frame count / frame size");
    if (chroma == W2XC_YUV_400) return fail(W2XC_ERR_ARG, "a frame without chroma (W2XC_YUV_400) has no colour to convert");
    if (chroma < W2XC_YUV_420 || chroma > W2XC_YUV_444) return fail(W2XC_ERR_ARG, "unknown chroma layout %d", chroma);
    if (range != W2XC_RANGE_FULL && range != W2XC_RANGE_LIMITED) return fail(W2XC_ERR_ARG, "unknown range %d", range);
    if (matrix < W2XC_MATRIX_BT601 || matrix > W2XC_MATRIX_BT2020) return fail(W2XC_ERR_ARG, "unknown colour matrix %d", matrix);
    const size_t plane = (size_t)4 * w * h;
    if ((image_stride_bytes & 3) || (plane_stride_bytes & 3) || plane_stride_bytes < plane || (n > 1 && image_stride_bytes < 2 * plane_stride_bytes + plane))
        return fail(W2XC_ERR_ARG, "plane / image strides: multiples of 4, a plane stride of at least a plane, an image stride of at least three planes");
    const int cw = chroma != W2XC_YUV_444 ? (w + 1) / 2 : w, ch = chroma == W2XC_YUV_420 ? (h + 1) / 2 : h;
    std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> iv;
    if (int rc = check_yuv_side(f, n, w, h, cw, ch, f_is_out ? 1 : 0, iv)) return rc;
    for (int i = 0; i < n; i++) for (int p = 0; p < 3; p++) {
        const uintptr_t at = (uintptr_t)rgb + i * image_stride_bytes + p * plane_stride_bytes;
        iv.push_back({{at, at + plane}, f_is_out ? 0 : 1});
    }
    return check_batch_overlap(iv);
}

int w2xc_yuv8_to_rgb_device(const w2xc_yuv_planes *d_src, int n, int w, int h, int chroma, int range, int matrix, float *d_rgb, size_t image_stride_bytes,
                            size_t plane_stride_bytes, void *hip_stream)
try {
    if (int rc = check_yuv_rgb_block_args(d_src, false, n, w, h, chroma, range, matrix, d_rgb, image_stride_bytes, plane_stride_bytes)) return rc;
    HIP_TRY(w2xc_launch_yuv8_to_rgb({d_src->y, (long long)d_src->y_frame_stride, (long long)d_src->y_stride, 1}, chroma_planes(*d_src), d_src->v, w, h, chroma, range,
                                    matrix, d_rgb, (long long)(image_stride_bytes / 4), (long long)(plane_stride_bytes / 4), n, (hipStream_t)hip_stream));
    return W2XC_OK;
} W2XC_CATCH_ALL

int w2xc_rgb_to_yuv8_device(const float *d_rgb, size_t image_stride_bytes, size_t plane_stride_bytes, int n, int w, int h, int chroma, int range, int matrix,
                            const w2xc_yuv_planes *d_dst, void *hip_stream)
try {
    if (int rc = check_yuv_rgb_block_args(d_dst, true, n, w, h, chroma, range, matrix, d_rgb, image_stride_bytes, plane_stride_bytes)) return rc;
    HIP_TRY(w2xc_launch_rgb_to_yuv8(d_rgb, (long long)(image_stride_bytes / 4), (long long)(plane_stride_bytes / 4), w, h, chroma, range, matrix,
                                    {d_dst->y, (long long)d_dst->y_frame_stride, (long long)d_dst->y_stride, 1}, chroma_planes(*d_dst), d_dst->v, n,
                                    (hipStream_t)hip_stream));
    return W2XC_OK;
} W2XC_CATCH_ALL

// what the three building blocks refuse: n byte planes of bw-byte rows x h at p and n planes of `other` bytes (rows / planes as given) on the other side
static int check_yuv_block_args(const void *p, size_t frame, size_t row, size_t row_bytes, int rows, int n, int w, int h, const void *q, size_t q_plane, size_t q_ext)
{
    if (!p || !q) return fail(W2XC_ERR_ARG, "null argument");
    if (n < 1 || n > (1 << 20) || w <= 0 || h <= 0 || w > (1 << 22) || h > (1 << 22)) return fail(W2XC_ERR_ARG, "bad plane count / plane size");
    const size_t ext = (size_t)(rows - 1) * row + row_bytes;
    if (row < row_bytes || (n > 1 && (frame < ext || q_plane < q_ext))) return fail(W2XC_ERR_ARG, "row / plane strides below a row / a plane");
    if (ranges_overlap(p, (size_t)(n - 1) * frame + ext, q, (size_t)(n - 1) * q_plane + q_ext)) return fail(W2XC_ERR_ARG, "source and destination overlap");
    return W2XC_OK;
}

int w2xc_y8_to_plane_device(const unsigned char *d_src, int n, size_t frame_stride_bytes, size_t stride_bytes, int w, int h, int range, float *d_dst,
                            size_t plane_stride_bytes, void *hip_stream)
{
    if (int rc = check_yuv_block_args(d_src, frame_stride_bytes, stride_bytes, (size_t)(w > 0 ? w : 1), h, n, w, h, d_dst, plane_stride_bytes, (size_t)4 * (w > 0 ? w : 1) * (h > 0 ? h : 1))) return rc;
    if ((plane_stride_bytes & 3) || (range != W2XC_RANGE_FULL && range != W2XC_RANGE_LIMITED)) return fail(W2XC_ERR_ARG, "plane stride no multiple of 4 / unknown range");
    HIP_TRY(w2xc_launch_y8_to_plane({const_cast<unsigned char *>(d_src), (long long)frame_stride_bytes, (long long)stride_bytes, 1}, w, h, range, d_dst,
                                    (long long)(plane_stride_bytes / 4), n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_plane_to_y8_device(const float *d_src, int n, size_t plane_stride_bytes, int w, int h, int range, unsigned char *d_dst, size_t frame_stride_bytes,
                            size_t stride_bytes, void *hip_stream)
{
    if (int rc = check_yuv_block_args(d_dst, frame_stride_bytes, stride_bytes, (size_t)(w > 0 ? w : 1), h, n, w, h, d_src, plane_stride_bytes, (size_t)4 * (w > 0 ? w : 1) * (h > 0 ? h : 1))) return rc;
    if ((plane_stride_bytes & 3) || (range != W2XC_RANGE_FULL && range != W2XC_RANGE_LIMITED)) return fail(W2XC_ERR_ARG, "plane stride no multiple of 4 / unknown range");
    HIP_TRY(w2xc_launch_plane_to_y8(d_src, (long long)(plane_stride_bytes / 4), w, h, range, {d_dst, (long long)frame_stride_bytes, (long long)stride_bytes, 1}, n,
                                    (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_chroma2x_u8_device(const unsigned char *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int cw, int ch,
                            unsigned char *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int ow, int oh, void *hip_stream)
{
    if ((src_px != 1 && src_px != 2) || (dst_px != 1 && dst_px != 2)) return fail(W2XC_ERR_ARG, "src_px / dst_px must be 1 or 2");
    if (ow < 1 || oh < 1 || ow > 2 * (long long)cw || oh > 2 * (long long)ch) return fail(W2XC_ERR_ARG, "the output size lies outside the 2x enlargement");
    const size_t drow = (size_t)dst_px * (ow - 1) + 1, dext = (size_t)(oh - 1) * dst_stride_bytes + drow;
    if (dst_stride_bytes < drow) return fail(W2XC_ERR_ARG, "row / plane strides below a row / a plane");
    if (int rc = check_yuv_block_args(d_src, src_frame_stride_bytes, src_stride_bytes, (size_t)src_px * ((cw > 0 ? cw : 1) - 1) + 1, ch, n, cw, ch, d_dst, dst_frame_stride_bytes, dext)) return rc;
    HIP_TRY(w2xc_launch_chroma2x_u8({const_cast<unsigned char *>(d_src), (long long)src_frame_stride_bytes, (long long)src_stride_bytes, src_px}, nullptr, cw, ch,
                                    {d_dst, (long long)dst_frame_stride_bytes, (long long)dst_stride_bytes, dst_px}, nullptr, ow, oh, n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_bleed_rgba_u8_device(const unsigned char *d_in, size_t in_stride_bytes, int w, int h, int passes, unsigned char *d_out_rgb, size_t out_stride_bytes,
                              void *hip_stream)
try {
    if (!d_in || !d_out_rgb || w <= 0 || h <= 0 || passes < 0 || in_stride_bytes < (size_t)w * 4 || out_stride_bytes < (size_t)w * 3)
        return fail(W2XC_ERR_ARG, "bad argument");
    if (ranges_overlap(d_in, image_extent(h, in_stride_bytes, w, 4), d_out_rgb, image_extent(h, out_stride_bytes, w, 3)))
        return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
    passes = std::min(passes, std::max(w, h) - 1);   // (no pixel is farther from an opaque one)
    if (passes > 65534) return fail(W2XC_ERR_ARG, "more than 65534 effective bleed passes");
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    BleedScratch &b = bleed_scratch();
    std::lock_guard<std::mutex> lk(b.mu);
    unsigned short *stamp = nullptr;   // (only the pass chain has stamps)
    if (w2xc_bleed_stamps(passes)) {
        Scratch &s = b.stamp[dev];
        if (int rc = s.reserve((size_t)w * 2 * h, "the bleed's pass stamps")) return rc;
        stamp = s.as<unsigned short>();
    }
    HIP_TRY(w2xc_launch_rgba_bleed(d_in, 0, in_stride_bytes, w, h, passes, d_out_rgb, 0, out_stride_bytes, stamp, 0, 1, (hipStream_t)hip_stream));
    return W2XC_OK;
} W2XC_CATCH_ALL

int w2xc_bleed_rgba_u8_trim(void)
try {
    BleedScratch &b = bleed_scratch();
    std::lock_guard<std::mutex> lk(b.mu);
    for (auto &kv : b.stamp) {
        if (!kv.second.bytes()) continue;
        DeviceGuard guard(kv.first);
        if (!guard.ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", kv.first);
        HIP_TRY(hipDeviceSynchronize());   // (a bleed on any stream may still use the stamps)
        kv.second.release();
    }
    return W2XC_OK;
} W2XC_CATCH_ALL

int w2xc_scale2x_image_u8_device(w2xc_model *m, const unsigned char *d_in, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                 size_t out_stride_bytes, int iterations, void *hip_stream, const w2xc_opts *opts)
{
    return w2xc_process_image_u8_device(nullptr, m, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, hip_stream, opts);
}

int w2xc_scale2x_image_u8(w2xc_model *m, const unsigned char *in, size_t in_stride_bytes, int w, int h, unsigned char *out,
                          size_t out_stride_bytes, int iterations, const w2xc_opts *opts)
{
    return w2xc_process_image_u8(nullptr, m, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, opts);
}

int w2xc_resize2x_cubic_device(const float *d_src, int w, int h, float *d_dst, void *hip_stream)
{
    if (!d_src || !d_dst || w <= 0 || h <= 0) return fail(W2XC_ERR_ARG, "bad argument");
    HIP_TRY(w2xc_launch_resize2x_cubic(d_src, w, h, d_dst, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_resize_linear_device(const float *d_src, int sw, int sh, float *d_dst, int dw, int dh, void *hip_stream)
{
    if (!d_src || !d_dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0) return fail(W2XC_ERR_ARG, "bad argument");
    HIP_TRY(w2xc_launch_resize_linear(d_src, sw, sh, d_dst, dw, dh, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_u8_to_yuv_device(const unsigned char *d_in, size_t in_stride_bytes, int w, int h, float *d_y, float *d_u, float *d_v, void *hip_stream)
{
    if (!d_in || !d_y || !d_u || !d_v || w <= 0 || h <= 0 || in_stride_bytes < (size_t)w * 3) return fail(W2XC_ERR_ARG, "bad argument");
    HIP_TRY(w2xc_launch_u8_to_yuv(d_in, in_stride_bytes, w, h, d_y, d_u, d_v, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_yuv_to_u8_device(const float *d_y, const float *d_u, const float *d_v, int w, int h, unsigned char *d_out, size_t out_stride_bytes,
                          void *hip_stream)
{
    if (!d_out || !d_y || !d_u || !d_v || w <= 0 || h <= 0 || out_stride_bytes < (size_t)w * 3) return fail(W2XC_ERR_ARG, "bad argument");
    HIP_TRY(w2xc_launch_yuv_to_u8(d_y, d_u, d_v, w, h, d_out, out_stride_bytes, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_u8_to_rgb_device(const unsigned char *d_in, size_t in_stride_bytes, int w, int h, float *d_c0, float *d_c1, float *d_c2, void *hip_stream)
{
    if (!d_in || !d_c0 || !d_c1 || !d_c2 || w <= 0 || h <= 0 || in_stride_bytes < (size_t)w * 3) return fail(W2XC_ERR_ARG, "bad argument");
    HIP_TRY(w2xc_launch_u8_to_rgb(d_in, in_stride_bytes, w, h, d_c0, d_c1, d_c2, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_rgb_to_u8_device(const float *d_c0, const float *d_c1, const float *d_c2, int w, int h, unsigned char *d_out, size_t out_stride_bytes,
                          void *hip_stream)
{
    if (!d_out || !d_c0 || !d_c1 || !d_c2 || w <= 0 || h <= 0 || out_stride_bytes < (size_t)w * 3) return fail(W2XC_ERR_ARG, "bad argument");
    HIP_TRY(w2xc_launch_rgb_to_u8(d_c0, d_c1, d_c2, w, h, d_out, out_stride_bytes, (hipStream_t)hip_stream));
    return W2XC_OK;
}

// ---- test-time augmentation: the plane calls and the two building blocks ------------------------------
int w2xc_convert_batch_tta_device(w2xc_model *m, int n, int nn2x, const float *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h,
                                  float *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    int rc = check_batch_device_args(m, n, nn2x, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes);
    if (rc) return rc;
    if (n > (1 << 24)) return fail(W2XC_ERR_ARG, "batch of %d planes under TTA", n);   // (8 n variant planes)
    const w2xc_opts o = resolve_opts(opts);
    LockedCtx lc;
    if ((rc = lc.open(nullptr, m, o.device))) return rc;
    if ((rc = reserve_aux(lc.cs, 0, tta_pass_floats(w, h, nn2x) * (size_t)n))) return rc;
    return tta_pass(TtaPass{m, lc.cs, nn2x, 1, 1, false}, n, {d_in, in_stride_bytes / 4, (long long)(in_plane_stride_bytes / 4)}, w, h,
                    {d_out, out_stride_bytes / 4, (long long)(out_plane_stride_bytes / 4)}, aux_planes(lc.cs, 0), (hipStream_t)hip_stream, o);
} W2XC_CATCH_ALL

int w2xc_convert_planes_tta_device(w2xc_model *m, int n_in_planes, int nn2x, const float *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w,
                                   int h, float *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    if (nn2x != 0 && nn2x != 1) return fail(W2XC_ERR_ARG, "nn2x must be 0 or 1");
    const w2xc_opts o = resolve_opts(opts);
    int rc = check_planes_args(m, nn2x, n_in_planes, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes, o);
    if (rc) return rc;
    if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    if (w > (1 << 28) || h > (1 << 28) || n_in_planes > (1 << 20)) return fail(W2XC_ERR_ARG, "plane too large / too many planes");
    // the plan of both orientations, for its errors (the plane count the model takes among them) before a device is touched
    for (int t = 0; t < 2; t++) {
        const int W = (t ? h : w) << nn2x, H = (t ? w : h) << nn2x;
        RowPlan P;
        if ((rc = plan_rows(m, o, W, H, 0, 0, H, H, n_in_planes, true, &P))) return rc;
    }
    const int nout = m->layers.back().nout;
    LockedCtx lc;
    if ((rc = lc.open(nullptr, m, o.device))) return rc;
    const size_t need = 8 * ((size_t)n_in_planes * plane_floats(w, h) + (size_t)nout * plane_floats(w << nn2x, h << nn2x));
    if ((rc = reserve_aux(lc.cs, 0, need))) return rc;
    return tta_pass(TtaPass{m, lc.cs, nn2x, n_in_planes, nout, true}, 1, {d_in, in_stride_bytes / 4, (long long)(in_plane_stride_bytes / 4)}, w, h,
                    {d_out, out_stride_bytes / 4, (long long)(out_plane_stride_bytes / 4)}, aux_planes(lc.cs, 0), (hipStream_t)hip_stream, o);
} W2XC_CATCH_ALL

// what both building blocks refuse: n planes of w x h at p (rows `row` bytes apart, planes `plane` bytes apart) and their 8 n variants at up / tr
static int check_tta_block_args(const void *p, size_t plane, size_t row, int n, int w, int h, const void *up, const void *tr, size_t variant)
{
    if (!p || !up || !tr) return fail(W2XC_ERR_ARG, "null argument");
    if (n < 1 || n > (1 << 24) || w <= 0 || h <= 0 || w > (1 << 29) || h > (1 << 29)) return fail(W2XC_ERR_ARG, "bad plane count / plane size");
    if (row < (size_t)w * 4 || (row & 3) || (plane & 3) || (variant & 3)) return fail(W2XC_ERR_ARG, "row strides must be multiples of 4 bytes and >= 4*width");
    if ((n > 1 && plane < (size_t)(h - 1) * row + (size_t)w * 4) || variant < (size_t)w * 4 * h) return fail(W2XC_ERR_ARG, "plane strides below one plane");
    const size_t group = 4 * (size_t)n * variant, ext = (size_t)(n - 1) * plane + (size_t)(h - 1) * row + (size_t)w * 4;
    if (ranges_overlap(up, group, tr, group) || ranges_overlap(p, ext, up, group) || ranges_overlap(p, ext, tr, group))
        return fail(W2XC_ERR_ARG, "the planes and the two groups of variant planes overlap");
    return W2XC_OK;
}

int w2xc_tta_spread_device(const float *d_src, int n, size_t src_plane_stride_bytes, size_t src_stride_bytes, int w, int h, float *d_up, float *d_tr,
                           size_t variant_plane_stride_bytes, void *hip_stream)
{
    if (int rc = check_tta_block_args(d_src, src_plane_stride_bytes, src_stride_bytes, n, w, h, d_up, d_tr, variant_plane_stride_bytes)) return rc;
    HIP_TRY(w2xc_launch_tta_spread(d_src, (long long)(src_plane_stride_bytes / 4), (long long)(src_stride_bytes / 4), w, h, d_up, d_tr,
                                   (long long)(variant_plane_stride_bytes / 4), n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_tta_gather_device(const float *d_up, const float *d_tr, size_t variant_plane_stride_bytes, int n, int w, int h, float *d_dst,
                           size_t dst_plane_stride_bytes, size_t dst_stride_bytes, void *hip_stream)
{
    if (int rc = check_tta_block_args(d_dst, dst_plane_stride_bytes, dst_stride_bytes, n, w, h, d_up, d_tr, variant_plane_stride_bytes)) return rc;
    HIP_TRY(w2xc_launch_tta_gather(d_up, d_tr, (long long)(variant_plane_stride_bytes / 4), w, h, d_dst, (long long)(dst_plane_stride_bytes / 4),
                                   (long long)(dst_stride_bytes / 4), n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

// ---- ... with the uint8 image at the outer side (w2xc_tta_u8.hip) ----
// what both refuse: n images of w x h pixels of px bytes at p (rows `row` bytes apart, images `img` bytes apart) and the 8 m variant planes at up / tr
static int check_tta_u8_block_args(const void *p, size_t img, size_t row, int px, int n, long long m, int w, int h, const void *up, const void *tr, size_t variant)
{
    if (!p || !up || !tr) return fail(W2XC_ERR_ARG, "null argument");
    if (px != 3 && px != 4) return fail(W2XC_ERR_ARG, "pixels of 3 or 4 bytes (got %d)", px);
    if (n < 1 || m < 1 || m > (1 << 24) || w <= 0 || h <= 0 || w > (1 << 29) || h > (1 << 29)) return fail(W2XC_ERR_ARG, "bad image count / image size");
    if (row < (size_t)w * px) return fail(W2XC_ERR_ARG, "row strides must be >= %d*width bytes", px);
    if (variant & 3) return fail(W2XC_ERR_ARG, "the variant plane stride must be a multiple of 4 bytes");
    const size_t ext = image_extent(h, row, w, px);
    if ((n > 1 && img < ext) || variant < (size_t)w * 4 * h) return fail(W2XC_ERR_ARG, "image / plane strides below one image / plane");
    const size_t group = 4 * (size_t)m * variant, all = (size_t)(n - 1) * img + ext;
    if (ranges_overlap(up, group, tr, group) || ranges_overlap(p, all, up, group) || ranges_overlap(p, all, tr, group))
        return fail(W2XC_ERR_ARG, "the images and the two groups of variant planes overlap");
    return W2XC_OK;
}

int w2xc_tta_spread_u8_device(const unsigned char *d_src, int n, size_t image_stride_bytes, size_t stride_bytes, int px_bytes, int ch0, int ch_step, int w, int h,
                              float *d_up, float *d_tr, size_t variant_plane_stride_bytes, void *hip_stream)
{
    if (int rc = check_tta_u8_block_args(d_src, image_stride_bytes, stride_bytes, px_bytes, n, 3ll * n, w, h, d_up, d_tr, variant_plane_stride_bytes)) return rc;
    if (ch0 < 0 || ch_step < 0 || ch0 + 2 * (long long)ch_step >= px_bytes) return fail(W2XC_ERR_ARG, "a selected byte lies outside the pixel");
    HIP_TRY(w2xc_launch_tta_spread_u8(d_src, image_stride_bytes, stride_bytes, px_bytes, ch0, ch_step, w, h, d_up, d_tr, (long long)(variant_plane_stride_bytes / 4),
                                      n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int w2xc_tta_gather_u8_device(const float *d_up, const float *d_tr, size_t variant_plane_stride_bytes, int n, int planes_per_image, int first_plane, int n_ch,
                              int w, int h, unsigned char *d_dst, size_t image_stride_bytes, size_t stride_bytes, int px_bytes, int byte0, void *hip_stream)
{
    if (planes_per_image < 1) return fail(W2XC_ERR_ARG, "bad plane count");
    if (int rc = check_tta_u8_block_args(d_dst, image_stride_bytes, stride_bytes, px_bytes, n, (long long)planes_per_image * n, w, h, d_up, d_tr,
                                         variant_plane_stride_bytes)) return rc;
    if (byte0 < 0 || n_ch < 1 || (long long)byte0 + n_ch > px_bytes) return fail(W2XC_ERR_ARG, "a selected byte lies outside the pixel");
    if (first_plane < 0 || (long long)first_plane + n_ch > planes_per_image) return fail(W2XC_ERR_ARG, "a selected plane lies outside the image's planes");
    HIP_TRY(w2xc_launch_tta_gather_u8(d_up, d_tr, (long long)(variant_plane_stride_bytes / 4), w, h, d_dst, image_stride_bytes, stride_bytes, px_bytes, byte0, n_ch,
                                      planes_per_image, first_plane, n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

}  // extern "C"
