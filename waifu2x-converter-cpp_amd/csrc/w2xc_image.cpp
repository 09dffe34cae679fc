// w2xc_image.cpp -- N2: the CLI's image pipeline around the plane conversion -- uint8 BGR -> float YUV, the noise /
// scale passes on Y through run_rows, bicubic U/V, the final shrink, YUV -> uint8 (main.cpp:74-76,83-98,126-172).
// And the same surface for RGB models (3 planes in, 3 out; w2xc_process_image_rgb_u8*): no chroma side path, every pass a CNN pass on all three planes,
// the first and the last layer of the call reading / writing the uint8 image themselves where their kernels can (no counterpart in v1).
#include "w2xc_engine.hpp"
#include "w2xc_host_geom.hpp"

namespace w2xc_eng {

namespace {

// the Y / U / V planes of both image pipelines live in the owning context's aux buffer, behind `skip` bytes (a multiple of 256) that are the caller's: the
// RGBA call keeps its uint8 images there.  (A buffer that grows loses its content: whoever owns such bytes reserves the whole call's need first.)
int reserve_aux(DevCtx *c, size_t skip, size_t floats) { return c->aux.reserve(skip + floats * sizeof(float), "the image planes"); }
float *aux_planes(DevCtx *c, size_t skip) { return reinterpret_cast<float *>(c->aux.as<unsigned char>() + skip); }
size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// An alpha plane that rides with Y (the Y route of w2xc_process_image_rgba_u8*): a = u8 / 255 of the RGBA image `src`, through every scale iteration as the
// second plane of a run_batch of two -- one plane stride behind the Y plane that feeds the iteration -- and through the shrink; never through the noise model.
// *plane = where the call left it (the final size, floats).  Only with iterations >= 1.
struct AlphaRide {
    const unsigned char *src;
    size_t stride;
    float *plane;
};
// float planes of process_image_device: level 0 (w x h) with a second Y for the noise pass, then one level per iteration and the shrink's; with alpha every Y
// plane has an alpha plane behind it
size_t y_image_floats(int w, int h, int iterations, double shrink, bool alpha)
{
    const size_t np = alpha ? 4 : 3, ya = alpha ? 2 : 1;
    size_t need = (np + ya) * (size_t)w * h, lvl = (size_t)w * h;
    for (int i = 1; i <= iterations; i++) { lvl *= 4; need += np * lvl; }
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    if (shrink > 0.0) need += np * (size_t)fw * fh;
    return need;
}

// noise (optional, main.cpp:83-98) then `iterations` 2x scale steps (optional model, main.cpp:126-156).
// `c` is the context that owns the plane buffer (the scale model's when present, else the noise model's);
// cn / cs are the contexts of the two models (locked by the caller).
int process_image_device(w2xc_model *mn, DevCtx *cn, w2xc_model *msc, DevCtx *cs, const unsigned char *d_in, size_t in_stride, int w,
                         int h, unsigned char *d_out, size_t out_stride, int iterations, double shrink, hipStream_t st, const w2xc_opts &o,
                         size_t skip = 0, AlphaRide *al = nullptr)
{
    DevCtx *c = cs ? cs : cn;
    const size_t ya = al ? 2 : 1;   // planes a Y takes: itself and its alpha
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    if (int rc = reserve_aux(c, skip, y_image_floats(w, h, iterations, shrink, al != nullptr))) return rc;
    float *base = aux_planes(c, skip);
    int cw = w, ch = h;
    float *y = base, *u = y + ya * (size_t)cw * ch, *v = u + (size_t)cw * ch, *yn = v + (size_t)cw * ch;
    base = yn + ya * (size_t)cw * ch;
    HIP_TRY(w2xc_launch_u8_to_yuv(d_in, in_stride, w, h, y, u, v, st));                                   // :75-76
    if (al) HIP_TRY(w2xc_launch_alpha_to_plane(al->src, al->stride, w, h, (mn ? yn : y) + (size_t)cw * ch, st));
    if (mn) {                                                                                             // :91-98
        int rc = run_rows(mn, cn, y, cw, ch, 0, cw, 0, ch, yn, cw, st, o, 0, 1, 0, 0, nullptr, ch);
        if (rc) return rc;
        y = yn;
    }
    for (int it = 0; it < iterations; it++) {
        const int nw = cw * 2, nh = ch * 2;
        float *y2 = base, *u2 = y2 + ya * (size_t)nw * nh, *v2 = u2 + (size_t)nw * nh;
        base = v2 + (size_t)nw * nh;
        // Y: INTER_NEAREST 2x folded into layer 1 (:136-140) + convertWithModels (:148); with alpha, Y and alpha as one batch of two planes (per plane
        // the bits of the single call: run_batch)
        int rc = al ? run_batch(msc, cs, 2, 1, y, (long long)cw * ch, (size_t)cw, cw, ch, y2, (long long)nw * nh, (size_t)nw, st, o)
                    : run_rows(msc, cs, y, cw, nh, 0, nw, 0, nh, y2, nw, st, o, 1, 1, 0, 0, nullptr, nh);
        if (rc) return rc;
        HIP_TRY(w2xc_launch_resize2x_cubic(u, cw, ch, u2, st));                                            // :144-146
        HIP_TRY(w2xc_launch_resize2x_cubic(v, cw, ch, v2, st));
        y = y2; u = u2; v = v2; cw = nw; ch = nh;
    }
    if (shrink > 0.0) {                                                                                   // :158-167
        float *ys = base, *us = ys + ya * (size_t)fw * fh, *vs = us + (size_t)fw * fh;
        HIP_TRY(w2xc_launch_resize_linear(y, cw, ch, ys, fw, fh, st));
        if (al) HIP_TRY(w2xc_launch_resize_linear(y + (size_t)cw * ch, cw, ch, ys + (size_t)fw * fh, fw, fh, st));
        HIP_TRY(w2xc_launch_resize_linear(u, cw, ch, us, fw, fh, st));
        HIP_TRY(w2xc_launch_resize_linear(v, cw, ch, vs, fw, fh, st));
        y = ys; u = us; v = vs; cw = fw; ch = fh;
    }
    HIP_TRY(w2xc_launch_yuv_to_u8(y, u, v, cw, ch, d_out, out_stride, st));                               // :171-172
    if (al) al->plane = y + (size_t)cw * ch;
    return W2XC_OK;
}

// ---- batches of same-size images (w2xc_process_image_u8_batch*) ----
// Images per sub-batch: as many as w2xc_opts.workspace_mb holds of the pipeline's own memory per image (the float planes of every level + the uint8 image
// in and out), at most the sub-batch run_batch takes at the LARGEST level where its batched chain applies (more images would only be cut again there, and
// the planes of a larger sub-batch would be memory without a launch saved), at least 1.  Also where the options' errors surface (host arithmetic only).
int image_sub_size(const w2xc_model *mn, const w2xc_model *msc, int w, int h, int iterations, double shrink, const w2xc_opts &o, int *sub)
{
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    const size_t budget = (size_t)(o.workspace_mb > 0 ? o.workspace_mb : 16384) << 20;
    const size_t per = image_aux_floats(w, h, iterations, shrink) * 4 + (size_t)w * 3 * h + (size_t)fw * 3 * fh;
    size_t k = std::min<size_t>(std::max<size_t>(budget / per, 1), 65535);
    const w2xc_model *pass[2] = {mn, iterations > 0 ? msc : nullptr};
    for (int i = 0; i < 2; i++) {
        if (!pass[i]) continue;
        const int W = i ? w << iterations : w, H = i ? h << iterations : h;   // (the last scale iteration: the largest planes of the call)
        RowPlan P;
        int rc = plan_rows(pass[i], o, W, H, 0, 0, H, H, 1, false, &P);
        if (rc) return rc;
        if (batch_eligible(pass[i], P)) {
            size_t img_f[2];
            batch_ws_floats(P, img_f);
            k = std::min<size_t>(k, (size_t)batch_sub_size(P.o, img_f));
        }
    }
    *sub = (int)k;
    return W2XC_OK;
}

// process_image_device for a sub-batch of S images (S <= cap, the call's sub-batch size: the planes are sized by cap, not by the call's n).  Per level the
// planes are S Y planes, S U planes, S V planes, all ps floats apart: the Y planes go to run_batch as they lie, U and V are 2 S adjacent planes for the
// bicubic launch, Y / U / V 3 S planes for the shrink.  One launch per colour / resize stage; the CNN passes are run_batch's.
int process_image_batch_device(w2xc_model *mn, DevCtx *cn, w2xc_model *msc, DevCtx *cs, int S, int cap, const unsigned char *d_in, size_t in_img,
                               size_t in_stride, int w, int h, unsigned char *d_out, size_t out_img, size_t out_stride, int iterations, double shrink,
                               hipStream_t st, const w2xc_opts &o)
{
    DevCtx *c = cs ? cs : cn;
    const size_t need = image_aux_floats(w, h, iterations, shrink) * (size_t)cap;
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    if (int rc = reserve_aux(c, 0, need)) return rc;
    float *base = c->aux.as<float>();
    int cw = w, ch = h;
    long long ps = (long long)plane_floats(cw, ch);
    float *y = base, *u = y + (size_t)S * ps, *v = u + (size_t)S * ps, *yn = v + (size_t)S * ps;
    base += 4 * (size_t)cap * ps;
    HIP_TRY(w2xc_launch_u8_to_yuv_batch(d_in, in_img, in_stride, w, h, y, u, v, ps, S, st));               // :75-76
    if (mn) {                                                                                             // :91-98
        int rc = run_batch(mn, cn, S, 0, y, ps, (size_t)cw, cw, ch, yn, ps, (size_t)cw, st, o);
        if (rc) return rc;
        y = yn;
    }
    for (int it = 0; it < iterations; it++) {
        const int nw = cw * 2, nh = ch * 2;
        const long long ps2 = (long long)plane_floats(nw, nh);
        float *y2 = base, *u2 = y2 + (size_t)S * ps2, *v2 = u2 + (size_t)S * ps2;
        base += 3 * (size_t)cap * ps2;
        int rc = run_batch(msc, cs, S, 1, y, ps, (size_t)cw, cw, ch, y2, ps2, (size_t)nw, st, o);         // :136-148
        if (rc) return rc;
        HIP_TRY(w2xc_launch_resize2x_cubic_batch(u, ps, cw, ch, u2, ps2, 2 * S, st));                      // :144-146 (v = u + S ps, v2 = u2 + S ps2)
        y = y2; u = u2; v = v2; cw = nw; ch = nh; ps = ps2;
    }
    if (shrink > 0.0) {                                                                                   // :158-167
        const long long pss = (long long)plane_floats(fw, fh);
        float *ys = base, *us = ys + (size_t)S * pss, *vs = us + (size_t)S * pss;
        HIP_TRY(w2xc_launch_resize_linear_batch(y, u, S, ps, cw, ch, ys, pss, fw, fh, 3 * S, st));
        y = ys; u = us; v = vs; cw = fw; ch = fh; ps = pss;
    }
    HIP_TRY(w2xc_launch_yuv_to_u8_batch(y, u, v, ps, cw, ch, d_out, out_img, out_stride, S, st));          // :171-172
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
};
RgbPlan rgb_plan(const w2xc_model *mn, const w2xc_model *msc, int w, int h, int iterations, double shrink, const w2xc_opts &o)
{
    RgbPlan R;
    const int passes = (mn ? 1 : 0) + iterations;
    R.src_u8 = u8_source_layer(mn ? mn : msc, o);
    R.dst_u8 = shrink == 0.0 && u8_sink_layer(iterations > 0 ? msc : mn, o);
    if (!R.src_u8) R.floats += 3 * plane_floats(w, h);
    for (int p = 1; p <= passes; p++) {
        const int lvl = p - (mn ? 1 : 0);   // the pass's output level: the noise pass stays on level 0
        if (p < passes || !R.dst_u8) R.floats += 3 * plane_floats(w << lvl, h << lvl);
    }
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    if (shrink > 0.0) R.floats += 3 * plane_floats(fw, fh);
    return R;
}

// A sub-batch of S images (S <= cap; the planes are sized by cap): per level the three planes of image i lie at level + i * 3 ps, ps floats apart.  The
// colour stages and the shrink are one launch for the sub-batch; RGB chains have no batch kernels, so every pass is the single-image launch sequence per
// image, enqueued back to back.  A single image is a sub-batch of one.
// (skip: the float planes start that many bytes into the aux buffer -- reserve_aux)
int process_rgb_batch_at(size_t skip, w2xc_model *mn, DevCtx *cn, w2xc_model *msc, DevCtx *cs, int S, int cap, const unsigned char *d_in, size_t in_img,
                         size_t in_stride, int w, int h, unsigned char *d_out, size_t out_img, size_t out_stride, int iterations, double shrink,
                         hipStream_t st, const w2xc_opts &o)
{
    DevCtx *c = cs ? cs : cn;
    const RgbPlan R = rgb_plan(mn, msc, w, h, iterations, shrink, o);
    float *base = nullptr;
    if (R.floats) {
        if (int rc = reserve_aux(c, skip, R.floats * (size_t)cap)) return rc;
        base = aux_planes(c, skip);
    }
    int cw = w, ch = h;
    long long ps = (long long)plane_floats(cw, ch);
    float *cur = nullptr;   // the current level's planes; nullptr = the image is still the caller's uint8 source
    if (!R.src_u8) {
        cur = base;
        base += 3 * (size_t)cap * ps;
        HIP_TRY(w2xc_launch_u8_to_rgb_batch(d_in, in_img, in_stride, w, h, cur, ps, 3 * ps, S, st));
    }
    const int passes = (mn ? 1 : 0) + iterations;
    for (int p = 1; p <= passes; p++) {
        const bool noise = mn && p == 1;
        w2xc_model *m = noise ? mn : msc;
        DevCtx *cm = noise ? cn : cs;
        const int up = noise ? 0 : 1, nw = cw << up, nh = ch << up;
        const long long ps2 = (long long)plane_floats(nw, nh);
        const bool from_u8 = cur == nullptr, to_u8 = p == passes && R.dst_u8;
        float *nxt = nullptr;
        if (!to_u8) { nxt = base; base += 3 * (size_t)cap * ps2; }
        for (int i = 0; i < S; i++) {
            const float *in = from_u8 ? reinterpret_cast<const float *>(d_in + (size_t)i * in_img) : cur + (size_t)i * 3 * ps;
            float *out = to_u8 ? reinterpret_cast<float *>(d_out + (size_t)i * out_img) : nxt + (size_t)i * 3 * ps2;
            int rc = run_rows(m, cm, in, from_u8 ? in_stride : (size_t)cw, nh, 0, nw, 0, nh, out, to_u8 ? out_stride : (size_t)nw, st, o, up, 3,
                              from_u8 ? 1 : ps, to_u8 ? 1 : ps2, nullptr, nh, (from_u8 ? ROWS_U8_SRC : 0) | (to_u8 ? ROWS_U8_DST : 0));
            if (rc) return rc;
        }
        if (to_u8) return W2XC_OK;
        cur = nxt; cw = nw; ch = nh; ps = ps2;
    }
    if (shrink > 0.0) {
        int fw, fh;
        final_size(w, h, iterations, shrink, &fw, &fh);
        const long long pss = (long long)plane_floats(fw, fh);
        float *dst = base;
        HIP_TRY(w2xc_launch_resize_linear_batch(cur, cur, 3 * S, ps, cw, ch, dst, pss, fw, fh, 3 * S, st));   // (the 3 S planes of a level are ps apart)
        cur = dst; cw = fw; ch = fh; ps = pss;
    }
    HIP_TRY(w2xc_launch_rgb_to_u8_batch(cur, ps, 3 * ps, cw, ch, d_out, out_img, out_stride, S, st));
    return W2XC_OK;
}

int process_rgb_batch_device(w2xc_model *mn, DevCtx *cn, w2xc_model *msc, DevCtx *cs, int S, int cap, const unsigned char *d_in, size_t in_img,
                             size_t in_stride, int w, int h, unsigned char *d_out, size_t out_img, size_t out_stride, int iterations, double shrink,
                             hipStream_t st, const w2xc_opts &o)
{
    return process_rgb_batch_at(0, mn, cn, msc, cs, S, cap, d_in, in_img, in_stride, w, h, d_out, out_img, out_stride, iterations, shrink, st, o);
}

// RGB forms: each model takes three planes and gives three (a Y model beside an RGB one fails here too), and the options' errors (plan_rows: host
// arithmetic) -- before any device is touched.  *sub = images per sub-batch of a batch: what w2xc_opts.workspace_mb holds of float planes + uint8 images.
int check_rgb_call(const w2xc_model *mn, const w2xc_model *msc, int w, int h, int iterations, double shrink, const w2xc_opts &o, int *sub)
{
    const w2xc_model *pass[2] = {mn, msc};
    for (const w2xc_model *m : pass) {
        if (!m) continue;
        if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
        if (m->layers[0].nin != 3 || m->layers.back().nout != 3)
            return fail(W2XC_ERR_PLANES, "w2xc_process_image_rgb_u8*: three planes in and three planes out (the model takes %d and gives %d)",
                        m->layers[0].nin, m->layers.back().nout);
    }
    pass[1] = iterations > 0 ? msc : nullptr;
    for (int i = 0; i < 2; i++) {
        if (!pass[i]) continue;
        const int W = i ? w << iterations : w, H = i ? h << iterations : h;
        RowPlan P;
        if (int rc = plan_rows(pass[i], o, W, H, 0, 0, H, H, 3, true, &P)) return rc;
    }
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    const size_t budget = (size_t)(o.workspace_mb > 0 ? o.workspace_mb : 16384) << 20;
    const size_t per = rgb_plan(mn, msc, w, h, iterations, shrink, o).floats * 4 + (size_t)w * 3 * h + (size_t)fw * 3 * fh;
    *sub = (int)std::min<size_t>(std::max<size_t>(budget / per, 1), 65535);
    return W2XC_OK;
}

// The contexts of the (up to two) models of an image call on `dev`; with l1 / l2 they are locked, TOGETHER (std::lock's deadlock avoidance): two threads
// that pass the same two models in opposite roles -- (A as noise, B as scale) and (B as noise, A as scale) -- would otherwise each hold one mutex and
// wait for the other.  The plane buffers and the host pipeline are the owning context's: the scale model's when present.
struct ImageCtx {
    DevCtx *cn = nullptr, *cs = nullptr;
    DevCtx *owner() const { return cs ? cs : cn; }
};
int image_contexts(w2xc_model *mn, w2xc_model *msc, int dev, ImageCtx *ic, std::unique_lock<std::mutex> *l1 = nullptr, std::unique_lock<std::mutex> *l2 = nullptr)
{
    int rc;
    if (mn && (rc = get_ctx(mn, dev, &ic->cn))) return rc;
    if (msc && (rc = get_ctx(msc, dev, &ic->cs))) return rc;
    if (!l1) return W2XC_OK;
    // (at least one model: check_process_args has refused a call without any before a context is asked for)
    if (ic->cn && ic->cs && ic->cn != ic->cs) {
        *l1 = std::unique_lock<std::mutex>(ic->cn->mu, std::defer_lock);
        *l2 = std::unique_lock<std::mutex>(ic->cs->mu, std::defer_lock);
        std::lock(*l1, *l2);
    } else *l1 = std::unique_lock<std::mutex>(ic->owner()->mu);
    return W2XC_OK;
}

// resolve device + contexts of the (up to two) models and run the pipeline under their locks
int process_image_locked(bool rgb, w2xc_model *mn, w2xc_model *msc, const unsigned char *d_in, size_t in_stride, int w, int h, unsigned char *d_out,
                         size_t out_stride, int iterations, double shrink, hipStream_t st, const w2xc_opts &o, int dev)
{
    ImageCtx ic;
    std::unique_lock<std::mutex> l1, l2;
    if (int rc = image_contexts(mn, msc, dev, &ic, &l1, &l2)) return rc;
    if (rgb) return process_rgb_batch_device(mn, ic.cn, msc, ic.cs, 1, 1, d_in, 0, in_stride, w, h, d_out, 0, out_stride, iterations, shrink, st, o);
    return process_image_device(mn, ic.cn, msc, ic.cs, d_in, in_stride, w, h, d_out, out_stride, iterations, shrink, st, o);
}

int check_process_args(const w2xc_model *mn, const w2xc_model *msc, int iterations)
{
    if (!mn && !msc) return fail(W2XC_ERR_ARG, "need a noise model, a scale model or both");
    if (iterations > 0 && !msc) return fail(W2XC_ERR_ARG, "scale iterations need a scale model");
    if (!mn && iterations == 0) return fail(W2XC_ERR_ARG, "nothing to do (no noise model, 0 iterations)");
    return W2XC_OK;
}

int check_image_args(const w2xc_model *m, const void *in, size_t in_stride, int w, int h, const void *out, size_t out_stride, int iterations,
                     double shrink = 0.0, int px = 3)
{
    if (!m || !in || !out) return fail(W2XC_ERR_ARG, "null argument");
    if (w <= 0 || h <= 0 || iterations < 0 || iterations > 4) return fail(W2XC_ERR_ARG, "bad image size / iteration count");
    if (shrink < 0.0 || shrink >= 1.0) return fail(W2XC_ERR_ARG, "shrink_ratio must be 0 (none) or in (0,1)");
    int fw, fh;
    final_size(w, h, iterations, shrink, &fw, &fh);
    if (fw < 1 || fh < 1) return fail(W2XC_ERR_ARG, "shrink_ratio leaves an empty image");
    if (in_stride < (size_t)w * px || out_stride < (size_t)fw * px) return fail(W2XC_ERR_ARG, "row strides must be >= %d*width bytes", px);
    return W2XC_OK;
}

// One host image on device `dev`, synchronously (w2xc_process_image_u8_ex; a batch of one image, which has nothing to overlap with): blocking copies
// around the pipeline on the null stream.
int process_image_host(bool rgb, w2xc_model *mn, w2xc_model *msc, const unsigned char *in, size_t in_stride, int w, int h, unsigned char *out, size_t out_stride,
                       int iterations, double shrink, const w2xc_opts &o, int dev)
{
    DeviceGuard guard(dev);
    if (!guard.ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", dev);
    int W, H;
    final_size(w, h, iterations, shrink, &W, &H);
    // contexts of the (up to two) models, locked for the whole call: the device copies of the image live in the owning context
    // (the scale model's when present) and are kept between calls -- no hipMalloc / hipFree per image
    ImageCtx ic;
    std::unique_lock<std::mutex> l1, l2;
    int rc = image_contexts(mn, msc, dev, &ic, &l1, &l2);
    if (rc) return rc;
    DevCtx *c = ic.owner();
    const size_t in_bytes = ((size_t)w * 3 * h + 255) & ~(size_t)255, out_bytes = (size_t)W * 3 * H;
    if ((rc = c->img_io.reserve(in_bytes + out_bytes, "the image"))) return rc;
    unsigned char *d_in = c->img_io.as<unsigned char>(), *d_out = d_in + in_bytes;
    HIP_TRY(hipMemcpy2D(d_in, (size_t)w * 3, in, in_stride, (size_t)w * 3, h, hipMemcpyHostToDevice));
    rc = rgb ? process_rgb_batch_device(mn, ic.cn, msc, ic.cs, 1, 1, d_in, 0, (size_t)w * 3, w, h, d_out, 0, (size_t)W * 3, iterations, shrink, nullptr, o)
             : process_image_device(mn, ic.cn, msc, ic.cs, d_in, (size_t)w * 3, w, h, d_out, (size_t)W * 3, iterations, shrink, nullptr, o);
    if (rc) { hipDeviceSynchronize(); return rc; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(out, out_stride, d_out, (size_t)W * 3, (size_t)W * 3, H, hipMemcpyDeviceToHost));
    return W2XC_OK;
}

// what both batch forms refuse before any device is touched (the image pointers are the caller's: checked there)
int check_image_batch_args(bool rgb, const w2xc_model *mn, const w2xc_model *msc, int n, size_t in_stride, int w, int h, size_t out_stride, int iterations,
                           double shrink)
{
    if (n < 1) return fail(W2XC_ERR_ARG, "batch of %d images", n);
    int rc = check_process_args(mn, msc, iterations);
    if (rc) return rc;
    rc = check_image_args(mn ? mn : msc, &n, in_stride, w, h, &n, out_stride, iterations, shrink);   // (pointers: see above)
    if (rc) return rc;
    if (w > (1 << 28) >> iterations || h > (1 << 28) >> iterations) return fail(W2XC_ERR_ARG, "image too large");
    if (rgb) return W2XC_OK;   // (the models' plane form: check_rgb_call, behind the caller's pointer checks)
    if (mn && (rc = check_batch_model(mn))) return rc;
    if (msc && (rc = check_batch_model(msc))) return rc;
    return W2XC_OK;
}

// ---- RGBA images (w2xc_process_image_rgba_u8*) ----
// bleed -> the 3-channel pipeline of the route on the bled image -> alpha through the scale model -> merge.  The call's uint8 images
// live at the head of the owning context's aux buffer, the pipelines' float planes behind them:
//   bled   the packed 3-channel image after the bleed      stamp  the bleed's pass stamps (16 bits per pixel)
//   res    the packed 3-channel result of the colour call  grey / ares (RGB route, iterations >= 1)  alpha as the image (A, A, A), and its result
struct RgbaPlan {
    bool rgb = false;
    int passes = 0;          // bleed passes that can change a pixel: no pixel is farther than max(w, h) - 1 from an opaque one
    size_t bled = 0, stamp = 0, res = 0, grey = 0, ares = 0, head = 0;   // byte offsets; head = where the float planes start
    size_t bytes = 0;        // the whole call
};

// The route (the models choose it), everything the 3-channel call of the route refuses, and the plan -- host arithmetic only.
int plan_rgba(const w2xc_model *mn, const w2xc_model *msc, int w, int h, int iterations, double shrink, int bleed_passes, const w2xc_opts &o, RgbaPlan *R)
{
    const w2xc_model *first = mn ? mn : msc;
    if (first->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    if (w > (1 << 28) >> iterations || h > (1 << 28) >> iterations) return fail(W2XC_ERR_ARG, "image too large");
    R->rgb = first->layers[0].nin == 3;
    int sub;
    if (R->rgb) {
        if (int rc = check_rgb_call(mn, msc, w, h, iterations, shrink, o, &sub)) return rc;
    } else {
        if (mn) if (int rc = check_batch_model(mn)) return rc;
        if (msc) if (int rc = check_batch_model(msc)) return rc;
        if (int rc = image_sub_size(mn, msc, w, h, iterations, shrink, o, &sub)) return rc;   // (the options' errors: plan_rows)
    }
    long long P = bleed_passes;
    if (P < 0) P = (long long)(mn ? mn->layers.size() : 0) + (long long)(msc ? msc->layers.size() : 0);   // the CNN's reach at source resolution
    P = std::min<long long>(P, std::max(w, h) - 1);
    if (P > 65534) return fail(W2XC_ERR_ARG, "more than 65534 effective bleed passes");
    R->passes = (int)P;
    int W, H;
    final_size(w, h, iterations, shrink, &W, &H);
    size_t at = 0;
    const auto take = [&](size_t bytes) { const size_t a = at; at += align256(bytes); return a; };
    R->bled = take((size_t)w * 3 * h);
    R->stamp = take((size_t)w * 2 * h);
    R->res = take((size_t)W * 3 * H);
    size_t floats;
    if (R->rgb) {
        floats = rgb_plan(mn, msc, w, h, iterations, shrink, o).floats;
        if (iterations > 0) {
            R->grey = take((size_t)w * 3 * h);
            R->ares = take((size_t)W * 3 * H);
            floats = std::max(floats, rgb_plan(nullptr, msc, w, h, iterations, shrink, o).floats);
        }
    } else floats = y_image_floats(w, h, iterations, shrink, iterations > 0);
    if (iterations == 0 && shrink > 0.0) floats = std::max(floats, (size_t)w * h + (size_t)W * H);   // alpha as a plane and its shrunk plane
    R->head = at;
    R->bytes = at + floats * sizeof(float);
    return W2XC_OK;
}

int process_rgba_device(const RgbaPlan &R, w2xc_model *mn, DevCtx *cn, w2xc_model *msc, DevCtx *cs, const unsigned char *d_in, size_t in_stride, int w, int h,
                        unsigned char *d_out, size_t out_stride, int iterations, double shrink, hipStream_t st, const w2xc_opts &o)
{
    DevCtx *c = cs ? cs : cn;
    if (int rc = c->aux.reserve(R.bytes, "the RGBA image and its planes")) return rc;   // (all of it first: a buffer that grows loses its content)
    unsigned char *a8 = c->aux.as<unsigned char>();
    int W, H;
    final_size(w, h, iterations, shrink, &W, &H);
    const size_t rs = (size_t)w * 3, RS = (size_t)W * 3;
    HIP_TRY(w2xc_launch_rgba_bleed(d_in, in_stride, w, h, R.passes, a8 + R.bled, rs, reinterpret_cast<unsigned short *>(a8 + R.stamp), st));
    if (R.rgb) {
        int rc = process_rgb_batch_at(R.head, mn, cn, msc, cs, 1, 1, a8 + R.bled, 0, rs, w, h, a8 + R.res, 0, RS, iterations, shrink, st, o);
        if (rc) return rc;
        if (iterations > 0) {   // alpha = channel 1 of the scale-only call on (A, A, A)
            HIP_TRY(w2xc_launch_alpha_to_grey(d_in, in_stride, w, h, a8 + R.grey, rs, st));
            rc = process_rgb_batch_at(R.head, nullptr, nullptr, msc, cs, 1, 1, a8 + R.grey, 0, rs, w, h, a8 + R.ares, 0, RS, iterations, shrink, st, o);
            if (rc) return rc;
            HIP_TRY(w2xc_launch_merge_rgba_u8(a8 + R.res, RS, a8 + R.ares + 1, RS, 3, W, H, d_out, out_stride, st));
            return W2XC_OK;
        }
    } else {
        AlphaRide al = {d_in, in_stride, nullptr};
        int rc = process_image_device(mn, cn, msc, cs, a8 + R.bled, rs, w, h, a8 + R.res, RS, iterations, shrink, st, o, R.head, iterations > 0 ? &al : nullptr);
        if (rc) return rc;
        if (iterations > 0) {
            HIP_TRY(w2xc_launch_merge_rgba(a8 + R.res, RS, al.plane, W, H, d_out, out_stride, st));
            return W2XC_OK;
        }
    }
    if (shrink > 0.0) {
        // no scale pass but a shrink (both routes): a = u8 / 255, INTER_LINEAR like every other plane, rounded in the merge.  The pipeline's float planes
        // are free again: its result is the uint8 image `res`, and everything here follows it on the stream.
        float *a0 = aux_planes(c, R.head), *a1 = a0 + (size_t)w * h;
        HIP_TRY(w2xc_launch_alpha_to_plane(d_in, in_stride, w, h, a0, st));
        HIP_TRY(w2xc_launch_resize_linear(a0, w, h, a1, W, H, st));
        HIP_TRY(w2xc_launch_merge_rgba(a8 + R.res, RS, a1, W, H, d_out, out_stride, st));
        return W2XC_OK;
    }
    HIP_TRY(w2xc_launch_merge_rgba_u8(a8 + R.res, RS, d_in + 3, in_stride, 4, W, H, d_out, out_stride, st));   // same size: the alpha bytes as they are
    return W2XC_OK;
}

// what both forms of the RGBA call refuse before any device is touched
int check_rgba_call(const w2xc_model *mn, const w2xc_model *msc, const void *in, size_t in_stride, int w, int h, const void *out, size_t out_stride,
                    int iterations, double shrink, int bleed_passes, const w2xc_opts &o, RgbaPlan *R)
{
    int rc = check_process_args(mn, msc, iterations);
    if (rc) return rc;
    if ((rc = check_image_args(mn ? mn : msc, in, in_stride, w, h, out, out_stride, iterations, shrink, 4))) return rc;
    int W, H;
    final_size(w, h, iterations, shrink, &W, &H);
    const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (size_t)(h - 1) * in_stride + (size_t)w * 4;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)(H - 1) * out_stride + (size_t)W * 4;
    if (i0 < o1 && o0 < i1) return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
    return plan_rgba(mn, msc, w, h, iterations, shrink, bleed_passes, o, R);
}

int rgba_ex_device(w2xc_model *mn, w2xc_model *msc, const unsigned char *d_in, size_t in_stride, int w, int h, unsigned char *d_out, size_t out_stride,
                   int iterations, double shrink, int bleed_passes, void *hip_stream, const w2xc_opts *opts)
{
    const w2xc_opts o = resolve_opts(opts);
    RgbaPlan R;
    int rc = check_rgba_call(mn, msc, d_in, in_stride, w, h, d_out, out_stride, iterations, shrink, bleed_passes, o, &R);
    if (rc) return rc;
    int dev = o.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    DeviceGuard guard(dev);
    if (!guard.ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", dev);
    ImageCtx ic;
    std::unique_lock<std::mutex> l1, l2;
    if ((rc = image_contexts(mn, msc, dev, &ic, &l1, &l2))) return rc;
    return process_rgba_device(R, mn, ic.cn, msc, ic.cs, d_in, in_stride, w, h, d_out, out_stride, iterations, shrink, (hipStream_t)hip_stream, o);
}

// one host image on w2xc_opts.device, synchronously: blocking copies around the device sequence on the null stream (process_image_host)
int rgba_ex_host(w2xc_model *mn, w2xc_model *msc, const unsigned char *in, size_t in_stride, int w, int h, unsigned char *out, size_t out_stride,
                 int iterations, double shrink, int bleed_passes, const w2xc_opts *opts)
{
    const w2xc_opts o = resolve_opts(opts);
    RgbaPlan R;
    int rc = check_rgba_call(mn, msc, in, in_stride, w, h, out, out_stride, iterations, shrink, bleed_passes, o, &R);
    if (rc) return rc;
    if (w2xc_device_count() <= 0) return fail(W2XC_ERR_HIP, "no HIP device available (libw2xc_hip has no CPU fallback)");
    int dev = o.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    DeviceGuard guard(dev);
    if (!guard.ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", dev);
    int W, H;
    final_size(w, h, iterations, shrink, &W, &H);
    ImageCtx ic;
    std::unique_lock<std::mutex> l1, l2;
    if ((rc = image_contexts(mn, msc, dev, &ic, &l1, &l2))) return rc;
    DevCtx *c = ic.owner();
    const size_t in_bytes = align256((size_t)w * 4 * h), out_bytes = (size_t)W * 4 * H;
    if ((rc = c->img_io.reserve(in_bytes + out_bytes, "the image"))) return rc;
    unsigned char *d_in = c->img_io.as<unsigned char>(), *d_out = d_in + in_bytes;
    HIP_TRY(hipMemcpy2D(d_in, (size_t)w * 4, in, in_stride, (size_t)w * 4, h, hipMemcpyHostToDevice));
    rc = process_rgba_device(R, mn, ic.cn, msc, ic.cs, d_in, (size_t)w * 4, w, h, d_out, (size_t)W * 4, iterations, shrink, nullptr, o);
    if (rc) { hipDeviceSynchronize(); return rc; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(out, out_stride, d_out, (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost));
    return W2XC_OK;
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
int image_ex_device(bool rgb, w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w, int h,
                    unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio, void *hip_stream, const w2xc_opts *opts)
{
    int rc = check_process_args(noise_model, scale_model, iterations);
    if (rc) return rc;
    rc = check_image_args(noise_model ? noise_model : scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio);
    if (rc) return rc;
    const w2xc_opts o = resolve_opts(opts);
    if (rgb) {
        // (the first layer may read the source while bands of the result are already written: the two must not share memory)
        int W, H, sub;
        final_size(w, h, iterations, shrink_ratio, &W, &H);
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)(h - 1) * in_stride_bytes + (size_t)w * 3;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)(H - 1) * out_stride_bytes + (size_t)W * 3;
        if (i0 < o1 && o0 < i1) return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
        if ((rc = check_rgb_call(noise_model, scale_model, w, h, iterations, shrink_ratio, o, &sub))) return rc;
    }
    int dev = o.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    DeviceGuard guard(dev);
    if (!guard.ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", dev);
    return process_image_locked(rgb, noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio,
                                (hipStream_t)hip_stream, o, dev);
}

int image_ex_host(bool rgb, w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                  unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
{
    int rc = check_process_args(noise_model, scale_model, iterations);
    if (rc) return rc;
    rc = check_image_args(noise_model ? noise_model : scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio);
    if (rc) return rc;
    const w2xc_opts o = resolve_opts(opts);
    int sub;
    if (rgb && (rc = check_rgb_call(noise_model, scale_model, w, h, iterations, shrink_ratio, o, &sub))) return rc;
    if (w2xc_device_count() <= 0) return fail(W2XC_ERR_HIP, "no HIP device available (libw2xc_hip has no CPU fallback)");
    int dev = o.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    return process_image_host(rgb, noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, o, dev);
}

int image_batch_device(bool rgb, w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                       size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes, size_t out_stride_bytes,
                       int iterations, double shrink_ratio, void *hip_stream, const w2xc_opts *opts)
{
    int rc = check_image_batch_args(rgb, noise_model, scale_model, n, in_stride_bytes, w, h, out_stride_bytes, iterations, shrink_ratio);
    if (rc) return rc;
    if (!d_in || !d_out) return fail(W2XC_ERR_ARG, "null argument");
    int W, H;
    final_size(w, h, iterations, shrink_ratio, &W, &H);
    const size_t in_ext = (size_t)(h - 1) * in_stride_bytes + (size_t)w * 3, out_ext = (size_t)(H - 1) * out_stride_bytes + (size_t)W * 3;
    if (n > 1 && out_image_stride_bytes < out_ext)
        return fail(W2XC_ERR_ARG, "output images overlap each other (image stride %zu < %zu bytes)", out_image_stride_bytes, out_ext);
    {
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)(n - 1) * in_image_stride_bytes + in_ext;
        const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)(n - 1) * out_image_stride_bytes + out_ext;
        if (i0 < o1 && o0 < i1) return fail(W2XC_ERR_ARG, "output images overlap the input images");
    }
    const w2xc_opts o = resolve_opts(opts);
    int sub = 1;
    rc = rgb ? check_rgb_call(noise_model, scale_model, w, h, iterations, shrink_ratio, o, &sub)
             : image_sub_size(noise_model, scale_model, w, h, iterations, shrink_ratio, o, &sub);
    if (rc) return rc;
    sub = std::min(sub, n);
    int dev = o.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    DeviceGuard guard(dev);
    if (!guard.ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", dev);
    ImageCtx ic;
    std::unique_lock<std::mutex> l1, l2;
    if ((rc = image_contexts(noise_model, scale_model, dev, &ic, &l1, &l2))) return rc;
    const auto run = rgb ? process_rgb_batch_device : process_image_batch_device;
    for (int b0 = 0; b0 < n; b0 += sub) {
        rc = run(noise_model, ic.cn, scale_model, ic.cs, std::min(sub, n - b0), sub, d_in + (size_t)b0 * in_image_stride_bytes, in_image_stride_bytes,
                 in_stride_bytes, w, h, d_out + (size_t)b0 * out_image_stride_bytes, out_image_stride_bytes, out_stride_bytes, iterations, shrink_ratio,
                 (hipStream_t)hip_stream, o);
        if (rc) return rc;
    }
    return W2XC_OK;
}

int image_batch_host(bool rgb, w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w, int h,
                     unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
{
    int rc = check_image_batch_args(rgb, noise_model, scale_model, n, in_stride_bytes, w, h, out_stride_bytes, iterations, shrink_ratio);
    if (rc) return rc;
    if (!in || !out) return fail(W2XC_ERR_ARG, "null argument");
    int W, H;
    final_size(w, h, iterations, shrink_ratio, &W, &H);
    rc = check_batch_host_ptrs(n, (const void *const *)in, (size_t)(h - 1) * in_stride_bytes + (size_t)w * 3, (void *const *)out,
                               (size_t)(H - 1) * out_stride_bytes + (size_t)W * 3);
    if (rc) return rc;
    const w2xc_opts o = resolve_opts(opts);
    int sub = 1;
    if (rgb && (rc = check_rgb_call(noise_model, scale_model, w, h, iterations, shrink_ratio, o, &sub))) return rc;
    if (n == 1) {   // nothing to overlap: the synchronous single-image sequence, on the first device of the mask
        std::vector<int> devs;
        if ((rc = host_devices(o, &devs))) return rc;
        return process_image_host(rgb, noise_model, scale_model, in[0], in_stride_bytes, w, h, out[0], out_stride_bytes, iterations, shrink_ratio, o, devs[0]);
    }
    if (!rgb && (rc = image_sub_size(noise_model, scale_model, w, h, iterations, shrink_ratio, o, &sub))) return rc;
    HostBatch b;
    b.n = n;
    b.in = (const void *const *)in; b.out = (void *const *)out;
    b.in_stride = in_stride_bytes; b.out_stride = out_stride_bytes;
    b.in_row = (size_t)w * 3; b.out_row = (size_t)W * 3;
    b.in_rows = h; b.out_rows = H;
    b.in_img = (b.in_row * h + 255) & ~(size_t)255; b.out_img = (b.out_row * H + 255) & ~(size_t)255;
    // both models' contexts, locked together for this device's share of the call; the pipeline is the owning context's
    b.acquire = [&](int dev, std::unique_lock<std::mutex> &l1, std::unique_lock<std::mutex> &l2, HostPipe **pipe) -> int {
        ImageCtx ic;
        int r = image_contexts(noise_model, scale_model, dev, &ic, &l1, &l2);
        if (r) return r;
        *pipe = &ic.owner()->pipe;
        return W2XC_OK;
    };
    b.run = [&](int dev, int cnt, const void *din, void *dout, hipStream_t st, int max_sub) -> int {
        ImageCtx ic;
        int r = image_contexts(noise_model, scale_model, dev, &ic);
        if (r) return r;
        const auto run = rgb ? process_rgb_batch_device : process_image_batch_device;
        return run(noise_model, ic.cn, scale_model, ic.cs, cnt, max_sub, (const unsigned char *)din, b.in_img, b.in_row, w, h, (unsigned char *)dout, b.out_img,
                   b.out_row, iterations, shrink_ratio, st, o);
    };
    return batch_host_run(b, o, sub);
}

}  // namespace

}  // namespace w2xc_eng

using namespace w2xc_eng;

extern "C" {

int w2xc_process_image_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                    int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                    void *hip_stream, const w2xc_opts *opts)
try {
    return image_ex_device(false, noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, hip_stream, opts);
} W2XC_CATCH_ALL

int w2xc_process_image_u8_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                 int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, void *hip_stream,
                                 const w2xc_opts *opts)
{
    return w2xc_process_image_u8_ex_device(noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, 0.0,
                                           hip_stream, opts);
}

int w2xc_process_image_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                             unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
try {
    return image_ex_host(false, noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts);
} W2XC_CATCH_ALL

int w2xc_process_image_u8(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                          unsigned char *out, size_t out_stride_bytes, int iterations, const w2xc_opts *opts)
{
    return w2xc_process_image_u8_ex(noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, 0.0, opts);
}

// ---- batches of same-size images ----------------------------------------------------------------
int w2xc_process_image_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in, size_t in_image_stride_bytes,
                                       size_t in_stride_bytes, int w, int h, unsigned char *d_out, size_t out_image_stride_bytes,
                                       size_t out_stride_bytes, int iterations, double shrink_ratio, void *hip_stream, const w2xc_opts *opts)
try {
    return image_batch_device(false, noise_model, scale_model, n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes,
                              out_stride_bytes, iterations, shrink_ratio, hip_stream, opts);
} W2XC_CATCH_ALL

int w2xc_process_image_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes, int w,
                                int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
try {
    return image_batch_host(false, noise_model, scale_model, n, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts);
} W2XC_CATCH_ALL

// ---- RGB models: the same four forms ---------------------------------------------------------------
int w2xc_process_image_rgb_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes,
                                        int w, int h, unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                        void *hip_stream, const w2xc_opts *opts)
try {
    return image_ex_device(true, noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, hip_stream, opts);
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                 unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, const w2xc_opts *opts)
try {
    return image_ex_host(true, noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts);
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_batch_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *d_in,
                                           size_t in_image_stride_bytes, size_t in_stride_bytes, int w, int h, unsigned char *d_out,
                                           size_t out_image_stride_bytes, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                           void *hip_stream, const w2xc_opts *opts)
try {
    return image_batch_device(true, noise_model, scale_model, n, d_in, in_image_stride_bytes, in_stride_bytes, w, h, d_out, out_image_stride_bytes,
                              out_stride_bytes, iterations, shrink_ratio, hip_stream, opts);
} W2XC_CATCH_ALL

int w2xc_process_image_rgb_u8_batch(w2xc_model *noise_model, w2xc_model *scale_model, int n, const unsigned char *const *in, size_t in_stride_bytes,
                                    int w, int h, unsigned char *const *out, size_t out_stride_bytes, int iterations, double shrink_ratio,
                                    const w2xc_opts *opts)
try {
    return image_batch_host(true, noise_model, scale_model, n, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, opts);
} W2XC_CATCH_ALL

// ---- RGBA images: alpha through the scale model, colour bled under the transparent pixels ----------
int w2xc_process_image_rgba_u8_ex_device(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *d_in, size_t in_stride_bytes, int w, int h,
                                         unsigned char *d_out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes,
                                         void *hip_stream, const w2xc_opts *opts)
try {
    return rgba_ex_device(noise_model, scale_model, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, iterations, shrink_ratio, bleed_passes, hip_stream, opts);
} W2XC_CATCH_ALL

int w2xc_process_image_rgba_u8_ex(w2xc_model *noise_model, w2xc_model *scale_model, const unsigned char *in, size_t in_stride_bytes, int w, int h,
                                  unsigned char *out, size_t out_stride_bytes, int iterations, double shrink_ratio, int bleed_passes, const w2xc_opts *opts)
try {
    return rgba_ex_host(noise_model, scale_model, in, in_stride_bytes, w, h, out, out_stride_bytes, iterations, shrink_ratio, bleed_passes, opts);
} W2XC_CATCH_ALL

int w2xc_bleed_rgba_u8_device(const unsigned char *d_in, size_t in_stride_bytes, int w, int h, int passes, unsigned char *d_out_rgb, size_t out_stride_bytes,
                              void *hip_stream)
try {
    if (!d_in || !d_out_rgb || w <= 0 || h <= 0 || passes < 0 || in_stride_bytes < (size_t)w * 4 || out_stride_bytes < (size_t)w * 3)
        return fail(W2XC_ERR_ARG, "bad argument");
    const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)(h - 1) * in_stride_bytes + (size_t)w * 4;
    const uintptr_t o0 = (uintptr_t)d_out_rgb, o1 = o0 + (size_t)(h - 1) * out_stride_bytes + (size_t)w * 3;
    if (i0 < o1 && o0 < i1) return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
    passes = std::min(passes, std::max(w, h) - 1);   // (no pixel is farther from an opaque one)
    if (passes > 65534) return fail(W2XC_ERR_ARG, "more than 65534 effective bleed passes");
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    BleedScratch &b = bleed_scratch();
    std::lock_guard<std::mutex> lk(b.mu);
    Scratch &s = b.stamp[dev];
    if (int rc = s.reserve((size_t)w * 2 * h, "the bleed's pass stamps")) return rc;
    HIP_TRY(w2xc_launch_rgba_bleed(d_in, in_stride_bytes, w, h, passes, d_out_rgb, out_stride_bytes, s.as<unsigned short>(), (hipStream_t)hip_stream));
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

}  // extern "C"
