// w2xc_image.cpp -- N2: the CLI's image pipeline around the plane conversion -- uint8 BGR -> float YUV, the noise /
// scale passes on Y, bicubic U/V, the final shrink, YUV -> uint8 (main.cpp:74-76,83-98,126-172).
// And the same surface for RGB models (3 planes in, 3 out; w2xc_process_image_rgb_u8*): no chroma side path, every pass a CNN pass on all three planes,
// the first and the last layer of the call reading / writing the uint8 image themselves where their kernels can (no counterpart in v1).
// One pipeline per route -- process_y_device, process_rgb_device -- for S images of one size: the single-image calls, the batches and the RGBA call
// (process_rgba_device, around either) all run these two.  What is fixed for a call travels as an ImageCall, the uint8 images as U8Images views.
// The other families -- tta_pass, RGBA images, YUV frames -- are units of their own beside this one; what they share, the call forms among it: w2xc_image.hpp.
#include "w2xc_image.hpp"

namespace w2xc_eng {

// The Y pipeline for a sub-batch of S images (S <= cap, the call's sub-batch size: the planes are sized by cap, not by the call's n): noise (optional,
// main.cpp:83-98) then `iterations` 2x scale steps (main.cpp:126-156), the shrink, the colour stages around them.  Every plane lies on a plane_floats
// boundary, ps floats from the next; a level holds the Y group (S Y planes, with alpha S alpha planes behind them), S U planes, S V planes, level 0 also
// the Y group of the noise pass (image_aux_floats).  So the Y planes go to run_batch as they lie, U and V are 2 S adjacent planes for the bicubic launch, all of them the
// planes of the one shrink launch.  One launch per colour / resize stage.
int process_y_device(const ImageCall &c, int S, int cap, U8In in, U8Out out, size_t skip, AlphaRide *al)
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
RgbPlan rgb_plan(const ImageCall &c)
{
    RgbPlan R;
    const int passes = (c.mn ? 1 : 0) + c.iterations;
    // (TTA: the mean is taken before the rounding, so no LAYER takes the uint8 image; the RGBA TTA calls have the spread and the gather take it -- whatever
    // the precision and the kernels -- the gather where the last pass is a scale pass with nothing behind it)
    R.src_u8 = c.tta ? c.tta_u8 : resolve_chain(c.mn ? c.mn : c.msc, c.o).u8_source;
    R.dst_u8 = c.tta ? c.tta_u8 && c.shrink == 0.0 && c.iterations > 0 : c.shrink == 0.0 && resolve_chain(c.iterations > 0 ? c.msc : c.mn, c.o).u8_sink;
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
int process_rgb_device(const ImageCall &c, int S, int cap, U8In in, U8Out out, size_t skip, int ends)
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

// ---- the plan of a call: host arithmetic only, before any device is touched ----
// The options' errors (plan_rows) of the noise pass and of the largest scale pass, and *sub = images per sub-batch of a batch: as many as
// w2xc_opts.workspace_mb holds of the pipeline's own memory per image (the float planes of every level + the uint8 image in and out), at least 1.
//   PLAN_RGB  first: each model takes three planes and gives three (a Y model beside an RGB one fails here too)
//   both      at most the sub-batch run_batch / run_batch_planes takes at the LARGEST level where a batched chain applies (more images would only be cut again
//             there, and the planes of a larger sub-batch would be memory without a launch saved)
// The RGBA call gives its own bytes per image (per_image; 0 = the 3-channel call's, above) and ya = 2 on the Y route: a Y brings its alpha plane, so a
// sub-batch run_batch takes whole holds half as many images.
int plan_image_call(PlanKind kind, const ImageCall &c, int *sub, size_t per_image, int ya, const char *call)
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
int check_process_args(const ImageCall &c, bool head_ok)
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
int check_image_size(ImageCall &c, size_t in_stride, size_t out_stride, int px)
{
    if (c.w <= 0 || c.h <= 0 || c.iterations < 0 || c.iterations > 4) return fail(W2XC_ERR_ARG, "bad image size / iteration count");
    if (c.shrink < 0.0 || c.shrink >= 1.0) return fail(W2XC_ERR_ARG, "shrink_ratio must be 0 (none) or in (0,1)");
    final_size(c.w, c.h, c.iterations, c.shrink, &c.fw, &c.fh);
    if (c.fw < 1 || c.fh < 1) return fail(W2XC_ERR_ARG, "shrink_ratio leaves an empty image");
    if (in_stride < (size_t)c.w * px || out_stride < (size_t)c.fw * px) return fail(W2XC_ERR_ARG, "row strides must be >= %d*width bytes", px);
    return W2XC_OK;
}

// the largest level of the call, (w << iterations) x (h << iterations), is at most 2^28 a side (what the plans and the layouts above compute with)
int check_image_extent(const ImageCall &c)
{
    if (c.w > (1 << 28) >> c.iterations || c.h > (1 << 28) >> c.iterations) return fail(W2XC_ERR_ARG, "image too large");
    return W2XC_OK;
}

// ---- the call forms (w2xc_image.hpp) ----
// The device copies of a single host image live in the owning context and are kept between calls -- no hipMalloc / hipFree per image.
int host_single_form(ImageCall &c, int px, U8In in, U8Out out, int dev, SubBatchRef enqueue)
{
    LockedCtx lc;
    if (int rc = lc.open(c.mn, c.msc, dev)) return rc;
    c.ctx = lc;
    c.rows = true;
    DevCtx *own = c.ctx.owner();
    const size_t rs = (size_t)c.w * px, RS = (size_t)c.fw * px, in_bytes = align256(rs * c.h);
    if (int rc = own->img_io.reserve(in_bytes + RS * c.fh, "the image")) return rc;
    unsigned char *d_in = own->img_io.as<unsigned char>(), *d_out = d_in + in_bytes;
    HIP_TRY(hipMemcpy2D(d_in, rs, in.p, in.row, rs, c.h, hipMemcpyHostToDevice));
    if (int rc = enqueue(c, 1, 1, U8In{d_in, 0, rs}, U8Out{d_out, 0, RS})) { hipDeviceSynchronize(); return rc; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(out.p, out.row, d_out, RS, RS, c.fh, hipMemcpyDeviceToHost));
    return W2XC_OK;
}

int host_batch_form(ImageCall &c, int n, const unsigned char *const *in, size_t in_stride, unsigned char *const *out, size_t out_stride, int px, int sub,
                    SubBatchRef enqueue)
{
    if (n == 1) {   // nothing to overlap: the synchronous single-image sequence, on the first device of the mask
        std::vector<int> devs;
        if (int rc = host_devices(c.o, &devs)) return rc;
        return host_single_form(c, px, U8In{in[0], 0, in_stride}, U8Out{out[0], 0, out_stride}, devs[0], enqueue);
    }
    HostBatch b;
    b.n = n;
    b.in = (const void *const *)in; b.out = (void *const *)out;
    b.in_stride = in_stride; b.out_stride = out_stride;
    b.in_row = (size_t)c.w * px; b.out_row = (size_t)c.fw * px;
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
        return enqueue(d, cnt, max_sub, U8In{(const unsigned char *)din, b.in_img, b.in_row}, U8Out{(unsigned char *)dout, b.out_img, b.out_row});
    };
    return batch_host_run(b, c.o, sub);
}

int check_device_batch_overlap(const ImageCall &c, int n, U8In in, U8Out out, int px)
{
    const size_t in_ext = image_extent(c.h, in.row, c.w, px), out_ext = image_extent(c.fh, out.row, c.fw, px);
    if (n > 1 && out.img < out_ext)
        return fail(W2XC_ERR_ARG, "output images overlap each other (image stride %zu < %zu bytes)", out.img, out_ext);
    if (ranges_overlap(in.p, (size_t)(n - 1) * in.img + in_ext, out.p, (size_t)(n - 1) * out.img + out_ext))
        return fail(W2XC_ERR_ARG, "output images overlap the input images");
    return W2XC_OK;
}

int device_batch_form(ImageCall &c, int n, int sub, U8In in, U8Out out, SubBatchRef enqueue)
{
    sub = std::min(sub, n);
    LockedCtx lc;
    if (int rc = lc.open(c.mn, c.msc, c.o.device)) return rc;
    c.ctx = lc;
    return for_sub_batches(n, sub, [&](int b0, int S) {
        return enqueue(c, S, sub, U8In{in.p + (size_t)b0 * in.img, in.img, in.row}, U8Out{out.p + (size_t)b0 * out.img, out.img, out.row});
    });
}

namespace {

// what the family gives the call forms: the pipeline of its route on a sub-batch
auto sub_batch_of(bool rgb)
{
    return [rgb](const ImageCall &c, int S, int cap, U8In in, U8Out out) { return rgb ? process_rgb_device(c, S, cap, in, out) : process_y_device(c, S, cap, in, out); };
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

// ---- the four forms of the image call, for Y models (rgb = false: w2xc_process_image_u8*) and RGB models (w2xc_process_image_rgb_u8*) ----
// what both single forms refuse.  device, RGB: the first layer may read the source while bands of the result are already written -- the two must not share memory
int check_image_single(bool rgb, ImageCall &c, U8In in, U8Out out, bool device)
{
    int rc = check_process_args(c, rgb), sub;
    if (rc) return rc;
    if (!in.p || !out.p) return fail(W2XC_ERR_ARG, "null argument");
    if ((rc = check_image_size(c, in.row, out.row))) return rc;
    if (rgb && device && ranges_overlap(in.p, image_extent(c.h, in.row, c.w, 3), out.p, image_extent(c.fh, out.row, c.fw, 3)))
        return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
    if (rgb) return plan_image_call(PLAN_RGB, c, &sub);
    return c.tta ? check_y_models(c) : W2XC_OK;
}

int image_ex_device(bool rgb, ImageCall c, U8In in, U8Out out)
{
    LockedCtx lc;
    int rc = check_image_single(rgb, c, in, out, true);
    if (rc || (rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    c.rows = true;
    return sub_batch_of(rgb)(c, 1, 1, in, out);
}

int image_ex_host(bool rgb, ImageCall c, U8In in, U8Out out)
{
    if (int rc = check_image_single(rgb, c, in, out, false)) return rc;
    if (w2xc_device_count() <= 0) return fail(W2XC_ERR_HIP, "no HIP device available (libw2xc_hip has no CPU fallback)");
    return host_single_form(c, 3, in, out, c.o.device, sub_batch_of(rgb));
}

int image_batch_device(bool rgb, ImageCall c, int n, U8In in, U8Out out)
{
    int rc = check_image_batch_args(rgb, c, n, in.row, out.row);
    if (rc) return rc;
    if (!in.p || !out.p) return fail(W2XC_ERR_ARG, "null argument");
    if ((rc = check_device_batch_overlap(c, n, in, out, 3))) return rc;
    int sub = 1;
    if ((rc = plan_image_call(rgb ? PLAN_RGB : PLAN_Y, c, &sub))) return rc;
    return device_batch_form(c, n, sub, in, out, sub_batch_of(rgb));
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
    return host_batch_form(c, n, in, in_stride, out, out_stride, 3, sub, sub_batch_of(rgb));
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

}  // extern "C"
