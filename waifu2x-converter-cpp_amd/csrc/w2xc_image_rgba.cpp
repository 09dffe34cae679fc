// w2xc_image_rgba.cpp -- RGBA images (w2xc_process_image_rgba_u8*): the colour bled under the transparent pixels, the 3-channel pipeline of the route
// (process_y_device / process_rgb_device, w2xc_image.cpp) on the bled images, alpha through the scale model, the merge; its forms through the call forms of
// w2xc_image.hpp.  And the bleed as a call of its own (w2xc_bleed_rgba_u8_device / _trim) with its scratch.
#include "w2xc_image.hpp"

namespace w2xc_eng {

namespace {

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
// (RgbaImageBytes, w2xc_host_geom.hpp: bytes per image of each of those, and the float planes per image; where they lie for a sub-batch: RgbaLayout, there)
struct RgbaPlan : RgbaImageBytes {
    bool rgb = false;
    bool fuse_src = false, fuse_dst = false;
    int passes = 0;          // bleed passes that can change a pixel: no pixel is farther than max(w, h) - 1 from an opaque one
    int sub = 1;             // images per sub-batch (plan_image_call)
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

// what every form of the RGBA call refuses before any device is touched.  in / out: the one image of a single call -- its pointers and their ranges are checked
// here, between the others; a batch checks its own pointers
int check_rgba_call(ImageCall &c, size_t in_stride, size_t out_stride, int bleed_passes, RgbaPlan *R, const U8In *in = nullptr, const U8Out *out = nullptr)
{
    int rc = check_process_args(c);
    if (rc) return rc;
    if (in && (!in->p || !out->p)) return fail(W2XC_ERR_ARG, "null argument");
    if ((rc = check_image_size(c, in_stride, out_stride, 4))) return rc;
    if (in && ranges_overlap(in->p, image_extent(c.h, in->row, c.w, 4), out->p, image_extent(c.fh, out->row, c.fw, 4)))
        return fail(W2XC_ERR_ARG, "the output image overlaps the input image");
    c.tta_u8 = c.tta && c.o.fusion != W2XC_FUSION_OFF;
    return plan_rgba(c, bleed_passes, R);
}

// what the family gives the call forms (w2xc_image.hpp): process_rgba_device by the call's plan
auto sub_batch_of(const RgbaPlan &R)
{
    return [&R](const ImageCall &c, int S, int cap, U8In in, U8Out out) { return process_rgba_device(R, c, S, cap, in, out); };
}

int rgba_ex_device(ImageCall c, U8In in, U8Out out, int bleed_passes)
{
    RgbaPlan R;
    LockedCtx lc;
    int rc = check_rgba_call(c, in.row, out.row, bleed_passes, &R, &in, &out);
    if (rc || (rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    c.rows = true;
    return process_rgba_device(R, c, 1, 1, in, out);
}

// one host image on w2xc_opts.device, synchronously
int rgba_ex_host(ImageCall c, U8In in, U8Out out, int bleed_passes)
{
    RgbaPlan R;
    if (int rc = check_rgba_call(c, in.row, out.row, bleed_passes, &R, &in, &out)) return rc;
    if (w2xc_device_count() <= 0) return fail(W2XC_ERR_HIP, "no HIP device available (libw2xc_hip has no CPU fallback)");
    return host_single_form(c, 4, in, out, c.o.device, sub_batch_of(R));
}

// ---- batches of RGBA images: image i byte for byte the single call's ----
int rgba_batch_device(ImageCall c, int n, U8In in, U8Out out, int bleed_passes)
{
    if (n < 1) return fail(W2XC_ERR_ARG, "batch of %d images", n);
    if (!in.p || !out.p) return fail(W2XC_ERR_ARG, "null argument");
    RgbaPlan R;
    int rc = check_rgba_call(c, in.row, out.row, bleed_passes, &R);
    if (rc || (rc = check_device_batch_overlap(c, n, in, out, 4))) return rc;
    c.rows = n == 1;   // (a batch of one is the single call, bands included)
    return device_batch_form(c, n, R.sub, in, out, sub_batch_of(R));
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
    return host_batch_form(c, n, in, in_stride, out, out_stride, 4, R.sub, sub_batch_of(R));
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

}  // namespace

}  // namespace w2xc_eng

using namespace w2xc_eng;

extern "C" {

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

}  // extern "C"
