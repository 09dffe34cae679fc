// w2xc_image_tta.cpp -- test-time augmentation: tta_pass (spread -> the CNN on the 8 variants -> gather; kernels in w2xc_tta.hip, and -- the uint8 image at the
// outer side: the RGB and head routes of the RGBA TTA calls -- w2xc_tta_u8.hip), which the image pipelines share (w2xc_image.hpp), the two TTA plane calls and
// the four spread / gather building blocks.
#include "w2xc_image.hpp"

namespace w2xc_eng {

int tta_pass(const TtaPass &t, int runs, PlanesIn src, int w, int h, PlanesOut dst, float *var, hipStream_t st, const w2xc_opts &o, const TtaU8 *u8)
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

}  // namespace w2xc_eng

using namespace w2xc_eng;

extern "C" {

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
