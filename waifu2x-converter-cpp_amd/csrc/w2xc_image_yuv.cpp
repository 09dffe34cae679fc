// w2xc_image_yuv.cpp -- frames that are Y, U and V already (w2xc_process_frames_yuv_u8*): process_yuv_device, the Y pipeline without its colour stages (kernels in
// w2xc_yuv.hip) -- and, through RGB and head models by a colour matrix the caller names (w2xc_process_frames_yuv_u8_rgb*), process_yuv_rgb_device: the passes of the
// RGB pipeline (rgb_passes, w2xc_image.cpp) between two kernels (w2xc_yuv_rgb.hip).  The host forms' device mirror, and the five building blocks.
// The same calls on 16-bit words (w2xc_process_frames_yuv_u16*, "16-bit YUV frames"): the checks, the geometry, the mirror and the sub-batches take the sample
// size; the ends of a route (luma_in, luma_out, chroma_out, to_rgb, from_rgb) pick their launcher (w2xc_yuv16.hip, w2xc_yuv16_rgb.hip) by it, and nothing else
// does: the routes and the bodies of the building blocks read the same for both widths.
// The sized forms (w2xc_process_frames_yuv_*_sized*, "Sized YUV frames") are the same two routes with `iterations` scale passes, a linear shrink of the last
// level where the output is smaller than it, and chroma resized in one step (w2xc_yuv_sized.hip, w2xc_yuv16_sized.hip); the base calls are sized calls whose
// output is the last level.
#include "w2xc_image.hpp"

namespace w2xc_eng {

namespace {

// ---- YUV frames (w2xc_process_frames_yuv_u8* / _u16*; the arithmetic: include/w2xc_hip.h) ----
// Luma through the models as the planes of run_batch, chroma from samples to samples in one launch: no colour matrix, no float plane of chroma.
struct YuvGeom {
    int chroma = W2XC_YUV_400, range = W2XC_RANGE_FULL;   // (defaults: a building block fills in only the format fields its end of a route reads)
    int cosited = 0;        // W2XC_CHROMA_COSITED_X | _Y: the siting flags of the call's `chroma` ("Chroma siting"); chroma above is the layout alone
    int bps = 1, depth = 8;   // bytes per sample (1: w2xc_yuv_planes, 2: w2xc_yuv16_planes) and the bits of a value
    bool rgb = false;       // the frames go through RGB / head models (w2xc_process_frames_yuv_u8_rgb*): process_yuv_rgb_device
    int matrix = 0;         // ... by this colour matrix (W2XC_MATRIX_*)
    int cw = 0, ch = 0;     // the chroma planes of a w x h frame (0 x 0: W2XC_YUV_400)
    int ocw = 0, och = 0;   // ... of the call's output frame
    int W = 0, H = 0;       // the last level of the passes: (w << iterations) x (h << iterations)
    int ow = 0, oh = 0;     // the output frame: W x H, or what a sized call names (w <= ow <= W, h <= oh <= H: the linear shrink of the last level)
    ChromaAxis ax = {1.0, 0.5}, ay = {1.0, 0.5};   // chroma from the input plane to the output plane, per axis (chroma_axis: the LUMA ratio, the siting's offset)
};
// what chroma_out runs: the samples as they are, the bicubic 2x kernels, or the resize kernels at g.ax / g.ay
enum ChromaMode { CHROMA_COPY, CHROMA_2X, CHROMA_RESIZE };
// (the sizes of the chroma planes, the float planes and the bytes of a frame: yuv_chroma_size, yuv_aux_floats, yuv_rgb_aux_floats, yuv_frame_bytes -- w2xc_host_geom.hpp)

// One side of a call as the engine takes it, from either struct of the interface: byte pointers, strides in bytes, c_px in samples, pack (0 for bytes)
struct YuvSide {
    unsigned char *y = nullptr;
    size_t y_stride = 0, y_frame_stride = 0;
    unsigned char *u = nullptr, *v = nullptr;
    size_t c_stride = 0, c_frame_stride = 0;
    int c_px = 0, pack = 0;
};
// (a null struct stays a null side: check_yuv_side refuses it where it refuses null planes)
template <class Planes> const YuvSide *side_of(const Planes *s, int pack, YuvSide *store)
{
    if (!s) return nullptr;
    *store = {reinterpret_cast<unsigned char *>(s->y), s->y_stride, s->y_frame_stride, reinterpret_cast<unsigned char *>(s->u), reinterpret_cast<unsigned char *>(s->v),
              s->c_stride, s->c_frame_stride, s->c_px, pack};
    return store;
}
const YuvSide *side_of(const w2xc_yuv_planes *s, YuvSide *store) { return side_of(s, 0, store); }
const YuvSide *side_of(const w2xc_yuv16_planes *s, YuvSide *store) { return side_of(s, s ? s->pack : 0, store); }

// one side's planes from frame b0 on
YuvSide yuv_from(const YuvSide &s, size_t b0, bool chroma)
{
    YuvSide t = s;
    t.y += b0 * s.y_frame_stride;
    if (chroma) { t.u += b0 * s.c_frame_stride; t.v += b0 * s.c_frame_stride; }
    return t;
}

// n frames of w x h luma and cw x ch chroma on one side, samples of bps bytes: pointers, strides, c_px, and for words their alignment and the packing; its byte
// ranges go to iv tagged `tag` (check_batch_overlap)
int check_yuv_side(const YuvSide *s, int bps, int n, int w, int h, int cw, int ch, int tag, std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> &iv)
{
    if (!s || !s->y) return fail(W2XC_ERR_ARG, "null argument");
    const size_t y_ext = image_extent(h, s->y_stride, w, bps);
    if (s->y_stride < (size_t)w * bps || (n > 1 && s->y_frame_stride < y_ext)) return fail(W2XC_ERR_ARG, "luma: row stride below the row's bytes / frame stride below a plane");
    if (bps == 2) {
        if (s->pack != W2XC_PACK_LOW && s->pack != W2XC_PACK_HIGH) return fail(W2XC_ERR_ARG, "pack must be W2XC_PACK_LOW or W2XC_PACK_HIGH, got %d", s->pack);
        if (((uintptr_t)s->y | s->y_stride | s->y_frame_stride) & 1) return fail(W2XC_ERR_ARG, "luma: 16-bit samples need an even pointer and even strides");
    }
    for (int i = 0; i < n; i++) iv.push_back({{(uintptr_t)s->y + i * s->y_frame_stride, (uintptr_t)s->y + i * s->y_frame_stride + y_ext}, tag});
    if (!cw) return W2XC_OK;
    if (!s->u || !s->v) return fail(W2XC_ERR_ARG, "null argument");
    if (s->c_px != 1 && s->c_px != 2) return fail(W2XC_ERR_ARG, "c_px must be 1 (planar) or 2 (interleaved), got %d", s->c_px);
    const size_t row = chroma_row_bytes(cw, s->c_px, bps), c_ext = (size_t)(ch - 1) * s->c_stride + row;
    if (s->c_stride < row || (n > 1 && s->c_frame_stride < c_ext)) return fail(W2XC_ERR_ARG, "chroma: row stride below the row's bytes / frame stride below a plane");
    if (bps == 2 && (((uintptr_t)s->u | (uintptr_t)s->v | s->c_stride | s->c_frame_stride) & 1))
        return fail(W2XC_ERR_ARG, "chroma: 16-bit samples need even pointers and even strides");
    // two interleaved planes (NV12: v = u + 1 sample) are one range of bytes, two planes otherwise
    const uintptr_t u = (uintptr_t)s->u, v = (uintptr_t)s->v;
    const bool pair = s->c_px == 2 && (v == u + bps || u == v + bps);
    for (int i = 0; i < n; i++) {
        const uintptr_t off = i * s->c_frame_stride;
        if (pair) iv.push_back({{std::min(u, v) + off, std::min(u, v) + off + c_ext + bps}, tag});
        else { iv.push_back({{u + off, u + off + c_ext}, tag}); iv.push_back({{v + off, v + off + c_ext}, tag}); }
    }
    return W2XC_OK;
}

// the siting flags alone (the chroma blocks of the Y route take them as `cosited`): only the two bits, and only on an axis that is subsampled
int check_cosited(int cosited, bool sub_x, bool sub_y)
{
    if (cosited < 0 || (cosited & ~(W2XC_CHROMA_COSITED_X | W2XC_CHROMA_COSITED_Y)))
        return fail(W2XC_ERR_ARG, "cosited must be a combination of W2XC_CHROMA_COSITED_X and W2XC_CHROMA_COSITED_Y, got %d", cosited);
    if (((cosited & W2XC_CHROMA_COSITED_X) && !sub_x) || ((cosited & W2XC_CHROMA_COSITED_Y) && !sub_y))
        return fail(W2XC_ERR_ARG, "chroma siting flags 0x%x name an axis the layout does not subsample", cosited);
    return W2XC_OK;
}
// the layout and range enums of a frame, and the colour matrix of the calls that have one: what the frame calls and the blocks refuse alike
// `chroma` is a layout with the siting flags or-ed on: *layout = chroma & 0xF, *cosited = chroma & 0x30 -- the ONE place that decodes and refuses them
int check_chroma_range(int chroma, int range, int *layout, int *cosited)
{
    const int flags = W2XC_CHROMA_COSITED_X | W2XC_CHROMA_COSITED_Y;
    if (chroma < 0 || (chroma & ~(0xF | flags)) || (chroma & 0xF) > W2XC_YUV_400) return fail(W2XC_ERR_ARG, "unknown chroma layout %d", chroma);
    *layout = chroma & 0xF;
    *cosited = chroma & flags;
    if (int rc = check_cosited(*cosited, *layout != W2XC_YUV_444 && *layout != W2XC_YUV_400, *layout == W2XC_YUV_420)) return rc;
    if (range != W2XC_RANGE_FULL && range != W2XC_RANGE_LIMITED) return fail(W2XC_ERR_ARG, "unknown range %d", range);
    return W2XC_OK;
}
int check_matrix(int matrix)
{
    if (matrix < W2XC_MATRIX_BT601 || matrix > W2XC_MATRIX_BT2020) return fail(W2XC_ERR_ARG, "unknown colour matrix %d", matrix);
    return W2XC_OK;
}
// the bits of a value in a 16-bit word (the calls on bytes have none to name: 8)
int check_depth(int bps, int depth)
{
    if (bps == 2 && (depth < 8 || depth > 16)) return fail(W2XC_ERR_ARG, "depth must be 8 .. 16, got %d", depth);
    return W2XC_OK;
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

// everything both forms refuse, before a device is touched; *g = the geometry (g->bps and g->depth are the caller's), *sub = frames per sub-batch.  rgb: the call
// is w2xc_process_frames_yuv_u8_rgb* / _u16_rgb* -- RGB models, or an upconv head model as scale model, and a colour matrix; a grey frame (W2XC_YUV_400) belongs
// to the Y call.  sz: the sized form ("Sized YUV frames") -- iterations 0 .. 4 or W2XC_ITERATIONS_AUTO (resolved here, into c.iterations) and an output size
// inside [w, w << iterations] x [h, h << iterations]; null: a base call, iterations 0 .. 1 and the last level as output, refused in the words it always had
struct YuvOutSize { int w, h; };
int check_yuv_call(ImageCall &c, bool rgb, int n, int chroma, int range, int matrix, const YuvSide *in, const YuvSide *out, YuvGeom *g, int *sub,
                   const YuvOutSize *sz = nullptr)
{
    if (sz) {   // (AUTO is resolved before the models are looked at: "iterations >= 1 without a scale model" is about the resolved count)
        if (c.w <= 0 || c.h <= 0 || c.w > (1 << 22) || c.h > (1 << 22)) return fail(W2XC_ERR_ARG, "bad frame size");
        if (c.iterations == W2XC_ITERATIONS_AUTO) c.iterations = sized_auto_iterations(c.w, c.h, sz->w, sz->h);
        if (c.iterations < 0 || c.iterations > 4)
            return fail(W2XC_ERR_ARG, "iterations must be 0 .. 4 or W2XC_ITERATIONS_AUTO (got %d; an output of %d x %d from %d x %d)", c.iterations, sz->w, sz->h, c.w, c.h);
        if (sz->w < c.w || sz->h < c.h || sz->w > c.w << c.iterations || sz->h > c.h << c.iterations)
            return fail(W2XC_ERR_ARG, "the output size %d x %d lies outside %d .. %d x %d .. %d (iterations = %d)", sz->w, sz->h, c.w, c.w << c.iterations, c.h,
                        c.h << c.iterations, c.iterations);
    }
    int rc = check_process_args(c, rgb);
    if (rc || (rc = rgb ? check_yuv_rgb_precision(c) : check_y_models(c))) return rc;
    if (!sz && (c.iterations < 0 || c.iterations > 1)) return fail(W2XC_ERR_ARG, "iterations must be 0 or 1 (got %d)", c.iterations);
    if (n < 1 || n > (1 << 20)) return fail(W2XC_ERR_ARG, "batch of %d frames", n);
    if (c.w <= 0 || c.h <= 0 || c.w > (1 << 22) || c.h > (1 << 22)) return fail(W2XC_ERR_ARG, "bad frame size");
    if ((rc = check_chroma_range(chroma, range, &chroma, &g->cosited)) || (rc = check_depth(g->bps, g->depth))) return rc;
    if (rgb && chroma == W2XC_YUV_400)
        return fail(W2XC_ERR_ARG, "a frame without chroma (W2XC_YUV_400) belongs to %s", g->bps == 2 ? "w2xc_process_frames_yuv_u16*" : "w2xc_process_frames_yuv_u8*");
    if (rgb && (rc = check_matrix(matrix))) return rc;
    g->chroma = chroma; g->range = range; g->rgb = rgb; g->matrix = matrix;
    g->W = c.w << c.iterations; g->H = c.h << c.iterations;
    g->ow = sz ? sz->w : g->W; g->oh = sz ? sz->h : g->H;
    const ChromaSize ci = yuv_chroma_size(c.w, c.h, chroma), co = yuv_chroma_size(g->ow, g->oh, chroma);
    g->cw = ci.cw; g->ch = ci.ch; g->ocw = co.cw; g->och = co.ch;
    g->ax = chroma_axis(c.w, g->ow, chroma != W2XC_YUV_444, g->cosited & W2XC_CHROMA_COSITED_X);
    g->ay = chroma_axis(c.h, g->oh, chroma == W2XC_YUV_420, g->cosited & W2XC_CHROMA_COSITED_Y);
    std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> iv;
    if ((rc = check_yuv_side(in, g->bps, n, c.w, c.h, g->cw, g->ch, 0, iv)) || (rc = check_yuv_side(out, g->bps, n, g->ow, g->oh, g->ocw, g->och, 1, iv))) return rc;
    if ((rc = check_batch_overlap(iv))) return rc;
    c.fw = g->ow; c.fh = g->oh;
    const size_t per = (rgb ? yuv_rgb_aux_floats(c.mn != nullptr, c.w, c.h, c.iterations, g->ow, g->oh) : yuv_aux_floats(c.w, c.h, c.iterations, g->ow, g->oh)) *
                           sizeof(float) +
                       yuv_frame_bytes(c.w, c.h, g->cw, g->ch, g->bps) + yuv_frame_bytes(g->ow, g->oh, g->ocw, g->och, g->bps);
    return plan_image_call(rgb ? PLAN_RGB : PLAN_Y, c, sub, per, 1, g->bps == 2 ? "w2xc_process_frames_yuv_u16_rgb*" : "w2xc_process_frames_yuv_u8_rgb*");
}

// one side's luma planes, and the geometry of its chroma planes at U (V: the same strides from s.v), as the launchers take them: bytes, or words (strides in words)
W2xcU8Planes luma_planes(const YuvSide &s) { return {s.y, (long long)s.y_frame_stride, (long long)s.y_stride, 1}; }
W2xcU8Planes chroma_planes(const YuvSide &s) { return {s.u, (long long)s.c_frame_stride, (long long)s.c_stride, s.c_px}; }
unsigned short *words(unsigned char *p) { return reinterpret_cast<unsigned short *>(p); }
W2xcU16Planes luma_words(const YuvSide &s) { return {words(s.y), (long long)(s.y_frame_stride / 2), (long long)(s.y_stride / 2), 1, s.pack}; }
W2xcU16Planes chroma_words(const YuvSide &s) { return {words(s.u), (long long)(s.c_frame_stride / 2), (long long)(s.c_stride / 2), s.c_px, s.pack}; }

// ---- the ends of the two routes on n frames of one side: the ONE place where the sample width (g.bps) picks a launcher, and it picks by nothing else -- the siting
// (g.cosited) goes to the launcher every time, which decides it.  Routes and building blocks call these ----
// luma samples of w x h -> float planes ps floats apart, and back
hipError_t luma_in(const YuvGeom &g, const YuvSide &s, int w, int h, float *y, long long ps, int n, hipStream_t st)
{
    return g.bps == 2 ? w2xc_launch_y16_to_plane(luma_words(s), w, h, g.range, g.depth, y, ps, n, st) : w2xc_launch_y8_to_plane(luma_planes(s), w, h, g.range, y, ps, n, st);
}
hipError_t luma_out(const YuvGeom &g, const float *y, long long ps, int w, int h, const YuvSide &s, int n, hipStream_t st)
{
    return g.bps == 2 ? w2xc_launch_plane_to_y16(y, ps, w, h, g.range, g.depth, luma_words(s), n, st) : w2xc_launch_plane_to_y8(y, ps, w, h, g.range, luma_planes(s), n, st);
}
// chroma samples to chroma samples: g.cw x g.ch -> the leading g.ocw x g.och of the bicubic 2x, or (CHROMA_COPY) as they are, or (CHROMA_RESIZE) the
// g.ocw x g.och samples of the bicubic at g.ax / g.ay.  A null v: one plane per frame
hipError_t chroma_out(const YuvGeom &g, ChromaMode mode, const YuvSide &in, const YuvSide &out, int n, hipStream_t st)
{
    if (mode == CHROMA_RESIZE)
        return g.bps == 2 ? w2xc_launch_chroma_resize_u16(chroma_words(in), words(in.v), g.cw, g.ch, chroma_words(out), words(out.v), g.ocw, g.och, g.depth, g.ax.r, g.ax.o,
                                                           g.ay.r, g.ay.o, n, st)
                          : w2xc_launch_chroma_resize_u8(chroma_planes(in), in.v, g.cw, g.ch, chroma_planes(out), out.v, g.ocw, g.och, g.ax.r, g.ax.o, g.ay.r, g.ay.o, n, st);
    const bool up2x = mode == CHROMA_2X;
    if (g.bps == 2)
        return up2x ? w2xc_launch_chroma2x_u16(chroma_words(in), words(in.v), g.cw, g.ch, chroma_words(out), words(out.v), g.ocw, g.och, g.depth, g.cosited, n, st)
                    : w2xc_launch_chroma_copy_u16(chroma_words(in), words(in.v), g.cw, g.ch, chroma_words(out), words(out.v), g.depth, n, st);
    return up2x ? w2xc_launch_chroma2x_u8(chroma_planes(in), in.v, g.cw, g.ch, chroma_planes(out), out.v, g.ocw, g.och, g.cosited, n, st)
                : w2xc_launch_chroma_copy_u8(chroma_planes(in), in.v, g.cw, g.ch, chroma_planes(out), out.v, n, st);
}
// frames of w x h <-> their R, G, B planes (frame i's at rgb + i * is + {0, 1, 2} * ps floats) by g.matrix
hipError_t to_rgb(const YuvGeom &g, const YuvSide &s, int w, int h, float *rgb, long long is, long long ps, int n, hipStream_t st)
{
    return g.bps == 2 ? w2xc_launch_yuv16_to_rgb(luma_words(s), chroma_words(s), words(s.v), w, h, g.chroma | g.cosited, g.range, g.matrix, g.depth, rgb, is, ps, n, st)
                      : w2xc_launch_yuv8_to_rgb(luma_planes(s), chroma_planes(s), s.v, w, h, g.chroma | g.cosited, g.range, g.matrix, rgb, is, ps, n, st);
}
hipError_t from_rgb(const YuvGeom &g, const float *rgb, long long is, long long ps, int w, int h, const YuvSide &s, int n, hipStream_t st)
{
    return g.bps == 2 ? w2xc_launch_rgb_to_yuv16(rgb, is, ps, w, h, g.chroma | g.cosited, g.range, g.matrix, g.depth, luma_words(s), chroma_words(s), words(s.v), n, st)
                      : w2xc_launch_rgb_to_yuv8(rgb, is, ps, w, h, g.chroma | g.cosited, g.range, g.matrix, luma_planes(s), chroma_planes(s), s.v, n, st);
}

// What a frame call runs for its chroma: the samples as they are where the output has the input's size, the bicubic 2x kernels at exactly twice it (the resize
// kernels' arithmetic at r = 0.5 is theirs, byte for byte: the header says why), the resize kernels everywhere else
ChromaMode frame_chroma_mode(const ImageCall &c, const YuvGeom &g)
{
    if (g.ow == c.w && g.oh == c.h) return CHROMA_COPY;
    return g.ow == 2 * c.w && g.oh == 2 * c.h ? CHROMA_2X : CHROMA_RESIZE;
}

// A sub-batch of S frames (S <= cap, the call's sub-batch size: the planes are sized by cap): luma samples -> planes, the noise pass, the scale pass with the
// nearest-2x folded into layer 1 -- run_batch, so bands, precisions, named kernels and fusion settings are those of w2xc_convert_batch_device --, planes ->
// luma samples; chroma in ONE launch, samples to samples.  The ends are those of the sample width; everything between them is the same.
int process_yuv_device(const ImageCall &c, const YuvGeom &g, int S, int cap, const YuvSide &in, const YuvSide &out)
{
    DevCtx *own = c.ctx.owner();
    if (int rc = reserve_aux(own, 0, yuv_aux_floats(c.w, c.h, c.iterations, g.ow, g.oh) * (size_t)cap)) return rc;
    float *base = aux_planes(own, 0);
    int lw = c.w, lh = c.h;   // the level the luma planes are on
    long long ps = (long long)plane_floats(lw, lh);
    float *y = base, *yn = y + (size_t)cap * ps;
    base += 2 * (size_t)cap * ps;
    HIP_TRY(luma_in(g, in, c.w, c.h, y, ps, S, c.st));
    if (c.mn) {
        if (int rc = run_batch(c.mn, c.ctx.cn, S, 0, {y, (size_t)c.w, ps}, c.w, c.h, {yn, (size_t)c.w, ps}, c.st, c.o)) return rc;
        y = yn;
    }
    for (int it = 0; it < c.iterations; it++) {   // (unclipped between the passes; a level's share of the planes is two per frame, yuv_aux_floats)
        const int nw = 2 * lw, nh = 2 * lh;
        const long long ps2 = (long long)plane_floats(nw, nh);
        if (int rc = run_batch(c.msc, c.ctx.cs, S, 1, {y, (size_t)lw, ps}, lw, lh, {base, (size_t)nw, ps2}, c.st, c.o)) return rc;
        y = base; ps = ps2; lw = nw; lh = nh;
        base += 2 * (size_t)cap * ps2;
    }
    if (g.ow != lw || g.oh != lh) {   // a sized call below its last level: w2xc_resize_linear_device on every luma plane, ONE launch
        const long long pss = (long long)plane_floats(g.ow, g.oh);
        HIP_TRY(w2xc_launch_resize_linear_batch(y, y, S, ps, lw, lh, base, pss, g.ow, g.oh, S, c.st));
        y = base; ps = pss;
    }
    HIP_TRY(luma_out(g, y, ps, g.ow, g.oh, out, S, c.st));
    if (g.cw) HIP_TRY(chroma_out(g, frame_chroma_mode(c, g), in, out, S, c.st));
    return W2XC_OK;
}

// YUV frames through RGB models, a sub-batch of S frames: ONE launch from the frames' samples to three float planes per frame (k_yuv8_to_rgb / k_yuv16_to_rgb),
// the passes of process_rgb_device with float planes at both ends (rgb_passes: S >= 2 one run_batch_planes per pass, S = 1 run_rows, so bands work; a head model's
// pass enlarges by itself), ONE launch from the planes to the samples of the output frames (k_rgb_to_yuv8 / k_rgb_to_yuv16).
int process_yuv_rgb_device(const ImageCall &c, const YuvGeom &g, int S, int cap, const YuvSide &in, const YuvSide &out)
{
    DevCtx *own = c.ctx.owner();
    RgbPlan R;   // (float planes at both ends: no layer takes a uint8 image)
    R.floats = yuv_rgb_aux_floats(c.mn != nullptr, c.w, c.h, c.iterations, g.ow, g.oh);
    if (int rc = reserve_aux(own, 0, R.floats * (size_t)cap)) return rc;
    float *base = aux_planes(own, 0);
    RgbLevel L = {base, c.w, c.h, (long long)plane_floats(c.w, c.h)};
    base += 3 * (size_t)cap * L.ps;
    HIP_TRY(to_rgb(g, in, c.w, c.h, L.p, 3 * L.ps, L.ps, S, c.st));
    if (int rc = rgb_passes(c, R, S, cap, U8In{nullptr, 0, 0}, U8Out{nullptr, 0, 0}, 0, &base, nullptr, &L)) return rc;
    if (g.ow != L.w || g.oh != L.h) {   // a sized call below its last level: w2xc_resize_linear_device on the 3 S planes of the level (ps apart), ONE launch
        const long long pss = (long long)plane_floats(g.ow, g.oh);
        HIP_TRY(w2xc_launch_resize_linear_batch(L.p, L.p, 3 * S, L.ps, L.w, L.h, base, pss, g.ow, g.oh, 3 * S, c.st));
        L = {base, g.ow, g.oh, pss};
    }
    HIP_TRY(from_rgb(g, L.p, 3 * L.ps, L.ps, L.w, L.h, out, S, c.st));
    return W2XC_OK;
}

int process_yuv_sub_batch(const ImageCall &c, const YuvGeom &g, int S, int cap, const YuvSide &in, const YuvSide &out)
{
    return g.rgb ? process_yuv_rgb_device(c, g, S, cap, in, out) : process_yuv_device(c, g, S, cap, in, out);
}

// what a call names besides its models, its size and its planes.  rgb: w2xc_process_frames_yuv_*_rgb* (RGB and head models by the colour matrix `matrix`);
// otherwise the Y call, which has no matrix.  bps / depth: 1 / 8 for the calls on bytes, 2 / the call's depth for those on words
struct YuvCall {
    bool rgb;
    int n, chroma, range, matrix;
    int bps = 1, depth = 8;
    bool sized = false;   // w2xc_process_frames_yuv_*_sized*: the output frame is out_w x out_h, iterations 0 .. 4 or W2XC_ITERATIONS_AUTO
    int out_w = 0, out_h = 0;
};

// ... of a sized call
YuvCall sized_call(bool rgb, int n, int chroma, int range, int matrix, int bps, int depth, int out_w, int out_h)
{
    YuvCall k{rgb, n, chroma, range, matrix, bps, depth};
    k.sized = true; k.out_w = out_w; k.out_h = out_h;
    return k;
}

int frames_yuv_device(ImageCall c, const YuvCall &k, const YuvSide *in, const YuvSide *out)
{
    YuvGeom g;
    g.bps = k.bps; g.depth = k.depth;
    int sub = 1;
    const YuvOutSize sz = {k.out_w, k.out_h};
    int rc = check_yuv_call(c, k.rgb, k.n, k.chroma, k.range, k.matrix, in, out, &g, &sub, k.sized ? &sz : nullptr);
    if (rc) return rc;
    sub = std::min(sub, k.n);
    LockedCtx lc;
    if ((rc = lc.open(c.mn, c.msc, c.o.device))) return rc;
    c.ctx = lc;
    return for_sub_batches(k.n, sub, [&](int b0, int S) { return process_yuv_sub_batch(c, g, S, sub, yuv_from(*in, b0, g.cw != 0), yuv_from(*out, b0, g.cw != 0)); });
}

// The device copy of one side of a host call, at `at` in the image buffer, laid out as L (yuv_mirror_layout, w2xc_host_geom.hpp): the side's planes as pointers
struct YuvMirror {
    YuvSide d;
    size_t c_copy_row;   // bytes of a chroma row the copies move (both interleaved planes at once; 0: no chroma)
    bool pair;
};
YuvMirror yuv_mirror(const YuvSide &host, unsigned char *at, const YuvMirrorLayout &L)
{
    YuvMirror m{host, L.c_copy_row, L.pair};
    m.d.y = at;
    m.d.y_stride = L.y_stride;
    m.d.y_frame_stride = L.y_frame_stride;
    if (L.c_copy_row) { m.d.u = at + L.u; m.d.v = at + L.v; m.d.c_stride = L.c_stride; m.d.c_frame_stride = L.c_frame_stride; }
    return m;
}
// frames [b0, b0 + S) of the host side <-> the mirror's first S frames, blocking; row = the bytes of a luma row
int yuv_copy(const YuvMirror &m, const YuvSide &host, size_t b0, int S, size_t row, int h, int ch, bool upload)
{
    const hipMemcpyKind kind = upload ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    const auto copy = [&](unsigned char *dev, size_t dev_row, unsigned char *hst, size_t hst_row, size_t row_bytes, int rows) {
        return upload ? hipMemcpy2D(dev, dev_row, hst, hst_row, row_bytes, rows, kind) : hipMemcpy2D(hst, hst_row, dev, dev_row, row_bytes, rows, kind);
    };
    for (int i = 0; i < S; i++) {
        HIP_TRY(copy(m.d.y + i * m.d.y_frame_stride, m.d.y_stride, host.y + (b0 + i) * host.y_frame_stride, host.y_stride, row, h));
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

int frames_yuv_host(ImageCall c, const YuvCall &k, const YuvSide *in, const YuvSide *out)
{
    YuvGeom g;
    g.bps = k.bps; g.depth = k.depth;
    int sub = 1;
    const int n = k.n;
    const YuvOutSize sz = {k.out_w, k.out_h};
    int rc = check_yuv_call(c, k.rgb, n, k.chroma, k.range, k.matrix, in, out, &g, &sub, k.sized ? &sz : nullptr);
    if (rc) return rc;
    if (g.cw) for (const YuvSide *s : {in, out})
        if (s->c_px == 2 && s->v != s->u + g.bps && s->u != s->v + g.bps)
            return fail(W2XC_ERR_ARG, "host planes with c_px = 2: the two chroma planes must interleave (NV12: v = u + 1; NV21: u = v + 1)");
    sub = std::min(sub, n);
    std::vector<int> devs;
    if ((rc = host_devices(c.o, &devs))) return rc;
    LockedCtx lc;
    if ((rc = lc.open(c.mn, c.msc, devs[0]))) return rc;
    c.ctx = lc;
    c.st = nullptr;
    DevCtx *own = c.ctx.owner();
    const YuvMirrorLayout li = yuv_mirror_layout(in->c_px, in->u < in->v, sub, c.w, c.h, g.cw, g.ch, g.bps),
                          lo = yuv_mirror_layout(out->c_px, out->u < out->v, sub, g.ow, g.oh, g.ocw, g.och, g.bps);
    if ((rc = own->img_io.reserve(li.bytes + lo.bytes, "the frames"))) return rc;
    unsigned char *dev = own->img_io.as<unsigned char>();
    YuvMirror mi = yuv_mirror(*in, dev, li), mo = yuv_mirror(*out, dev + li.bytes, lo);
    return for_sub_batches(n, sub, [&](int b0, int S) {
        if (int r = yuv_copy(mi, *in, b0, S, (size_t)c.w * g.bps, c.h, g.ch, true)) return r;
        if (int r = process_yuv_sub_batch(c, g, S, sub, mi.d, mo.d)) { hipDeviceSynchronize(); return r; }
        HIP_TRY(hipDeviceSynchronize());
        return yuv_copy(mo, *out, b0, S, (size_t)g.ow * g.bps, g.oh, g.och, false);
    });
}

// the call forms on either struct of the interface
template <class Planes> int frames_yuv(bool host, const ImageCall &c, const YuvCall &k, const Planes *in, const Planes *out)
{
    YuvSide si, so;
    const YuvSide *pi = side_of(in, &si), *po = side_of(out, &so);
    return host ? frames_yuv_host(c, k, pi, po) : frames_yuv_device(c, k, pi, po);
}

// what the two blocks of the RGB route refuse: the frames' side as check_yuv_side refuses it, the 3 n float planes, and the two sides overlapping
int check_yuv_rgb_block_args(const YuvSide *f, int bps, int depth, bool f_is_out, int n, int w, int h, int chroma, int range, int matrix, const float *rgb,
                             size_t image_stride_bytes, size_t plane_stride_bytes, int *cosited)
{
    if (!f || !rgb) return fail(W2XC_ERR_ARG, "null argument");
    if (n < 1 || n > (1 << 20) || w <= 0 || h <= 0 || w > (1 << 22) || h > (1 << 22)) return fail(W2XC_ERR_ARG, "bad frame count / frame size");
    if (chroma == W2XC_YUV_400) return fail(W2XC_ERR_ARG, "a frame without chroma (W2XC_YUV_400) has no colour to convert");
    if (int rc = check_chroma_range(chroma, range, &chroma, cosited)) return rc;
    if (int rc = check_depth(bps, depth)) return rc;
    if (int rc = check_matrix(matrix)) return rc;
    const size_t plane = (size_t)4 * w * h;
    if ((image_stride_bytes & 3) || (plane_stride_bytes & 3) || plane_stride_bytes < plane || (n > 1 && image_stride_bytes < 2 * plane_stride_bytes + plane))
        return fail(W2XC_ERR_ARG, "plane / image strides: multiples of 4, a plane stride of at least a plane, an image stride of at least three planes");
    const ChromaSize cs = yuv_chroma_size(w, h, chroma);
    std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> iv;
    if (int rc = check_yuv_side(f, bps, n, w, h, cs.cw, cs.ch, f_is_out ? 1 : 0, iv)) return rc;
    for (int i = 0; i < n; i++) for (int p = 0; p < 3; p++) {
        const uintptr_t at = (uintptr_t)rgb + i * image_stride_bytes + p * plane_stride_bytes;
        iv.push_back({{at, at + plane}, f_is_out ? 0 : 1});
    }
    return check_batch_overlap(iv);
}

// what the three building blocks of the Y route refuse: n planes of samples (bps bytes each) of row_bytes-byte rows x `rows` at p and n planes of `other` bytes (rows /
// planes as given) on the other side
int check_yuv_block_args(const void *p, size_t frame, size_t row, size_t row_bytes, int rows, int n, int w, int h, const void *q, size_t q_plane, size_t q_ext, int bps)
{
    if (!p || !q) return fail(W2XC_ERR_ARG, "null argument");
    if (n < 1 || n > (1 << 20) || w <= 0 || h <= 0 || w > (1 << 22) || h > (1 << 22)) return fail(W2XC_ERR_ARG, "bad plane count / plane size");
    const size_t ext = (size_t)(rows - 1) * row + row_bytes;
    if (row < row_bytes || (n > 1 && (frame < ext || q_plane < q_ext))) return fail(W2XC_ERR_ARG, "row / plane strides below a row / a plane");
    if (bps == 2 && (((uintptr_t)p | row | frame) & 1)) return fail(W2XC_ERR_ARG, "16-bit samples need an even pointer and even strides");
    if (ranges_overlap(p, (size_t)(n - 1) * frame + ext, q, (size_t)(n - 1) * q_plane + q_ext)) return fail(W2XC_ERR_ARG, "source and destination overlap");
    return W2XC_OK;
}
// ... and of their other arguments: the float planes' stride, the range, and for words the depth and the packing
int check_luma_block_format(size_t plane_stride_bytes, int range, int bps, int depth, int pack)
{
    if ((plane_stride_bytes & 3) || (range != W2XC_RANGE_FULL && range != W2XC_RANGE_LIMITED)) return fail(W2XC_ERR_ARG, "plane stride no multiple of 4 / unknown range");
    if (pack != W2XC_PACK_LOW && pack != W2XC_PACK_HIGH) return fail(W2XC_ERR_ARG, "pack must be W2XC_PACK_LOW or W2XC_PACK_HIGH, got %d", pack);
    return check_depth(bps, depth);
}

// ---- the bodies of the building blocks: a block on bytes and its twin on words are ONE of these, told apart by bps, depth and the packs (bytes: 1, 8,
// W2XC_PACK_LOW).  out: float planes -> samples ----
template <class Planes>
int yuv_rgb_block(bool out, const Planes *frames, int bps, int depth, int n, int w, int h, int chroma, int range, int matrix, float *d_rgb, size_t image_stride_bytes,
                  size_t plane_stride_bytes, void *hip_stream)
{
    YuvSide store;
    const YuvSide *s = side_of(frames, &store);
    YuvGeom g;   // (the format alone: what the ends take)
    if (int rc = check_yuv_rgb_block_args(s, bps, depth, out, n, w, h, chroma, range, matrix, d_rgb, image_stride_bytes, plane_stride_bytes, &g.cosited)) return rc;
    g.bps = bps; g.depth = depth; g.range = range; g.chroma = chroma & 0xF; g.matrix = matrix;
    const long long is = (long long)(image_stride_bytes / 4), ps = (long long)(plane_stride_bytes / 4);
    HIP_TRY(out ? from_rgb(g, d_rgb, is, ps, w, h, *s, n, (hipStream_t)hip_stream) : to_rgb(g, *s, w, h, d_rgb, is, ps, n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int luma_block(bool out, const void *samples, int bps, int depth, int pack, int n, size_t frame_stride_bytes, size_t stride_bytes, int w, int h, int range,
               const float *planes, size_t plane_stride_bytes, void *hip_stream)
{
    const size_t W = w > 0 ? w : 1, H = h > 0 ? h : 1;
    if (int rc = check_yuv_block_args(samples, frame_stride_bytes, stride_bytes, bps * W, h, n, w, h, planes, plane_stride_bytes, 4 * W * H, bps)) return rc;
    if (int rc = check_luma_block_format(plane_stride_bytes, range, bps, depth, pack)) return rc;
    YuvSide s;
    s.y = static_cast<unsigned char *>(const_cast<void *>(samples)); s.y_frame_stride = frame_stride_bytes; s.y_stride = stride_bytes; s.pack = pack;
    YuvGeom g;
    g.bps = bps; g.depth = depth; g.range = range;
    const long long ps = (long long)(plane_stride_bytes / 4);
    HIP_TRY(out ? luma_out(g, planes, ps, w, h, s, n, (hipStream_t)hip_stream) : luma_in(g, s, w, h, const_cast<float *>(planes), ps, n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

int chroma2x_block(const void *d_src, int bps, int depth, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw, int ch,
                   void *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack, int ow, int oh, int cosited, void *hip_stream)
{
    if (int rc = check_cosited(cosited, true, true)) return rc;
    if ((src_px != 1 && src_px != 2) || (dst_px != 1 && dst_px != 2)) return fail(W2XC_ERR_ARG, "src_px / dst_px must be 1 or 2");
    if (ow < 1 || oh < 1 || ow > 2 * (long long)cw || oh > 2 * (long long)ch) return fail(W2XC_ERR_ARG, "the output size lies outside the 2x enlargement");
    const size_t drow = chroma_row_bytes(ow, dst_px, bps), dext = (size_t)(oh - 1) * dst_stride_bytes + drow;
    if (dst_stride_bytes < drow) return fail(W2XC_ERR_ARG, "row / plane strides below a row / a plane");
    if (int rc = check_yuv_block_args(d_src, src_frame_stride_bytes, src_stride_bytes, chroma_row_bytes(cw > 0 ? cw : 1, src_px, bps), ch, n, cw, ch, d_dst, dst_frame_stride_bytes, dext, bps)) return rc;
    if (bps == 2 && (((uintptr_t)d_dst | dst_stride_bytes | dst_frame_stride_bytes) & 1)) return fail(W2XC_ERR_ARG, "16-bit samples need an even pointer and even strides");
    if ((src_pack != W2XC_PACK_LOW && src_pack != W2XC_PACK_HIGH) || (dst_pack != W2XC_PACK_LOW && dst_pack != W2XC_PACK_HIGH))
        return fail(W2XC_ERR_ARG, "src_pack / dst_pack must be W2XC_PACK_LOW or W2XC_PACK_HIGH");
    if (int rc = check_depth(bps, depth)) return rc;
    YuvSide in, to;   // one plane per frame: no v
    in.u = static_cast<unsigned char *>(const_cast<void *>(d_src)); in.c_frame_stride = src_frame_stride_bytes; in.c_stride = src_stride_bytes; in.c_px = src_px; in.pack = src_pack;
    to.u = static_cast<unsigned char *>(d_dst); to.c_frame_stride = dst_frame_stride_bytes; to.c_stride = dst_stride_bytes; to.c_px = dst_px; to.pack = dst_pack;
    YuvGeom g;
    g.bps = bps; g.depth = depth; g.cw = cw; g.ch = ch; g.ocw = ow; g.och = oh; g.cosited = cosited;
    HIP_TRY(chroma_out(g, CHROMA_2X, in, to, n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

// w2xc_chroma_resize_u8_device / _u16_device: chroma2x_block at any ratio -- the luma sizes of both sides give the ratios, the layout's two subsampling flags
// with `cosited` the offsets.  Always the resize kernels, at r = 1 and r = 0.5 too
int chroma_resize_block(const void *d_src, int bps, int depth, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw, int ch,
                        void *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack, int ow, int oh, int w, int h, int out_w, int out_h,
                        int sub_x, int sub_y, int cosited, void *hip_stream)
{
    if ((sub_x != 0 && sub_x != 1) || (sub_y != 0 && sub_y != 1)) return fail(W2XC_ERR_ARG, "sub_x / sub_y must be 0 or 1");
    if (int rc = check_cosited(cosited, sub_x != 0, sub_y != 0)) return rc;
    if ((src_px != 1 && src_px != 2) || (dst_px != 1 && dst_px != 2)) return fail(W2XC_ERR_ARG, "src_px / dst_px must be 1 or 2");
    if (w < 1 || h < 1 || out_w < w || out_h < h || out_w > (1 << 22) || out_h > (1 << 22))
        return fail(W2XC_ERR_ARG, "the luma sizes: %d x %d -> %d x %d (at least 1, at most 2^22, the output never smaller than the input)", w, h, out_w, out_h);
    if (ow < 1 || oh < 1 || ow > (1 << 22) || oh > (1 << 22)) return fail(W2XC_ERR_ARG, "bad output plane size");
    const size_t drow = chroma_row_bytes(ow, dst_px, bps), dext = (size_t)(oh - 1) * dst_stride_bytes + drow;
    if (dst_stride_bytes < drow) return fail(W2XC_ERR_ARG, "row / plane strides below a row / a plane");
    if (int rc = check_yuv_block_args(d_src, src_frame_stride_bytes, src_stride_bytes, chroma_row_bytes(cw > 0 ? cw : 1, src_px, bps), ch, n, cw, ch, d_dst, dst_frame_stride_bytes, dext, bps)) return rc;
    if (bps == 2 && (((uintptr_t)d_dst | dst_stride_bytes | dst_frame_stride_bytes) & 1)) return fail(W2XC_ERR_ARG, "16-bit samples need an even pointer and even strides");
    if ((src_pack != W2XC_PACK_LOW && src_pack != W2XC_PACK_HIGH) || (dst_pack != W2XC_PACK_LOW && dst_pack != W2XC_PACK_HIGH))
        return fail(W2XC_ERR_ARG, "src_pack / dst_pack must be W2XC_PACK_LOW or W2XC_PACK_HIGH");
    if (int rc = check_depth(bps, depth)) return rc;
    YuvSide in, to;   // one plane per frame: no v
    in.u = static_cast<unsigned char *>(const_cast<void *>(d_src)); in.c_frame_stride = src_frame_stride_bytes; in.c_stride = src_stride_bytes; in.c_px = src_px; in.pack = src_pack;
    to.u = static_cast<unsigned char *>(d_dst); to.c_frame_stride = dst_frame_stride_bytes; to.c_stride = dst_stride_bytes; to.c_px = dst_px; to.pack = dst_pack;
    YuvGeom g;
    g.bps = bps; g.depth = depth; g.cw = cw; g.ch = ch; g.ocw = ow; g.och = oh; g.cosited = cosited;
    g.ax = chroma_axis(w, out_w, sub_x != 0, cosited & W2XC_CHROMA_COSITED_X);
    g.ay = chroma_axis(h, out_h, sub_y != 0, cosited & W2XC_CHROMA_COSITED_Y);
    HIP_TRY(chroma_out(g, CHROMA_RESIZE, in, to, n, (hipStream_t)hip_stream));
    return W2XC_OK;
}

}  // namespace

}  // namespace w2xc_eng

using namespace w2xc_eng;

extern "C" {

// ---- YUV frames: luma through the models, chroma 2x on bytes ----
int w2xc_process_frames_yuv_u8_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *d_in,
                                      const w2xc_yuv_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), {false, n, chroma, range, 0}, d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u8(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *in,
                               const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), {false, n, chroma, range, 0}, in, out);
} W2XC_CATCH_ALL

// ---- YUV frames through RGB and head models, by a colour matrix ----
int w2xc_process_frames_yuv_u8_rgb_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                          const w2xc_yuv_planes *d_in, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), {true, n, chroma, range, matrix}, d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u8_rgb(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix, const w2xc_yuv_planes *in,
                                   const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), {true, n, chroma, range, matrix}, in, out);
} W2XC_CATCH_ALL

// ---- 16-bit YUV frames: the same four calls on words ----
int w2xc_process_frames_yuv_u16_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth,
                                       const w2xc_yuv16_planes *d_in, const w2xc_yuv16_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), {false, n, chroma, range, 0, 2, depth}, d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u16(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, const w2xc_yuv16_planes *in,
                                const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), {false, n, chroma, range, 0, 2, depth}, in, out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u16_rgb_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                           const w2xc_yuv16_planes *d_in, const w2xc_yuv16_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), {true, n, chroma, range, matrix, 2, depth}, d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u16_rgb(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                    const w2xc_yuv16_planes *in, const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), {true, n, chroma, range, matrix, 2, depth}, in, out);
} W2XC_CATCH_ALL

// ---- the two ends of the RGB route (yuv_rgb_block) ----
int w2xc_yuv8_to_rgb_device(const w2xc_yuv_planes *d_src, int n, int w, int h, int chroma, int range, int matrix, float *d_rgb, size_t image_stride_bytes,
                            size_t plane_stride_bytes, void *hip_stream)
try {
    return yuv_rgb_block(false, d_src, 1, 8, n, w, h, chroma, range, matrix, d_rgb, image_stride_bytes, plane_stride_bytes, hip_stream);
} W2XC_CATCH_ALL

int w2xc_rgb_to_yuv8_device(const float *d_rgb, size_t image_stride_bytes, size_t plane_stride_bytes, int n, int w, int h, int chroma, int range, int matrix,
                            const w2xc_yuv_planes *d_dst, void *hip_stream)
try {
    return yuv_rgb_block(true, d_dst, 1, 8, n, w, h, chroma, range, matrix, const_cast<float *>(d_rgb), image_stride_bytes, plane_stride_bytes, hip_stream);
} W2XC_CATCH_ALL

int w2xc_yuv16_to_rgb_device(const w2xc_yuv16_planes *d_src, int n, int w, int h, int chroma, int range, int depth, int matrix, float *d_rgb, size_t image_stride_bytes,
                             size_t plane_stride_bytes, void *hip_stream)
try {
    return yuv_rgb_block(false, d_src, 2, depth, n, w, h, chroma, range, matrix, d_rgb, image_stride_bytes, plane_stride_bytes, hip_stream);
} W2XC_CATCH_ALL

int w2xc_rgb_to_yuv16_device(const float *d_rgb, size_t image_stride_bytes, size_t plane_stride_bytes, int n, int w, int h, int chroma, int range, int depth, int matrix,
                             const w2xc_yuv16_planes *d_dst, void *hip_stream)
try {
    return yuv_rgb_block(true, d_dst, 2, depth, n, w, h, chroma, range, matrix, const_cast<float *>(d_rgb), image_stride_bytes, plane_stride_bytes, hip_stream);
} W2XC_CATCH_ALL

// ---- the building blocks of the Y route (luma_block, chroma2x_block) ----
int w2xc_y8_to_plane_device(const unsigned char *d_src, int n, size_t frame_stride_bytes, size_t stride_bytes, int w, int h, int range, float *d_dst,
                            size_t plane_stride_bytes, void *hip_stream)
{
    return luma_block(false, d_src, 1, 8, W2XC_PACK_LOW, n, frame_stride_bytes, stride_bytes, w, h, range, d_dst, plane_stride_bytes, hip_stream);
}

int w2xc_plane_to_y8_device(const float *d_src, int n, size_t plane_stride_bytes, int w, int h, int range, unsigned char *d_dst, size_t frame_stride_bytes,
                            size_t stride_bytes, void *hip_stream)
{
    return luma_block(true, d_dst, 1, 8, W2XC_PACK_LOW, n, frame_stride_bytes, stride_bytes, w, h, range, d_src, plane_stride_bytes, hip_stream);
}

int w2xc_chroma2x_u8_device(const unsigned char *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int cw, int ch,
                            unsigned char *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int ow, int oh, void *hip_stream)
{
    return chroma2x_block(d_src, 1, 8, n, src_frame_stride_bytes, src_stride_bytes, src_px, W2XC_PACK_LOW, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px,
                          W2XC_PACK_LOW, ow, oh, 0, hip_stream);
}

int w2xc_chroma2x_u8_sited_device(const unsigned char *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int cw, int ch,
                                  unsigned char *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int ow, int oh, int cosited,
                                  void *hip_stream)
{
    return chroma2x_block(d_src, 1, 8, n, src_frame_stride_bytes, src_stride_bytes, src_px, W2XC_PACK_LOW, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px,
                          W2XC_PACK_LOW, ow, oh, cosited, hip_stream);
}

int w2xc_y16_to_plane_device(const unsigned short *d_src, int n, size_t frame_stride_bytes, size_t stride_bytes, int w, int h, int range, int depth, int pack,
                             float *d_dst, size_t plane_stride_bytes, void *hip_stream)
{
    return luma_block(false, d_src, 2, depth, pack, n, frame_stride_bytes, stride_bytes, w, h, range, d_dst, plane_stride_bytes, hip_stream);
}

int w2xc_plane_to_y16_device(const float *d_src, int n, size_t plane_stride_bytes, int w, int h, int range, int depth, int pack, unsigned short *d_dst,
                             size_t frame_stride_bytes, size_t stride_bytes, void *hip_stream)
{
    return luma_block(true, d_dst, 2, depth, pack, n, frame_stride_bytes, stride_bytes, w, h, range, d_src, plane_stride_bytes, hip_stream);
}

int w2xc_chroma2x_u16_device(const unsigned short *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw, int ch,
                             int depth, unsigned short *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack, int ow, int oh,
                             void *hip_stream)
{
    return chroma2x_block(d_src, 2, depth, n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px,
                          dst_pack, ow, oh, 0, hip_stream);
}

int w2xc_chroma2x_u16_sited_device(const unsigned short *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw,
                                   int ch, int depth, unsigned short *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack,
                                   int ow, int oh, int cosited, void *hip_stream)
{
    return chroma2x_block(d_src, 2, depth, n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes, dst_px,
                          dst_pack, ow, oh, cosited, hip_stream);
}

// ---- Sized YUV frames: the eight frame calls with an output size, several 2x steps and W2XC_ITERATIONS_AUTO; the resize of chroma as a block ----
int w2xc_process_frames_yuv_u8_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *d_in,
                                            int out_w, int out_h, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream, const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), sized_call(false, n, chroma, range, 0, 1, 8, out_w, out_h), d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u8_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, const w2xc_yuv_planes *in, int out_w,
                                     int out_h, const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), sized_call(false, n, chroma, range, 0, 1, 8, out_w, out_h), in, out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u8_rgb_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                                const w2xc_yuv_planes *d_in, int out_w, int out_h, const w2xc_yuv_planes *d_out, int iterations, void *hip_stream,
                                                const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), sized_call(true, n, chroma, range, matrix, 1, 8, out_w, out_h), d_in,
                      d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u8_rgb_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int matrix,
                                         const w2xc_yuv_planes *in, int out_w, int out_h, const w2xc_yuv_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), sized_call(true, n, chroma, range, matrix, 1, 8, out_w, out_h), in, out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u16_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth,
                                             const w2xc_yuv16_planes *d_in, int out_w, int out_h, const w2xc_yuv16_planes *d_out, int iterations, void *hip_stream,
                                             const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), sized_call(false, n, chroma, range, 0, 2, depth, out_w, out_h), d_in,
                      d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u16_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth,
                                      const w2xc_yuv16_planes *in, int out_w, int out_h, const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), sized_call(false, n, chroma, range, 0, 2, depth, out_w, out_h), in, out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u16_rgb_sized_device(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                                 const w2xc_yuv16_planes *d_in, int out_w, int out_h, const w2xc_yuv16_planes *d_out, int iterations, void *hip_stream,
                                                 const w2xc_opts *opts)
try {
    return frames_yuv(false, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, hip_stream, opts), sized_call(true, n, chroma, range, matrix, 2, depth, out_w, out_h),
                      d_in, d_out);
} W2XC_CATCH_ALL

int w2xc_process_frames_yuv_u16_rgb_sized(w2xc_model *noise_model, w2xc_model *scale_model, int n, int w, int h, int chroma, int range, int depth, int matrix,
                                          const w2xc_yuv16_planes *in, int out_w, int out_h, const w2xc_yuv16_planes *out, int iterations, const w2xc_opts *opts)
try {
    return frames_yuv(true, ImageCall(noise_model, scale_model, w, h, iterations, 0.0, nullptr, opts), sized_call(true, n, chroma, range, matrix, 2, depth, out_w, out_h), in,
                      out);
} W2XC_CATCH_ALL

int w2xc_chroma_resize_u8_device(const unsigned char *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int cw, int ch,
                                 unsigned char *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int ow, int oh, int w, int h, int out_w,
                                 int out_h, int sub_x, int sub_y, int cosited, void *hip_stream)
{
    return chroma_resize_block(d_src, 1, 8, n, src_frame_stride_bytes, src_stride_bytes, src_px, W2XC_PACK_LOW, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes,
                               dst_px, W2XC_PACK_LOW, ow, oh, w, h, out_w, out_h, sub_x, sub_y, cosited, hip_stream);
}

int w2xc_chroma_resize_u16_device(const unsigned short *d_src, int n, size_t src_frame_stride_bytes, size_t src_stride_bytes, int src_px, int src_pack, int cw, int ch,
                                  int depth, unsigned short *d_dst, size_t dst_frame_stride_bytes, size_t dst_stride_bytes, int dst_px, int dst_pack, int ow, int oh,
                                  int w, int h, int out_w, int out_h, int sub_x, int sub_y, int cosited, void *hip_stream)
{
    return chroma_resize_block(d_src, 2, depth, n, src_frame_stride_bytes, src_stride_bytes, src_px, src_pack, cw, ch, d_dst, dst_frame_stride_bytes, dst_stride_bytes,
                               dst_px, dst_pack, ow, oh, w, h, out_w, out_h, sub_x, sub_y, cosited, hip_stream);
}

}  // extern "C"
