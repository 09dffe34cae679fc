// w2xc_rows.cpp -- the band loop that replaces convertWithModels / convertWithModelsBasic / convertWithModelsBlockSplit
// (src/convertRoutine.cpp:21-169) on MI355X, and the device-pointer entry points of include/w2xc_hip.h.
//
// Data layout in HBM: two ping-pong workspaces per (model, device) sized for one band; each boundary between layers picks
// NHWC or planar fp32 (resolve_chain, w2xc_select.cpp); layer 1 reads the caller's planar plane with clamp-to-edge
// addressing (= copyMakeBorder, convertRoutine.cpp:35,96) and the last layer writes the planar output rows in place
// (= crop + stitch, :40-46,143-161).  A band is `band_rows` output rows x full width; layer k of n computes a valid conv
// on the haloed band (SURVEY invariants I1/I2).
#include "w2xc_engine.hpp"
#include "w2xc_cuts.hpp"
#include <cmath>
#include <iostream>

namespace w2xc_eng {

namespace {

// a weight image packed on first use: *img = the device copy of the `floats` floats pack(dst) fills
template <class F> int packed(float **img, size_t floats, F &&pack)
{
    if (*img) return W2XC_OK;
    std::vector<float> pk(floats);
    pack(pk.data());
    return upload(pk, img);
}

// conv3x3_split / conv3x3_first2_split: the term-plane images of layer l (index terms + 3 * fmt) and, fused, of the last layer behind it
int split_weights(DevCtx *c, const w2xc_model *m, int l, W2xcKernelKind kind, W2xcConvDesc &d)
{
    DevLayer &dl = c->layers[l];
    if (d.terms < 1 || d.terms > 3 || d.fmt < 0 || d.fmt > 1) return fail(W2XC_ERR_ARG, "bad term count %d / format %d", d.terms, d.fmt);
    const int wi = d.terms + 3 * d.fmt;
    int rc = packed(&dl.w_split[wi], (w2xc_split_packed_bytes(d.cin, d.cout, d.terms) + 3) / 4,
                    [&](float *pk) { dl.split_scale[wi] = w2xc_split_pack(d.cin, d.cout, d.terms, d.fmt, m->layers[l].w.data(), pk); });
    if (rc) return rc;
    d.wpk = dl.w_split[wi];
    d.acc_scale = 1.0f / dl.split_scale[wi];
    if (kind == W2XC_K_FIRST2_SPLIT) {
        d.w1pk = c->layers[l - 1].w_fast;
        d.bias1 = c->layers[l - 1].bias;
    }
    if (d.out_terms != 9) return W2XC_OK;
    // the next (last) layer's weights ride along
    DevLayer &nl = c->layers[l + 1];
    const int nin = m->layers[l + 1].nin;
    const int lt = d.terms, li = d.terms == 3 ? 2 : d.terms == 1 ? 3 : d.fmt;   // the fused product uses the mode's own term count
    rc = packed(&nl.w_last_fused[li], (w2xc_split_pack_last_bytes(nin, lt) + 3) / 4,
                [&](float *pk) { nl.last_fused_scale[li] = w2xc_split_pack_last(nin, lt, d.fmt, m->layers[l + 1].w.data(), pk); });
    d.w7pk = nl.w_last_fused[li];
    d.g_scale = 1.0f / nl.last_fused_scale[li];
    return rc;
}

// the launcher of a kind (midv: which kernel runs a W2XC_K_MFMA layer); bd = the batch form, for the kinds that have one
hipError_t launch_kind(W2xcKernelKind kind, int midv, const W2xcConvDesc &d, const W2xcBatchDesc *bd, hipStream_t st)
{
    switch (kind) {
    case W2XC_K_LAST_GATHER: return bd ? w2xc_launch_last_gather_batch(d, *bd, st) : w2xc_launch_last_gather(d, st);
    case W2XC_K_FIRST2_WINO4: return bd ? w2xc_launch_first2_wino4_batch(d, *bd, st) : w2xc_launch_first2_wino4(d, st);
    case W2XC_K_MID_SPLIT: return bd ? hipErrorInvalidValue : w2xc_launch_split_mid(d, st);
    case W2XC_K_FIRST_SPLIT: return bd ? hipErrorInvalidValue : w2xc_launch_split_first(d, st);
    case W2XC_K_FIRST2_SPLIT: return bd ? hipErrorInvalidValue : w2xc_launch_first2_split(d, st);
    case W2XC_K_FIRST:
    case W2XC_K_FIRST_U8:
    case W2XC_K_LAST:
    case W2XC_K_LAST_U8: return bd ? w2xc_launch_conv_batch(kind, d, *bd, st) : w2xc_launch_conv(kind, d, st);
    case W2XC_K_UPCONV:
    case W2XC_K_UPCONV_U8:
    case W2XC_K_UPCONV_A_U8:
    case W2XC_K_UPCONV_A: return bd ? w2xc_launch_upconv_batch(kind, d, *bd, st) : w2xc_launch_upconv(kind, d, st);
    default: break;
    }
    if (midv == MID_WINO4) return bd ? w2xc_launch_wino4_batch(d, *bd, st) : w2xc_launch_wino4(d, st);
    if (midv == MID_WINO32) return bd ? w2xc_launch_wino_batch(d, *bd, st) : w2xc_launch_wino(d, st);
    return bd ? hipErrorInvalidValue : w2xc_launch_conv(kind, d, st);
}

}  // namespace

int launch_layer(DevCtx *c, const w2xc_model *m, int l, W2xcKernelKind kind, int midv, W2xcConvDesc d, hipStream_t st, const w2xc_opts &o, const W2xcBatchDesc *bd)
{
    DevLayer &dl = c->layers[l];
    d.cin = m->layers[l].nin;
    d.cout = m->layers[l].nout;
    int rc = W2XC_OK;
    switch (kind) {
    case W2XC_K_FUSED_AWAY: return W2XC_OK;   // computed by the next layer's W2XC_K_FIRST2_SPLIT / W2XC_K_FIRST2_WINO4 launch
    case W2XC_K_MID_SPLIT:
    case W2XC_K_FIRST2_SPLIT: rc = split_weights(c, m, l, kind, d); break;
    case W2XC_K_LAST_GATHER: d.wpk = nullptr; break;
    case W2XC_K_FIRST2_WINO4:
        rc = packed(&dl.w_first2, (size_t)36 * d.cin * d.cout, [&](float *pk) { w2xc_first2_wino4_pack(m->layers[l].w.data(), pk); });
        d.wpk = dl.w_first2;
        d.w1pk = c->layers[l - 1].w_fast;
        d.bias1 = c->layers[l - 1].bias;
        break;
    case W2XC_K_UPCONV_A:
    case W2XC_K_UPCONV_A_U8:   // the alpha head: channel 1 of the three-plane head as a one-plane head of its own (its image: get_ctx)
        if (d.cout != 3 || !dl.w_alpha) return fail(W2XC_ERR_ARG, "internal error: the alpha head of a layer that is no three-plane upconv head");
        d.cout = 1;
        d.wpk = dl.w_alpha;
        break;
    default: d.wpk = kind == W2XC_K_DIRECT ? dl.w_direct : dl.w_fast;
    }
    if (!rc && midv != MID_MFMA) {   // the fp32 Winograd images of a mid layer
        const float *w = m->layers[l].w.data();
        rc = midv == MID_WINO4 ? packed(&dl.w_wino4, (size_t)36 * d.cin * d.cout, [&](float *pk) { w2xc_wino4_pack(d.cin, d.cout, w, pk); })
                               : packed(&dl.w_wino, w2xc_wino_packed_floats(d.cin, d.cout), [&](float *pk) { w2xc_wino_pack(d.cin, d.cout, w, pk); });
        d.wpk = midv == MID_WINO4 ? dl.w_wino4 : dl.w_wino;
        if (!rc && d.out_terms == 9) {   // the next (last) layer's weights ride along (the fp32 last-layer fusion)
            const HostLayer &hn = m->layers[l + 1];
            rc = packed(&c->layers[l + 1].w_last_wino4, w2xc_wino4_pack_last_floats(hn.nin), [&](float *pk) { w2xc_wino4_pack_last(hn.nin, hn.w.data(), pk); });
            d.w7pk = c->layers[l + 1].w_last_wino4;
        }
    }
    if (rc) return rc;
    d.bias = kind == W2XC_K_UPCONV_A_U8 || kind == W2XC_K_UPCONV_A ? dl.bias + 1 : dl.bias;
    ProfEvent ev;
    const bool profile = o.profile != 0;
    if (profile) { rc = prof_begin(c, l, st, &ev); if (rc) return rc; }
    // (the seam of w2xc_debug_fail_nth: nothing is launched, an error code stands where the launcher's would)
    hipError_t e = fail_event(W2XC_DEBUG_FAIL_LAUNCH) ? hipErrorLaunchFailure : launch_kind(kind, midv, d, bd, st);
    if (e == hipSuccess && profile) e = hipEventRecord(ev.b, st);
    if (e != hipSuccess && profile) c->pool.push_back(ev);   // the pair of a launch that did not happen measures nothing: back to the pool, not to `pending`
    if (e != hipSuccess) return fail(W2XC_ERR_HIP, "launch of %s (layer %d, %d->%d) failed: %s", w2xc_kernel_name(kind, d.cin, d.cout), l, d.cin, d.cout, hipGetErrorString(e));
    if (profile) c->pending.push_back(ev);
    return W2XC_OK;
}

namespace {

// what the launch strategies of one band [y0, y1) of a run_rows call share
struct Band {
    w2xc_model *m; DevCtx *c; const RowPlan &P; const BandHooks *hk; hipStream_t st;
    float *out;   // the caller's rows of this band: row stride out_rs, planes out_cs apart
    long long out_rs, out_cs;
    int y0, y1, rb;
    int in_chunk;   // > 0: layer 1 (or the fused layers 1 + 2) runs in chunks of this many rows behind the upload (first_chunks)
    int u8;         // ROWS_U8_SRC / ROWS_U8_DST: the view / `out` is an interleaved uint8 image, its strides are in bytes (no hooks: every launch is the plain one)
    // run_batch_planes: > 0 = every launch is the batch form on this many images of the band's geometry (no hooks: every launch is the plain one), image i in_bs /
    // out_bs floats (a uint8 view / `out`: bytes) behind image 0 in the caller's planes and img_f[j] floats behind it in workspace j
    int batch = 0;
    long long in_bs = 0, out_bs = 0;
    size_t img_f[2] = {0, 0};

    int launch(int k, W2xcKernelKind kind, const W2xcConvDesc &d) const
    {
        const int midv = P.chain.layer[k - 1].midv;
        if (!batch) return launch_layer(c, m, k - 1, kind, midv, d, st, P.o);
        // the image strides of layer k: the first launched layer reads the caller's planes, layer n writes them; layer j < n writes workspace (j - 1) & 1
        W2xcBatchDesc bd;
        memset(&bd, 0, sizeof bd);
        bd.batch = batch;
        const bool first = k == 1 || (k == 2 && P.chain.layer[0].kind == W2XC_K_FUSED_AWAY);
        bd.in_bs = first ? in_bs : (long long)img_f[(k - 2) & 1];
        bd.out_bs = k == P.n ? out_bs : (long long)img_f[(k - 1) & 1];
        return launch_layer(c, m, k - 1, kind, midv, d, st, P.o, &bd);
    }
    // stage the next band's input while this one computes
    int prefetch() const { return (hk && hk->prefetch && y1 < rb) ? hk->prefetch(y1, std::min(rb, y1 + P.band)) : W2XC_OK; }
};

// rows [p0, p1) of the launch d (offsets move with them; plane / half strides stay those of the whole band)
W2xcConvDesc rows_of(const W2xcConvDesc &d, int p0, int p1)
{
    W2xcConvDesc dd = d;
    dd.out_h = p1 - p0;
    dd.off_y = d.off_y + p0;
    dd.out = d.out + (size_t)p0 * d.out_rs;
    return dd;
}

// the last layer's launch for output rows [a, b) of the band behind the launch d of layer n - 1: row y reads d's rows y + off .. y + off + 2
W2xcConvDesc last_rows_of(const Band &B, const W2xcConvDesc &d, int off, int a, int b)
{
    W2xcConvDesc dg;
    memset(&dg, 0, sizeof dg);
    dg.in = d.out; dg.in_rs = d.out_rs; dg.in_ps = d.out_ps; dg.in_cs = d.out_cs;
    dg.in_ts = d.out_ts; dg.in_gs = d.out_gs; dg.halves = d.halves; dg.fmt = d.fmt;
    dg.in_h = d.out_h; dg.in_w = d.out_w;
    dg.off_y = off + a;
    if (d.out_terms == 9) {   // the gather has no offsets: its input view starts at the partial planes' row off + a
        dg.in += (size_t)(off + a) * d.out_rs;
        dg.in_h = b - a + 2;
        dg.off_y = 0;
    }
    dg.out_h = b - a; dg.out_w = B.P.w;
    dg.out = B.out + (size_t)a * B.out_rs;
    dg.out_rs = B.out_rs; dg.out_ps = 1; dg.out_cs = B.out_cs;
    return dg;
}

// prog -- fp32, the launch of layer n - 1 FINISHES the fused one-plane last layer itself, rows completing top to bottom while it runs (conv3x3_wino4 PROG):
//   * host pipeline (hk->prog_begin): ONE launch of layer n - 1, no gather launch, no chunking -- its gather jobs write the band's output rows
//     straight into page-locked host memory and flag them; the drainer ships rows while the launch is still running (the 0.15-0.25 ms that
//     three chunked launches of the persistent kernel cost, the six gather launches and their events are gone: DESIGN 7);
//   * device entry points: only on request (w2xc_opts.fusion = W2XC_FUSION_PROG) -- with planes resident nothing waits for rows, and the launch
//     is 0.2 ms slower than layer n - 1 + its gather launch (the row-ordered walk, the write-through tap planes).
// Bit-identical to the gather launch either way (same sum, same order).
bool prog_eligible(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    const RowPlan &P = B.P;
    return P.chain.T == 0 && k == P.n - 1 && kind == W2XC_K_MFMA && d.out_terms == 9 && P.last_kind == W2XC_K_LAST_GATHER && P.last_direct && !P.all_out && d.in_ps == 1 &&
           P.chain.prog_gather && P.w >= 4 && (long long)d.out_h * d.out_rs * 4 < (1ll << 32) &&
           ((B.hk && B.hk->prog_begin) || (!B.hk && P.o.fusion == W2XC_FUSION_PROG));
}
// *launched = false: the hook has no page-locked band buffer to hand out, another strategy runs the layer
int run_prog(const Band &B, int k, W2xcKernelKind kind, W2xcConvDesc &d, int Tk, bool *launched)
{
    DevCtx *c = B.c;
    const BandHooks *hk = B.hk;
    int trows = 0, groups = 0;
    w2xc_wino4_prog_jobs(d.out_w, d.out_h, d.wino_py, &trows, &groups);
    BandHooks::ProgTail pt;
    pt.out = B.out;
    pt.out_stride_f = B.out_rs;
    if (hk) {
        pt.out = nullptr;
        int rc = hk->prog_begin(B.y0, B.y1, trows, groups, &pt);
        if (rc) return rc;
    }
    *launched = pt.out != nullptr;
    if (!pt.out) return W2XC_OK;
    const size_t nc = w2xc_wino4_prog_counters(d.out_w, d.out_h, d.wino_py);
    int rc = c->prog_cnt.reserve(nc * sizeof(unsigned), "the gather-job counters");
    if (rc) return rc;
    d.prog_cnt = c->prog_cnt.as<unsigned>();
    d.g_out = pt.out;
    d.g_out_rs = pt.out_stride_f;
    d.g_h = B.y1 - B.y0;
    d.g_w = B.P.w;
    d.g_off = B.y0 - 1 - Tk;   // rows of this launch's region above the last layer's first input row
    d.g_bias = c->layers[B.P.n - 1].bias;
    d.prog_flags = pt.flags;
    d.prog_epoch = pt.epoch;
    rc = B.prefetch();
    if (rc) return rc;
    rc = B.launch(k, kind, d);
    if (rc) return rc;
    // job (tile row jr, group jg) holds the output rows [16 jr - first, 16 jr - first + 16) (clipped to the band) x columns [256 jg, 256 jg + 256)
    return (hk && hk->prog_launched) ? hk->prog_launched(B.y0, B.y1, trows, groups, d.wino_py + d.g_off) : W2XC_OK;
}

// tail16 -- 16-bit modes, host pipeline: the last layer lives in layer n-1's epilogue + a 0.2 ms gather, too short to hide the band's download behind.
// So layer n-1 and the gather run TOGETHER in row chunks (cut_tail16).
// (16-bit producers only: conv3x3_wino4's fused epilogue wants chunks on whole 16-row tiles of ITS block grid -- tail32 below)
bool tail16_eligible(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    const RowPlan &P = B.P;
    const BandHooks *hk = B.hk;
    return hk && P.HL == 1 && k == P.n - 1 && P.n >= 3 && kind == W2XC_K_MID_SPLIT && d.out_terms == 9 && P.last_direct && hk->out_chunk_rows > 0 &&
           hk->output_ready && (B.y1 - B.y0) >= 128;
}
int run_tail16(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    int rc = B.prefetch();
    if (rc) return rc;
    return cut_tail16(
        B.y1 - B.y0, [&](int g0, int g1) { return B.launch(k, kind, rows_of(d, g0, g1)); },
        [&](int a, int b) {
            int r = B.launch(B.P.n, W2XC_K_LAST_GATHER, last_rows_of(B, d, 0, a, b));
            return r ? r : B.hk->output_ready(B.y0 + a, B.y0 + b);
        });
}

// tail32 -- fp32, host pipeline, no PROG: the last layer (0.8 ms on the 2160x3840 frame; fused: conv3x3_wino4's epilogue + the gather) is too short to hide
// the band's 33 MB download + stitch behind.  So layer n-1 and the last layer run TOGETHER in row chunks (cut_tail32): chunk j's output rows leave for the
// host under layer n-1 of chunk j+1.  The producer chunks are whole 16-row tiles of the SAME tile grid as the unchunked launch (bit-identical results,
// nothing is computed twice); the last layer follows two rows behind (it reads rows y .. y + 2 of the producer's region).
bool tail32_eligible(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    const RowPlan &P = B.P;
    const BandHooks *hk = B.hk;
    const bool tail_unfused = d.out_terms == 0 && P.last_kind == W2XC_K_LAST;
    const bool tail_fused4 = d.out_terms == 9 && P.last_kind == W2XC_K_LAST_GATHER && P.chain.layer[k - 1].wino4;
    return hk && P.chain.T == 0 && k == P.n - 1 && P.n >= 2 && kind == W2XC_K_MFMA && (tail_unfused || tail_fused4) && P.last_direct && hk->out_chunk_rows > 0 &&
           hk->output_ready && (B.y1 - B.y0) >= 256;
}
int run_tail32(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d, int Tk)
{
    int rc = B.prefetch();
    if (rc) return rc;
    const int off_l = B.y0 - 1 - Tk;   // rows of the producer's region above the last layer's first input row (0 on the one-row-per-layer geometry)
    const int items_per_row = ((d.out_w + 31) / 32) * std::max(1, B.m->layers[k - 1].nout / 64);
    return cut_tail32(
        d.out_h, B.y1 - B.y0, off_l, items_per_row, [&](int p0, int p1) { return B.launch(k, kind, rows_of(d, p0, p1)); },
        [&](int a, int b) {
            int r = B.launch(B.P.n, B.P.last_kind, last_rows_of(B, d, off_l, a, b));
            return r ? r : B.hk->output_ready(B.y0 + a, B.y0 + b);
        });
}

// first_chunks -- layer 1 (or layers 1 + 2 in one launch) in row chunks while the band's input is still arriving: the upload of rows [c0 + 2 + off_y ...] and
// layer 1 of the rows before them overlap: what stays exposed of the input side is the first slice and the last chunk, not upload + layer 1 back to back.
// (Layers 1 + 2 in one launch: the same, two rows deeper; chunks of whole 8-row tiles keep the 4x4 blocks where the unchunked launch has them.)
bool first_chunks_eligible(const Band &B, int k, W2xcKernelKind kind) { return (k == 1 || kind == W2XC_K_FIRST2_WINO4) && B.in_chunk > 0; }
int run_first_chunks(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    for (int c0 = 0, step = 0; c0 < d.out_h; c0 += step) {
        const int at = B.hk->in_chunk_at ? B.hk->in_chunk_at(c0) : 0;   // (the first chunks of a call may be shorter: BandHooks)
        step = at > 0 ? std::max(8, at & ~7) : B.in_chunk;
        const int rows = std::min(step, d.out_h - c0);
        int rc = B.hk->input_upto(first_chunk_last_row(c0, rows, kind == W2XC_K_FIRST2_WINO4, d.wino_py, d.off_y, d.in_h));
        if (rc) return rc;
        rc = B.launch(k, kind, rows_of(d, c0, c0 + rows));
        if (rc) return rc;
    }
    return W2XC_OK;
}

// last_chunks -- the last layer in row chunks (cut_taper): chunk j's rows leave for the host while chunk j+1 is computed
bool last_chunks_eligible(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    const BandHooks *hk = B.hk;
    return hk && k == B.P.n && B.P.last_direct && hk->out_chunk_rows > 0 && d.out_h > std::max(hk->out_chunk_min, 8) &&
           (kind == W2XC_K_LAST || kind == W2XC_K_LAST_GATHER || kind == W2XC_K_DIRECT);
}
int run_last_chunks(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    return cut_taper(d.out_h, B.hk->out_chunk_rows, B.hk->out_chunk_min, [&](int c0, int cr) {
        W2xcConvDesc dd = rows_of(d, c0, c0 + cr);
        if (kind == W2XC_K_LAST_GATHER) { dd.in = d.in + (size_t)c0 * d.in_rs; dd.off_y = d.off_y; }   // no offsets in that kernel
        int rc = B.launch(k, kind, dd);
        return (rc || !B.hk->output_ready) ? rc : B.hk->output_ready(B.y0 + c0, B.y0 + c0 + cr);
    });
}

// plain -- one launch for the layer's whole region; a last layer that cannot store planar goes through the workspace + a repack
int run_plain(const Band &B, int k, W2xcKernelKind kind, const W2xcConvDesc &d)
{
    const BandHooks *hk = B.hk;
    int rc = B.launch(k, kind, d);
    if (rc || k < B.P.n) return rc;
    if (!B.P.last_direct) {
        // outputPlanes[0] of a multi-plane last layer (convertRoutine.cpp:78)
        hipError_t e = w2xc_launch_repack(d.out, d.out_rs, d.out_ps, 1, B.out, B.out_rs, 1, B.out_cs, d.out_h, d.out_w, B.P.all_out ? B.m->layers[k - 1].nout : 1, B.st);
        if (e != hipSuccess) return fail(W2XC_ERR_HIP, "repack launch failed: %s", hipGetErrorString(e));
    }
    return (hk && hk->output_ready) ? hk->output_ready(B.y0, B.y1) : W2XC_OK;
}

// the layers of one band: build the layer's descriptor, pick ONE strategy for it (in this order), run it, move on to what it wrote
int run_band(Band &B, const LayerSrc &view, int up)
{
    const w2xc_model *m = B.m;
    const BandHooks *hk = B.hk;
    const RowPlan &P = B.P;
    const w2xc_opts &o = P.o;
    const int n = P.n;
    // a batched band is one plain launch per layer: every other strategy needs hooks or W2XC_FUSION_PROG, the repack a last layer that cannot store planar
    // (batch_eligible lets none of them through; nothing is launched otherwise)
    if (B.batch && (hk || o.fusion == W2XC_FUSION_PROG || !P.last_direct))
        return fail(W2XC_ERR_ARG, "internal error: a batched band that is not one plain launch per layer");
    // layer 1 of this band in row chunks (each waits only for the rows it reads) or in one launch behind the whole upload
    const W2xcKernelKind kind1 = P.chain.layer[0].kind;
    const bool first2_fp32 = kind1 == W2XC_K_FUSED_AWAY && n > 1 && P.chain.layer[1].kind == W2XC_K_FIRST2_WINO4;   // (layers 1 + 2 in one launch: chunked like layer 1)
    B.in_chunk = (hk && hk->in_chunk && hk->input_upto && n > 1 && (kind1 == W2XC_K_FIRST || kind1 == W2XC_K_DIRECT || first2_fp32)) ? hk->in_chunk(B.y0, B.y1) : 0;
    if (hk && hk->input_needed && B.in_chunk <= 0) { int rc = hk->input_needed(B.y0, B.y1); if (rc) return rc; }
    const LayerDst dst = {B.out, B.out_rs, B.out_cs, {B.c->ws[0].as<float>(), B.c->ws[1].as<float>()}};
    LayerSrc src = view, next;
    W2xcConvDesc first_d, d;
    memset(&first_d, 0, sizeof first_d);
    for (int k = 1; k <= n; k++, src = next) {
        if ((o.verbose & 1) && !B.batch) std::cout << "Iteration #" << k << "..." << std::endl;   // convertRoutine.cpp:67
        W2xcKernelKind kind = layer_desc(m, P, k, B.y0, B.y1, up, src, dst, first_d, &d, &next);
        if (kind == W2XC_K_FUSED_AWAY) continue;
        // the uint8 forms (run_rows has checked the kinds they stand in for): the descriptor's strides are the image's, in bytes
        if (k == 1 && (B.u8 & ROWS_U8_SRC)) kind = W2XC_K_FIRST_U8;
        if (k == n && (B.u8 & ROWS_U8_DST)) {
            // (a head's sink may be RGBA pixels, and the alpha head one byte of them: check_u8_views lets neither through for conv3x3_last)
            kind = kind != W2XC_K_UPCONV ? W2XC_K_LAST_U8 : (B.u8 & ROWS_U8_DST_A) ? W2XC_K_UPCONV_A_U8 : W2XC_K_UPCONV_U8;
            d.out_ps = (B.u8 & ROWS_U8_DST_PX4) ? 4 : 3;
        }
        if (k == n && (B.u8 & ROWS_F32_DST_A)) kind = W2XC_K_UPCONV_A;   // (check_u8_views: the last layer is a three-plane head)
        const int Tk = next.top;   // first plane row of the layer's region
        // the strategies that run layer n - 1 and the last layer together end the band
        if (prog_eligible(B, k, kind, d)) {
            bool launched = false;
            int rc = run_prog(B, k, kind, d, Tk, &launched);
            if (rc || launched) return rc;
        }
        if (tail16_eligible(B, k, kind, d)) return run_tail16(B, k, kind, d);
        if (tail32_eligible(B, k, kind, d)) return run_tail32(B, k, kind, d, Tk);
        int rc = k == n ? B.prefetch() : W2XC_OK;
        if (rc) return rc;
        rc = first_chunks_eligible(B, k, kind)      ? run_first_chunks(B, k, kind, d)
             : last_chunks_eligible(B, k, kind, d) ? run_last_chunks(B, k, kind, d)
                                                   : run_plain(B, k, kind, d);
        if (rc) return rc;
    }
    return W2XC_OK;
}

}  // namespace

// the uint8 views of a call planned as P: no hooks, channels one byte apart, and the layers they touch have the uint8 kernels
static int check_u8_views(const w2xc_model *m, const RowPlan &P, int u8, bool hooks, long long in_ps, long long out_ps)
{
    if (u8 && (hooks || ((u8 & ROWS_U8_SRC) && (in_ps != ((u8 & ROWS_U8_SRC_A) ? 0 : 1) || !P.chain.u8_source)) ||
               ((u8 & ROWS_U8_DST) && (out_ps != 1 || !P.last_direct || !P.chain.u8_sink))))
        return fail(W2XC_ERR_ARG, "internal error: a uint8 view for a layer without the uint8 kernel");
    // the forms of the RGBA head call: each beside the flag of its side, the sink's only where the last layer is a head (the alpha head: a three-plane one)
    const bool src_a = (u8 & ROWS_U8_SRC_A) != 0, dst_x = (u8 & (ROWS_U8_DST_PX4 | ROWS_U8_DST_A)) != 0, dst_fa = (u8 & ROWS_F32_DST_A) != 0;
    const bool head3 = P.last_kind == W2XC_K_UPCONV && m->layers[P.n - 1].nout == 3;
    if ((src_a && !(u8 & ROWS_U8_SRC)) || (dst_x && (!(u8 & ROWS_U8_DST) || !head3)) || (dst_fa && ((u8 & ROWS_U8_DST) || hooks || !P.last_direct || !head3)))
        return fail(W2XC_ERR_ARG, "internal error: an RGBA pixel view for a layer without that form");
    return W2XC_OK;
}

// one call of the band loop (RowsCall, w2xc_engine.hpp): plan, reserve the workspaces, run_band per band
int run_rows(w2xc_model *m, DevCtx *c, const RowsCall &r, hipStream_t st, const w2xc_opts &o_in)
{
    RowPlan P;
    if (int rc = plan_rows(m, o_in, r.w, r.view_h, r.view_y0, r.ra, r.rb, r.plane_h, r.n_in, r.out.ps != 0, &P)) return rc;
    if (int rc = check_u8_views(m, P, r.u8, r.hk != nullptr, r.in.ps, r.out.ps)) return rc;
    if (m->has_head() && (r.hk || r.up)) return fail(W2XC_ERR_ARG, "internal error: an upconv head model behind hooks or a nearest-2x");
    for (int i = 0; i < 2; i++)
        if (P.need[i]) { int rc = c->ws[i].reserve((P.need[i] + 3) / 4 * sizeof(float), "the activation workspace"); if (rc) return rc; }
    LayerSrc view;   // the source view; its first row is plane row view_y0
    view.p = r.in.p; view.rs = (long long)r.in.rs; view.cs = r.in.ps;
    view.h = r.view_h; view.w = r.w; view.top = r.view_y0;
    if (r.u8 & ROWS_U8_SRC) view.ps = (r.u8 & ROWS_U8_SRC_A) ? 4 : 3;   // (bytes: row stride in.rs, pixels 3 apart, channels in.ps = 1 apart; the alpha byte of RGBA pixels: 4 and 0)
    const size_t out_rows_per_row = m->has_head() ? 2 : 1;   // (an upconv head model: ra, rb and the bands count SOURCE rows, each gives two output rows)
    for (int y0 = r.ra; y0 < r.rb; y0 += P.band) {
        // the band's first output row: out.rs floats per row, or -- a uint8 image -- as many BYTES
        const size_t row0 = (size_t)(y0 - r.ra) * out_rows_per_row;
        float *band_out = (r.u8 & ROWS_U8_DST) ? reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(r.out.p) + row0 * r.out.rs) : r.out.p + row0 * r.out.rs;
        Band B = {m, c, P, r.hk, st, band_out, (long long)r.out.rs, r.out.ps, y0, std::min(r.rb, y0 + P.band), r.rb, 0, r.u8};
        if (int rc = run_band(B, view, r.up)) return rc;
    }
    return W2XC_OK;
}

// what the one-plane device calls refuse: a w x h plane (view) in, rows (w << up) wide out
static int check_plane_args(const w2xc_model *m, const void *in, size_t in_stride, int w, int h, const void *out, size_t out_stride, int up = 0)
{
    if (!m || !in || !out) return fail(W2XC_ERR_ARG, "null argument");
    if (int rc = refuse_head(m, "w2xc_convert_plane* / w2xc_convert_rows_device")) return rc;
    if (int rc = check_plane_size(w, h, false)) return rc;
    return check_row_strides(in_stride, w, out_stride, (size_t)w << up);
}

int check_planes_args(const w2xc_model *m, int up, int n_in_planes, const void *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h,
                      const void *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes, const w2xc_opts &o)
{
    if (!m || !d_in || !d_out) return fail(W2XC_ERR_ARG, "null argument");
    // up = 2: w2xc_convert_planes_up2x_device -- a head model, and only there; the output planes are 2w x 2h as with up = 1
    if (up == 2 ? !m->has_head() : m->has_head())
        return up == 2 ? fail(W2XC_ERR_ARG, "w2xc_convert_planes_up2x[_batch]_device: the model has no upconv head") : refuse_head(m, "w2xc_convert_planes[_nn2x][_batch]_device");
    up = up ? 1 : 0;
    if (int rc = check_plane_size(w, h, up != 0)) return rc;
    const int W = w << up, H = h << up;
    if (int rc = check_row_strides(in_stride_bytes, w, out_stride_bytes, W)) return rc;
    if (n_in_planes < 1 || (in_plane_stride_bytes & 3) || (out_plane_stride_bytes & 3) ||
        (n_in_planes > 1 && in_plane_stride_bytes < in_stride_bytes * (size_t)h) || out_plane_stride_bytes < out_stride_bytes * (size_t)H)
        return fail(W2XC_ERR_ARG, "bad plane count / plane strides");
    if (o.precision != W2XC_PRECISION_FP32 && split_terms(o) == 0)
        return fail(W2XC_ERR_UNSUPPORTED, "w2xc_convert_planes_* supports W2XC_PRECISION_FP32 / BF16X2 / BF16X3 / FP16X2");
    return W2XC_OK;
}

// nimg images of one size (w2xc_convert_batch*: one plane each; w2xc_convert_planes_batch_device and the RGB image calls: io.n_in planes in, all planes of
// the last layer out).  The plan is that of ONE image, exactly as the single-image device call makes it.  Where a batched chain
// applies (batch_eligible), a sub-batch of k images is run_band on ONE batched band [0, H): one launch per layer, the descriptor of every launch the
// single-image one (same regions, offsets, wino_py, clamps, strides), and the batch kernels add image x stride (Band::launch) to their scalar bases -- input
// planes, the k per-image blocks of the two workspaces, output planes.  Everything else runs the single-image launch sequence per image on the same stream
// (no host synchronisation in between).
int run_batch_planes(w2xc_model *m, DevCtx *c, int nimg, int up, const BatchIO &io, int w, int h, hipStream_t st, const w2xc_opts &o_in, int max_sub)
{
    const int W = w << up, H = h << up;
    RowPlan P;
    if (int rc = plan_rows(m, o_in, W, H, 0, 0, H, H, io.n_in, io.out.ps != 0, &P)) return rc;
    // image i's view: its stride is floats, or -- a uint8 image -- bytes
    const auto image_in = [&](size_t i) -> PlanesIn {
        if (io.u8 & ROWS_U8_SRC) return {reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(io.in.p) + i * (size_t)io.in_is), io.in.rs, io.in.ps};
        return {io.in.p + i * (size_t)io.in_is, io.in.rs, io.in.ps};
    };
    const auto image_out = [&](size_t i) -> PlanesOut {
        if (io.u8 & ROWS_U8_DST) return {reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(io.out.p) + i * (size_t)io.out_is), io.out.rs, io.out.ps};
        return {io.out.p + i * (size_t)io.out_is, io.out.rs, io.out.ps};
    };
    if (!batch_eligible(m, P)) {
        for (int i = 0; i < nimg; i++)
            if (int rc = run_rows(m, c, RowsCall::whole(image_in(i), io.n_in, W, H, image_out(i), up, io.u8), st, o_in)) return rc;
        return W2XC_OK;
    }
    if (int rc = check_u8_views(m, P, io.u8, false, io.in.ps, io.out.ps)) return rc;
    size_t img_f[2];
    batch_ws_floats(P, img_f);
    int sub = batch_sub_size(P.o, img_f);
    if (max_sub > 0 && sub > max_sub) sub = max_sub;
    if (sub > nimg) sub = nimg;
    for (int i = 0; i < 2; i++)
        if (img_f[i]) { int rc = c->ws[i].reserve(img_f[i] * (size_t)sub * sizeof(float), "the activation workspace"); if (rc) return rc; }

    for (int b0 = 0; b0 < nimg; b0 += sub) {
        const PlanesIn in0 = image_in(b0);
        Band B = {m, c, P, nullptr, st, image_out(b0).p, (long long)io.out.rs, io.out.ps, 0, H, H, 0, io.u8};
        B.batch = std::min(sub, nimg - b0); B.in_bs = io.in_is; B.out_bs = io.out_is;
        B.img_f[0] = img_f[0]; B.img_f[1] = img_f[1];
        LayerSrc view;   // (as run_rows makes it: the W x H plane, also where up = 1)
        view.p = in0.p; view.rs = (long long)in0.rs; view.cs = in0.ps; view.h = H; view.w = W;
        if (io.u8 & ROWS_U8_SRC) view.ps = (io.u8 & ROWS_U8_SRC_A) ? 4 : 3;
        if (int rc = run_band(B, view, up)) return rc;
    }
    return W2XC_OK;
}

// one plane in, one plane out per image: plane i at in.p + i * in.ps
int run_batch(w2xc_model *m, DevCtx *c, int nimg, int up, PlanesIn in, int w, int h, PlanesOut out, hipStream_t st, const w2xc_opts &o_in, int max_sub)
{
    const BatchIO io = {{in.p, in.rs, 0}, in.ps, 1, {out.p, out.rs, 0}, out.ps, 0};
    return run_batch_planes(m, c, nimg, up, io, w, h, st, o_in, max_sub);
}

// the argument checks of the batch entry points (no device is touched): n >= 1, sizes, strides, planes that do not overlap.  head_call: the call is
// w2xc_convert_planes_up2x_batch_device, which runs a head model (and nothing else: check_planes_args); its nn2x is 1, the size of what it writes
int check_batch_args(const w2xc_model *m, int nimg, int nn2x, int w, int h, size_t in_stride, size_t out_stride, bool head_call)
{
    if (!m) return fail(W2XC_ERR_ARG, "null model");
    if (!head_call) if (int rc = refuse_head(m, "the batch calls")) return rc;
    if (nimg < 1) return fail(W2XC_ERR_ARG, "batch of %d planes", nimg);
    if (nn2x != 0 && nn2x != 1) return fail(W2XC_ERR_ARG, "nn2x must be 0 or 1");
    if (int rc = check_plane_size(w, h, true)) return rc;
    return check_row_strides(in_stride, w, out_stride, (size_t)w << nn2x);
}

// everything w2xc_convert_batch_device refuses
int check_batch_device_args(const w2xc_model *m, int n, int nn2x, const void *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h,
                            const void *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes)
{
    if (int rc = check_batch_args(m, n, nn2x, w, h, in_stride_bytes, out_stride_bytes)) return rc;
    if (!d_in || !d_out) return fail(W2XC_ERR_ARG, "null argument");
    if ((in_plane_stride_bytes & 3) || (out_plane_stride_bytes & 3)) return fail(W2XC_ERR_ARG, "plane strides must be multiples of 4 bytes");
    const int H = h << nn2x, W = w << nn2x;
    const size_t in_ext = image_extent(h, in_stride_bytes, w, 4), out_ext = image_extent(H, out_stride_bytes, W, 4);
    if (n > 1 && out_plane_stride_bytes < out_ext) return fail(W2XC_ERR_ARG, "output planes overlap each other (plane stride %zu < %zu bytes)", out_plane_stride_bytes, out_ext);
    if (ranges_overlap(d_in, (size_t)(n - 1) * in_plane_stride_bytes + in_ext, d_out, (size_t)(n - 1) * out_plane_stride_bytes + out_ext))
        return fail(W2XC_ERR_ARG, "output planes overlap the input planes");
    return check_batch_model(m);
}

// everything w2xc_convert_planes_batch_device refuses: check_batch_args + check_planes_args, the plane counts, and images that overlap
int check_planes_batch_device_args(const w2xc_model *m, int n, int nn2x, int n_in_planes, const void *d_in, size_t in_image_stride_bytes, size_t in_plane_stride_bytes,
                                   size_t in_stride_bytes, int w, int h, const void *d_out, size_t out_image_stride_bytes, size_t out_plane_stride_bytes,
                                   size_t out_stride_bytes, const w2xc_opts &o, bool head_call)
{
    if (head_call) nn2x = 1;   // (the head's own 2x: the output planes are 2w x 2h as with a nearest-2x)
    if (int rc = check_batch_args(m, n, nn2x, w, h, in_stride_bytes, out_stride_bytes, head_call)) return rc;
    if (int rc = check_planes_args(m, head_call ? 2 : nn2x, n_in_planes, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes, o)) return rc;
    if (head_call && o.precision != W2XC_PRECISION_FP32) return fail(W2XC_ERR_UNSUPPORTED, "16-bit precision modes: not available for a model with an upconv head (W2XC_PRECISION_FP32 only)");
    if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    if (m->layers[0].nin != n_in_planes)
        return fail(W2XC_ERR_PLANES, "Error : Model-filter : \nnumber of input planes mismatch.\n%d,%d", n_in_planes, m->layers[0].nin);
    if ((in_image_stride_bytes & 3) || (out_image_stride_bytes & 3)) return fail(W2XC_ERR_ARG, "image strides must be multiples of 4 bytes");
    const int H = h << nn2x, W = w << nn2x, nout = m->layers.back().nout;
    const size_t in_ext = (size_t)(n_in_planes - 1) * in_plane_stride_bytes + image_extent(h, in_stride_bytes, w, 4);
    const size_t out_ext = (size_t)(nout - 1) * out_plane_stride_bytes + image_extent(H, out_stride_bytes, W, 4);
    if (n > 1 && out_image_stride_bytes < out_ext)
        return fail(W2XC_ERR_ARG, "output images overlap each other (image stride %zu < %zu bytes)", out_image_stride_bytes, out_ext);
    if (ranges_overlap(d_in, (size_t)(n - 1) * in_image_stride_bytes + in_ext, d_out, (size_t)(n - 1) * out_image_stride_bytes + out_ext))
        return fail(W2XC_ERR_ARG, "output images overlap the input images");
    return W2XC_OK;
}

// [lo, hi) byte ranges: does any output overlap another output or any input?  (inputs may share memory with each other)
int check_batch_overlap(std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> &iv)
{
    std::sort(iv.begin(), iv.end());
    uintptr_t end_out = 0, end_in = 0;
    for (const auto &e : iv) {
        const uintptr_t lo = e.first.first, hi = e.first.second;
        if (lo < end_out || (e.second && lo < end_in)) return fail(W2XC_ERR_ARG, "output planes overlap each other or an input plane");
        if (e.second) end_out = std::max(end_out, hi);
        else end_in = std::max(end_in, hi);
    }
    return W2XC_OK;
}

}  // namespace w2xc_eng

using namespace w2xc_eng;

// what every device entry point does behind its argument checks: open the model's locked context on the call's device (LockedCtx), then enqueue
static int rows_on_device(w2xc_model *m, const RowsCall &r, void *hip_stream, const w2xc_opts &o)
{
    LockedCtx lc;
    if (int rc = lc.open(nullptr, m, o.device)) return rc;
    return run_rows(m, lc.cs, r, (hipStream_t)hip_stream, o);
}

extern "C" {

// ---- hot path -------------------------------------------------------------------------------------
int w2xc_convert_plane_device(w2xc_model *m, const float *d_in, size_t in_stride_bytes, int w, int h, float *d_out,
                              size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    if (int rc = check_plane_args(m, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes)) return rc;
    const w2xc_opts o = resolve_opts(opts);
    return rows_on_device(m, RowsCall::whole({d_in, in_stride_bytes / 4, 0}, 1, w, h, {d_out, out_stride_bytes / 4, 0}, 0), hip_stream, o);
} W2XC_CATCH_ALL

int w2xc_convert_rows_device(w2xc_model *m, const float *d_view, size_t view_stride_bytes, int view_h, int view_y0, int w,
                             int plane_h, int row_begin, int row_end, float *d_out, size_t out_stride_bytes,
                             void *hip_stream, const w2xc_opts *opts)
try {
    if (int rc = check_plane_args(m, d_view, view_stride_bytes, w, view_h, d_out, out_stride_bytes)) return rc;
    const int n = (int)m->layers.size();
    if (plane_h <= 0 || row_begin < 0 || row_end > plane_h || row_begin >= row_end)
        return fail(W2XC_ERR_ARG, "bad row range [%d,%d) for a %d-row plane", row_begin, row_end, plane_h);
    if (view_y0 < 0 || view_y0 + view_h > plane_h || view_y0 > std::max(0, row_begin - n) ||
        view_y0 + view_h < std::min(plane_h, row_end + n))
        return fail(W2XC_ERR_ARG, "view rows [%d,%d) do not cover [%d,%d) +- %d halo rows", view_y0, view_y0 + view_h,
                    row_begin, row_end, n);
    const w2xc_opts o = resolve_opts(opts);
    // a view that starts/ends inside the plane has artificial edges, but every row within n of
    // them lies outside [row_begin, row_end), so clamping there never reaches a kept output row
    // (conv3x3_wino4, the F(4x4) kernel: a view with 4 n halo rows gets its banding-invariant geometry; on a narrower one
    //  W2XC_KERNEL_AUTO runs the F(2x2) kernels: run_rows)
    RowsCall r = RowsCall::whole({d_view, view_stride_bytes / 4, 0}, 1, w, plane_h, {d_out, out_stride_bytes / 4, 0}, 0);
    r.view_h = view_h; r.view_y0 = view_y0; r.ra = row_begin; r.rb = row_end;
    return rows_on_device(m, r, hip_stream, o);
} W2XC_CATCH_ALL

// w2xc_convert_planes_device (up = 0) and its nearest-2x form (up = 1: (w, h) is the SOURCE size, the output planes are 2w x 2h)
static int convert_planes(w2xc_model *m, int up, int n_in_planes, const float *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h,
                          float *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
{
    const int W = w << up, H = h << up;
    const w2xc_opts o = resolve_opts(opts);
    if (int rc = check_planes_args(m, up, n_in_planes, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes, o))
        return rc;
    const PlanesIn in{d_in, in_stride_bytes / 4, (long long)(in_plane_stride_bytes / 4)};
    return rows_on_device(m, RowsCall::whole(in, n_in_planes, W, H, {d_out, out_stride_bytes / 4, (long long)(out_plane_stride_bytes / 4)}, up), hip_stream, o);
}

int w2xc_convert_planes_device(w2xc_model *m, int n_in_planes, const float *d_in, size_t in_plane_stride_bytes,
                               size_t in_stride_bytes, int w, int h, float *d_out, size_t out_plane_stride_bytes,
                               size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    return convert_planes(m, 0, n_in_planes, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes, hip_stream, opts);
} W2XC_CATCH_ALL

int w2xc_convert_planes_nn2x_device(w2xc_model *m, int n_in_planes, const float *d_in, size_t in_plane_stride_bytes,
                                    size_t in_stride_bytes, int w, int h, float *d_out, size_t out_plane_stride_bytes,
                                    size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    return convert_planes(m, 1, n_in_planes, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes, hip_stream, opts);
} W2XC_CATCH_ALL

// an upconv head model on float planes: (w, h) is the source size, the output planes are 2w x 2h; the band loop runs on SOURCE rows (run_rows)
int w2xc_convert_planes_up2x_device(w2xc_model *m, int n_in_planes, const float *d_in, size_t in_plane_stride_bytes,
                                    size_t in_stride_bytes, int w, int h, float *d_out, size_t out_plane_stride_bytes,
                                    size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    const w2xc_opts o = resolve_opts(opts);
    if (int rc = check_planes_args(m, 2, n_in_planes, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes, o))
        return rc;
    if (o.precision != W2XC_PRECISION_FP32) return fail(W2XC_ERR_UNSUPPORTED, "16-bit precision modes: not available for a model with an upconv head (W2XC_PRECISION_FP32 only)");
    const PlanesIn in{d_in, in_stride_bytes / 4, (long long)(in_plane_stride_bytes / 4)};
    return rows_on_device(m, RowsCall::whole(in, n_in_planes, w, h, {d_out, out_stride_bytes / 4, (long long)(out_plane_stride_bytes / 4)}, 0), hip_stream, o);
} W2XC_CATCH_ALL

int w2xc_convert_plane_nn2x_device(w2xc_model *m, const float *d_in, size_t in_stride_bytes, int w, int h, float *d_out,
                                   size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    if (int rc = check_plane_args(m, d_in, in_stride_bytes, w, h, d_out, out_stride_bytes, 1)) return rc;
    const w2xc_opts o = resolve_opts(opts);
    return rows_on_device(m, RowsCall::whole({d_in, in_stride_bytes / 4, 0}, 1, 2 * w, 2 * h, {d_out, out_stride_bytes / 4, 0}, 1), hip_stream, o);
} W2XC_CATCH_ALL

// ---- batches of same-size planes -----------------------------------------------------------------
int w2xc_convert_batch_device(w2xc_model *m, int n, int nn2x, const float *d_in, size_t in_plane_stride_bytes, size_t in_stride_bytes, int w, int h,
                              float *d_out, size_t out_plane_stride_bytes, size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    int rc = check_batch_device_args(m, n, nn2x, d_in, in_plane_stride_bytes, in_stride_bytes, w, h, d_out, out_plane_stride_bytes, out_stride_bytes);
    if (rc) return rc;
    const w2xc_opts o = resolve_opts(opts);
    const long long in_ps = (long long)(in_plane_stride_bytes / 4), out_ps = (long long)(out_plane_stride_bytes / 4);
    LockedCtx lc;
    if ((rc = lc.open(nullptr, m, o.device))) return rc;
    return run_batch(m, lc.cs, n, nn2x, {d_in, in_stride_bytes / 4, in_ps}, w, h, {d_out, out_stride_bytes / 4, out_ps}, (hipStream_t)hip_stream, o);
} W2XC_CATCH_ALL

// a one-plane model gives one plane: the call is then w2xc_convert_batch_device's (the same launches as w2xc_convert_planes_device on each image)
static bool one_plane_model(const w2xc_model *m, int n_in_planes) { return n_in_planes == 1 && m->layers.back().nout == 1; }

int w2xc_convert_planes_batch_device(w2xc_model *m, int n, int nn2x, int n_in_planes, const float *d_in, size_t in_image_stride_bytes, size_t in_plane_stride_bytes,
                                     size_t in_stride_bytes, int w, int h, float *d_out, size_t out_image_stride_bytes, size_t out_plane_stride_bytes,
                                     size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    const w2xc_opts o = resolve_opts(opts);
    int rc = check_planes_batch_device_args(m, n, nn2x, n_in_planes, d_in, in_image_stride_bytes, in_plane_stride_bytes, in_stride_bytes, w, h, d_out,
                                            out_image_stride_bytes, out_plane_stride_bytes, out_stride_bytes, o);
    if (rc) return rc;
    const bool one = one_plane_model(m, n_in_planes);
    const BatchIO io = {{d_in, in_stride_bytes / 4, (long long)(in_plane_stride_bytes / 4)}, (long long)(in_image_stride_bytes / 4), n_in_planes,
                        {d_out, out_stride_bytes / 4, one ? 0 : (long long)(out_plane_stride_bytes / 4)}, (long long)(out_image_stride_bytes / 4), 0};
    LockedCtx lc;
    if ((rc = lc.open(nullptr, m, o.device))) return rc;
    return run_batch_planes(m, lc.cs, n, nn2x, io, w, h, (hipStream_t)hip_stream, o);
} W2XC_CATCH_ALL

// a batch of head-model conversions: image i is w2xc_convert_planes_up2x_device on image i, bit for bit; one launch per layer where the chain has batch kernels
int w2xc_convert_planes_up2x_batch_device(w2xc_model *m, int n, int n_in_planes, const float *d_in, size_t in_image_stride_bytes, size_t in_plane_stride_bytes,
                                          size_t in_stride_bytes, int w, int h, float *d_out, size_t out_image_stride_bytes, size_t out_plane_stride_bytes,
                                          size_t out_stride_bytes, void *hip_stream, const w2xc_opts *opts)
try {
    const w2xc_opts o = resolve_opts(opts);
    int rc = check_planes_batch_device_args(m, n, 1, n_in_planes, d_in, in_image_stride_bytes, in_plane_stride_bytes, in_stride_bytes, w, h, d_out,
                                            out_image_stride_bytes, out_plane_stride_bytes, out_stride_bytes, o, true);
    if (rc) return rc;
    RowPlan P;   // (the plan's own refusals -- a head shape without a kernel among them -- before a device is touched)
    if ((rc = plan_rows(m, o, w, h, 0, 0, h, h, n_in_planes, true, &P))) return rc;
    // (all planes of the head, also where it gives one: out.ps != 0, as w2xc_convert_planes_up2x_device)
    const BatchIO io = {{d_in, in_stride_bytes / 4, (long long)(in_plane_stride_bytes / 4)}, (long long)(in_image_stride_bytes / 4), n_in_planes,
                        {d_out, out_stride_bytes / 4, (long long)(out_plane_stride_bytes / 4)}, (long long)(out_image_stride_bytes / 4), 0};
    LockedCtx lc;
    if ((rc = lc.open(nullptr, m, o.device))) return rc;
    return run_batch_planes(m, lc.cs, n, 0, io, w, h, (hipStream_t)hip_stream, o);
} W2XC_CATCH_ALL

// host arithmetic only: the plan of one image of the batch, as run_batch_planes makes it.  nn2x = 2: the plan of w2xc_convert_planes_up2x_batch_device (a head
// model on its source size)
int w2xc_batch_plan(const w2xc_model *m, int n_in_planes, int w, int h, int nn2x, const w2xc_opts *opts, int *batched, int *sub_batch)
try {
    if (!m || !batched || !sub_batch) return fail(W2XC_ERR_ARG, "null argument");
    if (nn2x < 0 || nn2x > 2) return fail(W2XC_ERR_ARG, "nn2x must be 0, 1 or 2 (the plan of w2xc_convert_planes_up2x_batch_device)");
    if (int rc = check_plane_size(w, h, true)) return rc;
    if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    const bool head_plan = nn2x == 2;
    if (head_plan) {
        if (!m->has_head()) return fail(W2XC_ERR_ARG, "w2xc_batch_plan with nn2x = 2: the model has no upconv head");
        nn2x = 0;   // (the head enlarges: the layers run on the source size)
    } else if (m->has_head()) { *batched = 0; *sub_batch = 1; return W2XC_OK; }   // (the batch calls these values of nn2x plan refuse an upconv head model)
    const w2xc_opts o = resolve_opts(opts);
    const int W = w << nn2x, H = h << nn2x;
    RowPlan P;
    if (int rc = plan_rows(m, o, W, H, 0, 0, H, H, n_in_planes, head_plan || !one_plane_model(m, n_in_planes), &P)) return rc;   // (the head call writes all planes of the head)
    *batched = batch_eligible(m, P) ? 1 : 0;
    *sub_batch = 1;
    if (*batched) {
        size_t img_f[2];
        batch_ws_floats(P, img_f);
        *sub_batch = batch_sub_size(P.o, img_f);
    }
    return W2XC_OK;
} W2XC_CATCH_ALL

}  // extern "C"
