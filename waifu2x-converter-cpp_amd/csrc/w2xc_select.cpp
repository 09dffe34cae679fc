// w2xc_select.cpp -- which kernel runs which layer, which layers fuse, and the layouts between layers: resolved once per call into a table (resolve_chain).
#include "w2xc_engine.hpp"

#include <cmath>

namespace w2xc_eng {

// 16-bit terms per activation value between the layers of the split pipeline, w2xc_split.hip (0 = not that pipeline)
int split_terms(const w2xc_opts &o)
{
    if (o.precision == W2XC_PRECISION_BF16) return 1;   // plain bf16 = the same pipeline with ONE term
    return (o.precision == W2XC_PRECISION_BF16X2 || o.precision == W2XC_PRECISION_FP16X2) ? 2 : o.precision == W2XC_PRECISION_BF16X3 ? 3 : 0;
}
int split_fmt(const w2xc_opts &o) { return o.precision == W2XC_PRECISION_FP16X2 ? 1 : 0; }

// the 128 -> 256 layer in front of the head of an upconv model (the published upconv_7 topology; half of its work): conv3x3_wino4 has an instantiation
// for it, planar in and NHWC out, and no other fast kernel has -- with any other choice of w2xc_opts.kernel it runs conv3x3_direct like every shape
// without a kernel.  Models without a head are not asked: their selection stays w2xc_pick_kernel's.
static bool wide_layer(const w2xc_model *m, int l)
{
    const int n = (int)m->layers.size();
    return m->has_head() && l == n - 2 && l > 0 && m->layers[l].nin == 128 && m->layers[l].nout == 256;
}

W2xcKernelKind pick_kind(const w2xc_model *m, int l)
{
    if (m->layers[l].head) return W2XC_K_UPCONV;
    if (wide_layer(m, l)) return W2XC_K_MFMA;
    return w2xc_pick_kernel(m->layers[l].nin, m->layers[l].nout);
}

// fp32 path, layers with 32 / 64 / 128 planes in and out (W2XC_K_MFMA): which kernel runs them.
//   MID_MFMA    conv3x3_mfma2: direct implicit GEMM, a k-ordered fp32 fma chain (the closest MFMA analogue of modelHandler.cpp:134-145)
//   MID_WINO32  conv3x3_wino:   Winograd F(2x2,3x3) on v_mfma_f32_32x32x2_f32, one wave per SIMD (round 2)
// Same arithmetic type (fp32 throughout); Winograd does 2.25x fewer multiplies in another summation order and is held to the same
// rtol 1e-4 gate against the CPU oracle by the same tests.  w2xc_opts.kernel picks per call (W2XC_KERNEL_MFMA / _WINOGRAD /
// _WINOGRAD32 / _WINOGRAD4); W2XC_KERNEL_AUTO = W2XC_KERNEL_WINOGRAD4: conv3x3_wino4 (F(4x4,3x3)) where it applies (>= 64 output planes),
// conv3x3_wino for the rest.  No environment variable takes part in the choice.
//   MID_WINO4   conv3x3_wino4:  Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32 (round 3, the default: 1.78x fewer multiplies again, ~1.3x the rounding error of
//               F(2x2); needs the four-rows-per-layer band geometry of run_rows to stay banding-invariant)
namespace {
int mid_variant(const w2xc_opts &o)
{
    switch (o.kernel) {
    case W2XC_KERNEL_MFMA: return MID_MFMA;
    case W2XC_KERNEL_WINOGRAD:     // (= _WINOGRAD32 since round 5: the round-3 F(2x2) kernel on 16x16x4 tiles, conv3x3_wino16, is retired)
    case W2XC_KERNEL_WINOGRAD32: return MID_WINO32;
    default: return MID_WINO4;   // W2XC_KERNEL_AUTO = W2XC_KERNEL_WINOGRAD4 (no environment switches: the choice is the caller's, per call)
    }
}
// the variant that really runs a (cin, cout) layer: conv3x3_wino4 needs 64-plane output blocks, the F(2x2) kernel takes the rest
int mid_variant_for(int midv, int cin, int cout)
{
    if (midv == MID_WINO4 && !w2xc_wino4_supported(cin, cout)) midv = MID_WINO32;
    if (midv == MID_WINO32 && !w2xc_wino_supported(cin, cout)) midv = MID_MFMA;
    return midv;
}
}  // namespace

// What the model runs with these options.  Nine passes in dependency order; each reads the model, the options and what EARLIER passes filled in, and none
// calls a function of (m, o) -- so the order below is the whole dependency graph, and it has no cycle:
//   1 shape      the kind of every layer by its plane counts (pick_kind, with the wide-layer rule)            <- the model
//   2 mid        the kernel variant of the W2XC_K_MFMA shapes, and which of them are wino4 layers             <- 1, the options
//   3 last       the last-layer fusion                                                                        <- 1, 2
//   4 first      the first-layer fusion; it stands back where the last-layer fusion claims the same layer     <- 1, 2, 3
//   5 kinds      the kind that runs every layer                                                               <- 1 .. 4
//   6 terms      out_terms of every layer's output, and the halves of a tap-plane producer                    <- 3, 5
//   7 layouts    planar or NHWC between two layers                                                            <- 2, 4, 5
//   8 gather     may the producer of the tap planes finish the last layer itself (conv3x3_wino4 PROG)         <- 3, 7
//   9 uint8      may layer 1 read / the last layer write the caller's uint8 image                             <- 5
Chain resolve_chain(const w2xc_model *m, const w2xc_opts &o)
{
    Chain c;
    const int n = (int)m->layers.size();
    const int T = c.T = split_terms(o);
    c.fmt = split_fmt(o);
    c.layer.resize(n);
    if (n == 0) return c;
    const std::vector<HostLayer> &hl = m->layers;
    const bool fp32 = T == 0 && o.precision == W2XC_PRECISION_FP32;
    const bool fast = o.kernel != W2XC_KERNEL_DIRECT;   // W2XC_KERNEL_DIRECT runs every layer alone on conv3x3_direct, whatever `fusion` says
    // w2xc_opts.fusion: which of the two cross-layer fusions a call may use (both precisions; no environment switch takes part)
    const bool first_on = o.fusion != W2XC_FUSION_OFF && o.fusion != W2XC_FUSION_LAST, last_on = o.fusion != W2XC_FUSION_OFF && o.fusion != W2XC_FUSION_FIRST;

    // 1 shape
    std::vector<W2xcKernelKind> shape(n);
    for (int l = 0; l < n; l++) shape[l] = pick_kind(m, l);

    // 2 mid: the variant a W2XC_K_MFMA shape really runs with these options (the wide layer: conv3x3_wino4 or nothing -- pass 5 makes it conv3x3_direct).
    // A wino4 layer is one of the fp32 path: conv3x3_wino4's 4x4 blocks make results depend on where a band's per-layer regions end, unless they end on
    // block boundaries -- run_rows then computes FOUR rows of halo per layer instead of one (and needs 4 n halo rows in its view): any_wino4.
    std::vector<int> midv(n, MID_MFMA);
    for (int l = 0; l < n; l++) {
        if (shape[l] != W2XC_K_MFMA) continue;
        const int want = mid_variant(o);
        midv[l] = wide_layer(m, l) ? (want == MID_WINO4 ? MID_WINO4 : MID_MFMA) : mid_variant_for(want, hl[l].nin, hl[l].nout);
        c.layer[l].wino4 = fp32 && fast && midv[l] == MID_WINO4;
        c.any_wino4 |= c.layer[l].wino4;
    }

    // 3 last: the one-plane last layer is computed inside the epilogue of the mid layer before it, which writes partial tap planes instead of activations
    // (out_terms = 9), and finished by conv3x3_last_gather.  16-bit modes: the producer is conv3x3_split (cin in {32,64,128}).  fp32: the producer runs
    // conv3x3_wino4 (Cout 64 / 128) and writes Cout / 64 x 9 tap planes instead of Cout activation planes.  w2xc_opts.fusion = W2XC_FUSION_OFF / _FIRST
    // disables; W2XC_FUSION_AUTO = on.  (A head model has no W2XC_K_LAST layer: no cross-layer fusion.)
    if (last_on && fast && n >= 3 && hl[n - 1].nout == 1 && shape[n - 1] == W2XC_K_LAST && shape[n - 2] == W2XC_K_MFMA)
        c.fused_last = T > 0 || (fp32 && hl[n - 1].nin == hl[n - 2].nout && midv[n - 2] == MID_WINO4);

    // 4 first: layers 1 (ONE plane -> 32) and 2 in one launch; layer 1's 32 activation planes never reach HBM (convertRoutine.cpp:66-76's loop collapsed by
    // one more launch).  w2xc_opts.fusion = W2XC_FUSION_OFF / _LAST disables; head models: no cross-layer fusion.
    //   16-bit modes  conv3x3_first2_split: layer 2 (32 -> {32,64,128}) is an ordinary split mid layer.
    //   fp32          conv3x3_first2_wino4 (layer 1 on the fly per Winograd patch, layer 2 (32 -> 32) as F(4x4,3x3) with its weights stationary in registers)
    //                 when the default kernels run the model and layer 3 is a wino4 layer: it reads layer 2's planar planes.
    if (first_on && fast && n >= 3 && !m->has_head()) {
        if (T > 0) c.fused_first = hl[0].nin == 1 && hl[0].nout == 32 && shape[1] == W2XC_K_MFMA;
        else if (fp32)
            c.fused_first = (o.kernel == W2XC_KERNEL_AUTO || o.kernel == W2XC_KERNEL_WINOGRAD4) && w2xc_first2_wino4_supported(hl[0].nin, hl[0].nout, hl[1].nout) &&
                            hl[1].nin == hl[0].nout && c.layer[2].wino4;
        if (T > 0 && n == 3 && c.fused_last) c.fused_first = false;    // (layer 2 would be the fused-last producer: keep that fusion instead)
        if (T == 0 && n == 4 && c.fused_last) c.fused_first = false;   // (layer 3 would carry the fused last layer: that instantiation reads 32 NHWC planes only)
    }

    // 5 kinds
    for (int l = 0; l < n; l++) {
        W2xcKernelKind &k = c.layer[l].kind;
        k = shape[l];
        if (k == W2XC_K_UPCONV) continue;   // (the head has one kernel, whatever runs the 3x3 layers)
        if (!fast || (wide_layer(m, l) && midv[l] != MID_WINO4)) k = W2XC_K_DIRECT;
        else if (l <= 1 && c.fused_first) k = l == 0 ? W2XC_K_FUSED_AWAY : T > 0 ? W2XC_K_FIRST2_SPLIT : W2XC_K_FIRST2_WINO4;
        else if (T > 0) {
            // term planes live only BETWEEN a first/mid layer and a mid layer; everything that touches the
            // caller's planes or the last layer is fp32.  Shapes without an MFMA kernel are unsupported.
            if (k == W2XC_K_MFMA) k = l > 0 ? W2XC_K_MID_SPLIT : W2XC_K_DIRECT;
            else if (k == W2XC_K_FIRST && l == 0) k = (n > 1 && shape[1] == W2XC_K_MFMA) ? W2XC_K_FIRST_SPLIT : W2XC_K_FIRST;
            else if (k == W2XC_K_LAST && l == n - 1 && l > 0) k = c.fused_last ? W2XC_K_LAST_GATHER : W2XC_K_LAST;
            else k = W2XC_K_DIRECT;   // plan_rows rejects this
        } else if (k == W2XC_K_LAST && l == n - 1 && c.fused_last) k = W2XC_K_LAST_GATHER;
        if (k == W2XC_K_MFMA) c.layer[l].midv = midv[l];
    }

    // 6 terms: of layer l's OUTPUT in the split pipeline: T when layer l + 1 is a split mid layer, else 0 (fp32); 9 = this layer writes the partial tap
    // planes of the last layer it computes in its epilogue (16-bit modes: conv3x3_split; fp32: conv3x3_wino4) -- `halves` of them per tap: wave columns
    // of the split tile shapes, 64-plane blocks of conv3x3_wino4 (its epilogue sums the four plane tiles of a block on chip)
    for (int l = 0; l + 1 < n; l++) {
        LayerPick &L = c.layer[l];
        if (l == n - 2 && c.fused_last) {
            L.out_terms = 9;
            L.halves = T > 0 ? w2xc_split_halves(T, hl[l].nin, hl[l].nout) : hl[l].nout / 64;
        } else if (c.layer[l + 1].kind == W2XC_K_MID_SPLIT) L.out_terms = T;
    }

    // 7 layouts: conv3x3_wino4 reads PLANAR activations (one plane per channel, rows of roundup32(w) floats: 16-byte aligned pixel quads, tiles on 128-byte
    // lines) -- with 32 input planes also the NHWC pixels (one 128-byte line each) that the 32-plane producers conv3x3_first / conv3x3_wino write.
    // Layer l's output (l = 0 .. n-2) is planar when its consumer is a wino4 layer with 64 / 128 input planes, when layer l is the fused
    // conv3x3_first2_wino4 launch (layers 1 + 2; its consumer conv3x3_wino4<32, .> then reads planar), or when layer l is a wino4 layer and its
    // consumer is conv3x3_direct (any strides); everything else stays NHWC (conv3x3_wino4 writes either).  Producers that write planar:
    // conv3x3_wino4, conv3x3_first2_wino4, conv3x3_first (3 -> 64 / 128), conv3x3_direct.
    // (Why planar rows are roundup32(w) floats: a tile's 32-pixel row segment -- tiles start at multiples of 32 pixels -- is then ONE 128-byte line; with
    // rows of roundup4(w) floats every segment straddled two lines, each written in two pieces by different workgroups: the 32 -> 32 layer in front took
    // 2.0 ms instead of 0.8, measured.  layer_desc applies it.)
    for (int l = 0; l + 1 < n; l++) {
        bool &planar = c.layer[l].planar_out;
        if (c.layer[l].kind == W2XC_K_FIRST2_WINO4) planar = true;   // (conv3x3_first2_wino4 writes planar planes; conv3x3_wino4<32, .> reads either)
        else if (c.layer[l + 1].wino4) planar = hl[l + 1].nin != 32;   // (32 input planes: conv3x3_wino4 reads the producer's NHWC pixels, one 128-byte line each)
        else if (c.layer[l].wino4) planar = c.layer[l + 1].kind == W2XC_K_DIRECT;   // (conv3x3_last reads NHWC at 5.4 TB/s; its planar variant measured half of that: NHWC out there)
    }

    // 8 gather: fp32, last layer fused: does the producing launch also FINISH it (conv3x3_wino4 PROG: the partial tap planes are summed by the workgroup
    // whose arrival completes a 16-row x 256-column job, rows complete top to bottom while the launch runs), or does a conv3x3_last_gather launch follow
    // (rounds 4 / 5; w2xc_opts.fusion = W2XC_FUSION_GATHER_LAUNCH, and the shapes PROG has no instantiation for)?  The two are bit-identical.
    // (Where it may, the tap planes' rows start on 128-byte lines -- layer_desc, ws_need: a tile's 32-pixel row segment of a tap plane is then exactly ONE
    // line, written whole, and a gather job never pulls a line into its XCD's L2 that holds columns of a tile it does not depend on -- with rows of out_w
    // floats such a line, cached before its last columns were written, was served stale to the neighbouring job later: intermittent mismatches on small planes.)
    c.prog_gather = T == 0 && c.fused_last && o.fusion != W2XC_FUSION_GATHER_LAUNCH && w2xc_wino4_prog_supported(hl[n - 2].nin, hl[n - 2].nout) &&
                           c.layer[n - 3].planar_out;   // (the PROG instantiations read planar planes)

    // 9 uint8: the RGB image pipeline (w2xc_image.cpp): the layer that touches the caller's interleaved uint8 image converts in its own load / store where a
    // kernel for that exists -- the W2XC_K_FIRST layer of the call's first pass (3 -> 32 / 64 / 128), the W2XC_K_LAST layer of its last pass (32 / 64 / 128
    // -> 3) or the head of an upconv model (upconv4x4_head, U8) -- and the float copy of that image never reaches HBM.  fp32 and the fast kernels only;
    // w2xc_opts.fusion = W2XC_FUSION_OFF keeps the colour kernels around float planes (the same float operations in the same order: the same bytes).
    if (fp32 && fast && o.fusion != W2XC_FUSION_OFF) {
        c.u8_source = hl[0].nin == 3 && c.layer[0].kind == W2XC_K_FIRST;
        c.u8_sink = hl[n - 1].nout == 3 && (c.layer[n - 1].kind == W2XC_K_LAST || c.layer[n - 1].kind == W2XC_K_UPCONV);
    }
    return c;
}

// ------------------------------------------------------------------------------------------------
// The band geometry of run_rows (w2xc_rows.cpp) as pure host arithmetic: no device, no allocation.  w2xc_plan_rows exposes it
// (tests/test_plan.py runs it on the CPU box).
//
// conv3x3_wino4 (F(4x4,3x3)): an output of a 4x4 block depends, at rounding level, on all 36 patch values, so a block cut by the edge of a
// band's region (clamped rows instead of the plane's) would make results depend on the banding.  HL = 4: every layer k < n computes the rows
//     [floor4(y0) - 4 (n - k), ceil4(y1) + 4 (n - k))  clipped to the layer's plane extent [-(n - k), H + (n - k))
// of a band [y0, y1) instead of [y0 - (n - k), y1 + (n - k)): every region edge that is not a plane edge is a block edge (blocks sit on rows
// = 0 mod 4 of the plane), and layer k + 1 finds the rows it reads (one more each side) inside.  Costs up to 3 + 3 (n - k) more rows per side.
void RowPlan::region(int k, int y0, int y1, int &T_, int &B_) const   // plane rows [T, B) layer k computes for the band [y0, y1)
{
    if (HL == 1 || k == n) { T_ = y0 - (n - k); B_ = y1 + (n - k); return; }
    T_ = std::max(-(n - k), (y0 & ~3) - 4 * (n - k));
    B_ = std::min(plane_h + (n - k), ((y1 + 3) & ~3) + 4 * (n - k));
}

// BYTES per band of `rows` output rows for the two ping-pong buffers (layer k's output goes to ws[(k - 1) & 1])
void RowPlan::ws_need(const w2xc_model *m, int rows, size_t need[2]) const
{
    need[0] = need[1] = 0;
    for (int k = 1; k <= n; k++) {
        if (k == n && last_direct) break;   // written straight to d_out
        const LayerPick &L = chain.layer[k - 1];
        if (L.kind == W2XC_K_FUSED_AWAY) continue;   // layer 1's activations stay on chip
        const size_t hk = (size_t)rows + ((HL == 1 || k == n) ? 2 * (n - k) : 6 + 8 * (n - k)), wk = (size_t)w + 2 * (n - k);
        const int ot = L.out_terms;
        const bool fused = ot == 9;   // partial G planes of the fused last layer
        const size_t bpe = (ot >= 1 && ot <= 3) ? 2 * (size_t)ot : 4;   // bytes per activation element of layer k's output
        const size_t px_bytes = fused ? (size_t)L.halves * 9 * 4 : m->layers[k - 1].nout * bpe;
        const size_t wk_mem = (L.planar_out || (fused && chain.prog_gather)) ? ((wk + 31) & ~(size_t)31) : wk;   // planar rows (and the tap planes a PROG launch gathers itself) start on 128-byte lines
        need[(k - 1) & 1] = std::max(need[(k - 1) & 1], hk * wk_mem * px_bytes);
    }
}

// The tallest band every launch of the chain can address (NO_CAP: no rule binds): the launchers' 32-bit rules restated over the region heights of a band of
// `rows` output rows -- layer k computes at most min(rows + halo(k), plane_h + 2 (n - k)) rows (RowPlan::region; halo as in ws_need), and a plane whose
// whole extent satisfies a rule is not capped by it.
//   conv3x3_first2_wino4   32-bit lane offsets over its 32 output planes (12 plane strides + a row): planes of at most 64 Mi floats (w2xc_launch_first2_wino4)
//   conv3x3_wino4          planar in: 3 in_cs 4 + 24 in_rs 4 < 2^32, in_cs = in_rs x the rows of the layer in front; 32 NHWC planes in: 24 in_rs 4 < 2^32, which
//                          no band changes; tiles_x tiles_y (COUT / 64) < 2^31 items (w2xc_launch_wino4, launch_wino4)
// (PROG's rule, out_h out_rs 4 < 2^32, caps nothing: prog_eligible (w2xc_rows.cpp) leaves such a band to the gather launch.)
namespace {
const long long NO_CAP = 1ll << 62;
long long halo_of(const RowPlan &P, int k) { return (P.HL == 1 || k == P.n) ? 2 * (long long)(P.n - k) : 6 + 8 * (long long)(P.n - k); }
// rows of a band when layer k may compute at most `max_h` rows
long long band_for(const RowPlan &P, int k, long long max_h) { return P.plane_h > 0 && (long long)P.plane_h + 2 * (P.n - k) <= max_h ? NO_CAP : std::max(0ll, max_h - halo_of(P, k)); }
long long first2_max_band(const RowPlan &P)
{
    const long long wk = ((long long)P.w + 2 * (P.n - 2) + 31) & ~31ll;
    return std::max(0ll, (64ll << 20) / wk - halo_of(P, 2));   // (every band, whatever the plane's height: the cap as it has always been)
}
long long addr_max_band(const w2xc_model *m, const RowPlan &P, const char **rule)
{
    const int n = P.n;
    long long best = NO_CAP;
    auto cap = [&](long long b, const char *what) { if (b < best) { best = b; *rule = what; } };
    if (P.chain.fused_first && P.chain.T == 0) cap(first2_max_band(P), "conv3x3_first2_wino4: planes of at most 64 Mi floats");
    for (int k = 2; k <= n; k++) {
        if (!P.chain.layer[k - 1].wino4) continue;
        const long long in_w = (long long)P.w + 2 * (n - k + 1), out_w = (long long)P.w + 2 * (n - k);
        if (P.chain.layer[k - 2].planar_out) {
            const long long in_rs = (in_w + 31) & ~31ll;
            cap(band_for(P, k - 1, (((1ll << 30) - 1) / in_rs - 24) / 3), "3 in_cs 4 + 24 in_rs 4 < 2^32");
        } else if (24 * in_w * m->layers[k - 1].nin * 4 >= (1ll << 32)) cap(0, "24 in_rs 4 < 2^32 with 32 NHWC planes in");
        const long long per_row = ((out_w + 31) / 32) * (m->layers[k - 1].nout / 64);
        cap(band_for(P, k, 16 * (((1ll << 31) - 1) / per_row) - 18), "tiles_x tiles_y (COUT / 64) < 2^31");   // (tiles_y <= (out_h + 3 + 15) / 16)
    }
    return best;
}
}  // namespace

// Output rows [ra, rb) of an h-row plane of which the view holds rows [vy0, vy0 + vh): halo geometry, band height, workspace bytes, and the
// options the call really runs with (W2XC_FUSION_AUTO gives up a fusion whose kernel cannot address the plane; an explicit request fails instead).
int plan_rows(const w2xc_model *m, const w2xc_opts &o_in, int w, int vh, int vy0, int ra, int rb, int plane_h, int n_in, bool all_out, RowPlan *p)
{
    RowPlan &P = *p;
    const int n = (int)m->layers.size();
    if (n == 0) return fail(W2XC_ERR_ARG, "model has no layers");
    P.o = o_in;
    P.chain = resolve_chain(m, P.o);
    P.n = n; P.w = w; P.plane_h = plane_h; P.all_out = all_out;
    P.HL = 1;
    if (P.chain.any_wino4) {
        const int hs = 4 * n;
        if (plane_h > 0 && vy0 <= std::max(0, ra - hs) && vy0 + vh >= std::min(plane_h, rb + hs)) P.HL = 4;
        else if (P.o.kernel == W2XC_KERNEL_AUTO)   // a view with n halo rows only: no silent change of kernel (and rounding) -- the caller decides
            return fail(W2XC_ERR_ARG, "row-band view [%d,%d) of rows [%d,%d): the default F(4x4) kernel needs %d halo rows (4 per layer) for banding-invariant results; "
                                      "pass the wide view or choose w2xc_opts.kernel explicitly (W2XC_KERNEL_WINOGRAD32: F(2x2), banding-invariant on the minimum view)",
                        vy0, vy0 + vh, ra, rb, hs);
        // (an explicit W2XC_KERNEL_WINOGRAD4 on a narrow view runs as asked: results then depend on the banding at rounding level)
    }
    const bool head = m->has_head();
    if (head) {   // (the entry points that run a head model: every other one has refused it -- refuse_head)
        const HostLayer &hd = m->layers[n - 1];
        if (P.chain.T != 0) return fail(W2XC_ERR_UNSUPPORTED, "16-bit precision modes: not available for a model with an upconv head (W2XC_PRECISION_FP32 only)");
        if (n < 2) return fail(W2XC_ERR_UNSUPPORTED, "an upconv head needs at least one 3x3 layer in front of it");
        if (!w2xc_upconv_supported(hd.nin, hd.nout))
            return fail(W2XC_ERR_UNSUPPORTED, "upconv head %d->%d: the head kernel takes 32, 64, 128 or 256 planes (fewer than 32 are zero-padded) and gives 1 or 3", hd.decl_nin(), hd.decl_nout());
    }
    if (m->layers[0].nin != n_in)   // convertWithModelsBasic pushes exactly one plane (convertRoutine.cpp:63-64)
        return fail(W2XC_ERR_PLANES, "Error : Model-filter : \nnumber of input planes mismatch.\n%d,%d", n_in, m->layers[0].nin);
    for (int l = 1; l < n; l++)
        if (m->layers[l].decl_nin() != m->layers[l - 1].decl_nout())   // (what the model declares: a head model's zero padding would hide 16 against 20)
            return fail(W2XC_ERR_PLANES, "Error : Model-filter : \nnumber of input planes mismatch.\n%d,%d", m->layers[l - 1].decl_nout(), m->layers[l].decl_nin());
    if (P.o.precision != W2XC_PRECISION_FP32 && P.chain.T == 0) return fail(W2XC_ERR_ARG, "unknown precision %d", P.o.precision);
    if (P.o.fusion < W2XC_FUSION_AUTO || P.o.fusion > W2XC_FUSION_PROG) return fail(W2XC_ERR_ARG, "unknown w2xc_opts.fusion %d", P.o.fusion);
    if (P.chain.T > 0)
        for (int l = 0; l < n; l++)
            if (P.chain.layer[l].kind == W2XC_K_DIRECT)
                return fail(W2XC_ERR_UNSUPPORTED, "16-bit precision modes: layer %d (%d->%d) has no kernel ({1,3}->{32,64,128} first, {32,64,128}->{32,64,128}, ->{1,3} last only)",
                            l + 1, m->layers[l].nin, m->layers[l].nout);
    // The launchers' 32-bit limits as a cap on the band (addr_max_band above).  A plane too wide for conv3x3_first2_wino4 even in the shortest band:
    // W2XC_FUSION_AUTO runs the first two layers unfused, an explicit request is refused.  A plane no band makes addressable for conv3x3_wino4: refused
    // here, before a device is touched -- not as a launch error in the middle of a call.
    const char *cap_rule = "";
    long long max_band = addr_max_band(m, P, &cap_rule);
    if (max_band < 8 && P.chain.fused_first && P.chain.T == 0 && first2_max_band(P) < 8) {
        if (P.o.fusion != W2XC_FUSION_AUTO)
            return fail(W2XC_ERR_UNSUPPORTED, "plane too wide (%d pixels) for the fused first layers; use w2xc_opts.fusion = W2XC_FUSION_AUTO, _LAST or _OFF", w);
        P.o.fusion = W2XC_FUSION_LAST;
        P.chain = resolve_chain(m, P.o);   // (the options changed: the one place in a call where the chain is resolved a second time)
        max_band = addr_max_band(m, P, &cap_rule);
    }
    if (max_band < 8)
        return fail(W2XC_ERR_UNSUPPORTED, "plane too wide (%d pixels) for conv3x3_wino4's 32-bit offsets in any band (%s); use w2xc_opts.kernel = W2XC_KERNEL_WINOGRAD32 or _MFMA", w, cap_rule);
    // the last layer stores straight into the caller's planar plane(s) when its kernel can address planar
    // output (conv3x3_last / conv3x3_direct); otherwise it goes through the NHWC workspace + a repack
    P.last_kind = P.chain.layer[n - 1].kind;
    P.last_direct = head || ((m->layers[n - 1].nout == 1 || all_out) &&
                    (P.last_kind == W2XC_K_LAST || P.last_kind == W2XC_K_LAST_GATHER || P.last_kind == W2XC_K_DIRECT ||
                     (m->layers[n - 1].nout == 1 && P.last_kind != W2XC_K_MFMA && P.last_kind != W2XC_K_FIRST)));
    int band = P.o.band_rows;
    const int total = rb - ra;
    if (band <= 0) {
        const size_t budget = (size_t)(P.o.workspace_mb > 0 ? P.o.workspace_mb : 16384) << 20;
        size_t need[2];
        P.ws_need(m, total, need);
        if (need[0] + need[1] <= budget) band = total;
        else {
            // bytes grow linearly in rows: solve on two probes
            size_t n1[2], n2[2];
            P.ws_need(m, 1, n1);
            P.ws_need(m, 2, n2);
            const double per_row = (double)((n2[0] + n2[1]) - (n1[0] + n1[1]));
            const double base = (double)(n1[0] + n1[1]) - per_row;
            band = (int)std::floor(((double)budget - base) / per_row);
            if (band < 1) band = 1;
            if (band > total) band = total;
            // each buffer's need is a MAX over layers, so the slope measured at 1..2 rows is that of the wide-halo,
            // few-plane layers and under-estimates large bands: re-evaluate the real need and shrink until it fits
            for (int it = 0; it < 64 && band > 1; it++) {
                P.ws_need(m, band, need);
                if (need[0] + need[1] <= budget) break;
                const int nb2 = (int)((double)band * (double)budget / (double)(need[0] + need[1]));
                band = std::max(1, std::min(band - 1, nb2));
            }
            const int nb = (total + band - 1) / band;
            band = (total + nb - 1) / nb;   // equalise (never larger than the band that was just checked)
        }
    }
    // (the addressing limits also bound a band the caller asked for: w2xc_plan_rows reports the height that runs)
    if ((long long)band > max_band) band = (int)max_band;
    if (P.HL > 1 && band < total) band = std::max(4, band & ~3);   // (band edges on block rows: no rounding-out rows)
    P.band = std::min(band, total);
    P.ws_need(m, P.band, P.need);
    return W2XC_OK;
}

// The launch descriptor of layer k of the band [y0, y1): region, offsets into what it reads, Winograd block phase, the fused-first merge, the gather's
// rebased view, and the layout of what it writes (the layouts between layers above).  The one place this is derived: run_rows and run_batch (w2xc_rows.cpp).
W2xcKernelKind layer_desc(const w2xc_model *m, const RowPlan &P, int k, int y0, int y1, int up, const LayerSrc &src, const LayerDst &dst,
                          W2xcConvDesc &first_d, W2xcConvDesc *dp, LayerSrc *next)
{
    const int n = P.n, T = P.chain.T;
    const HostLayer &hl = m->layers[k - 1];
    const LayerPick &L = P.chain.layer[k - 1];
    W2xcConvDesc &d = *dp;
    memset(&d, 0, sizeof d);
    d.in = src.p; d.in_rs = src.rs; d.in_ps = src.ps; d.in_cs = src.cs;
    d.in_h = src.h; d.in_w = src.w;
    int Tk, Bk;
    P.region(k, y0, y1, Tk, Bk);
    d.out_h = Bk - Tk;
    d.out_w = P.w + 2 * (n - k);
    d.off_y = Tk - 1 - src.top;   // (k = 1: y0 - n - vy0; k > 1: 0 on the one-row-per-layer geometry)
    d.off_x = k == 1 ? -n : 0;
    // this launch's first output row in the coordinates of the whole plane, modulo the Winograd block height (2; conv3x3_wino4: 4) -- read by the Winograd kernels only
    const W2xcKernelKind kind = L.kind;
    d.wino_py = Tk & ((L.midv == MID_WINO4 || kind == W2XC_K_FIRST2_WINO4) ? 3 : 1);
    d.in_shift = k == 1 ? up : 0;
    *next = src;
    next->top = Tk;
    if (kind == W2XC_K_FUSED_AWAY) {   // layer 1 inside layer 2's kernel: keep its input description for that launch
        first_d = d;
        return kind;
    }
    if (kind == W2XC_K_FIRST2_SPLIT || kind == W2XC_K_FIRST2_WINO4) {
        d.in = first_d.in; d.in_rs = first_d.in_rs; d.in_ps = first_d.in_ps; d.in_cs = first_d.in_cs;
        d.in_h = first_d.in_h; d.in_w = first_d.in_w;
        d.in_shift = first_d.in_shift;
        // conv3x3_first2_wino4 takes layer 1's input view; a source row of layer 2's output row y, taps r' and r: y + r' + r + (both offsets)
        if (kind == W2XC_K_FIRST2_WINO4) { d.off_y += first_d.off_y; d.off_x += first_d.off_x; }
        else { d.off_y = first_d.off_y; d.off_x = first_d.off_x; }
    }
    d.out_terms = L.out_terms;
    d.in_ts = src.ts; d.in_gs = src.gs;   // (0 unless src holds term planes or the partial planes of a fused last layer; fp32: only that one uses the term fields)
    if (kind == W2XC_K_LAST_GATHER) d.halves = src.halves;
    if (T == 0 && kind == W2XC_K_LAST_GATHER) {
        d.in += (long long)d.off_y * d.in_rs;   // (no offsets in that kernel; off_y > 0 on the four-rows-per-layer geometry only)
        d.in_h -= d.off_y;
        d.off_y = 0;
    }
    const int split_grp = T > 0 ? 16 : 0;   // channel-group size of the blocked term planes
    if (T > 0) {
        d.terms = (kind == W2XC_K_MID_SPLIT || kind == W2XC_K_FIRST2_SPLIT) ? T : 0;
        d.fmt = P.chain.fmt;
        d.out_ts = (long long)d.out_h * d.out_w * hl.nout;
        d.out_gs = (long long)d.out_h * d.out_w * split_grp;
    }
    if (k == n && P.last_direct) {
        d.out = dst.out;
        d.out_rs = dst.out_rs; d.out_ps = 1; d.out_cs = dst.out_cs;
    } else {
        d.out = dst.ws[(k - 1) & 1];
        d.out_rs = (long long)d.out_w * hl.nout; d.out_ps = hl.nout; d.out_cs = 1;
        if (L.planar_out) {   // planes of out_h rows of roundup32(out_w) floats (resolve_chain, pass 7: why 32)
            d.out_rs = (d.out_w + 31) & ~31; d.out_ps = 1; d.out_cs = d.out_rs * (long long)d.out_h;
        }
        if (T > 0 && d.out_terms >= 1 && d.out_terms <= 3) { d.out_rs = (long long)d.out_w * split_grp; d.out_ps = split_grp; }
        if (d.out_terms == 9) {   // G[half][tap][y][x]; rows on 128-byte lines where the producing launch finishes the last layer itself (resolve_chain, pass 8: why)
            d.out_rs = P.chain.prog_gather ? ((d.out_w + 31) & ~31) : d.out_w; d.out_ps = 1;
            d.out_gs = (long long)d.out_h * d.out_rs;
            d.out_ts = 9 * d.out_gs;
            d.halves = L.halves;
        }
    }
    next->p = d.out; next->rs = d.out_rs; next->ps = d.out_ps; next->cs = d.out_cs; next->ts = d.out_ts; next->gs = d.out_gs;
    next->halves = d.halves; next->h = d.out_h; next->w = d.out_w;
    return kind;
}

// ------------------------------------------------------------------------------------------------
// Batches of same-size planes (w2xc_convert_batch*, run_batch in w2xc_rows.cpp): the launch chain that has batch kernels is exactly the default fp32 one --
// conv3x3_first2_wino4 (layers 1 + 2), conv3x3_wino4 with planar planes in and out (layers 3 .. n - 2), conv3x3_wino4 FUSE7 (layer n - 1 + the last layer's
// taps), the gather -- with one plane in, one plane out and the whole image in one band.  The decision is on the plan of ONE image, so it is the chain the
// single-image call runs with the same options: an image of a batch is bit-identical to it either way.
//
// The second chain is that of a multi-plane (RGB) model (w2xc_convert_planes_batch_device, the RGB image calls, their TTA passes), under the same conditions:
// conv3x3_first (three planes in; NHWC or planar out), then W2XC_K_MFMA layers run by conv3x3_wino4 or conv3x3_wino in a layout combination that has a batch
// form (w2xc_wino4_batch_supported / w2xc_wino4_batch_layout_supported / w2xc_wino_batch_supported), then conv3x3_last storing all three planes in place.
//
// A three-plane upconv head model (w2xc_convert_planes_up2x_batch_device, the head-model image batch and its TTA pass) has the same chain with the head in
// conv3x3_last's place: layer n - 1 is W2XC_K_UPCONV (upconv4x4_head_batch) on the NHWC planes of layer n - 2, which may be the 128 -> 256 layer
// (conv3x3_wino4_batch_l<128, 256>: the predicate says so).  A one-plane head model has no batched chain: the single-image launch sequence per image.
namespace {
bool batch_chain_planes(const w2xc_model *m, const RowPlan &P)
{
    const std::vector<LayerPick> &L = P.chain.layer;
    const int n = P.n;
    if (n < 2 || !P.all_out || !P.last_direct) return false;
    if (m->layers[0].nin != 3 || m->layers[n - 1].nout != 3) return false;
    const bool head = m->has_head();
    if (L[0].kind != W2XC_K_FIRST || L[n - 1].kind != (head ? W2XC_K_UPCONV : W2XC_K_LAST) || L[0].out_terms != 0) return false;
    if (head && !w2xc_upconv_supported(m->layers[n - 1].nin, m->layers[n - 1].nout)) return false;
    if (L[n - 2].planar_out) return false;   // (conv3x3_last and upconv4x4_head read NHWC pixels)
    for (int l = 1; l <= n - 2; l++) {
        const HostLayer &hl = m->layers[l];
        if (L[l].kind != W2XC_K_MFMA || L[l].out_terms != 0) return false;
        const bool in_planar = L[l - 1].planar_out, out_planar = L[l].planar_out;
        switch (L[l].midv) {
        case MID_WINO4:
            if (in_planar && out_planar ? !w2xc_wino4_batch_supported(hl.nin, hl.nout, false) : !w2xc_wino4_batch_layout_supported(hl.nin, hl.nout, !in_planar, out_planar))
                return false;
            break;
        case MID_WINO32:
            if (in_planar || out_planar || !w2xc_wino_batch_supported(hl.nin, hl.nout)) return false;
            break;
        default: return false;
        }
    }
    return true;
}
}  // namespace

bool batch_eligible(const w2xc_model *m, const RowPlan &P)
{
    const w2xc_opts &o = P.o;
    const std::vector<LayerPick> &L = P.chain.layer;
    const int n = P.n;
    if (P.chain.T != 0 || o.precision != W2XC_PRECISION_FP32 || o.kernel != W2XC_KERNEL_AUTO || o.fusion == W2XC_FUSION_PROG) return false;
    if (P.band < P.plane_h || P.plane_h <= 0) return false;
    if (batch_chain_planes(m, P)) return true;
    if (n < 5 || P.HL != 4 || P.all_out || !P.last_direct) return false;
    if (m->layers[0].nin != 1 || m->layers[n - 1].nout != 1) return false;
    if (L[0].kind != W2XC_K_FUSED_AWAY || L[1].kind != W2XC_K_FIRST2_WINO4) return false;
    if (L[n - 1].kind != W2XC_K_LAST_GATHER || L[n - 2].out_terms != 9) return false;
    for (int l = 2; l <= n - 2; l++) {
        const HostLayer &hl = m->layers[l];
        if (L[l].kind != W2XC_K_MFMA || !L[l].wino4 || !L[l - 1].planar_out) return false;
        if (l < n - 2 && (!L[l].planar_out || L[l].out_terms != 0)) return false;
        if (!w2xc_wino4_batch_supported(hl.nin, hl.nout, l == n - 2)) return false;
    }
    return true;
}

void batch_ws_floats(const RowPlan &P, size_t img_floats[2])
{
    for (int i = 0; i < 2; i++) img_floats[i] = P.need[i] ? (((P.need[i] + 3) / 4 + 63) & ~(size_t)63) : 0;   // (every image's planes on 256-byte boundaries)
}

int batch_sub_size(const w2xc_opts &o, const size_t img_floats[2])
{
    const size_t budget = (size_t)(o.workspace_mb > 0 ? o.workspace_mb : 16384) << 20;   // the budget that sizes bands (plan_rows)
    const size_t per = 4 * (img_floats[0] + img_floats[1]);
    if (per == 0) return 1;
    const size_t k = budget / per;
    return k < 1 ? 1 : k > 65535 ? 65535 : (int)k;   // (the gather's grid has one row of workgroups per image)
}

// a batch converts one plane into one plane: what the multi-plane entry points (w2xc_convert_planes_device) are for is refused
int check_batch_model(const w2xc_model *m)
{
    if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    if (m->layers[0].nin != 1 || m->layers.back().nout != 1)
        return fail(W2XC_ERR_PLANES, "w2xc_convert_batch*: one plane in and one plane out (the model takes %d and gives %d; see w2xc_convert_planes_device)",
                    m->layers[0].nin, m->layers.back().nout);
    return W2XC_OK;
}

}  // namespace w2xc_eng
