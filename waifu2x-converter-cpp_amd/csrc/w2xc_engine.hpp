// w2xc_engine.hpp -- what the translation units of the engine share (internal; the public boundary is include/w2xc_hip.h).
//
//   w2xc_model.cpp          error state, model container + JSON loader (the reference's Model / modelUtility,
//                           src/modelHandler.{hpp,cpp}), per-(model, device) contexts, the measurement entry points
//   w2xc_select.cpp         which kernel runs which layer, which layers fuse, the layouts between layers, the band geometry
//                           (plan_rows) and the launch descriptor of one layer of a band (layer_desc) -- pure host arithmetic:
//                           unit-tested on the CPU through w2xc_plan_rows
//   w2xc_pack.cpp           which kernel kind a (cin, cout) layer has, the shape predicates of every kernel family and ALL weight packers
//                           (w2xc_pack.hpp; no HIP header: tests/cpp/pack_test.cpp builds it with g++ and checks the images).  The kernel
//                           files (*.hip) hold kernels and their launchers only; w2xc_layout.h = the constants both sides share,
//                           w2xc_launch.hpp = the large-LDS opt-in and the persistent grid rule of the launchers
//   w2xc_cuts.hpp           where the chunked launch strategies cut a band's rows (integers only; tests/cpp/cuts_test.cpp)
//   w2xc_rows.cpp           launch_layer, run_rows (the band loop that replaces convertWithModels / ...Basic / ...BlockSplit,
//                           src/convertRoutine.cpp:21-169: run_band picks one launch strategy per layer -- prog, tail16, tail32,
//                           first_chunks, last_chunks, plain), run_batch (the same run_band on a batched Band), and the device-pointer entry points
//   (this file)             what those calls are made of: Planes (PlanesIn / PlanesOut: float planes of one size in device memory), RowsCall (one run_rows call;
//                           RowsCall::whole = the whole plane, no hooks), LockedCtx (the call's context(s), locked), check_plane_size / check_row_strides, ranges_overlap
//   w2xc_scratch.hpp        Scratch: the one owner of every grow-only device / page-locked buffer (reserve, release, the drain rule); a context lists its
//                           buffers once, DevCtx::for_each_scratch below -- destruction, w2xc_model_trim and w2xc_debug_fill_scratch go by that list
//   w2xc_host_geom.hpp      the integers of the host side: a unit's rows and source view, staging chunks and their taper, the rows finished job rows
//                           cover, the job flags' epoch test, sub-batch striping, the image pipelines' planes, the RGBA call's and the YUV mirror's layout (no HIP header;
//                           tests/cpp/host_geom_test.cpp)
//   w2xc_host_pipeline.cpp  host plane in -> host plane out: staging rings, three streams, the feeder with its Uploader, the drainer (Stitcher), the unit
//                           fan-out (run_units), the host batch pipeline
//   w2xc_filter.cpp         Model::filter at the host / device boundary (src/modelHandler.cpp:26-72)
//   w2xc_image.hpp          what the image units share: ImageCall, the U8Images views, the two pipelines' entry, tta_pass, the plan and the argument checks, and the call
//                           forms -- host single, host batch, device batch -- every family runs its sub-batch callable through
//   w2xc_image.cpp          N2: the CLI's image pipeline around the plane conversion (main.cpp:74-172): one pipeline for Y models and one for RGB models, each
//                           for S images of one size (process_y_device, process_rgb_device; rgb_passes); the plan, the checks, the call forms' bodies; the
//                           single-image and batch entry points of both, the colour and resize blocks
//   w2xc_image_tta.cpp      test-time augmentation: tta_pass (spread -> the CNN on the 8 variants -> gather; kernels in w2xc_tta.hip, and -- the uint8 image at the
//                           outer side -- w2xc_tta_u8.hip), the TTA plane calls, the spread / gather blocks
//   w2xc_image_rgba.cpp     RGBA images (w2xc_process_image_rgba_u8*): process_rgba_device around either pipeline; the bleed call and its scratch
//   w2xc_image_yuv.cpp      YUV frames (w2xc_process_frames_yuv_u8*): process_yuv_device -- luma bytes through run_batch, chroma bytes to bytes (w2xc_yuv.hip) -- and,
//                           through RGB and head models by a colour matrix (..._rgb*), process_yuv_rgb_device -- rgb_passes between two kernels (w2xc_yuv_rgb.hip)
#pragma once
#include "../../include/w2xc_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "w2xc_kernels.h"
#include "w2xc_scratch.hpp"

namespace w2xc_eng {

extern thread_local std::string g_last_error;
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(W2XC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// no C++ exception (std::bad_alloc from a staging vector, std::system_error from std::thread ...) may cross the C ABI
#define W2XC_CATCH_ALL                                                                                       \
    catch (const std::bad_alloc &) { return fail(W2XC_ERR_NOMEM, "out of host memory"); }                    \
    catch (const std::exception &e_) { return fail(W2XC_ERR_HIP, "internal error: %s", e_.what()); }         \
    catch (...) { return fail(W2XC_ERR_HIP, "internal error"); }

struct HostLayer {
    int nin = 0, nout = 0;
    std::vector<float> w;       // [nout][nin][3][3], index o*nin+i (modelHandler.cpp:102)
    std::vector<double> bias;   // modelHandler.cpp:109-112 keeps doubles
    // upconv head models (include/w2xc_hip.h): the last layer is the head -- w is [nin][nout][4][4] -- and plane counts below 32 between the layers are
    // zero-padded to 32 (pad_head_model, w2xc_model.cpp): nin / nout / w / bias above are what the engine runs, nin0 / nout0 / w0 what the model declares
    // (w0 empty: w as it is).  Models without a head are never padded.
    bool head = false;
    int nin0 = 0, nout0 = 0;
    std::vector<float> w0;
    int decl_nin() const { return nin0 ? nin0 : nin; }
    int decl_nout() const { return nout0 ? nout0 : nout; }
};

struct DevLayer {
    W2xcKernelKind fast = W2XC_K_DIRECT;
    float *w_fast = nullptr;
    float *w_direct = nullptr;
    float *w_wino = nullptr;     // w2xc_wino_pack image (fp32 Winograd path, 32x32x2 kernel), packed on first use
    float *w_first2 = nullptr;  // w2xc_first2_wino4_pack image (layer 2 of the fused first two layers), packed on first use
    float *w_wino4 = nullptr;    // w2xc_wino4_pack image (F(4x4,3x3) kernel), packed on first use
    float *w_split[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // conv3x3_split images, index terms + 3*fmt, packed on first use
    float split_scale[6] = {1, 1, 1, 1, 1, 1};                                   // power-of-two weight scale of each image
    float *w_last_fused[4] = {nullptr, nullptr, nullptr, nullptr};   // w2xc_split_pack_last images: [0] 2 bf16 terms, [1] 2 fp16 terms, [2] 3 bf16 terms, [3] 1 bf16 term
    float last_fused_scale[4] = {1, 1, 1, 1};
    float *w_last_wino4 = nullptr;    // w2xc_wino4_pack_last image (fp32 path: last layer inside conv3x3_wino4's epilogue)
    float *w_alpha = nullptr;         // w2xc_upconv_pack_alpha image (a three-plane upconv head: channel 1 alone, the RGBA call's alpha head), uploaded with the model
    float *bias = nullptr;
};

struct ProfEvent {
    hipEvent_t a, b;
    int layer;
};

// The host->host tile farm of one (model, device): everything a w2xc_convert_plane call needs beyond the
// kernels, created once and kept (no hipMalloc / hipStreamCreate / hipHostMalloc on the per-call path):
//   three streams   s_h2d: staging ring -> d_in      s_compute: the layer launches of every band
//                   s_d2h: d_out -> staging ring     (ordered by events; copies run on the SDMA engines)
//   d_in / d_out    this device's share of the caller's plane (source rows incl. halo / output rows)
//   pin_in/pin_out  rings of pinned staging slots between the caller's pageable planes and the DMA engines
// This is the parallel replacement of the sequential block walk of convertRoutine.cpp:114-165.
struct HostPipe {
    static constexpr int IN_SLOTS = 3, OUT_SLOTS = 4;
    hipStream_t s_compute = nullptr, s_h2d = nullptr, s_d2h = nullptr;
    Scratch d_in, d_out;
    Scratch pin_in{Scratch::PINNED}, pin_out{Scratch::PINNED};   // IN_SLOTS / OUT_SLOTS slots each (default policy: ROCm places pinned host memory near the allocating device)
    size_t in_slot_bytes() const { return pin_in.bytes() / IN_SLOTS; }
    size_t out_slot_bytes() const { return pin_out.bytes() / OUT_SLOTS; }
    hipEvent_t ev_in_slot[IN_SLOTS] = {}, ev_out_slot[OUT_SLOTS] = {};   // last DMA that used the slot
    hipEvent_t ev_input = nullptr, ev_chunk = nullptr;                   // band input landed / last-layer chunk computed
    hipEvent_t ev_batch[4] = {};   // w2xc_convert_batch: [slot] = the layers of the sub-batch in device slot `slot` done, [2 + slot] = its download done
    // conv3x3_wino4 PROG: two page-locked band buffers the gather jobs write the output rows into over PCIe (bands alternate), and their job flags
    Scratch pin_band[2] = {Scratch(Scratch::PINNED_COHERENT), Scratch(Scratch::PINNED_COHERENT)};
    ProgFlags flags[2];
    bool ready = false;

    void destroy()   // streams and events; the buffers are the context's (DevCtx::for_each_scratch)
    {
        hipStream_t *const streams[3] = {&s_compute, &s_h2d, &s_d2h};
        for (hipStream_t *s : streams) if (*s) hipStreamSynchronize(*s);
        for (auto &e : ev_in_slot) if (e) { hipEventDestroy(e); e = nullptr; }
        for (auto &e : ev_out_slot) if (e) { hipEventDestroy(e); e = nullptr; }
        if (ev_input) { hipEventDestroy(ev_input); ev_input = nullptr; }
        if (ev_chunk) { hipEventDestroy(ev_chunk); ev_chunk = nullptr; }
        for (auto &e : ev_batch) if (e) { hipEventDestroy(e); e = nullptr; }
        for (hipStream_t *s : streams) if (*s) { hipStreamDestroy(*s); *s = nullptr; }
        ready = false;
    }
};

// Model::filter at the host boundary (w2xc_layer_filter): persistent device buffers, a pinned bounce ring and one stream
// per (model, device), and what the previous call left on the device for a caller that chains filter() by hand
// (the reference's test.cpp:72-85 pattern) -- see w2xc_opts.filter_resident.
struct FilterCache {
    static constexpr int SLOTS = 2;
    Scratch planar[2], nhwc[2];   // ping-pong: a call reads [ob ^ 1], writes [ob]
    Scratch pad, pout;            // conv3x3_wino4: the replicate-padded planar copy of the input planes / an aligned planar result
    Scratch pin{Scratch::PINNED};   // SLOTS pinned bounce slots between the caller's pageable planes and the DMA engine
    size_t slot_bytes() const { return pin.bytes() / SLOTS; }
    hipStream_t st = nullptr;
    hipEvent_t ev[SLOTS] = {};
    int ob = 0;                     // buffer index the LAST call wrote
    bool res_valid = false, res_nhwc = false;
    int res_planes = 0, res_w = 0, res_h = 0;
    std::vector<const float *> res_host;   // the host planes the result was downloaded to
    size_t res_stride = 0;
};

struct DevCtx {
    int device = 0;
    std::vector<DevLayer> layers;
    Scratch ws[2];              // the two ping-pong activation workspaces
    HostPipe pipe;
    FilterCache fc;
    Scratch prog_cnt;           // conv3x3_wino4 PROG: gather-job counters of the launch in flight (zeroed by the launcher)
    Scratch aux;                // N2: Y/U/V planes of the image pipeline
    Scratch img_io;             // N2, host entry points: device copies of the uint8 image in / out
    std::vector<ProfEvent> pending, pool;
    std::vector<double> layer_ms;
    std::vector<int> layer_launches;
    std::mutex mu;

    // THE list of the context's grow-only buffers: destruction, w2xc_model_trim and w2xc_debug_fill_scratch go by it and by nothing else
    template <class F> void for_each_scratch(F f)
    {
        for (auto &s : ws) f(s, ScratchTag::DATA);
        f(aux, ScratchTag::DATA);
        f(img_io, ScratchTag::DATA);
        f(prog_cnt, ScratchTag::SYNC);
        for (Scratch *s : {&pipe.d_in, &pipe.d_out, &pipe.pin_in, &pipe.pin_out, &pipe.pin_band[0], &pipe.pin_band[1]}) f(*s, ScratchTag::DATA);
        for (auto &fl : pipe.flags) f(fl.words, ScratchTag::SYNC);
        for (Scratch *s : {&fc.planar[0], &fc.planar[1], &fc.nhwc[0], &fc.nhwc[1], &fc.pad, &fc.pout, &fc.pin}) f(*s, ScratchTag::DATA);
    }

    ~DevCtx()
    {
        int prev = 0;
        hipGetDevice(&prev);
        hipSetDevice(device);
        for (auto &l : layers) {   // the weights: uploaded once (upload, w2xc_model.cpp), not scratch
            for (float *p : {l.w_fast, l.w_direct, l.w_wino, l.w_wino4, l.w_first2, l.w_last_wino4, l.w_alpha, l.bias}) if (p) hipFree(p);
            for (float *p : l.w_split) if (p) hipFree(p);
            for (float *p : l.w_last_fused) if (p) hipFree(p);
        }
        pipe.destroy();
        if (fc.st) hipStreamSynchronize(fc.st);
        for (auto &e : fc.ev) if (e) hipEventDestroy(e);
        if (fc.st) hipStreamDestroy(fc.st);
        for_each_scratch([](Scratch &s, ScratchTag) { s.release(); });
        for (auto &e : pending) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
        for (auto &e : pool) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
        hipSetDevice(prev);
    }
};

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) return;
        ok = (dev == prev) || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) hipSetDevice(prev);
    }
};

}  // namespace w2xc_eng

struct w2xc_model {
    std::vector<w2xc_eng::HostLayer> layers;
    bool has_head() const { return !layers.empty() && layers.back().head; }
    std::mutex mu;
    std::map<int, std::unique_ptr<w2xc_eng::DevCtx>> ctx;
};

namespace w2xc_eng {

// ---- w2xc_model.cpp ----
w2xc_opts resolve_opts(const w2xc_opts *o);
int njob();                                  // modelUtility's nJob (w2xc_get_jobs)
int upload(const std::vector<float> &h, float **d);
int get_ctx(w2xc_model *m, int device, DevCtx **out);
int prof_begin(DevCtx *c, int layer, hipStream_t st, ProfEvent *ev);

// The contexts of the (up to two) models of a call on `dev` (the image calls: noise and scale; the plane calls: their one model as msc); with l1 / l2 they are
// locked, TOGETHER (std::lock's deadlock avoidance; one model is one plain lock): two threads that pass the same two models in opposite roles -- (A as noise, B as
// scale) and (B as noise, A as scale) -- would otherwise each hold one mutex and wait for the other.  The plane buffers and the host pipeline are the owning context's.
struct CallCtx {
    DevCtx *cn = nullptr, *cs = nullptr;
    DevCtx *owner() const { return cs ? cs : cn; }
};
inline int call_contexts(w2xc_model *mn, w2xc_model *msc, int dev, CallCtx *ic, std::unique_lock<std::mutex> *l1 = nullptr, std::unique_lock<std::mutex> *l2 = nullptr)
{
    int rc;
    if (mn && (rc = get_ctx(mn, dev, &ic->cn))) return rc;
    if (msc && (rc = get_ctx(msc, dev, &ic->cs))) return rc;
    if (!l1) return W2XC_OK;
    // (at least one model: the entry points refuse a call without any before a context is asked for)
    if (ic->cn && ic->cs && ic->cn != ic->cs) {
        *l1 = std::unique_lock<std::mutex>(ic->cn->mu, std::defer_lock);
        *l2 = std::unique_lock<std::mutex>(ic->cs->mu, std::defer_lock);
        std::lock(*l1, *l2);
    } else *l1 = std::unique_lock<std::mutex>(ic->owner()->mu);
    return W2XC_OK;
}
// ... on the device of a call (dev < 0: the current one), selected and locked until this goes out of scope -- what every device entry point opens behind its
// argument checks.  The lock covers the enqueue; the device guard outlives the lock (members are destroyed in reverse order).
struct LockedCtx : CallCtx {
    std::optional<DeviceGuard> guard;
    std::unique_lock<std::mutex> l1, l2;
    int open(w2xc_model *mn, w2xc_model *msc, int dev)
    {
        if (dev < 0) HIP_TRY(hipGetDevice(&dev));
        guard.emplace(dev);
        if (!guard->ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", dev);
        return call_contexts(mn, msc, dev, this, &l1, &l2);
    }
};

// what the argument checks of the entry points share -- a w x h plane: positive and, where `cap` (the calls that compute with twice the size, or with a batch of them), at most 2^28 a side
inline int check_plane_size(int w, int h, bool cap)
{
    if (w <= 0 || h <= 0) return fail(W2XC_ERR_ARG, "plane size must be positive (got %dx%d)", w, h);
    return cap && (w > (1 << 28) || h > (1 << 28)) ? fail(W2XC_ERR_ARG, "plane too large") : W2XC_OK;
}
// the row strides (bytes) of float planes in_w wide in and out_w wide out
inline int check_row_strides(size_t in_stride, size_t in_w, size_t out_stride, size_t out_w)
{
    const bool ok = in_stride >= in_w * 4 && out_stride >= out_w * 4 && !((in_stride | out_stride) & 3);
    return ok ? W2XC_OK : fail(W2XC_ERR_ARG, "row strides must be multiples of 4 bytes and >= 4*width");
}
// bytes from the first pixel of an image (a plane) of `rows` rows of w pixels of px bytes to behind its last one
inline size_t image_extent(int rows, size_t stride, int w, int px) { return (size_t)(rows - 1) * stride + (size_t)w * px; }
inline bool ranges_overlap(const void *in, size_t in_extent, const void *out, size_t out_extent)
{
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
    return i0 < o0 + out_extent && o0 < i0 + in_extent;
}

// what every entry point but w2xc_convert_planes_up2x_device and w2xc_process_image_rgb_u8_ex[_device] -- and, since 0.4.1.6.1, their batch / TTA forms
// w2xc_convert_planes_up2x_batch_device and w2xc_process_image_rgb_u8_up2x_batch[_device], since 0.4.1.6.2 w2xc_process_image_rgba_u8_up2x_batch[_device] --
// answers for an upconv head model, in its argument checks (no device is touched; the message is pinned by tests/test_upconv_api.py)
inline int refuse_head(const w2xc_model *m, const char *call)
{
    if (!m || !m->has_head()) return W2XC_OK;
    return fail(W2XC_ERR_UNSUPPORTED, "%s: the model ends in an upconv head (a 2x transposed convolution); such models run through "
                "w2xc_convert_planes_up2x_device and w2xc_process_image_rgb_u8_ex[_device] only", call);
}

// ---- w2xc_select.cpp ----
// the fast path's kernel kind for layer l by its shape: w2xc_pick_kernel, but the head of an upconv model is W2XC_K_UPCONV and the 128 -> 256 layer in
// front of one is a W2XC_K_MFMA layer (conv3x3_wino4 alone has a kernel for it: resolve_chain turns it into W2XC_K_DIRECT for every other choice)
W2xcKernelKind pick_kind(const w2xc_model *m, int l);
int split_terms(const w2xc_opts &o);
int split_fmt(const w2xc_opts &o);
enum MidVariant { MID_MFMA = 0, MID_WINO32 = 1, MID_WINO4 = 3 };

// What a model runs with given options, decided ONCE (resolve_chain) and handed around as data: every consumer -- the plan, the descriptors, the launch
// strategies, the batch rule, the image routes, w2xc_layer_kernel_name -- reads this table and takes no selection decision of its own.
struct LayerPick {            // what runs layer l (0-based) and what it leaves behind
    W2xcKernelKind kind = W2XC_K_DIRECT;   // the kernel kind that runs it (W2XC_K_FUSED_AWAY: the next layer's launch does)
    int midv = MID_MFMA;      // which kernel runs a W2XC_K_MFMA layer (MID_MFMA for every other kind)
    bool wino4 = false;       // fp32 and conv3x3_wino4 (F(4x4,3x3)) runs it
    int out_terms = 0;        // of its output: 0 = fp32 activations, T = 16-bit term planes, 9 = the partial tap planes of the last layer it computes in its epilogue
    bool planar_out = false;  // its output (= layer l + 1's input) is planar planes, not NHWC pixels
    int halves = 0;           // out_terms == 9: partial planes per tap (wave columns of the split tile shapes, 64-plane blocks of conv3x3_wino4)
};
struct Chain {
    int T = 0, fmt = 0;       // 16-bit terms per activation value (0 = fp32) and their format: split_terms / split_fmt of the options
    bool fused_first = false, fused_last = false;   // layers 1 + 2 in one launch / the last layer inside the epilogue of the one before it (either precision)
    bool prog_gather = false; // fp32, fused_last: the producing launch may finish the last layer itself (conv3x3_wino4 PROG)
    bool any_wino4 = false;   // some layer is a wino4 layer: the band geometry needs four halo rows per layer
    bool u8_source = false, u8_sink = false;   // the RGB image pipeline: layer 1 may read / the last layer may write the caller's interleaved uint8 image itself
    std::vector<LayerPick> layer;
};
// resolved per call (no cache on the model or the context: nothing to invalidate, nothing shared between threads)
Chain resolve_chain(const w2xc_model *m, const w2xc_opts &o);

// the band geometry of one run_rows call (plan_rows, w2xc_select.cpp): pure host arithmetic
struct RowPlan {
    w2xc_opts o;              // the options the call runs with (W2XC_FUSION_AUTO gives up a fusion whose kernel cannot address the plane)
    Chain chain;              // resolve_chain(m, o), for exactly that o
    int n = 0, w = 0, plane_h = 0;
    int HL = 1;               // halo rows per layer: 1, or 4 = the banding-invariant geometry of conv3x3_wino4
    int band = 0;             // output rows per band
    bool last_direct = false, all_out = false;
    W2xcKernelKind last_kind = W2XC_K_DIRECT;
    size_t need[2] = {0, 0};  // bytes of the two ping-pong workspaces for one band
    void region(int k, int y0, int y1, int &T_, int &B_) const;
    void ws_need(const w2xc_model *m, int rows, size_t need_[2]) const;
};
int plan_rows(const w2xc_model *m, const w2xc_opts &o_in, int w, int vh, int vy0, int ra, int rb, int plane_h, int n_in, bool all_out, RowPlan *p);

// the buffer a layer of a band reads: the caller's view (layer 1) or what the layer before it wrote
struct LayerSrc {
    const float *p = nullptr;
    long long rs = 0, ps = 1, cs = 0, ts = 0, gs = 0;
    int halves = 0, h = 0, w = 0;
    int top = 0;   // first plane row it holds
};
// where a band's layers write: `out` = the caller's rows of this band (the last layer when P.last_direct), ws = the two ping-pong workspaces
struct LayerDst {
    float *out;
    long long out_rs, out_cs;
    float *ws[2];
};
// The launch descriptor *d of layer k (1 .. n) of the band [y0, y1) (no HIP call), the kind that runs it, and *next = what layer k + 1 reads.  first_d keeps
// layer 1's input description from the W2XC_K_FUSED_AWAY call (no launch: *d is not to be used) to layer 2's.  run_band (w2xc_rows.cpp) is the one loop that builds with this.
W2xcKernelKind layer_desc(const w2xc_model *m, const RowPlan &P, int k, int y0, int y1, int up, const LayerSrc &src, const LayerDst &dst,
                          W2xcConvDesc &first_d, W2xcConvDesc *d, LayerSrc *next);

// ---- w2xc_rows.cpp ----
// midv = LayerPick::midv of layer l (which kernel runs a W2XC_K_MFMA layer); bd != nullptr: the batch form of the launch (conv3x3_first2_wino4 / conv3x3_wino4 / the gather; conv3x3_first / conv3x3_wino / conv3x3_last) on bd->batch images
int launch_layer(DevCtx *c, const w2xc_model *m, int l, W2xcKernelKind kind, int midv, W2xcConvDesc d, hipStream_t st, const w2xc_opts &o,
                 const W2xcBatchDesc *bd = nullptr);

// Hooks of the host->host tile farm into the band loop (all optional; enqueue-only, never synchronise the device):
struct BandHooks {
    int out_chunk_rows = 0;                              // > 0: the last layer of a band is launched in row chunks of at most this size,
    int out_chunk_min = 0;                               //      tapering to this size at the end of the band (the exposed D2H tail)
    std::function<int(int, int)> input_needed;           // before layer 1 of band [y0, y1): make the launch stream wait for its input rows
    // layer 1 in row chunks while the band's input is still arriving: in_chunk(y0, y1) > 0 = output rows of layer 1 per chunk
    // (0: the band's rows are already staged / one launch); input_upto(v) = make the launch stream wait for view rows <= v
    std::function<int(int, int)> in_chunk;
    // optional: rows of the chunk that starts at output row c0 of the launch's region (multiples of 8; <= 0 = in_chunk's value) -- the first chunks of a call
    // are short, so that the first launch follows the first kilobytes of the upload and not its first 2 MiB slice
    std::function<int(int)> in_chunk_at;
    std::function<int(int)> input_upto;
    std::function<int(int, int)> prefetch;               // layers 1..n-1 of the current band are enqueued; [y0, y1) = the NEXT band
    std::function<int(int, int)> output_ready;           // output rows [r0, r1) have been enqueued on the launch stream
    // conv3x3_wino4 PROG (the launch of layer n - 1 finishes the last layer itself, rows completing in order): prog_begin hands out where the band's output
    // rows [y0, y1) go -- page-locked host memory the kernel writes over PCIe -- and the job flags (tile_rows x groups words) with the value a finished job
    // stores; out == nullptr on return: not available, the chunked path runs.  prog_launched: the launch is enqueued; job (jr, jg) holds the band's rows
    // [16 jr - first, 16 jr - first + 16) clipped, columns [256 jg, 256 jg + 256).
    struct ProgTail { float *out = nullptr; long long out_stride_f = 0; unsigned *flags = nullptr; unsigned epoch = 0; };
    std::function<int(int, int, int, int, ProgTail *)> prog_begin;
    std::function<int(int, int, int, int, int)> prog_launched;
};

// planes of one size in device memory, in FLOATS: plane i at p + i * ps, its rows rs apart.  The uint8 forms of run_rows (ROWS_U8_SRC / ROWS_U8_DST below) keep
// the type: p is the reinterpret-cast pointer to the interleaved image, rs its row stride in BYTES, ps = 1 (the channels lie one byte apart).
template <class T> struct Planes {
    T *p; size_t rs; long long ps;
    Planes from(size_t i) const { return {p + i * ps, rs, ps}; }    // the planes from plane i on
    Planes plane(size_t i) const { return {p + i * ps, rs, 0}; }    // plane i alone
    operator Planes<const T>() const { return {p, rs, ps}; }
};
typedef Planes<const float> PlanesIn;   // (a PlanesOut converts to it)
typedef Planes<float> PlanesOut;

// u8 (the RGB image pipeline; no hooks): ROWS_U8_SRC = `in` is an interleaved uint8 image of three channels (layer 1 runs as W2XC_K_FIRST_U8); ROWS_U8_DST =
// the same for `out` and the last layer (W2XC_K_LAST_U8).  The caller asks only where the chain's u8_source / u8_sink say yes.
// The RGBA call for upconv head models (w2xc_process_image_rgba_u8_up2x_batch*) reads and writes the caller's 4-byte pixels with three more, each beside the
// flag of its side:
//   ROWS_U8_SRC_A    `in` points at the ALPHA byte of an RGBA image and in.ps = 0: pixels 4 bytes apart, all three input planes that byte -- the grey image
//                    (A, A, A) without its copy
//   ROWS_U8_DST_PX4  the pixels of `out` are 4 bytes apart (a head model's last layer only): the three channels go to bytes 0 .. 2 of RGBA pixels
//   ROWS_U8_DST_A    channel 1 only (a three-plane head only): the alpha head (W2XC_K_UPCONV_A_U8) writes ONE byte per pixel, at out.p -- the caller points it
//                    at byte 3 of the first pixel
// And one form with FLOAT planes (the alpha pass of the RGBA TTA call for head models):
//   ROWS_F32_DST_A   channel 1 only of a three-plane head, as ONE float plane at out.p (W2XC_K_UPCONV_A: the alpha head's image and bias[1] with the float sink)
enum { ROWS_U8_SRC = 1, ROWS_U8_DST = 2, ROWS_U8_SRC_A = 4, ROWS_U8_DST_PX4 = 8, ROWS_U8_DST_A = 16, ROWS_F32_DST_A = 32 };
// One run_rows call: output rows [ra, rb) of convertWithModels on a plane of plane_h rows, w wide.
struct RowsCall {
    // the source view: n_in planar input planes in.ps floats apart, of which `in` holds rows [view_y0, view_y0 + view_h) -- every row in [ra - n, rb + n)
    // clipped to the plane must be inside the view
    PlanesIn in;
    int n_in, view_h, view_y0;
    // plane_h = rows of the whole plane (the units of view_h / view_y0 / ra / rb), 0 = unknown.  With it, and a view that holds 4 n halo rows, the layers run
    // on the banding-invariant geometry conv3x3_wino4 needs (plan_rows); without, W2XC_KERNEL_AUTO is refused (W2XC_ERR_ARG).
    int w, plane_h, ra, rb;
    // where rows [ra, rb) go (out.p = row ra).  out.ps != 0: ALL planes of the last layer, planar, that many floats apart (w2xc_convert_planes_*); 0 = plane 0
    // only -- with n_in == 1 convertWithModels proper, which returns only outputPlanes[0] (convertRoutine.cpp:78).
    PlanesOut out;
    // up = 1 folds a nearest-neighbour 2x (main.cpp:132-140) into layer 1: view_h, view_y0, w, plane_h, ra, rb are then in UPSCALED coordinates while `in`
    // holds the (view_h / 2) x (w / 2) source rows starting at source row view_y0 / 2.
    int up, u8;              // (u8: ROWS_U8_SRC | ROWS_U8_DST, and the forms of the RGBA head call beside them)
    const BandHooks *hk;     // the host pipeline's hooks into the band loop
    // the common case: the whole plane of a W x H result (view = plane, every row), no hooks
    static RowsCall whole(PlanesIn in, int n_in, int W, int H, PlanesOut out, int up, int u8 = 0) { return {in, n_in, H, 0, W, H, 0, H, out, up, u8, nullptr}; }
};
int run_rows(w2xc_model *m, DevCtx *c, const RowsCall &r, hipStream_t st, const w2xc_opts &o_in);
// what w2xc_convert_planes[_nn2x]_device refuses (no device is touched); o = the resolved options
int check_planes_args(const w2xc_model *m, int up, int n_in_planes, const void *d_in, size_t in_plane_stride, size_t in_stride, int w, int h, const void *d_out,
                      size_t out_plane_stride, size_t out_stride, const w2xc_opts &o);

// ---- batches of same-size planes (w2xc_convert_batch*) ----
// a batched launch chain runs a call planned as P (one image of the batch): fp32, W2XC_KERNEL_AUTO, the whole image in one band, and either conv3x3_first2_wino4 ->
// conv3x3_wino4 (planar) ... -> conv3x3_wino4 FUSE7 -> gather with one plane in and out, or -- three planes in, three out -- conv3x3_first -> conv3x3_wino /
// conv3x3_wino4 ... -> conv3x3_last, or -- a three-plane upconv head model -- -> upconv4x4_head.  Everything else takes the single-image launch sequence per image.
bool batch_eligible(const w2xc_model *m, const RowPlan &P);
// images per sub-batch for a per-image workspace of img_floats[2] floats under the call's workspace_mb budget (>= 1)
int batch_sub_size(const w2xc_opts &o, const size_t img_floats[2]);
// the nimg planes `out` of the (w << up) x (h << up) conversion of the w x h source planes `in` on `st`; enqueue-only.  max_sub > 0 caps the sub-batch
// size.  The caller holds c->mu.
int run_batch(w2xc_model *m, DevCtx *c, int nimg, int up, PlanesIn in, int w, int h, PlanesOut out, hipStream_t st, const w2xc_opts &o_in, int max_sub = 0);
// nimg IMAGES of planes: image i's planes start in_is / out_is floats behind image 0's, in.ps / out.ps apart (out.ps != 0: all planes of the last layer;
// 0: plane 0 alone, as RowsCall).  u8 (ROWS_U8_SRC / ROWS_U8_DST, with ROWS_U8_SRC_A / ROWS_U8_DST_PX4 / ROWS_U8_DST_A): that side is interleaved uint8 images
// as in RowsCall, its image stride in BYTES.
struct BatchIO {
    PlanesIn in; long long in_is; int n_in;
    PlanesOut out; long long out_is;
    int u8;
};
int run_batch_planes(w2xc_model *m, DevCtx *c, int nimg, int up, const BatchIO &io, int w, int h, hipStream_t st, const w2xc_opts &o_in, int max_sub = 0);
// per-image workspace floats of the batched chain (0, 0 when P is not eligible) -- what a sub-batch of k images needs is k times this
void batch_ws_floats(const RowPlan &P, size_t img_floats[2]);
int check_batch_model(const w2xc_model *m);
int check_batch_args(const w2xc_model *m, int nimg, int nn2x, int w, int h, size_t in_stride, size_t out_stride, bool head_call = false);
int check_batch_device_args(const w2xc_model *m, int n, int nn2x, const void *d_in, size_t in_plane_stride, size_t in_stride, int w, int h, const void *d_out,
                            size_t out_plane_stride, size_t out_stride);
int check_planes_batch_device_args(const w2xc_model *m, int n, int nn2x, int n_in_planes, const void *d_in, size_t in_image_stride, size_t in_plane_stride,
                                   size_t in_stride, int w, int h, const void *d_out, size_t out_image_stride, size_t out_plane_stride, size_t out_stride,
                                   const w2xc_opts &o, bool head_call = false);
// byte ranges [lo, hi) tagged 1 = output, 0 = input (sorted in place): W2XC_ERR_ARG when an output overlaps another output or an input
int check_batch_overlap(std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> &iv);

// ---- w2xc_host_pipeline.cpp: what the host batch forms share (w2xc_convert_batch: float planes, w2xc_process_image_u8_batch: uint8 images) ----
int host_devices(const w2xc_opts &o, std::vector<int> *devs);   // the devices of w2xc_opts.device_mask that exist (W2XC_ERR_HIP: none at all)
// n host images of one size in and out, in BYTES, and the two things the pipeline cannot know
struct HostBatch {
    int n = 0;
    const void *const *in = nullptr;
    void *const *out = nullptr;
    size_t in_stride = 0, out_stride = 0;   // the caller's row strides
    size_t in_row = 0, out_row = 0;         // bytes of one row
    int in_rows = 0, out_rows = 0;
    size_t in_img = 0, out_img = 0;         // bytes per image in the device slots (a multiple of 256)
    // the context(s) of device `dev` and their lock(s); *pipe = the host pipeline (three streams, device slots, pinned rings) the call runs through
    std::function<int(int dev, std::unique_lock<std::mutex> &l1, std::unique_lock<std::mutex> &l2, HostPipe **pipe)> acquire;
    // enqueue cnt images din -> dout (device slots, images in_img / out_img bytes apart) on st, no synchronisation; max_sub = the call's largest sub-batch
    std::function<int(int dev, int cnt, const void *din, void *dout, hipStream_t st, int max_sub)> run;
};
// sub-batches of at most `sub` images striped over the devices, one worker thread each: upload of k + 1 || launches of k || download of k - 1
int batch_host_run(const HostBatch &b, const w2xc_opts &o, int sub);
// no null image pointer, no output range [out[i], out[i] + out_ext) that overlaps another output or an input (check_batch_overlap)
int check_batch_host_ptrs(int n, const void *const *in, size_t in_ext, void *const *out, size_t out_ext);

}  // namespace w2xc_eng
