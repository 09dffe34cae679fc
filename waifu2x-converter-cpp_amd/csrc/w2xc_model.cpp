// w2xc_model.cpp -- error state, the model container + JSON loader (the reference's Model / modelUtility,
// src/modelHandler.{hpp,cpp}), the per-(model, device) contexts that hold packed weights and workspaces, and the
// measurement entry points of include/w2xc_hip.h.
#include "w2xc_engine.hpp"

#include <cmath>
#include <fstream>
#include <iostream>
#include <sstream>

#include "json_min.hpp"

namespace w2xc_eng {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// modelUtility singleton state (modelHandler.hpp:92-100)
static std::mutex g_util_mu;
static int g_njob = 4;
static int g_block_w = 512, g_block_h = 512;

int njob() { std::lock_guard<std::mutex> lk(g_util_mu); return g_njob; }

// what `opts == NULL` resolves to (w2xc_set_default_opts): w2xc_opts_init's defaults + the two environment variables the library reads
static std::mutex g_defaults_mu;
static w2xc_opts g_defaults;
static bool g_defaults_set = false;
static w2xc_opts env_defaults()
{
    w2xc_opts r;
    w2xc_opts_init(&r);
    // callers that pass no options (the C++ adapter behind the reference's CLI): the default precision can
    // be switched without recompiling -- W2XC_PRECISION = fp32 | bf16x3 | fp16x2 | bf16x2 | bf16
    if (const char *e = getenv("W2XC_PRECISION")) {
        if (!strcmp(e, "bf16x3")) r.precision = W2XC_PRECISION_BF16X3;
        else if (!strcmp(e, "bf16x2")) r.precision = W2XC_PRECISION_BF16X2;
        else if (!strcmp(e, "fp16x2")) r.precision = W2XC_PRECISION_FP16X2;
        else if (!strcmp(e, "bf16")) r.precision = W2XC_PRECISION_BF16;
    }
    if (const char *e = getenv("W2XC_FILTER_RESIDENT")) r.filter_resident = atoi(e) != 0 ? 1 : 0;
    return r;
}

w2xc_opts resolve_opts(const w2xc_opts *o)
{
    w2xc_opts r;
    if (o) {
        w2xc_opts_init(&r);
        size_t n = o->struct_size > 0 && (size_t)o->struct_size < sizeof(w2xc_opts) ? (size_t)o->struct_size : sizeof(w2xc_opts);
        memcpy(&r, o, n);
        r.struct_size = (int)sizeof(w2xc_opts);
    } else {
        std::lock_guard<std::mutex> lk(g_defaults_mu);
        if (!g_defaults_set) { g_defaults = env_defaults(); g_defaults_set = true; }
        r = g_defaults;
    }
    return r;
}

// ---- the failure seam (w2xc_debug_fail_nth): process-wide, three kinds of event ----
std::atomic<unsigned> g_fail_watch{0};
static std::atomic<long long> g_fail_seen[4], g_fail_armed[4];   // events since the last call of the entry point / events left until one fails (0: none)

bool fail_event_watched(int kind)
{
    if (!((g_fail_watch.load(std::memory_order_relaxed) >> kind) & 1u)) return false;
    g_fail_seen[kind].fetch_add(1, std::memory_order_relaxed);
    long long left = g_fail_armed[kind].load(std::memory_order_relaxed);
    while (left > 0)   // (events of several threads: exactly one of them takes the count from 1 to 0)
        if (g_fail_armed[kind].compare_exchange_weak(left, left - 1, std::memory_order_relaxed)) return left == 1;
    return false;
}

// A weight image: *d = a device copy of h, or -- on any failure -- null with nothing allocated (a lazily packed image is tested by its pointer: `packed`,
// w2xc_rows.cpp).  A failed allocation is W2XC_ERR_NOMEM like every other one, a failed copy W2XC_ERR_HIP.
int upload(const std::vector<float> &h, float **d)
{
    *d = nullptr;
    const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(float);
    hipError_t e = fail_event(W2XC_DEBUG_FAIL_ALLOC) ? hipErrorOutOfMemory : hipMalloc((void **)d, bytes);
    if (e != hipSuccess) {
        *d = nullptr;
        (void)hipGetLastError();
        return fail(W2XC_ERR_NOMEM, "allocating %zu bytes of device memory for a weight image failed: %s", bytes, hipGetErrorString(e));
    }
    e = fail_event(W2XC_DEBUG_FAIL_COPY) ? hipErrorUnknown : hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(*d);
        *d = nullptr;
        (void)hipGetLastError();
        return fail(W2XC_ERR_HIP, "hipMemcpy of a weight image (%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    return W2XC_OK;
}

// per-(model, device) context: packed weights + biases resident in HBM; created on first use
int get_ctx(w2xc_model *m, int device, DevCtx **out)
{
    std::lock_guard<std::mutex> lk(m->mu);
    auto it = m->ctx.find(device);
    if (it != m->ctx.end()) { *out = it->second.get(); return W2XC_OK; }
    std::unique_ptr<DevCtx> c(new DevCtx());
    c->device = device;
    c->layers.resize(m->layers.size());
    c->layer_ms.assign(m->layers.size(), 0.0);
    c->layer_launches.assign(m->layers.size(), 0);
    for (size_t l = 0; l < m->layers.size(); l++) {
        const HostLayer &hl = m->layers[l];
        DevLayer &dl = c->layers[l];
        int rc;
        std::vector<float> pk;
        if (hl.head) {   // the head has one kernel and one image (a shape without it: plan_rows refuses the call)
            dl.fast = W2XC_K_UPCONV;
            if (w2xc_upconv_supported(hl.nin, hl.nout)) {
                pk.resize(w2xc_upconv_packed_floats(hl.nin, hl.nout));
                w2xc_upconv_pack(hl.nin, hl.nout, hl.w.data(), pk.data());
                if ((rc = upload(pk, &dl.w_fast))) return rc;
                if (hl.nout == 3) {   // the alpha head of the RGBA call: channel 1 alone, 16 * nin floats
                    pk.resize(w2xc_upconv_packed_floats(hl.nin, 1));
                    w2xc_upconv_pack_alpha(hl.nin, hl.w.data(), pk.data());
                    if ((rc = upload(pk, &dl.w_alpha))) return rc;
                }
            }
        } else {
            dl.fast = w2xc_pick_kernel(hl.nin, hl.nout);
            pk.resize(w2xc_packed_weight_floats(W2XC_K_DIRECT, hl.nin, hl.nout));
            w2xc_pack_weights(W2XC_K_DIRECT, hl.nin, hl.nout, hl.w.data(), pk.data());
            if ((rc = upload(pk, &dl.w_direct))) return rc;
            if (dl.fast != W2XC_K_DIRECT) {
                pk.assign(w2xc_packed_weight_floats(dl.fast, hl.nin, hl.nout), 0.f);
                w2xc_pack_weights(dl.fast, hl.nin, hl.nout, hl.w.data(), pk.data());
                if ((rc = upload(pk, &dl.w_fast))) return rc;
            }
        }
        std::vector<float> bf(hl.nout);
        for (int o = 0; o < hl.nout; o++) bf[o] = (float)hl.bias[o];   // cv::add(UMat, double) narrows to the array depth
        rc = upload(bf, &dl.bias);
        if (rc) return rc;
    }
    *out = c.get();
    m->ctx[device] = std::move(c);
    return W2XC_OK;
}

// An upconv head model as the engine runs it: plane counts below 32 between its layers zero-padded to 32 -- zero weights and zero bias for the added output
// planes of a 3x3 layer (leaky(0) = 0: those planes are exact zeros), zero weights for the added input planes of the layer behind it (exact zeros added to
// its sums) -- so that 3 -> 16 -> 32 of the published topology runs as conv3x3_first 3 -> 32 and a 32 -> 32 layer instead of conv3x3_direct.  The model's own
// planes (layer 1's input, the head's output) stay.  What the model declares is kept beside (HostLayer::nin0 / nout0 / w0) for the getters.
static void pad_head_model(w2xc_model *m)
{
    const int n = (int)m->layers.size();
    for (int l = 0; l < n; l++) {
        HostLayer &hl = m->layers[l];
        hl.nin0 = hl.nin; hl.nout0 = hl.nout;
        const int nin_p = (l > 0 && hl.nin < 32) ? 32 : hl.nin, nout_p = (!hl.head && hl.nout < 32) ? 32 : hl.nout;
        if (nin_p == hl.nin && nout_p == hl.nout) continue;
        hl.w0 = hl.w;
        hl.w.assign((size_t)nin_p * nout_p * (hl.head ? 16 : 9), 0.f);
        if (hl.head) w2xc_pad_head(hl.nin, hl.nout, nin_p, hl.w0.data(), hl.w.data());
        else w2xc_pad_layer(hl.nin, hl.nout, nin_p, nout_p, hl.w0.data(), hl.w.data());
        hl.bias.resize(nout_p, 0.0);
        hl.nin = nin_p; hl.nout = nout_p;
    }
}

int prof_begin(DevCtx *c, int layer, hipStream_t st, ProfEvent *ev)
{
    if (!c->pool.empty()) { *ev = c->pool.back(); c->pool.pop_back(); }
    else {
        HIP_TRY(hipEventCreate(&ev->a));
        hipError_t e = hipEventCreate(&ev->b);
        if (e != hipSuccess) {
            hipEventDestroy(ev->a);
            return fail(W2XC_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
        }
    }
    ev->layer = layer;
    const hipError_t e = hipEventRecord(ev->a, st);
    if (e != hipSuccess) {
        c->pool.push_back(*ev);   // (the pair stays the context's)
        return fail(W2XC_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
    }
    return W2XC_OK;
}

}  // namespace w2xc_eng

using namespace w2xc_eng;

extern "C" {

void w2xc_opts_init(w2xc_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->struct_size = (int)sizeof(w2xc_opts);
    o->precision = W2XC_PRECISION_FP32;
    o->kernel = W2XC_KERNEL_AUTO;
    o->device = -1;
}

void w2xc_opts_init_sized(w2xc_opts *o, size_t struct_size)
{
    if (!o || struct_size < 4 * sizeof(int)) return;   // (struct_size, precision, kernel, device: every version of the struct has them)
    w2xc_opts full;
    w2xc_opts_init(&full);
    const size_t n = std::min(struct_size, sizeof(w2xc_opts));
    full.struct_size = (int)n;
    memcpy(o, &full, n);
}

int w2xc_set_default_opts(const w2xc_opts *defaults)
{
    w2xc_opts r;
    if (defaults) {
        w2xc_opts_init(&r);
        const size_t n = defaults->struct_size > 0 && (size_t)defaults->struct_size < sizeof(w2xc_opts) ? (size_t)defaults->struct_size : sizeof(w2xc_opts);
        memcpy(&r, defaults, n);
        r.struct_size = (int)sizeof(w2xc_opts);
    } else {
        r = env_defaults();
    }
    std::lock_guard<std::mutex> lk(g_defaults_mu);
    g_defaults = r;
    g_defaults_set = true;
    return W2XC_OK;
}

const char *w2xc_last_error(void) { return g_last_error.c_str(); }
// 0.2: w2xc_opts grew (host_numa; 56 bytes), W2XC_FUSION_FIRST / _LAST, w2xc_opts_init_sized, w2xc_set_default_opts, w2xc_plan_rows; since 0.1 (rounds 3-5)
// also: W2XC_KERNEL_WINOGRAD = _WINOGRAD32, W2XC_KERNEL_AUTO refused on a minimum-halo row view, `verbose` a bit mask (INTEGRATION.md "ABI history")
// 0.3: w2xc_convert_batch / w2xc_convert_batch_device; 0.4: w2xc_debug_fill_scratch (both additive, no struct change)
// 0.4.1: the RGB image calls (w2xc_process_image_rgb_u8*), w2xc_convert_planes_nn2x_device, w2xc_u8_to_rgb_device / w2xc_rgb_to_u8_device (additive)
// 0.4.1.1: the RGBA image calls (w2xc_process_image_rgba_u8_ex[_device]), w2xc_bleed_rgba_u8_device / _trim (additive; the prefix "w2xc_hip 0.4.1" stays -- callers
// find the symbols by lookup)
// 0.4.1.2: test-time augmentation -- w2xc_process_image_[rgb_]u8[_batch]_tta[_device], w2xc_convert_batch_tta_device / w2xc_convert_planes_tta_device,
//          w2xc_tta_spread_device / w2xc_tta_gather_device (additive; w2xc_opts stays 56 bytes)
// 0.4.1.3: the batch forms of the RGBA call, w2xc_process_image_rgba_u8_batch[_device] (additive; w2xc_opts stays 56 bytes)
// 0.4.1.4: w2xc_resize_linear_device, the INTER_LINEAR resize of the image calls' shrink as a building block (additive; w2xc_opts stays 56 bytes)
// 0.4.1.5: w2xc_convert_planes_batch_device (n images of several planes: the batched chain of RGB models) and w2xc_batch_plan (additive; w2xc_opts stays 56 bytes)
// 0.4.1.6: upconv head models -- w2xc_model_add_upconv_head, w2xc_model_has_head, w2xc_convert_planes_up2x_device; the JSON loader takes a last layer that is
//          an nn.SpatialFullConvolution 4x4 / stride 2 / padding 3; every other entry point refuses such a model (additive; w2xc_opts stays 56 bytes)
// 0.4.1.6.1: the batch and TTA forms for upconv head models -- w2xc_convert_planes_up2x_batch_device, w2xc_process_image_rgb_u8_up2x_batch[_device] (with tta),
// w2xc_batch_plan with nn2x = 2; no struct change, and every existing call refuses a head model as before.
// 0.4.1.6.2: the RGBA call for upconv head models -- w2xc_process_image_rgba_u8_up2x_batch[_device] (additive; w2xc_opts stays 56 bytes).  The string below
// stays at 0.4.1.6.1 (callers compare it for equality): the new revision is found by the presence of the symbols.
// 0.4.1.7: YUV frames -- w2xc_process_frames_yuv_u8[_device], w2xc_y8_to_plane_device, w2xc_plane_to_y8_device, w2xc_chroma2x_u8_device and the struct
// w2xc_yuv_planes (additive; w2xc_opts stays 56 bytes; the string stays, the revision is found by the presence of the symbols).
// 0.4.1.8: YUV frames through RGB and head models -- w2xc_process_frames_yuv_u8_rgb[_device], w2xc_yuv8_to_rgb_device, w2xc_rgb_to_yuv8_device and the constants
// W2XC_MATRIX_* (additive; w2xc_opts stays 56 bytes; the string stays, the revision is found by the presence of the symbols).
// 0.4.1.9: 16-bit YUV frames -- w2xc_process_frames_yuv_u16[_rgb][_device], w2xc_y16_to_plane_device, w2xc_plane_to_y16_device, w2xc_chroma2x_u16_device,
// w2xc_yuv16_to_rgb_device, w2xc_rgb_to_yuv16_device, the struct w2xc_yuv16_planes and W2XC_PACK_* (additive; w2xc_opts stays 56 bytes; the string stays).
// 0.4.1.12: w2xc_debug_fail_nth and W2XC_DEBUG_FAIL_* (test aid, additive; w2xc_opts stays 56 bytes; the string stays, the revision is found by the symbol).
const char *w2xc_version(void) { return "w2xc_hip 0.4.1.6.1 (gfx950)"; }

int w2xc_plan_rows(const w2xc_model *m, int w, int view_y0, int view_h, int plane_h, int row_begin, int row_end, const w2xc_opts *opts, w2xc_row_plan *plan)
try {
    if (!m || !plan) return fail(W2XC_ERR_ARG, "null argument");
    const int n = (int)m->layers.size();
    if (w <= 0 || plane_h <= 0 || row_begin < 0 || row_end > plane_h || row_begin >= row_end)
        return fail(W2XC_ERR_ARG, "bad row range [%d,%d) for a %d-row plane", row_begin, row_end, plane_h);
    if (view_y0 < 0 || view_h <= 0 || view_y0 + view_h > plane_h || view_y0 > std::max(0, row_begin - n) || view_y0 + view_h < std::min(plane_h, row_end + n))
        return fail(W2XC_ERR_ARG, "view rows [%d,%d) do not cover [%d,%d) +- %d halo rows", view_y0, view_y0 + view_h, row_begin, row_end, n);
    RowPlan P;
    int rc = plan_rows(m, resolve_opts(opts), w, view_h, view_y0, row_begin, row_end, plane_h, m->layers.empty() ? 1 : m->layers[0].nin, false, &P);
    if (rc) return rc;
    w2xc_row_plan r;
    memset(&r, 0, sizeof r);
    r.struct_size = (int)sizeof r;
    r.n_layers = P.n;
    r.halo_rows_per_layer = P.HL;
    r.band_rows = P.band;
    r.n_bands = (row_end - row_begin + P.band - 1) / P.band;
    r.fused_first = P.chain.fused_first ? 1 : 0;
    r.fused_last = P.chain.fused_last ? 1 : 0;
    r.workspace_bytes[0] = P.need[0];
    r.workspace_bytes[1] = P.need[1];
    const size_t nb = plan->struct_size > 0 && (size_t)plan->struct_size < sizeof r ? (size_t)plan->struct_size : sizeof r;
    r.struct_size = (int)nb;
    memcpy(plan, &r, nb);
    return W2XC_OK;
} W2XC_CATCH_ALL

int w2xc_plan_region(const w2xc_row_plan *plan, int plane_h, int layer, int y0, int y1, int *top, int *bottom)
{
    if (!plan || !top || !bottom || layer < 1 || layer > plan->n_layers || y0 >= y1) return fail(W2XC_ERR_ARG, "bad argument");
    RowPlan P;
    P.n = plan->n_layers;
    P.HL = plan->halo_rows_per_layer;
    P.plane_h = plane_h;
    P.region(layer, y0, y1, *top, *bottom);
    return W2XC_OK;
}

int w2xc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- model container ---------------------------------------------------------------------------
int w2xc_model_from_arrays(int n_layers, const int *nin, const int *nout, const float *const *weight,
                           const double *const *bias, w2xc_model **out)
try {
    if (!out || n_layers <= 0 || !nin || !nout || !weight || !bias) return fail(W2XC_ERR_ARG, "bad argument");
    std::unique_ptr<w2xc_model> m(new w2xc_model());
    m->layers.resize(n_layers);
    for (int l = 0; l < n_layers; l++) {
        if (nin[l] <= 0 || nout[l] <= 0 || !weight[l] || !bias[l]) return fail(W2XC_ERR_ARG, "bad layer %d", l);
        HostLayer &hl = m->layers[l];
        hl.nin = nin[l];
        hl.nout = nout[l];
        hl.w.assign(weight[l], weight[l] + (size_t)nin[l] * nout[l] * 9);
        hl.bias.assign(bias[l], bias[l] + nout[l]);
    }
    *out = m.release();
    return W2XC_OK;
} catch (const std::bad_alloc &) {
    return fail(W2XC_ERR_NOMEM, "out of memory while copying the model");
}

int w2xc_model_add_upconv_head(w2xc_model *m, int nout, const float *weight, const double *bias)
try {
    if (!m || !weight) return fail(W2XC_ERR_ARG, "null argument");
    if (nout != 1 && nout != 3) return fail(W2XC_ERR_ARG, "an upconv head gives 1 or 3 planes (got %d)", nout);
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    if (m->has_head()) return fail(W2XC_ERR_ARG, "the model has a head already");
    if (!m->ctx.empty()) return fail(W2XC_ERR_ARG, "w2xc_model_add_upconv_head must come before the model's first use on a device");
    HostLayer hl;
    hl.head = true;
    hl.nin = m->layers.back().nout;
    hl.nout = nout;
    hl.w.assign(weight, weight + (size_t)hl.nin * nout * 16);
    hl.bias.assign(nout, 0.0);
    if (bias) hl.bias.assign(bias, bias + nout);
    m->layers.push_back(std::move(hl));
    pad_head_model(m);
    return W2XC_OK;
} catch (const std::bad_alloc &) {
    return fail(W2XC_ERR_NOMEM, "out of memory while copying the head");
}

int w2xc_model_has_head(const w2xc_model *m) { return m && m->has_head() ? 1 : 0; }

// the number behind an optional numeric key of a layer object (absent or not a number: `missing`)
static double json_num(const jsonmin::Value &o, const char *key, double missing)
{
    const jsonmin::Value *v = o.find(key);
    return v && v->is_number() ? v->num : missing;
}

// Is element o of the model array -- the last one -- the head of an upconv model?  kW = kH = 4, dW = dH = 2, padW = padH = 3, and class_name, if present,
// "nn.SpatialFullConvolution" (include/w2xc_hip.h).  Anything else with a 4x4 kernel is a non-3x3 layer like any other.
static bool json_is_head(const jsonmin::Value &o)
{
    if (json_num(o, "kW", 0) != 4 || json_num(o, "kH", 0) != 4) return false;
    if (json_num(o, "dW", 0) != 2 || json_num(o, "dH", 0) != 2 || json_num(o, "padW", -1) != 3 || json_num(o, "padH", -1) != 3) return false;
    const jsonmin::Value *cn = o.find("class_name");
    return !cn || (cn->type == jsonmin::Value::String && cn->str == "nn.SpatialFullConvolution");
}

static int model_load_json_impl(const char *path, w2xc_model **out)
{
    if (!path || !out) return fail(W2XC_ERR_ARG, "null argument");
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) {
        std::cerr << "Error : couldn't open " << path << std::endl;   // modelHandler.cpp:176-178
        return fail(W2XC_ERR_IO, "Error : couldn't open %s", path);
    }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();   // c_str() is NUL-terminated: strtod cannot overrun
    jsonmin::Value root;
    std::string err;
    jsonmin::Parser p(text.c_str(), text.c_str() + text.size());
    if (!p.parse(root, err)) {
        std::cerr << "Error : JSON Error : " << err << std::endl;      // modelHandler.cpp:183-186
        return fail(W2XC_ERR_JSON, "Error : JSON Error : %s", err.c_str());
    }
    if (!root.is_array() || root.arr.empty()) return fail(W2XC_ERR_JSON, "model file is not a non-empty JSON array of layers");
    std::unique_ptr<w2xc_model> m(new w2xc_model());
    for (size_t l = 0; l < root.arr.size(); l++) {   // one Model per element (:189-194)
        const jsonmin::Value &o = root.arr[l];
        if (!o.is_object()) return fail(W2XC_ERR_JSON, "layer %zu is not an object", l);
        const jsonmin::Value *nip = o.find("nInputPlane"), *nop = o.find("nOutputPlane"), *kw = o.find("kW"),
                             *kh = o.find("kH"), *wv = o.find("weight"), *bv = o.find("bias");
        const bool head = l + 1 == root.arr.size() && l > 0 && json_is_head(o);   // (its bias may be absent: upstream builds the head with :noBias())
        if (!nip || !nop || !kw || !kh || !wv || (!bv && !head) || !nip->is_number() || !nop->is_number() || !kw->is_number() ||
            !kh->is_number() || !wv->is_array() || (bv && !bv->is_array()))
            return fail(W2XC_ERR_JSON, "layer %zu lacks one of nInputPlane/nOutputPlane/kW/kH/weight/bias", l);
        HostLayer hl;
        // the reference casts these doubles straight to int (modelHandler.hpp:50-51); a library first makes sure the cast
        // is defined and the sizes are sane (NaN / 1e300 / a hostile plane count must not reach resize())
        auto small_int = [](double v) { return std::isfinite(v) && v >= 0.0 && v <= 65536.0; };
        if (!small_int(nip->num) || !small_int(nop->num) || !small_int(kw->num) || !small_int(kh->num))
            return fail(W2XC_ERR_JSON, "layer %zu: nInputPlane / nOutputPlane / kW / kH out of range", l);
        hl.nin = (int)nip->num;     // static_cast<int>(double), modelHandler.hpp:50-51
        hl.nout = (int)nop->num;
        const int ks = (int)kw->num;
        if (ks != (int)kh->num) {   // the reference exit(-1)s here (hpp:52-58); a library reports it
            std::cerr << "Error : Model-Constructor : \nkernel in model is not square.\nstop." << std::endl;
            return fail(W2XC_ERR_UNSUPPORTED, "kernel in model is not square");
        }
        if (ks != 3 && !head) return fail(W2XC_ERR_UNSUPPORTED, "layer %zu: kernel size %d; only 3x3 is supported (convertWithModels pads by the layer count, which assumes 3x3)", l, ks);
        if (hl.nin <= 0 || hl.nout <= 0 || hl.nin > 4096 || hl.nout > 4096) return fail(W2XC_ERR_JSON, "layer %zu: bad plane counts (%d, %d)", l, hl.nin, hl.nout);
        if (head) {   // weight[nInputPlane][nOutputPlane][4][4], torch's layout of nn.SpatialFullConvolution
            if (hl.nout != 1 && hl.nout != 3) return fail(W2XC_ERR_UNSUPPORTED, "layer %zu: an upconv head gives 1 or 3 planes (got %d)", l, hl.nout);
            if ((int)wv->arr.size() != hl.nin || (bv && (int)bv->arr.size() < hl.nout))
                return fail(W2XC_ERR_JSON, "layer %zu: weight/bias outer size does not match nInputPlane / nOutputPlane of the head", l);
            hl.head = true;
            hl.w.resize((size_t)hl.nin * hl.nout * 16);
            hl.bias.assign(hl.nout, 0.0);
            for (int i = 0; i < hl.nin; i++) {
                const jsonmin::Value &wi = wv->arr[i];
                if (!wi.is_array() || (int)wi.arr.size() != hl.nout) return fail(W2XC_ERR_JSON, "layer %zu: weight[%d] size != nOutputPlane", l, i);
                for (int oo = 0; oo < hl.nout; oo++) {
                    const jsonmin::Value &km = wi.arr[oo];
                    if (!km.is_array() || (int)km.arr.size() < 4) return fail(W2XC_ERR_JSON, "layer %zu: weight[%d][%d] is not a 4x4 matrix", l, i, oo);
                    for (int r = 0; r < 4; r++) {
                        const jsonmin::Value &row = km.arr[r];
                        if (!row.is_array() || (int)row.arr.size() < 4) return fail(W2XC_ERR_JSON, "layer %zu: weight[%d][%d][%d] too short", l, i, oo, r);
                        for (int cidx = 0; cidx < 4; cidx++) {
                            if (!row.arr[cidx].is_number()) return fail(W2XC_ERR_JSON, "layer %zu: non-numeric weight", l);
                            hl.w[((size_t)i * hl.nout + oo) * 16 + r * 4 + cidx] = (float)row.arr[cidx].num;
                        }
                    }
                }
            }
            for (int oo = 0; bv && oo < hl.nout; oo++) {
                if (!bv->arr[oo].is_number()) return fail(W2XC_ERR_JSON, "layer %zu: non-numeric bias", l);
                hl.bias[oo] = bv->arr[oo].num;
            }
            m->layers.push_back(std::move(hl));
            break;
        }
        if ((int)wv->arr.size() != hl.nout || (int)bv->arr.size() < hl.nout)
            return fail(W2XC_ERR_JSON, "layer %zu: weight/bias outer size does not match nOutputPlane", l);
        hl.w.resize((size_t)hl.nout * hl.nin * 9);
        hl.bias.resize(hl.nout);
        for (int oo = 0; oo < hl.nout; oo++) {
            const jsonmin::Value &wi = wv->arr[oo];
            if (!wi.is_array() || (int)wi.arr.size() != hl.nin) return fail(W2XC_ERR_JSON, "layer %zu: weight[%d] size != nInputPlane", l, oo);
            for (int i = 0; i < hl.nin; i++) {
                const jsonmin::Value &km = wi.arr[i];
                if (!km.is_array() || (int)km.arr.size() < ks) return fail(W2XC_ERR_JSON, "layer %zu: weight[%d][%d] is not a %dx%d matrix", l, oo, i, ks, ks);
                for (int r = 0; r < ks; r++) {
                    const jsonmin::Value &row = km.arr[r];
                    if (!row.is_array() || (int)row.arr.size() < ks) return fail(W2XC_ERR_JSON, "layer %zu: weight[%d][%d][%d] too short", l, oo, i, r);
                    for (int cidx = 0; cidx < ks; cidx++) {
                        if (!row.arr[cidx].is_number()) return fail(W2XC_ERR_JSON, "layer %zu: non-numeric weight", l);
                        hl.w[((size_t)oo * hl.nin + i) * 9 + r * 3 + cidx] = (float)row.arr[cidx].num;   // double -> float, :95-97
                    }
                }
            }
            if (!bv->arr[oo].is_number()) return fail(W2XC_ERR_JSON, "layer %zu: non-numeric bias", l);
            hl.bias[oo] = bv->arr[oo].num;   // stays double, :109-112
        }
        m->layers.push_back(std::move(hl));
    }
    if (m->has_head()) pad_head_model(m.get());
    *out = m.release();
    return W2XC_OK;
}

// no C++ exception may cross the C ABI: a hostile / truncated model file or an allocation failure becomes an error code
int w2xc_model_load_json(const char *path, w2xc_model **out)
{
    try {
        return model_load_json_impl(path, out);
    } catch (const std::bad_alloc &) {
        return fail(W2XC_ERR_NOMEM, "out of memory while loading %s", path ? path : "(null)");
    } catch (const std::exception &e) {
        return fail(W2XC_ERR_JSON, "Error : JSON Error : %s", e.what());
    } catch (...) {
        return fail(W2XC_ERR_JSON, "unknown error while loading the model");
    }
}

void w2xc_model_free(w2xc_model *m) { delete m; }

int w2xc_model_trim(w2xc_model *m)
{
    if (!m) return fail(W2XC_ERR_ARG, "null model");
    std::lock_guard<std::mutex> lk(m->mu);
    int prev = 0;
    hipGetDevice(&prev);
    for (auto &kv : m->ctx) {
        DevCtx *c = kv.second.get();
        std::lock_guard<std::mutex> lk2(c->mu);
        hipSetDevice(c->device);
        hipDeviceSynchronize();
        c->for_each_scratch([](Scratch &s, ScratchTag) { s.release(); });
        c->fc.res_valid = false;
    }
    hipSetDevice(prev);
    return W2XC_OK;
}
int w2xc_model_layers(const w2xc_model *m) { return m ? (int)m->layers.size() : 0; }
// (an upconv head model: the plane counts and weights the model declares, not the zero-padded ones the engine runs -- pad_head_model)
int w2xc_model_nin(const w2xc_model *m, int l) { return (m && l >= 0 && l < (int)m->layers.size()) ? m->layers[l].decl_nin() : -1; }
int w2xc_model_nout(const w2xc_model *m, int l) { return (m && l >= 0 && l < (int)m->layers.size()) ? m->layers[l].decl_nout() : -1; }

int w2xc_model_get_layer(const w2xc_model *m, int l, float *weight, double *bias)
{
    if (!m || l < 0 || l >= (int)m->layers.size()) return fail(W2XC_ERR_ARG, "bad layer index");
    const HostLayer &hl = m->layers[l];
    const std::vector<float> &w = hl.w0.empty() ? hl.w : hl.w0;
    if (weight) memcpy(weight, w.data(), w.size() * sizeof(float));
    if (bias) memcpy(bias, hl.bias.data(), (size_t)hl.decl_nout() * sizeof(double));
    return W2XC_OK;
}

// ---- modelUtility knobs --------------------------------------------------------------------------
int w2xc_set_jobs(int n)
{
    if (n < 1) return W2XC_ERR_ARG;   // modelHandler.cpp:200
    std::lock_guard<std::mutex> lk(g_util_mu);
    g_njob = n;
    return W2XC_OK;
}
int w2xc_get_jobs(void) { std::lock_guard<std::mutex> lk(g_util_mu); return g_njob; }
int w2xc_set_block_size(int w, int h)
{
    if (w < 0 || h < 0) return W2XC_ERR_ARG;   // :210
    std::lock_guard<std::mutex> lk(g_util_mu);
    g_block_w = w; g_block_h = h;
    return W2XC_OK;
}
int w2xc_set_block_size_exp2(int exp)
{
    if (exp < 0 || exp > 30) return W2XC_ERR_ARG;   // :216
    std::lock_guard<std::mutex> lk(g_util_mu);
    g_block_w = g_block_h = 1 << exp;
    return W2XC_OK;
}
void w2xc_get_block_size(int *w, int *h)
{
    std::lock_guard<std::mutex> lk(g_util_mu);
    if (w) *w = g_block_w;
    if (h) *h = g_block_h;
}

// ---- measurement ----------------------------------------------------------------------------------
int w2xc_profile_read(w2xc_model *m, int device, float *layer_ms, int *layer_launches, int n_layers)
{
    if (!m) return fail(W2XC_ERR_ARG, "null model");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    DevCtx *c = nullptr;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        auto it = m->ctx.find(device);
        if (it == m->ctx.end()) return fail(W2XC_ERR_ARG, "no context for device %d", device);
        c = it->second.get();
    }
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard guard(device);
    for (auto &e : c->pending) {
        HIP_TRY(hipEventSynchronize(e.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
        c->layer_ms[e.layer] += ms;
        c->layer_launches[e.layer] += 1;
        c->pool.push_back(e);
    }
    c->pending.clear();
    for (int l = 0; l < n_layers && l < (int)c->layer_ms.size(); l++) {
        if (layer_ms) layer_ms[l] = (float)c->layer_ms[l];
        if (layer_launches) layer_launches[l] = c->layer_launches[l];
    }
    return W2XC_OK;
}

void w2xc_profile_reset(w2xc_model *m, int device)
{
    if (!m) return;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(m->mu);
    auto it = m->ctx.find(device);
    if (it == m->ctx.end()) return;
    DevCtx *c = it->second.get();
    std::lock_guard<std::mutex> lk2(c->mu);
    for (auto &e : c->pending) c->pool.push_back(e);
    c->pending.clear();
    std::fill(c->layer_ms.begin(), c->layer_ms.end(), 0.0);
    std::fill(c->layer_launches.begin(), c->layer_launches.end(), 0);
}

// Test aid (tests/test_gpu_scratch_poison.py): every grow-only DATA buffer of the context, whole, so that a kernel which reads what its producer did not
// write meets `word` and not the previous call's answer.  Synchronisation words stay as they are -- prog_cnt, pipe.flags and their epochs, events: they are
// not data (ScratchTag::SYNC in DevCtx::for_each_scratch), a wrong value there could only make a launch wait for ever.  Weights and biases are not scratch.
int w2xc_debug_fill_scratch(w2xc_model *m, int device, unsigned word, unsigned long long *bytes)
{
    if (!m || !bytes) return fail(W2XC_ERR_ARG, "null argument");
    *bytes = 0;
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    DeviceGuard guard(device);
    if (!guard.ok) return fail(W2XC_ERR_HIP, "cannot select HIP device %d", device);
    DevCtx *c = nullptr;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        auto it = m->ctx.find(device);
        if (it == m->ctx.end()) return W2XC_OK;   // nothing to fill; the context is not created for this
        c = it->second.get();
    }
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long total = 0;
    hipError_t e = hipSuccess;
    c->for_each_scratch([&](Scratch &s, ScratchTag tag) {
        const size_t nbytes = s.bytes();
        if (tag != ScratchTag::DATA || !nbytes || e != hipSuccess) return;
        total += nbytes;
        if (s.on_device()) {
            e = hipMemsetD32((hipDeviceptr_t)s.as<char>(), (int)word, nbytes / 4);
            if (e == hipSuccess && (nbytes & 3)) e = hipMemsetD8((hipDeviceptr_t)(s.as<char>() + (nbytes & ~(size_t)3)), (unsigned char)word, nbytes & 3);
            return;
        }
        for (size_t i = 0; i < nbytes / 4; i++) s.as<unsigned>()[i] = word;   // (page-locked host memory: page aligned; the device was drained above)
        for (size_t i = nbytes & ~(size_t)3; i < nbytes; i++) s.as<unsigned char>()[i] = (unsigned char)word;
    });
    HIP_TRY(e);
    HIP_TRY(hipDeviceSynchronize());
    c->fc.res_valid = false;   // the resident copy w2xc_opts.filter_resident promises is gone
    *bytes = total;
    return W2XC_OK;
}

// Test aid (tests/test_gpu_fail_paths.py): see include/w2xc_hip.h.  The sites: Scratch::reserve and upload (ALLOC), upload (COPY), launch_layer (LAUNCH).
long long w2xc_debug_fail_nth(int kind, long long nth)
{
    if (kind < W2XC_DEBUG_FAIL_ALLOC || kind > W2XC_DEBUG_FAIL_LAUNCH || nth < 0) return -1;
    g_fail_watch.fetch_or(1u << kind, std::memory_order_relaxed);
    g_fail_armed[kind].store(nth, std::memory_order_relaxed);
    return g_fail_seen[kind].exchange(0, std::memory_order_relaxed);
}

const char *w2xc_layer_kernel_name(const w2xc_model *m, int layer, const w2xc_opts *opts)
{
    if (!m || layer < 0 || layer >= (int)m->layers.size()) return "";
    const w2xc_opts o = resolve_opts(opts);
    const Chain chain = resolve_chain(m, o);
    const LayerPick &L = chain.layer[layer];
    // (what the DEVICE entry points launch: conv3x3_wino4 PROG finishes the last layer itself there only on request; the host entry points always use it)
    if (L.kind == W2XC_K_LAST_GATHER && chain.prog_gather && o.fusion == W2XC_FUSION_PROG) return "(in_previous_layer)";
    if (L.midv != MID_MFMA) return L.midv == MID_WINO4 ? "conv3x3_wino4" : "conv3x3_wino";
    return w2xc_kernel_name(L.kind, m->layers[layer].nin, m->layers[layer].nout);
}

}  // extern "C"
