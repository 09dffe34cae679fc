// w2xc_host_pipeline.cpp -- host plane in -> host plane out (w2xc_convert_plane / _nn2x / _rows): per (model, device) a
// persistent pipe of three HIP streams, device copies of the unit's rows and pinned staging rings; a feeder and a drainer
// thread per unit; units fan out over devices.  The parallel replacement of the sequential block walk of
// src/convertRoutine.cpp:114-165 (host-side gather only, no exchange between units).
#include "w2xc_engine.hpp"
#include <sched.h>
#include <pthread.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <thread>

#include "w2xc_copy_pool.hpp"
#include "w2xc_host_geom.hpp"

namespace w2xc_eng {

namespace {

// true when [p, p + bytes) is page-locked memory the DMA engines can address directly (hipHostMalloc /
// hipHostRegister, e.g. a pinned torch tensor): such planes skip the staging rings
bool host_range_pinned(const void *p, size_t bytes)
{
    if (!p || bytes == 0) return false;
    // both ends must be page-locked AND belong to ONE allocation / registration that spans the whole range: two registered
    // regions with a pageable (or unmapped) gap between them would pass a probe of the end points alone
    const void *base[2] = {nullptr, nullptr};
    int i = 0;
    for (const char *q : {(const char *)p, (const char *)p + bytes - 1}) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();   // an unregistered pointer is not an error of ours
            return false;
        }
        if (at.type != hipMemoryTypeHost) return false;
        hipDeviceptr_t b = nullptr;
        size_t sz = 0;
        if (hipMemGetAddressRange(&b, &sz, (hipDeviceptr_t)at.devicePointer) == hipSuccess && b && sz) {
            const char *hb = (const char *)at.hostPointer - ((const char *)at.devicePointer - (const char *)b);   // host address of the allocation's start
            if ((const char *)p < hb || (const char *)p + bytes > hb + sz) return false;
            base[i] = hb;
        } else {
            (void)hipGetLastError();
            base[i] = nullptr;   // range unknown for this kind of registration: fall back to comparing what we have
        }
        i++;
    }
    return base[0] == base[1];
}

int pipe_init(HostPipe &p)
{
    if (p.ready) return W2XC_OK;
    HIP_TRY(hipStreamCreateWithFlags(&p.s_compute, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&p.s_h2d, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&p.s_d2h, hipStreamNonBlocking));
    for (auto &e : p.ev_in_slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : p.ev_out_slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_input, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p.ev_chunk, hipEventDisableTiming));
    p.ready = true;
    return W2XC_OK;
}

// ---- NUMA placement of a device's host pipeline (multi-socket hosts: the pinned rings and the threads that fill / drain them belong
// on the CPU node the GPU hangs off, or every staged byte crosses the inter-socket link twice).  w2xc_opts.host_numa = 1 disables. ----
int numa_node_of_device(int dev)
{
    int node = -1;
    if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, dev) == hipSuccess && node >= 0) return node;
    (void)hipGetLastError();
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *q = bus; *q; q++) *q = (char)tolower(*q);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

// the CPUs of a node ("0-63,128-191" in /sys/devices/system/node/nodeN/cpulist); false when unknown or the node has none
bool cpus_of_node(int node, cpu_set_t *set)
{
    if (node < 0) return false;
    char path[96];
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    char buf[4096] = {0};
    const size_t got = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[got] = 0;
    CPU_ZERO(set);
    int count = 0;
    for (const char *q = buf; *q;) {
        char *end = nullptr;
        const long a = strtol(q, &end, 10);
        if (end == q) break;
        long b = a;
        q = end;
        if (*q == '-') { b = strtol(q + 1, &end, 10); q = end; }
        for (long cpu = a; cpu <= b && cpu < CPU_SETSIZE; cpu++) { CPU_SET((int)cpu, set); count++; }
        while (*q == ',' || *q == '\n' || *q == ' ') q++;
    }
    return count > 0;
}

// Binds the calling thread to a device's CPU node for its lifetime and restores the previous affinity afterwards
struct NodeCpus { int node = -1; bool have = false; cpu_set_t set; };
const NodeCpus &node_cpus_of_device(int dev)   // looked up once per device: no /sys read or attribute query on the per-call path
{
    static std::mutex mu;
    static std::map<int, NodeCpus> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    NodeCpus nc;
    nc.node = numa_node_of_device(dev);
    nc.have = cpus_of_node(nc.node, &nc.set);
    return cache.emplace(dev, nc).first->second;
}
struct NodeAffinity {
    cpu_set_t prev;
    bool bound = false;
    int node = -1;
    explicit NodeAffinity(int dev, bool enabled)
    {
        if (!enabled) return;
        const NodeCpus &nc = node_cpus_of_device(dev);
        node = nc.node;
        if (!nc.have) return;
        const cpu_set_t want = nc.set;
        if (pthread_getaffinity_np(pthread_self(), sizeof prev, &prev) != 0) return;
        cpu_set_t both;
        CPU_AND(&both, &prev, &want);          // never leave the set the caller (or a cgroup) already confined us to
        if (CPU_COUNT(&both) == 0) return;
        bound = pthread_setaffinity_np(pthread_self(), sizeof both, &both) == 0;
    }
    ~NodeAffinity() { if (bound) pthread_setaffinity_np(pthread_self(), sizeof prev, &prev); }
};

// grow-only device rows and pinned staging rings of the pipe (a slot size of 0: no ring needed, the planes are page-locked)
int pipe_reserve(HostPipe &p, size_t in_bytes, size_t out_bytes, size_t in_slot, size_t out_slot)
{
    int rc = p.d_in.reserve(in_bytes, "the input rows");
    if (!rc) rc = p.d_out.reserve(out_bytes, "the output rows");
    if (!rc) rc = p.pin_in.reserve(in_slot * HostPipe::IN_SLOTS, "the input staging ring");
    if (!rc) rc = p.pin_out.reserve(out_slot * HostPipe::OUT_SLOTS, "the output staging ring");
    return rc;
}

// (debug aid) the clock of one unit's phase timestamps on stderr: w2xc_opts.verbose & 2
struct Trace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// The input side of one unit: source rows [0, svh) of its view (`src` = view row 0), uploaded in order up to a high-water mark -- DMA'd straight from a
// page-locked plane, staged through the pinned ring otherwise.
struct Uploader {
    HostPipe &p;
    const char *src;
    size_t in_stride, in_row;
    int w, svh, chunk_rows, copy_threads;
    bool pinned;
    const Trace &tr;
    int uploaded = 0;    // view rows already queued on s_h2d
    long seq = 0;        // staging slots used so far
    double t_done = -1;

    // view rows < s_end are queued on s_h2d; compute_waits: and the launch stream waits for them
    int upto(int s_end, bool compute_waits = false)
    {
        s_end = std::min(s_end, svh);
        float *const d_in = p.d_in.as<float>();
        while (uploaded < s_end) {
            if (pinned) {   // DMA straight from the caller's plane
                const int rows = s_end - uploaded;
                const char *from = src + (size_t)uploaded * in_stride;
                if (in_stride == in_row) HIP_TRY(hipMemcpyAsync(d_in + (size_t)uploaded * w, from, (size_t)rows * in_row, hipMemcpyHostToDevice, p.s_h2d));
                else HIP_TRY(hipMemcpy2DAsync(d_in + (size_t)uploaded * w, in_row, from, in_stride, in_row, rows, hipMemcpyHostToDevice, p.s_h2d));
                uploaded = s_end;
                break;
            }
            const int rows = std::min(chunk_rows, s_end - uploaded);
            const int slot = (int)(seq % HostPipe::IN_SLOTS);
            if (seq >= HostPipe::IN_SLOTS) HIP_TRY(hipEventSynchronize(p.ev_in_slot[slot]));   // its last DMA has read it
            char *stage = p.pin_in.as<char>() + (size_t)slot * p.in_slot_bytes();
            w2xc_host::CopyPool::get().copy_rows(stage, in_row, src + (size_t)uploaded * in_stride, in_stride, in_row, rows, copy_threads);
            HIP_TRY(hipMemcpyAsync(d_in + (size_t)uploaded * w, stage, (size_t)rows * in_row, hipMemcpyHostToDevice, p.s_h2d));
            HIP_TRY(hipEventRecord(p.ev_in_slot[slot], p.s_h2d));
            seq++;
            uploaded += rows;
        }
        if (tr.on && t_done < 0 && uploaded >= svh) t_done = tr.ms();
        if (compute_waits) {
            HIP_TRY(hipEventRecord(p.ev_input, p.s_h2d));
            HIP_TRY(hipStreamWaitEvent(p.s_compute, p.ev_input, 0));
        }
        return W2XC_OK;
    }
};

// The output side of one unit whose plane is pageable: the drainer thread and everything it shares with the feeder.  The feeder takes a free staging slot,
// queues the D2H of a chunk into it and submits it; or, for a band whose last layer the launch of layer n - 1 finishes itself (conv3x3_wino4 PROG), waits
// until the band buffer is free and submits the band.  The drainer copies what arrives into the caller's plane (`out` = its row 0), in order.
class Stitcher {
public:
    Stitcher(HostPipe &p, int dev, char *out, size_t out_stride, size_t out_row, int copy_threads, const Trace &tr)
        : p_(p), dev_(dev), out_(out), out_stride_(out_stride), out_row_(out_row), copy_threads_(copy_threads), tr_(tr) {}
    ~Stitcher() { finish(); }   // (an exception in the feeder must not unwind past a joinable thread)

    int take_slot(int *slot)
    {
        std::unique_lock<std::mutex> ql(mu_);
        cv_.wait(ql, [&] { return queued_ - drained_ < HostPipe::OUT_SLOTS; });
        *slot = (int)(queued_ % HostPipe::OUT_SLOTS);
        return rc_.load();
    }
    // rows [r0, r1) arrive in staging slot `slot` behind its D2H event
    void submit_chunk(int r0, int r1, int slot) { push(Item{r0, r1, slot}, queued_); }
    // the band buffers alternate: band s waits until band s - 2 has been stitched (the drainer reads the buffer and its flags until then)
    int wait_band_free()
    {
        std::unique_lock<std::mutex> ql(mu_);
        cv_.wait(ql, [&] { return bands_drained_ >= bands_ - 1 || rc_.load() != W2XC_OK; });
        return rc_.load();
    }
    // rows [r0, r1) are written by a launch into the page-locked band buffer `src` and flagged per job: job (jr, jg) = rows [16 jr - first, 16 jr - first + 16)
    // x columns [256 jg, 256 jg + 256) of the band; the drainer follows the flags and stitches rows while the launch runs
    void submit_band(int r0, int r1, int trows, int groups, int first, const unsigned *flags, unsigned epoch, const char *src)
    {
        push(Item{r0, r1, -1, trows, groups, first, flags, epoch, src}, bands_);
    }
    long bands() const { return bands_; }   // (the feeder's own count)
    void finish()
    {
        if (!th_.joinable()) return;
        { std::lock_guard<std::mutex> ql(mu_); done_ = true; }
        cv_.notify_all();
        th_.join();
    }
    int rc() const { return rc_.load(); }
    const std::string &error() const { return err_; }   // after finish()

private:
    struct Item { int r0, r1, slot; int trows = 0, groups = 0, first = 0; const volatile unsigned *flags = nullptr; unsigned epoch = 0; const char *src = nullptr; };

    // (the thread starts with the first item it is handed, not at the call's start: creating a thread costs tens of microseconds the first upload would wait behind)
    void push(const Item &it, long &counter)
    {
        if (!th_.joinable()) th_ = std::thread([this] { run(); });
        {
            std::lock_guard<std::mutex> ql(mu_);
            pending_.push_back(it);
            counter++;
        }
        cv_.notify_all();
    }
    void run()
    {
        hipSetDevice(dev_);
        for (;;) {
            Item it;
            {
                std::unique_lock<std::mutex> ql(mu_);
                cv_.wait(ql, [&] { return !pending_.empty() || done_; });
                if (pending_.empty()) return;
                it = pending_.front();
                pending_.pop_front();
            }
            if (it.slot < 0) stitch_band(it);
            else if (rc_.load() == W2XC_OK) stitch_chunk(it);
            {
                std::lock_guard<std::mutex> ql(mu_);
                (it.slot < 0 ? bands_drained_ : drained_)++;
            }
            cv_.notify_all();
        }
    }
    void set_error(int code, const std::string &text) { err_ = text; rc_.store(code); }
    // `rows` rows from `src` (packed) to the caller's rows from row0 on (a std::bad_alloc / std::system_error on this thread would be std::terminate, not an error code)
    void copy_out(int row0, const char *src, int rows, const char *what)
    {
        try {
            w2xc_host::CopyPool::get().copy_rows(out_ + (size_t)row0 * out_stride_, out_stride_, src, out_row_, out_row_, rows, copy_threads_);
        }
        catch (const std::exception &ex) { set_error(W2XC_ERR_NOMEM, std::string("host copy of ") + what + " failed: " + ex.what()); }
        catch (...) { set_error(W2XC_ERR_NOMEM, std::string("host copy of ") + what + " failed"); }
    }
    void stitch_chunk(const Item &it)
    {
        const hipError_t e = hipEventSynchronize(p_.ev_out_slot[it.slot]);
        if (e != hipSuccess) return set_error(W2XC_ERR_HIP, std::string("hipEventSynchronize(D2H chunk) failed: ") + hipGetErrorString(e));
        copy_out(it.r0, p_.pin_out.as<char>() + (size_t)it.slot * p_.out_slot_bytes(), it.r1 - it.r0, "a downloaded chunk");
    }
    // follow the job flags: tile rows complete top to bottom (roughly); every run of finished tile rows is stitched at once
    void stitch_band(const Item &it)
    {
        const int R = it.r1 - it.r0;
        int jr = 0, runs = 0;
        long spins = 0;
        bool launch_over = false;
        double t_first_seen = 0, t_last_seen = 0;
        while (jr < it.trows && rc_.load() == W2XC_OK) {
            int ready = jr;
            while (ready < it.trows) {
                bool all = true;
                for (int g = 0; g < it.groups && all; g++) all = flag_reached(it.flags[(size_t)ready * it.groups + g], it.epoch);
                if (!all && !launch_over) break;
                ready++;
            }
            if (ready == jr) {
                // nothing new: the launch may be over (every row written, the flags' last stores included -- or it failed)
                if ((++spins & 1023) == 0) {
                    const hipError_t q = hipStreamQuery(p_.s_compute);
                    if (q == hipSuccess) launch_over = true;
                    else if (q != hipErrorNotReady) set_error(W2XC_ERR_HIP, std::string("the launch that finishes the last layer failed: ") + hipGetErrorString(q));
                }
#if defined(__x86_64__)
                __builtin_ia32_pause();
#endif
                continue;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            const auto [a, b] = tile_rows_span(jr, ready, it.first, R);
            const double t_seen = tr_.on ? tr_.ms() : 0.0;
            if (b > a) copy_out(it.r0 + a, it.src + (size_t)a * out_row_, b - a, "finished rows");
            if (tr_.on) {
                if (runs == 0) t_first_seen = t_seen;
                runs++;
                t_last_seen = t_seen;
            }
            jr = ready;
        }
        if (tr_.on) fprintf(stderr, "[w2xc host] rows %d..%d finished by the launch of layer n-1 itself: %d tile rows stitched in %d runs, first seen %.3f ms, last seen %.3f ms, "
                                    "stitched %.3f ms%s\n", it.r0, it.r1, it.trows, runs, t_first_seen, t_last_seen, tr_.ms(), launch_over ? " (the launch was over before its last flags were seen)" : "");
    }

    HostPipe &p_;
    const int dev_;
    char *const out_;
    const size_t out_stride_, out_row_;
    const int copy_threads_;
    const Trace &tr_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Item> pending_;      // submitted, not yet stitched (consumed in order)
    long queued_ = 0, drained_ = 0;             // slot chunks (slots are used round-robin)
    long bands_ = 0, bands_drained_ = 0;        // PROG bands handed over / stitched
    bool done_ = false;
    std::atomic<int> rc_{W2XC_OK};
    std::string err_;               // written before rc_, read by the feeder after finish()
    std::thread th_;
};

// Output rows [ra, rb) of the (w << up) x (h << up) conversion of the HOST plane `in` (h rows of w floats) on device
// `dev`, written to rows [ra, rb) of the HOST plane `out`.  One unit of the tile farm: the caller runs one of these
// per device (threads) or per rank (processes); units never exchange data.
//
//   feeder (this thread)   stages the band's source rows (Uploader: pageable -> pinned slot -> s_h2d), enqueues the band's
//                          layers on s_compute, stages the NEXT band's rows while it computes, then launches the
//                          last layer in row chunks and queues each chunk's D2H on s_d2h into a pinned slot
//   drainer (Stitcher)     waits for each chunk's D2H and copies it into the caller's plane (the "stitch" of
//                          convertRoutine.cpp:143-161), freeing the slot
// so H2D(band k+1) || layers(band k) || D2H + stitch(band k-1 / earlier chunks).  Planes that are already pinned
// are DMA'd in place without staging.
// hs = halo rows of the source view per side (convert_plane_host decides: n, or 4 n for the banding-invariant geometry of conv3x3_wino4)
int host_rows_on_device(w2xc_model *m, int dev, const float *in_, size_t in_stride, int w, int h, int up, int ra, int rb,
                        float *out_, size_t out_stride, const w2xc_opts &o, int copy_threads, int in_row0, int out_row0, int hs)
{
    // `in_` points at source row in_row0, `out_` at output row out_row0: rebase both to row 0 (only rows that exist are touched)
    const char *in = (const char *)in_ - (ptrdiff_t)in_row0 * (ptrdiff_t)in_stride;
    char *out = (char *)out_ - (ptrdiff_t)out_row0 * (ptrdiff_t)out_stride;
    HIP_TRY(hipSetDevice(dev));
    // this thread is the unit's feeder: it (and the drainer it starts, which inherits the affinity) runs on the device's CPU node, and
    // the pinned rings it allocates land there; the caller's affinity is restored on return
    NodeAffinity node_guard(dev, o.host_numa == 0);
    DevCtx *c = nullptr;
    int rc = get_ctx(m, dev, &c);
    if (rc) return rc;
    // the context (its workspace and pipe) stays locked for the whole call: calls that share a device serialise
    std::lock_guard<std::mutex> lk(c->mu);
    HostPipe &p = c->pipe;
    if ((rc = pipe_init(p))) return rc;

    // ---- planning ----
    const int W = w << up, H = h << up;
    const RowSpan sv = src_rows(ra, rb, hs, up, H);
    const int sy0 = sv.first, sy1 = sv.second, svh = sy1 - sy0;
    const size_t in_row = (size_t)w * 4, out_row = (size_t)W * 4;
    const char *in_lo = in + (size_t)sy0 * in_stride, *in_hi = in + (size_t)(sy1 - 1) * in_stride + in_row;
    const char *out_lo = out + (size_t)ra * out_stride, *out_hi = out + (size_t)(rb - 1) * out_stride + out_row;
    const bool in_pinned = host_range_pinned(in_lo, (size_t)(in_hi - in_lo)), out_pinned = host_range_pinned(out_lo, (size_t)(out_hi - out_lo));
    // in-place / overlapping planes (the reference never does this, main.cpp:94-96 copies first; a library must survive it):
    // the drainer writes band b's rows while later bands still read theirs, so every source row is staged before any output exists
    const bool overlap = ranges_overlap(in_lo, (size_t)(in_hi - in_lo), out_lo, (size_t)(out_hi - out_lo));
    const HostChunks ck = host_chunks(o.host_chunk_kb, in_row, out_row);
    const int l1_chunk = layer1_chunk(ck.in_rows, up);
    rc = pipe_reserve(p, (size_t)svh * in_row, (size_t)(rb - ra) * out_row, in_pinned ? 0 : (size_t)ck.in_rows * in_row, out_pinned ? 0 : (size_t)ck.out_rows * out_row);
    if (rc) return rc;
    const Trace tr{(o.verbose & 2) != 0, std::chrono::steady_clock::now()};
    double t_first_out = -1;
    Uploader input{p, in_lo, in_stride, in_row, w, svh, ck.in_rows, copy_threads, in_pinned, tr};
    Stitcher stitch(p, dev, out, out_stride, out_row, copy_threads, tr);
    auto src_end = [&](int y1) { return band_src_end(y1, hs, up, H, sy0, overlap, svh); };

    // ---- the hooks of the band loop: enqueue-only ----
    BandHooks hk;
    hk.out_chunk_rows = ck.out_rows;
    hk.out_chunk_min = ck.out_min;
    hk.input_needed = [&](int, int y1) -> int { return input.upto(src_end(y1), true); };
    hk.prefetch = [&](int, int y1n) -> int { return input.upto(src_end(y1n)); };
    // a band whose rows were prefetched under the previous band is launched whole; otherwise layer 1 follows the upload slice by slice
    hk.in_chunk = [&](int, int y1) -> int { return overlap || input.uploaded >= std::min(src_end(y1), svh) ? 0 : l1_chunk; };
    hk.in_chunk_at = [&](int c0) -> int {
        if (input.uploaded > 0 && c0 == 0) return 0;   // (a later band whose first rows were prefetched)
        return taper_chunk(c0, l1_chunk);              // (pageable: staged by the copy threads first)
    };
    hk.input_upto = [&](int vlast) -> int { return input.upto((vlast >> up) + 1, true); };
    hk.output_ready = [&](int r0, int r1) -> int {
        if (tr.on && t_first_out < 0) t_first_out = tr.ms();
        HIP_TRY(hipEventRecord(p.ev_chunk, p.s_compute));
        HIP_TRY(hipStreamWaitEvent(p.s_d2h, p.ev_chunk, 0));
        const float *d_out = p.d_out.as<float>();
        if (out_pinned) {
            char *dst = out + (size_t)r0 * out_stride;
            const float *src = d_out + (size_t)(r0 - ra) * W;
            if (out_stride == out_row) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)(r1 - r0) * out_row, hipMemcpyDeviceToHost, p.s_d2h));
            else HIP_TRY(hipMemcpy2DAsync(dst, out_stride, src, out_row, out_row, r1 - r0, hipMemcpyDeviceToHost, p.s_d2h));
            return W2XC_OK;
        }
        for (int a = r0; a < r1; a += ck.out_rows) {   // (an unchunked last layer reports the whole band at once)
            const int b2 = std::min(r1, a + ck.out_rows);
            int slot;
            int r = stitch.take_slot(&slot);
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(p.pin_out.as<char>() + (size_t)slot * p.out_slot_bytes(), d_out + (size_t)(a - ra) * W, (size_t)(b2 - a) * out_row,
                                   hipMemcpyDeviceToHost, p.s_d2h));
            HIP_TRY(hipEventRecord(p.ev_out_slot[slot], p.s_d2h));
            stitch.submit_chunk(a, b2, slot);
        }
        return W2XC_OK;
    };
    // conv3x3_wino4 PROG: the band's rows are written by the launch of layer n - 1 itself, into the caller's plane when it is page-locked, else into one of
    // two page-locked band buffers (bands alternate) and flagged per job for the drainer
    hk.prog_begin = [&](int y0, int y1, int trows, int groups, BandHooks::ProgTail *pt) -> int {
        if (o.fusion == W2XC_FUSION_GATHER_LAUNCH) return W2XC_OK;   // (pt->out stays null: the chunked launches + gather of rounds 4 / 5)
        if (out_pinned) {   // nothing to stitch: the rows are complete when the launch is (the closing synchronisation)
            pt->out = (float *)(out + (size_t)y0 * out_stride);
            pt->out_stride_f = (long long)(out_stride / 4);
            pt->flags = nullptr;
            return W2XC_OK;
        }
        const int par = (int)(stitch.bands() & 1);
        ProgFlags &fl = p.flags[par];
        // (first: the drainer may still read this buffer and its flags for band s - 2, and either may be about to grow)
        int r = stitch.wait_band_free();
        if (!r) r = p.pin_band[par].reserve((size_t)(y1 - y0) * out_row, "the band buffer");
        if (!r) r = fl.reserve((size_t)trows * groups);
        if (r) return r;
        pt->out = p.pin_band[par].as<float>();
        pt->out_stride_f = (long long)W;
        pt->flags = fl.words.as<unsigned>();
        pt->epoch = fl.next_epoch();   // (nothing is in flight on this buffer)
        return W2XC_OK;
    };
    hk.prog_launched = [&](int y0, int y1, int trows, int groups, int first) -> int {
        if (tr.on && t_first_out < 0) t_first_out = tr.ms();
        if (out_pinned) return W2XC_OK;
        const int par = (int)(stitch.bands() & 1);
        stitch.submit_band(y0, y1, trows, groups, first, p.flags[par].words.as<unsigned>(), p.flags[par].epoch(), p.pin_band[par].as<char>());
        return W2XC_OK;
    };

    RowsCall r = RowsCall::whole({p.d_in.as<float>(), (size_t)w, 0}, 1, W, H, {p.d_out.as<float>(), (size_t)W, 0}, up);   // (of that plane: this unit's rows, from the source rows staged for them)
    r.view_h = svh << up; r.view_y0 = sy0 << up; r.ra = ra; r.rb = rb; r.hk = &hk;
    rc = run_rows(m, c, r, p.s_compute, o);
    const double t_enq = tr.ms();
    double t_comp = 0;
    // (not while a PROG band is being followed: the drainer polls hipStreamQuery on the same stream, and a synchronise in flight here holds it up until the launch ends)
    if (tr.on && stitch.bands() == 0) { hipStreamSynchronize(p.s_compute); t_comp = tr.ms(); }
    std::string err = g_last_error;
    stitch.finish();
    if (tr.on) fprintf(stderr, "[w2xc host] device %d (cpu node %d%s) rows %d..%d: input queued %.3f ms, first output chunk enqueued %.3f ms, enqueued %.3f ms, layers done %.3f ms, stitched %.3f ms (in %s, out %s, %d copy threads)\n",
                       dev, node_guard.node, node_guard.bound ? ", threads bound" : "", ra, rb, input.t_done, t_first_out, t_enq, t_comp,
                       tr.ms(), in_pinned ? "pinned" : "pageable", out_pinned ? "pinned" : "pageable", copy_threads);
    // leave nothing in flight, whatever happened: the pipe and the caller's planes are reused by the next call
    hipError_t e1 = hipStreamSynchronize(p.s_h2d), e2 = hipStreamSynchronize(p.s_compute), e3 = hipStreamSynchronize(p.s_d2h);
    if (rc) { g_last_error = err; return rc; }
    if (stitch.rc()) return fail(stitch.rc(), "%s", stitch.error().c_str());
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
        return fail(W2XC_ERR_HIP, "stream synchronisation failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2 != hipSuccess ? e2 : e3));
    return W2XC_OK;
}

// fn(t) for every unit t < nd: on this thread when nd == 1, else one thread each.  No exception leaves a unit's thread (std::terminate) or crosses the C ABI;
// the caller's device is restored; the first failing unit's code is returned and its message is w2xc_last_error() (the C++ adapter prints it, a C-ABI
// consumer decides itself).  `what` names a unit in the messages.
int run_units(int nd, const char *what, const std::function<int(int)> &fn)
{
    int prev = 0;
    hipGetDevice(&prev);
    std::vector<int> rcs(nd, W2XC_OK);
    std::vector<std::string> errs(nd);
    auto worker = [&](int t) {
        try {
            rcs[t] = fn(t);
            if (rcs[t]) errs[t] = g_last_error;
        }
        catch (const std::bad_alloc &) { rcs[t] = W2XC_ERR_NOMEM; errs[t] = std::string("out of host memory in ") + what; }
        catch (const std::exception &ex) { rcs[t] = W2XC_ERR_HIP; errs[t] = std::string("exception in ") + what + ": " + ex.what(); }
        catch (...) { rcs[t] = W2XC_ERR_HIP; errs[t] = std::string("unknown exception in ") + what; }
    };
    if (nd == 1) worker(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nd; t++) th.emplace_back(worker, t);
        for (auto &x : th) x.join();
    }
    hipSetDevice(prev);
    for (int t = 0; t < nd; t++)
        if (rcs[t]) { g_last_error = errs[t]; return rcs[t]; }
    return W2XC_OK;
}

}  // namespace

// host-pointer path shared by w2xc_convert_plane (up = 0), w2xc_convert_plane_nn2x (up = 1) and w2xc_convert_plane_rows.
// (w, h) is the SOURCE plane; the output is (w << up) x (h << up), of which rows [row_begin, row_end) are produced.
int convert_plane_host(w2xc_model *m, const float *in, size_t in_stride_bytes, int w, int h, float *out,
                       size_t out_stride_bytes, const w2xc_opts *opts, int up, int row_begin = 0, int row_end = -1,
                       int in_row0 = 0, int in_rows = -1)
{
    if (!m || !in || !out) return fail(W2XC_ERR_ARG, "null argument");
    if (int rc = refuse_head(m, "w2xc_convert_plane[_nn2x / _rows]")) return rc;
    if (int rc = check_plane_size(w, h, false)) return rc;
    const int W = w << up, H = h << up;
    if (row_end < 0) row_end = H;
    if (row_begin < 0 || row_end > H || row_begin >= row_end) return fail(W2XC_ERR_ARG, "bad row range [%d,%d) for a %d-row plane", row_begin, row_end, H);
    if (int rc = check_row_strides(in_stride_bytes, w, out_stride_bytes, W)) return rc;
    if (m->layers.empty()) return fail(W2XC_ERR_ARG, "model has no layers");
    {   // the source rows handed over must cover the rows [row_begin - n, row_end + n) reads (clipped to the plane)
        const int n = (int)m->layers.size();
        const auto [need0, need1] = src_rows(row_begin, row_end, n, up, H);
        if (in_rows < 0) in_rows = h - in_row0;
        if (in_row0 < 0 || in_row0 > need0 || in_row0 + in_rows < need1 || in_row0 + in_rows > h)
            return fail(W2XC_ERR_ARG, "source rows [%d,%d) do not cover the rows [%d,%d) this row range reads", in_row0, in_row0 + in_rows, need0, need1);
    }
    w2xc_opts o = resolve_opts(opts);
    // halo rows of the units' source views: n, or 4 n when conv3x3_wino4 runs (its banding-invariant geometry, run_rows) -- if the rows handed
    // over hold that much around [row_begin, row_end); otherwise W2XC_KERNEL_AUTO means the F(2x2) kernels for this call
    int hs = (int)m->layers.size();
    if (resolve_chain(m, o).any_wino4) {
        const int h4 = 4 * hs;
        const auto [need0, need1] = src_rows(row_begin, row_end, h4, up, H);
        if (in_row0 <= need0 && in_row0 + in_rows >= need1) hs = h4;
        else if (o.kernel == W2XC_KERNEL_AUTO)   // (as run_rows: no silent change of kernel and rounding with the view's halo)
            return fail(W2XC_ERR_ARG, "source rows [%d,%d) hold the minimum halo only: the default F(4x4) kernel needs rows [%d,%d) (4 halo rows per layer) for "
                                      "banding-invariant results; pass them or choose w2xc_opts.kernel explicitly (W2XC_KERNEL_WINOGRAD32: F(2x2))",
                        in_row0, in_row0 + in_rows, need0, need1);
    }
    std::vector<int> devs;
    {
        int rc = host_devices(o, &devs);
        if (rc) return rc;
    }
    int nd = (int)devs.size();
    // w2xc_opts.host_units = k (test aid): cut the rows into k units, round-robin over the selected devices,
    // so the multi-device arithmetic below can be exercised on a single-GPU box
    {
        const int k = o.host_units;
        if (k > nd) {
            const size_t have = devs.size();
            for (int i = (int)have; i < k && i < 64; i++) devs.push_back(devs[i % have]);
            nd = (int)devs.size();
        }
    }
    const int R = row_end - row_begin;
    if (nd > R) nd = R;
    // In-place / overlapping planes with MORE THAN ONE unit: unit t writes output rows that are the halo source rows of units t-1 and
    // t+1 (each unit only protects its own rows, host_rows_on_device), on one device in a deterministic wrong order, on several
    // devices as a race.  The reference survives convertWithModels(img, img, ...) through its copyMakeBorder temporary
    // (convertRoutine.cpp:35,96); here the source rows are snapshotted once before the units fan out.
    std::vector<float> snapshot;
    if (nd > 1) {
        const auto [s0, s1] = src_rows(row_begin, row_end, hs, up, H);
        const char *in_lo = (const char *)in + (ptrdiff_t)(s0 - in_row0) * (ptrdiff_t)in_stride_bytes;
        const char *in_hi = (const char *)in + (ptrdiff_t)(s1 - 1 - in_row0) * (ptrdiff_t)in_stride_bytes + (size_t)w * 4;
        const char *out_lo = (const char *)out, *out_hi = (const char *)out + (size_t)(R - 1) * out_stride_bytes + (size_t)W * 4;
        if (ranges_overlap(in_lo, (size_t)(in_hi - in_lo), out_lo, (size_t)(out_hi - out_lo))) {
            snapshot.resize((size_t)(s1 - s0) * w);
            w2xc_host::CopyPool::get().copy_rows((char *)snapshot.data(), (size_t)w * 4, in_lo, in_stride_bytes, (size_t)w * 4, s1 - s0,
                                                 std::max(1, std::min(w2xc_get_jobs(), 32)));
            in = snapshot.data();
            in_stride_bytes = (size_t)w * 4;
            in_row0 = s0;
        }
    }
    // modelUtility's nJob (modelHandler.hpp:99; the CLI's -j) = host threads that move rows in and out of the staging rings, shared by the units
    const int copy_threads = std::max(1, std::min(w2xc_get_jobs(), 32) / nd);   // nJob bounds the total: never more than nJob staging threads over all units
    // the pool's workers are created HERE, on the caller's (unbound) thread: a unit's feeder binds itself to its device's NUMA node, and workers created
    // lazily from there would keep that node's mask while serving every device
    w2xc_host::CopyPool::get().reserve(std::min(w2xc_get_jobs(), 32) - 1);

    return run_units(nd, "a conversion unit", [&](int t) {
        const auto [ra, rb] = unit_rows(row_begin, row_end, t, nd);
        return host_rows_on_device(m, devs[t], in, in_stride_bytes, w, h, up, ra, rb, out, out_stride_bytes, o, copy_threads, in_row0, row_begin, hs);
    });
}

// ---- batches of same-size images from host memory (w2xc_convert_batch: float planes; w2xc_process_image_u8_batch: uint8 images) ----
// One device's share: the sub-batches `subs` ([first image, count), in order) of the call.  Device slots 0 / 1 of sub images each for the inputs and the outputs
// alternate between sub-batches, so that sub-batch j + 1's upload (s_h2d), sub-batch j's launches (s_compute: b.run) and sub-batch j - 1's download (s_d2h)
// overlap; this thread stages the next sub-batch's pageable images into a pinned slot and stitches the previous one's out of its pinned slot meanwhile.
// Page-locked images are DMA'd in place.  Kernels only ever see device memory: every output leaves by a D2H copy.
int batch_host_on_device(const HostBatch &b, int dev, const w2xc_opts &o, int copy_threads, const std::vector<std::pair<int, int>> &subs,
                         const std::vector<char> &in_pin, const std::vector<char> &out_pin)
{
    if (subs.empty()) return W2XC_OK;
    HIP_TRY(hipSetDevice(dev));
    NodeAffinity node_guard(dev, o.host_numa == 0);
    std::unique_lock<std::mutex> l1, l2;   // (as every entry point: calls that share a (model, device) serialise)
    HostPipe *pp = nullptr;
    int rc = b.acquire(dev, l1, l2, &pp);
    if (rc) return rc;
    HostPipe &p = *pp;
    if ((rc = pipe_init(p))) return rc;
    for (auto &e : p.ev_batch)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const size_t in_img = b.in_img, out_img = b.out_img;   // bytes per image in the device slots
    int sub = 0;
    bool any_in_pageable = false, any_out_pageable = false;
    for (const auto &sb : subs) {
        sub = std::max(sub, sb.second);
        for (int i = sb.first; i < sb.first + sb.second; i++) { any_in_pageable |= !in_pin[i]; any_out_pageable |= !out_pin[i]; }
    }
    rc = pipe_reserve(p, 2 * (size_t)sub * in_img, 2 * (size_t)sub * out_img, any_in_pageable ? (size_t)sub * in_img : 0,
                      any_out_pageable ? (size_t)sub * out_img : 0);
    if (rc) return rc;
    const size_t in_row = b.in_row, out_row = b.out_row;
    auto stitch = [&](int j) -> int {   // sub-batch j's pageable images out of its pinned slot, behind its download
        const int os = j % HostPipe::OUT_SLOTS;
        HIP_TRY(hipEventSynchronize(p.ev_out_slot[os]));
        const char *stage = p.pin_out.as<char>() + (size_t)os * p.out_slot_bytes();
        for (int k = 0; k < subs[j].second; k++) {
            const int i = subs[j].first + k;
            if (!out_pin[i])
                w2xc_host::CopyPool::get().copy_rows((char *)b.out[i], b.out_stride, stage + (size_t)k * out_img, out_row, out_row, b.out_rows, copy_threads);
        }
        return W2XC_OK;
    };
    // the sub-batches; whatever fails inside, nothing stays in flight (below)
    rc = [&]() -> int {
        for (int j = 0; j < (int)subs.size(); j++) {
            const int first = subs[j].first, cnt = subs[j].second, slot = j & 1;
            char *din = p.d_in.as<char>() + (size_t)slot * sub * in_img, *dout = p.d_out.as<char>() + (size_t)slot * sub * out_img;
            // ---- upload into device slot `slot` once the launches of sub-batch j - 2 have read it ----
            if (j >= 2) HIP_TRY(hipStreamWaitEvent(p.s_h2d, p.ev_batch[slot], 0));
            const int is = j % HostPipe::IN_SLOTS;
            char *stage = any_in_pageable ? p.pin_in.as<char>() + (size_t)is * p.in_slot_bytes() : nullptr;
            if (any_in_pageable && j >= HostPipe::IN_SLOTS) HIP_TRY(hipEventSynchronize(p.ev_in_slot[is]));   // its last DMA has read it
            for (int k = 0; k < cnt; k++) {
                const int i = first + k;
                if (in_pin[i]) {
                    HIP_TRY(hipMemcpy2DAsync(din + (size_t)k * in_img, in_row, b.in[i], b.in_stride, in_row, b.in_rows, hipMemcpyHostToDevice, p.s_h2d));
                } else {
                    char *st = stage + (size_t)k * in_img;
                    w2xc_host::CopyPool::get().copy_rows(st, in_row, (const char *)b.in[i], b.in_stride, in_row, b.in_rows, copy_threads);
                    HIP_TRY(hipMemcpyAsync(din + (size_t)k * in_img, st, in_row * b.in_rows, hipMemcpyHostToDevice, p.s_h2d));
                }
            }
            HIP_TRY(hipEventRecord(p.ev_in_slot[is], p.s_h2d));
            HIP_TRY(hipEventRecord(p.ev_input, p.s_h2d));
            // ---- the launches, behind the upload and behind the download of sub-batch j - 2 out of the same output slot ----
            HIP_TRY(hipStreamWaitEvent(p.s_compute, p.ev_input, 0));
            if (j >= 2) HIP_TRY(hipStreamWaitEvent(p.s_compute, p.ev_batch[2 + slot], 0));
            rc = b.run(dev, cnt, din, dout, p.s_compute, sub);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(p.ev_batch[slot], p.s_compute));
            // ---- download: page-locked images in place, the others into pinned slot j % OUT_SLOTS (stitched below, one sub-batch later) ----
            HIP_TRY(hipStreamWaitEvent(p.s_d2h, p.ev_batch[slot], 0));
            const int os = j % HostPipe::OUT_SLOTS;
            for (int k = 0; k < cnt; k++) {
                const int i = first + k;
                if (out_pin[i]) HIP_TRY(hipMemcpy2DAsync(b.out[i], b.out_stride, dout + (size_t)k * out_img, out_row, out_row, b.out_rows, hipMemcpyDeviceToHost, p.s_d2h));
                else HIP_TRY(hipMemcpyAsync(p.pin_out.as<char>() + (size_t)os * p.out_slot_bytes() + (size_t)k * out_img, dout + (size_t)k * out_img, out_row * b.out_rows,
                                            hipMemcpyDeviceToHost, p.s_d2h));
            }
            HIP_TRY(hipEventRecord(p.ev_out_slot[os], p.s_d2h));
            HIP_TRY(hipEventRecord(p.ev_batch[2 + slot], p.s_d2h));
            if (j >= 1 && any_out_pageable) { rc = stitch(j - 1); if (rc) return rc; }   // (the previous sub-batch, while this one computes)
        }
        if (any_out_pageable) { rc = stitch((int)subs.size() - 1); if (rc) return rc; }
        HIP_TRY(hipStreamSynchronize(p.s_compute));
        HIP_TRY(hipStreamSynchronize(p.s_d2h));
        return W2XC_OK;
    }();
    if (rc) {
        // A sub-batch failed with earlier ones still on the streams: uploads out of the caller's page-locked images and the pinned ring, launches on
        // the device slots, downloads into page-locked outputs.  The caller may free its images and the next call reuses slots and rings on return:
        // wait for all three streams, as host_rows_on_device does (the message is the failure's, not the wait's).
        const std::string err = g_last_error;
        for (hipStream_t s : {p.s_h2d, p.s_compute, p.s_d2h}) (void)hipStreamSynchronize(s);
        g_last_error = err;
    }
    return rc;
}

// the devices a host-pointer call runs on: those of w2xc_opts.device_mask that exist
int host_devices(const w2xc_opts &o, std::vector<int> *devs)
{
    const int ndev_all = w2xc_device_count();
    if (ndev_all <= 0) return fail(W2XC_ERR_HIP, "no HIP device available (libw2xc_hip has no CPU fallback)");
    for (int d = 0; d < ndev_all && d < 32; d++)
        if (o.device_mask == 0 || (o.device_mask >> d) & 1u) devs->push_back(d);
    if (devs->empty()) return fail(W2XC_ERR_ARG, "device_mask 0x%x selects no available device (%d present)", o.device_mask, ndev_all);
    return W2XC_OK;
}

// What the two host batch forms share behind their argument checks: the device list, sub-batches of at most `sub` images striped over the devices (at least
// two per device where there are images enough, so that uploads, launches and downloads have something to overlap with), which images are page-locked,
// one worker thread per device.
int batch_host_run(const HostBatch &b, const w2xc_opts &o, int sub)
{
    std::vector<int> devs;
    int rc = host_devices(o, &devs);
    if (rc) return rc;
    const int n = b.n;
    const auto share = batch_stripes(n, batch_stripe_sub(sub, n, (int)devs.size()), (int)devs.size());
    const int nd = (int)share.size();
    const size_t in_ext = (size_t)(b.in_rows - 1) * b.in_stride + b.in_row, out_ext = (size_t)(b.out_rows - 1) * b.out_stride + b.out_row;
    std::vector<char> in_pin(n), out_pin(n);
    for (int i = 0; i < n; i++) {
        in_pin[i] = host_range_pinned(b.in[i], in_ext);
        out_pin[i] = host_range_pinned(b.out[i], out_ext);
    }
    const int copy_threads = std::max(1, std::min(w2xc_get_jobs(), 32) / nd);
    w2xc_host::CopyPool::get().reserve(std::min(w2xc_get_jobs(), 32) - 1);
    return run_units(nd, "a batch unit", [&](int t) { return batch_host_on_device(b, devs[t], o, copy_threads, share[t], in_pin, out_pin); });
}

// byte ranges of n host images in / out ([ptr, ptr + ext)): no null pointer, no output that overlaps another output or an input
int check_batch_host_ptrs(int n, const void *const *in, size_t in_ext, void *const *out, size_t out_ext)
{
    std::vector<std::pair<std::pair<uintptr_t, uintptr_t>, int>> iv;
    iv.reserve(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        if (!in[i] || !out[i]) return fail(W2XC_ERR_ARG, "null plane pointer (plane %d)", i);
        iv.push_back({{(uintptr_t)in[i], (uintptr_t)in[i] + in_ext}, 0});
        iv.push_back({{(uintptr_t)out[i], (uintptr_t)out[i] + out_ext}, 1});
    }
    return check_batch_overlap(iv);
}

int convert_batch_host(w2xc_model *m, int n, int nn2x, const float *const *in, size_t in_stride, int w, int h, float *const *out, size_t out_stride,
                       const w2xc_opts *opts)
{
    int rc = check_batch_args(m, n, nn2x, w, h, in_stride, out_stride);
    if (rc) return rc;
    if (!in || !out) return fail(W2XC_ERR_ARG, "null argument");
    const int W = w << nn2x, H = h << nn2x;
    rc = check_batch_host_ptrs(n, (const void *const *)in, image_extent(h, in_stride, w, 4), (void *const *)out, image_extent(H, out_stride, W, 4));
    if (rc) return rc;
    rc = check_batch_model(m);
    if (rc) return rc;
    const w2xc_opts o = resolve_opts(opts);
    RowPlan P;   // (host arithmetic: the options' errors before any device is touched)
    rc = plan_rows(m, o, W, H, 0, 0, H, H, 1, false, &P);
    if (rc) return rc;
    // sub-batch size: the workspace budget's (as run_batch) and at most ~32 MiB of output planes (a pinned slot each)
    int sub = 1 << 20;
    if (batch_eligible(m, P)) {
        size_t img_f[2];
        batch_ws_floats(P, img_f);
        sub = batch_sub_size(P.o, img_f);
    }
    sub = std::min<long long>(sub, std::max<long long>(1, ((long long)32 << 20) / ((long long)W * H * 4)));
    HostBatch b;
    b.n = n;
    b.in = (const void *const *)in; b.out = (void *const *)out;
    b.in_stride = in_stride; b.out_stride = out_stride;
    b.in_row = (size_t)w * 4; b.out_row = (size_t)W * 4;
    b.in_rows = h; b.out_rows = H;
    b.in_img = (((size_t)w * h + 63) & ~(size_t)63) * 4; b.out_img = (((size_t)W * H + 63) & ~(size_t)63) * 4;
    b.acquire = [&](int dev, std::unique_lock<std::mutex> &l1, std::unique_lock<std::mutex> &, HostPipe **pipe) -> int {
        DevCtx *c = nullptr;
        int r = get_ctx(m, dev, &c);
        if (r) return r;
        l1 = std::unique_lock<std::mutex>(c->mu);
        *pipe = &c->pipe;
        return W2XC_OK;
    };
    b.run = [&](int dev, int cnt, const void *din, void *dout, hipStream_t st, int max_sub) -> int {
        DevCtx *c = nullptr;
        int r = get_ctx(m, dev, &c);
        if (r) return r;
        return run_batch(m, c, cnt, nn2x, {(const float *)din, (size_t)w, (long long)(b.in_img / 4)}, w, h, {(float *)dout, (size_t)W, (long long)(b.out_img / 4)},
                         st, o, max_sub);
    };
    return batch_host_run(b, o, sub);
}

}  // namespace w2xc_eng

using namespace w2xc_eng;

extern "C" {

int w2xc_convert_plane(w2xc_model *m, const float *in, size_t in_stride_bytes, int w, int h, float *out,
                       size_t out_stride_bytes, int block_splitting, const w2xc_opts *opts)
try {
    (void)block_splitting;   // results do not depend on the reference's block split
    return convert_plane_host(m, in, in_stride_bytes, w, h, out, out_stride_bytes, opts, 0);
} W2XC_CATCH_ALL

int w2xc_convert_plane_nn2x(w2xc_model *m, const float *in, size_t in_stride_bytes, int w, int h, float *out,
                            size_t out_stride_bytes, const w2xc_opts *opts)
try {
    return convert_plane_host(m, in, in_stride_bytes, w, h, out, out_stride_bytes, opts, 1);
} W2XC_CATCH_ALL

int w2xc_convert_plane_rows(w2xc_model *m, const float *in_view, size_t in_stride_bytes, int view_y0, int view_h, int w, int h, int nn2x,
                            int row_begin, int row_end, float *out, size_t out_stride_bytes, const w2xc_opts *opts)
try {
    if (nn2x != 0 && nn2x != 1) return fail(W2XC_ERR_ARG, "nn2x must be 0 or 1");
    if (view_h <= 0) return fail(W2XC_ERR_ARG, "empty source view");
    return convert_plane_host(m, in_view, in_stride_bytes, w, h, out, out_stride_bytes, opts, nn2x, row_begin, row_end, view_y0, view_h);
} W2XC_CATCH_ALL

int w2xc_convert_batch(w2xc_model *m, int n, int nn2x, const float *const *in, size_t in_stride_bytes, int w, int h, float *const *out,
                       size_t out_stride_bytes, const w2xc_opts *opts)
try {
    return convert_batch_host(m, n, nn2x, in, in_stride_bytes, w, h, out, out_stride_bytes, opts);
} W2XC_CATCH_ALL

}  // extern "C"
