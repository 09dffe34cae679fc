// w2xc_scratch.hpp -- the ONE owner of the engine's grow-only buffers: the only place (beside the weights, uploaded once: upload / ~DevCtx) where
// memory is allocated or freed (tests/test_host_geom.py checks that).  A context lists its buffers once, DevCtx::for_each_scratch (w2xc_engine.hpp).
#pragma once
#include "../../include/w2xc_hip.h"
#include "w2xc_host_geom.hpp"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstring>

namespace w2xc_eng {

int fail(int code, const char *fmt, ...);

// The failure seam of w2xc_debug_fail_nth (test aid; state and slow path in w2xc_model.cpp): true = this event of `kind` (W2XC_DEBUG_FAIL_*) is the one
// armed to fail -- the caller then puts an error code where the runtime call would have been.  Until the entry point has been called once in the
// process this is one relaxed load of a word that is zero.
extern std::atomic<unsigned> g_fail_watch;   // bit k: events of kind k are counted
bool fail_event_watched(int kind);
inline bool fail_event(int kind) { return g_fail_watch.load(std::memory_order_relaxed) != 0 && fail_event_watched(kind); }

// what a buffer holds: DATA is filled by w2xc_debug_fill_scratch; SYNC words (job flags, job counters) never are -- a wrong value there could only make a
// launch wait for ever
enum class ScratchTag { DATA, SYNC };

class Scratch {
public:
    // the three flavours in use: device memory, page-locked host memory, and page-locked host memory that is uncached on the GPU side (every store goes
    // out over PCIe at once -- default host allocations may sit in the GPU's L2 until the launch ends: a system-scope flag then arrived long before the
    // rows it announces, measured)
    enum Kind { DEVICE, PINNED, PINNED_COHERENT };
    explicit Scratch(Kind kind = DEVICE) : kind_(kind) {}
    Scratch(Scratch &&o) noexcept : kind_(o.kind_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Scratch &operator=(Scratch &&) = delete;   // (move-only, and a buffer stays the member it is)
    ~Scratch() { release(); }

    template <class T> T *as() const { return static_cast<T *>(p_); }
    size_t bytes() const { return bytes_; }
    bool on_device() const { return kind_ == DEVICE; }

    // No-op when the buffer holds `bytes` already (the warm path: no HIP call).  Otherwise the old buffer goes and a new one comes; its content is undefined.
    // THE drain rule of every buffer: the whole device is waited for before an old buffer is freed -- an earlier launch on any stream, the caller's
    // included, may still use it (hipFree waits for the device anyway).  A wait that is not the device's (a host thread still reading a page-locked
    // buffer) is the caller's, before this.
    int reserve(size_t bytes, const char *what)
    {
        if (bytes_ >= bytes) return W2XC_OK;
        if (p_ && hipDeviceSynchronize() != hipSuccess) return fail(W2XC_ERR_HIP, "hipDeviceSynchronize failed before %s could grow", what);
        release();
        // (the seam stands where a real failure lands: behind the drain and the release, in place of the runtime call)
        const hipError_t e = fail_event(W2XC_DEBUG_FAIL_ALLOC) ? hipErrorOutOfMemory
                             : kind_ == DEVICE             ? hipMalloc(&p_, bytes)
                                                           : hipHostMalloc(&p_, bytes, kind_ == PINNED ? hipHostMallocDefault : hipHostMallocCoherent);
        if (e != hipSuccess) {
            p_ = nullptr;
            (void)hipGetLastError();
            return fail(W2XC_ERR_NOMEM, "allocating %zu MiB of %s memory for %s failed: %s", bytes >> 20, kind_ == DEVICE ? "device" : "page-locked host", what,
                        hipGetErrorString(e));
        }
        bytes_ = bytes;
        return W2XC_OK;
    }
    void release()
    {
        if (p_) (void)(kind_ == DEVICE ? hipFree(p_) : hipHostFree(p_));
        p_ = nullptr;
        bytes_ = 0;
    }

private:
    Kind kind_;
    void *p_ = nullptr;
    size_t bytes_ = 0;
};

// conv3x3_wino4 PROG: the job flags of one page-locked band buffer and the epoch a finished job stores into them live together.  Flags that grew are zero
// and their epoch is 0; released flags (`words` is in DevCtx::for_each_scratch) have no epoch either, whoever released them.
class ProgFlags {
public:
    Scratch words{Scratch::PINNED_COHERENT};
    unsigned epoch() const { return words.bytes() ? epoch_ : 0; }   // of the band handed out last
    int reserve(size_t n)
    {
        if (words.bytes() >= n * sizeof(unsigned)) return W2XC_OK;
        const int rc = words.reserve(n * sizeof(unsigned), "the job flags");
        if (!rc) restart();
        return rc;
    }
    // the next band's epoch; nothing may be in flight on these flags.  The test of a flag is signed (flag_reached), so after PROG_EPOCH_LAST they start over
    unsigned next_epoch() { if (epoch_ == PROG_EPOCH_LAST) restart(); return ++epoch_; }

private:
    void restart() { memset(words.as<unsigned>(), 0, words.bytes()); epoch_ = 0; }
    unsigned epoch_ = 0;
};

}  // namespace w2xc_eng
