// w2xc_launch.hpp -- what the launchers of the persistent, large-LDS kernels share (host side, included by the .hip files).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

// More than 64 KiB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize, and function attributes are per DEVICE (the in-process multi-GPU
// path launches one kernel on several devices from several threads).  One object per kernel -- a function-local static of its launcher -- remembers the
// devices done in a bit mask: no lock; a thread that finds its device's bit clear sets the attribute itself before it launches (two threads may both do
// so: harmless), so the attribute is always set before the first launch of that kernel on that device.  Devices 64 and up set it every time.
struct W2xcLdsOptIn {
    std::atomic<unsigned long long> done{0};

    template <typename KernelT>
    hipError_t operator()(KernelT kern, size_t lds_bytes)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev >= 64 || !((done.load() >> dev) & 1ull)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return e;
            if (dev < 64) done.fetch_or(1ull << dev);
        }
        return hipSuccess;
    }
};

// grid of a persistent kernel: per_cu workgroups on each of the 256 CUs, never more than the work items rounded up to a multiple of 8 (one share per XCD)
static inline int w2xc_persistent_grid(int items, int per_cu = 1)
{
    const int cap = per_cu * 256, need = (items + 7) & ~7;
    return cap < need ? cap : need;
}
