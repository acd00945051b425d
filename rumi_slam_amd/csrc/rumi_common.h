// Error plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "rumi_orb.h"

namespace rumi {
extern thread_local std::string g_lastError;
void set_error(const char *fmt, const char *a, const char *b, int line);

// The opt-in for more than 64 KiB of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize) is state of the FUNCTION, shared by every thread and
// stream of the process.  Handles on several host threads launch the same kernels with different sizes, so the limit only ever grows: a thread
// with a smaller problem must not lower it between another thread's request and launch.  One entry per (function, device).
inline hipError_t raise_lds_limit(const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> cur;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    size_t &c = cur[{fn, dev}];
    if (bytes <= c) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) c = bytes;
    return e;
}
}  // namespace rumi

// Any failing HIP call ends the C-ABI function with RUMI_E_NO_DEVICE and a message for rumi_last_error().
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            rumi::set_error("HIP error: %s -> %s (line %d)", #expr, hipGetErrorString(e_), __LINE__); \
            return RUMI_E_NO_DEVICE;                                                           \
        }                                                                                      \
    } while (0)

namespace rumi {
// The allocation helpers of the C-ABI translation units: a failure ends the caller through HIP_TRY's message and RUMI_E_NO_DEVICE.
// n elements of T (at least one) in device / pinned host memory; *p is null on failure
template <class T> int dev_alloc(T **p, size_t n) {
    *p = nullptr;
    HIP_TRY(hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return RUMI_OK;
}
template <class T> int pin_alloc(T **p, size_t n) {
    *p = nullptr;
    HIP_TRY(hipHostMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T), hipHostMallocDefault));
    return RUMI_OK;
}
// a block grown on demand: the old one is released, `bytes` of device or pinned host memory take its place (the contents are not kept)
template <class T> int regrow(T **p, size_t bytes, bool pinned) {
    if (*p) { if (pinned) (void)hipHostFree(*p); else (void)hipFree(*p); *p = nullptr; }
    if (pinned) HIP_TRY(hipHostMalloc((void **)p, bytes, hipHostMallocDefault));
    else HIP_TRY(hipMalloc((void **)p, bytes));
    return RUMI_OK;
}
}  // namespace rumi
