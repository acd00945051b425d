// Error and host plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
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

// ---- host plumbing of the handles ("Host plumbing"): a new entry point uses these instead of writing its own ----

// "Is there a device": the one check and the one message of a library without a CPU path.  *count: how many there are.
inline int require_device(int *count = nullptr) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_lastError = "no HIP device visible: librumi_hip has no CPU fallback";
        return RUMI_E_NO_DEVICE;
    }
    if (count) *count = ndev;
    return RUMI_OK;
}

// The parts of an upload or result block start 16-byte aligned.
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// A device block grown on demand.  reserve(need, want): nothing when `need` elements fit, else the old block is released (its contents are not
// kept) and `want` elements take its place.  After a failed allocation p is null and cap is 0, so the next call allocates again and nothing
// writes through a stale block.  An empty buffer makes no HIP call, in release() or in the destructor.
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;                 // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    int reserve(size_t need, size_t want) {
        if (need <= cap) return RUMI_OK;
        release();
        const int rc = dev_alloc(&p, want);
        if (rc == RUMI_OK) cap = want;
        return rc;
    }
};

// A pinned host block and its device twin behind one capacity, with DevBuf's rules: after a failure of either half both are null and cap is 0.
template <class T> struct MirrorBuf {
    T *h = nullptr, *d = nullptr;
    size_t cap = 0;                 // elements
    MirrorBuf() = default;
    MirrorBuf(const MirrorBuf &) = delete;
    MirrorBuf &operator=(const MirrorBuf &) = delete;
    ~MirrorBuf() { release(); }
    void release() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        h = d = nullptr; cap = 0;
    }
    int reserve(size_t need, size_t want) {
        if (need <= cap) return RUMI_OK;
        release();
        int rc = pin_alloc(&h, want);
        if (rc == RUMI_OK) rc = dev_alloc(&d, want);
        if (rc == RUMI_OK) cap = want; else release();
        return rc;
    }
};

// A mapped, coherent pinned block that kernels read and write in place (a stop word, published scalars), with the address the device uses for
// it.  MirrorBuf's rules; a new block comes back zeroed.
template <class T> struct MappedBuf {
    T *h = nullptr, *d = nullptr;   // one memory, as the host and as the device see it
    size_t cap = 0;                 // elements
    MappedBuf() = default;
    MappedBuf(const MappedBuf &) = delete;
    MappedBuf &operator=(const MappedBuf &) = delete;
    ~MappedBuf() { release(); }
    void release() { if (h) (void)hipHostFree((void *)h); h = d = nullptr; cap = 0; }
    int reserve(size_t need, size_t want) {
        if (need <= cap) return RUMI_OK;
        release();
        hipError_t e = hipHostMalloc((void **)&h, std::max<size_t>(want, 1) * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) h = nullptr;
        else e = hipHostGetDevicePointer((void **)&d, (void *)h, 0);
        if (e != hipSuccess) { release(); HIP_TRY(e); }
        std::memset((void *)h, 0, std::max<size_t>(want, 1) * sizeof(T));
        cap = want;
        return RUMI_OK;
    }
};

// A stream (non-blocking) and an event that are destroyed with their owner; empty until create(), which does nothing the second time.
struct StreamHold {
    hipStream_t s = nullptr;
    StreamHold() = default;
    StreamHold(const StreamHold &) = delete;
    StreamHold &operator=(const StreamHold &) = delete;
    ~StreamHold() { if (s) (void)hipStreamDestroy(s); }
    int create() { if (!s) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return RUMI_OK; }
    operator hipStream_t() const { return s; }
};
struct EventHold {
    hipEvent_t e = nullptr;
    EventHold() = default;
    EventHold(const EventHold &) = delete;
    EventHold &operator=(const EventHold &) = delete;
    ~EventHold() { if (e) (void)hipEventDestroy(e); }
    int create() { if (!e) HIP_TRY(hipEventCreate(&e)); return RUMI_OK; }
    operator hipEvent_t() const { return e; }
};

// What a set of owning buffers holds right now, in bytes: device memory and pinned host memory.
struct Footprint {
    int64_t dev = 0, pin = 0;
    template <class T> void one(const DevBuf<T> &b) { dev += (int64_t)(b.cap * sizeof(T)); }
    template <class T> void one(const MirrorBuf<T> &b) { dev += (int64_t)(b.cap * sizeof(T)); pin += (int64_t)(b.cap * sizeof(T)); }
    template <class T> void one(const MappedBuf<T> &b) { pin += (int64_t)(b.cap * sizeof(T)); }
    template <class... B> void add(const B &...b) { (one(b), ...); }
};

// The device of a handle that binds at its first call past validation, so that creating one, its argument checks and its destruction run on a
// machine without a GPU: an unbound handle has made no HIP call.  bind(): require_device, the current device when none was named, hipSetDevice;
// on later calls hipSetDevice only.  With `first` the caller has allocations of its own to make when *first comes back true, and sets `bound`
// itself once they are in place.  A destroy function makes the device current before its `delete` only when `bound`.
struct DeviceBinding {
    int device = -1;
    bool bound = false;
    int bind(bool *first = nullptr) {
        if (first) *first = !bound;
        if (!bound) {
            const int rc = require_device();
            if (rc != RUMI_OK) return rc;
            if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
        }
        HIP_TRY(hipSetDevice(device));
        if (!first) bound = true;
        return RUMI_OK;
    }
};

// The wall clock of a call in three stages: start(), a mark() at each of the two boundaries, finish() at the end writes the three differences
// in milliseconds.  A third mark() moves the second boundary (the local-map query of covis.hip reads in two steps).
struct StageClock {
    std::chrono::steady_clock::time_point t[3];
    int n = 0;
    void start() { t[0] = std::chrono::steady_clock::now(); n = 1; }
    void mark() { t[n < 3 ? n++ : 2] = std::chrono::steady_clock::now(); }
    void finish(float ms[3]) const {
        const auto end = std::chrono::steady_clock::now();
        ms[0] = std::chrono::duration<float, std::milli>(t[1] - t[0]).count();
        ms[1] = std::chrono::duration<float, std::milli>(t[2] - t[1]).count();
        ms[2] = std::chrono::duration<float, std::milli>(end - t[2]).count();
    }
};

// The observation table of the twin entries of rumi_mapping.h (rumi_keyframe_culling, rumi_refresh_map_points): every (obs_kf, obs_feature)
// pair inside the key-frame table (nOf(k): the feature count of key-frame k), then every point's slice inside 0..n_obs, followed at once by the
// entry's own check of that point (each(p): RUMI_OK, or its code with the message set).  *tooMany: a slice longer than maxObs.
template <class Point, class FeatCount, class EachPoint>
int check_observation_table(const char *entry, int n_kf, FeatCount nOf, const Point *pts, int n_pts, const int32_t *obs_kf, const int32_t *obs_feature,
                            int n_obs, int maxObs, bool *tooMany, EachPoint each) {
    for (int o = 0; o < n_obs; o++)
        if (obs_kf[o] < 0 || obs_kf[o] >= n_kf || obs_feature[o] < 0 || obs_feature[o] >= nOf(obs_kf[o])) {
            g_lastError = std::string(entry) + ": an observation names a key-frame outside the table or a feature outside its key-frame";
            return RUMI_E_INVALID;
        }
    *tooMany = false;
    for (int p = 0; p < n_pts; p++) {
        const Point &P = pts[p];
        if (P.obs_begin < 0 || P.obs_end < P.obs_begin || P.obs_end > n_obs) {
            g_lastError = std::string(entry) + ": a point's observation slice lies outside 0..n_obs";
            return RUMI_E_INVALID;
        }
        const int rc = each(p);
        if (rc != RUMI_OK) return rc;
        *tooMany = *tooMany || P.obs_end - P.obs_begin > maxObs;
    }
    return RUMI_OK;
}
}  // namespace rumi
