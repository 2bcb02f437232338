// hip_owner.h -- the error helpers of the host files and the four owners of what they create on the device: a device buffer and a pinned host buffer
// with their capacities, an event, a stream.  Each is move-only, releases what it holds when it goes, and converts to its raw handle, so launch sites
// and pointer arithmetic read as with a raw pointer.  A group that one "is it there" test stands for is built into locals and moved into its members
// once every creation has succeeded ("Ownership"): after any return it is complete or absent.
#pragma once
#include "../../include/xfr_amd.h"
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

namespace xfr {

inline thread_local std::string g_err;      // text of the calling thread's last error (xfr_last_error)

inline xfr_status fail(xfr_status st, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail(_e == hipErrorOutOfMemory ? XFR_OOM : XFR_HIP_ERROR, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(_e), __FILE__, __LINE__);                                       \
    } while (0)

#define XFR_TRY(expr)                         \
    do {                                      \
        const xfr_status _s = (expr);         \
        if (_s != XFR_OK) return _s;          \
    } while (0)

// `cap` elements of T on the device (T = char: bytes)
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    xfr_status alloc(size_t n) { reset(); HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T))); cap = n; return XFR_OK; }
    // at least `need` elements: nothing happens when there are, and growing frees the old buffer behind a device synchronisation
    xfr_status grow(size_t need)
    {
        if (cap >= need) return XFR_OK;
        if (p) HIP_TRY(hipDeviceSynchronize());
        return alloc(need);
    }
};

// `cap` elements of T in pinned host memory
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~PinnedBuf() { reset(); }
    operator T*() const { return p; }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    xfr_status alloc(size_t n) { reset(); HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), hipHostMallocDefault)); cap = n; return XFR_OK; }
};

struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); ev = o.ev; o.ev = nullptr; } return *this; }
    ~Event() { reset(); }
    operator hipEvent_t() const { return ev; }
    void reset() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    xfr_status create(bool timing = false) { reset(); HIP_TRY(hipEventCreateWithFlags(&ev, timing ? hipEventDefault : hipEventDisableTiming)); return XFR_OK; }
};

// a non-blocking stream
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s = o.s; o.s = nullptr; } return *this; }
    ~Stream() { reset(); }
    operator hipStream_t() const { return s; }
    void reset() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
    xfr_status create() { reset(); HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return XFR_OK; }
    xfr_status create(int priority) { reset(); HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority)); return XFR_OK; }
};

}  // namespace xfr
