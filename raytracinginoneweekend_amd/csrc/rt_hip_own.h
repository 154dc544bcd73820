// rt_hip_own.h — move-only owners of what the host side allocates through HIP: a device buffer, a
// pinned host buffer, an event, a stream. The destructor releases the handle and that is all they
// add: no reference counts, no allocator, no device bookkeeping. The owner of a record makes the
// right device current before it allocates through one or lets one go, as before.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>

#include "rt_host_build.h"
#include "rt_host_sync.h"

namespace rthost {

// The moves every owner shares: H is the handle, Free lets a non-null one go.
template <class H, hipError_t (*Free)(H)>
class Owned {
public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, H{})) {}
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            (void)release();
            h_ = std::exchange(o.h_, H{});
        }
        return *this;
    }
    ~Owned() { (void)release(); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != H{}; }
    hipError_t release() { return h_ ? Free(std::exchange(h_, H{})) : hipSuccess; }

protected:
    H h_{};
};

inline hipError_t free_device(void *p) { return hipFree(p); }
inline hipError_t free_pinned(void *p) { return hipHostFree(p); }

// A device buffer of T and the bytes it was asked for.
template <class T>
class DevBuf : public Owned<void *, free_device> {
public:
    T *get() const { return static_cast<T *>(h_); }
    size_t bytes() const { return h_ ? bytes_ : 0; }
    // A new allocation of exactly n bytes (what it held is freed first).
    hipError_t alloc(size_t n)
    {
        hipError_t e = release();
        if (e == hipSuccess) e = hipMalloc(&h_, n);
        bytes_ = n;
        return e;
    }
    // At least `want` bytes: nothing when it holds them, else the device goes idle, the buffer is
    // freed and max(want, 256) allocated; the size recorded is `want` (rt_scene_usage_get counts it).
    // *fresh (optional): set when the buffer was (re)allocated, whatever address it got back (the
    // allocator may return the freed one; ADVICE r5: callers key their resets on this, not on the address)
    int ensure(size_t want, bool *fresh = nullptr)
    {
        if (fresh) *fresh = false;
        if (bytes() >= want && h_) return RT_OK;
        if (fresh) *fresh = true;
        if (h_) {
            RT_HIP(hipDeviceSynchronize());
            RT_HIP(release());
        }
        RT_HIP(alloc(std::max<size_t>(want, 256)));
        bytes_ = want;
        return RT_OK;
    }

private:
    size_t bytes_ = 0;
};

// Pinned host memory of T; map() also asks for its device alias (hipHostMallocMapped).
template <class T>
class PinnedBuf : public Owned<void *, free_pinned> {
public:
    T *get() const { return static_cast<T *>(h_); }
    hipError_t alloc(size_t n, unsigned flags)
    {
        hipError_t e = release();
        if (e == hipSuccess) e = hipHostMalloc(&h_, n, flags);
        return e;
    }
    hipError_t map(T **dev) const { return hipHostGetDevicePointer(reinterpret_cast<void **>(dev), h_, 0); }
};

// An event; make() creates it on first use with the flags given there and does nothing after.
class Event : public Owned<hipEvent_t, hipEventDestroy> {
public:
    hipError_t make(unsigned flags = hipEventDisableTiming) { return h_ ? hipSuccess : hipEventCreateWithFlags(&h_, flags); }
};

class Stream : public Owned<hipStream_t, hipStreamDestroy> {
public:
    hipError_t make(unsigned flags = hipStreamNonBlocking) { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, flags); }
};

} // namespace rthost
