// Move-only owners of what a context allocates: device and page-locked buffers, events, the copy stream.  Each frees
// its resource in its destructor, so lr_context needs no list of them; a buffer converts to T* so that launches,
// copies and pointer arithmetic read as they would with a plain pointer.
#pragma once
#include <algorithm>
#include <utility>

#include "common.h"

namespace lramd {

// the LR_HIP report for a call whose status was kept in a variable
inline int hip_failed(const char* call, hipError_t e) {
    (void)hipGetLastError();
    set_error(std::string(call) + ": " + hipGetErrorString(e));
    return 1;
}

template <class T, bool Pinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~Buffer() { reset(); }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    // frees what it holds, then allocates `count` elements (at least one): the old block is gone even if this fails
    hipError_t alloc(size_t count) {
        reset();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p_, bytes) : hipMalloc((void**)&p_, bytes);
        if (e == hipSuccess) cap_ = count;
        else p_ = nullptr;
        return e;
    }
    int grow(size_t count) {  // ... reporting a failure like LR_HIP
        const hipError_t e = alloc(count);
        return e == hipSuccess ? 0 : hip_failed(Pinned ? "hipHostMalloc" : "hipMalloc", e);
    }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }  // elements asked for by the last successful alloc / grow

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <class T>
using DeviceBuffer = Buffer<T, false>;
template <class T>
using PinnedBuffer = Buffer<T, true>;

// a device buffer and its page-locked mirror, grown together
template <class T>
struct MirroredBuffer {
    DeviceBuffer<T> d;
    PinnedBuffer<T> h;
    int grow(size_t count) { return d.grow(count) || h.grow(count); }
    size_t cap() const { return h.cap(); }  // (0 unless both were made)
};

class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        std::swap(e_, o.e_);
        return *this;
    }
    ~Event() {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e_, flags); }
    int ensure(unsigned flags) {  // made on first use
        if (e_) return 0;
        const hipError_t e = create(flags);
        return e == hipSuccess ? 0 : hip_failed("hipEventCreateWithFlags", e);
    }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

class Stream {
public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s_) (void)hipStreamDestroy(s_);
    }
    hipStream_t* put() { return &s_; }  // for hipStreamCreate*
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

}  // namespace lramd
