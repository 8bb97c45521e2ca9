// holders.hpp -- owners of HIP memory, streams and events for the host library's drivers (pipeline.cpp, runbatch.cpp).
// Each holder is empty until it is allocated or created, frees what it holds when it is destroyed or re-allocated, and
// can be moved (into a std::vector) but not copied.
#ifndef ABUB3HS_HOLDERS_HPP
#define ABUB3HS_HOLDERS_HPP

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include <hip/hip_runtime_api.h>

#include "pipeline.hpp"

namespace abub {

// what a failed allocation throws: a std::runtime_error that a caller with a fall-back can catch by its type
struct AllocError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// HBM, or pinned host memory
template <bool Pinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    ~Buffer() { release(); }
    uint8_t *get() const { return p_; }
    size_t capacity() const { return cap_; }
    // at least `bytes`; when it has to grow it takes a quarter more, for the batches to come (the contents are not kept)
    void grow(size_t bytes)
    {
        if (bytes > cap_)
            allocate(bytes + bytes / 4 + 256);
    }
    // exactly `bytes`; the old storage is freed first (the caller makes sure no queued work still uses it)
    void allocate(size_t bytes)
    {
        release();
        void *q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
        if (e != hipSuccess)
            throw AllocError(std::string(Pinned ? "hipHostMalloc" : "hipMalloc") + " of " + std::to_string(bytes) +
                             " bytes: " + hipGetErrorString(e));
        p_ = (uint8_t *)q;
        cap_ = bytes;
    }

private:
    void release()
    {
        if (p_)
            (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    uint8_t *p_ = nullptr;
    size_t cap_ = 0;
};
using DeviceBuffer = Buffer<false>;
using PinnedBuffer = Buffer<true>;

// n elements of T, and 256 bytes of slack behind them that kernels may read into; used where a T * is
template <class T, bool Pinned>
class Array {
public:
    void allocate(size_t n) { b_.allocate(n * sizeof(T) + 256); }
    operator T *() const { return (T *)b_.get(); }

private:
    Buffer<Pinned> b_;
};
template <class T>
using DeviceArray = Array<T, false>;
template <class T>
using PinnedArray = Array<T, true>;

// a device array and its pinned host mirror; the copies take element counts and offsets
template <class T>
struct Mirror {
    DeviceArray<T> d;
    PinnedArray<T> h;
    void allocate(size_t n)
    {
        d.allocate(n);
        h.allocate(n);
    }
    void toDevice(size_t n, hipStream_t s, size_t first = 0) const
    {
        HIPOK(hipMemcpyAsync(d + first, h + first, n * sizeof(T), hipMemcpyHostToDevice, s));
    }
    void toHost(size_t n, hipStream_t s, size_t first = 0) const
    {
        HIPOK(hipMemcpyAsync(h + first, d + first, n * sizeof(T), hipMemcpyDeviceToHost, s));
    }
};

// The part of a GrowList that does not depend on its element type: its capacity in entries and how it grows.  The contents
// are not kept and the old storage is freed first, so a list grows only once the streams that used it have been synchronised
class Growable {
public:
    size_t cap() const { return cap_; } // (0 while the list is being grown, and after a failed allocation)
    void seed(size_t n) // exactly n entries
    {
        cap_ = 0;
        allocateEntries(n);
        cap_ = n;
    }
    // at least n entries; when it has to grow it takes a quarter more and its slack, for the batches to come
    void reserve(size_t n)
    {
        if (n > cap_)
            seed(n + n / 4 + slack_);
    }
    // The redo rule of a batch whose kernels count past the capacity: true if `needed` entries fit; else the list grows and
    // the caller redoes the batch -- once: a list that overflows again in the same batch, or past its limit, throws
    bool fit(size_t needed, const char *message)
    {
        if (needed <= cap_)
            return true;
        if (grown_ || needed > limit_)
            throw std::runtime_error(message);
        reserve(needed);
        grown_ = true;
        return false;
    }
    void newBatch() { grown_ = false; }

protected:
    Growable(size_t slack, size_t limit) : slack_(slack), limit_(limit) {}

private:
    virtual void allocateEntries(size_t n) = 0;
    size_t cap_ = 0, slack_, limit_;
    bool grown_ = false;
};

// A Mirror that knows its capacity in entries of `per` elements each (the boxes of the localize knob: 4)
template <class T>
struct GrowList final : Mirror<T>, Growable {
    explicit GrowList(size_t slack, size_t per = 1, size_t limit = SIZE_MAX) : Growable(slack, limit), per_(per) {}

private:
    void allocateEntries(size_t n) override { Mirror<T>::allocate(per_ * n); }
    size_t per_;
};

// A non-blocking stream of the current device; its work is finished before it goes
class Stream {
public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    ~Stream() { reset(); }
    // made now, with a priority (numerically lower = higher, see hipDeviceGetStreamPriorityRange)
    void create(int priority)
    {
        reset();
        HIPOK(hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, priority));
    }
    // made on first use otherwise
    hipStream_t get()
    {
        if (!s_)
            HIPOK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
        return s_;
    }

private:
    void reset()
    {
        if (s_) {
            (void)hipStreamSynchronize(s_);
            (void)hipStreamDestroy(s_);
        }
        s_ = nullptr;
    }
    hipStream_t s_ = nullptr;
};

// An event of the current device; timing = false makes it with hipEventDisableTiming
class Event {
public:
    Event() = default;
    Event(Event &&o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    ~Event() { reset(); }
    void create(bool timing)
    {
        reset();
        HIPOK(hipEventCreateWithFlags(&ev_, timing ? hipEventDefault : hipEventDisableTiming));
    }
    hipEvent_t get() const { return ev_; }
    // ms between `start` and this one, both recorded with timing and both reached
    float msSince(const Event &start) const
    {
        float ms = 0;
        HIPOK(hipEventElapsedTime(&ms, start.ev_, ev_));
        return ms;
    }

private:
    void reset()
    {
        if (ev_)
            (void)hipEventDestroy(ev_);
        ev_ = nullptr;
    }
    hipEvent_t ev_ = nullptr;
};

} // namespace abub
#endif
