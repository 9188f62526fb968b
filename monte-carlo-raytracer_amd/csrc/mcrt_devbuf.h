// mcrt_devbuf.h -- DevBuf<T>: the one owner of a device allocation of the host runtime.
//
// A struct of DevBufs frees its memory when it is destroyed or assigned over, so a buffer is named
// once, where it is declared.  The type reaches the device through the three functions below only
// (mcrt_capi.cpp defines them over hipMalloc / hipFree / hipStreamSynchronize; tests/asan/host_asan.cpp
// over malloc / free), and this header needs no HIP header.
#pragma once
#include <cstddef>
#include <utility>

namespace mcrt {

// 0 on success, else the device runtime's error code; `stream` is the runtime's stream handle
int dev_alloc(void** p, size_t bytes);
void dev_free(void* p);
int dev_sync(void* stream);

template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        DevBuf t(std::move(o));
        swap(t);   // t frees what this held
        return *this;
    }
    ~DevBuf() { reset(); }
    void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); }

    T* get() const { return p_; }
    size_t size() const { return n_; }   // elements
    explicit operator bool() const { return p_ != nullptr; }

    void reset() {
        if (p_) dev_free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // `count` elements for an empty buffer
    int alloc(size_t count) {
        void* p = nullptr;
        const int e = dev_alloc(&p, sizeof(T) * count);
        if (e != 0) return e;
        p_ = static_cast<T*>(p);
        n_ = count;
        return 0;
    }
    // At least `count` elements, contents not kept: the old memory may still be in use on `stream`,
    // which is finished before it is freed.  On failure the buffer is empty.
    int grow(size_t count, void* stream) {
        if (n_ >= count) return 0;
        const int e = dev_sync(stream);
        if (e != 0) return e;
        reset();
        return alloc(count);
    }
    // takes over `count` elements a device builder allocated with the runtime's allocator
    void adopt(T* p, size_t count) {
        reset();
        p_ = p;
        n_ = count;
    }
};
template <class T>
void swap(DevBuf<T>& a, DevBuf<T>& b) noexcept { a.swap(b); }

}  // namespace mcrt
