// trsim_mem.hpp — the owner of every device and pinned allocation of libtrsim.so.  Host-only: never part of a kernel parameter block.
// Memory the library allocates is held by a DevBuf / PinnedBuf member or local and released by its destructor; raw pointers elsewhere are views.
// Nothing here waits for the GPU: whoever replaces or releases a buffer the device may still use waits first, at the call site.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace trsim {
template <class T, bool Pinned>                              // Pinned: hipHostMalloc / hipHostFree memory, else hipMalloc / hipFree
class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buf& operator=(Buf&& o) noexcept { if (this != &o) { (void)reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); } return *this; }
    ~Buf() { (void)reset(); }
    T* get() const { return p_; }
    T* operator->() const { return p_; }
    size_t bytes() const { return bytes_; }
    hipError_t reset() { const hipError_t rc = !p_ ? hipSuccess : Pinned ? hipHostFree(p_) : hipFree(p_); p_ = nullptr; bytes_ = 0; return rc; }
    hipError_t alloc(size_t bytes, unsigned flags = 0)       // releases what it holds, then allocates `bytes` (empty after a failure); flags: hipHostMalloc's
    {
        (void)reset();
        void* p = nullptr;
        const hipError_t rc = Pinned ? hipHostMalloc(&p, bytes, flags) : hipMalloc(&p, bytes);
        if (rc == hipSuccess) { p_ = static_cast<T*>(p); bytes_ = bytes; }
        return rc;
    }
    // the grow pattern: holds at least `bytes` afterwards; what it held is kept when that is enough and released otherwise
    hipError_t reserve(size_t bytes, unsigned flags = 0) { return bytes <= bytes_ ? hipSuccess : alloc(bytes, flags); }
private:
    T* p_ = nullptr; size_t bytes_ = 0;
};
template <class T = unsigned char> using DevBuf = Buf<T, false>;
template <class T = unsigned char> using PinnedBuf = Buf<T, true>;
}  // namespace trsim
