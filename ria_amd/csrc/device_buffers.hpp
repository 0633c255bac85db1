// ria_amd/csrc/device_buffers.hpp — owners of one hipMalloc / hipHostMalloc block.  A handle's memory is a set of these:
// it is freed by their destructors, and grown by reserve() in one way everywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace ria {

template <bool Pinned>
class HipBuf {
public:
    HipBuf() = default;
    HipBuf(const HipBuf&) = delete;
    HipBuf& operator=(const HipBuf&) = delete;
    ~HipBuf() { release(); }

    // A no-op when the block holds `bytes` already.  Otherwise: waits for *drain when one is given and there is a block
    // that work on that stream may still use, frees the block, records "empty", allocates.  A failed allocation leaves
    // a buffer that is empty and says so.  (A pointer, because the null stream is a stream too.)
    hipError_t reserve(size_t bytes, const hipStream_t* drain = nullptr) {
        if (bytes <= bytes_) return hipSuccess;
        if (p_ && drain) { hipError_t e = hipStreamSynchronize(*drain); if (e != hipSuccess) return e; }
        release();
        hipError_t e = Pinned ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        bytes_ = bytes;
        return hipSuccess;
    }
    void release() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; bytes_ = 0;
    }
    template <typename T = void>
    T* as() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};
using DevBuf = HipBuf<false>;
using PinBuf = HipBuf<true>;

// a host table on the device, allocated with 16 spare bytes behind the data
template <typename T>
hipError_t upload(DevBuf& dst, const std::vector<T>& v) {
    hipError_t e = dst.reserve(v.size() * sizeof(T) + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(dst.as<>(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace ria
