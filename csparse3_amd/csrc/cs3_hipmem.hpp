// Device memory of the host layer (api.cpp, apps.cpp, substrate.hip's host functions): the one place that allocates and
// frees HBM, the error macro and the device check that go with it.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "cs3_internal.hpp"

namespace cs3 {

#define CS3_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            cs3::set_error(std::string(#call) + ": " + hipGetErrorString(e_));          \
            return CS3_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

inline bool device_visible()
{
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

// true (and the error text) when `who` cannot run: the caller returns CS3_ERR_HIP
inline bool no_device(const char *who)
{
    if (device_visible()) return false;
    set_error(std::string("no HIP device visible: ") + who + " runs on the GPU only");
    return true;
}

// blocks held through DevBuf right now, process-wide (cs3_debug_live_device_buffers)
inline std::atomic<long long> g_live_device_buffers{0};

// A device array of `count` T that frees itself.  Move-only.  An empty array still gets a block (8 bytes at least), so
// that get() is a valid address for a kernel argument.  Errors come back as hipError_t; nothing throws.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), count_(o.count_) { o.p_ = nullptr; o.count_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(count_, o.count_); }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    size_t count() const { return count_; }

    void reset()
    {
        if (p_) { (void) hipFree(p_); g_live_device_buffers -= 1; }
        p_ = nullptr; count_ = 0;
    }
    // A fresh block of `count` entries, contents undefined; what was held is freed first.  On failure the buffer is empty.
    hipError_t alloc(size_t count)
    {
        reset();
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count * sizeof(T), 8));
        if (e != hipSuccess) return e;
        g_live_device_buffers += 1;
        p_ = static_cast<T *>(p);
        count_ = count;
        return hipSuccess;
    }
    // Grow-only: keeps a block that is large enough.  (A caller that has to synchronise before the old block goes compares
    // count() itself, synchronises, and calls alloc.)
    hipError_t reserve(size_t count) { return count <= count_ && p_ ? hipSuccess : alloc(count); }
    hipError_t upload(const T *src, size_t count)
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess && count) e = hipMemcpy(p_, src, count * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t upload(const std::vector<T> &src) { return upload(src.data(), src.size()); }

private:
    T *p_ = nullptr;
    size_t count_ = 0;
};

}  // namespace cs3
