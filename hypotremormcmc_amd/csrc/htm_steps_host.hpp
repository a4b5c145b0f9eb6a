// htm_steps_host.hpp -- the host idioms that the entry points of htm_steps.hip share, and the locate entry points (htm_locate.hip)
// with them.  Internal: the handles of htm_forward.hip and htm_chains_setup.hip keep their own pools (dev_alloc / dev_upload of htm_host.hpp).
// StreamBuf is the workspace of a *_dev form, DevPool the device arrays of a host-pointer form; Int<N>; kMaxWorkItems and env_mib
// come with htm_limits.hpp.
#pragma once
#include "htm_host.hpp"
#include "htm_limits.hpp"

#include <type_traits>

#pragma GCC visibility push(hidden)

namespace htm {

// a template argument chosen at run time: switch (r) { case 2: launch(Int<2>()); ... } with one generic lambda `launch`
template <int N>
using Int = std::integral_constant<int, N>;

// Workspace on a stream: one block, handed out in typed pieces.  alloc(st, carve) runs `carve`, a function of the buffer that
// take()s every array, twice: once to add the lengths up, once on the block (at least a byte; hipMallocAsync, or hipMalloc where
// the device has no memory pools) to set the pointers.  So each array's length is written once.  The pieces are consecutive in
// the order of the take() calls, each aligned to 16 bytes (double2).  release() after the last launch that uses the block:
// hipFreeAsync, or for a hipMalloc'ed block hipStreamSynchronize and hipFree.  A buffer that goes out of scope unreleased, on an
// early return, releases itself.
class StreamBuf {
public:
    StreamBuf() = default;
    StreamBuf(const StreamBuf &) = delete;
    StreamBuf &operator=(const StreamBuf &) = delete;
    ~StreamBuf() { (void)free_block(); }

    template <class T>
    void take(T *&piece, size_t n)
    {
        piece = p_ ? reinterpret_cast<T *>(p_ + used_) : nullptr;
        used_ += (n * sizeof(T) + 15) / 16 * 16;
    }
    template <class F>
    int alloc(hipStream_t st, F &&carve)
    {
        carve(*this);
        st_ = st;
        const size_t total = std::max<size_t>(used_, 1);
        async_ = hipMallocAsync(reinterpret_cast<void **>(&p_), total, st_) == hipSuccess;
        if (!async_) {
            (void)hipGetLastError();
            if (hipMalloc(reinterpret_cast<void **>(&p_), total) != hipSuccess) { p_ = nullptr; return fail(HTM_EHIP, "hipMalloc of %zu bytes failed", total); }
        }
        used_ = 0;
        carve(*this);
        return HTM_OK;
    }
    int release()
    {
        const char *call = async_ ? "hipFreeAsync" : "hipStreamSynchronize";
        const hipError_t e = free_block();
        return e == hipSuccess ? HTM_OK : fail(HTM_EHIP, "%s of a workspace failed: %s", call, hipGetErrorString(e));
    }
    void *data() const { return p_; }
    size_t bytes() const { return used_; }      // of the pieces and the padding between them

private:
    hipError_t free_block()
    {
        if (!p_) return hipSuccess;
        char *q = p_;
        p_ = nullptr;
        if (async_) return hipFreeAsync(q, st_);
        const hipError_t e = hipStreamSynchronize(st_);
        (void)hipFree(q);
        return e;
    }
    char *p_ = nullptr;
    bool async_ = false;
    hipStream_t st_ = nullptr;
    size_t used_ = 0;
};

// The device arrays of a host-pointer form.  Frees them when it goes out of scope, so every return is leak-free; it adds no
// synchronisation of its own (download is a blocking hipMemcpy on the null stream).
class DevPool {
public:
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() { for (void *p : pool_) (void)hipFree(p); }

    template <class T> int alloc(T **p, size_t n) { return dev_alloc(pool_, p, n); }
    template <class T> int upload(T **p, const T *src, size_t n) { return dev_upload(pool_, p, src, n); }
    template <class T>
    int download(T *host, const T *dev, size_t n, const char *what)
    {
        if (hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return fail(HTM_EHIP, "%s download failed", what);
        return HTM_OK;
    }

private:
    std::vector<void *> pool_;
};

}  // namespace htm

#pragma GCC visibility pop
