// uvs_hip_buf.h -- host-only owners of the HIP memory of the library's handles and the one way a failed HIP call becomes a handle's error
// text.  Included by every translation unit that owns a handle: the solver's units through uvs_solver_handle.h, the front-end units through uvs_handle.h (which adds
// what those handles share besides their buffers).  Nothing here runs on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>
#include <utility>

#include "../../include/uvs_solver.h"

// "<what>: <HIP's error string>" into `err` (the handle's error text); returns UVS_ERR_HIP
inline int hip_fail(std::string& err, hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return UVS_ERR_HIP;
}
// a HIP call that fails leaves the calling function with UVS_ERR_HIP, the call's text and HIP's error string in `err`
#define UVS_HIP(err, call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail((err), e_, #call); } while (0)

// growth rules of HipBuf::ensure: the bytes allocated when `need` does not fit
inline size_t grow_exact(size_t need) { return need; }
inline size_t grow_half(size_t need) { return need + need / 2; }              // the marginalization's sub-window blob and workspace
inline size_t grow_pinned(size_t need) { return need + need / 2 + 4096; }      // pinned staging: pinning costs milliseconds, never per call

// Move-only owner of one device (hipMalloc) or pinned host (hipHostMalloc) allocation, freed by the destructor.  Converts to T* so that
// it is passed to kernels and copies like the pointer it replaces.
template <class T, bool Pinned>
class HipBuf {
public:
    HipBuf() = default;
    HipBuf(HipBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    HipBuf& operator=(HipBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~HipBuf() { release(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }      // bytes
    // grow-only: when fewer than `need` bytes are held, the buffer is freed and grow(need) bytes are allocated (the contents are not kept)
    int ensure(size_t need, std::string& err, size_t (*grow)(size_t) = grow_exact) {
        if (cap_ >= need) return UVS_OK;
        release();
        void* p = nullptr;
        const size_t want = grow(need);
        const hipError_t e = Pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e != hipSuccess) return hip_fail(err, e, Pinned ? "hipHostMalloc" : "hipMalloc");
        p_ = static_cast<T*>(p); cap_ = want;
        return UVS_OK;
    }

private:
    void release() {
        if (p_) { if (Pinned) (void)hipHostFree(p_); else (void)hipFree(p_); }
        p_ = nullptr; cap_ = 0;
    }
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;
