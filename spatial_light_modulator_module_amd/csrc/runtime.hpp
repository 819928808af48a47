// Error and device plumbing shared by the host translation units of
// libslm_hip.so (defined in slm_capi.hip): the thread-local error text behind
// slm_last_error, the process's current device, the try-macros, and the owning
// device buffer (DevBuf) of the trap lists and the any-size engine.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/slm_hip.h"

namespace slm {

// records the formatted text for slm_last_error and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// selects the device slm_init chose on the calling thread (device 0 if none was chosen yet)
int ensure_device();
// Blocking copies go through an explicit stream, never the legacy null stream:
// slm_gs_multi runs plans from several host threads, and a legacy-stream copy
// in one thread while another thread captures its plan's graph is an error.
int copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st);

template <typename T>
int dev_alloc(T** ptr, size_t bytes) {
    hipError_t e = hipMalloc((void**)ptr, bytes);
    if (e != hipSuccess) return fail(SLM_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return 0;
}

}  // namespace slm

#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return slm::fail(SLM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                             __LINE__);                                                                      \
    } while (0)

#define NCCL_TRY(expr)                                                                                            \
    do {                                                                                                          \
        ncclResult_t r_ = (expr);                                                                                 \
        if (r_ != ncclSuccess) return slm::fail(SLM_ERR_COMM, "%s failed: %s", #expr, ncclGetErrorString(r_));  \
    } while (0)

#define RC(x)                 \
    do {                      \
        int rc_ = (x);        \
        if (rc_) return rc_;  \
    } while (0)

namespace slm {

// an owning device buffer that only grows (non-copyable, freed with its owner)
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // bytes
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    // at least `bytes`; work on `st` may still read a live buffer, so the stream is waited for before
    // it is freed. The buffer is empty if the allocation fails.
    int need(size_t bytes, hipStream_t st) {
        if (bytes <= cap) return 0;
        if (p) {
            if (hipStreamSynchronize(st) != hipSuccess) return slm::fail(SLM_ERR_HIP, "hipStreamSynchronize failed");
            (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
        RC(slm::dev_alloc(&p, bytes));
        cap = bytes;
        return 0;
    }
};

}  // namespace slm
