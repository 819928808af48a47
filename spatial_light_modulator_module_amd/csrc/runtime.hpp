// Error and device plumbing shared by the host translation units of
// libslm_hip.so (defined in slm_capi.hip): the thread-local error text behind
// slm_last_error, the process's current device, and the try-macros.
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
