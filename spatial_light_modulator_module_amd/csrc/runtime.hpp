// Error and device plumbing shared by the host translation units of
// libslm_hip.so (defined in slm_capi.hip): the thread-local error text behind
// slm_last_error, the process's current device, the try-macros, the owning
// device buffer (DevBuf) of the trap lists and the any-size engine, and the few
// host helpers the handles share: the grid of an element-wise kernel, the a_in
// check and the event-pair stopwatch of the timed runs.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

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

// blocks of 256 threads that stride over n elements
inline int grid_for(long long n) { return (int)std::min<long long>(8192, (n + 255) / 256); }

// a_in [n], or nullptr = ones: no non-finite entry, not zero everywhere; *sum_a2 (if asked for) = sum a^2
inline int check_ain(const float* ain, size_t n, double* sum_a2) {
    double sum = ain ? 0.0 : (double)n;
    for (size_t i = 0; ain && i < n; ++i) {
        if (!std::isfinite(ain[i])) return fail(SLM_ERR_ARG, "a_in has a non-finite entry");
        sum += (double)ain[i] * (double)ain[i];
    }
    if (!(sum > 0.0)) return fail(SLM_ERR_ARG, "a_in is zero everywhere");
    if (sum_a2) *sum_a2 = sum;
    return 0;
}

// begin / end event pairs around the kernels of each class of a timed run (events are kept and used
// again). Not EventPool (plan.hpp), whose pairs the dispatch packets of the fused engine stamp.
struct Stopwatch {
    std::vector<hipEvent_t> ev;
    std::vector<int> cls;  // pair k is ev[2 k], ev[2 k + 1], of class cls[k]
    size_t used = 0;
    bool timed = false;
    Stopwatch() = default;
    Stopwatch(const Stopwatch&) = delete;
    Stopwatch& operator=(const Stopwatch&) = delete;
    ~Stopwatch() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void reset(bool on) {
        timed = on;
        used = 0;
        cls.clear();
    }
    int mark(hipStream_t st) {
        if (used == ev.size()) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
        HIP_TRY(hipEventRecord(ev[used++], st));
        return 0;
    }
    int begin(int c, hipStream_t st) {
        if (!timed) return 0;
        cls.push_back(c);
        return mark(st);
    }
    int end(hipStream_t st) { return timed ? mark(st) : 0; }
    // after the stream has been waited for: the microseconds of each of `classes` classes
    int read(double* us_per_class, int classes) const {
        for (int c = 0; c < classes; ++c) us_per_class[c] = 0.0;
        for (size_t k = 0; k < cls.size(); ++k) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
            us_per_class[cls[k]] += 1e3 * ms;
        }
        return 0;
    }
};

}  // namespace slm
