// libslm_hip.so C boundary (include/slm_hip.h): argument checks, the plan's
// shared buffers, graph capture and replay of a run, HIP-event timing, reads,
// image sequences (slm_plan_sequence: frames landed and run as one chain at the
// Engine interface, their epilogue kernels in frames.hip), and the one-shot
// helpers. The iterations themselves run in an engine
// (plan.hpp: fused.hip or generic.hip); the gathers are in comm.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "generic.hpp"
#include "kernels.hpp"
#include "plan.hpp"
#include "seq_frames.hpp"

using namespace slm;

namespace {
thread_local std::string g_err;
int g_device = -1;
// per-shard timing of the last slm_gs_multi of this process (slm_gs_multi_timing)
std::mutex g_multi_mu;
std::vector<double> g_multi_wall, g_multi_run;
}  // namespace

namespace slm {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    if (!bytes) return 0;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int ensure_device() {
    if (g_device >= 0) {
        HIP_TRY(hipSetDevice(g_device));
        return 0;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(SLM_ERR_HIP, "no HIP device available (%s); libslm_hip has no CPU path",
                    hipGetErrorString(e));
    g_device = 0;
    HIP_TRY(hipSetDevice(0));
    return 0;
}

// what an engine without the feature answers
int Engine::fft2_z(PlanState&, const double2*, double2*, int) {
    return fail(SLM_ERR_STATE, "fft2_c128 runs on the any-size engine");
}
int Engine::generic_info(int*) const {
    return fail(SLM_ERR_STATE, "not an any-size plan (fused float32 engine: see slm_plan_info)");
}
int Engine::land_weights(PlanState&, const float*, bool*) {
    return fail(SLM_ERR_STATE, "weights belong to weighted-GS plans of the fused engine");
}
int Engine::read_weights(PlanState&, bool, float*) {
    return fail(SLM_ERR_STATE, "weights belong to weighted-GS plans of the fused engine");
}
int Engine::land_region(PlanState&, const uint8_t*) {
    return fail(SLM_ERR_STATE, "a signal region belongs to MRAF plans of the fused engine");
}
int Engine::land_region_dev(PlanState&, const uint8_t*) {
    return fail(SLM_ERR_STATE, "a signal region belongs to MRAF plans of the fused engine");
}
int Engine::mraf_refresh(PlanState&, bool, int*) {
    return fail(SLM_ERR_STATE, "a signal region belongs to MRAF plans of the fused engine");
}
int Engine::read_trace(PlanState&, int, unsigned long long*) {
    return fail(SLM_ERR_STATE, "no trace buffer (set SLM_TRACE_BUF=1 before creating the plan)");
}

// the resident zoom's door to the frames of the last sequence (seq_frames.hpp)
SeqFrames plan_seq_frames(const slm_plan* p) {
    SeqFrames q;
    q.stream = p->s.stream;
    q.n = p->seq.n_frames * p->s.B;
    q.H = p->s.H;
    q.W = p->s.W;
    if (p->seq.n_frames && p->seq.has_frames) q.frames = p->seq.frames.p;
    return q;
}

}  // namespace slm

int engine_of(slm_plan* p, Engine** e) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    if (!p->eng) return fail(SLM_ERR_STATE, "the plan lost its engine (failed slm_plan_set_precision)");
    *e = p->eng;
    return 0;
}

namespace {

// Holds a stream for `ticks` of the 100 MHz s_memrealtime clock (one wave,
// bounded by time alone). slm_plan_run_timed queues it first so the host
// enqueues every launch of the timed run while it waits: the timed kernels then
// run back to back, as in the replayed graph of slm_plan_run, instead of each
// starting on an idle device behind the host's per-launch enqueue cost (which
// measured up to 0.5 us shorter per 1024^2 launch than the same kernel in the
// graph, profiles/r04).
__global__ void __launch_bounds__(64) hold_kernel(unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

// Streaming copy, 16 B per lane, four non-temporal loads in flight per lane
// before their stores, grid-stride (slm_copy_bandwidth): the practical HBM /
// Infinity-Cache rate the roofline fractions are read against.
typedef float v4f __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) copy_f4_kernel(const v4f* __restrict__ in, v4f* __restrict__ out,
                                                      long long n) {
    const long long stride = (long long)gridDim.x * 1024;
    for (long long base = blockIdx.x * 1024LL + threadIdx.x; base < n; base += stride) {
        v4f r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (base + k * 256 < n) r[k] = __builtin_nontemporal_load(in + base + k * 256);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (base + k * 256 < n) __builtin_nontemporal_store(r[k], out + base + k * 256);
    }
}

// max(T) and sum(T^2) per hologram in double (np.amax(demanded_output),
// src/algorithms.py:23; sum(T^2) is the constant term of the error expansion).
// Stage 1: ts_blocks(holo) workgroups per hologram, each thread reducing
// kTsPerThread consecutive elements from 16-B vector loads (64 MB of a 4096^2
// float32 target stream at HBM rate: 4096 workgroups, not 64); stage 2 folds
// a hologram's partials in a fixed order (deterministic).
constexpr int kTsPerThread = 16;
constexpr int kTsThreads = 256;
inline int ts_blocks(long long holo) {
    return (int)std::max<long long>(1, holo / ((long long)kTsThreads * kTsPerThread));
}
template <typename TT>
__global__ void __launch_bounds__(kTsThreads) target_stats_partial_kernel(const TT* tgt, long long holo, double* part) {
    const int b = blockIdx.y;
    const int nblk = gridDim.x;
    const long long chunk = (holo + nblk - 1) / nblk;
    const long long lo = (long long)blockIdx.x * chunk, hi = min(holo, lo + chunk);
    const TT* p = tgt + (long long)b * holo;
    double mx = 0.0, s2 = 0.0, d = 0.0;
    constexpr int VEC = 16 / sizeof(TT);  // elements per 16-B load
    const long long vlo = lo / VEC, vhi = hi / VEC;  // holo and chunk are multiples of VEC for supported shapes
    if ((lo % VEC) == 0 && (hi % VEC) == 0) {
        for (long long i = vlo + threadIdx.x; i < vhi; i += kTsThreads) {
            const uint4 q = reinterpret_cast<const uint4*>(p)[i];
            const TT* e = reinterpret_cast<const TT*>(&q);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const double v = (double)e[k];
                mx = fmax(mx, v);
                s2 += v * v;
            }
        }
    } else {
        for (long long i = lo + threadIdx.x; i < hi; i += kTsThreads) {
            const double v = (double)p[i];
            mx = fmax(mx, v);
            s2 += v * v;
        }
    }
    block_reduce_stats<kTsThreads>(mx, s2, d);
    if (threadIdx.x == 0) {
        double* o = part + ((long long)b * nblk + blockIdx.x) * 2;
        o[0] = mx;
        o[1] = s2;
    }
}
__global__ void __launch_bounds__(kTsThreads) target_stats_final_kernel(const double* part, int nblk, double* norm,
                                                                        float* normf, double* sum_t2) {
    const int b = blockIdx.x;
    double mx = 0.0, s2 = 0.0, d = 0.0;
    for (int k = threadIdx.x; k < nblk; k += kTsThreads) {
        mx = fmax(mx, part[((long long)b * nblk + k) * 2]);
        s2 += part[((long long)b * nblk + k) * 2 + 1];
    }
    block_reduce_stats<kTsThreads>(mx, s2, d);
    if (threadIdx.x == 0) {
        norm[b] = mx;
        normf[b] = (float)mx;
        sum_t2[b] = s2;
    }
}
template <typename TT>
void target_stats_partial(slm_plan* p, const void* tgt) {
    hipLaunchKernelGGL(target_stats_partial_kernel<TT>, dim3(ts_blocks(p->s.holo), p->s.B), dim3(kTsThreads), 0,
                       p->s.stream, (const TT*)tgt, p->s.holo, p->ts_part);
}

// The captured run bakes in kernels, tables and buffers: dropped before any of
// them changes. Runs are asynchronous, so a replay may still be queued.
int drop_graph(slm_plan* p) {
    if (!p->gexec) return 0;
    HIP_TRY(hipStreamSynchronize(p->s.stream));
    HIP_TRY(hipGraphExecDestroy(p->gexec));
    p->gexec = nullptr;
    return 0;
}

int mraf_no_support(int b) {
    return fail(SLM_ERR_ARG, "the signal region of hologram %d holds no pixel with T > 0", b);
}

// MRAF runs need a region in force, with target light inside it (a replayed run is checked too)
int mraf_ready(const slm_plan* p) {
    if (p->s.algo != SLM_ALGO_MRAF) return 0;
    if (!p->region_set) return fail(SLM_ERR_STATE, "signal region not set (slm_plan_set_region)");
    if (p->target_set && p->mraf_bad >= 0) return mraf_no_support(p->mraf_bad);
    return 0;
}

// MRAF: the region constants follow every change of target, region, a_in or m
// (reduce = false: m alone changed)
int mraf_update(slm_plan* p, bool reduce) {
    if (p->s.algo != SLM_ALGO_MRAF || !p->target_set || !p->region_set) return 0;
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    int bad = -1;
    RC(e->mraf_refresh(p->s, reduce, &bad));
    if (reduce) p->mraf_bad = bad;
    return 0;
}

int enqueue_run(slm_plan* p, int loops, double tol, int checked, float wa) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    if (!p->target_set) return fail(SLM_ERR_STATE, "target not set");
    if (loops < 1 || loops > p->s.max_loops)
        return fail(SLM_ERR_ARG, "loops %d outside [1, %d]", loops, p->s.max_loops);
    if (p->s.algo == SLM_ALGO_GD && !p->lr_set) return fail(SLM_ERR_STATE, "learning rates not set");
    RC(mraf_ready(p));
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    HIP_TRY(hipSetDevice(p->s.device));
    p->field_fresh = false;  // the run writes the field
    p->weights_fresh = false;
    p->ran = true;
    RC(enqueue_stop_reset(p->s));
    RC(e->enqueue(p->s, loops, tol, checked, wa, p->phase_set, p->field_set));
    return enqueue_stats_reduce(p->s, loops, tol);
}

// After the plan stream drained: the engine checks its last run; a run it
// reports invalid is redone by the caller, without the graph that held it.
int settle(slm_plan* p, bool* redo) {
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    RC(e->settle(p->s, redo));
    if (*redo) RC(drop_graph(p));
    return 0;
}

// ---- image sequences (slm_plan_sequence) ----

constexpr size_t kSeqPitch = 256;  // every frame of an uploaded stack starts as aligned as a lone upload does
inline size_t seq_pitch(size_t bytes) { return (bytes + kSeqPitch - 1) / kSeqPitch * kSeqPitch; }

// a host stack of n_frames slices to the device, one slice per pitch
int seq_upload(char* dst, const void* src, size_t slice, size_t n_frames, hipStream_t st) {
    const size_t pitch = seq_pitch(slice);
    if (pitch == slice) {
        HIP_TRY(hipMemcpyAsync(dst, src, slice * n_frames, hipMemcpyHostToDevice, st));
        return 0;
    }
    for (size_t f = 0; f < n_frames; ++f)
        HIP_TRY(hipMemcpyAsync(dst + f * pitch, static_cast<const char*>(src) + f * slice, slice,
                               hipMemcpyHostToDevice, st));
    return 0;
}

// MRAF: the first (frame, hologram) whose region holds no pixel with T > 0.
// regions == nullptr: `fixed` [B][holo] serves every frame.
template <typename TT>
bool seq_mraf_unsupported(const PlanState& s, int n_frames, const void* targets, const uint8_t* regions,
                          const uint8_t* fixed, int* frame, int* holo) {
    const size_t n = (size_t)s.holo;
    for (int f = 0; f < n_frames; ++f)
        for (int b = 0; b < s.B; ++b) {
            const size_t k = (size_t)f * s.B + b;
            const TT* t = static_cast<const TT*>(targets) + k * n;
            const uint8_t* r = regions ? regions + k * n : fixed + (size_t)b * n;
            size_t i = 0;
            while (i < n && !(r[i] && t[i] > 0)) ++i;
            if (i == n) {
                *frame = f;
                *holo = b;
                return true;
            }
        }
    return false;
}

// slm_plan_set_target (and slm_plan_set_region) of frame f from the uploaded
// stacks, enqueued only: the same kernels on the same bytes
int seq_land(slm_plan* p, Engine* e, const char* tgt, const uint8_t* region) {
    PlanState& s = p->s;
    // an engine that reads the target where it was staged keeps it there
    if (e->target_stage(s) == s.tgt) {
        HIP_TRY(hipMemcpyAsync(s.tgt, tgt, (size_t)s.B * s.holo * (s.tt == SLM_TGT_U8 ? 1 : 4),
                               hipMemcpyDeviceToDevice, s.stream));
        tgt = static_cast<const char*>(s.tgt);
    }
    if (s.tt == SLM_TGT_U8)
        target_stats_partial<uint8_t>(p, tgt);
    else
        target_stats_partial<float>(p, tgt);
    RC(e->land_target(s, tgt));
    hipLaunchKernelGGL(target_stats_final_kernel, dim3(s.B), dim3(kTsThreads), 0, s.stream, p->ts_part,
                       ts_blocks(s.holo), s.norm, s.normf, s.sum_t2);
    HIP_TRY(hipGetLastError());
    if (s.algo != SLM_ALGO_MRAF) return 0;
    if (region) RC(e->land_region_dev(s, region));
    return e->mraf_refresh(s, true, nullptr);
}

struct SeqArgs {
    int n_frames, loops_first, loops, resume, rule;
    double tol, ct2pi;
    bool regions, mask, want_frames, want_phases, want_expected;
};

// The chain: per frame the landing, the run from the previous frame's phase,
// and the epilogue into the frame's slabs. Nothing here waits for the device.
int seq_enqueue(slm_plan* p, Engine* e, const SeqArgs& a) {
    PlanState& s = p->s;
    SeqState& q = p->seq;
    const size_t n = (size_t)s.B * s.holo, tpitch = seq_pitch(n * (s.tt == SLM_TGT_U8 ? 1 : 4)), rpitch = seq_pitch(n);
    const bool mraf = s.algo == SLM_ALGO_MRAF;
    // the caller's start phase stays in force after the sequence: frames f > 0
    // read the chain's own buffer in its place
    float* const caller_phase = s.phase_in;
    const bool caller_set = p->phase_set;
    int rc = 0;
    for (int f = 0; f < a.n_frames && !rc; ++f) {
        rc = seq_land(p, e, q.targets.p + (size_t)f * tpitch, a.regions ? q.regions.p + (size_t)f * rpitch : nullptr);
        if (rc) break;
        const bool chained = f > 0 || a.resume;
        s.phase_in = chained ? q.start.p : caller_phase;
        p->phase_set = chained || caller_set;
        rc = enqueue_run(p, chained ? a.loops : a.loops_first, a.tol, a.tol > 0.0 ? 1 : 0, 0.f);
        if (rc) break;
        const size_t fb = (size_t)f * s.B;
        rc = enqueue_phase_frame(s.stream, s.phase_out, a.mask ? q.mask.p : nullptr, (long long)n, s.holo, a.ct2pi,
                                 a.rule, a.want_frames ? q.frames.p + fb * s.holo : nullptr, q.start.p,
                                 a.want_phases ? q.phases.p + fb * s.holo : nullptr);
        if (rc) break;
        if (a.want_expected) {
            const hipError_t err = hipMemcpyAsync(q.expected.p + fb * s.holo, s.e_out, n * sizeof(float),
                                                  hipMemcpyDeviceToDevice, s.stream);
            if (err != hipSuccess) rc = fail(SLM_ERR_HIP, "sequence: copy of E failed: %s", hipGetErrorString(err));
            if (rc) break;
        }
        rc = enqueue_frame_rows(s.stream, s.stats, mraf ? s.eff : nullptr, s.stop, s.B, s.max_loops, q.rows,
                                q.stats.p + fb * q.rows * 4, mraf ? q.eff.p + fb * q.rows : nullptr, q.stop.p + fb);
    }
    s.phase_in = caller_phase;
    p->phase_set = caller_set;
    return rc;
}

void free_plan(slm_plan* p) {
    if (!p) return;
    PlanState& s = p->s;
    (void)hipSetDevice(s.device);
    // work still queued on the plan stream (an unsynchronised run, a
    // stream-ordered device gather or RCCL send) finishes before its buffers go
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    gather_free(p->gather);
    for (void* ptr : {(void*)s.xa, s.tgt, (void*)s.ain, (void*)s.phase_in, (void*)s.phase_out, (void*)s.e_out,
                      (void*)s.partials, (void*)s.stats, (void*)s.stop, (void*)s.norm, (void*)s.normf,
                      (void*)s.sum_t2, (void*)s.field0, (void*)s.lr, (void*)p->ts_part, (void*)s.weights0,
                      (void*)s.region, (void*)s.mraf, (void*)s.eff})
        if (ptr) (void)hipFree(ptr);
    for (auto& e : p->events.pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    if (p->gexec) (void)hipGraphExecDestroy(p->gexec);
    delete p->eng;
    for (hipEvent_t e : p->marks)
        if (e) (void)hipEventDestroy(e);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    delete p;
}

int plan_create_on(int device, int algo, int batch, int height, int width, int tgt_type, int has_ain,
                   int max_loops, slm_plan** out) {
    if (!out) return fail(SLM_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (algo != SLM_ALGO_GS && algo != SLM_ALGO_GD && algo != SLM_ALGO_GSW && algo != SLM_ALGO_MRAF)
        return fail(SLM_ERR_ARG, "unknown algorithm %d", algo);
    if (batch < 1 || max_loops < 1) return fail(SLM_ERR_ARG, "batch and max_loops must be >= 1");
    if (tgt_type != SLM_TGT_U8 && tgt_type != SLM_TGT_F32) return fail(SLM_ERR_ARG, "unknown target type");
    if (height < 1 || width < 1) return fail(SLM_ERR_ARG, "image shape %dx%d", height, width);
    // sides without a radix plan (plans.hpp) run the any-size engine (generic.hpp:
    // mixed-radix kernels, chirp-z line transforms for large prime factors).
    // $SLM_ENGINE=float64
    // sends every shape there: complex128 state and float64 arithmetic
    // throughout, the reference's own dtypes -- the radix plans keep complex64
    // between their passes, which sets GD's float64-butterfly floor at ~3e-5
    // rms after configs[2]'s 500 iterations (profiles/r05/gd_precision_s19.txt)
    const char* eng = std::getenv("SLM_ENGINE");
    const bool forced64 = eng && !std::strcmp(eng, "float64");
    HIP_TRY(hipSetDevice(device));
    // every early return below frees what exists so far
    std::unique_ptr<slm_plan, void (*)(slm_plan*)> guard(new slm_plan(), free_plan);
    slm_plan* p = guard.get();
    PlanState& s = p->s;
    p->any_size = forced64 || !slm_supported_length(height) || !slm_supported_length(width);
    // weighted GS is built into the fused engine's column pass only
    if (algo == SLM_ALGO_GSW && p->any_size)
        return fail(SLM_ERR_UNSUPPORTED,
                    "weighted GS (SLM_ALGO_GSW) runs on the fused engine only: both sides must be one of 64, 128, "
                    "256, 512, 1024, 2048, 4096 (powers of two) or 768%s; got %d x %d",
                    forced64 ? ", and SLM_ENGINE=float64 must not be set" : "", height, width);
    // ... and so is MRAF
    if (algo == SLM_ALGO_MRAF && p->any_size)
        return fail(SLM_ERR_UNSUPPORTED,
                    "MRAF (SLM_ALGO_MRAF) runs on the fused engine only: both sides must be one of 64, 128, "
                    "256, 512, 1024, 2048, 4096 (powers of two) or 768%s; got %d x %d",
                    forced64 ? ", and SLM_ENGINE=float64 must not be set" : "", height, width);
    s.algo = algo;
    s.B = batch;
    s.H = height;
    s.W = width;
    s.tt = tgt_type;
    s.has_ain = has_ain ? 1 : 0;
    s.max_loops = max_loops;
    s.device = device;
    s.holo = (long long)height * width;
    // GS on uint8 targets -- the CLI's input (src/generate_hologram.py:102-110) --
    // takes float64 butterflies by default: float32 measured 7.7e-6 (1024^2) and
    // 8.2e-6 (768 x 1024, the CLI's own shape) of the 1e-5 bar at the +200 warm
    // start, float64 rows alone still 8.5e-6 at 768 x 1024, float64 butterflies
    // <= 3.3e-6 on all six targets (profiles/r06/u8_margin.txt), for ~3 us per
    // iteration. Float32 targets (the bench's) keep float32; $SLM_PRECISION
    // (f32 / f64) overrides both.
    if (gs_like(algo) && tgt_type == SLM_TGT_U8) s.prec = PREC_F64;
    if (const char* e = std::getenv("SLM_PRECISION")) s.prec = (std::strcmp(e, "f64") == 0) ? PREC_F64 : PREC_F32;
    hipError_t se = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
    if (se != hipSuccess) return fail(SLM_ERR_HIP, "stream creation failed: %s", hipGetErrorString(se));
    const size_t n = (size_t)batch * s.holo;
    // X ahead of the engine's Y: the 1024^2 column pass measured 2 % slower with the two the other way round
    RC(dev_alloc(&s.xa, n * sizeof(float2)));
    int max_nwg = 0;  // the partials hold the finest tiling of both precisions
    AnySizeChoice choice;
    if (p->any_size) {
        // float32 GS (float32 targets unless $SLM_PRECISION) on the complex64
        // radix kernels where both sides have one (13-smooth panels, e.g.
        // 1080 x 1920), float64 otherwise and always under $SLM_ENGINE=float64
        const int asked = forced64 ? PREC_F64 : s.prec;
        choice = generic_choose(batch, height, width, algo, asked);
        s.prec = choice.prec;
        s.nwg = choice.nwg;
        // slm_plan_set_precision may switch engines: partials for either tiling
        const int other = asked == PREC_F32 ? PREC_F64 : PREC_F32;
        max_nwg = std::max(choice.nwg, generic_choose(batch, height, width, algo, other).nwg);
    } else {
        RC(fused_create(s, &p->eng, &max_nwg));
    }
    if (algo == SLM_ALGO_GD) {
        RC(dev_alloc(&s.field0, n * sizeof(float2)));
        RC(dev_alloc(&s.lr, (size_t)max_loops * sizeof(float)));
    }
    if (algo == SLM_ALGO_GSW) RC(dev_alloc(&s.weights0, n * sizeof(float)));
    if (algo == SLM_ALGO_MRAF) {
        RC(dev_alloc(&s.region, n + (size_t)2 * batch * sizeof(double)));  // the plane, then the scale rows
        RC(dev_alloc(&s.mraf, ((size_t)kMrafRows * batch + 1) * sizeof(double)));
        RC(dev_alloc(&s.eff, (size_t)batch * max_loops * sizeof(double)));
    }
    RC(dev_alloc(&s.tgt, n * (tgt_type == SLM_TGT_U8 ? 1 : 4)));
    if (has_ain) RC(dev_alloc(&s.ain, (size_t)s.holo * sizeof(float)));
    RC(dev_alloc(&s.phase_out, n * sizeof(float)));
    RC(dev_alloc(&s.e_out, n * sizeof(float)));
    RC(dev_alloc(&s.partials, (size_t)batch * max_loops * max_nwg * 4 * sizeof(double)));
    RC(dev_alloc(&s.stats, (size_t)batch * max_loops * 4 * sizeof(double)));
    RC(dev_alloc(&s.stop, (size_t)batch * sizeof(int)));
    RC(dev_alloc(&s.norm, (size_t)batch * sizeof(double)));
    RC(dev_alloc(&s.normf, (size_t)batch * sizeof(float)));
    RC(dev_alloc(&s.sum_t2, (size_t)batch * sizeof(double)));
    RC(dev_alloc(&p->ts_part, (size_t)batch * ts_blocks(s.holo) * 2 * sizeof(double)));
    if (p->any_size) RC(generic_create(s, choice, &p->eng));
    *out = guard.release();
    return 0;
}

// slm_fft2_c128's float64 engines, cached per (device, batch, h, w) like the
// drop-in's plans: move_traps.update_hologram calls it for every non-blank
// image of the interactive trap loop, which rebuilt stream, buffers, line
// plans and tables each time before r06. A few shapes are kept (oldest out);
// slm_release_caches frees them (algorithms.clear_plans). generic_choose reads
// the engine and geometry overrides from the environment, so an entry also
// keeps their values at its creation: a call under other values builds its own.
struct C128Entry {
    std::string knobs;
    PlanState s;  // device, shape and the entry's own stream; no plan buffers
    Engine* eng = nullptr;
    double2* buf = nullptr;
};
std::mutex g_c128_mu;
std::vector<C128Entry> g_c128;
constexpr size_t kC128CacheMax = 4;

void c128_free(C128Entry& e) {
    if (e.s.stream) (void)hipStreamSynchronize(e.s.stream);
    if (e.buf) (void)hipFree(e.buf);
    delete e.eng;
    if (e.s.stream) (void)hipStreamDestroy(e.s.stream);
    e = C128Entry();
}

// the environment generic_choose (generic.hip) reads: a hit skips the choice,
// so the cache is looked up by the knobs' text, not by their outcome
std::string c128_knobs() {
    std::string s;
    for (const char* name : {"SLM_ENGINE", "SLM_GENERIC_ENGINE", "SLM_RZ_PLAN", "SLM_RZ_ROW_PLAN", "SLM_RZ_COL_PLAN",
                             "SLM_RZ_CW", "SLM_RZ_LAYOUT", "SLM_RZ_PANEL", "SLM_MR_RPW", "SLM_MR_CW"}) {
        const char* v = std::getenv(name);
        s += v ? v : "";
        s += '\n';
    }
    return s;
}

int c128_entry(int batch, int height, int width, C128Entry** out) {
    const std::string knobs = c128_knobs();
    for (auto& e : g_c128)
        if (e.s.device == g_device && e.s.B == batch && e.s.H == height && e.s.W == width && e.knobs == knobs) {
            *out = &e;
            return 0;
        }
    if (g_c128.size() >= kC128CacheMax) {
        (void)hipSetDevice(g_c128.front().s.device);
        c128_free(g_c128.front());
        g_c128.erase(g_c128.begin());
        HIP_TRY(hipSetDevice(g_device));
    }
    C128Entry e;
    e.knobs = knobs;
    PlanState& s = e.s;
    s.algo = SLM_ALGO_GS;
    s.B = batch;
    s.H = height;
    s.W = width;
    s.holo = (long long)height * width;
    s.max_loops = 1;
    const AnySizeChoice choice = generic_choose(batch, height, width, SLM_ALGO_GS, PREC_F64);
    s.prec = choice.prec;
    s.nwg = choice.nwg;
    s.device = g_device;
    int rc = 0;
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess)
        rc = fail(SLM_ERR_HIP, "fft2_c128: stream creation failed");
    const size_t bytes = (size_t)batch * s.holo * sizeof(double2);
    if (!rc && hipMalloc(&e.buf, bytes) != hipSuccess) rc = fail(SLM_ERR_HIP, "fft2_c128: allocation of %zu bytes", bytes);
    if (!rc) rc = generic_create(s, choice, &e.eng);
    if (rc) {
        c128_free(e);
        return rc;
    }
    g_c128.push_back(e);
    *out = &g_c128.back();
    return 0;
}
}  // namespace

// ==========================================================================
// C-ABI
// ==========================================================================
extern "C" {

int slm_init(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(SLM_ERR_HIP, "no HIP device available (%s); libslm_hip has no CPU path",
                    hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(SLM_ERR_ARG, "device %d outside [0, %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    g_device = device;
    return 0;
}

int slm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* slm_last_error(void) { return g_err.c_str(); }

int slm_copy_bandwidth(long long bytes, int reps, double* gbs) {
    if (!gbs || bytes < 16 || reps < 1) return fail(SLM_ERR_ARG, "bad copy-bandwidth arguments");
    RC(ensure_device());
    const long long n = bytes / 16;
    v4f *a = nullptr, *b = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int dev = 0, cus = 0, rc = 0;
    auto hip = [&](hipError_t e) {
        if (e != hipSuccess && !rc) rc = fail(SLM_ERR_HIP, "copy bandwidth: %s", hipGetErrorString(e));
        return rc == 0;
    };
    if (hip(hipGetDevice(&dev)) && hip(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) &&
        hip(hipMalloc(&a, n * 16)) && hip(hipMalloc(&b, n * 16)) && hip(hipStreamCreate(&st)) &&
        hip(hipEventCreate(&e0)) && hip(hipEventCreate(&e1)) && hip(hipMemsetAsync(a, 1, n * 16, st)) &&
        hip(hipMemsetAsync(b, 0, n * 16, st))) {
        // enough workgroups that a working-set-sized copy still fills the chip
        const int grid = (int)std::max<long long>(1, std::min<long long>((long long)cus * 32, (n + 1023) / 1024));
        hipLaunchKernelGGL(copy_f4_kernel, dim3(grid), dim3(256), 0, st, a, b, n);  // warm-up
        // a failed launch would leave the event pair timing an empty stream
        if (hip(hipGetLastError()) && hip(hipEventRecord(e0, st))) {
            for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(copy_f4_kernel, dim3(grid), dim3(256), 0, st, a, b, n);
            float ms = 0.f;
            if (hip(hipGetLastError()) && hip(hipEventRecord(e1, st)) && hip(hipEventSynchronize(e1)) &&
                hip(hipEventElapsedTime(&ms, e0, e1)))
                *gbs = 2.0 * 16.0 * (double)n * reps / (ms * 1e-3) / 1e9;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    return rc;
}

const char* slm_version(void) { return "libslm_hip 0.1 (gfx950)"; }

int slm_supported_length(int n) { return plan_index(n) >= 0 ? 1 : 0; }

int slm_device_pci_bus_id(int device, char* buf, int len) {
    if (!buf || len < 13) return fail(SLM_ERR_ARG, "need a buffer of at least 13 bytes");
    HIP_TRY(hipDeviceGetPCIBusId(buf, len, device));
    return 0;
}

int slm_plan_create(int algo, int batch, int height, int width, int tgt_type, int has_ain, int max_loops,
                    slm_plan** out) {
    RC(ensure_device());
    return plan_create_on(g_device, algo, batch, height, width, tgt_type, has_ain, max_loops, out);
}

int slm_plan_read_trace(slm_plan* p, int kernel_class, unsigned long long* out) {
    if (!p || !out) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    return e->read_trace(p->s, kernel_class, out);
}

int slm_plan_destroy(slm_plan* plan) {
    free_plan(plan);
    return 0;
}

int slm_plan_set_target(slm_plan* p, const void* tgt) {
    if (!p || !tgt) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    PlanState& s = p->s;
    p->seq.resumable = false;
    HIP_TRY(hipSetDevice(s.device));
    const size_t bytes = (size_t)s.B * s.holo * (s.tt == SLM_TGT_U8 ? 1 : 4);
    void* stage = e->target_stage(s);
    // host arrays stay pageable: HIP's staged copies run at ~45 GB/s for a 4 MB
    // target here; pinning the caller's buffer or a pinned staging buffer plus a
    // host memcpy measured no faster (tools/xfer_probe.py)
    HIP_TRY(hipMemcpyAsync(stage, tgt, bytes, hipMemcpyHostToDevice, s.stream));
    if (s.tt == SLM_TGT_U8)
        target_stats_partial<uint8_t>(p, stage);
    else
        target_stats_partial<float>(p, stage);
    RC(e->land_target(s, stage));
    hipLaunchKernelGGL(target_stats_final_kernel, dim3(s.B), dim3(kTsThreads), 0, s.stream, p->ts_part,
                       ts_blocks(s.holo), s.norm, s.normf, s.sum_t2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s.stream));
    p->target_set = true;
    // host-set weights were validated on the previous target's support
    s.weights_set = false;
    p->weights_fresh = false;
    // MRAF: a region that no longer fits the target is refused when a run is asked for
    return mraf_update(p, true);
}

int slm_plan_set_precision(slm_plan* p, int precision) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    if (precision != SLM_PRECISION_F32 && precision != SLM_PRECISION_F64)
        return fail(SLM_ERR_ARG, "unknown precision %d", precision);
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    PlanState& s = p->s;
    p->seq.resumable = false;
    HIP_TRY(hipSetDevice(s.device));
    if (!p->any_size) {  // in place: the plan keeps its layout pair
        RC(drop_graph(p));
        return e->set_precision(s, precision);
    }
    // any-size engine: rebuilt when the precision it runs at changes
    const AnySizeChoice choice = generic_choose(s.B, s.H, s.W, s.algo, precision);
    if (choice.prec == s.prec) return 0;
    HIP_TRY(hipStreamSynchronize(s.stream));
    RC(drop_graph(p));
    const AnySizeChoice old = generic_choice(*e);
    auto rebuild = [&](const AnySizeChoice& c) {
        s.prec = c.prec;
        s.nwg = c.nwg;
        return generic_create(s, c, &p->eng);
    };
    delete p->eng;
    p->eng = nullptr;
    const int rc = rebuild(choice);
    if (rc) {  // keep a usable plan: the engine it had (its error stays the reported one)
        const std::string msg = slm_last_error();
        if (rebuild(old)) p->eng = nullptr;
        return fail(rc, "%s", msg.c_str());
    }
    return 0;
}

int slm_plan_get_precision(slm_plan* p) { return p ? p->s.prec : -1; }

int slm_plan_set_ain(slm_plan* p, const float* ain) {
    if (!p || !ain) return fail(SLM_ERR_ARG, "null argument");
    if (!p->s.has_ain) return fail(SLM_ERR_STATE, "plan was created without an incoming amplitude");
    HIP_TRY(hipSetDevice(p->s.device));
    // Uploads go on the plan stream: the plan's non-blocking stream is not
    // ordered after null-stream copies, and a pageable hipMemcpy may return
    // before its DMA has landed.
    HIP_TRY(hipMemcpyAsync(p->s.ain, ain, (size_t)p->s.holo * sizeof(float), hipMemcpyHostToDevice, p->s.stream));
    HIP_TRY(hipStreamSynchronize(p->s.stream));
    p->ain_set = true;
    p->seq.resumable = false;
    return mraf_update(p, true);
}

int slm_plan_set_phase(slm_plan* p, const float* phase) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    PlanState& s = p->s;
    if (!gs_like(s.algo)) return fail(SLM_ERR_STATE, "initial phase applies to GS plans");
    p->seq.resumable = false;
    HIP_TRY(hipSetDevice(s.device));
    if (!phase) {
        p->phase_set = false;
        return 0;
    }
    const size_t bytes = (size_t)s.B * s.holo * sizeof(float);
    if (!s.phase_in) HIP_TRY(hipMalloc((void**)&s.phase_in, bytes));
    HIP_TRY(hipMemcpyAsync(s.phase_in, phase, bytes, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    p->phase_set = true;
    return 0;
}

int slm_plan_set_field(slm_plan* p, const float* field) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    if (p->s.algo != SLM_ALGO_GD) return fail(SLM_ERR_STATE, "initial field applies to GD plans");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    HIP_TRY(hipSetDevice(p->s.device));
    if (!field) {
        p->field_set = false;
        return 0;
    }
    RC(e->land_field(p->s, field));
    HIP_TRY(hipStreamSynchronize(p->s.stream));
    p->field_set = true;
    p->field_fresh = true;
    return 0;
}

int slm_plan_set_feedback(slm_plan* p, float feedback) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    if (!(feedback >= 0.f) || !std::isfinite(feedback))
        return fail(SLM_ERR_ARG, "feedback exponent %g is not a finite number >= 0", (double)feedback);
    if (p->s.algo != SLM_ALGO_GSW) return fail(SLM_ERR_STATE, "the feedback exponent applies to weighted-GS plans");
    p->s.feedback = feedback;
    p->seq.resumable = false;
    return 0;
}

int slm_plan_set_weights(slm_plan* p, const float* w) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    PlanState& s = p->s;
    if (s.algo != SLM_ALGO_GSW) return fail(SLM_ERR_STATE, "weights apply to weighted-GS plans");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    p->seq.resumable = false;
    HIP_TRY(hipSetDevice(s.device));
    if (!w) {
        s.weights_set = false;
        p->weights_fresh = true;
        return 0;
    }
    if (!p->target_set) return fail(SLM_ERR_STATE, "set the target first: weights are checked on its support");
    HIP_TRY(hipStreamSynchronize(s.stream));  // the staging buffer is scratch of a queued run
    s.weights_set = false;
    bool bad = false;
    RC(e->land_weights(s, w, &bad));
    if (bad) return fail(SLM_ERR_ARG, "weights on the support (T > 0) must be positive and finite");
    s.weights_set = true;
    p->weights_fresh = true;
    return 0;
}

int slm_plan_read_weights(slm_plan* p, float* w) {
    if (!p || !w) return fail(SLM_ERR_ARG, "null argument");
    PlanState& s = p->s;
    if (s.algo != SLM_ALGO_GSW) return fail(SLM_ERR_STATE, "weights are the state of weighted-GS plans");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    RC(slm_plan_sync(p));
    const bool fresh = p->weights_fresh || !p->ran;
    if (fresh && !s.weights_set) {  // ones
        std::fill(w, w + (size_t)s.B * s.holo, 1.f);
        return 0;
    }
    if (!p->target_set) return fail(SLM_ERR_STATE, "target not set");
    return e->read_weights(s, fresh, w);
}

int slm_plan_set_region(slm_plan* p, const uint8_t* region) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    PlanState& s = p->s;
    if (s.algo != SLM_ALGO_MRAF) return fail(SLM_ERR_STATE, "a signal region applies to MRAF plans");
    if (!region) return fail(SLM_ERR_ARG, "null region");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    HIP_TRY(hipSetDevice(s.device));
    HIP_TRY(hipStreamSynchronize(s.stream));  // the staging buffer is scratch of a queued run
    p->region_set = false;
    p->mraf_bad = -1;
    p->seq.resumable = false;
    RC(e->land_region(s, region));
    HIP_TRY(hipStreamSynchronize(s.stream));
    p->region_set = true;
    p->region_host.assign(region, region + (size_t)s.B * s.holo);
    RC(mraf_update(p, true));
    if (p->mraf_bad >= 0) {
        p->region_set = false;
        return mraf_no_support(p->mraf_bad);
    }
    return 0;
}

int slm_plan_set_mixing(slm_plan* p, float m) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    if (!(m > 0.f && m <= 1.f)) return fail(SLM_ERR_ARG, "mixing parameter %g is not in (0, 1]", (double)m);
    if (p->s.algo != SLM_ALGO_MRAF) return fail(SLM_ERR_STATE, "the mixing parameter applies to MRAF plans");
    HIP_TRY(hipSetDevice(p->s.device));
    p->s.mixing = m;
    p->seq.resumable = false;
    return mraf_update(p, false);
}

int slm_plan_read_efficiency(slm_plan* p, double* eff) {
    if (!p || !eff) return fail(SLM_ERR_ARG, "null argument");
    PlanState& s = p->s;
    if (s.algo != SLM_ALGO_MRAF) return fail(SLM_ERR_STATE, "the efficiency is a statistic of MRAF plans");
    RC(slm_plan_sync(p));
    return copy_sync(eff, s.eff, (size_t)s.B * s.max_loops * sizeof(double), hipMemcpyDeviceToHost, s.stream);
}

int slm_plan_set_lr(slm_plan* p, const float* lr) {
    if (!p || !lr) return fail(SLM_ERR_ARG, "null argument");
    PlanState& s = p->s;
    if (s.algo != SLM_ALGO_GD) return fail(SLM_ERR_STATE, "learning rates apply to GD plans");
    HIP_TRY(hipSetDevice(s.device));
    HIP_TRY(hipMemcpyAsync(s.lr, lr, (size_t)s.max_loops * sizeof(float), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    p->lr_set = true;
    return 0;
}

int slm_plan_run(slm_plan* p, int loops, double tol, int checked, float wa) {
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    PlanState& s = p->s;
    RC(mraf_ready(p));
    p->field_fresh = false;  // replays skip enqueue_run
    p->weights_fresh = false;
    p->seq.resumable = false;
    p->seq_tail = false;
    p->last_loops = loops;
    p->last_tol = tol;
    p->last_checked = checked;
    p->last_wa = wa;
    static const bool use_graph = [] {
        const char* v = std::getenv("SLM_GRAPH");
        return !v || std::atoi(v) != 0;
    }();
    if (!use_graph) {
        RC(enqueue_run(p, loops, tol, checked, wa));
        e->queued(s, checked);
        return 0;
    }
    const int state = (p->phase_set ? 1 : 0) | (p->field_set ? 2 : 0) | (s.weights_set ? 4 : 0);
    if (!p->gexec || p->g_state != state || p->g_fb != s.feedback || p->g_loops != loops || p->g_tol != tol || p->g_checked != checked || p->g_wa != wa) {
        HIP_TRY(hipSetDevice(s.device));
        RC(drop_graph(p));
        HIP_TRY(hipStreamBeginCapture(s.stream, hipStreamCaptureModeThreadLocal));
        int rc = enqueue_run(p, loops, tol, checked, wa);
        hipGraph_t g = nullptr;
        hipError_t err = hipStreamEndCapture(s.stream, &g);
        if (rc) {
            if (g) (void)hipGraphDestroy(g);
            return rc;
        }
        HIP_TRY(err);
        err = hipGraphInstantiate(&p->gexec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIP_TRY(err);
        p->g_loops = loops;
        p->g_tol = tol;
        p->g_checked = checked;
        p->g_wa = wa;
        p->g_fb = s.feedback;
        p->g_state = state;
    }
    HIP_TRY(hipSetDevice(s.device));
    HIP_TRY(hipGraphLaunch(p->gexec, s.stream));
    e->queued(s, checked);
    return 0;
}

int slm_plan_run_timed(slm_plan* p, int loops, double tol, int checked, float wa, double* us, int* counts) {
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    PlanState& s = p->s;
    // $SLM_TIMED_HOLD: 100 MHz ticks of hold per launch of the run (0 = no hold)
    static const long long hold = [] {
        const char* v = std::getenv("SLM_TIMED_HOLD");
        return v ? std::atoll(v) : 1000LL;
    }();
    if (hold > 0) {
        // ~10 us of host enqueue per launch of the run, at most 0.2 s
        const long long launches = 2LL * loops + 16;
        const unsigned long long ticks = (unsigned long long)std::min<long long>(launches * hold, 20000000LL);
        HIP_TRY(hipSetDevice(s.device));
        hipLaunchKernelGGL(hold_kernel, dim3(1), dim3(64), 0, s.stream, ticks);
        HIP_TRY(hipGetLastError());
    }
    p->events.used = 0;
    p->seq.resumable = false;
    p->seq_tail = false;
    s.timing = &p->events;
    int rc = enqueue_run(p, loops, tol, checked, wa);
    s.timing = nullptr;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s.stream));
    bool redo = false;
    RC(settle(p, &redo));
    if (redo) return slm_plan_run_timed(p, loops, tol, checked, wa, us, counts);  // now on two launches
    for (int k = 0; k < SLM_NUM_KERNEL_CLASSES; ++k) {
        if (us) us[k] = 0.0;
        if (counts) counts[k] = 0;
    }
    for (size_t i = 0; i < p->events.used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p->events.pool[i].first, p->events.pool[i].second));
        const int c = p->events.cls[i];
        if (us) us[c] += 1000.0 * ms;
        if (counts) counts[c] += 1;
    }
    return 0;
}

int slm_plan_sync(slm_plan* p) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    HIP_TRY(hipSetDevice(p->s.device));
    HIP_TRY(hipStreamSynchronize(p->s.stream));
    if (p->gather.comm_stream) HIP_TRY(hipStreamSynchronize(p->gather.comm_stream));  // queued gathers
    bool redo = false;
    RC(settle(p, &redo));
    if (redo) {  // the last run again, on the two-launch column side (cannot fault)
        RC(slm_plan_run(p, p->last_loops, p->last_tol, p->last_checked, p->last_wa));
        HIP_TRY(hipStreamSynchronize(p->s.stream));
    }
    return 0;
}

int slm_plan_gd_recoveries(slm_plan* p) {
    Engine* e = nullptr;
    return engine_of(p, &e) ? -1 : e->recoveries();
}

int slm_plan_mark(slm_plan* p, int which) {
    if (!p || which < 0 || which > 1) return fail(SLM_ERR_ARG, "bad mark arguments");
    HIP_TRY(hipSetDevice(p->s.device));
    if (!p->marks[which]) HIP_TRY(hipEventCreate(&p->marks[which]));
    // the stopwatch covers the gathers queued on the comm stream too
    RC(gather_order_after(p->gather, p->s.stream));
    HIP_TRY(hipEventRecord(p->marks[which], p->s.stream));
    return 0;
}

int slm_plan_marked_ms(slm_plan* p, double* ms) {
    if (!p || !ms) return fail(SLM_ERR_ARG, "null argument");
    if (!p->marks[0] || !p->marks[1]) return fail(SLM_ERR_STATE, "record marks 0 and 1 first");
    HIP_TRY(hipEventSynchronize(p->marks[1]));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, p->marks[0], p->marks[1]));
    *ms = t;
    return 0;
}

int slm_plan_read(slm_plan* p, float* phase, float* expected, double* stats, int* iters) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    if (p->seq_tail)
        return fail(SLM_ERR_STATE, "no run since the last sequence (its results: slm_plan_sequence_read)");
    RC(slm_plan_sync(p));
    PlanState& s = p->s;
    const size_t n = (size_t)s.B * s.holo;
    if (phase) RC(copy_sync(phase, s.phase_out, n * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    if (expected) RC(copy_sync(expected, s.e_out, n * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    if (stats)
        RC(copy_sync(stats, s.stats, (size_t)s.B * s.max_loops * 4 * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    if (iters) {
        RC(copy_sync(iters, s.stop, (size_t)s.B * sizeof(int), hipMemcpyDeviceToHost, s.stream));
        stop_to_iterations(iters, s.B);
    }
    return 0;
}

int slm_plan_read_target_stats(slm_plan* p, double* norm, double* sum_t2) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    PlanState& s = p->s;
    HIP_TRY(hipSetDevice(s.device));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (norm) RC(copy_sync(norm, s.norm, (size_t)s.B * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    if (sum_t2) RC(copy_sync(sum_t2, s.sum_t2, (size_t)s.B * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    return 0;
}

int slm_plan_set_target_stats(slm_plan* p, const double* norm, const double* sum_t2) {
    if (!p || !norm || !sum_t2) return fail(SLM_ERR_ARG, "null argument");
    if (!p->target_set) return fail(SLM_ERR_STATE, "target not set");
    PlanState& s = p->s;
    p->seq.resumable = false;
    HIP_TRY(hipSetDevice(s.device));
    std::vector<float> nf(s.B);
    for (int b = 0; b < s.B; ++b) nf[b] = (float)norm[b];
    HIP_TRY(hipMemcpyAsync(s.norm, norm, (size_t)s.B * sizeof(double), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(s.normf, nf.data(), (size_t)s.B * sizeof(float), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(s.sum_t2, sum_t2, (size_t)s.B * sizeof(double), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

int slm_plan_sequence(slm_plan* p, int n_frames, const void* targets, const uint8_t* regions, int loops_first,
                      int loops, double tol, int resume, const double* mask, double ct2pi, int rule, int want_frames,
                      int want_phases, int want_expected) {
    if (!p || !targets) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    PlanState& s = p->s;
    SeqState& q = p->seq;
    RC(slm::check_sequence_args(n_frames, loops_first, loops, s.max_loops, tol, rule, ct2pi));
    const bool mraf = s.algo == SLM_ALGO_MRAF;
    if (!gs_like(s.algo)) return fail(SLM_ERR_STATE, "sequences run on GS, weighted-GS and MRAF plans, not on GD plans");
    if (s.has_ain && !p->ain_set) return fail(SLM_ERR_STATE, "slm_plan_sequence before slm_plan_set_ain");
    if (regions && !mraf) return fail(SLM_ERR_STATE, "regions apply to MRAF plans");
    if (mraf && !regions && !p->region_set)
        return fail(SLM_ERR_STATE, "an MRAF sequence needs regions, or a region in force (slm_plan_set_region)");
    if (resume && !q.resumable)
        return fail(SLM_ERR_STATE, "resume needs a previous sequence on this plan with no slm_plan_set_* or run since");
    if (mraf) {
        int f = 0, b = 0;
        const bool bad = s.tt == SLM_TGT_U8
                             ? seq_mraf_unsupported<uint8_t>(s, n_frames, targets, regions, p->region_host.data(), &f, &b)
                             : seq_mraf_unsupported<float>(s, n_frames, targets, regions, p->region_host.data(), &f, &b);
        if (bad)
            return fail(SLM_ERR_ARG, "frame %d: the signal region of hologram %d holds no pixel with T > 0", f, b);
    }
    HIP_TRY(hipSetDevice(s.device));

    // ---- buffers, sized for this call ----
    const size_t F = (size_t)n_frames, n = (size_t)s.B * s.holo, tbytes = n * (s.tt == SLM_TGT_U8 ? 1 : 4);
    const int rows = std::max(loops_first, loops);
    q.n_frames = 0;  // nothing to read, and nothing to resume from, if this call fails half way
    q.resumable = false;
    RC(q.targets.need(F * seq_pitch(tbytes), s.stream));
    if (regions) RC(q.regions.need(F * seq_pitch(n), s.stream));
    if (want_frames && mask) RC(q.mask.need((size_t)s.holo * sizeof(double), s.stream));
    RC(q.start.need(n * sizeof(float), s.stream));
    if (want_frames) RC(q.frames.need(F * n, s.stream));
    if (want_phases) RC(q.phases.need(F * n * sizeof(float), s.stream));
    if (want_expected) RC(q.expected.need(F * n * sizeof(float), s.stream));
    RC(q.stats.need(F * s.B * rows * 4 * sizeof(double), s.stream));
    if (mraf) RC(q.eff.need(F * s.B * rows * sizeof(double), s.stream));
    RC(q.stop.need(F * s.B * sizeof(int), s.stream));

    // ---- everything the chain reads goes up once, and has landed before the first launch ----
    RC(seq_upload(q.targets.p, targets, tbytes, F, s.stream));
    if (regions) RC(seq_upload(reinterpret_cast<char*>(q.regions.p), regions, n, F, s.stream));
    if (want_frames && mask)
        HIP_TRY(hipMemcpyAsync(q.mask.p, mask, (size_t)s.holo * sizeof(double), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));

    // ---- the plan is as after slm_plan_set_target (and _set_region) with the last frame ----
    p->target_set = true;
    s.weights_set = false;  // weighted GS: every frame starts from ones, as after slm_plan_set_target
    p->weights_fresh = false;
    if (regions) {
        const uint8_t* last = regions + (F - 1) * n;
        p->region_host.assign(last, last + n);
        p->region_set = true;
    }
    p->mraf_bad = -1;  // checked above, frame by frame

    const SeqArgs a{n_frames, loops_first, loops, resume, rule, tol, ct2pi, regions != nullptr,
                    want_frames && mask, want_frames != 0, want_phases != 0, want_expected != 0};
    q.rows = rows;
    RC(seq_enqueue(p, e, a));
    q.n_frames = n_frames;
    q.has_frames = want_frames != 0;
    q.has_phases = want_phases != 0;
    q.has_expected = want_expected != 0;
    q.resumable = true;
    p->seq_tail = true;
    return 0;
}

int slm_plan_sequence_read(slm_plan* p, unsigned char* frames, float* phases, float* expected, double* stats,
                           double* efficiency, int* iters) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    PlanState& s = p->s;
    const SeqState& q = p->seq;
    if (!q.n_frames) return fail(SLM_ERR_STATE, "slm_plan_sequence_read before a sequence");
    if (frames && !q.has_frames) return fail(SLM_ERR_STATE, "the sequence was run without frames");
    if (phases && !q.has_phases) return fail(SLM_ERR_STATE, "the sequence was run without phases");
    if (expected && !q.has_expected) return fail(SLM_ERR_STATE, "the sequence was run without expected outputs");
    if (efficiency && s.algo != SLM_ALGO_MRAF)
        return fail(SLM_ERR_STATE, "the efficiency is a statistic of MRAF plans");
    HIP_TRY(hipSetDevice(s.device));
    HIP_TRY(hipStreamSynchronize(s.stream));
    const size_t fb = (size_t)q.n_frames * s.B, n = fb * s.holo;
    if (frames) RC(copy_sync(frames, q.frames.p, n, hipMemcpyDeviceToHost, s.stream));
    if (phases) RC(copy_sync(phases, q.phases.p, n * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    if (expected) RC(copy_sync(expected, q.expected.p, n * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    if (stats) RC(copy_sync(stats, q.stats.p, fb * q.rows * 4 * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    if (efficiency) RC(copy_sync(efficiency, q.eff.p, fb * q.rows * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    if (iters) {
        RC(copy_sync(iters, q.stop.p, fb * sizeof(int), hipMemcpyDeviceToHost, s.stream));
        stop_to_iterations(iters, (long long)fb);
    }
    return 0;
}

long long slm_plan_kernel_bytes(slm_plan* p, int cls) {
    Engine* e = nullptr;
    return engine_of(p, &e) ? -1 : e->kernel_bytes(p->s, cls);
}

int slm_plan_info(slm_plan* p, int* info) {
    if (!p || !info) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    e->info(p->s, info);
    return 0;
}

int slm_plan_generic_info(slm_plan* p, int* info) {
    if (!p || !info) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    return e->generic_info(info);
}

int slm_plan_engine(slm_plan* p, int* col_engine, int* row_engine) {
    if (!p || !col_engine || !row_engine) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    e->codes(p->s, col_engine, row_engine);
    return 0;
}

int slm_plan_device(slm_plan* p) { return p ? p->s.device : -1; }

int slm_plan_layout(slm_plan* p, int* x_log2, int* y_log2) {
    if (!p || !x_log2 || !y_log2) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    e->layout(x_log2, y_log2);
    return 0;
}

int slm_gs(const void* tgt, int tgt_type, const float* ain, int batch, int height, int width, int max_loops,
           double tol, const float* init_phase, float* out_phase, float* out_expected, double* out_stats,
           int* out_iters) {
    slm_plan* p = nullptr;
    RC(slm_plan_create(SLM_ALGO_GS, batch, height, width, tgt_type, ain != nullptr, max_loops, &p));
    int rc = slm_plan_set_target(p, tgt);
    if (!rc && ain) rc = slm_plan_set_ain(p, ain);
    if (!rc && init_phase) rc = slm_plan_set_phase(p, init_phase);
    if (!rc) rc = slm_plan_run(p, max_loops, tol, tol > 0.0 ? 1 : 0, 0.f);
    if (!rc) rc = slm_plan_read(p, out_phase, out_expected, out_stats, out_iters);
    free_plan(p);
    return rc;
}

int slm_gsw(const void* tgt, int tgt_type, const float* ain, int batch, int height, int width, int max_loops,
            double tol, const float* init_phase, float* out_phase, float* out_expected, double* out_stats,
            int* out_iters, float feedback, const float* init_weights, float* out_weights) {
    slm_plan* p = nullptr;
    RC(slm_plan_create(SLM_ALGO_GSW, batch, height, width, tgt_type, ain != nullptr, max_loops, &p));
    int rc = slm_plan_set_target(p, tgt);
    if (!rc) rc = slm_plan_set_feedback(p, feedback);
    if (!rc && ain) rc = slm_plan_set_ain(p, ain);
    if (!rc && init_phase) rc = slm_plan_set_phase(p, init_phase);
    if (!rc && init_weights) rc = slm_plan_set_weights(p, init_weights);
    if (!rc) rc = slm_plan_run(p, max_loops, tol, tol > 0.0 ? 1 : 0, 0.f);
    if (!rc) rc = slm_plan_read(p, out_phase, out_expected, out_stats, out_iters);
    if (!rc && out_weights) rc = slm_plan_read_weights(p, out_weights);
    free_plan(p);
    return rc;
}

int slm_gd(const void* tgt, int tgt_type, const float* ain, int batch, int height, int width, int max_loops,
           double tol, const float* init_field, const float* lr, float wa, float* out_phase, float* out_expected,
           double* out_stats, int* out_iters) {
    slm_plan* p = nullptr;
    RC(slm_plan_create(SLM_ALGO_GD, batch, height, width, tgt_type, ain != nullptr, max_loops, &p));
    int rc = slm_plan_set_target(p, tgt);
    if (!rc && ain) rc = slm_plan_set_ain(p, ain);
    if (!rc && init_field) rc = slm_plan_set_field(p, init_field);
    if (!rc) rc = slm_plan_set_lr(p, lr);
    if (!rc) rc = slm_plan_run(p, max_loops, tol, tol > 0.0 ? 1 : 0, wa);
    if (!rc) rc = slm_plan_read(p, out_phase, out_expected, out_stats, out_iters);
    free_plan(p);
    return rc;
}

int slm_gs_multi_timing(int max_shards, double* wall_ms, double* run_ms) {
    std::lock_guard<std::mutex> lk(g_multi_mu);
    const int n = (int)g_multi_wall.size();
    for (int r = 0; r < n && r < max_shards; ++r) {
        if (wall_ms) wall_ms[r] = g_multi_wall[r];
        if (run_ms) run_ms[r] = g_multi_run[r];
    }
    return n;
}

static int gs_multi_run(int algo, float feedback, int n_gpus, const int* devices, const void* tgt, int tgt_type,
                        const float* ain, int batch, int height, int width, int max_loops, double tol,
                        const float* init_phase, float* out_phase, float* out_expected, double* out_stats,
                        int* out_iters);

int slm_gs_multi(int n_gpus, const int* devices, const void* tgt, int tgt_type, const float* ain, int batch,
                 int height, int width, int max_loops, double tol, const float* init_phase, float* out_phase,
                 float* out_expected, double* out_stats, int* out_iters) {
    return gs_multi_run(SLM_ALGO_GS, 0.f, n_gpus, devices, tgt, tgt_type, ain, batch, height, width, max_loops, tol,
                        init_phase, out_phase, out_expected, out_stats, out_iters);
}

int slm_gsw_multi(int n_gpus, const int* devices, const void* tgt, int tgt_type, const float* ain, int batch,
                  int height, int width, int max_loops, double tol, const float* init_phase, float* out_phase,
                  float* out_expected, double* out_stats, int* out_iters, float feedback) {
    return gs_multi_run(SLM_ALGO_GSW, feedback, n_gpus, devices, tgt, tgt_type, ain, batch, height, width, max_loops,
                        tol, init_phase, out_phase, out_expected, out_stats, out_iters);
}

// slm_gs_multi / slm_gsw_multi: shard r of the batch on devices[r], one host thread and plan each
static int gs_multi_run(int algo, float feedback, int n_gpus, const int* devices, const void* tgt, int tgt_type,
                        const float* ain, int batch, int height, int width, int max_loops, double tol,
                        const float* init_phase, float* out_phase, float* out_expected, double* out_stats,
                        int* out_iters) {
    if (n_gpus < 1) return fail(SLM_ERR_ARG, "n_gpus must be >= 1");
    if (!tgt || batch < 1) return fail(SLM_ERR_ARG, "need a target batch");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SLM_ERR_HIP, "no HIP device available; libslm_hip has no CPU path");
    std::vector<int> dev(n_gpus);
    for (int r = 0; r < n_gpus; ++r) {
        dev[r] = devices ? devices[r] : r;
        if (dev[r] < 0 || dev[r] >= ndev) return fail(SLM_ERR_ARG, "shard %d: device %d outside [0, %d)", r, dev[r], ndev);
    }
    // contiguous shards in batch order, the first batch % n_gpus one larger
    // (parallel.shard_counts; the same arithmetic as slm_gather_layout)
    std::vector<int> counts(n_gpus);
    for (int r = 0; r < n_gpus; ++r) counts[r] = batch / n_gpus + (r < batch % n_gpus ? 1 : 0);
    std::vector<long long> off(n_gpus + 1);
    RC(slm_gather_layout(n_gpus, counts.data(), 1, off.data()));
    const long long holo = (long long)height * width;
    const size_t tb = tgt_type == SLM_TGT_U8 ? 1 : 4;
    std::vector<int> rcs(n_gpus, 0);
    std::vector<std::string> errs(n_gpus);
    std::vector<double> wall(n_gpus, 0.0), run(n_gpus, 0.0);
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    auto shard = [&](int r) {
        if (!counts[r]) return;
        const auto t0 = clk::now();
        const long long h0 = off[r];
        slm_plan* p = nullptr;
        int rc = plan_create_on(dev[r], algo, counts[r], height, width, tgt_type, ain != nullptr, max_loops, &p);
        if (!rc && algo == SLM_ALGO_GSW) rc = slm_plan_set_feedback(p, feedback);
        if (!rc) rc = slm_plan_set_target(p, static_cast<const char*>(tgt) + (size_t)h0 * holo * tb);
        if (!rc && ain) rc = slm_plan_set_ain(p, ain);
        if (!rc && init_phase) rc = slm_plan_set_phase(p, init_phase + h0 * holo);
        const auto t1 = clk::now();
        if (!rc) rc = slm_plan_run(p, max_loops, tol, tol > 0.0 ? 1 : 0, 0.f);
        if (!rc) rc = slm_plan_sync(p);
        run[r] = ms_since(t1);
        // each shard lands in its own slice of the caller's arrays over its GPU's own link
        if (!rc)
            rc = slm_plan_read(p, out_phase ? out_phase + h0 * holo : nullptr,
                               out_expected ? out_expected + h0 * holo : nullptr,
                               out_stats ? out_stats + h0 * (long long)max_loops * 4 : nullptr,
                               out_iters ? out_iters + h0 : nullptr);
        if (rc) errs[r] = g_err;  // thread-local message of this shard's thread
        free_plan(p);
        rcs[r] = rc;
        wall[r] = ms_since(t0);
    };
    if (n_gpus == 1) {
        shard(0);
    } else {
        std::vector<std::thread> th;
        for (int r = 0; r < n_gpus; ++r) th.emplace_back(shard, r);
        for (auto& t : th) t.join();
    }
    {
        std::lock_guard<std::mutex> lk(g_multi_mu);
        g_multi_wall = wall;
        g_multi_run = run;
    }
    for (int r = 0; r < n_gpus; ++r)
        if (rcs[r]) return fail(rcs[r], "shard %d (device %d): %s", r, dev[r], errs[r].c_str());
    return 0;
}

int slm_fft2(const float* in, float* out, int batch, int height, int width, int inverse) {
    if (!in || !out) return fail(SLM_ERR_ARG, "null argument");
    slm_plan* p = nullptr;
    RC(slm_plan_create(SLM_ALGO_GS, batch, height, width, SLM_TGT_F32, 0, 1, &p));
    const int rc = p->eng->fft2(p->s, in, out, inverse);
    free_plan(p);
    return rc;
}

int slm_fft2_intensity(const float* phase, int batch, int height, int width, float* intensity_out) {
    if (!phase || !intensity_out) return fail(SLM_ERR_ARG, "null argument");
    slm_plan* p = nullptr;
    RC(slm_plan_create(SLM_ALGO_GS, batch, height, width, SLM_TGT_F32, 0, 1, &p));
    int rc = slm_plan_set_phase(p, phase);
    if (!rc) rc = p->eng->intensity(p->s);
    if (!rc) rc = slm_plan_read(p, nullptr, intensity_out, nullptr, nullptr);
    free_plan(p);
    return rc;
}

int slm_plan_read_field(slm_plan* p, float* field) {
    if (!p || !field) return fail(SLM_ERR_ARG, "null argument");
    if (p->s.algo != SLM_ALGO_GD) return fail(SLM_ERR_STATE, "the field is the state of GD plans");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    HIP_TRY(hipSetDevice(p->s.device));
    if (!p->field_fresh && !p->ran) return fail(SLM_ERR_STATE, "no field yet: neither set_field nor a run");
    return e->read_field(p->s, p->field_fresh, field);
}

int slm_fft2_c128(const double* in, double* out, int batch, int height, int width, int inverse) {
    if (!in || !out) return fail(SLM_ERR_ARG, "null argument");
    if (batch < 1 || height < 1 || width < 1) return fail(SLM_ERR_ARG, "shape %d x %d x %d", batch, height, width);
    RC(ensure_device());
    HIP_TRY(hipSetDevice(g_device));
    // the float64 engine of the any-size plans (radix-plan kernels on 2^k / 768
    // sides, mixed radix where the sides factor, else chirp-z line
    // transforms), whatever the shape, cached per shape
    std::lock_guard<std::mutex> lk(g_c128_mu);
    C128Entry* e = nullptr;
    RC(c128_entry(batch, height, width, &e));
    const size_t bytes = (size_t)batch * e->s.holo * sizeof(double2);
    if (hipMemcpyAsync(e->buf, in, bytes, hipMemcpyHostToDevice, e->s.stream) != hipSuccess)
        return fail(SLM_ERR_HIP, "fft2_c128: upload failed");
    RC(e->eng->fft2_z(e->s, e->buf, e->buf, inverse));
    return copy_sync(out, e->buf, bytes, hipMemcpyDeviceToHost, e->s.stream);
}

int slm_release_caches(void) {
    std::lock_guard<std::mutex> lk(g_c128_mu);
    int dev = 0;
    const bool have = hipGetDevice(&dev) == hipSuccess;
    for (auto& e : g_c128) {
        (void)hipSetDevice(e.s.device);
        c128_free(e);
    }
    g_c128.clear();
    if (have) (void)hipSetDevice(dev);
    return 0;
}

}  // extern "C"
