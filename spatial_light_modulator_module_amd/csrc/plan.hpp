// A plan as the host runtime sees it: the state both engines read and write
// (PlanState), the interface an engine implements (Engine: fused.hip runs the
// radix-plan shapes, generic.hip every other), the gather state of comm.hip,
// and slm_plan itself. slm_capi.hip owns the shared buffers, the captured
// graph and the timing; an engine owns its layouts, tables and work buffers.
#pragma once
#include <climits>
#include <utility>
#include <vector>

#include "runtime.hpp"

namespace slm {

// Per-launch event pairs of a timed run (slm_plan_run_timed), reused between runs.
struct EventPool {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    std::vector<int> cls;  // kernel class of each used pair
    size_t used = 0;
    // the next pair, for a launch of kernel class c
    int next(int c, std::pair<hipEvent_t, hipEvent_t>** ev) {
        if (used == pool.size()) {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            pool.emplace_back(a, b);
            cls.push_back(c);
        }
        cls[used] = c;
        *ev = &pool[used++];
        return 0;
    }
};

// What both engines read and write: shape, the plan stream, and the buffers
// slm_capi.hip allocates (row-major [B][H][W] unless an engine lands them in
// its own layout: the fused engine keeps tgt and field0 blocked).
struct PlanState {
    int algo = 0, B = 0, H = 0, W = 0, tt = 1, has_ain = 0, max_loops = 0;
    // statistics blocks per hologram (the partials' tiling): fused_create's pick,
    // or AnySizeChoice::nwg (generic.hpp) of the engine the plan has
    int nwg = 0;
    // arithmetic the engine runs (SLM_PRECISION_*); parity at both: tests/test_gpu_precision.py
    int prec = SLM_PRECISION_F32;
    int device = 0;
    long long holo = 0;
    hipStream_t stream = nullptr;
    void* tgt = nullptr;          // target intensity (uint8 or float32; the fused GS engine: its amplitude)
    float* ain = nullptr;         // incoming amplitude [H][W] or nullptr
    float* phase_in = nullptr;    // GS warm start
    float2* field0 = nullptr;     // GD: host-set initial field, never overwritten by a run
    float* weights0 = nullptr;    // weighted GS: host-set initial weights, never overwritten by a run
    bool weights_set = false;     // ... in force (else every run starts from ones)
    float feedback = 1.f;         // weighted GS: exponent p of g *= (a_T / |C|)^p
    // MRAF: signal region R (R > 0), laid out like a uint8 target, and its two scale
    // rows behind it (kernels.hpp, mraf_scales); runs never write either
    uint8_t* region = nullptr;
    float mixing = 0.4f;          // MRAF: mixing parameter m
    // MRAF: per-hologram constants, kMrafRows rows of [B] doubles (MrafRow), then
    // sum a_in^2; reduced on the device when the target, the region or a_in
    // changes, rescaled when m does (FusedEngine::mraf_refresh)
    double* mraf = nullptr;
    double* eff = nullptr;        // MRAF: efficiency sum_sr E / P, [B][max_loops]
    float* lr = nullptr;          // GD learning rate per iteration
    float* phase_out = nullptr;
    float* e_out = nullptr;       // |C|^2 (GS) / |F|^2 (GD) of the last iteration, float32
    double* partials = nullptr;   // [B][max_loops][nwg][4]
    double* stats = nullptr;      // [B][max_loops][4]
    int* stop = nullptr;          // [B]
    double* norm = nullptr;       // max(T) [B]
    float* normf = nullptr;       // the same as float32 (the fused kernels' operand)
    double* sum_t2 = nullptr;     // sum T^2 [B]
    // complex64 [B][H][W]: the fused engine's X state; the any-size engine's
    // staging for complex64 transfers (fft2, read_field)
    float2* xa = nullptr;
    EventPool* timing = nullptr;  // a timed run is being enqueued: every launch takes an event pair
};

// GS, weighted GS and MRAF share the iteration and the warm start
inline bool gs_like(int algo) { return algo == SLM_ALGO_GS || algo == SLM_ALGO_GSW || algo == SLM_ALGO_MRAF; }

// rows of PlanState::mraf, each [B]: the reductions over the signal region sr
// (pixels, sum a_T^2, max T, sum T^2, pixels with T > 0) and what follows from
// them (1 / N_sr, P = S sum a_in^2); m kappa and 1 - m sit behind the region
// plane, where the column kernel reads them (kernels.hpp, mraf_scales)
enum MrafRow : int {
    MRAF_N = 0, MRAF_SUM_A2, MRAF_MAX_T, MRAF_SUM_T2, MRAF_NPOS, MRAF_INV_N, MRAF_POWER, kMrafRows
};

struct Engine {
    virtual ~Engine() {}
    // set_target: the upload goes to stage(), then land_target puts it where
    // the kernels read it (s.tgt, the engine's layout)
    virtual void* target_stage(const PlanState& s) = 0;
    virtual int land_target(PlanState& s, const void* staged) = 0;
    // host complex64 [B][H][W] -> s.field0 (enqueued; the caller synchronises)
    virtual int land_field(PlanState& s, const float* field) = 0;
    // weighted GS (the fused engine only): host float32 [B][H][W] -> s.weights0,
    // validated on the support; the weights to the host (mean 1 on the support)
    virtual int land_weights(PlanState& s, const float* w, bool* bad);
    virtual int read_weights(PlanState& s, bool fresh, float* w);
    // MRAF (the fused engine only): host uint8 [B][H][W] -> s.region; the region
    // constants of s.mraf from the target, the region, a_in and m (`reduce`: the
    // reductions too, else the two rows that depend on m alone); *bad_holo: the
    // first hologram whose region holds no pixel with T > 0, or -1
    // land_region_dev: the same from a row-major plane already on the device (a
    // sequence's uploaded stack). bad_holo == nullptr: the caller has checked
    // the support itself, and the refresh is enqueued without the copy back
    // that the check costs (nothing synchronises with the host).
    virtual int land_region(PlanState& s, const uint8_t* region);
    virtual int land_region_dev(PlanState& s, const uint8_t* region);
    virtual int mraf_refresh(PlanState& s, bool reduce, int* bad_holo);
    // one full run (setup, loops iterations, phase and expected output), on s.stream
    virtual int enqueue(PlanState& s, int loops, double tol, int checked, float wa, bool phase_set,
                        bool field_set) = 0;
    // a run of the plan was queued (launched or replayed)
    virtual void queued(const PlanState& s, int checked) {}
    // a queued run may still have to be settled (checked and, if need be, redone)
    virtual bool unsettled() const { return false; }
    // after the stream drained: *redo if the last run's results are invalid and
    // the caller has to drop its captured graph and run it again
    virtual int settle(PlanState& s, bool* redo) {
        *redo = false;
        return 0;
    }
    virtual int recoveries() const { return 0; }
    // in-place change of arithmetic (the any-size engine is rebuilt instead)
    virtual int set_precision(PlanState& s, int precision) = 0;
    // the GD field to the host: field0 if `fresh` (set since the last run), else the state
    virtual int read_field(PlanState& s, bool fresh, float* field) = 0;
    // unscaled 2-D DFT, host complex64 [B][H][W] in and out
    virtual int fft2(PlanState& s, const float* in, float* out, int inverse) = 0;
    // unscaled 2-D DFT of complex128 [B][H][W] (device in / out; in may equal out)
    virtual int fft2_z(PlanState& s, const double2* in, double2* out, int inverse);
    // |fft2(exp(i phase_in))|^2 into s.e_out
    virtual int intensity(PlanState& s) = 0;
    virtual long long kernel_bytes(const PlanState& s, int cls) const = 0;
    virtual void codes(const PlanState& s, int* col_engine, int* row_engine) const = 0;  // slm_plan_engine
    virtual void layout(int* x_log2, int* y_log2) const = 0;
    virtual void info(const PlanState& s, int info[8]) const = 0;  // slm_plan_info
    virtual int generic_info(int info[8]) const;                   // slm_plan_generic_info
    virtual int read_trace(PlanState& s, int kernel_class, unsigned long long* out);
};

// s.stop as read back (the index of the stopping iteration, INT_MAX if none)
// -> iterations executed, -1: ran all loops
inline void stop_to_iterations(int* v, long long n) {
    for (long long k = 0; k < n; ++k) v[k] = v[k] == INT_MAX ? -1 : v[k] + 1;
}

// s.stop to "ran all loops" before a run; the statistics of its iterations
// after it (fused.hip, the one translation unit that includes layout_kernels.hpp)
int enqueue_stop_reset(PlanState& s);
int enqueue_stats_reduce(PlanState& s, int loops, double tol);

// the fused radix engine of a shape whose sides both have a radix plan
// (plans.hpp): picks tilings and layouts, allocates its buffers, sets s.nwg.
// *max_nwg: the finest statistics tiling of either precision.
int fused_create(PlanState& s, Engine** out, int* max_nwg);

// Gathers of one plan (comm.hip). They may run on their own stream behind a
// staging copy, so a rank's next run (plan stream) overlaps the RCCL transfer
// of the previous step's slab: two staging buffers, used alternately; the copy
// into one waits for the send that last read it (done).
struct GatherState {
    struct Slab {  // root-side destination of one gathered array, grown as needed
        void* buf = nullptr;
        long long elems = 0;
    } phase, stats, stop;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ready = nullptr;
    hipEvent_t done[2] = {nullptr, nullptr};
    bool done_set[2] = {false, false};
    int last = -1;  // slot of the last staged gather (its done event orders marks / timing)
    void* stage[2] = {nullptr, nullptr};
    size_t stage_cap[2] = {0, 0};
    int stage_next = 0;
};
// the plan stream waits for the last staged gather
int gather_order_after(GatherState& g, hipStream_t stream);
// waits for queued gathers, frees buffers, events and the comm stream
void gather_free(GatherState& g);

// The last image sequence of a plan (slm_plan_sequence): the uploaded stacks
// the chain reads and the per-frame slabs it writes. Sized at the call, only
// grow, go with the plan.
struct SeqState {
    DevBuf<char> targets;      // [F] frames of [B][H][W], each at a 256-byte pitch
    DevBuf<uint8_t> regions;   // MRAF: the same for the regions
    DevBuf<double> mask;       // [H][W]
    DevBuf<float> start;       // [B][H][W]: the phase the last frame ended with = the next frame's start
    DevBuf<uint8_t> frames;    // [F][B][H][W]
    DevBuf<float> phases, expected;  // [F][B][H][W]
    DevBuf<double> stats;      // [F][B][rows][4]
    DevBuf<double> eff;        // MRAF: [F][B][rows]
    DevBuf<int> stop;          // [F][B], as PlanState::stop
    int n_frames = 0;          // of the last sequence (0: none to read)
    int rows = 0;              // max(loops_first, loops) of the last sequence
    bool has_frames = false, has_phases = false, has_expected = false;
    bool resumable = false;    // no slm_plan_set_* and no run since the last sequence
};

// The per-frame epilogue of a sequence (frames.hip), enqueued on `st`: the
// run's float32 phase [n] -> the uint8 frame (quantize.hpp; frame may be
// nullptr), the next frame's start phase, and the kept phase slice (keep may
// be nullptr). mask [holo] float64 or nullptr.
int enqueue_phase_frame(hipStream_t st, const float* phase, const double* mask, long long n, long long holo,
                        double ct2pi, int rule, uint8_t* frame, float* next_start, float* keep);
// rows 0 .. rows-1 of every hologram's statistics (and efficiency, unless
// nullptr) and the stop words of the run that just ended -> frame slabs
int enqueue_frame_rows(hipStream_t st, const double* stats, const double* eff, const int* stop, int B, int max_loops,
                       int rows, double* stats_out, double* eff_out, int* stop_out);

}  // namespace slm

struct slm_plan {
    slm::PlanState s;
    slm::Engine* eng = nullptr;  // null only after a failed rebuild (slm_plan_set_precision)
    // sides without a radix plan (or $SLM_ENGINE=float64): the any-size engine
    // (generic.hpp), rebuilt when its precision changes
    bool any_size = false;
    double* ts_part = nullptr;  // target statistics, stage 1
    bool target_set = false, phase_set = false, field_set = false, lr_set = false;
    bool ran = false;          // a run was enqueued (the state buffers hold something)
    bool field_fresh = false;  // set_field since the last run: the plan's field is field0
    bool weights_fresh = false;  // set_weights since the last run: the plan's weights are weights0 (or ones)
    bool region_set = false;     // MRAF: slm_plan_set_region succeeded
    int mraf_bad = -1;           // MRAF: a hologram whose region holds no pixel with T > 0 (a run refuses it)
    bool ain_set = false;        // slm_plan_set_ain succeeded
    // MRAF: the region in force as the caller gave it (a sequence without
    // regions of its own checks every frame's support against it on the host)
    std::vector<uint8_t> region_host;
    slm::SeqState seq;           // slm_plan_sequence
    bool seq_tail = false;       // a sequence and no run since: slm_plan_read has nothing of a run to return
    // parameters of the last enqueued run (settling a faulted run redoes it)
    int last_loops = 0, last_checked = 0;
    double last_tol = 0.0;
    float last_wa = 0.f;
    slm::EventPool events;  // slm_plan_run_timed
    hipEvent_t marks[2] = {nullptr, nullptr};  // slm_plan_mark stopwatch
    // replayed run (default; SLM_GRAPH=0 launches kernel by kernel): the whole
    // enqueue_run captured once per (loops, tol, checked, wa, warm-start state)
    // and relaunched as one graph -- 3 % per 1024^2 GS iteration, 6 % at 256^2
    // (gpurun_out/exp17: the inter-kernel gaps of 400 dependent launches)
    hipGraphExec_t gexec = nullptr;
    int g_loops = -1, g_checked = -1, g_state = -1;
    double g_tol = 0.0;
    float g_wa = 0.f, g_fb = 0.f;
    slm::GatherState gather;
};

// the plan's engine; the one place a plan without one (a failed rebuild) is refused
int engine_of(slm_plan* p, slm::Engine** e);
