// The fused radix engine (plan.hpp Engine): GS / GD iterations on shapes whose
// sides both have a radix plan (plans.hpp), as one column launch and one row
// launch per iteration on complex64 state in blocked layouts (kernels.hpp).
// Owns the tiling and layout choice, the twiddle cache, its state buffers and
// the grid-barrier fault recovery of the one-launch GD column side.
#include <hip/hip_ext.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "dispatch.hpp"
#include "layout_kernels.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace slm {

namespace {

std::mutex g_mu;
std::map<std::tuple<int, int, int>, void*> g_twiddles;  // (device, plan key, precision) -> table

// Twiddle table of one radix plan, in its pass order: entry
// [(r - 1) * Ns + j] = exp(-2 pi i j r / (Ns R)), computed in double and
// stored as float2 (PREC_F32) or double2 (PREC_F64).
int get_twiddles(int pk, int prec, const void** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));  // tables live on the calling thread's current device
    std::lock_guard<std::mutex> lk(g_mu);
    auto key = std::make_tuple(dev, pk, prec);
    auto it = g_twiddles.find(key);
    if (it != g_twiddles.end()) {
        *out = it->second;
        return 0;
    }
    if (pk < 0 || pk >= kNumPlans) return fail(SLM_ERR_UNSUPPORTED, "unknown plan key %d", pk);
    const RadixPlan& pl = kPlans[pk];
    std::vector<double> host;  // interleaved re, im
    int ns = 1;
    for (int k = 0; k < pl.npass; ++k) {
        const int r_ = pl.r[k];
        if (ns > 1) {
            const long long L = (long long)ns * r_;
            for (int r = 1; r < r_; ++r)
                for (int j = 0; j < ns; ++j) {
                    const long long q = ((long long)j * r) % L;
                    const double ang = -2.0 * M_PI * (double)q / (double)L;
                    host.push_back(std::cos(ang));
                    host.push_back(std::sin(ang));
                }
        }
        ns *= r_;
    }
    if (host.empty()) {
        host.push_back(1.0);
        host.push_back(0.0);
    }
    if (pl.n == kShufN && pl.e == 8) {
        // the wave-shuffle pair's table (fft_shuffle.hpp): the N roots
        // exp(-2 pi i e / N), after the Stockham entries (twiddle_count_key)
        for (int e = 0; e < pl.n; ++e) {
            const double ang = -2.0 * M_PI * (double)e / (double)pl.n;
            host.push_back(std::cos(ang));
            host.push_back(std::sin(ang));
        }
    }
    void* d = nullptr;
    if (prec == PREC_F64) {
        HIP_TRY(hipMalloc(&d, host.size() * sizeof(double)));
        RC(copy_sync(d, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, hipStreamPerThread));
    } else {
        std::vector<float> f(host.begin(), host.end());
        HIP_TRY(hipMalloc(&d, f.size() * sizeof(float)));
        RC(copy_sync(d, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice, hipStreamPerThread));
    }
    g_twiddles[key] = d;
    *out = d;
    return 0;
}

__global__ void fill_int_kernel(int* p, int n, int v) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}

__global__ void fill_float_kernel(float* out, long long n, float v) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = v;
}
__global__ void copy_float_kernel(const float* in, float* out, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = in[i];
}

// Weighted GS, off the iteration path. Support statistics of one hologram per
// workgroup, in a fixed order: the number of support pixels (device target
// > 0: the uint8 target, or the amplitude of a float32 one) and, with a weight
// plane w in the same blocked layout, the sum of w over the support; *bad is
// raised by a support weight that is not positive and finite.
constexpr int kGswThreads = 1024;
template <typename TT>
__global__ void __launch_bounds__(kGswThreads) gsw_support_kernel(const TT* tgt, const float* w, long long holo,
                                                                   double* count, double* sum, int* bad) {
    const int b = blockIdx.x;
    const TT* t = tgt + (long long)b * holo;
    double mx = 0.0, n = 0.0, sw = 0.0;
    int flag = 0;
    for (long long i = threadIdx.x; i < holo; i += kGswThreads) {
        if (!(t[i] > (TT)0)) continue;
        n += 1.0;
        if (w) {
            const float g = w[(long long)b * holo + i];
            if (!(g > 0.f && g <= 3.40282347e38f)) flag = 1;
            sw += (double)g;
        }
    }
    block_reduce_stats<kGswThreads>(mx, n, sw);
    if (flag && bad) atomicOr(bad, 1);
    if (threadIdx.x == 0) {
        if (count) count[b] = n;
        if (sum) sum[b] = sw;
    }
}
// weights as read back: g count / sum g on the support (mean 1), exactly 1 off it
template <typename TT>
__global__ void gsw_normalize_kernel(const TT* tgt, const float* g, float* out, long long holo, long long n,
                                     const double* count, const double* sum) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / holo;
        out[i] = tgt[i] > (TT)0 ? (float)((double)g[i] * (count[b] / sum[b])) : 1.f;
    }
}

// MRAF, off the iteration path. Region constants of one hologram per workgroup,
// in a fixed order (a rerun repeats bit for bit): over the signal region R > 0
// the pixel count, sum a_T^2 (a_T as the iteration kernels form it), max T,
// sum T^2 and the count of pixels with T > 0. tgt and region share one layout.
template <int TT, typename TV>
__global__ void __launch_bounds__(kGswThreads) mraf_region_kernel(const TV* tgt, const uint8_t* region, long long holo,
                                                                   int B, double* rows) {
    const int b = blockIdx.x;
    const TV* t = tgt + (long long)b * holo;
    const uint8_t* r = region + (long long)b * holo;
    double mx = 0.0, n = 0.0, sa2 = 0.0, st2 = 0.0, np = 0.0, z0 = 0.0;
    for (long long i = threadIdx.x; i < holo; i += kGswThreads) {
        if (r[i] == 0) continue;
        const float tf = (float)t[i];
        const double a = (double)TgtLoad<TT>::amp(tf), td = (double)tf;
        n += 1.0;
        sa2 += a * a;
        mx = fmax(mx, td);
        st2 += td * td;
        if (tf > 0.f) np += 1.0;
    }
    block_reduce_stats<kGswThreads>(mx, n, sa2);
    lds_barrier();
    block_reduce_stats<kGswThreads>(z0, st2, np);
    if (threadIdx.x == 0) {
        rows[MRAF_N * B + b] = n;
        rows[MRAF_SUM_A2 * B + b] = sa2;
        rows[MRAF_MAX_T * B + b] = mx;
        rows[MRAF_SUM_T2 * B + b] = st2;
        rows[MRAF_NPOS * B + b] = np;
    }
}
// sum a_in^2 (one workgroup, fixed order)
__global__ void __launch_bounds__(kGswThreads) mraf_ain_kernel(const float* ain, long long holo, double* out) {
    double z0 = 0.0, s = 0.0, z1 = 0.0;
    for (long long i = threadIdx.x; i < holo; i += kGswThreads) s += (double)ain[i] * (double)ain[i];
    block_reduce_stats<kGswThreads>(z0, s, z1);
    if (threadIdx.x == 0) *out = s;
}
// what follows from the reductions and m: 1 / N_sr, P = S sum a_in^2 (S^2 for
// uniform light), and behind the region plane (kernels.hpp, mraf_scales) m kappa
// with kappa = sqrt(P / sum_sr a_T^2), and 1 - m
__global__ void mraf_scale_kernel(double* rows, double* scales, int B, double m, double holo, int has_ain) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double power = holo * (has_ain ? rows[kMrafRows * B] : holo);
    rows[MRAF_INV_N * B + b] = 1.0 / rows[MRAF_N * B + b];
    rows[MRAF_POWER * B + b] = power;
    scales[b] = m * sqrt(power / rows[MRAF_SUM_A2 * B + b]);
    scales[B + b] = 1.0 - m;
}

// plog: panel width log2 of the destination / source blocked layout
// (layout_x_log2(lid): X buffers, the target; layout_y_log2(lid): Y, the GD field)
// float / complex64 planes of 64-multiple sides move through LDS tiles
// (layout_kernels.hpp, tile_relayout_kernel), byte planes element-wise
template <int PLOG, typename V>
void relayout_launch(const V* in, V* out, long long n, int H, int W, bool to_blocked, hipStream_t st) {
    if constexpr (sizeof(V) == 4 || sizeof(V) == 8) {
        if (H % 64 == 0 && W % 64 == 0) {
            const dim3 grid(W / 64, H / 64, (unsigned)(n / ((long long)H * W)));
            if (to_blocked)
                hipLaunchKernelGGL((tile_relayout_kernel<V, PLOG, true>), grid, dim3(256), 0, st, in, out, H, W);
            else
                hipLaunchKernelGGL((tile_relayout_kernel<V, PLOG, false>), grid, dim3(256), 0, st, in, out, H, W);
            return;
        }
    }
    const int grid = (int)std::min<long long>(8192, (n + 255) / 256);
    if (to_blocked)
        hipLaunchKernelGGL((relayout_kernel<V, true, PLOG>), dim3(grid), dim3(256), 0, st, in, out, n, H, W);
    else
        hipLaunchKernelGGL((relayout_kernel<V, false, PLOG>), dim3(grid), dim3(256), 0, st, in, out, n, H, W);
}
template <typename V>
int relayout(int plog, const V* in, V* out, long long n, int H, int W, bool to_blocked, hipStream_t st) {
    switch (plog) {
        case 1: relayout_launch<1>(in, out, n, H, W, to_blocked, st); break;
        case 2: relayout_launch<2>(in, out, n, H, W, to_blocked, st); break;
        case 3: relayout_launch<3>(in, out, n, H, W, to_blocked, st); break;
        case 4: relayout_launch<4>(in, out, n, H, W, to_blocked, st); break;
        default: return fail(SLM_ERR_UNSUPPORTED, "no relayout for panel log2 %d", plog);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// Column tile width. With the blocked state layout a 4-column panel is one
// contiguous run, so a 4-column tile moves whole lines (2-column tiles, which
// rely on the partner tile fetching the other half of each line through the
// same XCD's L2, measured slower at 4096). SLM_COL_CW overrides.
int pick_cw(int ck, int W) {
    if (const char* s = std::getenv("SLM_COL_CW")) {
        const int cw = std::atoi(s);
        if (col_fn(ck, cw, COL_GS_MAIN, TGT_AMP, PREC_F32) && W % cw == 0) return cw;
    }
    // narrow plans (a single small image) take 2-column tiles: twice the
    // workgroups per CU, the partner tile reads the other half of each line
    // through the same XCD's L2 (measured 13.0 -> 10.7 us per 1024^2 pass)
    if (kPlans[ck].variant == 1 && W % 2 == 0 && col_fn(ck, 2, COL_GS_MAIN, TGT_AMP, PREC_F32)) return 2;
    // first tile (in this order) whose complex64 LDS leaves room for two
    // workgroups per CU; 2-column tiles only with >= 8 waves (long columns)
    for (int cw : {4, 8, 16, 2}) {
        if (W % cw || !col_fn(ck, cw, COL_GS_MAIN, TGT_AMP, PREC_F32)) continue;
        const long long lds = (long long)lds_line(kPlans[ck].n) * cw * 8;
        const int threads = cw * (kPlans[ck].n / kPlans[ck].e);
        if (lds <= 80 * 1024 && (cw != 2 || threads >= 512)) return cw;
    }
    for (int cw : {4, 8, 16, 2})
        if (W % cw == 0 && col_fn(ck, cw, COL_GS_MAIN, TGT_AMP, PREC_F32)) return cw;
    return 0;
}

// Radix plan of one axis: the narrow variant (half the elements per thread)
// when the wide one would leave fewer than 4 waves per SIMD on the chip
// (e.g. a single 1024^2 hologram), else the wide one. $SLM_PLAN=wide|narrow
// forces a variant where it exists.
// Float32 transforms take the narrow plan where the wide one holds more than
// 16 elements per thread (4096: 32 spill).
int pick_plan(int n, long long elems, int prec, bool row = false) {
    const int wide = plan_index(n, 0), narrow = plan_index(n, 1);
    if (narrow < 0) return wide;
    if (const char* s = std::getenv(row ? "SLM_ROW_PLAN" : "SLM_COL_PLAN")) {
        if (!std::strcmp(s, "wide")) return wide;
        if (!std::strcmp(s, "narrow")) return narrow;
    }
    if (const char* s = std::getenv("SLM_PLAN")) {
        if (!std::strcmp(s, "wide")) return wide;
        if (!std::strcmp(s, "narrow")) return narrow;
    }
    if (prec == PREC_F32 && kPlans[wide].e > 16 && kPlans[narrow].e <= 16) return narrow;
    // 2048-point rows: the 4-pass E = 8 plan beats the 3-pass E = 16 one at
    // every batch (gpurun_out/exp19: 1 image 26.7 -> 21.7 us, 16 images
    // 405 -> 292 us per row launch); columns keep the rule below
    if (row && prec == PREC_F32 && n == 2048) return narrow;
    // float64 4096-point rows: the 3-pass E = 16 plan (one row per workgroup)
    // beats the 4-pass E = 32 one (gpurun_out/s5: 4096^2 row pass 180 -> 142 us,
    // columns keep the wide plan: 200 vs 238 us)
    if (row && prec == PREC_F64 && n == 4096) return narrow;
    const long long waves = elems / kPlans[wide].e / 64;
    return waves < 4LL * 1024 ? narrow : wide;
}

// Every kernel of a run is launched through here. In a timed run
// (slm_plan_run_timed) each launch carries its own start/stop events
// (hipExtLaunchKernelGGL): the dispatch packet stamps them, so they bracket the
// kernel's execution alone, as rocprofv3's kernel trace does, with no marker
// packets between kernels.
template <typename F, typename... Args>
int launch(const PlanState& s, int cls, F fn, dim3 grid, dim3 block, Args... args) {
    if (s.timing) {
        std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
        RC(s.timing->next(cls, &ev));
        hipExtLaunchKernelGGL(fn, grid, block, 0, s.stream, ev->first, ev->second, 0, args...);
    } else {
        hipLaunchKernelGGL(fn, grid, block, 0, s.stream, args...);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// One workgroup per tile (kernels.hpp, tile_loop).
int tile_grid(long long tiles, int* grid) {
    if (tiles > INT_MAX) return fail(SLM_ERR_ARG, "%lld tiles exceed one launch", tiles);
    *grid = (int)tiles;
    return 0;
}

StatsParams stats_params(const PlanState& s, double tol) {
    StatsParams p{};
    p.partials = s.partials;
    p.stats = s.stats;
    p.stop_iter = s.stop;
    p.norm = s.norm;
    p.sum_t2 = s.sum_t2;
    p.inv_s = 1.0 / (double)s.holo;
    p.tol = tol;
    p.max_loops = s.max_loops;
    p.nwg = s.nwg;
    if (s.algo == SLM_ALGO_MRAF) {  // the error over the signal region, and the efficiency
        p.norm = s.mraf + MRAF_MAX_T * s.B;
        p.sum_t2 = s.mraf + MRAF_SUM_T2 * s.B;
        p.inv_n = s.mraf + MRAF_INV_N * s.B;
        p.power = s.mraf + MRAF_POWER * s.B;
        p.eff = s.eff;
    }
    return p;
}

// GD iteration structures (FusedEngine::gd_mode, $SLM_GD_MODE at plan creation)
enum GdMode : int { GD_AUTO = 0, GD_LIN = 1, GD_FUSED = 2, GD_TWO = 3 };

struct FusedEngine : Engine {
    int dev_tt = 1;  // TgtType of the device target buffer: tt, or TGT_AMP for float32 GS targets
    int cw = 4, col_threads = 0, row_threads = 0, rpw = 0;
    int row_key = -1, col_key = -1;  // radix plans (kPlans) of the row / column transforms
    int lid = -1;                    // blocked layout pair (LayoutId), fixed at the first configure
    // row kernels' precision: s.prec, unless $SLM_ROW_PRECISION (f32 / f64, read at
    // creation) splits the two kernels (A/B of float64 in one pass only)
    int prec_row = PREC_F32, prec_row_force = -1;
    // write-through field stores per pass ($SLM_WT=0/1 forces both). Measured
    // (float32): write-through is faster for single images up to 1024^2 (no
    // dirty L2 at the kernel boundary); columns of 2048+ (2-column tiles:
    // half lines, merged in L2 before write-back) and rows of 4096 or of
    // launches with 32M+ elements are faster written back (4096^2 column pass
    // 129 -> 105 us, 4 x 4096^2 row pass 548 -> 480 us).
    int wt_col = 1, wt_row = 1;
    unsigned long long* trace_col = nullptr;  // SLM_TRACE diagnostics ($SLM_TRACE_BUF=1)
    unsigned long long* trace_row = nullptr;
    const void* tw_row = nullptr;
    const void* tw_col = nullptr;
    float2 *xb = nullptr, *y = nullptr, *field = nullptr;  // with s.xa: the X pair, Y, the GD field (blocked)
    // COL_GD_FUSED grid max-barrier: [B][max_loops] results, then [B][max_loops][nwg]
    // workgroup slots (preset to kUnset per run), and a fault flag
    double* gsync = nullptr;
    int* gfault = nullptr;
    int gd_fuse = 1;  // one-launch column side allowed ($SLM_GD_FUSE=0 at creation; cleared by a grid fault)
    // GD iteration structure ($SLM_GD_MODE=auto|lin|fused|two at plan creation):
    // GD_AUTO (default): GD_FUSED where the column grid is resident at once
    //   (float32, unchecked runs), else GD_TWO;
    // GD_FUSED: one column launch -- forward transform, grid max-barrier,
    //   gradient and inverse transform on F in registers -- plus the row launch;
    // GD_TWO: statistics launch + gradient launch that recomputes F;
    // GD_LIN: column launch stores both inverse-transformed terms (Y, Y2), the
    //   row launch folds the maxima and combines them (no in-launch wait at all).
    int gd_mode = GD_AUTO;
    int skip_wg_plus1 = 0;       // $SLM_GD_FAULT_TEST: fused-path fault injection (tests)
    int gd_recoveries = 0;       // runs redone on the two-launch path after a grid fault
    bool fused_pending = false;  // a one-launch GD run is queued and its fault flag not read yet
    float2* y2 = nullptr;        // GD_LIN: column-inverse transform of mask F T
    double* gmax = nullptr;      // GD_LIN: [B][max_loops][nwg] column-workgroup maxima of |F|^2
    // weighted GS: the running weight plane g (layout X, updated in place by
    // COL_GSW_MAIN), per hologram the support size and the support sums of the
    // host-set weights (s.weights0) and of the plane being read back, a flag word
    float* gw = nullptr;
    double *gsw_n = nullptr, *gsw_sum0 = nullptr, *gsw_tmp = nullptr;
    int* gsw_bad = nullptr;

    ~FusedEngine() override {
        for (void* ptr : {(void*)xb, (void*)y, (void*)field, (void*)gsync, (void*)gfault, (void*)y2, (void*)gmax,
                          (void*)trace_col, (void*)trace_row, (void*)gw, (void*)gsw_n, (void*)gsw_sum0,
                          (void*)gsw_tmp, (void*)gsw_bad})
            if (ptr) (void)hipFree(ptr);
    }

    // Radix plans, tiles and twiddle tables for one arithmetic precision
    // (fused_create, slm_plan_set_precision).
    int set_precision(PlanState& s, int prec) override {
        const long long elems = (long long)s.B * s.holo;
        const int prow = prec_row_force >= 0 ? prec_row_force : prec;
        const int rk = pick_plan(s.W, elems, prow, true);
        const int ck = pick_plan(s.H, elems, prec);
        const int w = pick_cw(ck, s.W);
        if (!w) return fail(SLM_ERR_UNSUPPORTED, "no column tiling for %dx%d", s.H, s.W);
        const void *tr = nullptr, *tc = nullptr;
        RC(get_twiddles(rk, prow, &tr));
        RC(get_twiddles(ck, prec, &tc));
        // layout pair: the narrow one where both transforms have kernels for it
        // ($SLM_LAYOUT=default forces the default pair; GS 1024^2 20.9 -> 19.6 us
        // per iteration at r02). Device buffers are laid out at upload, so a plan
        // keeps the pair it was created with.
        int l = LAYOUT_DEFAULT;
        // GD takes the narrow pair too since its column side became one launch
        // (GD 1024^2 fused column pass 14.55 -> 13.66 us, 25.97 -> 25.19 us per
        // iteration, bitwise the same phases: gpurun_out/s11; $SLM_GD_LAYOUT=default
        // keeps the default pair for GD only)
        const char* gl = std::getenv("SLM_GD_LAYOUT");
        const bool algo_ok = gs_like(s.algo) || !(gl && !std::strcmp(gl, "default"));
        const bool narrow_ok = algo_ok && row_fn(rk, ROW_GS_MAIN, prow, LAYOUT_NARROW) &&
                               col_fn(ck, w, COL_GS_MAIN, TGT_AMP, prec, LAYOUT_NARROW);
        const char* ls = std::getenv("SLM_LAYOUT");
        if (narrow_ok && !(ls && !std::strcmp(ls, "default"))) l = LAYOUT_NARROW;
        if (lid >= 0 && l != lid) {
            if (lid == LAYOUT_NARROW && !narrow_ok)
                return fail(SLM_ERR_UNSUPPORTED, "precision change leaves the plan's layout unsupported");
            l = lid;
        }
        lid = l;
        s.prec = prec;
        prec_row = prow;
        row_key = rk;
        col_key = ck;
        cw = w;
        s.nwg = s.W / w;
        col_threads = slm::col_threads(ck, w);
        row_threads = slm::row_threads(rk, prow);
        rpw = row_rpw(rk, prow);
        tw_row = tr;
        tw_col = tc;
        return 0;
    }

    RowParams row_params(const PlanState& s) const {
        RowParams r{};
        r.ain = s.ain;
        r.phase_in = s.phase_in;
        r.phase_out = s.phase_out;
        r.field = field;
        r.field_src = field;
        r.lr = s.lr;
        r.stop_iter = s.stop;
        r.W = s.W;
        r.H = s.H;
        r.holo = s.holo;
        r.inv_s = (float)(1.0 / (double)s.holo);
        r.tw = tw_row;
        r.wt = wt_row;
        r.trace = trace_row;
        return r;
    }

    ColParams col_params(const PlanState& s) const {
        ColParams c{};
        c.tgt = s.tgt;
        c.partials = s.partials;
        c.stop_iter = s.stop;
        c.norm = s.normf;
        c.max_loops = s.max_loops;
        c.W = s.W;
        c.nwg = s.nwg;
        c.holo = s.holo;
        c.stat_k = std::ldexp(1.0f, -2 * (int)std::ceil(std::log2((double)s.holo)));
        c.tw = tw_col;
        c.wt = wt_col;
        c.trace = trace_col;
        return c;
    }

    int launch_row(const PlanState& s, int mode, const RowParams& rp, int cls) {
        RowFn fn = row_fn(row_key, mode, prec_row, lid);
        if (!fn) return fail(SLM_ERR_UNSUPPORTED, "no row kernel for width %d mode %d", s.W, mode);
        RowParams r = rp;
        r.B = s.B;
        r.ntile = s.H / rpw;
        int grid = 0;
        RC(tile_grid((long long)r.ntile * s.B, &grid));
        return launch(s, cls, fn, dim3(grid), dim3(row_threads), r);
    }

    int launch_col(const PlanState& s, int mode, const ColParams& cp, int cls) {
        const int tt = (mode == COL_EXPECTED || mode == COL_FFT_FWD || mode == COL_FFT_INV) ? TGT_F32 : dev_tt;
        ColFn fn = col_fn(col_key, cw, mode, tt, s.prec, lid);
        if (!fn) return fail(SLM_ERR_UNSUPPORTED, "no column kernel for height %d cw %d mode %d", s.H, cw, mode);
        ColParams c = cp;
        c.B = s.B;
        int grid = 0;
        RC(tile_grid((long long)s.nwg * s.B, &grid));
        return launch(s, cls, fn, dim3(grid), dim3(col_threads), c);
    }

    // the expected output E written by the GS column pass in layout Y (e_blk) ->
    // the row-major e_out (LDS-tiled transpose; one launch for the batch)
    int unblock_expected(const PlanState& s, const float* e_blk) {
        const dim3 grid(s.W / 64, s.H / 64, s.B);
        switch (layout_y_log2(lid)) {
            case 1: return launch(s, SLM_KERNEL_OTHER, tile_relayout_kernel<float, 1, false>, grid, dim3(256), e_blk, s.e_out, s.H, s.W);
            case 2: return launch(s, SLM_KERNEL_OTHER, tile_relayout_kernel<float, 2, false>, grid, dim3(256), e_blk, s.e_out, s.H, s.W);
            case 3: return launch(s, SLM_KERNEL_OTHER, tile_relayout_kernel<float, 3, false>, grid, dim3(256), e_blk, s.e_out, s.H, s.W);
            case 4: return launch(s, SLM_KERNEL_OTHER, tile_relayout_kernel<float, 4, false>, grid, dim3(256), e_blk, s.e_out, s.H, s.W);
            default: return fail(SLM_ERR_UNSUPPORTED, "no unblock kernel for panel log2 %d", layout_y_log2(lid));
        }
    }

    // expected output |C|^2 (src/algorithms.py:36) of GD (and the intensity
    // helper): a forward column pass writes it in layout Y into the free Y buffer
    // (every reader of Y precedes this on the stream), then the tiled unblock
    int launch_expected(const PlanState& s, ColParams cp) {
        cp.e_blk = reinterpret_cast<float*>(y);
        RC(launch_col(s, COL_EXPECTED, cp, SLM_KERNEL_OTHER));
        return unblock_expected(s, reinterpret_cast<const float*>(y));
    }

    int launch_finalize(const PlanState& s, double tol, int iter) {
        StatsParams p = stats_params(s, tol);
        p.iter = iter;
        return launch(s, SLM_KERNEL_OTHER, stats_finalize_kernel, dim3(s.B), dim3(256), p);
    }

    int enqueue_gs(const PlanState& s, int loops, double tol, int checked, bool phase_set) {
        RowParams rp = row_params(s);
        ColParams cp = col_params(s);
        cp.loops = loops;
        rp.checked = cp.checked = checked;
        // weighted GS: the same iteration with COL_GSW_MAIN as its column pass.
        // Every run starts from the host-set weights (never written by a run) or ones.
        const bool gsw = s.algo == SLM_ALGO_GSW;
        const bool mraf = s.algo == SLM_ALGO_MRAF;
        const int col_mode = gsw ? COL_GSW_MAIN : mraf ? COL_MRAF_MAIN : COL_GS_MAIN;
        if (mraf) {  // region and scales live in device memory: a captured run follows set_region / set_mixing
            cp.region = s.region;
        }
        if (gsw) {
            const long long n = (long long)s.B * s.holo;
            const int grid = (int)std::min<long long>(8192, (n + 255) / 256);
            if (s.weights_set)
                RC(launch(s, SLM_KERNEL_OTHER, copy_float_kernel, dim3(grid), dim3(256), (const float*)s.weights0, gw, n));
            else
                RC(launch(s, SLM_KERNEL_OTHER, fill_float_kernel, dim3(grid), dim3(256), gw, n, 1.f));
            cp.gw = gw;
            cp.gsw_n = gsw_n;
            cp.gsw_sum0 = s.weights_set ? gsw_sum0 : gsw_n;
            cp.fb = s.feedback;
        }
        // setup: X0 = rowFFT(a_in A0/|A0|), A0 = ifft2(sqrt T) (src/algorithms.py:14-27),
        // or the warm start B = a_in exp(i phi).
        if (phase_set) {
            rp.out = s.xa;
            RC(launch_row(s, ROW_PHASE_FWD, rp, SLM_KERNEL_OTHER));
        } else {
            cp.out = y;
            RC(launch_col(s, COL_REAL_INV, cp, SLM_KERNEL_OTHER));
            rp.in = y;
            rp.out = s.xa;
            rp.iter = -1;
            RC(launch_row(s, ROW_GS_MAIN, rp, SLM_KERNEL_OTHER));
        }
        // expected_outcome = |C|^2 of the last iteration (src/algorithms.py:36): the
        // column pass of the last iteration (of every iteration in a checked run,
        // where the last is not known in advance; a stopped hologram's later passes
        // leave it untouched) stores it in layout Y into phase_out, free until the
        // phase extraction below
        float* const e_blk = s.phase_out;
        for (int i = 0; i < loops; ++i) {
            cp.in = s.xa;
            cp.out = y;
            cp.iter = i;
            cp.e_blk = (checked || i + 1 == loops) ? e_blk : nullptr;
            RC(launch_col(s, col_mode, cp, SLM_KERNEL_COL_MAIN));
            if (checked) RC(launch_finalize(s, tol, i));
            if (i + 1 < loops) {
                rp.in = y;
                rp.out = s.xa;
                rp.iter = i;
                RC(launch_row(s, ROW_GS_MAIN, rp, SLM_KERNEL_ROW_MAIN));
            }
        }
        RC(unblock_expected(s, e_blk));
        // hologram = np.angle(A) (src/algorithms.py:48)
        rp.in = y;
        RC(launch_row(s, ROW_GS_PHASE, rp, SLM_KERNEL_OTHER));
        return 0;
    }

    // GD column side in one launch (COL_GD_FUSED, a grid barrier for the global
    // max of |F|^2) when it is safe and built: unchecked runs (no workgroup leaves
    // early), float32 kernels, and a grid whose workgroups are all resident at once
    // (occupancy x CUs, one tile per workgroup). Otherwise the statistics pass and
    // the gradient pass run as two launches. $SLM_GD_FUSE=0 forces two launches.
    ColFn gd_fused_fn(const PlanState& s, int checked) const {
        if (!gd_fuse || !gsync || checked) return nullptr;
        if (gd_mode != GD_AUTO && gd_mode != GD_FUSED) return nullptr;
        if (2LL * s.B * s.max_loops * (1 + s.nwg) > INT_MAX) return nullptr;  // slot area: two launches instead
        ColFn fn = col_fn(col_key, cw, COL_GD_FUSED, s.tt, s.prec, lid);
        if (!fn) return nullptr;
        int dev = 0, cus = 0, per_cu = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)fn, col_threads, 0) != hipSuccess)
            return nullptr;
        return (long long)s.nwg * s.B <= (long long)per_cu * cus ? fn : nullptr;
    }

    int enqueue_gd(const PlanState& s, int loops, double tol, int checked, float wa, bool field_set) {
        RowParams rp = row_params(s);
        ColParams cp = col_params(s);
        cp.loops = loops;
        rp.checked = cp.checked = checked;
        cp.wa = wa;
        // setup (make_initial_guess, src/algorithms.py:115-158): host-provided field
        // or the "fourier" guess a_in exp(i angle(ifft2(sqrt T))).
        if (field_set) {
            rp.out = s.xa;
            rp.field_src = s.field0;
            RC(launch_row(s, ROW_GD_INIT_FIELD, rp, SLM_KERNEL_OTHER));
        } else {
            cp.out = y;
            RC(launch_col(s, COL_REAL_INV, cp, SLM_KERNEL_OTHER));
            rp.in = y;
            rp.out = s.xa;
            RC(launch_row(s, ROW_GD_INIT_Y, rp, SLM_KERNEL_OTHER));
        }
        const bool lin = gd_mode == GD_LIN;
        const bool fused = !lin && gd_fused_fn(s, checked) != nullptr;
        if (fused) {
            cp.gresult = gsync;
            cp.gslots = gsync + (long long)s.B * s.max_loops;
            cp.fault = gfault;
            cp.skip_wg_plus1 = skip_wg_plus1;
            // every result and slot word to kUnset (all bits set) before the run
            // (gd_fused_fn keeps the slot area within INT_MAX words)
            const long long words = 2LL * s.B * s.max_loops * (1 + s.nwg);
            RC(launch(s, SLM_KERNEL_OTHER, fill_int_kernel, dim3((int)std::min<long long>(65535, (words + 255) / 256)),
                      dim3(256), (int*)gsync, (int)words, -1));
        }
        for (int i = 0; i < loops; ++i) {
            float2* xi = (i & 1) ? xb : s.xa;
            float2* xn = (i & 1) ? s.xa : xb;
            // iteration 0 reads a host-set field from field0 (kept intact for reruns)
            rp.field_src = (i == 0 && field_set) ? s.field0 : field;
            cp.in = xi;
            cp.iter = i;
            cp.out = y;
            if (lin) {
                cp.out2 = y2;
                cp.gmax = gmax;
                RC(launch_col(s, COL_GD_LIN, cp, SLM_KERNEL_COL_MAIN));
                if (checked) RC(launch_finalize(s, tol, i));
                rp.in = y;
                rp.in2 = y2;
                rp.gmax = gmax;
                rp.norm = s.normf;
                rp.nwg_col = s.nwg;
                rp.max_loops = s.max_loops;
                rp.out = xn;
                rp.iter = i;
                RC(launch_row(s, ROW_GD_LIN, rp, SLM_KERNEL_ROW_MAIN));
                continue;
            }
            if (fused) {
                RC(launch_col(s, COL_GD_FUSED, cp, SLM_KERNEL_COL_MAIN));
            } else {
                RC(launch_col(s, COL_GD_STATS, cp, SLM_KERNEL_GD_STATS));
                if (checked) RC(launch_finalize(s, tol, i));
                RC(launch_col(s, COL_GD_GRAD, cp, SLM_KERNEL_COL_MAIN));
            }
            rp.in = y;
            rp.out = xn;
            rp.iter = i;
            RC(launch_row(s, ROW_GD_MAIN, rp, SLM_KERNEL_ROW_MAIN));
        }
        {
            const long long n = (long long)s.B * s.holo;
            const int grid = (int)std::min<long long>(4096, (n + 255) / 256);
            const int yl = layout_y_log2(lid);
            auto fk = yl == 1 ? field_phase_kernel<1>
                      : yl == 3 ? field_phase_kernel<3> : yl == 4 ? field_phase_kernel<4> : field_phase_kernel<2>;
            RC(launch(s, SLM_KERNEL_OTHER, fk, dim3(grid), dim3(256), (const float2*)field, s.phase_out, n, s.H, s.W));
        }
        cp.in = s.xa;
        cp.in_alt = xb;
        RC(launch_expected(s, cp));
        return 0;
    }

    int enqueue(PlanState& s, int loops, double tol, int checked, float wa, bool phase_set, bool field_set) override {
        return gs_like(s.algo) ? enqueue_gs(s, loops, tol, checked, phase_set)
                                     : enqueue_gd(s, loops, tol, checked, wa, field_set);
    }

    void queued(const PlanState& s, int checked) override {
        if (gfault && gd_fused_fn(s, checked)) fused_pending = true;
    }
    bool unsettled() const override { return fused_pending; }
    int recoveries() const override { return gd_recoveries; }

    // A grid wait of COL_GD_FUSED that gave up (kernels.hpp, wait_set) leaves a
    // fault flag: that run's results are invalid. Read it after the stream has
    // drained; on a fault the plan gives up its one-launch column side for good
    // (its workgroups were not co-resident: other work shares the device) and
    // the caller redoes the same run, now on the two-launch path (the run's
    // inputs -- target, field0, learning rates -- are untouched by a run; the
    // captured graph holds the fused kernel).
    int settle(PlanState& s, bool* redo) override {
        *redo = false;
        if (!gfault) return 0;
        fused_pending = false;  // the caller drained the stream: the flag below covers every queued run
        int f = 0;
        RC(copy_sync(&f, gfault, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        if (!f) return 0;
        HIP_TRY(hipMemsetAsync(gfault, 0, sizeof(int), s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        *redo = true;
        gd_fuse = 0;
        gd_recoveries += 1;
        return 0;
    }

    void* target_stage(const PlanState& s) override { return s.e_out; }

    // support statistics of weight plane w (nullptr: the support size alone)
    int gsw_support(PlanState& s, const float* w, double* count, double* sum, int* bad) {
        if (s.tt == SLM_TGT_U8)
            hipLaunchKernelGGL(gsw_support_kernel<uint8_t>, dim3(s.B), dim3(kGswThreads), 0, s.stream,
                               (const uint8_t*)s.tgt, w, s.holo, count, sum, bad);
        else
            hipLaunchKernelGGL(gsw_support_kernel<float>, dim3(s.B), dim3(kGswThreads), 0, s.stream,
                               (const float*)s.tgt, w, s.holo, count, sum, bad);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    int land_target(PlanState& s, const void* staged) override {
        RC(land_target_layout(s, staged));
        if (s.algo == SLM_ALGO_GSW) RC(gsw_support(s, nullptr, gsw_n, nullptr, nullptr));
        return 0;
    }

    // host uint8 [B][H][W] -> s.region (layout X, as a uint8 target)
    int land_region(PlanState& s, const uint8_t* region) override {
        const long long n = (long long)s.B * s.holo;
        uint8_t* const stage = reinterpret_cast<uint8_t*>(y);  // scratch between runs
        HIP_TRY(hipMemcpyAsync(stage, region, (size_t)n, hipMemcpyHostToDevice, s.stream));
        return land_region_dev(s, stage);
    }

    // the same from a row-major plane on the device
    int land_region_dev(PlanState& s, const uint8_t* region) override {
        return relayout(layout_x_log2(lid), region, s.region, (long long)s.B * s.holo, s.H, s.W, true, s.stream);
    }

    int mraf_refresh(PlanState& s, bool reduce, int* bad_holo) override {
        if (bad_holo) *bad_holo = -1;
        if (reduce) {
            if (s.tt == SLM_TGT_U8)
                hipLaunchKernelGGL((mraf_region_kernel<TGT_U8, uint8_t>), dim3(s.B), dim3(kGswThreads), 0, s.stream,
                                   (const uint8_t*)s.tgt, (const uint8_t*)s.region, s.holo, s.B, s.mraf);
            else
                hipLaunchKernelGGL((mraf_region_kernel<TGT_F32, float>), dim3(s.B), dim3(kGswThreads), 0, s.stream,
                                   (const float*)s.tgt, (const uint8_t*)s.region, s.holo, s.B, s.mraf);
            HIP_TRY(hipGetLastError());
            if (s.has_ain) {
                hipLaunchKernelGGL(mraf_ain_kernel, dim3(1), dim3(kGswThreads), 0, s.stream, (const float*)s.ain, s.holo,
                                   s.mraf + (long long)kMrafRows * s.B);
                HIP_TRY(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(mraf_scale_kernel, dim3((s.B + 255) / 256), dim3(256), 0, s.stream, s.mraf,
                           const_cast<double*>(mraf_scales(s.region, s.B, s.holo)), s.B, (double)s.mixing, (double)s.holo, s.has_ain);
        HIP_TRY(hipGetLastError());
        if (!bad_holo) return 0;  // a sequence: checked on the host up front, enqueued only
        if (reduce) {
            std::vector<double> npos(s.B);
            RC(copy_sync(npos.data(), s.mraf + MRAF_NPOS * s.B, (size_t)s.B * sizeof(double), hipMemcpyDeviceToHost,
                         s.stream));
            for (int b = 0; b < s.B && *bad_holo < 0; ++b)
                if (!(npos[b] > 0.0)) *bad_holo = b;
        } else {
            HIP_TRY(hipStreamSynchronize(s.stream));
        }
        return 0;
    }

    // host float32 [B][H][W] -> s.weights0 (layout X); *bad: an entry on the
    // support is not positive and finite
    int land_weights(PlanState& s, const float* w, bool* bad) override {
        const long long n = (long long)s.B * s.holo;
        float* const stage = reinterpret_cast<float*>(y);  // scratch between runs
        HIP_TRY(hipMemcpyAsync(stage, w, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s.stream));
        RC(relayout(layout_x_log2(lid), (const float*)stage, s.weights0, n, s.H, s.W, true, s.stream));
        HIP_TRY(hipMemsetAsync(gsw_bad, 0, sizeof(int), s.stream));
        RC(gsw_support(s, s.weights0, nullptr, gsw_sum0, gsw_bad));
        int f = 0;
        RC(copy_sync(&f, gsw_bad, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        *bad = f != 0;
        return 0;
    }

    // the weights to the host, mean 1 over the support and 1 off it: the host-set
    // plane if `fresh` (set since the last run), else the running plane
    int read_weights(PlanState& s, bool fresh, float* out) override {
        const long long n = (long long)s.B * s.holo;
        const float* src = fresh ? s.weights0 : gw;
        float* const blk = reinterpret_cast<float*>(y);     // scratch between runs
        float* const rm = reinterpret_cast<float*>(s.xa);   // (every run rebuilds X from its start state)
        RC(gsw_support(s, src, gsw_tmp, gsw_tmp + s.B, nullptr));
        const int grid = (int)std::min<long long>(8192, (n + 255) / 256);
        if (s.tt == SLM_TGT_U8)
            hipLaunchKernelGGL(gsw_normalize_kernel<uint8_t>, dim3(grid), dim3(256), 0, s.stream, (const uint8_t*)s.tgt,
                               src, blk, s.holo, n, gsw_tmp, gsw_tmp + s.B);
        else
            hipLaunchKernelGGL(gsw_normalize_kernel<float>, dim3(grid), dim3(256), 0, s.stream, (const float*)s.tgt,
                               src, blk, s.holo, n, gsw_tmp, gsw_tmp + s.B);
        HIP_TRY(hipGetLastError());
        RC(relayout(layout_x_log2(lid), (const float*)blk, rm, n, s.H, s.W, false, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        return copy_sync(out, rm, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s.stream);
    }

    int land_target_layout(PlanState& s, const void* staged) {
        const long long n = (long long)s.B * s.holo;
        const int xl = layout_x_log2(lid);
        if (s.tt == SLM_TGT_U8)
            return relayout(xl, (const uint8_t*)staged, (uint8_t*)s.tgt, n, s.H, s.W, true, s.stream);
        if (dev_tt != TGT_AMP) return relayout(xl, (const float*)staged, (float*)s.tgt, n, s.H, s.W, true, s.stream);
        // a_T = sqrt(T) in the blocked layout (H, W multiples of 64)
        auto k = xl == 1 ? tile_relayout_kernel<float, 1, true, true>
                 : xl == 3 ? tile_relayout_kernel<float, 3, true, true>
                 : xl == 4 ? tile_relayout_kernel<float, 4, true, true> : tile_relayout_kernel<float, 2, true, true>;
        hipLaunchKernelGGL(k, dim3(s.W / 64, s.H / 64, s.B), dim3(256), 0, s.stream, (const float*)staged,
                           (float*)s.tgt, s.H, s.W);
        return 0;
    }

    int land_field(PlanState& s, const float* f) override {
        const long long n = (long long)s.B * s.holo;
        HIP_TRY(hipMemcpyAsync(y, f, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, s.stream));
        return relayout(layout_y_log2(lid), (const float2*)y, s.field0, n, s.H, s.W, true, s.stream);
    }

    int read_field(PlanState& s, bool fresh, float* out) override {
        const long long n = (long long)s.B * s.holo;
        // y is scratch between runs (every run rewrites it before reading it); a
        // field set since the last run is read back from field0 (runs never write it)
        const float2* src = fresh ? s.field0 : field;
        RC(relayout(layout_y_log2(lid), src, y, n, s.H, s.W, false, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        return copy_sync(out, y, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, s.stream);
    }

    int fft2(PlanState& s, const float* in, float* out, int inverse) override {
        const long long n = (long long)s.B * s.holo;
        const size_t bytes = (size_t)n * sizeof(float2);
        const int yl = layout_y_log2(lid);
        hipError_t e = hipMemcpyAsync(y, in, bytes, hipMemcpyHostToDevice, s.stream);
        if (e != hipSuccess) return fail(SLM_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
        RC(relayout(yl, (const float2*)y, s.xa, n, s.H, s.W, true, s.stream));  // row-pass input
        RowParams rp = row_params(s);
        rp.in = s.xa;
        rp.out = y;
        RC(launch_row(s, inverse ? ROW_FFT_INV : ROW_FFT_FWD, rp, SLM_KERNEL_OTHER));
        ColParams cp = col_params(s);
        cp.in = y;
        cp.out = s.xa;
        RC(launch_col(s, inverse ? COL_FFT_INV : COL_FFT_FWD, cp, SLM_KERNEL_OTHER));
        RC(relayout(yl, (const float2*)s.xa, y, n, s.H, s.W, false, s.stream));  // col-pass output
        e = hipStreamSynchronize(s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out, y, bytes, hipMemcpyDeviceToHost, s.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
        if (e != hipSuccess) return fail(SLM_ERR_HIP, "fft2 failed: %s", hipGetErrorString(e));
        return 0;
    }

    int intensity(PlanState& s) override {
        // fft2(exp(1j phase)) = column FFT of the row-transformed field; |.|^2 row-major
        RowParams rp = row_params(s);
        rp.out = s.xa;
        RC(enqueue_stop_reset(s));
        RC(launch_row(s, ROW_PHASE_FWD, rp, SLM_KERNEL_OTHER));
        ColParams cp = col_params(s);
        cp.loops = 1;
        cp.in = s.xa;
        cp.in_alt = s.xa;
        return launch_expected(s, cp);
    }

    long long kernel_bytes(const PlanState& s, int cls) const override {
        const long long px = (long long)s.B * s.holo;
        const long long tb = s.tt == SLM_TGT_U8 ? 1 : 4;
        const long long ab = s.has_ain ? 4 : 0;
        const bool lin = s.algo == SLM_ALGO_GD && gd_mode == GD_LIN;  // + Y2 out (column) / in (row)
        switch (cls) {
            case SLM_KERNEL_COL_MAIN:  // X (GD: F) in, T in, Y out (+ weighted GS: g in and out; MRAF: R in)
                return px * (8 + tb + 8 + (lin ? 8 : 0) + (s.algo == SLM_ALGO_GSW ? 8 : 0) +
                             (s.algo == SLM_ALGO_MRAF ? 1 : 0));
            case SLM_KERNEL_ROW_MAIN:                                 // Y in, X out (+ a_in) (+ field r/w for GD)
                return px * (16 + ab + (s.algo == SLM_ALGO_GD ? 16 : 0) + (lin ? 8 : 0));
            case SLM_KERNEL_GD_STATS: return px * (8 + tb);           // X in, T in
            default: return 0;
        }
    }

    void codes(const PlanState& s, int* col_engine, int* row_engine) const override {
        // mirrors kernels.hpp: kShuffle<K, P> && (CW == 2 | RPW == 2) && one line per thread
        auto shuf = [&](int key, int prec) {
            return (prec == PREC_F32 || gs_like(s.algo)) && key >= 0 && kPlans[key].n == kShufN &&
                   kPlans[key].e == 8;
        };
        *col_engine = shuf(col_key, s.prec) && cw == 2 ? 1 : 0;
        *row_engine = shuf(row_key, prec_row) && rpw == 2 ? 1 : 0;
    }

    void layout(int* x_log2, int* y_log2) const override {
        *x_log2 = layout_x_log2(lid);
        *y_log2 = layout_y_log2(lid);
    }

    void info(const PlanState& s, int info[8]) const override {
        const int v[8] = {cw, s.nwg, col_threads, row_threads, rpw, row_key, col_key, s.prec};
        std::copy(v, v + 8, info);
    }

    int read_trace(PlanState& s, int kernel_class, unsigned long long* out) override {
        unsigned long long* src = kernel_class == SLM_KERNEL_COL_MAIN ? trace_col
                                  : kernel_class == SLM_KERNEL_ROW_MAIN ? trace_row : nullptr;
        if (!src) return Engine::read_trace(s, kernel_class, out);
        const long long n = (long long)s.B * (kernel_class == SLM_KERNEL_COL_MAIN ? s.nwg : s.H / rpw) * kTraceSlots;
        HIP_TRY(hipStreamSynchronize(s.stream));
        return copy_sync(out, src, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream);
    }
};

}  // namespace

int enqueue_stop_reset(PlanState& s) {
    return launch(s, SLM_KERNEL_OTHER, fill_int_kernel, dim3((s.B + 255) / 256), dim3(256), s.stop, s.B, (int)INT_MAX);
}

int enqueue_stats_reduce(PlanState& s, int loops, double tol) {
    return launch(s, SLM_KERNEL_OTHER, stats_reduce_kernel, dim3(loops, s.B), dim3(256), stats_params(s, tol));
}

int fused_create(PlanState& s, Engine** out, int* max_nwg) {
    std::unique_ptr<FusedEngine> f(new FusedEngine());
    // GS keeps a float32 target as its amplitude on the device (land_target)
    // (weighted GS keeps T itself: its error statistics need the exact target, kernels.hpp)
    f->dev_tt = (s.algo == SLM_ALGO_GS && s.tt == SLM_TGT_F32) ? TGT_AMP : s.tt;
    f->wt_col = s.H >= 2048 ? 0 : 1;
    f->wt_row = ((long long)s.B * s.holo >= (32LL << 20) || s.W >= 4096) ? 0 : 1;
    if (const char* e = std::getenv("SLM_WT")) f->wt_col = f->wt_row = std::atoi(e) != 0;
    if (const char* e = std::getenv("SLM_GD_FUSE")) f->gd_fuse = std::atoi(e) != 0;
    if (const char* e = std::getenv("SLM_GD_MODE"))
        f->gd_mode = !std::strcmp(e, "fused") ? GD_FUSED
                     : !std::strcmp(e, "two") ? GD_TWO
                     : !std::strcmp(e, "lin") ? GD_LIN
                                              : GD_AUTO;
    if (!f->gd_fuse && f->gd_mode != GD_LIN) f->gd_mode = GD_TWO;
    if (f->gd_mode == GD_TWO || f->gd_mode == GD_LIN) f->gd_fuse = 0;
    if (const char* e = std::getenv("SLM_GD_FAULT_TEST")) f->skip_wg_plus1 = std::atoi(e);
    if (const char* e = std::getenv("SLM_ROW_PRECISION"))
        f->prec_row_force = (std::strcmp(e, "f64") == 0) ? PREC_F64 : PREC_F32;
    // buffers indexed by column panel / row group hold the finer tiling of both precisions
    const int want = s.prec;
    int nwg = 0, min_rpw = INT_MAX;
    for (int prec : {PREC_F32, PREC_F64}) {
        RC(f->set_precision(s, prec));
        nwg = std::max(nwg, s.nwg);
        min_rpw = std::min(min_rpw, f->rpw);
    }
    RC(f->set_precision(s, want));
    const size_t n = (size_t)s.B * s.holo;
    RC(dev_alloc(&f->y, n * sizeof(float2)));
    if (s.algo == SLM_ALGO_GD) {
        RC(dev_alloc(&f->xb, n * sizeof(float2)));
        RC(dev_alloc(&f->field, n * sizeof(float2)));
        if (f->gd_mode == GD_LIN) {
            RC(dev_alloc(&f->y2, n * sizeof(float2)));
            RC(dev_alloc(&f->gmax, (size_t)s.B * s.max_loops * nwg * sizeof(double)));
        }
        // the one-launch column side needs the whole grid resident: never beyond 8192 workgroups
        if ((f->gd_mode == GD_FUSED || f->gd_mode == GD_AUTO) && (long long)s.B * nwg <= 8192) {
            RC(dev_alloc(&f->gsync, (size_t)s.B * s.max_loops * (1 + nwg) * sizeof(double)));
            RC(dev_alloc(&f->gfault, sizeof(int)));
            HIP_TRY(hipMemsetAsync(f->gfault, 0, sizeof(int), s.stream));
            HIP_TRY(hipStreamSynchronize(s.stream));
        }
    }
    if (s.algo == SLM_ALGO_GSW) {
        RC(dev_alloc(&f->gw, n * sizeof(float)));
        RC(dev_alloc(&f->gsw_n, (size_t)s.B * sizeof(double)));
        RC(dev_alloc(&f->gsw_sum0, (size_t)s.B * sizeof(double)));
        RC(dev_alloc(&f->gsw_tmp, (size_t)2 * s.B * sizeof(double)));
        RC(dev_alloc(&f->gsw_bad, sizeof(int)));
    }
    if (const char* e = std::getenv("SLM_TRACE_BUF"); e && std::atoi(e)) {
        RC(dev_alloc(&f->trace_col, (size_t)s.B * nwg * kTraceSlots * sizeof(unsigned long long)));
        RC(dev_alloc(&f->trace_row, (size_t)s.B * (s.H / min_rpw) * kTraceSlots * sizeof(unsigned long long)));
    }
    *max_nwg = nwg;
    *out = f.release();
    return 0;
}

}  // namespace slm
