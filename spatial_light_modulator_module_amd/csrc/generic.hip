// Any-size engine (generic.hpp): GS / GD iterations on image sides that no
// float32 radix plan covers, in complex float64 like the reference's loop.
//
// Three transform back ends:
//  * radix plans (radix_c128.hpp; the default where both sides have a radix
//    plan, plans.hpp): the mixed-radix launch structure and contract on
//    compile-time Stockham transforms with the line in registers and LDS
//    exchanges. Complex128 on 2^k and 768 sides (reached through
//    $SLM_ENGINE=float64); complex64 for GS at float32 precision where a side
//    is a 13-smooth SLM panel length (600 .. 1920, plans.hpp variant 3) --
//    e.g. 1080 x 1920 -- the float32 engine's numerics on these shapes;
//  * mixed radix (mixed_radix.hpp, mr_inst.hip; the default wherever both
//    sides factor into 2, 3, 5, 7, 11, 13 and fit a workgroup's LDS): the
//    iteration is two fused launches -- column pass (forward transform,
//    projection and statistics, inverse transform) and row pass (inverse,
//    projection, forward) -- O(N log N), hand-written kernels only;
//  * line transforms (any other side, e.g. one with a large prime factor, or
//    $SLM_GENERIC_ENGINE=bluestein): each 2-D transform is a pass of 1-D
//    transforms along the rows, a tiled transpose, a pass along the (former)
//    columns and a transpose back, with element-wise kernels between the
//    transforms. A side with a mixed-radix plan transforms directly; any other
//    side by Bluestein's chirp-z over a mixed-radix length M >= 2n - 1
//    (mr_line_kernel, mr_inst.hip) -- O(N log N) for every length, hand-written
//    kernels only. (Until r05 these sides were products with dense DFT matrices
//    on rocBLAS ZGEMM, O(N^3).)
//
// Numerics follow the reference's float64 path (src/algorithms.py:10-49,
// 60-112): complex128 state, float64 statistics (E = |C|^2 unrounded),
// amplitudes as numpy forms them (sqrt(uint8) -> float16, sqrt(float32) ->
// float32), the cold start's ifft2 of a float amplitude rounded to complex64.
//
// This file, top to bottom:
//  1. the element-wise, statistics and transpose kernels;
//  2. what the back ends share on the host: launch helpers, table uploads,
//     mixed-radix line plans, and AnySizeEngine -- every Engine method but
//     enqueue, written once on two device primitives a back end provides (the
//     unscaled 2-D transform at its precision, the GD field as complex64);
//  3. LinesEngine: the line transforms (chirp-z plans, its GS / GD loops);
//  4. TiledEngine: mixed radix and radix plans, one launch structure and one
//     set of buffers; they differ in how a tile is launched (row, col) and in
//     their tables, nowhere else;
//  5. the choice (generic_choose: back end, precision, tiles -- every
//     environment knob and occupancy query of this file) and generic_create.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <memory>
#include <vector>

#include "../../include/slm_hip.h"
#include "generic.hpp"
#include "kernels.hpp"
#include "mixed_radix.hpp"
#include "radix_c128.hpp"

namespace slm {

namespace {

constexpr int kGT = 256;  // threads per block of the element-wise kernels

// the error text is HIP's message alone
#define G_HIP(expr)                                                                   \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) return fail(SLM_ERR_HIP, "%s", hipGetErrorString(e_));  \
    } while (0)

int grid_of(long long n) { return (int)std::min<long long>(16384, (n + kGT - 1) / kGT); }

// numpy's amplitude of the target: sqrt(uint8) is float16,
// sqrt(float32) float32; then widened (the loop multiplies it with complex128)
__device__ __forceinline__ double g_amp(const void* tgt, int tt, long long i) {
    if (tt == TGT_U8) return (double)TgtLoad<TGT_U8>::amp(TgtLoad<TGT_U8>::load(tgt, i));
    return (double)(float)sqrt((double)static_cast<const float*>(tgt)[i]);
}
__device__ __forceinline__ double g_t(const void* tgt, int tt, long long i) {
    return tt == TGT_U8 ? (double)static_cast<const uint8_t*>(tgt)[i] : (double)static_cast<const float*>(tgt)[i];
}
__device__ __forceinline__ double g_ain(const float* ain, long long i, long long holo) {
    return ain ? (double)ain[i % holo] : 1.0;
}
// a exp(i angle(z)) == a z / |z|, angle(0) = 0 -> a (src/algorithms.py:30,33)
__device__ __forceinline__ double2 g_unit(double2 z, double a) {
    const double n2 = z.x * z.x + z.y * z.y;
    if (n2 == 0.0) return make_double2(a, 0.0);
    const double r = a / sqrt(n2);
    return make_double2(z.x * r, z.y * r);
}

__global__ void __launch_bounds__(kGT) k_unit(const double2* A, double2* B, const float* ain, long long holo,
                                              long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        B[i] = g_unit(A[i], g_ain(ain, i, holo));
}
// warm start: B = a_in exp(1j phi) with exp of a float32 phase in complex64 (numpy)
__global__ void __launch_bounds__(kGT) k_warm(const float* phi, double2* B, const float* ain, long long holo,
                                              long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        double s, c;
        sincos((double)phi[i], &s, &c);
        const double a = g_ain(ain, i, holo);
        B[i] = make_double2((double)(float)c * a, (double)(float)s * a);
    }
}
// a_T + 0i (the cold start's ifft2(sqrt(T)) and the "fourier" guess)
__global__ void __launch_bounds__(kGT) k_amp(const void* tgt, int tt, double2* D, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        D[i] = make_double2(g_amp(tgt, tt, i), 0.0);
}
// ifft2 of a float16 / float32 amplitude is complex64 in the reference (src/algorithms.py:27)
__global__ void __launch_bounds__(kGT) k_round_c64(double2* A, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        A[i] = make_double2((double)(float)A[i].x, (double)(float)A[i].y);
}
// "fourier" guess a_in exp(1j angle(ifft2(sqrt T))): angle of complex64 is float32, exp complex64
// (src/algorithms.py:153-156)
__global__ void __launch_bounds__(kGT) k_fourier(const double2* A, double2* X, const float* ain, long long holo,
                                                 long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const float ang = atan2f((float)A[i].y, (float)A[i].x);
        double s, c;
        sincos((double)ang, &s, &c);
        const double a = g_ain(ain, i, holo);
        X[i] = make_double2((double)(float)c * a, (double)(float)s * a);
    }
}
__global__ void __launch_bounds__(kGT) k_c64_to_c128(const float2* in, double2* out, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        out[i] = make_double2((double)in[i].x, (double)in[i].y);
}
__global__ void __launch_bounds__(kGT) k_c128_to_c64(const double2* in, float2* out, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        out[i] = make_float2((float)in[i].x, (float)in[i].y);
}
// Mixed-radix GD keeps its field x with every row in the digit-reversed order
// of the row transform (element e of a row holds column rev[e]: the row pass
// reads and writes it in place, coalesced); these read it back row-major.
__global__ void __launch_bounds__(kGT) k_phase_rev(const double2* X, float* phase, const int* rev, int W, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const long long r = i / W;
        const int e = (int)(i - r * W);
        phase[r * W + rev[e]] = (float)atan2(X[i].y, X[i].x);
    }
}
__global__ void __launch_bounds__(kGT) k_c128_to_c64_rev(const double2* X, float2* out, const int* rev, int W,
                                                        long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const long long r = i / W;
        const int e = (int)(i - r * W);
        out[r * W + rev[e]] = make_float2((float)X[i].x, (float)X[i].y);
    }
}
// a_in [H][W] with every row in that order (read by the iteration row passes)
__global__ void __launch_bounds__(kGT) k_ain_rev(const float* ain, float* out, const int* rev, int W, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const long long r = i / W;
        out[i] = ain[r * W + rev[(int)(i - r * W)]];
    }
}
// the target (uint8 or float32, row-major) as float in the complex128 radix
// kernels' B2 layout (radix_c128.hpp, b2_index): the column passes' reads of it
// are then contiguous like their field reads
__global__ void __launch_bounds__(kGT) k_tgt_b2(const void* tgt, int tt, float* out, int H, int W, long long n) {
    const long long holo = (long long)H * W;
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const long long b = i / holo, r = i - b * holo;
        const int y = (int)(r / W), x = (int)(r - (long long)y * W);
        const float t = tt == TGT_U8 ? (float)static_cast<const uint8_t*>(tgt)[i] : static_cast<const float*>(tgt)[i];
        out[b * holo + rz::b2_index(y, x, H)] = t;
    }
}
__global__ void __launch_bounds__(kGT) k_phase(const double2* A, float* phase, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        phase[i] = (float)atan2(A[i].y, A[i].x);
}
__global__ void __launch_bounds__(kGT) k_phase_exp(const float* phase, double2* B, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        double s, c;
        sincos((double)phase[i], &s, &c);
        B[i] = make_double2(c, s);
    }
}
__global__ void __launch_bounds__(kGT) k_abs2(const double2* C, float* out, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        out[i] = (float)(C[i].x * C[i].x + C[i].y * C[i].y);
}
// complex64 engine: exp(1j phase) of a float32 phase is complex64 (numpy), |C|^2 float32
__global__ void __launch_bounds__(kGT) k_phase_exp_c64(const float* phase, float2* B, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        double s, c;
        sincos((double)phase[i], &s, &c);
        B[i] = make_float2((float)c, (float)s);
    }
}
__global__ void __launch_bounds__(kGT) k_abs2_c64(const float2* C, float* out, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT)
        out[i] = C[i].x * C[i].x + C[i].y * C[i].y;
}

// Statistics block `blockIdx.x` of hologram `blockIdx.y`: a contiguous chunk.
struct ChunkOf {
    long long lo, hi;
    __device__ ChunkOf(long long holo, int nwg) {
        const long long chunk = (holo + nwg - 1) / nwg;
        lo = (long long)blockIdx.x * chunk;
        hi = lo + chunk < holo ? lo + chunk : holo;
    }
};
__device__ __forceinline__ void store_partials(double* partials, int b, int iter, int max_loops, int nwg, double mx,
                                               double s2, double st) {
    block_reduce_stats<kGT>(mx, s2, st);
    if (threadIdx.x == 0) {
        double* dst = partials + (((long long)b * max_loops + iter) * nwg + blockIdx.x) * 4;
        dst[0] = mx;
        dst[1] = s2;
        dst[2] = st;
        dst[3] = 0.0;
    }
}

// GS: E = |C|^2 and its statistics, expected output, D = a_T C/|C| (src/algorithms.py:33,36-38).
// A hologram whose checked run has stopped keeps D (and E): its later products repeat.
__global__ void __launch_bounds__(kGT) k_gs_project(const double2* C, const void* tgt, int tt, double2* D,
                                                    float* e_out, double* partials, const int* stop, int iter,
                                                    int checked, int write_e, long long holo, int nwg, int max_loops) {
    const int b = blockIdx.y;
    if (checked && iter > stop[b]) return;
    const ChunkOf ch(holo, nwg);
    double mx = 0.0, s2 = 0.0, st = 0.0;
    for (long long r = ch.lo + threadIdx.x; r < ch.hi; r += kGT) {
        const long long i = (long long)b * holo + r;
        const double2 z = C[i];
        const double e = z.x * z.x + z.y * z.y;
        mx = fmax(mx, e);
        s2 += e * e;
        st += e * g_t(tgt, tt, i);
        if (write_e) e_out[i] = (float)e;
        D[i] = g_unit(z, g_amp(tgt, tt, i));
    }
    store_partials(partials, b, iter, max_loops, nwg, mx, s2, st);
}

// GD: u = x / |x| a_in (src/algorithms.py:84; |x| = 0 gives NaN as there)
__global__ void __launch_bounds__(kGT) k_gd_u(const double2* X, double2* U, const float* ain, long long holo,
                                              long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const double2 x = X[i];
        const double r = g_ain(ain, i, holo) / sqrt(x.x * x.x + x.y * x.y);
        U[i] = make_double2(x.x * r, x.y * r);
    }
}
// GD: P = |F|^2 statistics (max for the normalisation, src/algorithms.py:85-86) and output
__global__ void __launch_bounds__(kGT) k_gd_stats(const double2* F, const void* tgt, int tt, float* e_out,
                                                  double* partials, const int* stop, int iter, int checked, int write_e,
                                                  long long holo, int nwg, int max_loops) {
    const int b = blockIdx.y;
    if (checked && iter > stop[b]) return;
    const ChunkOf ch(holo, nwg);
    double mx = 0.0, s2 = 0.0, st = 0.0;
    for (long long r = ch.lo + threadIdx.x; r < ch.hi; r += kGT) {
        const long long i = (long long)b * holo + r;
        const double2 z = F[i];
        const double e = z.x * z.x + z.y * z.y;
        mx = fmax(mx, e);
        s2 += e * e;
        st += e * g_t(tgt, tt, i);
        if (write_e) e_out[i] = (float)e;
    }
    store_partials(partials, b, iter, max_loops, nwg, mx, s2, st);
}
// one (hologram, iteration) slab -> stats, and the tolerance test (src/algorithms.py:29,83,92)
__global__ void __launch_bounds__(256) k_reduce_iter(StatsParams p) {
    const int b = blockIdx.x;
    if (p.iter > p.stop_iter[b]) return;
    __shared__ double o[4];
    reduce_slab(p, b, p.iter, o);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; ++k) p.stats[((long long)b * p.max_loops + p.iter) * 4 + k] = o[k];
        if (p.tol >= 0.0 && !(o[3] > p.tol)) p.stop_iter[b] = p.iter;
    }
}
// GD: G = mask F (s P - T), s = norm / max P, mask = 1 + wa T / 255 (src/algorithms.py:80,85-88)
__global__ void __launch_bounds__(kGT) k_gd_grad(const double2* F, const void* tgt, int tt, const double* stats,
                                                 const double* norm, double2* G, float wa, const int* stop, int iter,
                                                 int checked, long long holo, int max_loops, long long n) {
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const int b = (int)(i / holo);
        if (checked && iter > stop[b]) continue;
        const double s = norm[b] / stats[((long long)b * max_loops + iter) * 4];
        const double2 z = F[i];
        const double t = g_t(tgt, tt, i);
        // numpy's mask dtype: float32 for a float32 target (the python float scalars are
        // weak), float64 for uint8 (src/algorithms.py:80)
        const double mask = tt == TGT_U8 ? 1.0 + (double)wa * t / 255.0
                                         : (double)(1.0f + __fdiv_rn(__fmul_rn(wa, (float)t), 255.0f));
        const double w = mask * ((z.x * z.x + z.y * z.y) * s - t);
        G[i] = make_double2(z.x * w, z.y * w);
    }
}
// GD: dEdF = ifft2(G) a_in, dEdX_complex (src/algorithms.py:179-185), x -= lr dEdX (:91)
__global__ void __launch_bounds__(kGT) k_gd_update(double2* X, const double2* g, const float* ain, const float* lr,
                                                   const int* stop, int iter, int checked, double inv_s,
                                                   long long holo, long long n) {
    const double l = (double)lr[iter];
    for (long long i = blockIdx.x * (long long)kGT + threadIdx.x; i < n; i += (long long)gridDim.x * kGT) {
        const int b = (int)(i / holo);
        if (checked && iter > stop[b]) continue;
        const double a = g_ain(ain, i, holo) * inv_s;
        const double gx = g[i].x * a, gy = g[i].y * a;
        double2 x = X[i];
        const double ax2 = x.x * x.x + x.y * x.y;
        const double ax = sqrt(ax2);
        const double re = x.x * gx + x.y * gy;
        x.x -= l * ((gx - x.x * (re / ax2)) / ax);
        x.y -= l * ((gy - x.y * (re / ax2)) / ax);
        X[i] = x;
    }
}

// [B][R][C] -> [B][C][R] complex128 through 32 x 32 LDS tiles (the line
// transforms run along contiguous rows only)
__global__ void __launch_bounds__(256) k_transpose(const double2* in, double2* out, int R, int C) {
    __shared__ double2 tile[32][33];
    const long long hb = (long long)blockIdx.z * R * C;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        if (r < R && c < C) tile[k][tx] = in[hb + (long long)r * C + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (r < R && c < C) out[hb + (long long)c * R + r] = tile[tx][k];
    }
}

// ------------------------------------------------------------------------
// 2. shared by the back ends (host side)
// ------------------------------------------------------------------------
// an element-wise kernel over n elements (every one takes n as its last parameter)
template <typename K, typename... A>
void each(K k, hipStream_t st, long long n, A... args) {
    hipLaunchKernelGGL(k, dim3(grid_of(n)), dim3(kGT), 0, st, args..., n);
}

// one (hologram, iteration) slab -> stats; tol < 0: no stop flags (k_reduce_iter
// sets them for checked runs only)
void reduce_iter(const PlanState& v, double tol, int iter) {
    StatsParams s{};
    s.partials = v.partials;
    s.stats = v.stats;
    s.stop_iter = v.stop;
    s.norm = v.norm;
    s.sum_t2 = v.sum_t2;
    s.inv_s = 1.0 / (double)v.holo;
    s.tol = tol;
    s.max_loops = v.max_loops;
    s.nwg = v.nwg;
    s.iter = iter;
    hipLaunchKernelGGL(k_reduce_iter, dim3(v.B), dim3(256), 0, v.stream, s);
}

// a timed run's event pair around a launch (slm_plan_run_timed; the any-size
// engine launches directly, so the events are recorded on the plan stream)
struct Mark {
    const PlanState& v;
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
    Mark(const PlanState& vv, int cls) : v(vv) {
        if (v.timing && !v.timing->next(cls, &ev)) (void)hipEventRecord(ev->first, v.stream);
    }
    ~Mark() {
        if (ev) (void)hipEventRecord(ev->second, v.stream);
    }
};

// Device tables of one line plan: twiddles and output order, and for a chirp-z
// line the chirp and the transform of its kernel. They upload in pairs: both
// allocations, then both copies (the order of the hipMalloc calls is kept, see
// the build() of each engine).
struct LineTables {
    DevBuf<void> tw, rev, chirp, bhat;
};
int upload_pair(DevBuf<void>& a, const void* host_a, size_t bytes_a, DevBuf<void>& b, const void* host_b,
                size_t bytes_b, hipStream_t st) {
    RC(a.need(bytes_a, st));
    RC(b.need(bytes_b, st));
    G_HIP(hipMemcpyAsync(a.p, host_a, bytes_a, hipMemcpyHostToDevice, st));
    G_HIP(hipMemcpyAsync(b.p, host_b, bytes_b, hipMemcpyHostToDevice, st));
    G_HIP(hipStreamSynchronize(st));
    return 0;
}

// DIF stage radices of a length: 8s (then a 4 or a 2) for the powers of two,
// then 3, 5, 7, 11, 13; false if another prime divides n or n is too long
bool mr_radices(int n, std::vector<int>& rad) {
    rad.clear();
    if (n < 1 || n > mr::kMaxLine) return false;
    int t = n, twos = 0;
    while (t % 2 == 0) {
        t /= 2;
        ++twos;
    }
    while (twos >= 3 && twos != 4) {
        rad.push_back(8);
        twos -= 3;
    }
    if (twos == 4) {
        rad.push_back(4);
        rad.push_back(4);
    } else if (twos == 2) {
        rad.push_back(4);
    } else if (twos == 1) {
        rad.push_back(2);
    }
    for (int p : {3, 5, 7, 11, 13})
        while (t % p == 0) {
            rad.push_back(p);
            t /= p;
        }
    return t == 1 && (int)rad.size() <= mr::kMaxPass;
}

// the mixed-radix plan of n uses a radix outside mr::small_radix (7, 11, 13):
// its launches take the kernels built for the full radix set
bool big_radix(int n) {
    std::vector<int> r;
    if (!mr_radices(n, r)) return false;
    for (int x : r)
        if (!mr::small_radix(x)) return true;
    return false;
}

// twiddles exp(-2 pi i t / n) and the DIF output order's natural indices
int mr_plan_line(LineTables& t, int n, mr::LinePlan* pl, hipStream_t st, std::vector<int>* rev_out = nullptr) {
    std::vector<int> rad;
    if (!mr_radices(n, rad)) return fail(SLM_ERR_UNSUPPORTED, "mixed radix: unsupported length");
    pl->n = n;
    pl->np = (int)rad.size();
    for (int i = 0; i < pl->np; ++i) pl->radix[i] = rad[i];
    std::vector<double> tw((size_t)n * 2);
    for (long long t = 0; t < n; ++t) {
        const double ang = 2.0 * M_PI * (double)t / (double)n;
        tw[t * 2] = std::cos(ang);
        tw[t * 2 + 1] = -std::sin(ang);
    }
    std::vector<int> rev(n);
    for (int e = 0; e < n; ++e) {
        int k = 0, mul = 1, m = n, rem = e;
        for (int R : rad) {
            m /= R;
            const int q = rem / m;
            rem -= q * m;
            k += q * mul;
            mul *= R;
        }
        rev[e] = k;
    }
    RC(upload_pair(t.tw, tw.data(), tw.size() * sizeof(double), t.rev, rev.data(), rev.size() * sizeof(int), st));
    pl->tw = static_cast<const double2*>(t.tw.p);
    pl->rev = static_cast<const int*>(t.rev.p);
    if (rev_out) *rev_out = rev;
    return 0;
}

int mr_roots(hipStream_t st) {
    std::vector<double2> roots((mr::kMaxRadix + 1) * mr::kMaxRadix, make_double2(0.0, 0.0));
    for (int R = 1; R <= mr::kMaxRadix; ++R)
        for (int q = 0; q < R; ++q) {
            const double ang = 2.0 * M_PI * (double)q / (double)R;
            roots[R * mr::kMaxRadix + q] = make_double2(std::cos(ang), -std::sin(ang));
        }
    if (mr::mr_set_roots(roots.data(), st)) return fail(SLM_ERR_HIP, "mixed radix: root table upload failed");
    return 0;
}

// What every back end is to a plan. A back end allocates in build(), runs the
// iterations in enqueue() and provides the two device primitives; the rest of
// the Engine interface is written here, once, on top of them.
struct AnySizeEngine : Engine {
    const AnySizeChoice ch;
    // state every back end has (row-major complex128 [B][H][W]; the complex64
    // radix kernels keep float2 in the same buffers). Lines GS: A, then B and C
    // in place; GD: the inverse-transformed gradient g, then u and F in place.
    // Tiled: row-pass output, column-pass output. x: the GD field.
    DevBuf<double2> a, b, x;

    explicit AnySizeEngine(const AnySizeChoice& c) : ch(c) {}
    virtual int build(const PlanState& v) = 0;
    // out = fft2 / unscaled ifft2 of in, device [B][H][W] at ch.prec (complex64
    // behind the pointers at PREC_F32); in may equal out
    virtual int transform(const PlanState& v, const double2* in, double2* out, bool inverse) = 0;
    // the GD field x, row-major complex64
    virtual int field_c64(const PlanState& v, float2* out) = 0;

    void* target_stage(const PlanState& v) override { return v.tgt; }  // kept row-major as uploaded
    int land_target(PlanState&, const void*) override { return 0; }
    int land_field(PlanState& v, const float* field) override {
        HIP_TRY(hipMemcpyAsync(v.field0, field, (size_t)v.B * v.holo * sizeof(float2), hipMemcpyHostToDevice,
                               v.stream));
        return 0;
    }
    int set_precision(PlanState&, int) override { return fail(SLM_ERR_STATE, "any-size engines are rebuilt"); }
    int read_field(PlanState& v, bool fresh, float* field) override {
        if (!fresh) {
            if (!x.p) return fail(SLM_ERR_STATE, "the field is the state of GD plans");
            RC(field_c64(v, v.xa));
        }
        return copy_sync(field, fresh ? v.field0 : v.xa, (size_t)v.B * v.holo * sizeof(float2),
                         hipMemcpyDeviceToHost, v.stream);
    }
    // device complex64 [B][H][W] (in may equal out)
    int fft2_c64(const PlanState& v, const float2* in, float2* out, int inverse) {
        if (ch.prec == PREC_F32)  // complex64 radix kernels: straight on the caller's buffers
            return transform(v, reinterpret_cast<const double2*>(in), reinterpret_cast<double2*>(out), inverse != 0);
        const long long n = (long long)v.B * v.holo;
        each(k_c64_to_c128, v.stream, n, in, b.p);
        RC(transform(v, b.p, b.p, inverse != 0));
        each(k_c128_to_c64, v.stream, n, b.p, out);
        G_HIP(hipGetLastError());
        return 0;
    }
    // row-major in place through the plan's staging buffer
    int fft2(PlanState& v, const float* in, float* out, int inverse) override {
        const size_t bytes = (size_t)v.B * v.holo * sizeof(float2);
        hipError_t e = hipMemcpyAsync(v.xa, in, bytes, hipMemcpyHostToDevice, v.stream);
        if (e != hipSuccess) return fail(SLM_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
        RC(fft2_c64(v, v.xa, v.xa, inverse));
        return copy_sync(out, v.xa, bytes, hipMemcpyDeviceToHost, v.stream);
    }
    int fft2_z(PlanState& v, const double2* in, double2* out, int inverse) override {
        if (ch.prec != PREC_F64) return fail(SLM_ERR_STATE, "fft2_c128 on a complex64 engine");
        return transform(v, in, out, inverse != 0);
    }
    int intensity(PlanState& v) override {
        const long long n = (long long)v.B * v.holo;
        if (ch.prec == PREC_F32) {
            float2* b32 = reinterpret_cast<float2*>(b.p);
            each(k_phase_exp_c64, v.stream, n, v.phase_in, b32);
            RC(transform(v, b.p, b.p, false));
            each(k_abs2_c64, v.stream, n, b32, v.e_out);
        } else {
            each(k_phase_exp, v.stream, n, v.phase_in, b.p);
            RC(transform(v, b.p, b.p, false));
            each(k_abs2, v.stream, n, b.p, v.e_out);
        }
        G_HIP(hipGetLastError());
        return 0;
    }
    long long kernel_bytes(const PlanState& v, int cls) const override {
        if (ch.kind == 2) return 0;  // line transforms: no column / row kernel classes
        // mixed radix / radix plans, complex128 state (complex64: z = 8): column pass
        // in z + T + out z (GD statistics: in + T); row pass in z + out z (+ a_in)
        // (+ GD field read and write 2z)
        const long long px = (long long)v.B * v.holo;
        const long long tb = v.tt == SLM_TGT_U8 ? 1 : 4;
        const long long ab = v.has_ain ? 4 : 0;
        const long long z = ch.prec == PREC_F32 ? 8 : 16;
        switch (cls) {
            case SLM_KERNEL_COL_MAIN: return px * (2 * z + tb);
            case SLM_KERNEL_ROW_MAIN: return px * (2 * z + ab + (v.algo == SLM_ALGO_GD ? 2 * z : 0));
            case SLM_KERNEL_GD_STATS: return px * (z + tb);
            default: return 0;
        }
    }
    void codes(const PlanState&, int* col_engine, int* row_engine) const override {
        *col_engine = *row_engine = ch.kind;
    }
    void layout(int* x_log2, int* y_log2) const override { *x_log2 = *y_log2 = 0; }  // row-major
    void info(const PlanState& v, int info[8]) const override {
        const int i[8] = {0, v.nwg, 0, 0, 1, -1, -1, v.prec};  // no fused-engine tiles or plan keys
        std::copy(i, i + 8, info);
    }
    int generic_info(int info[8]) const override {
        const int i[8] = {ch.kind, ch.prec, ch.rkey, ch.ckey, ch.rpw, ch.cw, ch.lay, ch.kind == 2 ? 0 : ch.nwg};
        std::copy(i, i + 8, info);
        return 0;
    }
};

// ------------------------------------------------------------------------
// 3. line transforms
// ------------------------------------------------------------------------
// Line transform of length n (mr::LineArgs): direct where n has a mixed-radix
// plan (unless `chirp_z`), else Bluestein over the smallest M >= 2n - 1 made of
// the radices 2, 3, 4, 5, 8 (the small-radix kernels): the chirp w_j =
// exp(i pi j^2 / n) (angle from j^2 mod 2n, exact) and bhat = FFT_M(b) / M in
// the DIF output order, b_m = w_m for m < n, b_(M - m) = w_m for 0 < m < n,
// else 0 (one O(M^2) float64 DFT at plan creation, from a table of the M roots)
int line_plan(LineTables& t, int n, bool chirp_z, mr::LineArgs* la, bool* big, hipStream_t st) {
    std::vector<int> rad;
    *la = mr::LineArgs{};
    la->n = n;
    if (!chirp_z && mr_radices(n, rad)) {
        la->direct = 1;
        *big = big_radix(n);
        return mr_plan_line(t, n, &la->pl, st);
    }
    int M = std::max(1, 2 * n - 1);
    auto smooth5 = [](int m) {
        for (int p : {2, 3, 5})
            while (m % p == 0) m /= p;
        return m == 1;
    };
    while (!smooth5(M)) ++M;
    if (M > mr::kMaxLine)
        return fail(SLM_ERR_UNSUPPORTED,
                    "unsupported side: a side over 4096 with a prime factor above 13, or any side over "
                    "8192, does not fit one workgroup's chirp-z line (8192 points)");
    std::vector<int> rev;
    if (int rc = mr_plan_line(t, M, &la->pl, st, &rev)) return rc;
    la->direct = 0;
    *big = big_radix(M);
    std::vector<double> chirp((size_t)n * 2), b((size_t)M * 2, 0.0), bh((size_t)M * 2);
    for (long long j = 0; j < n; ++j) {
        const double ang = M_PI * (double)((j * j) % (2LL * n)) / (double)n;
        chirp[j * 2] = std::cos(ang);
        chirp[j * 2 + 1] = std::sin(ang);
        b[j * 2] = chirp[j * 2];
        b[j * 2 + 1] = chirp[j * 2 + 1];
        if (j > 0) {
            b[(M - j) * 2] = chirp[j * 2];
            b[(M - j) * 2 + 1] = chirp[j * 2 + 1];
        }
    }
    std::vector<double> rc_((size_t)M), rs_((size_t)M);
    for (int t = 0; t < M; ++t) {
        const double ang = 2.0 * M_PI * (double)t / (double)M;
        rc_[t] = std::cos(ang);
        rs_[t] = -std::sin(ang);
    }
    std::vector<double> bhat((size_t)M * 2);
    for (long long k = 0; k < M; ++k) {
        double re = 0.0, im = 0.0;
        long long idx = 0;
        for (long long m = 0; m < M; ++m) {
            const double br = b[m * 2], bi = b[m * 2 + 1];
            if (br != 0.0 || bi != 0.0) {
                re += br * rc_[idx] - bi * rs_[idx];
                im += br * rs_[idx] + bi * rc_[idx];
            }
            idx += k;
            if (idx >= M) idx -= M;
        }
        bhat[k * 2] = re / M;
        bhat[k * 2 + 1] = im / M;
    }
    for (int e = 0; e < M; ++e) {
        bh[(size_t)e * 2] = bhat[(size_t)rev[e] * 2];
        bh[(size_t)e * 2 + 1] = bhat[(size_t)rev[e] * 2 + 1];
    }
    RC(upload_pair(t.chirp, chirp.data(), chirp.size() * sizeof(double), t.bhat, bh.data(), bh.size() * sizeof(double),
                   st));
    la->chirp = static_cast<const double2*>(t.chirp.p);
    la->bhat = static_cast<const double2*>(t.bhat.p);
    return 0;
}

struct LinesEngine : AnySizeEngine {
    using AnySizeEngine::AnySizeEngine;
    DevBuf<double2> d;     // GS: D; GD: G
    DevBuf<double2> tmp;   // the row-transformed image
    DevBuf<double2> tmp2;  // the transposed image [B][W][H]
    mr::LineArgs lw, lh;   // the row (length W) and column (length H) transforms
    bool big_w = false, big_h = false;  // their plans need the odd-radix kernels
    LineTables tab_w, tab_h;

    // hipMalloc order (kept as it always was: the order of two allocations has
    // measured 2 % on a column pass, slm_capi.hip plan_create_on): a, b, d, tmp,
    // tmp2, x (GD); then per side, W before H: twiddles, output order, and on a
    // chirp-z side the chirp and bhat
    int build(const PlanState& v) override {
        const size_t bytes = (size_t)v.B * v.holo * sizeof(double2);
        hipStream_t st = v.stream;
        for (DevBuf<double2>* p : {&a, &b, &d, &tmp, &tmp2}) RC(p->need(bytes, st));
        if (v.algo == SLM_ALGO_GD) RC(x.need(bytes, st));
        RC(line_plan(tab_w, v.W, ch.chirp_all, &lw, &big_w, st));
        RC(line_plan(tab_h, v.H, ch.chirp_all, &lh, &big_h, st));
        return mr_roots(st);
    }

    // 1-D transforms of `lines` rows of the line plan's length
    int pass(const mr::LineArgs& base, bool big, const double2* in, double2* out, long long lines, bool inverse,
             hipStream_t st) {
        if (lines > 0x7fffffffLL) return fail(SLM_ERR_UNSUPPORTED, "line transforms: too many lines");
        mr::LineArgs la = base;
        la.in = in;
        la.out = out;
        la.inverse = inverse ? 1 : 0;
        if (mr::mr_line_launch(big, la, (int)lines, (size_t)la.pl.n * sizeof(double2), st))
            return fail(SLM_ERR_HIP, "line transform launch failed");
        return 0;
    }

    // rows -> transpose -> rows -> transpose
    int transform(const PlanState& v, const double2* in, double2* out, bool inverse) override {
        hipStream_t st = v.stream;
        RC(pass(lw, big_w, in, tmp.p, (long long)v.B * v.H, inverse, st));
        hipLaunchKernelGGL(k_transpose, dim3((v.W + 31) / 32, (v.H + 31) / 32, v.B), dim3(256), 0, st, tmp.p, tmp2.p,
                           v.H, v.W);
        RC(pass(lh, big_h, tmp2.p, tmp2.p, (long long)v.B * v.W, inverse, st));
        hipLaunchKernelGGL(k_transpose, dim3((v.H + 31) / 32, (v.W + 31) / 32, v.B), dim3(256), 0, st, tmp2.p, out,
                           v.W, v.H);
        G_HIP(hipGetLastError());
        return 0;
    }

    int field_c64(const PlanState& v, float2* out) override {
        each(k_c128_to_c64, v.stream, (long long)v.B * v.holo, x.p, out);
        G_HIP(hipGetLastError());
        return 0;
    }

    // a = ifft2(sqrt T) in complex64: the GS cold start and the "fourier" guess of GD
    int amp_ifft2(const PlanState& v, long long n) {
        each(k_amp, v.stream, n, v.tgt, v.tt, d.p);
        RC(transform(v, d.p, a.p, true));
        each(k_round_c64, v.stream, n, a.p);
        return 0;
    }

    int enqueue(PlanState& v, int loops, double tol, int checked, float wa, bool phase_set, bool field_set) override {
        const long long n = (long long)v.B * v.holo;
        const dim3 sgrid(v.nwg, v.B);
        hipStream_t st = v.stream;
        const double tol_or_none = checked ? tol : -1.0;
        if (v.algo == SLM_ALGO_GS) {
            if (phase_set)
                each(k_warm, st, n, v.phase_in, b.p, v.ain, v.holo);
            else
                RC(amp_ifft2(v, n));
            for (int i = 0; i < loops; ++i) {
                if (i > 0 || !phase_set) each(k_unit, st, n, a.p, b.p, v.ain, v.holo);
                RC(transform(v, b.p, b.p, false));  // C
                hipLaunchKernelGGL(k_gs_project, sgrid, dim3(kGT), 0, st, b.p, v.tgt, v.tt, d.p, v.e_out, v.partials,
                                   v.stop, i, checked, (checked || i + 1 == loops) ? 1 : 0, v.holo, v.nwg,
                                   v.max_loops);
                RC(transform(v, d.p, a.p, true));  // A = ifft2(D) * S
                if (checked) reduce_iter(v, tol_or_none, i);
            }
            each(k_phase, st, n, a.p, v.phase_out);
        } else {
            if (field_set) {
                each(k_c64_to_c128, st, n, v.field0, x.p);
            } else {
                RC(amp_ifft2(v, n));
                each(k_fourier, st, n, a.p, x.p, v.ain, v.holo);
            }
            const double inv_s = 1.0 / (double)v.holo;
            for (int i = 0; i < loops; ++i) {
                each(k_gd_u, st, n, x.p, b.p, v.ain, v.holo);
                RC(transform(v, b.p, b.p, false));  // F
                hipLaunchKernelGGL(k_gd_stats, sgrid, dim3(kGT), 0, st, b.p, v.tgt, v.tt, v.e_out, v.partials, v.stop,
                                   i, checked, (checked || i + 1 == loops) ? 1 : 0, v.holo, v.nwg, v.max_loops);
                // this iteration's max |F|^2 (and, checked, its error against the tolerance)
                reduce_iter(v, tol_or_none, i);
                each(k_gd_grad, st, n, b.p, v.tgt, v.tt, v.stats, v.norm, d.p, wa, v.stop, i, checked, v.holo,
                     v.max_loops);
                RC(transform(v, d.p, a.p, true));  // g = ifft2(G) * S
                each(k_gd_update, st, n, x.p, a.p, v.ain, v.lr, v.stop, i, checked, inv_s, v.holo);
            }
            each(k_phase, st, n, x.p, v.phase_out);
        }
        G_HIP(hipGetLastError());
        return 0;
    }
};

// ------------------------------------------------------------------------
// 4. mixed radix and radix plans
// ------------------------------------------------------------------------
// Stockham twiddle table of a plan key (the float32 engine's layout,
// slm_capi.hip get_twiddles: every pass after the first holds (R - 1) Ns
// entries exp(-2 pi i j r / (Ns R)); a mixed plan appends the same for its
// reversed pass order; float2 for the complex64 kernels) and the identity
// order (natural in and out)
int rz_plan_line(LineTables& t, int key, int prec, mr::LinePlan* pl, hipStream_t st) {
    const RadixPlan& rp = kPlans[key];
    std::vector<double> tw;
    // the forward pass order, then (mixed plans) the reversed one the inverse runs
    for (int rev = 0; rev < (plan_mixed(key) ? 2 : 1); ++rev) {
        int ns = 1;
        for (int k = 0; k < rp.npass; ++k) {
            const int r_ = pass_radix(key, rev != 0, k);
            if (ns > 1) {
                const long long L = (long long)ns * r_;
                for (int r = 1; r < r_; ++r)
                    for (int j = 0; j < ns; ++j) {
                        const long long q = ((long long)j * r) % L;
                        const double ang = -2.0 * M_PI * (double)q / (double)L;
                        tw.push_back(std::cos(ang));
                        tw.push_back(std::sin(ang));
                    }
            }
            ns *= r_;
        }
    }
    if (tw.empty()) {
        tw.push_back(1.0);
        tw.push_back(0.0);
    }
    std::vector<int> rev(rp.n);
    for (int e = 0; e < rp.n; ++e) rev[e] = e;
    std::vector<float> twf(tw.begin(), tw.end());
    const bool f32 = prec == PREC_F32;
    RC(upload_pair(t.tw, f32 ? (const void*)twf.data() : (const void*)tw.data(),
                   f32 ? twf.size() * sizeof(float) : tw.size() * sizeof(double), t.rev, rev.data(),
                   rev.size() * sizeof(int), st));
    pl->n = rp.n;
    pl->np = 0;
    pl->tw = static_cast<const double2*>(t.tw.p);
    pl->rev = static_cast<const int*>(t.rev.p);
    return 0;
}

// Both back ends run an iteration as a column launch and a row launch on tiles
// (mr::RowArgs / mr::ColArgs, mixed_radix.hpp); the radix plans put the same
// contract on compile-time Stockham transforms (their line plans hold Stockham
// twiddle tables and the identity order). Which of the two a plan is shows in
// build(), row() and col() only.
struct TiledEngine : AnySizeEngine {
    using AnySizeEngine::AnySizeEngine;
    mr::LinePlan pw, ph;      // row (length W) and column (length H) transforms
    LineTables tab_w, tab_h;  // their twiddles and output orders
    int cw_log2 = 0;          // mixed radix: ch.cw = 2^cw_log2 (the radix kernels take ch.cw itself)
    DevBuf<float> ain_rev;    // a_in with rows in the row transform's digit-reversed order (has_ain)
    DevBuf<float> tgt_blk;    // radix plans: the target as float in their B2 layout (rebuilt per run)

    bool radix_plans() const { return ch.kind >= 4; }

    // hipMalloc order (kept as it always was: the order of two allocations has
    // measured 2 % on a column pass, slm_capi.hip plan_create_on): a, b, x (GD),
    // ain_rev (a_in), tgt_blk (radix plans, either layout); then the row plan's
    // twiddles and output order, then the column plan's
    int build(const PlanState& v) override {
        const size_t n = (size_t)v.B * v.holo;
        hipStream_t st = v.stream;
        RC(a.need(n * sizeof(double2), st));
        RC(b.need(n * sizeof(double2), st));
        if (v.algo == SLM_ALGO_GD) RC(x.need(n * sizeof(double2), st));
        if (v.has_ain) RC(ain_rev.need((size_t)v.holo * sizeof(float), st));
        if (radix_plans()) {
            RC(tgt_blk.need(n * sizeof(float), st));
            RC(rz_plan_line(tab_w, ch.rkey, ch.prec, &pw, st));
            RC(rz_plan_line(tab_h, ch.ckey, ch.prec, &ph, st));
        } else {
            while ((1 << cw_log2) < ch.cw) ++cw_log2;
            RC(mr_plan_line(tab_w, v.W, &pw, st));
            RC(mr_plan_line(tab_h, v.H, &ph, st));
            RC(mr_roots(st));
        }
        // the state is defined before any run (read_field of a fresh plan is refused upstream)
        if (hipMemsetAsync(a.p, 0, n * sizeof(double2), st) != hipSuccess)
            return fail(SLM_ERR_HIP, "%s: state initialisation failed", radix_plans() ? "radix c128" : "mixed radix");
        return 0;
    }

    int row(const PlanState& v, int op, mr::RowArgs ra, int cls = SLM_KERNEL_OTHER) {
        ra.pl = pw;
        ra.B = v.B;
        ra.H = v.H;
        ra.W = v.W;
        ra.rpw = ch.rpw;
        ra.holo = v.holo;
        ra.inv_s = 1.0 / (double)v.holo;
        ra.ain = v.ain;
        ra.ain_rev = v.ain ? ain_rev.p : nullptr;
        ra.stop = v.stop;
        const int grid = v.B * ((v.H + ch.rpw - 1) / ch.rpw);
        const size_t lds = (size_t)ch.rpw * v.W * sizeof(double2);
        Mark mk(v, cls);
        if (radix_plans()) {
            // an unchecked run's iterations before the last never take the phase branch
            if (op == mr::RO_GS && !ra.checked && !ra.last) op = mr::RO_GS_MID;
            if (rz::rz_row_launch(ch.rkey, ch.prec, ch.lay, op, ra, grid, v.stream))
                return fail(SLM_ERR_HIP, "radix-plan row launch failed");
            return 0;
        }
        if (mr::mr_row_launch(op, ch.big, ra, grid, lds, v.stream))
            return fail(SLM_ERR_HIP, "mixed-radix row launch failed");
        return 0;
    }

    int col(const PlanState& v, int op, mr::ColArgs ca, int cls = SLM_KERNEL_OTHER) {
        ca.pl = ph;
        ca.B = v.B;
        ca.H = v.H;
        ca.W = v.W;
        ca.cw_log2 = cw_log2;
        ca.nwg = ch.nwg;
        ca.holo = v.holo;
        ca.tgt = v.tgt;
        ca.tgt_blk = tgt_blk.p;
        ca.tt = v.tt;
        ca.e_out = v.e_out;
        ca.partials = v.partials;
        ca.stop = v.stop;
        ca.stats = v.stats;
        ca.norm = v.norm;
        ca.max_loops = v.max_loops;
        const int grid = v.B * ch.nwg;
        const size_t lds = ((size_t)v.H << cw_log2) * sizeof(double2);
        Mark mk(v, cls);
        if (radix_plans()) {
            if (op == mr::CO_GD_GRAD && v.tt == TGT_U8) op = mr::CO_GD_GRAD_U8;
            if (rz::rz_col_launch(ch.ckey, ch.prec, ch.lay, ch.cw, op, ca, grid, v.stream))
                return fail(SLM_ERR_HIP, "radix-plan column launch failed");
            return 0;
        }
        if (mr::mr_col_launch(op, ch.big, ca, grid, lds, v.stream))
            return fail(SLM_ERR_HIP, "mixed-radix column launch failed");
        return 0;
    }

    // a row launch into a, a column launch out of it
    int transform(const PlanState& v, const double2* in, double2* out, bool inverse) override {
        mr::RowArgs r;
        r.in = in;
        r.out = a.p;
        RC(row(v, inverse ? mr::RO_INV : mr::RO_FWD, r));
        mr::ColArgs c;
        c.in = a.p;
        c.out = out;
        return col(v, inverse ? mr::CO_INV : mr::CO_FWD, c);
    }

    // The field x is kept with every row in the row transform's output order
    // (k_c128_to_c64_rev; the identity on radix plans)
    int field_c64(const PlanState& v, float2* out) override {
        each(k_c128_to_c64_rev, v.stream, (long long)v.B * v.holo, x.p, out, pw.rev, v.W);
        G_HIP(hipGetLastError());
        return 0;
    }

    int enqueue(PlanState& v, int loops, double tol, int checked, float wa, bool phase_set, bool field_set) override {
        const long long n = (long long)v.B * v.holo;
        hipStream_t st = v.stream;
        const double tol_or_none = checked ? tol : -1.0;
        mr::RowArgs r;
        mr::ColArgs c;
        r.checked = c.checked = checked;
        c.wa = wa;
        if (ch.lay == rz::LAY_B2)  // the target in B2 (set_target may have changed it)
            each(k_tgt_b2, st, n, v.tgt, v.tt, tgt_blk.p, v.H, v.W);
        if (v.ain)  // the row passes read a_in in their digit-reversed order
            each(k_ain_rev, st, v.holo, v.ain, ain_rev.p, pw.rev, v.W);
        if (v.algo == SLM_ALGO_GS) {
            // setup (src/algorithms.py:14-27): the warm start B = a_in exp(i phi), or
            // A0 = ifft2(sqrt T) in complex64, B = a_in A0/|A0|; row-transformed into a
            if (phase_set) {
                r.phase_in = v.phase_in;
                r.out = a.p;
                RC(row(v, mr::RO_WARM, r));
            } else {
                c.out = b.p;
                RC(col(v, mr::CO_AMP_INV, c));
                r.in = b.p;
                r.out = a.p;
                RC(row(v, mr::RO_COLD, r));
            }
            for (int i = 0; i < loops; ++i) {
                c.in = a.p;
                c.out = b.p;
                c.iter = i;
                c.write_e = (checked || i + 1 == loops) ? 1 : 0;
                RC(col(v, mr::CO_GS, c, SLM_KERNEL_COL_MAIN));
                if (checked) reduce_iter(v, tol_or_none, i);
                r.in = b.p;
                r.out = a.p;
                r.iter = i;
                r.last = i + 1 == loops;
                r.phase_out = v.phase_out;
                RC(row(v, mr::RO_GS, r, SLM_KERNEL_ROW_MAIN));
            }
        } else {
            // setup (make_initial_guess, src/algorithms.py:115-158): the host field, or
            // the "fourier" guess a_in exp(i angle(ifft2(sqrt T)))
            r.x = x.p;
            if (field_set) {
                r.field0 = v.field0;
                r.out = a.p;
                RC(row(v, mr::RO_GD_INIT, r));
            } else {
                c.out = b.p;
                RC(col(v, mr::CO_AMP_INV, c));
                r.in = b.p;
                r.out = a.p;
                RC(row(v, mr::RO_GD_FOURIER, r));
            }
            r.lr = v.lr;
            for (int i = 0; i < loops; ++i) {
                c.in = a.p;
                c.iter = i;
                c.write_e = (checked || i + 1 == loops) ? 1 : 0;
                RC(col(v, mr::CO_GD_STATS, c, SLM_KERNEL_GD_STATS));
                // this iteration's max |F|^2 (and, checked, its error against the tolerance)
                reduce_iter(v, tol_or_none, i);
                c.out = b.p;
                RC(col(v, mr::CO_GD_GRAD, c, SLM_KERNEL_COL_MAIN));
                r.in = b.p;
                r.out = a.p;
                r.iter = i;
                r.last = i + 1 == loops;
                RC(row(v, mr::RO_GD, r, SLM_KERNEL_ROW_MAIN));
            }
            each(k_phase_rev, st, n, x.p, v.phase_out, pw.rev, v.W);
        }
        G_HIP(hipGetLastError());
        return 0;
    }
};

// ------------------------------------------------------------------------
// 5. the choice
// ------------------------------------------------------------------------
// $SLM_GENERIC_ENGINE: mr keeps a plan off the radix-plan kernels; bluestein
// (alias: gemm, r05's name of that back end) sends every side through the line
// transforms, chirp-z included
enum Forced { FORCE_NONE, FORCE_MR, FORCE_LINES };
Forced forced_back_end() {
    const char* e = std::getenv("SLM_GENERIC_ENGINE");
    if (e && (!std::strcmp(e, "bluestein") || !std::strcmp(e, "gemm"))) return FORCE_LINES;
    return e && !std::strcmp(e, "mr") ? FORCE_MR : FORCE_NONE;
}

// Mixed-radix tiles of the two launches. A launch of `wgs` workgroups of `e`
// elements on `cus` CUs that hold `occ` of them at once takes about rounds x
// (workgroups per CU in a round) x e: so the rows per row tile / columns per
// column tile minimise ceil(wgs / (cus occ)) * min(occ, ceil(wgs / cus)) * e (a
// grid one workgroup too large for a round doubles the launch: 1080 rows in 540
// two-row tiles on 512 slots did, 62.6 against ~35 us). Column tiles that tie
// go to 2 columns (32-B row segments), then the narrower: 1080 x 1920 columns
// in tiles of 2 measured 48.2 us against 58.0 in tiles of 1 and 55.0 in tiles
// of 4 (profiles/r05/mr_tiles_s13.txt); row tiles that tie go to the wider.
// $SLM_MR_RPW / $SLM_MR_CW override.
void mr_tiling(int B, int H, int W, AnySizeChoice* t) {
    const bool big = t->big;
    int cw_log2 = 0;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    auto cost = [&](long long wgs, int occ, long long e) {
        const long long slots = (long long)cus * occ;
        const long long rounds = (wgs + slots - 1) / slots;
        const long long per = std::min<long long>(occ, (wgs + cus - 1) / cus);
        return rounds * per * e;
    };
    long long best = -1;
    for (int r = 1; r == 1 || (long long)r * W <= mr::kTileElems; r *= 2) {
        if (r > 1 && r > H) break;
        const int occ = mr::mr_row_occupancy(mr::RO_GS, big, (size_t)r * W * sizeof(double2));
        if (occ < 1) continue;
        const long long c = cost((long long)B * ((H + r - 1) / r), occ, (long long)r * W);
        if (best < 0 || c <= best) {
            best = c;
            t->rpw = r;
        }
    }
    best = -1;
    for (int c : {1, 0, 2, 3, 4}) {  // tie order
        if (c > 0 && (((long long)H << c) > mr::kTileElems || (1 << c) > 2 * W)) continue;
        const int occ = mr::mr_col_occupancy(mr::CO_GS, big, ((size_t)H << c) * sizeof(double2));
        if (occ < 1) continue;
        const long long v = cost((long long)B * ((W + (1 << c) - 1) >> c), occ, (long long)H << c);
        if (best < 0 || v < best) {
            best = v;
            cw_log2 = c;
        }
    }
    if (const char* e = std::getenv("SLM_MR_RPW")) t->rpw = std::max(1, std::min(H, std::atoi(e)));
    if (const char* e = std::getenv("SLM_MR_CW")) {
        int c = 0;
        while (c < 4 && (2 << c) <= std::atoi(e)) ++c;
        cw_log2 = c;
    }
    t->cw = 1 << cw_log2;
    t->nwg = (W + t->cw - 1) >> cw_log2;
}

// Plan key of one axis: both sides need a built radix plan (rz::key_built) at
// the engine's precision; a 13-smooth panel side (plans.hpp variant 3,
// complex64 only) has its one plan.
// As the float32 engine's pick: the narrow variant (half the elements per
// thread) where the wide one would leave fewer than 4 waves per SIMD over
// the chip, else the wide one; $SLM_RZ_PLAN=wide|narrow forces a variant.
// Column transforms take the E = 8 plan where one exists (4096: 1024-thread
// two-column tiles at <= 128 VGPRs, 16 waves per CU where the E = 16 tiles
// hold 8); $SLM_RZ_PLAN / $SLM_RZ_ROW_PLAN / $SLM_RZ_COL_PLAN =
// wide|narrow|e8 force a variant (per axis for the last two).
int rz_key(int n, long long elems, bool col, int prec, int algo) {
    const int wide = plan_index(n, 0), narrow = plan_index(n, 1), e8 = plan_index(n, 2), panel = plan_index(n, 3);
    if (rz::key_built(panel, prec)) {
        // variant 4 (1920 = 8.16.15 on 240 threads) for rows, where it measured
        // faster (complex64 GS 1080 x 1920 row pass 30.1 -> 25.3 us, complex128 GD
        // 52.3 -> 43.9), variant 3 (15.16.8, 128 threads) for columns (1920 x 1080
        // column pass 36.0 against 39.8, profiles/r06/speed_c64_alt_q.txt) and for
        // complex128 GS rows (34.6 -> 29.0 us, profiles/r06/ab_rows_f64_zh.txt);
        // $SLM_RZ_PANEL=alt|main forces one
        const int alt = plan_index(n, 4);
        const char* a = std::getenv("SLM_RZ_PANEL");
        const bool use_alt = a ? !std::strcmp(a, "alt") : !col && !(prec == PREC_F64 && algo == SLM_ALGO_GS);
        return use_alt && rz::key_built(alt, prec) ? alt : panel;
    }
    const bool w_ok = rz::key_built(wide, prec), n_ok = rz::key_built(narrow, prec), e_ok = rz::key_built(e8, prec);
    const char* s = std::getenv(col ? "SLM_RZ_COL_PLAN" : "SLM_RZ_ROW_PLAN");
    if (!s) s = std::getenv("SLM_RZ_PLAN");
    if (s) {
        if (!std::strcmp(s, "wide") && w_ok) return wide;
        if (!std::strcmp(s, "narrow") && n_ok) return narrow;
        if (!std::strcmp(s, "e8") && e_ok) return e8;
    }
    if (col && e_ok) return e8;
    if (!w_ok && !n_ok) return e_ok ? e8 : -1;
    if (!w_ok) return narrow;
    if (!n_ok) return wide;
    const long long waves = elems / kPlans[wide].e / 64;
    return waves < 4LL * 1024 ? narrow : wide;
}

// Columns per column tile: 256 threads where the line's LDS allows two
// workgroups per CU (4 columns of 64 threads, 2 of 128), 2 for 256-thread
// lines (4096: one 512-thread workgroup per CU, 32-B row segments), 8 for
// 8-thread lines; $SLM_RZ_CW overrides.
int rz_cw_of(int ckey, int W, int prec) {
    const int T = kPlans[ckey].n / kPlans[ckey].e;
    // complex64 lines of 64+ threads: 2 (1080 x 1920 column pass 35.4 -> 25.4 us,
    // 768 x 1280 18.7 -> 16.7 us with 4 -> 2 columns, profiles/r06/speed_c64_cw2_p.txt)
    int cw = T >= (prec == PREC_F32 || kPlans[ckey].variant >= 3 ? 64 : 128) ? 2 : T >= 16 ? 4 : 8;
    if (const char* e = std::getenv("SLM_RZ_CW")) cw = std::atoi(e);
    if (cw < 1 || W % cw || !rz::rz_col_ok(ckey, prec, cw)) return 0;
    return cw;
}

// State layout of the radix kernels (radix_c128.hpp LAY_RM / LAY_B2): B2 (whole
// lines on the column side, 64-B pieces on the row side) except GS plans with a
// 4096-point side, whose row-major rows measured faster than B2 row pairs by
// more than the B2 columns gained (profiles/r06); $SLM_RZ_LAYOUT=rm|b2 forces one.
// The complex64 kernels are built on B2 only.
int rz_layout(int algo, int H, int W, int prec) {
    if (prec == PREC_F32) return rz::LAY_B2;
    if (const char* e = std::getenv("SLM_RZ_LAYOUT")) {
        if (!std::strcmp(e, "rm")) return rz::LAY_RM;
        if (!std::strcmp(e, "b2")) return rz::LAY_B2;
    }
    return (algo == SLM_ALGO_GS && std::max(H, W) >= 4096) ? rz::LAY_RM : rz::LAY_B2;
}

// The radix-plan choice at `prec`, if the shape has one. Complex64 radix
// kernels: GS only (GD's 500-iteration gradient loop keeps complex128 state,
// DESIGN.md section 3)
bool rz_shape(int B, int H, int W, int algo, int prec, AnySizeChoice* out) {
    if (prec == PREC_F32 && algo != SLM_ALGO_GS) return false;
    AnySizeChoice c;
    c.kind = prec == PREC_F32 ? 5 : 4;
    c.prec = prec;
    const long long elems = (long long)B * H * W;
    c.rkey = rz_key(W, elems, false, prec, algo);
    c.ckey = rz_key(H, elems, true, prec, algo);
    if (c.rkey < 0 || c.ckey < 0) return false;
    c.cw = rz_cw_of(c.ckey, W, prec);
    c.lay = rz_layout(algo, H, W, prec);
    if (rz::key_panel(c.rkey) || rz::key_panel(c.ckey)) c.lay = rz::LAY_B2;  // panel keys: B2 only
    c.rpw = rz::rz_row_rpw(c.rkey, c.lay);
    if (!(c.cw > 0 && c.rpw > 0 && H % c.rpw == 0 && W % 2 == 0)) return false;  // B2 panels (and the target copy)
    c.nwg = W / c.cw;
    *out = c;
    return true;
}

}  // namespace

// Radix plans where both sides have one at the precision (complex64 if float32
// was asked for and GS can run it, else complex128); else mixed radix where both
// sides factor into 2 .. 13; else line transforms.
AnySizeChoice generic_choose(int B, int H, int W, int algo, int prec) {
    AnySizeChoice c;
    const Forced forced = forced_back_end();
    if (forced == FORCE_NONE &&
        ((prec == PREC_F32 && rz_shape(B, H, W, algo, PREC_F32, &c)) || rz_shape(B, H, W, algo, PREC_F64, &c)))
        return c;
    std::vector<int> r;
    if (forced != FORCE_LINES && mr_radices(H, r) && mr_radices(W, r)) {
        c.kind = 3;
        c.big = big_radix(H) || big_radix(W);
        mr_tiling(B, H, W, &c);
        return c;
    }
    c.chirp_all = forced == FORCE_LINES;
    c.nwg = (int)std::max<long long>(1, std::min<long long>(1024, (long long)H * W / (kGT * 8)));
    return c;
}

int generic_create(const PlanState& v, const AnySizeChoice& c, Engine** out) {
    *out = nullptr;
    std::unique_ptr<AnySizeEngine> e;
    if (c.kind == 2)
        e.reset(new LinesEngine(c));
    else
        e.reset(new TiledEngine(c));
    RC(e->build(v));
    *out = e.release();
    return 0;
}

const AnySizeChoice& generic_choice(const Engine& e) { return static_cast<const AnySizeEngine&>(e).ch; }

}  // namespace slm
