// Spot-based weighted Gerchberg-Saxton for trap lists (include/slm_hip.h,
// "trap lists"; DESIGN.md section 3, "Trap lists"). No reference counterpart.
//
// The field is evaluated at the M traps only, so there is no transform and no
// radix plan: every panel shape runs. The trap phase is separable,
//     D_m(k, l) = fy_m(k) + fx_m(l),
//     fy_m(k) = 2 pi frac(k y_m / H) + z_m (k - H/2)^2   (fx likewise on l, x_m, W),
// so with the tables Py[k][m] = exp(i fy_m(k)) and Px[l][m] = exp(i fx_m(l)) one
// iteration is two complex matrix products with the trap count as a dimension:
//     V_m     = sum_k conj(Py[k][m]) sum_l (a U)[k][l] conj(Px[l][m])     spot_fields_kernel
//     weights, statistics, c_m = a_T,m w_m V_m / |V_m|  (float64)        spot_update_kernel
//     S[k][l] = sum_m (Py[k][m] c_m) Px[l][m];  U = S / |S|              spot_superpose_kernel
// The state is the unit field U = exp(i phi), complex64: the loop never takes
// an angle; the float32 phase is formed by the last superposition.
//
// Both products run on v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fmaf
// chain). A complex product is a real one with K doubled. The K = 2 of one
// instruction is spread over the two lane halves, so lane half h carries summed
// index 2 j + h and one MFMA each takes the real and the imaginary parts:
//     re += a.x * b.x;  im += a.x * b.y;  re += a.y * (-b.y);  im += a.y * b.x
// (for the fields product b is conj(Px), which moves the sign). Four MFMAs per
// step and 32 x 32 output tile = 8 FLOP per pixel and trap.
//
// Tables, built at slm_spots_set_traps in float64 and rounded to complex64,
// are kept in two layouts so that every operand is read along its fast index:
//   row layout   [n][Mp]  (Py, Px): lanes run over traps; the fields product's
//                B operand (256 B per lane half per step) and its epilogue
//   trap layout  [m][n]   (PyT, PxT): lanes run over pixels; both operands of
//                the superposition (256 B per lane half per step)
// Mp is M padded with zero columns to a multiple of 32.
// The fields product's A operand is the field itself, [k][l] with l summed:
// lanes run over rows there, so each 32 x 32 tile goes through LDS, written as
// whole 256 B row segments and read back as 8 B per lane with a row stride of
// 66 floats: lane (i, h) reads banks 2 i + 2 h (+1) mod 64 of step j's 4 j
// offset, all 64 banks once per 32 lanes.
//
// Trap trajectories (slm_spots_sequence): F frames of a moving list as one
// chain on the stream. Per frame one launch builds the four tables from
// coordinates that went up once for all frames; the frame's iterations follow,
// starting from the U and w the frame before left. One int per frame and
// hologram is 0 while the frame runs and its iteration count afterwards: the
// update kernel sets it (the fixed last iteration, or std(r) <= tol), later
// launches of the frame return at once on it, and the superposition of that
// very iteration also stores the float32 phase and the quantised uint8 frame.
//
// Host side: every device buffer is a DevBuf (runtime.hpp); a list's four tables are one
// launch (launch_tables), for slm_spots_set_traps and for a frame alike; and
// run_frame issues the iterations a Frame describes: a run is the handle's own
// buffers without a stop word (own_frame), a trajectory one slice per frame.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "quantize.hpp"
#include "runtime.hpp"
#include "seq_frames.hpp"
#include "spot_tiles.hpp"  // the tile constants, acc_row, mfma and table_entry (shared with zoom.hip)

namespace {

using namespace slm::tiles;

constexpr double kGolden = 0.6180339887498949;
constexpr int kUpdThreads = 1024; // spot_update_kernel: one trap per thread after the fold
constexpr int kMaxTraps = 1024;
constexpr int kFieldsThreads = 64 * kWaves;
constexpr int kTargetWaves = 4096;  // fields grid: split columns until this many waves per hologram

// ---- tables ---------------------------------------------------------------
// All four tables of one list (a handle's, or one frame's of a trajectory) in
// one launch, from coordinates that are already on the device: elements
// [0, H Mp) are Py, then PyT, Px and PxT, each stored along its own fast index.
// grid = (blocks, batch).
struct SeqTableParams {
    const double *ys, *xs, *zs;  // this list's [B][M]
    float2 *py, *pyt, *px, *pxt;
    int H, W, M, Mp;
};

__global__ void __launch_bounds__(256) spot_seq_tables_kernel(SeqTableParams p) {
    const long long n_y = (long long)p.H * p.Mp, n_x = (long long)p.W * p.Mp, n_el = 2 * (n_y + n_x);
    const int b = blockIdx.y;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n_el; i += (long long)gridDim.x * 256) {
        const bool is_x = i >= 2 * n_y;
        const long long n_t = is_x ? n_x : n_y;
        long long j = is_x ? i - 2 * n_y : i;
        const bool transposed = j >= n_t;
        if (transposed) j -= n_t;
        const int N = is_x ? p.W : p.H;
        int n, m;
        if (transposed) {
            m = (int)(j / N);
            n = (int)(j - (long long)m * N);
        } else {
            n = (int)(j / p.Mp);
            m = (int)(j - (long long)n * p.Mp);
        }
        float2 v = make_float2(0.0f, 0.0f);
        if (m < p.M) v = table_entry(n, N, (is_x ? p.xs : p.ys)[(size_t)b * p.M + m], p.zs[(size_t)b * p.M + m]);
        float2* out = is_x ? (transposed ? p.pxt : p.px) : (transposed ? p.pyt : p.py);
        out[(size_t)b * n_t + j] = v;
    }
}

// U0 = exp(i phase), float64 sine and cosine of the float32 phase
__global__ void __launch_bounds__(256) spot_phase_kernel(const float* phase, float2* u, long long n) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        double s, c;
        sincos((double)phase[i], &s, &c);
        u[i] = make_float2((float)c, (float)s);
    }
}

// ---- fields: V partials ---------------------------------------------------
struct FieldsParams {
    const float2* u;    // [B][H][W]
    const float* ain;   // [H][W] or nullptr
    const float2* px;   // [B][W][Mp]
    const float2* py;   // [B][H][Mp]
    double2* partial;   // [B][units][Mp]
    int H, W, Mp;
    int col_splits, cols_per_split, units;
    const int* stop;    // [B] or nullptr: nonzero = this hologram's frame has ended (sequences)
};

// Four waves per workgroup; each wave takes 32 rows x cols_per_split columns of
// the field against 32 traps (one accumulator tile each for re and im) through
// an LDS tile of its own, and the workgroup folds its four partial V in order:
// one partial per 128 rows x cols_per_split columns. All four waves run the
// same column range, so they pass the same barriers; a wave past the last row
// works on zeros. grid = (groups of 4 row tiles x column splits, 32-trap tiles, batch).
__global__ void __launch_bounds__(kFieldsThreads) spot_fields_kernel(FieldsParams p) {
    __shared__ float tiles[kWaves][kTile * kLdsStride];
    __shared__ double2 vsum[kWaves][kTile];
    if (p.stop && p.stop[blockIdx.z] != 0) return;  // the whole workgroup, before any barrier
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    float* tile = tiles[wave];
    const int unit = blockIdx.x, rg = unit / p.col_splits, cs = unit - rg * p.col_splits;
    const int b = blockIdx.z, m0 = blockIdx.y * kTile;
    const int row0 = (rg * kWaves + wave) * kTile;
    const int c_begin = cs * p.cols_per_split, c_end = min(p.W, c_begin + p.cols_per_split);
    const float2* u = p.u + (size_t)b * p.H * p.W;
    const float2* px = p.px + (size_t)b * p.W * p.Mp + m0 + li;
    const float2* py = p.py + (size_t)b * p.H * p.Mp + m0 + li;

    f32x16 are, aim;
#pragma unroll
    for (int r = 0; r < 16; ++r) are[r] = aim[r] = 0.0f;

    // Registers carry the next tile of the field (ut, at) and the table rows of
    // the next eight steps (q0 / q1) while the matrix cores work on this one.
    constexpr int kHalf = kTile / 4;  // steps per half tile (a step = 2 columns)
    float2 ut[16], q0[kHalf], q1[kHalf];
    float at[16];
    // a 32 x 32 tile of the field: lanes 0-31 one row, lanes 32-63 the next (256 B each)
    auto load_tile = [&](int c0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gr = row0 + 2 * r + lh, gc = c0 + li;
            ut[r] = make_float2(0.0f, 0.0f);
            at[r] = 1.0f;
            if (gr < p.H && gc < c_end) {
                ut[r] = u[(size_t)gr * p.W + gc];
                if (p.ain) at[r] = p.ain[(size_t)gr * p.W + gc];
            }
        }
    };
    // lane (m, h): Px of column c0 + 2 (j0 + s) + h; columns past the edge read the last one (their field is zero)
    auto load_q = [&](float2(&q)[kHalf], int c0, int j0) {
#pragma unroll
        for (int s = 0; s < kHalf; ++s) q[s] = px[(size_t)min(c0 + 2 * (j0 + s) + lh, p.W - 1) * p.Mp];
    };
    auto mma = [&](const float2(&q)[kHalf], int j0) {
#pragma unroll
        for (int s = 0; s < kHalf; ++s) {
            // lane (i, h): pixel (row0 + i, c0 + 2 (j0 + s) + h)
            const float2 a = *reinterpret_cast<const float2*>(&tile[li * kLdsStride + 4 * (j0 + s) + 2 * lh]);
            are = mfma(a.x, q[s].x, are);
            aim = mfma(a.x, -q[s].y, aim);
            are = mfma(a.y, q[s].y, are);
            aim = mfma(a.y, q[s].x, aim);
        }
    };

    load_tile(c_begin);
    load_q(q0, c_begin, 0);
    for (int c0 = c_begin; c0 < c_end; c0 += kTile) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            *reinterpret_cast<float2*>(&tile[(2 * r + lh) * kLdsStride + 2 * li]) =
                make_float2(ut[r].x * at[r], ut[r].y * at[r]);
        __syncthreads();
        load_q(q1, c0, kHalf);
        load_tile(c0 + kTile);  // past c_end: zeros, nothing is read
        mma(q0, 0);
        load_q(q0, c0 + kTile, 0);
        mma(q1, kHalf);
        __syncthreads();
    }

    // V partial = sum over the tile's rows of conj(Py) R, in float64; lane (m, h) holds 16 rows of trap m
    double vr = 0.0, vi = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gr = row0 + acc_row(r, lh);
        if (gr < p.H) {
            const float2 y = py[(size_t)gr * p.Mp];
            const double rr = are[r], ri = aim[r];
            vr += (double)y.x * rr + (double)y.y * ri;
            vi += (double)y.x * ri - (double)y.y * rr;
        }
    }
    vr += __shfl_xor(vr, 32);
    vi += __shfl_xor(vi, 32);
    if (lh == 0) vsum[wave][li] = make_double2(vr, vi);
    __syncthreads();
    if (threadIdx.x < kTile) {
        double2 v = vsum[0][li];
#pragma unroll
        for (int k = 1; k < kWaves; ++k) {
            v.x += vsum[k][li].x;
            v.y += vsum[k][li].y;
        }
        p.partial[((size_t)b * p.units + unit) * p.Mp + m0 + li] = v;
    }
}

// ---- update: fold, statistics, weights, coefficients ----------------------
struct UpdateParams {
    const double2* partial;  // [B][units][Mp]
    const double* a_t;       // [B][Mp] sqrt(I)
    const double* w_in;      // [B][Mp]
    double* w_out;           // [B][Mp]
    double2* v;              // [B][Mp]
    float2* c;               // [B][Mp]
    double* stats;           // [B][max_loops][4], this iteration's row at + 4 it
    int M, Mp, units, max_loops, it;
    double feedback, inv_norm;  // inv_norm = 1 / (H W sum a^2)
    // sequences (nullptr otherwise): stop[b] = 0 while hologram b's frame runs, then the number of
    // iterations it took: set at iteration last_it, or earlier once std(r) <= tol (tol > 0)
    int* stop;
    int last_it;
    double tol;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the same value in every thread, in an order fixed by the thread index alone
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kUpdThreads / 64; ++i) s += sh[i];
    return s;
}

__device__ __forceinline__ double block_min(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int i = 1; i < kUpdThreads / 64; ++i) s = fmin(s, sh[i]);
    return s;
}

__global__ void __launch_bounds__(kUpdThreads) spot_update_kernel(UpdateParams p) {
    __shared__ double2 fold[kUpdThreads];
    __shared__ double red[kUpdThreads / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    if (p.stop && p.stop[b] != 0) return;  // the whole workgroup, before any barrier
    const bool live = t < p.M;

    // fold the partials: group g takes units g, g + G, ...; the groups are then added in order
    const int groups = kUpdThreads / p.Mp;
    const int g = t / p.Mp, mm = t - g * p.Mp;
    double2 acc = make_double2(0.0, 0.0);
    if (g < groups) {
        const double2* src = p.partial + (size_t)b * p.units * p.Mp + mm;
        // eight loads in flight, added in the order of the units
        for (int u = g; u < p.units; u += 8 * groups) {
            double2 d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int uu = u + i * groups;
                d[i] = uu < p.units ? src[(size_t)uu * p.Mp] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                acc.x += d[i].x;
                acc.y += d[i].y;
            }
        }
    }
    fold[t] = acc;
    __syncthreads();
    double vr = 0.0, vi = 0.0;
    if (live) {
        for (int k = 0; k < groups; ++k) {
            vr += fold[k * p.Mp + t].x;
            vi += fold[k * p.Mp + t].y;
        }
    }
    const size_t at = (size_t)b * p.Mp + t;
    const double a_t = live ? p.a_t[at] : 1.0;
    const double e = vr * vr + vi * vi, amp = sqrt(e);
    const double q = live ? e / (a_t * a_t) : 0.0;

    // statistics of this iteration's field (before the update)
    const double sum_e = block_sum(live ? e : 0.0, red);
    const double mean_q = block_sum(q, red) / p.M;
    const double r = q / mean_q;
    const double mean_r = block_sum(live ? r : 0.0, red) / p.M;
    const double dev = live ? (r - mean_r) * (r - mean_r) : 0.0;
    const double var_r = block_sum(dev, red) / p.M;
    const double min_r = block_min(live ? r : INFINITY, red);
    const double max_r = -block_min(live ? -r : INFINITY, red);
    if (t == 0) {
        double* st = p.stats + ((size_t)b * p.max_loops + p.it) * 4;
        st[0] = sum_e * p.inv_norm;
        st[1] = sqrt(var_r);
        st[2] = min_r;
        st[3] = max_r;
        if (p.stop && (p.it == p.last_it || (p.tol > 0.0 && sqrt(var_r) <= p.tol))) p.stop[b] = p.it + 1;
    }

    // weights: w *= (a_T / |V|)^p where |V| > 0, factor clamped to [2^-64, 2^64]; then mean 1
    double w = live ? p.w_in[at] : 0.0;
    if (live && amp > 0.0) {
        double f = pow(a_t / amp, p.feedback);
        f = fmin(fmax(f, 0x1p-64), 0x1p64);
        w *= f;
    }
    const double mean_w = block_sum(w, red) / p.M;
    w /= mean_w;
    if (t < p.Mp) {
        float2 c = make_float2(0.0f, 0.0f);
        if (live) {
            const double s = a_t * w;
            c = amp > 0.0 ? make_float2((float)(s * (vr / amp)), (float)(s * (vi / amp))) : make_float2((float)s, 0.0f);
            p.w_out[at] = w;
        }
        p.v[at] = make_double2(vr, vi);
        p.c[at] = c;
    }
}

// ---- superposition: U = S / |S| -------------------------------------------
struct SuperposeParams {
    const float2* pyt;  // [B][Mp][H]
    const float2* pxt;  // [B][Mp][W]
    const float2* c;    // [B][Mp]
    float2* u;          // [B][H][W]
    float* phase;       // [B][H][W] or nullptr (only the run's last iteration stores it)
    int H, W, M, Mp;
    // sequences (stop = nullptr otherwise): iteration `it` of a frame is hologram b's last one when
    // stop[b] == it + 1; only then are the phase and the quantised frame stored
    const int* stop;     // [B]
    int it;
    uint8_t* frame;      // [B][H][W] or nullptr
    const double* mask;  // [H][W] or nullptr
    double ct2pi;
    int rule;
};

// One wave per 32 x 32 output tile, four adjacent column tiles per workgroup (a
// workgroup puts one wave on each SIMD of its CU). grid = (column tiles / 4, row tiles, batch).
__global__ void __launch_bounds__(kFieldsThreads) spot_superpose_kernel(SuperposeParams p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int b = blockIdx.z, row0 = blockIdx.y * kTile, col0 = (blockIdx.x * kWaves + wave) * kTile;
    bool last = true;
    if (p.stop) {
        const int n_it = p.stop[b];  // the same for the whole workgroup
        if (n_it != 0 && n_it != p.it + 1) return;
        last = n_it != 0;
    }
    if (col0 >= p.W) return;  // no barriers below
    // rows / columns past the edge read the last valid line; their results are not stored
    const float2* py = p.pyt + (size_t)b * p.Mp * p.H + min(row0 + li, p.H - 1);
    const float2* px = p.pxt + (size_t)b * p.Mp * p.W + min(col0 + li, p.W - 1);
    const float2* c = p.c + (size_t)b * p.Mp;
    f32x16 sre, sim;
#pragma unroll
    for (int r = 0; r < 16; ++r) sre[r] = sim[r] = 0.0f;
    // Groups of 8 steps = 16 traps (the padded columns are zero and 16 divides into Mp); the next
    // group's table rows and coefficients are in flight while the matrix cores work on this one.
    constexpr int kGroup = 8;
    float2 y[kGroup], x[kGroup], cm[kGroup], yn[kGroup], xn[kGroup], cn[kGroup];
    const int groups = (p.M + 2 * kGroup - 1) / (2 * kGroup);
#pragma unroll
    for (int s = 0; s < kGroup; ++s) {
        const int m = 2 * s + lh;
        y[s] = py[(size_t)m * p.H];
        x[s] = px[(size_t)m * p.W];
        cm[s] = c[m];
    }
    for (int g = 0; g < groups; ++g) {
        if (g + 1 < groups) {
#pragma unroll
            for (int s = 0; s < kGroup; ++s) {
                const int m = 2 * (kGroup * (g + 1) + s) + lh;
                yn[s] = py[(size_t)m * p.H];
                xn[s] = px[(size_t)m * p.W];
                cn[s] = c[m];
            }
        }
#pragma unroll
        for (int s = 0; s < kGroup; ++s) {
            const float ar = y[s].x * cm[s].x - y[s].y * cm[s].y, ai = y[s].x * cm[s].y + y[s].y * cm[s].x;
            sre = mfma(ar, x[s].x, sre);
            sim = mfma(ar, x[s].y, sim);
            sre = mfma(ai, -x[s].y, sre);
            sim = mfma(ai, x[s].x, sim);
        }
        if (g + 1 == groups) break;
#pragma unroll
        for (int s = 0; s < kGroup; ++s) {
            y[s] = yn[s];
            x[s] = xn[s];
            cm[s] = cn[s];
        }
    }
    const int gc = col0 + li;
    if (gc >= p.W) return;
    const size_t base = (size_t)b * p.H * p.W + gc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gr = row0 + acc_row(r, lh);
        if (gr >= p.H) continue;
        float sr = sre[r], si = sim[r];
        float2 v = make_float2(1.0f, 0.0f);  // S = 0: angle 0
        const float big = fmaxf(fabsf(sr), fabsf(si));
        if (big > 0.0f) {
            int ex;  // scale by a power of two: no overflow or underflow of the square
            (void)frexpf(big, &ex);
            sr = ldexpf(sr, -ex);
            si = ldexpf(si, -ex);
            const float inv = rsqrtf(sr * sr + si * si);
            v = make_float2(sr * inv, si * inv);
        }
        p.u[base + (size_t)gr * p.W] = v;
        if (last && (p.phase || p.frame)) {
            const float ph = (float)atan2((double)sim[r], (double)sre[r]);
            if (p.phase) p.phase[base + (size_t)gr * p.W] = ph;
            if (p.frame)
                p.frame[base + (size_t)gr * p.W] =
                    slm::quantize((double)ph, p.mask ? p.mask[(size_t)gr * p.W + gc] : 0.0, p.ct2pi, p.rule);
        }
    }
}

int padded_traps(int m) { return (m + kTile - 1) / kTile * kTile; }

}  // namespace

using slm::DevBuf;
using slm::fail;
using slm::grid_for;
using slm::Stopwatch;

struct slm_spots {
    int B = 0, H = 0, W = 0, max_traps = 0, has_ain = 0, max_loops = 0;
    int M = 0, Mp = 0;  // the current list (0 = none set)
    int col_splits = 1, cols_per_split = 0, units = 0;
    double feedback = 1.0, sum_a2 = 0.0;
    bool ain_set = false, custom_phase = false, u0_valid = false, has_run = false;
    int last_loops = 0;
    hipStream_t stream = nullptr;
    DevBuf<float> ain;
    DevBuf<float2> u0, u;  // the start (runs read it, never write it) and the state
    DevBuf<float> phase;
    DevBuf<float2> py, px, pyt, pxt;
    DevBuf<double> coords;  // ys, xs, zs [3][B][M]
    DevBuf<double> a_t, w0, w, stats;
    DevBuf<double2> v, partial;  // partial is sized for the list (set_list_size)
    DevBuf<float2> c, c0;
    std::vector<double> host_a_t;  // [B][M], for the default start
    // the last sequence (slm_spots_sequence): per-frame slices, sized at the call
    int seq_frames = 0, seq_traps = 0, seq_loops = 0;  // frames, traps and statistics rows per frame (0 = none yet)
    bool seq_resumable = false, seq_has_frames = false, seq_has_phases = false;
    DevBuf<double> seq_coords;  // ys, xs, zs [3][F][B][M]
    DevBuf<double> seq_a_t;     // [F][B][Mp]
    DevBuf<double> seq_w;       // [F + 1][B][Mp]: slice 0 is the start, slice f + 1 frame f's
    DevBuf<double2> seq_v;      // [F][B][Mp]
    DevBuf<double> seq_stats;   // [F][B][seq_loops][4]
    DevBuf<int> seq_iters;      // [F][B]: the stop words, then the iteration counts
    DevBuf<uint8_t> seq_out;    // [F][B][H][W] quantised frames
    DevBuf<float> seq_phase;    // [F][B][H][W]
    DevBuf<double> seq_mask;    // [H][W]
    DevBuf<double> seq_w_last;  // [B][Mp]: the weights the last sequence ended with (resume)
};

// the resident zoom's door to the frames of the last sequence (seq_frames.hpp)
slm::SeqFrames slm::spots_seq_frames(const slm_spots* s) {
    SeqFrames q;
    q.stream = s->stream;
    q.n = s->seq_frames * s->B;
    q.H = s->H;
    q.W = s->W;
    if (s->seq_frames && s->seq_has_frames) q.frames = s->seq_out.p;
    return q;
}

namespace {

void spots_free(slm_spots* s) {
    if (!s) return;
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int up(slm_spots* s, void* dst, const void* src, size_t bytes) {
    return slm::copy_sync(dst, src, bytes, hipMemcpyHostToDevice, s->stream);
}
int down(slm_spots* s, void* dst, const void* src, size_t bytes) {
    return slm::copy_sync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream);
}

// ---- host helpers shared by the list and the sequence entry points --------
// `n` traps (all holograms, all frames): finite coordinates, positive finite intensities
int check_traps(size_t n, const double* ys, const double* xs, const double* zs, const float* intensity) {
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(ys[i]) || !std::isfinite(xs[i]) || (zs && !std::isfinite(zs[i])))
            return fail(SLM_ERR_ARG, "trap %zu has a non-finite coordinate", i);
        if (intensity && !(intensity[i] > 0.0f && std::isfinite(intensity[i])))
            return fail(SLM_ERR_ARG, "trap %zu: the intensity must be positive and finite", i);
    }
    return 0;
}

// start weights [B][M] or nullptr (= ones)
int check_weights(const slm_spots* s, int M, const float* weights) {
    for (size_t i = 0; weights && i < (size_t)s->B * M; ++i)
        if (!(weights[i] > 0.0f && std::isfinite(weights[i])))
            return fail(SLM_ERR_ARG, "weight %d of hologram %d is not positive and finite", (int)(i % M), (int)(i / M));
    return 0;
}

// [rows][M] -> [rows][Mp]: entry (r, m) is at(r M + m), the padding is `fill`
template <typename T, typename At>
std::vector<T> pad(size_t rows, int M, int Mp, T fill, At at) {
    std::vector<T> out(rows * Mp, fill);
    for (size_t r = 0; r < rows; ++r)
        for (int m = 0; m < M; ++m) out[r * Mp + m] = at(r * M + m);
    return out;
}

// device V [rows][Mp] -> fields [rows][M][2]
int read_fields(slm_spots* s, const double2* dev, size_t rows, int M, int Mp, double* fields) {
    std::vector<double2> v(rows * Mp);
    RC(down(s, v.data(), dev, v.size() * sizeof(double2)));
    for (size_t r = 0; r < rows; ++r)
        for (int m = 0; m < M; ++m) {
            fields[2 * (r * M + m)] = v[r * Mp + m].x;
            fields[2 * (r * M + m) + 1] = v[r * Mp + m].y;
        }
    return 0;
}

// device w [rows][Mp] float64 -> weights [rows][M] float32
int read_weights(slm_spots* s, const double* dev, size_t rows, int M, int Mp, float* weights) {
    std::vector<double> w(rows * Mp);
    RC(down(s, w.data(), dev, w.size() * sizeof(double)));
    for (size_t r = 0; r < rows; ++r)
        for (int m = 0; m < M; ++m) weights[r * M + m] = (float)w[r * Mp + m];
    return 0;
}

// the current list's a_T on the host, from its padded form [B][Mp]
void refill_host_a_t(slm_spots* s, const double* a_t) {
    s->host_a_t.resize((size_t)s->B * s->M);
    for (int b = 0; b < s->B; ++b) std::copy_n(a_t + (size_t)b * s->Mp, s->M, &s->host_a_t[(size_t)b * s->M]);
}

// ys, xs, zs (nullptr = 0) of n traps each to dst[0 .. 3 n)
int upload_coords(slm_spots* s, double* dst, size_t n, const double* ys, const double* xs, const double* zs) {
    RC(up(s, dst, ys, n * sizeof(double)));
    RC(up(s, dst + n, xs, n * sizeof(double)));
    if (zs) return up(s, dst + 2 * n, zs, n * sizeof(double));
    HIP_TRY(hipMemsetAsync(dst + 2 * n, 0, n * sizeof(double), s->stream));
    return 0;
}

// weights [B][M] of the current list, or nullptr = ones, to dst [B][Mp]
int upload_weights(slm_spots* s, double* dst, const float* weights) {
    const std::vector<double> w =
        pad(s->B, s->M, s->Mp, 1.0, [&](size_t i) { return weights ? (double)weights[i] : 1.0; });
    return up(s, dst, w.data(), w.size() * sizeof(double));
}

// ---- launches -------------------------------------------------------------
// Where one frame's a_T, weights, V, statistics, stop word and outputs live: a
// slice of the sequence buffers, or (own_frame) the handle's buffers for a run.
struct Frame {
    const double* a_t;   // [B][Mp]
    const double* w_in;  // the weights iteration 0 reads: the start, or the previous frame's
    double* w;
    double2* v;
    double* stats;       // [B][stats_loops][4]
    int stats_loops;
    int* stop;           // [B], or nullptr: all `loops` iterations run and only the last stores the phase
    int loops;           // this frame's iteration count (at most, with a stop word)
    double tol;
    float* phase;        // [B][H][W] or nullptr
    uint8_t* frame;      // [B][H][W] or nullptr
    const double* mask;
    double ct2pi;
    int rule;
};

Frame own_frame(slm_spots* s, int loops) {
    return Frame{s->a_t.p, s->w0.p, s->w.p, s->v.p, s->stats.p, s->max_loops, nullptr, loops, 0.0,
                 s->phase.p, nullptr, nullptr, 0.0, 0};
}

// Each launch fills its parameter block once, in the order of the struct's fields.
// launch_tables: the four tables of the current list, whose ys, xs, zs [B][M] are on the device
int launch_tables(slm_spots* s, const double* ys, const double* xs, const double* zs) {
    const SeqTableParams p{ys, xs, zs, s->py.p, s->pyt.p, s->px.p, s->pxt.p, s->H, s->W, s->M, s->Mp};
    hipLaunchKernelGGL(spot_seq_tables_kernel, dim3(grid_for(2LL * (s->H + s->W) * s->Mp), s->B), dim3(256), 0,
                       s->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_fields(slm_spots* s, const float2* u, const int* stop) {
    const FieldsParams p{u, s->ain_set ? s->ain.p : nullptr, s->px.p, s->py.p, s->partial.p, s->H, s->W, s->Mp,
                         s->col_splits, s->cols_per_split, s->units, stop};
    hipLaunchKernelGGL(spot_fields_kernel, dim3(s->units, s->Mp / kTile, s->B), dim3(kFieldsThreads), 0, s->stream,
                       p);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_update(slm_spots* s, const Frame& fr, int it) {
    const UpdateParams p{s->partial.p, fr.a_t, it == 0 ? fr.w_in : fr.w, fr.w, fr.v, s->c.p, fr.stats,
                         s->M, s->Mp, s->units, fr.stats_loops, it,
                         s->feedback, 1.0 / ((double)s->H * s->W * s->sum_a2),
                         fr.stop, fr.loops - 1, fr.tol};
    hipLaunchKernelGGL(spot_update_kernel, dim3(s->B), dim3(kUpdThreads), 0, s->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// u = the unit field of sum_m c_m exp(i D_m). Without a stop word only the frame's last iteration
// is handed the phase; with one every iteration is, and the kernel stores it where the word says.
int launch_superpose(slm_spots* s, const Frame& fr, int it, const float2* c, float2* u) {
    const dim3 grid((s->W + kWaves * kTile - 1) / (kWaves * kTile), (s->H + kTile - 1) / kTile, s->B);
    const SuperposeParams p{s->pyt.p, s->pxt.p, c, u, fr.stop || it == fr.loops - 1 ? fr.phase : nullptr,
                            s->H, s->W, s->M, s->Mp, fr.stop, it, fr.frame, fr.mask, fr.ct2pi, fr.rule};
    hipLaunchKernelGGL(spot_superpose_kernel, grid, dim3(kFieldsThreads), 0, s->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the start of a run without a caller's phase: angle(sum_m a_T,m exp(i (D_m + theta_m)))
int default_start(slm_spots* s) {
    if (s->custom_phase || s->u0_valid) return 0;
    const std::vector<float2> c0 = pad(s->B, s->M, s->Mp, make_float2(0.0f, 0.0f), [&](size_t i) {
        double th = (double)(i % s->M) * kGolden;
        th = kTwoPi * (th - std::floor(th));
        const double a = s->host_a_t[i];
        return make_float2((float)(a * std::cos(th)), (float)(a * std::sin(th)));
    });
    RC(up(s, s->c0.p, c0.data(), c0.size() * sizeof(float2)));
    RC(launch_superpose(s, Frame{}, 0, s->c0.p, s->u0.p));  // no frame: nothing but the unit field is stored
    s->u0_valid = true;
    return 0;
}

// one frame: fr.loops iterations of fields, update and superposition; the first reads `start`,
// the others the state the one before left
int run_frame(slm_spots* s, const Frame& fr, const float2* start, Stopwatch& tm) {
    const hipStream_t st = s->stream;
    for (int it = 0; it < fr.loops; ++it) {
        RC(tm.begin(SLM_SPOTS_KERNEL_FIELDS, st));
        RC(launch_fields(s, it == 0 ? start : s->u.p, fr.stop));
        RC(tm.end(st));
        RC(tm.begin(SLM_SPOTS_KERNEL_UPDATE, st));
        RC(launch_update(s, fr, it));
        RC(tm.end(st));
        RC(tm.begin(SLM_SPOTS_KERNEL_SUPERPOSE, st));
        RC(launch_superpose(s, fr, it, s->c.p, s->u.p));
        RC(tm.end(st));
    }
    return 0;
}

int run_loops(slm_spots* s, int loops, double* us_per_class) {
    if (!s) return fail(SLM_ERR_ARG, "null spots handle");
    if (!s->M) return fail(SLM_ERR_STATE, "slm_spots_run before slm_spots_set_traps");
    if (s->has_ain && !s->ain_set) return fail(SLM_ERR_STATE, "slm_spots_run before slm_spots_set_ain");
    if (loops < 1 || loops > s->max_loops)
        return fail(SLM_ERR_ARG, "loops %d outside 1 .. max_loops %d", loops, s->max_loops);
    RC(slm::ensure_device());
    s->seq_resumable = false;  // the run overwrites the unit field a sequence left
    RC(default_start(s));
    Stopwatch tm;
    tm.reset(us_per_class != nullptr);
    RC(run_frame(s, own_frame(s, loops), s->u0.p, tm));
    s->has_run = true;
    s->last_loops = loops;
    if (!us_per_class) return 0;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return tm.read(us_per_class, SLM_SPOTS_NUM_KERNEL_CLASSES);
}

// how the fields product is cut for Mp: a function of the shape and the list alone, never of the batch
void plan_fields(slm_spots* s) {
    const int row_tiles = (s->H + kTile - 1) / kTile, chunks = (s->W + kTile - 1) / kTile;
    const int groups = s->Mp / kTile;
    int splits = (kTargetWaves + row_tiles * groups - 1) / (row_tiles * groups);
    splits = std::max(1, std::min(splits, chunks));
    const int chunks_per = (chunks + splits - 1) / splits;
    s->col_splits = (chunks + chunks_per - 1) / chunks_per;
    s->cols_per_split = chunks_per * kTile;
    s->units = (row_tiles + kWaves - 1) / kWaves * s->col_splits;
}

// a list of n_traps: the padded count, the cut of the fields product and its partial sums
int set_list_size(slm_spots* s, int n_traps) {
    s->M = n_traps;
    s->Mp = padded_traps(n_traps);
    s->has_run = false;
    s->u0_valid = false;
    plan_fields(s);
    return s->partial.need((size_t)s->B * s->units * s->Mp * sizeof(double2), s->stream);
}

// every buffer whose size the handle's shape fixes
int size_buffers(slm_spots* s) {
    const size_t holo = (size_t)s->H * s->W, bm = (size_t)s->B * padded_traps(s->max_traps);
    const hipStream_t st = s->stream;
    if (s->has_ain) RC(s->ain.need(holo * sizeof(float), st));
    RC(s->u0.need(s->B * holo * sizeof(float2), st));
    RC(s->u.need(s->B * holo * sizeof(float2), st));
    RC(s->phase.need(s->B * holo * sizeof(float), st));
    RC(s->py.need(bm * s->H * sizeof(float2), st));
    RC(s->pyt.need(bm * s->H * sizeof(float2), st));
    RC(s->px.need(bm * s->W * sizeof(float2), st));
    RC(s->pxt.need(bm * s->W * sizeof(float2), st));
    RC(s->coords.need(3 * (size_t)s->B * s->max_traps * sizeof(double), st));
    RC(s->a_t.need(bm * sizeof(double), st));
    RC(s->w0.need(bm * sizeof(double), st));
    RC(s->w.need(bm * sizeof(double), st));
    RC(s->v.need(bm * sizeof(double2), st));
    RC(s->c.need(bm * sizeof(float2), st));
    RC(s->c0.need(bm * sizeof(float2), st));
    return s->stats.need((size_t)s->B * s->max_loops * 4 * sizeof(double), st);
}

}  // namespace

extern "C" {

int slm_spots_create(int batch, int height, int width, int max_traps, int has_ain, int max_loops, slm_spots** out) {
    if (!out) return fail(SLM_ERR_ARG, "null output handle");
    *out = nullptr;
    if (batch < 1 || max_loops < 1) return fail(SLM_ERR_ARG, "batch and max_loops must be positive");
    if (height < kMinSide || width < kMinSide || height > kMaxSide || width > kMaxSide)
        return fail(SLM_ERR_ARG, "trap lists run on sides %d .. %d, got %d x %d", kMinSide, kMaxSide, height, width);
    if (max_traps < 1 || max_traps > kMaxTraps)
        return fail(SLM_ERR_ARG, "max_traps %d outside 1 .. %d", max_traps, kMaxTraps);
    RC(slm::ensure_device());
    slm_spots* s = new slm_spots;
    s->B = batch;
    s->H = height;
    s->W = width;
    s->max_traps = max_traps;
    s->has_ain = has_ain != 0;
    s->max_loops = max_loops;
    s->sum_a2 = (double)height * width;
    const int rc = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess
                       ? fail(SLM_ERR_HIP, "hipStreamCreate failed")
                       : size_buffers(s);
    if (rc) {
        spots_free(s);
        return rc;
    }
    *out = s;
    return 0;
}

int slm_spots_destroy(slm_spots* sp) {
    if (sp) {
        if (sp->stream) (void)hipStreamSynchronize(sp->stream);
        spots_free(sp);
    }
    return 0;
}

int slm_spots_set_traps(slm_spots* s, int n_traps, const double* ys, const double* xs, const double* zs,
                        const float* intensity) {
    if (!s || !ys || !xs) return fail(SLM_ERR_ARG, "null argument");
    if (n_traps < 1 || n_traps > s->max_traps)
        return fail(SLM_ERR_ARG, "%d traps outside 1 .. max_traps %d", n_traps, s->max_traps);
    const size_t n = (size_t)s->B * n_traps;
    RC(check_traps(n, ys, xs, zs, intensity));
    RC(slm::ensure_device());
    s->seq_resumable = false;
    RC(set_list_size(s, n_traps));
    double* d = s->coords.p;
    RC(upload_coords(s, d, n, ys, xs, zs));
    const std::vector<double> a_t = pad(s->B, n_traps, s->Mp, 1.0, [&](size_t i) {
        return intensity ? std::sqrt((double)intensity[i]) : 1.0;
    });
    refill_host_a_t(s, a_t.data());
    RC(up(s, s->a_t.p, a_t.data(), a_t.size() * sizeof(double)));
    RC(upload_weights(s, s->w0.p, nullptr));
    RC(launch_tables(s, d, d + n, d + 2 * n));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

int slm_spots_set_ain(slm_spots* s, const float* ain) {
    if (!s || !ain) return fail(SLM_ERR_ARG, "null argument");
    if (!s->has_ain) return fail(SLM_ERR_STATE, "the handle was created without a_in");
    const size_t holo = (size_t)s->H * s->W;
    double sum = 0.0;
    RC(slm::check_ain(ain, holo, &sum));
    RC(slm::ensure_device());
    s->seq_resumable = false;
    RC(up(s, s->ain.p, ain, holo * sizeof(float)));
    s->sum_a2 = sum;
    s->ain_set = true;
    return 0;
}

int slm_spots_set_phase(slm_spots* s, const float* phase) {
    if (!s) return fail(SLM_ERR_ARG, "null spots handle");
    RC(slm::ensure_device());
    s->seq_resumable = false;
    s->u0_valid = false;
    s->custom_phase = phase != nullptr;
    if (!phase) return 0;
    const long long n = (long long)s->B * s->H * s->W;
    // the float32 phase passes through the state buffer on its way to the start field
    RC(up(s, s->phase.p, phase, n * sizeof(float)));
    hipLaunchKernelGGL(spot_phase_kernel, dim3(grid_for(n)), dim3(256), 0, s->stream, s->phase.p, s->u0.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->has_run = false;
    return 0;
}

int slm_spots_set_weights(slm_spots* s, const float* weights) {
    if (!s) return fail(SLM_ERR_ARG, "null spots handle");
    if (!s->M) return fail(SLM_ERR_STATE, "slm_spots_set_weights before slm_spots_set_traps");
    s->seq_resumable = false;
    RC(check_weights(s, s->M, weights));
    RC(slm::ensure_device());
    return upload_weights(s, s->w0.p, weights);
}

int slm_spots_set_feedback(slm_spots* s, float feedback) {
    if (!s) return fail(SLM_ERR_ARG, "null spots handle");
    if (!(feedback >= 0.0f) || !std::isfinite(feedback))
        return fail(SLM_ERR_ARG, "feedback must be finite and >= 0, got %g", (double)feedback);
    s->seq_resumable = false;
    s->feedback = feedback;
    return 0;
}

int slm_spots_run(slm_spots* s, int loops) { return run_loops(s, loops, nullptr); }

int slm_spots_run_timed(slm_spots* s, int loops, double* us_per_class) {
    if (!us_per_class) return fail(SLM_ERR_ARG, "null argument");
    return run_loops(s, loops, us_per_class);
}

int slm_spots_read(slm_spots* s, float* phase, double* fields, double* stats, float* weights) {
    if (!s) return fail(SLM_ERR_ARG, "null spots handle");
    if (!s->has_run) return fail(SLM_ERR_STATE, "slm_spots_read before a run");
    RC(slm::ensure_device());
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (phase) RC(down(s, phase, s->phase.p, (size_t)s->B * s->H * s->W * sizeof(float)));
    if (fields) RC(read_fields(s, s->v.p, s->B, s->M, s->Mp, fields));
    if (stats) {
        std::vector<double> st((size_t)s->B * s->max_loops * 4);
        RC(down(s, st.data(), s->stats.p, st.size() * sizeof(double)));
        for (int b = 0; b < s->B; ++b)
            std::copy_n(&st[(size_t)b * s->max_loops * 4], (size_t)s->last_loops * 4,
                        &stats[(size_t)b * s->last_loops * 4]);
    }
    if (weights) RC(read_weights(s, s->w.p, s->B, s->M, s->Mp, weights));
    return 0;
}

int slm_spots_sequence(slm_spots* s, int n_frames, int n_traps, const double* ys, const double* xs, const double* zs,
                       const float* intensity, const float* weights0, int loops_first, int loops, double tol,
                       int resume, const double* mask, double ct2pi, int rule, int want_frames, int want_phases) {
    if (!s || !ys || !xs) return fail(SLM_ERR_ARG, "null argument");
    if (n_traps < 1 || n_traps > s->max_traps)
        return fail(SLM_ERR_ARG, "%d traps outside 1 .. max_traps %d", n_traps, s->max_traps);
    RC(slm::check_sequence_args(n_frames, loops_first, loops, s->max_loops, tol, rule, ct2pi));
    if (resume && weights0) return fail(SLM_ERR_ARG, "a resumed sequence takes its weights from the previous one");
    const size_t bm_in = (size_t)s->B * n_traps, n = (size_t)n_frames * bm_in;
    RC(check_traps(n, ys, xs, zs, intensity));
    RC(check_weights(s, n_traps, weights0));
    if (s->has_ain && !s->ain_set) return fail(SLM_ERR_STATE, "slm_spots_sequence before slm_spots_set_ain");
    if (resume && !(s->seq_resumable && s->seq_traps == n_traps))
        return fail(SLM_ERR_STATE, "resume needs a previous sequence of %d traps with no set_* or run since", n_traps);
    RC(slm::ensure_device());

    // ---- buffers, sized for this call ----
    const int mp = padded_traps(n_traps), stats_loops = std::max(loops_first, loops);
    const size_t bmp = (size_t)s->B * mp, holo = (size_t)s->H * s->W, F = (size_t)n_frames;
    s->seq_frames = 0;  // nothing to read, and nothing to resume from, if this call fails half way
    s->seq_resumable = false;
    RC(s->seq_coords.need(3 * n * sizeof(double), s->stream));
    RC(s->seq_a_t.need(F * bmp * sizeof(double), s->stream));
    RC(s->seq_w.need((F + 1) * bmp * sizeof(double), s->stream));
    RC(s->seq_v.need(F * bmp * sizeof(double2), s->stream));
    RC(s->seq_stats.need(F * s->B * stats_loops * 4 * sizeof(double), s->stream));
    RC(s->seq_iters.need(F * s->B * sizeof(int), s->stream));
    RC(s->seq_w_last.need((size_t)s->B * padded_traps(s->max_traps) * sizeof(double), s->stream));
    if (want_frames) RC(s->seq_out.need(F * s->B * holo, s->stream));
    if (want_frames && mask) RC(s->seq_mask.need(holo * sizeof(double), s->stream));
    if (want_phases) RC(s->seq_phase.need(F * s->B * holo * sizeof(float), s->stream));
    RC(set_list_size(s, n_traps));

    // ---- everything the chain reads goes up once ----
    const double *dy = s->seq_coords.p, *dx = dy + n, *dz = dx + n;
    RC(upload_coords(s, s->seq_coords.p, n, ys, xs, zs));
    const std::vector<double> a_t = pad(F * s->B, n_traps, mp, 1.0, [&](size_t i) {
        return intensity ? std::sqrt((double)intensity[i]) : 1.0;
    });
    RC(up(s, s->seq_a_t.p, a_t.data(), a_t.size() * sizeof(double)));
    if (resume)
        HIP_TRY(hipMemcpyAsync(s->seq_w.p, s->seq_w_last.p, bmp * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    else
        RC(upload_weights(s, s->seq_w.p, weights0));
    if (want_frames && mask) RC(up(s, s->seq_mask.p, mask, holo * sizeof(double)));
    // the handle's own list becomes the last frame's, its weights ones (the chain reads neither)
    RC(up(s, s->a_t.p, a_t.data() + (F - 1) * bmp, bmp * sizeof(double)));
    RC(upload_weights(s, s->w0.p, nullptr));
    // the stop words start at 0 and the statistics rows a frame does not reach stay 0
    HIP_TRY(hipMemsetAsync(s->seq_iters.p, 0, F * s->B * sizeof(int), s->stream));
    HIP_TRY(hipMemsetAsync(s->seq_stats.p, 0, F * s->B * stats_loops * 4 * sizeof(double), s->stream));

    // ---- the chain: per frame one table launch, then its iterations ----
    Stopwatch untimed;
    for (size_t f = 0; f < F; ++f) {
        RC(launch_tables(s, dy + f * bm_in, dx + f * bm_in, dz + f * bm_in));
        const bool first = f == 0 && !resume;
        if (first) {
            refill_host_a_t(s, a_t.data());
            RC(default_start(s));
        }
        const size_t fb = f * s->B;  // slice f of every sequence buffer, in the order of Frame's fields
        const Frame fr{s->seq_a_t.p + f * bmp, s->seq_w.p + f * bmp, s->seq_w.p + (f + 1) * bmp, s->seq_v.p + f * bmp,
                       s->seq_stats.p + fb * stats_loops * 4, stats_loops, s->seq_iters.p + fb,
                       first ? loops_first : loops, tol,
                       want_phases ? s->seq_phase.p + fb * holo : nullptr,
                       want_frames ? s->seq_out.p + fb * holo : nullptr,
                       want_frames && mask ? s->seq_mask.p : nullptr, ct2pi, rule};
        RC(run_frame(s, fr, first ? s->u0.p : s->u.p, untimed));
    }
    HIP_TRY(hipMemcpyAsync(s->seq_w_last.p, s->seq_w.p + F * bmp, bmp * sizeof(double), hipMemcpyDeviceToDevice,
                           s->stream));

    // ---- the handle is as after slm_spots_set_traps with the last list ----
    refill_host_a_t(s, a_t.data() + (F - 1) * bmp);
    s->u0_valid = false;
    s->has_run = false;
    s->seq_frames = n_frames;
    s->seq_traps = n_traps;
    s->seq_loops = stats_loops;
    s->seq_has_frames = want_frames != 0;
    s->seq_has_phases = want_phases != 0;
    s->seq_resumable = true;
    return 0;
}

int slm_spots_sequence_read(slm_spots* s, unsigned char* frames, float* phases, double* fields, double* stats,
                            float* weights, int* iters) {
    if (!s) return fail(SLM_ERR_ARG, "null spots handle");
    if (!s->seq_frames) return fail(SLM_ERR_STATE, "slm_spots_sequence_read before a sequence");
    if (frames && !s->seq_has_frames) return fail(SLM_ERR_STATE, "the sequence was run without frames");
    if (phases && !s->seq_has_phases) return fail(SLM_ERR_STATE, "the sequence was run without phases");
    RC(slm::ensure_device());
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int mt = s->seq_traps, mp = padded_traps(mt);
    const size_t F = (size_t)s->seq_frames, fb = F * s->B, holo = (size_t)s->H * s->W;
    if (frames) RC(down(s, frames, s->seq_out.p, fb * holo));
    if (phases) RC(down(s, phases, s->seq_phase.p, fb * holo * sizeof(float)));
    if (fields) RC(read_fields(s, s->seq_v.p, fb, mt, mp, fields));
    if (stats) RC(down(s, stats, s->seq_stats.p, fb * s->seq_loops * 4 * sizeof(double)));
    if (weights) RC(read_weights(s, s->seq_w.p + (size_t)s->B * mp, fb, mt, mp, weights));
    if (iters) RC(down(s, iters, s->seq_iters.p, fb * sizeof(int)));
    return 0;
}

int slm_spots_info(slm_spots* s, int* info) {
    if (!s || !info) return fail(SLM_ERR_ARG, "null argument");
    if (!s->M) return fail(SLM_ERR_STATE, "slm_spots_info before slm_spots_set_traps");
    info[0] = s->Mp;
    info[1] = s->units;
    info[2] = s->cols_per_split;
    info[3] = kWaves;
    return 0;
}

int slm_spots_fields(int batch, int height, int width, int n_traps, const double* ys, const double* xs,
                     const double* zs, const float* ain, const float* phase, double* fields_out) {
    if (!phase || !fields_out) return fail(SLM_ERR_ARG, "null argument");
    slm_spots* s = nullptr;
    RC(slm_spots_create(batch, height, width, n_traps, ain != nullptr, 1, &s));
    int rc = slm_spots_set_traps(s, n_traps, ys, xs, zs, nullptr);
    if (!rc && ain) rc = slm_spots_set_ain(s, ain);
    if (!rc) rc = slm_spots_set_phase(s, phase);
    if (!rc) rc = launch_fields(s, s->u0.p, nullptr);
    if (!rc) rc = launch_update(s, own_frame(s, 1), 0);
    if (!rc) {
        s->has_run = true;
        s->last_loops = 1;
        rc = slm_spots_read(s, nullptr, fields_out, nullptr, nullptr);
    }
    slm_spots_destroy(s);
    return rc;
}

int slm_spots_superpose(int batch, int height, int width, int n_traps, const double* ys, const double* xs,
                        const double* zs, const double* c_re_im, float* phase_out) {
    if (!c_re_im || !phase_out) return fail(SLM_ERR_ARG, "null argument");
    slm_spots* s = nullptr;
    RC(slm_spots_create(batch, height, width, n_traps, 0, 1, &s));
    int rc = slm_spots_set_traps(s, n_traps, ys, xs, zs, nullptr);
    if (!rc) {
        const std::vector<float2> c = pad(batch, n_traps, s->Mp, make_float2(0.0f, 0.0f), [&](size_t i) {
            return make_float2((float)c_re_im[2 * i], (float)c_re_im[2 * i + 1]);
        });
        rc = up(s, s->c.p, c.data(), c.size() * sizeof(float2));
    }
    if (!rc) rc = launch_superpose(s, own_frame(s, 1), 0, s->c.p, s->u.p);
    if (!rc) {
        s->has_run = true;
        s->last_loops = 1;
        rc = slm_spots_read(s, phase_out, nullptr, nullptr, nullptr);
    }
    slm_spots_destroy(s);
    return rc;
}

}  // extern "C"
