// Zoomed far field of a hologram (include/slm_hip.h, "zoomed far field";
// DESIGN.md section 3, "Zoomed far field"). No reference counterpart.
//
// The far field on a regular fractional grid y_j = y0 + j dy, x_i = x0 + i dx
// with one defocus z is separable in the trap-list convention (spots.hip):
//     fy_j(k) = 2 pi frac(k y_j / H) + z (k - H/2)^2      (fx_i(l) likewise on l, x_i, W)
//     R[k][i] = sum_l (a u)[k][l] conj(Px[l][i])          zoom_rows_kernel   (H x W)(W x nx)
//     V[j][i] = sum_k conj(Py[k][j]) R[k][i]              zoom_cols_kernel   (ny x H)(H x nx)
//     I[j][i] = |V[j][i]|^2                               zoom_fold_kernel
// with the tables Px[l][i] = exp(i fx_i(l)) and Py[k][j] = exp(i fy_j(k)) in the
// row layout of spots.hip (lanes over samples), nx and ny padded to 32 with
// zero columns, every entry from table_entry (spot_tiles.hpp). Both products
// run on v_mfma_f32_32x32x2_f32 as there: a complex product is four real MFMAs
// per step of two summed indices.
//
// The field a u is formed once per hologram by a pass of its own
// (zoom_field_kernel: the float64 sine and cosine of a float32 phase, or a
// 256-entry table of the uint8 levels, rounded to complex64, times a_in), so
// that the float64 sincos is not repeated by every group of sample tiles and
// the first product stages plain complex64 tiles through LDS (32 x 32, the
// 66-float row stride) exactly as spot_fields_kernel does. The second product
// reads both operands along their fast index and needs no LDS.
//
// Accumulation: no float32 chain is longer than kChunk = 256 summed indices,
// and chunk c is always the pixels [256 c, 256 c + 256) of the summed axis.
// A chunk's result is a float32 number; the chunks are added in float64 from
// zero in their order, wherever that happens. The first product adds them in
// registers and rounds R to complex64 once; while its output tiles are few
// (kSplitBelowWaves) it splits the columns over workgroups instead, one chunk
// each, and zoom_rows_fold_kernel does the same additions from a partial
// buffer. The second product always splits K that way (zoom_fold_kernel), so a
// window of one tile still runs W / 256, then H / 256 workgroups. So there are
// no atomics, and a sample's value depends on its own position and the pixel
// indices alone: never on the window around it, the tile it sits in, whether
// the columns were split, or the batch. The window is worked off in bands of
// whole tile rows that bound the partial buffer.
//
// One host drives the kernels: the resident zoom (slm_zoom_*; DESIGN.md
// section 3, "Resident zoom"). It keeps stream, buffers and tables, takes a
// group of holograms through each launch (a window per hologram if asked),
// takes a correction mask off in the field pass, and reads the frames of a
// sequence in place (seq_frames.hpp), ordered with the sequence's stream by
// events in both directions. By the accumulation rule above neither the group,
// the band nor the split moves a bit. The one-shot (slm_farfield_zoom) is a
// resident zoom of one hologram, created and destroyed by the call, that the
// holograms of the batch pass through one after the other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "runtime.hpp"
#include "seq_frames.hpp"
#include "spot_tiles.hpp"

namespace {

using namespace slm::tiles;

constexpr int kChunk = 256;                 // summed indices per float32 chain, both products
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxSamples = 4096;           // per window side
constexpr size_t kPartialBytes = 64u << 20; // the partial buffer of one band, at most (one tile row always fits)
// first product: fewer output tiles (= waves) than this split the columns, one chunk per workgroup, so
// that the waves spread evenly over the 1024 SIMDs, if the chunk results fit this many bytes
constexpr int kSplitBelowWaves = 4096;
constexpr size_t kRowsPartialBytes = 128u << 20;

// ---- tables ---------------------------------------------------------------
// Every kernel below serves a group of holograms in one launch: the hologram's
// index within the group rides in the grid (blockIdx.y of the element-wise
// kernels, blockIdx.z / units of the products), and a table is reached at
// base + hologram * stride, the stride 0 where the holograms share a window.
// The one-shot launches them with groups of one hologram.

// P[n][s] = exp(i f_s(n)) for sample s < count at pos0 + s pitch, 0 for the padding; [windows][N][padded],
// window blockIdx.y at pos0s[window] with zs[window], or at (pos0, z) where pos0s is null
struct TableParams {
    float2* out;
    const double *pos0s, *zs;  // [windows] on the device, or nullptr
    double pos0, pitch, z;
    int N, count, padded;
};

__global__ void __launch_bounds__(256) zoom_table_kernel(TableParams p) {
    const long long n_el = (long long)p.N * p.padded;
    const double pos0 = p.pos0s ? p.pos0s[blockIdx.y] : p.pos0, z = p.pos0s ? p.zs[blockIdx.y] : p.z;
    float2* out = p.out + (size_t)blockIdx.y * n_el;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n_el; i += (long long)gridDim.x * 256) {
        const int n = (int)(i / p.padded), s = (int)(i - (long long)n * p.padded);
        float2 v = make_float2(0.0f, 0.0f);
        // pos0 + s pitch with the product rounded before the sum (no contraction into an fma)
        if (s < p.count) v = table_entry(n, p.N, __dadd_rn(pos0, __dmul_rn((double)s, p.pitch)), z);
        out[i] = v;
    }
}

// ---- the field a u --------------------------------------------------------
// kind SLM_ZOOM_PHASE_F32: u = float64 sincos of the float32 phase, as spot_phase_kernel forms it;
// SLM_ZOOM_LEVELS_U8: u = levels[level], the 256 entries evaluated in float64 on the host.
// With a correction mask (the resident zoom): u = float64 sincos of t - mask, one rounded float64
// subtraction, t = (double)phase or level_t[level] = 2 pi level / ct2pi as the level table forms it.
struct FieldParams {
    const void* holo;       // [holograms][H][W] float32 or uint8
    const float* ain;       // [H][W] or nullptr
    const double* mask;     // [H][W] or nullptr
    const float2* levels;   // [256], levels without a mask
    const double* level_t;  // [256], levels with a mask
    float2* field;          // [holograms][H][W]
    long long n;            // H W
    int kind;
};

__global__ void __launch_bounds__(256) zoom_field_kernel(FieldParams p) {
    const size_t base = (size_t)blockIdx.y * p.n;
    const uint8_t* lv = static_cast<const uint8_t*>(p.holo) + base;
    const float* ph = static_cast<const float*>(p.holo) + base;
    float2* field = p.field + base;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < p.n; i += (long long)gridDim.x * 256) {
        float2 u;
        if (p.mask) {
            const double t = p.kind == SLM_ZOOM_LEVELS_U8 ? p.level_t[lv[i]] : (double)ph[i];
            double s, c;
            sincos(__dsub_rn(t, p.mask[i]), &s, &c);
            u = make_float2((float)c, (float)s);
        } else if (p.kind == SLM_ZOOM_LEVELS_U8) {
            u = p.levels[lv[i]];
        } else {
            double s, c;
            sincos((double)ph[i], &s, &c);
            u = make_float2((float)c, (float)s);
        }
        const float a = p.ain ? p.ain[i] : 1.0f;
        field[i] = make_float2(u.x * a, u.y * a);
    }
}

// ---- product 1: R = (a u) conj(Px) ----------------------------------------
struct RowsParams {
    const float2* field;  // [holograms][H][W]
    const float2* px;     // [W][nxp] of the group's first hologram
    float2* out;          // R [holograms][H][nxp], or with a split the chunk results [holograms][chunks][H][nxp]
    size_t px_stride;     // elements between the tables of two holograms (0: shared)
    int H, W, nxp;
    int cols_per_unit;    // columns per unit: all of them, or with a split one chunk
    int units;            // units per hologram: blockIdx.z = hologram * units + unit
};

// One workgroup per 32 rows x 128 samples: its four waves share the staged
// field tiles (two LDS buffers, filled in turn: one barrier per tile) and take
// one 32-sample tile each. A wave past the last sample tile only helps to
// stage. A window of few sample tiles splits the columns over workgroups, one
// chunk each, and zoom_rows_fold_kernel adds the chunk results as this kernel
// adds them in its registers otherwise: R is the same bit for bit either way.
// grid = (groups of 4 sample tiles, row tiles, holograms x (1 or chunks)).
__global__ void __launch_bounds__(kThreads) zoom_rows_kernel(RowsParams p) {
    __shared__ float tiles[2][kTile * kLdsStride];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int row0 = blockIdx.y * kTile, s0 = (blockIdx.x * kWaves + wave) * kTile;
    const bool active = s0 < p.nxp;
    const int holo = blockIdx.z / p.units, unit = blockIdx.z - holo * p.units;
    const int c_begin = unit * p.cols_per_unit, c_end = min(p.W, c_begin + p.cols_per_unit);
    const float2* field = p.field + (size_t)holo * p.H * p.W;
    const float2* px = p.px + (size_t)holo * p.px_stride + (active ? s0 : 0) + li;

    f32x16 are, aim;
    double dre[16], dim[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        are[r] = aim[r] = 0.0f;
        dre[r] = dim[r] = 0.0;
    }

    // thread t stages elements t, t + 256, t + 512, t + 768 of the 32 x 32 tile: 8 rows apart, column t & 31
    const int tr = threadIdx.x >> 5, tc = threadIdx.x & 31;
    float2 ft[4];
    auto load_tile = [&](int c0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int gr = row0 + tr + 8 * e, gc = c0 + tc;
            ft[e] = make_float2(0.0f, 0.0f);
            if (gr < p.H && gc < p.W) ft[e] = field[(size_t)gr * p.W + gc];
        }
    };
    constexpr int kSteps = kTile / 2;  // a step = 2 columns
    // lane (i, h): Px of column c0 + 2 s + h; columns past the edge read the last one (their field is zero)
    float2 q[kSteps], qn[kSteps];
    auto load_q = [&](float2(&qq)[kSteps], int c0) {
#pragma unroll
        for (int s = 0; s < kSteps; ++s) qq[s] = px[(size_t)min(c0 + 2 * s + lh, p.W - 1) * p.nxp];
    };

    // registers carry the next field tile and the next tile's table rows while the matrix cores work on this one
    load_tile(c_begin);
    load_q(q, c_begin);
    int buf = 0;
    for (int c0 = c_begin; c0 < c_end; c0 += kTile, buf ^= 1) {
        float* tile = tiles[buf];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            *reinterpret_cast<float2*>(&tile[(tr + 8 * e) * kLdsStride + 2 * tc]) = ft[e];
        __syncthreads();
        load_tile(c0 + kTile);  // past c_end: read by nobody
        if (active) {
            load_q(qn, c0 + kTile);
#pragma unroll
            for (int s = 0; s < kSteps; ++s) {
                // lane (k, h): pixel (row0 + k, c0 + 2 s + h)
                const float2 a = *reinterpret_cast<const float2*>(&tile[li * kLdsStride + 4 * s + 2 * lh]);
                are = mfma(a.x, q[s].x, are);
                aim = mfma(a.x, -q[s].y, aim);
                are = mfma(a.y, q[s].y, are);
                aim = mfma(a.y, q[s].x, aim);
            }
            // the end of a 256-column chunk (or of the row): fold the float32 chain into float64
            if (((c0 + kTile) & (kChunk - 1)) == 0 || c0 + kTile >= c_end) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dre[r] += (double)are[r];
                    dim[r] += (double)aim[r];
                    are[r] = aim[r] = 0.0f;
                }
            }
#pragma unroll
            for (int s = 0; s < kSteps; ++s) q[s] = qn[s];
        }
    }
    if (!active) return;
    float2* out = p.out + (size_t)blockIdx.z * p.H * p.nxp + s0 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gr = row0 + acc_row(r, lh);
        if (gr < p.H) out[(size_t)gr * p.nxp] = make_float2((float)dre[r], (float)dim[r]);
    }
}

// R = the chunk results of a split first product, added in float64 in their order and rounded once;
// partial [holograms][chunks][n], r [holograms][n], hologram blockIdx.y
__global__ void __launch_bounds__(256) zoom_rows_fold_kernel(const float2* partial, float2* r, int chunks,
                                                             long long n) {
    partial += (size_t)blockIdx.y * chunks * n;
    r += (size_t)blockIdx.y * n;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        double re = 0.0, im = 0.0;
        for (int c = 0; c < chunks; ++c) {
            const float2 t = partial[(size_t)c * n + e];
            re += (double)t.x;
            im += (double)t.y;
        }
        r[e] = make_float2((float)re, (float)im);
    }
}

// ---- product 2: V chunks = conj(Py) R -------------------------------------
struct ColsParams {
    const float2* py;  // [H][nyp] of the group's first hologram
    const float2* r;   // [holograms][H][nxp]
    float2* partial;   // [holograms][chunks][band rows][nxp]
    size_t py_stride;  // elements between the tables of two holograms (0: shared)
    int H, nyp, nxp;
    int j0, band_rows;  // this band: sample rows j0 .. j0 + band_rows (a multiple of 32)
    int chunks;         // per hologram: blockIdx.z = hologram * chunks + chunk
};

// One wave per 32 x 32 output tile and chunk of 256 pixel rows, four adjacent
// column tiles per workgroup; no barriers. grid = (column tiles / 4, the band's row tiles, holograms x chunks).
__global__ void __launch_bounds__(kThreads) zoom_cols_kernel(ColsParams p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int i0 = (blockIdx.x * kWaves + wave) * kTile, jb = blockIdx.y * kTile;
    const int holo = blockIdx.z / p.chunks, chunk = blockIdx.z - holo * p.chunks;
    if (i0 >= p.nxp) return;
    const int k0 = chunk * kChunk;
    const float2* py = p.py + (size_t)holo * p.py_stride + p.j0 + jb + li;
    const float2* rr = p.r + (size_t)holo * p.H * p.nxp + i0 + li;
    f32x16 vre, vim;
#pragma unroll
    for (int r = 0; r < 16; ++r) vre[r] = vim[r] = 0.0f;
    // Groups of 8 steps = 16 pixel rows; the next group's rows are in flight while the matrix
    // cores work on this one. Rows past H read the last row and enter as conj(Py) = 0.
    constexpr int kGroup = 8, kGroups = kChunk / (2 * kGroup);
    float2 y[kGroup], b[kGroup], yn[kGroup], bn[kGroup];
    auto load = [&](float2(&yy)[kGroup], float2(&bb)[kGroup], int g) {
#pragma unroll
        for (int s = 0; s < kGroup; ++s) {
            const int k = k0 + 2 * (kGroup * g + s) + lh, kc = min(k, p.H - 1);
            yy[s] = py[(size_t)kc * p.nyp];
            bb[s] = rr[(size_t)kc * p.nxp];
            if (k >= p.H) yy[s] = make_float2(0.0f, 0.0f);
        }
    };
    load(y, b, 0);
    for (int g = 0; g < kGroups; ++g) {
        if (k0 + 2 * kGroup * g >= p.H) break;  // the same for the whole wave
        if (g + 1 < kGroups) load(yn, bn, g + 1);
#pragma unroll
        for (int s = 0; s < kGroup; ++s) {
            // conj(y) b = (y.x b.x + y.y b.y) + i (y.x b.y - y.y b.x)
            vre = mfma(y[s].x, b[s].x, vre);
            vim = mfma(y[s].x, b[s].y, vim);
            vre = mfma(y[s].y, b[s].y, vre);
            vim = mfma(-y[s].y, b[s].x, vim);
        }
#pragma unroll
        for (int s = 0; s < kGroup; ++s) {
            y[s] = yn[s];
            b[s] = bn[s];
        }
    }
    float2* out = p.partial + ((size_t)blockIdx.z * p.band_rows + jb) * p.nxp + i0 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(size_t)acc_row(r, lh) * p.nxp] = make_float2(vre[r], vim[r]);
}

// ---- fold: V = the chunks added in float64 in their order, I = |V|^2 ------
struct FoldParams {
    const float2* partial;  // [holograms][chunks][band rows][nxp]
    float* intensity;       // the band's [rows][nx] of the group's first hologram
    double2* v;             // likewise, or nullptr
    size_t out_stride;      // elements between the outputs of two holograms
    int chunks, band_rows, rows, nx, nxp;  // rows = the band's samples that exist (<= band_rows)
};

// hologram blockIdx.y
__global__ void __launch_bounds__(256) zoom_fold_kernel(FoldParams p) {
    const long long n = (long long)p.rows * p.nx;
    const float2* partial = p.partial + (size_t)blockIdx.y * p.chunks * p.band_rows * p.nxp;
    float* intensity = p.intensity + blockIdx.y * p.out_stride;
    double2* v = p.v ? p.v + blockIdx.y * p.out_stride : nullptr;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int j = (int)(e / p.nx), i = (int)(e - (long long)j * p.nx);
        double vr = 0.0, vi = 0.0;
        for (int c = 0; c < p.chunks; ++c) {
            const float2 t = partial[((size_t)c * p.band_rows + j) * p.nxp + i];
            vr += (double)t.x;
            vi += (double)t.y;
        }
        intensity[e] = (float)(vr * vr + vi * vi);
        if (v) v[e] = make_double2(vr, vi);
    }
}

int padded(int n) { return (n + kTile - 1) / kTile * kTile; }

}  // namespace

using slm::DevBuf;
using slm::fail;
using slm::grid_for;

// ---- the resident zoom ----------------------------------------------------
// Stream, buffers and tables stay with the handle; a run enqueues groups of
// holograms back to back and returns, slm_zoom_read waits.
struct slm_zoom {
    int B = 0, H = 0, W = 0, max_ny = 0, max_nx = 0;
    size_t cols_cap = 0, rows_cap = 0;  // the partial buffers of a band of product 2 and of a split product 1, at most
    hipStream_t stream = nullptr;
    hipEvent_t frames_written = nullptr, frames_read = nullptr;  // the two orderings with a sequence's stream
    hipEvent_t levels_landed = nullptr;                          // the last upload from level_host
    DevBuf<float> ain;
    DevBuf<double> mask, level_t, origins;  // origins: y0 [B], x0 [B], z [B]
    DevBuf<float2> levels, px, py, field, r, partial;
    DevBuf<uint8_t> holo;
    DevBuf<float> intensity;
    DevBuf<double2> v;
    // the level tables, their pinned source and its event come with the first run on levels
    void* level_host = nullptr;  // pinned: float2 [256], then double [256]
    double level_ct2pi = 0.0;    // what the level tables on the device were built for (0: nothing)
    bool ain_set = false, mask_set = false, window_set = false, per_hologram = false, timed = false;
    int ny = 0, nx = 0;
    // the last run
    bool ran = false, ran_field = false, ran_timed = false;
    int ran_count = 0, ran_ny = 0, ran_nx = 0, groups = 0, bands = 0, split_launches = 0;
    slm::Stopwatch watch, table_watch;  // the last run's kernels; the last window's two table launches
};

namespace {

// ---- argument checks, shared by the handle's entry points and the one-shot --
int check_kind(int kind) {
    if (kind != SLM_ZOOM_PHASE_F32 && kind != SLM_ZOOM_LEVELS_U8) return fail(SLM_ERR_ARG, "unknown kind %d", kind);
    return 0;
}
int check_sides(int height, int width) {
    if (height < kMinSide || width < kMinSide || height > kMaxSide || width > kMaxSide)
        return fail(SLM_ERR_ARG, "the zoom runs on sides %d .. %d, got %d x %d", kMinSide, kMaxSide, height, width);
    return 0;
}
int check_samples(int ny, int nx) {
    if (ny < 1 || nx < 1 || ny > kMaxSamples || nx > kMaxSamples)
        return fail(SLM_ERR_ARG, "a window has 1 .. %d samples per side, got %d x %d", kMaxSamples, ny, nx);
    return 0;
}
// the origins and defocus of `windows` windows and their pitch: finite, the pitch positive
int check_positions(int windows, const double* y0, const double* x0, const double* z, double dy, double dx) {
    bool finite = std::isfinite(dy) && std::isfinite(dx);
    for (int i = 0; i < windows; ++i) finite = finite && std::isfinite(y0[i]) && std::isfinite(x0[i]) && std::isfinite(z[i]);
    if (!finite) return fail(SLM_ERR_ARG, "the window's origin, pitch and defocus must be finite");
    if (!(dy > 0.0) || !(dx > 0.0)) return fail(SLM_ERR_ARG, "the pitch must be positive, got %g x %g", dy, dx);
    return 0;
}
int check_ct2pi(int kind, double ct2pi) {
    if (kind == SLM_ZOOM_LEVELS_U8 && (!(ct2pi > 0.0) || !std::isfinite(ct2pi)))
        return fail(SLM_ERR_ARG, "ct2pi must be finite and positive, got %g", ct2pi);
    return 0;
}

int launch_table(hipStream_t st, float2* out, int windows, int N, int count, int padded_count, const double* pos0s,
                 const double* zs, double pos0, double pitch, double z) {
    const TableParams tp{out, pos0s, zs, pos0, pitch, z, N, count, padded_count};
    hipLaunchKernelGGL(zoom_table_kernel, dim3(grid_for((long long)N * padded_count), windows), dim3(256), 0, st, tp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- one group of holograms through the five kernels ----------------------
// How a run is cut: the padded window, the band, and the tables' strides (0: one window for all).
struct Cut {
    int kind, nyp, nxp, band_rows;
    size_t px_stride, py_stride;
};

// product 1 of `n` holograms in one launch splits its columns if the launch's output tiles are few
bool splits_rows(const slm_zoom* zm, const Cut& q, int n) {
    const int row_tiles = (zm->H + kTile - 1) / kTile, wchunks = (zm->W + kChunk - 1) / kChunk;
    const size_t r_bytes = (size_t)zm->H * q.nxp * sizeof(float2);
    return wchunks > 1 && (long long)n * row_tiles * (q.nxp / kTile) < kSplitBelowWaves &&
           (size_t)n * wchunks * r_bytes <= zm->rows_cap;
}

// `n` holograms at `holo` (device, [n][H][W]), the first of them hologram `first` of the run: the field, R,
// and band by band V and I into the run's outputs, which hold the whole window of every hologram (a band's
// fold enters them at its row j0). Everything is enqueued; nothing waits.
int enqueue_group(slm_zoom* zm, const Cut& q, const void* holo, int first, int n, bool want_field) {
    const hipStream_t st = zm->stream;
    const int H = zm->H, W = zm->W, ny = zm->ny, nx = zm->nx;
    const long long holo_n = (long long)H * W;
    const size_t window = (size_t)ny * nx;
    const int chunks = (H + kChunk - 1) / kChunk, wchunks = (W + kChunk - 1) / kChunk;
    const int row_tiles = (H + kTile - 1) / kTile, sample_groups = (q.nxp / kTile + kWaves - 1) / kWaves;
    float* intensity = zm->intensity.p + first * window;
    double2* v = want_field ? zm->v.p + first * window : nullptr;

    RC(zm->watch.begin(SLM_ZOOM_KERNEL_FIELD, st));
    const FieldParams fp{holo, zm->ain_set ? zm->ain.p : nullptr, zm->mask_set ? zm->mask.p : nullptr, zm->levels.p,
                         zm->level_t.p, zm->field.p, holo_n, q.kind};
    hipLaunchKernelGGL(zoom_field_kernel, dim3(grid_for(holo_n), n), dim3(256), 0, st, fp);
    HIP_TRY(hipGetLastError());
    RC(zm->watch.end(st));

    RC(zm->watch.begin(SLM_ZOOM_KERNEL_ROWS, st));
    const bool split = splits_rows(zm, q, n);
    const int units = split ? wchunks : 1;
    const RowsParams rp{zm->field.p, zm->px.p + (size_t)first * q.px_stride, split ? zm->partial.p : zm->r.p,
                        q.px_stride, H, W, q.nxp, split ? kChunk : wchunks * kChunk, units};
    hipLaunchKernelGGL(zoom_rows_kernel, dim3(sample_groups, row_tiles, n * units), dim3(kThreads), 0, st, rp);
    HIP_TRY(hipGetLastError());
    if (split) {
        const long long r_el = (long long)H * q.nxp;
        hipLaunchKernelGGL(zoom_rows_fold_kernel, dim3(grid_for(r_el), n), dim3(256), 0, st, zm->partial.p, zm->r.p,
                           wchunks, r_el);
        HIP_TRY(hipGetLastError());
        ++zm->split_launches;
    }
    RC(zm->watch.end(st));

    for (int j0 = 0; j0 < ny; j0 += q.band_rows) {
        const int tile_rows = std::min(q.band_rows, q.nyp - j0), rows = std::min(q.band_rows, ny - j0);
        RC(zm->watch.begin(SLM_ZOOM_KERNEL_COLS, st));
        const ColsParams cp{zm->py.p + (size_t)first * q.py_stride, zm->r.p, zm->partial.p, q.py_stride, H, q.nyp,
                            q.nxp, j0, q.band_rows, chunks};
        hipLaunchKernelGGL(zoom_cols_kernel, dim3(sample_groups, tile_rows / kTile, n * chunks), dim3(kThreads), 0, st,
                           cp);
        HIP_TRY(hipGetLastError());
        const size_t at = (size_t)j0 * nx;
        const FoldParams fo{zm->partial.p, intensity + at, v ? v + at : nullptr, window, chunks, q.band_rows, rows, nx,
                            q.nxp};
        hipLaunchKernelGGL(zoom_fold_kernel, dim3(grid_for((long long)rows * nx), n), dim3(256), 0, st, fo);
        HIP_TRY(hipGetLastError());
        RC(zm->watch.end(st));
    }
    return 0;
}

// bytes of the partial buffer a group of n holograms needs
size_t partial_bytes(const slm_zoom* zm, const Cut& q, int n) {
    const int chunks = (zm->H + kChunk - 1) / kChunk, wchunks = (zm->W + kChunk - 1) / kChunk;
    const size_t cols = (size_t)n * chunks * q.band_rows * q.nxp * sizeof(float2);
    const size_t rows = splits_rows(zm, q, n) ? (size_t)n * wchunks * zm->H * q.nxp * sizeof(float2) : 0;
    return std::max(cols, rows);
}

// the band of n holograms: whole tile rows whose chunk results fit `cap` (one tile row always fits)
int band_rows_for(int H, int nyp, int nxp, size_t cap, int n) {
    const size_t row_bytes = (size_t)n * ((H + kChunk - 1) / kChunk) * nxp * sizeof(float2);
    return (int)std::min<size_t>(nyp, std::max<size_t>(kTile, cap / row_bytes / kTile * kTile));
}

// ---- the handle's own host code -------------------------------------------
constexpr int kMaxBatch = 1024;
// the field of one group, at most: with windows of a few tiles the partial caps alone would admit hundreds
// of holograms of any size
constexpr size_t kGroupFieldBytes = 1u << 30;

void zoom_free(slm_zoom* zm) {
    if (!zm) return;
    if (zm->stream) (void)hipStreamSynchronize(zm->stream);
    for (hipEvent_t e : {zm->frames_written, zm->frames_read, zm->levels_landed})
        if (e) (void)hipEventDestroy(e);
    if (zm->level_host) (void)hipHostFree(zm->level_host);
    if (zm->stream) (void)hipStreamDestroy(zm->stream);
    delete zm;
}

// a handle of checked sizes with the two caps of its partial buffers
int zoom_create(int batch, int height, int width, int max_ny, int max_nx, size_t cols_cap, size_t rows_cap,
                slm_zoom** out) {
    RC(slm::ensure_device());
    slm_zoom* zm = new slm_zoom;
    zm->B = batch;
    zm->H = height;
    zm->W = width;
    zm->max_ny = max_ny;
    zm->max_nx = max_nx;
    zm->cols_cap = cols_cap;
    zm->rows_cap = rows_cap;
    int rc = [&]() {
        HIP_TRY(hipStreamCreateWithFlags(&zm->stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&zm->frames_written, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&zm->frames_read, hipEventDisableTiming));
        return 0;
    }();
    if (rc) {
        zoom_free(zm);
        return rc;
    }
    *out = zm;
    return 0;
}

// a checked a_in (nullptr = ones)
int zoom_put_ain(slm_zoom* zm, const float* ain) {
    const size_t holo = (size_t)zm->H * zm->W;
    RC(slm::ensure_device());
    zm->ain_set = false;
    if (!ain) return 0;
    RC(zm->ain.need(holo * sizeof(float), zm->stream));
    RC(slm::copy_sync(zm->ain.p, ain, holo * sizeof(float), hipMemcpyHostToDevice, zm->stream));
    zm->ain_set = true;
    return 0;
}

// a checked window: its tables
int zoom_put_window(slm_zoom* zm, int per_hologram, const double* y0, const double* x0, const double* z, double dy,
                    double dx, int ny, int nx) {
    RC(slm::ensure_device());
    const hipStream_t st = zm->stream;
    const int windows = per_hologram ? zm->B : 1, nxp = padded(nx), nyp = padded(ny);
    zm->window_set = false;
    RC(zm->px.need((size_t)windows * zm->W * nxp * sizeof(float2), st));
    RC(zm->py.need((size_t)windows * zm->H * nyp * sizeof(float2), st));
    const double *dev_y0 = nullptr, *dev_x0 = nullptr, *dev_z = nullptr;
    if (per_hologram) {
        RC(zm->origins.need(3 * (size_t)windows * sizeof(double), st));
        dev_y0 = zm->origins.p;
        dev_x0 = dev_y0 + windows;
        dev_z = dev_x0 + windows;
        const size_t bytes = (size_t)windows * sizeof(double);
        RC(slm::copy_sync(zm->origins.p, y0, bytes, hipMemcpyHostToDevice, st));
        RC(slm::copy_sync(zm->origins.p + windows, x0, bytes, hipMemcpyHostToDevice, st));
        RC(slm::copy_sync(zm->origins.p + 2 * windows, z, bytes, hipMemcpyHostToDevice, st));
    }
    zm->table_watch.reset(zm->timed);
    RC(zm->table_watch.begin(SLM_ZOOM_KERNEL_TABLES, st));
    RC(launch_table(st, zm->px.p, windows, zm->W, nx, nxp, dev_x0, dev_z, x0[0], dx, z[0]));
    RC(launch_table(st, zm->py.p, windows, zm->H, ny, nyp, dev_y0, dev_z, y0[0], dy, z[0]));
    RC(zm->table_watch.end(st));
    zm->per_hologram = per_hologram != 0;
    zm->ny = ny;
    zm->nx = nx;
    zm->window_set = true;
    return 0;
}

// the 256 level phases t = 2 pi level / ct2pi and their u, evaluated in float64 on the host and uploaded
int upload_levels(slm_zoom* zm, double ct2pi) {
    const hipStream_t st = zm->stream;
    if (!zm->levels_landed) HIP_TRY(hipEventCreateWithFlags(&zm->levels_landed, hipEventDisableTiming));
    RC(zm->levels.need(256 * sizeof(float2), st));
    RC(zm->level_t.need(256 * sizeof(double), st));
    if (!zm->level_host)
        HIP_TRY(hipHostMalloc(&zm->level_host, 256 * (sizeof(float2) + sizeof(double)), hipHostMallocDefault));
    // the pinned tables are written only after their last upload has left them
    HIP_TRY(hipEventSynchronize(zm->levels_landed));
    float2* levels = static_cast<float2*>(zm->level_host);
    double* level_t = reinterpret_cast<double*>(levels + 256);
    for (int v = 0; v < 256; ++v) {
        const double t = kTwoPi * (double)v / ct2pi;
        levels[v] = make_float2((float)std::cos(t), (float)std::sin(t));
        level_t[v] = t;
    }
    zm->level_ct2pi = 0.0;
    HIP_TRY(hipMemcpyAsync(zm->levels.p, levels, 256 * sizeof(float2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(zm->level_t.p, level_t, 256 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(zm->levels_landed, st));
    zm->level_ct2pi = ct2pi;
    return 0;
}

// holograms per group and the band of a run of `count`: as many holograms as keep the second product's
// partials of the whole window within the cap (and the field within kGroupFieldBytes), spread evenly over
// the groups; a window whose partials exceed the cap for one hologram runs hologram by hologram in bands
void cut_run(const slm_zoom* zm, int count, int* group, int* band_rows) {
    const int nyp = padded(zm->ny), nxp = padded(zm->nx);
    const size_t whole = (size_t)((zm->H + kChunk - 1) / kChunk) * nyp * nxp * sizeof(float2);
    size_t g = 1;
    if (whole <= zm->cols_cap) {
        g = std::min(zm->cols_cap / whole, std::max<size_t>(1, kGroupFieldBytes / ((size_t)zm->H * zm->W * 8)));
        g = std::min<size_t>(g, count);
        const size_t n_groups = (count + g - 1) / g;
        g = (count + n_groups - 1) / n_groups;
    }
    *group = (int)g;
    *band_rows = band_rows_for(zm->H, nyp, nxp, zm->cols_cap, (int)g);
}

// `count` holograms already on the device (levels or phases), on the handle's stream. `writer`, if not
// null, is the stream that writes `dev_holo`: its later work waits for this run.
int zoom_enqueue(slm_zoom* zm, const void* dev_holo, int kind, int count, double ct2pi, int want_field,
                 hipStream_t writer) {
    const hipStream_t st = zm->stream;
    const int nxp = padded(zm->nx), nyp = padded(zm->ny);
    const size_t holo = (size_t)zm->H * zm->W, el = kind == SLM_ZOOM_LEVELS_U8 ? 1 : sizeof(float);
    const size_t window = (size_t)zm->ny * zm->nx;
    zm->ran = false;
    if (kind == SLM_ZOOM_LEVELS_U8 && ct2pi != zm->level_ct2pi) RC(upload_levels(zm, ct2pi));
    int group = 1, band_rows = kTile;
    cut_run(zm, count, &group, &band_rows);
    const Cut q{kind, nyp, nxp, band_rows, zm->per_hologram ? (size_t)zm->W * nxp : 0,
                zm->per_hologram ? (size_t)zm->H * nyp : 0};
    const int last = count - (count - 1) / group * group;  // the last group's holograms
    RC(zm->field.need((size_t)group * holo * sizeof(float2), st));
    RC(zm->r.need((size_t)group * zm->H * nxp * sizeof(float2), st));
    RC(zm->partial.need(std::max(partial_bytes(zm, q, group), partial_bytes(zm, q, last)), st));
    RC(zm->intensity.need((size_t)count * window * sizeof(float), st));
    if (want_field) RC(zm->v.need((size_t)count * window * sizeof(double2), st));

    zm->watch.reset(zm->timed);
    zm->groups = zm->split_launches = 0;
    zm->bands = (zm->ny + band_rows - 1) / band_rows;
    for (int first = 0; first < count; first += group, ++zm->groups)
        RC(enqueue_group(zm, q, static_cast<const uint8_t*>(dev_holo) + (size_t)first * holo * el, first,
                         std::min(group, count - first), want_field != 0));
    if (writer) {
        // the source's next write to its frames comes after this run's reads
        HIP_TRY(hipEventRecord(zm->frames_read, st));
        HIP_TRY(hipStreamWaitEvent(writer, zm->frames_read, 0));
    }
    zm->ran = true;
    zm->ran_field = want_field != 0;
    zm->ran_timed = zm->timed;
    zm->ran_count = count;
    zm->ran_ny = zm->ny;
    zm->ran_nx = zm->nx;
    return 0;
}

int check_run(const slm_zoom* zm, int kind, int count, double ct2pi) {
    if (!zm) return fail(SLM_ERR_ARG, "null zoom handle");
    RC(check_kind(kind));
    if (count < 1 || count > zm->B)
        return fail(SLM_ERR_ARG, "a run takes 1 .. %d holograms (the handle's batch), got %d", zm->B, count);
    RC(check_ct2pi(kind, ct2pi));
    if (!zm->window_set) return fail(SLM_ERR_STATE, "slm_zoom_run before slm_zoom_set_window");
    return 0;
}

// holograms [first, first + count) of a sequence's frames, ordered after the chain that writes them
int zoom_run_frames(slm_zoom* zm, const slm::SeqFrames& src, const char* what, int first, int count, double ct2pi,
                    int want_field) {
    if (!src.n) return fail(SLM_ERR_STATE, "%s before a sequence", what);
    if (!src.frames) return fail(SLM_ERR_STATE, "the sequence was run without frames");
    if (src.H != zm->H || src.W != zm->W)
        return fail(SLM_ERR_ARG, "the frames are %d x %d, the zoom handle's holograms %d x %d", src.H, src.W, zm->H,
                    zm->W);
    if (first < 0 || count < 1 || first > src.n - count)
        return fail(SLM_ERR_ARG, "frames %d .. %d lie outside the sequence's %d", first, first + count - 1, src.n);
    RC(check_run(zm, SLM_ZOOM_LEVELS_U8, count, ct2pi));
    RC(slm::ensure_device());
    HIP_TRY(hipEventRecord(zm->frames_written, src.stream));
    HIP_TRY(hipStreamWaitEvent(zm->stream, zm->frames_written, 0));
    return zoom_enqueue(zm, src.frames + (size_t)first * zm->H * zm->W, SLM_ZOOM_LEVELS_U8, count, ct2pi, want_field,
                        src.stream);
}

}  // namespace

extern "C" {

// The one-shot: a resident zoom of one hologram that lives for the call. Everything is checked before the
// handle is created; the holograms of the batch go through it one after the other.
int slm_farfield_zoom_timed(const void* hologram, int kind, int batch, int height, int width, const float* ain,
                            double ct2pi, double y0, double x0, double dy, double dx, int ny, int nx, double z,
                            float* intensity, double* field, double* kernel_us) {
    if (!hologram || !intensity) return fail(SLM_ERR_ARG, "null argument");
    RC(check_kind(kind));
    if (batch < 1) return fail(SLM_ERR_ARG, "batch must be positive, got %d", batch);
    RC(check_sides(height, width));
    RC(check_samples(ny, nx));
    RC(check_positions(1, &y0, &x0, &z, dy, dx));
    RC(check_ct2pi(kind, ct2pi));
    const size_t holo = (size_t)height * width, window = (size_t)ny * nx;
    RC(slm::check_ain(ain, holo, nullptr));
    slm_zoom* zm = nullptr;
    RC(zoom_create(1, height, width, ny, nx, kPartialBytes, kRowsPartialBytes, &zm));  // never the environment's caps
    const int rc = [&]() {
        constexpr int kClasses = SLM_ZOOM_NUM_KERNEL_CLASSES;
        double us[kClasses], total[kClasses] = {};
        zm->timed = kernel_us != nullptr;
        RC(zoom_put_ain(zm, ain));
        RC(zoom_put_window(zm, 0, &y0, &x0, &z, dy, dx, ny, nx));
        const size_t holo_bytes = holo * (kind == SLM_ZOOM_LEVELS_U8 ? 1 : sizeof(float));
        for (int b = 0; b < batch; ++b) {
            RC(slm_zoom_run(zm, static_cast<const uint8_t*>(hologram) + b * holo_bytes, kind, 1, ct2pi,
                            field != nullptr));
            RC(slm_zoom_read(zm, intensity + b * window, field ? field + 2 * b * window : nullptr,
                             kernel_us ? us : nullptr));
            for (int c = 0; kernel_us && c < kClasses; ++c) total[c] += us[c];
        }
        if (!kernel_us) return 0;
        RC(zm->table_watch.read(us, kClasses));  // the reads above have waited for the stream
        for (int c = 0; c < kClasses; ++c) kernel_us[c] = total[c] + us[c];
        return 0;
    }();
    zoom_free(zm);
    return rc;
}

int slm_farfield_zoom(const void* hologram, int kind, int batch, int height, int width, const float* ain, double ct2pi,
                      double y0, double x0, double dy, double dx, int ny, int nx, double z, float* intensity,
                      double* field) {
    return slm_farfield_zoom_timed(hologram, kind, batch, height, width, ain, ct2pi, y0, x0, dy, dx, ny, nx, z,
                                   intensity, field, nullptr);
}

int slm_zoom_create(int batch, int height, int width, int max_ny, int max_nx, slm_zoom** out) {
    if (!out) return fail(SLM_ERR_ARG, "null argument");
    *out = nullptr;
    if (batch < 1 || batch > kMaxBatch)
        return fail(SLM_ERR_ARG, "a zoom handle takes 1 .. %d holograms per run, got %d", kMaxBatch, batch);
    RC(check_sides(height, width));
    RC(check_samples(max_ny, max_nx));
    size_t cols_cap = kPartialBytes, rows_cap = kRowsPartialBytes;
    if (const char* env = std::getenv("SLM_ZOOM_PARTIAL_BYTES")) {
        char* end = nullptr;
        const long long v = std::strtoll(env, &end, 10);
        if (end == env || *end || v < 1)
            return fail(SLM_ERR_ARG, "$SLM_ZOOM_PARTIAL_BYTES must be a positive whole number, got \"%s\"", env);
        cols_cap = rows_cap = (size_t)v;
    }
    return zoom_create(batch, height, width, max_ny, max_nx, cols_cap, rows_cap, out);
}

int slm_zoom_destroy(slm_zoom* zm) {
    if (zm) (void)slm::ensure_device();
    zoom_free(zm);
    return 0;
}

int slm_zoom_set_ain(slm_zoom* zm, const float* ain) {
    if (!zm) return fail(SLM_ERR_ARG, "null zoom handle");
    RC(slm::check_ain(ain, (size_t)zm->H * zm->W, nullptr));
    return zoom_put_ain(zm, ain);
}

int slm_zoom_set_mask(slm_zoom* zm, const double* mask) {
    if (!zm) return fail(SLM_ERR_ARG, "null zoom handle");
    const size_t holo = (size_t)zm->H * zm->W;
    for (size_t i = 0; mask && i < holo; ++i)
        if (!std::isfinite(mask[i])) return fail(SLM_ERR_ARG, "the mask has a non-finite entry");
    RC(slm::ensure_device());
    zm->mask_set = false;
    if (!mask) return 0;
    RC(zm->mask.need(holo * sizeof(double), zm->stream));
    RC(slm::copy_sync(zm->mask.p, mask, holo * sizeof(double), hipMemcpyHostToDevice, zm->stream));
    zm->mask_set = true;
    return 0;
}

int slm_zoom_set_window(slm_zoom* zm, int per_hologram, const double* y0, const double* x0, const double* z,
                        double dy, double dx, int ny, int nx) {
    if (!zm || !y0 || !x0 || !z) return fail(SLM_ERR_ARG, "null argument");
    RC(check_samples(ny, nx));
    if (ny > zm->max_ny || nx > zm->max_nx)
        return fail(SLM_ERR_ARG, "a window of %d x %d samples exceeds the handle's %d x %d", ny, nx, zm->max_ny,
                    zm->max_nx);
    RC(check_positions(per_hologram ? zm->B : 1, y0, x0, z, dy, dx));
    return zoom_put_window(zm, per_hologram, y0, x0, z, dy, dx, ny, nx);
}

int slm_zoom_set_timed(slm_zoom* zm, int timed) {
    if (!zm) return fail(SLM_ERR_ARG, "null zoom handle");
    zm->timed = timed != 0;
    return 0;
}

int slm_zoom_run(slm_zoom* zm, const void* hologram, int kind, int count, double ct2pi, int want_field) {
    RC(check_run(zm, kind, count, ct2pi));
    if (!hologram) return fail(SLM_ERR_ARG, "null argument");
    RC(slm::ensure_device());
    const size_t bytes = (size_t)count * zm->H * zm->W * (kind == SLM_ZOOM_LEVELS_U8 ? 1 : sizeof(float));
    zm->ran = false;
    RC(zm->holo.need(bytes, zm->stream));
    HIP_TRY(hipMemcpyAsync(zm->holo.p, hologram, bytes, hipMemcpyHostToDevice, zm->stream));
    return zoom_enqueue(zm, zm->holo.p, kind, count, ct2pi, want_field, nullptr);
}

int slm_zoom_run_spots(slm_zoom* zm, slm_spots* sp, int first, int count, double ct2pi, int want_field) {
    if (!zm || !sp) return fail(SLM_ERR_ARG, "null argument");
    return zoom_run_frames(zm, slm::spots_seq_frames(sp), "slm_zoom_run_spots", first, count, ct2pi, want_field);
}

int slm_zoom_run_plan(slm_zoom* zm, slm_plan* plan, int first, int count, double ct2pi, int want_field) {
    if (!zm || !plan) return fail(SLM_ERR_ARG, "null argument");
    return zoom_run_frames(zm, slm::plan_seq_frames(plan), "slm_zoom_run_plan", first, count, ct2pi, want_field);
}

int slm_zoom_read(slm_zoom* zm, float* intensity, double* field, double* kernel_us) {
    if (!zm) return fail(SLM_ERR_ARG, "null zoom handle");
    if (!zm->ran) return fail(SLM_ERR_STATE, "slm_zoom_read before a run");
    if (field && !zm->ran_field) return fail(SLM_ERR_STATE, "the run was not asked for the field");
    if (kernel_us && !zm->ran_timed) return fail(SLM_ERR_STATE, "the run was not timed (slm_zoom_set_timed)");
    RC(slm::ensure_device());
    HIP_TRY(hipStreamSynchronize(zm->stream));
    const size_t n = (size_t)zm->ran_count * zm->ran_ny * zm->ran_nx;
    if (intensity) RC(slm::copy_sync(intensity, zm->intensity.p, n * sizeof(float), hipMemcpyDeviceToHost, zm->stream));
    if (field) RC(slm::copy_sync(field, zm->v.p, n * sizeof(double2), hipMemcpyDeviceToHost, zm->stream));
    if (kernel_us) RC(zm->watch.read(kernel_us, SLM_ZOOM_NUM_KERNEL_CLASSES));
    return 0;
}

int slm_zoom_info(slm_zoom* zm, int* info) {
    if (!zm || !info) return fail(SLM_ERR_ARG, "null argument");
    if (!zm->ran) return fail(SLM_ERR_STATE, "slm_zoom_info before a run");
    info[0] = zm->groups;
    info[1] = zm->bands;
    info[2] = zm->split_launches;
    return 0;
}

}  // extern "C"
