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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "runtime.hpp"
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
// P[n][s] = exp(i f_s(n)) for sample s < count at pos0 + s pitch, 0 for the padding; [N][padded]
__global__ void __launch_bounds__(256) zoom_table_kernel(float2* out, int N, int count, int padded, double pos0,
                                                         double pitch, double z) {
    const long long n_el = (long long)N * padded;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n_el; i += (long long)gridDim.x * 256) {
        const int n = (int)(i / padded), s = (int)(i - (long long)n * padded);
        float2 v = make_float2(0.0f, 0.0f);
        // pos0 + s pitch with the product rounded before the sum (no contraction into an fma)
        if (s < count) v = table_entry(n, N, __dadd_rn(pos0, __dmul_rn((double)s, pitch)), z);
        out[i] = v;
    }
}

// ---- the field a u --------------------------------------------------------
// kind SLM_ZOOM_PHASE_F32: u = float64 sincos of the float32 phase, as spot_phase_kernel forms it;
// SLM_ZOOM_LEVELS_U8: u = levels[level], the 256 entries evaluated in float64 on the host
__global__ void __launch_bounds__(256) zoom_field_kernel(const void* holo, int kind, const float* ain,
                                                         const float2* levels, float2* field, long long n) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float2 u;
        if (kind == SLM_ZOOM_LEVELS_U8) {
            u = levels[static_cast<const uint8_t*>(holo)[i]];
        } else {
            double s, c;
            sincos((double)static_cast<const float*>(holo)[i], &s, &c);
            u = make_float2((float)c, (float)s);
        }
        const float a = ain ? ain[i] : 1.0f;
        field[i] = make_float2(u.x * a, u.y * a);
    }
}

// ---- product 1: R = (a u) conj(Px) ----------------------------------------
struct RowsParams {
    const float2* field;  // [H][W]
    const float2* px;     // [W][nxp]
    float2* out;          // R [H][nxp], or with a split the chunk results [chunks][H][nxp]
    int H, W, nxp;
    int cols_per_unit;    // columns per blockIdx.z: all of them, or with a split one chunk
};

// One workgroup per 32 rows x 128 samples: its four waves share the staged
// field tiles (two LDS buffers, filled in turn: one barrier per tile) and take
// one 32-sample tile each. A wave past the last sample tile only helps to
// stage. A window of few sample tiles splits the columns over workgroups, one
// chunk each, and zoom_rows_fold_kernel adds the chunk results as this kernel
// adds them in its registers otherwise: R is the same bit for bit either way.
// grid = (groups of 4 sample tiles, row tiles, 1 or chunks).
__global__ void __launch_bounds__(kThreads) zoom_rows_kernel(RowsParams p) {
    __shared__ float tiles[2][kTile * kLdsStride];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int row0 = blockIdx.y * kTile, s0 = (blockIdx.x * kWaves + wave) * kTile;
    const bool active = s0 < p.nxp;
    const int c_begin = blockIdx.z * p.cols_per_unit, c_end = min(p.W, c_begin + p.cols_per_unit);
    const float2* px = p.px + (active ? s0 : 0) + li;

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
            if (gr < p.H && gc < p.W) ft[e] = p.field[(size_t)gr * p.W + gc];
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

// R = the chunk results of a split first product, added in float64 in their order and rounded once
__global__ void __launch_bounds__(256) zoom_rows_fold_kernel(const float2* partial, float2* r, int chunks,
                                                             long long n) {
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
    const float2* py;  // [H][nyp]
    const float2* r;   // [H][nxp]
    float2* partial;   // [chunks][band rows][nxp]
    int H, nyp, nxp;
    int j0, band_rows;  // this band: sample rows j0 .. j0 + band_rows (a multiple of 32)
};

// One wave per 32 x 32 output tile and chunk of 256 pixel rows, four adjacent
// column tiles per workgroup; no barriers. grid = (column tiles / 4, the band's row tiles, chunks).
__global__ void __launch_bounds__(kThreads) zoom_cols_kernel(ColsParams p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int i0 = (blockIdx.x * kWaves + wave) * kTile, jb = blockIdx.y * kTile, chunk = blockIdx.z;
    if (i0 >= p.nxp) return;
    const int k0 = chunk * kChunk;
    const float2* py = p.py + p.j0 + jb + li;
    const float2* rr = p.r + i0 + li;
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
    float2* out = p.partial + ((size_t)chunk * p.band_rows + jb) * p.nxp + i0 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(size_t)acc_row(r, lh) * p.nxp] = make_float2(vre[r], vim[r]);
}

// ---- fold: V = the chunks added in float64 in their order, I = |V|^2 ------
struct FoldParams {
    const float2* partial;  // [chunks][band rows][nxp]
    float* intensity;       // [rows][nx]
    double2* v;             // [rows][nx] or nullptr
    int chunks, band_rows, rows, nx, nxp;  // rows = the band's samples that exist (<= band_rows)
};

__global__ void __launch_bounds__(256) zoom_fold_kernel(FoldParams p) {
    const long long n = (long long)p.rows * p.nx;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int j = (int)(e / p.nx), i = (int)(e - (long long)j * p.nx);
        double vr = 0.0, vi = 0.0;
        for (int c = 0; c < p.chunks; ++c) {
            const float2 t = p.partial[((size_t)c * p.band_rows + j) * p.nxp + i];
            vr += (double)t.x;
            vi += (double)t.y;
        }
        p.intensity[e] = (float)(vr * vr + vi * vi);
        if (p.v) p.v[e] = make_double2(vr, vi);
    }
}

int grid_for(long long n) { return (int)std::min<long long>(8192, (n + 255) / 256); }
int padded(int n) { return (n + kTile - 1) / kTile * kTile; }

using slm::DevBuf;
using slm::fail;

// the call's stream, buffers and (when timed) events, all released when it returns
struct Zoom {
    hipStream_t stream = nullptr;
    DevBuf<float> ain;
    DevBuf<float2> levels, px, py, field, r, partial;
    DevBuf<uint8_t> holo;
    DevBuf<float> intensity;
    DevBuf<double2> v;
    std::vector<hipEvent_t> ev;  // begin / end pairs, pair k of class cls[k]
    std::vector<int> cls;
    bool timed = false;
    ~Zoom() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
    int mark() {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
        HIP_TRY(hipEventRecord(e, stream));
        return 0;
    }
    int begin(int c) {
        if (!timed) return 0;
        cls.push_back(c);
        return mark();
    }
    int end() { return timed ? mark() : 0; }
};

int check_args(const void* hologram, int kind, int batch, int height, int width, const float* ain, double ct2pi,
               double y0, double x0, double dy, double dx, int ny, int nx, double z, const float* intensity) {
    if (!hologram || !intensity) return fail(SLM_ERR_ARG, "null argument");
    if (kind != SLM_ZOOM_PHASE_F32 && kind != SLM_ZOOM_LEVELS_U8) return fail(SLM_ERR_ARG, "unknown kind %d", kind);
    if (batch < 1) return fail(SLM_ERR_ARG, "batch must be positive, got %d", batch);
    if (height < kMinSide || width < kMinSide || height > kMaxSide || width > kMaxSide)
        return fail(SLM_ERR_ARG, "the zoom runs on sides %d .. %d, got %d x %d", kMinSide, kMaxSide, height, width);
    if (ny < 1 || nx < 1 || ny > kMaxSamples || nx > kMaxSamples)
        return fail(SLM_ERR_ARG, "a window has 1 .. %d samples per side, got %d x %d", kMaxSamples, ny, nx);
    if (!std::isfinite(y0) || !std::isfinite(x0) || !std::isfinite(dy) || !std::isfinite(dx) || !std::isfinite(z))
        return fail(SLM_ERR_ARG, "the window's origin, pitch and defocus must be finite");
    if (!(dy > 0.0) || !(dx > 0.0)) return fail(SLM_ERR_ARG, "the pitch must be positive, got %g x %g", dy, dx);
    if (kind == SLM_ZOOM_LEVELS_U8 && (!(ct2pi > 0.0) || !std::isfinite(ct2pi)))
        return fail(SLM_ERR_ARG, "ct2pi must be finite and positive, got %g", ct2pi);
    if (ain) {
        const size_t holo = (size_t)height * width;
        double sum = 0.0;
        for (size_t i = 0; i < holo; ++i) {
            if (!std::isfinite(ain[i])) return fail(SLM_ERR_ARG, "a_in has a non-finite entry");
            sum += (double)ain[i] * (double)ain[i];
        }
        if (!(sum > 0.0)) return fail(SLM_ERR_ARG, "a_in is zero everywhere");
    }
    return 0;
}

int zoom_run(Zoom& zm, const void* hologram, int kind, int batch, int H, int W, const float* ain, double ct2pi,
             double y0, double x0, double dy, double dx, int ny, int nx, double z, float* intensity, double* field) {
    HIP_TRY(hipStreamCreateWithFlags(&zm.stream, hipStreamNonBlocking));
    const hipStream_t st = zm.stream;
    const int nxp = padded(nx), nyp = padded(ny), chunks = (H + kChunk - 1) / kChunk;
    const size_t holo = (size_t)H * W, el = kind == SLM_ZOOM_LEVELS_U8 ? 1 : sizeof(float);
    // the band: whole tile rows whose chunk results fit the partial buffer
    const size_t row_bytes = (size_t)chunks * nxp * sizeof(float2);
    const int band_rows = std::min<size_t>(nyp, std::max<size_t>(kTile, kPartialBytes / row_bytes / kTile * kTile));

    if (ain) RC(zm.ain.need(holo * sizeof(float), st));
    if (kind == SLM_ZOOM_LEVELS_U8) RC(zm.levels.need(256 * sizeof(float2), st));
    RC(zm.px.need((size_t)W * nxp * sizeof(float2), st));
    RC(zm.py.need((size_t)H * nyp * sizeof(float2), st));
    RC(zm.holo.need(holo * el, st));
    RC(zm.field.need(holo * sizeof(float2), st));
    RC(zm.r.need((size_t)H * nxp * sizeof(float2), st));
    // the first product splits its columns over workgroups while its tiles are few (the same R either way)
    const int row_tiles = (H + kTile - 1) / kTile, wchunks = (W + kChunk - 1) / kChunk;
    const size_t r_bytes = (size_t)H * nxp * sizeof(float2);
    const bool split_rows =
        wchunks > 1 && row_tiles * (nxp / kTile) < kSplitBelowWaves && wchunks * r_bytes <= kRowsPartialBytes;
    RC(zm.partial.need(std::max(row_bytes * band_rows, split_rows ? wchunks * r_bytes : 0), st));
    RC(zm.intensity.need((size_t)band_rows * nx * sizeof(float), st));
    if (field) RC(zm.v.need((size_t)band_rows * nx * sizeof(double2), st));

    if (ain) RC(slm::copy_sync(zm.ain.p, ain, holo * sizeof(float), hipMemcpyHostToDevice, st));
    if (kind == SLM_ZOOM_LEVELS_U8) {
        float2 levels[256];
        for (int v = 0; v < 256; ++v) {
            const double t = kTwoPi * (double)v / ct2pi;
            levels[v] = make_float2((float)std::cos(t), (float)std::sin(t));
        }
        RC(slm::copy_sync(zm.levels.p, levels, sizeof(levels), hipMemcpyHostToDevice, st));
    }
    RC(zm.begin(SLM_ZOOM_KERNEL_TABLES));
    hipLaunchKernelGGL(zoom_table_kernel, dim3(grid_for((long long)W * nxp)), dim3(256), 0, st, zm.px.p, W, nx, nxp,
                       x0, dx, z);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(zoom_table_kernel, dim3(grid_for((long long)H * nyp)), dim3(256), 0, st, zm.py.p, H, ny, nyp,
                       y0, dy, z);
    HIP_TRY(hipGetLastError());
    RC(zm.end());

    for (int b = 0; b < batch; ++b) {
        RC(slm::copy_sync(zm.holo.p, static_cast<const uint8_t*>(hologram) + (size_t)b * holo * el, holo * el,
                          hipMemcpyHostToDevice, st));
        RC(zm.begin(SLM_ZOOM_KERNEL_FIELD));
        hipLaunchKernelGGL(zoom_field_kernel, dim3(grid_for((long long)holo)), dim3(256), 0, st, zm.holo.p, kind,
                           ain ? zm.ain.p : nullptr, zm.levels.p, zm.field.p, (long long)holo);
        HIP_TRY(hipGetLastError());
        RC(zm.end());
        RC(zm.begin(SLM_ZOOM_KERNEL_ROWS));
        const RowsParams rp{zm.field.p, zm.px.p, split_rows ? zm.partial.p : zm.r.p, H, W, nxp,
                            split_rows ? kChunk : wchunks * kChunk};
        const int sample_groups = (nxp / kTile + kWaves - 1) / kWaves;
        hipLaunchKernelGGL(zoom_rows_kernel, dim3(sample_groups, row_tiles, split_rows ? wchunks : 1), dim3(kThreads),
                           0, st, rp);
        HIP_TRY(hipGetLastError());
        if (split_rows) {
            hipLaunchKernelGGL(zoom_rows_fold_kernel, dim3(grid_for((long long)H * nxp)), dim3(256), 0, st,
                               zm.partial.p, zm.r.p, wchunks, (long long)H * nxp);
            HIP_TRY(hipGetLastError());
        }
        RC(zm.end());
        for (int j0 = 0; j0 < ny; j0 += band_rows) {
            const int tile_rows = std::min(band_rows, nyp - j0), rows = std::min(band_rows, ny - j0);
            RC(zm.begin(SLM_ZOOM_KERNEL_COLS));
            const ColsParams cp{zm.py.p, zm.r.p, zm.partial.p, H, nyp, nxp, j0, band_rows};
            hipLaunchKernelGGL(zoom_cols_kernel, dim3(sample_groups, tile_rows / kTile, chunks), dim3(kThreads), 0, st,
                               cp);
            HIP_TRY(hipGetLastError());
            const FoldParams fp{zm.partial.p, zm.intensity.p, field ? zm.v.p : nullptr, chunks, band_rows, rows, nx,
                                nxp};
            hipLaunchKernelGGL(zoom_fold_kernel, dim3(grid_for((long long)rows * nx)), dim3(256), 0, st, fp);
            HIP_TRY(hipGetLastError());
            RC(zm.end());
            const size_t at = ((size_t)b * ny + j0) * nx, n = (size_t)rows * nx;
            RC(slm::copy_sync(intensity + at, zm.intensity.p, n * sizeof(float), hipMemcpyDeviceToHost, st));
            if (field) RC(slm::copy_sync(field + 2 * at, zm.v.p, n * sizeof(double2), hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

int slm_farfield_zoom_timed(const void* hologram, int kind, int batch, int height, int width, const float* ain,
                            double ct2pi, double y0, double x0, double dy, double dx, int ny, int nx, double z,
                            float* intensity, double* field, double* kernel_us) {
    RC(check_args(hologram, kind, batch, height, width, ain, ct2pi, y0, x0, dy, dx, ny, nx, z, intensity));
    RC(slm::ensure_device());
    Zoom zm;
    zm.timed = kernel_us != nullptr;
    RC(zoom_run(zm, hologram, kind, batch, height, width, ain, ct2pi, y0, x0, dy, dx, ny, nx, z, intensity, field));
    if (kernel_us) {
        for (int c = 0; c < SLM_ZOOM_NUM_KERNEL_CLASSES; ++c) kernel_us[c] = 0.0;
        for (size_t k = 0; k < zm.cls.size(); ++k) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, zm.ev[2 * k], zm.ev[2 * k + 1]));
            kernel_us[zm.cls[k]] += 1e3 * ms;
        }
    }
    return 0;
}

int slm_farfield_zoom(const void* hologram, int kind, int batch, int height, int width, const float* ain, double ct2pi,
                      double y0, double x0, double dy, double dx, int ny, int nx, double z, float* intensity,
                      double* field) {
    return slm_farfield_zoom_timed(hologram, kind, batch, height, width, ain, ct2pi, y0, x0, dy, dx, ny, nx, z,
                                   intensity, field, nullptr);
}

}  // extern "C"
