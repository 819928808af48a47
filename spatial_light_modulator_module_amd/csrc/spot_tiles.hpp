// Device pieces the two matrix-core translation units share (spots.hip: trap
// lists; zoom.hip: the zoomed far field): the MFMA tile constants, the
// accumulator layout, the f32 MFMA itself and the float64 table entry.
#pragma once
#include <hip/hip_runtime.h>

namespace slm {
namespace tiles {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr double kTwoPi = 6.283185307179586;
constexpr int kTile = 32;         // MFMA tile side
constexpr int kLdsStride = 66;    // floats per staged field row (64 + 2: conflict-free 8 B reads)
constexpr int kMinSide = 2, kMaxSide = 4096;
constexpr int kWaves = 4;         // waves per workgroup of the product kernels

// row of accumulator register r of a 32x32 MFMA result in lane half h (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// one table entry: float64 with the argument reduced first, rounded to complex64
__device__ __forceinline__ float2 table_entry(int n, int N, double pos, double z) {
    double t = (double)n * pos / (double)N;
    t -= floor(t);  // the argument of the sine is reduced to [0, 2 pi) first
    const double d = (double)n - 0.5 * (double)N;
    double s, c;
    sincos(kTwoPi * t + z * d * d, &s, &c);
    return make_float2((float)c, (float)s);
}

}  // namespace tiles
}  // namespace slm
