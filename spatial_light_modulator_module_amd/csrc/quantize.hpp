// The one definition of the SLM quantisation rules (SLM_QUANT_* in
// include/slm_hip.h): phase (+ correction mask) to the panel's 8-bit levels.
// Shared by the frame kernels (frames.hip) and the quantising epilogue of the
// trap-list superposition (spots.hip). The expressions hold no product that
// feeds a sum, so they give the same bits under either contraction setting.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/slm_hip.h"

namespace slm {

constexpr double kQuantTwoPi = 6.283185307179586;  // 2 * np.pi as float64

// Python / numpy float remainder: sign of the divisor (`%` on float64).
__device__ __forceinline__ double py_mod(double a, double b) {
    double r = fmod(a, b);
    if (r != 0.0 && ((r < 0.0) != (b < 0.0))) r += b;
    return r;
}

// numpy float64 -> uint8 astype: C truncation of the value (through int64,
// so out-of-range levels wrap as they do on x86).
__device__ __forceinline__ uint8_t astype_u8(double v) { return (uint8_t)(long long)v; }

// PIL Image.fromarray(float64) is mode 'F' (float32); convert('L') clips to
// [0, 255] and truncates (probed on Pillow 12.2, see tests/test_frames.py).
__device__ __forceinline__ uint8_t pil_f_to_l(double v) {
    const float f = (float)v;
    if (!(f > 0.0f)) return 0;
    if (f >= 255.0f) return 255;
    return (uint8_t)(int)f;
}

__device__ __forceinline__ uint8_t quantize(double h, double m, double ct2pi, int rule) {
    if (rule == SLM_QUANT_ASTYPE) return astype_u8(py_mod(h + m, kQuantTwoPi) * ct2pi / kQuantTwoPi);
    return pil_f_to_l(py_mod(h + m, kQuantTwoPi) / kQuantTwoPi * ct2pi);
}

}  // namespace slm
