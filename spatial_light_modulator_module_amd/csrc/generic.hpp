// Any-size engine of the GS / GD loops: image sides that no float32 radix plan
// (plans.hpp) covers. The reference takes any (h, w) (src/algorithms.py:20-27;
// scipy.fft handles every length), so such plans run in complex float64 with
// row-major state: on the complex128 radix-plan kernels (radix_c128.hpp) where
// both sides have a radix plan ($SLM_ENGINE=float64; their complex64 variant
// runs GS on 13-smooth SLM panels such as 1080 x 1920), on hand-written
// mixed-radix transforms (mixed_radix.hpp) where both sides factor into 2, 3,
// 5, 7, 11, 13, otherwise as 1-D line transforms (direct, or Bluestein's
// chirp-z over a mixed-radix length) plus element-wise kernels. slm_capi.hip
// owns the plan's buffers (plan.hpp PlanState); this engine owns its work
// buffers and line plans.
#pragma once
#include "plan.hpp"

namespace slm {

// statistics blocks per hologram (the partials' nwg): column tiles of the
// mixed-radix / radix-plan back ends, element chunks of the line-transform one
int generic_nwg(int B, int H, int W, long long holo, int algo = 0, int prec = 1);
// the precision a plan of this shape, algorithm and requested precision runs
// at: PREC_F32 takes the complex64 radix kernels where both sides have one
// (GS only), else the engine runs in float64
int generic_precision(int B, int H, int W, int algo, int prec);
// The any-size engine of s (shape, algorithm, s.prec as generic_precision
// reports it, s.nwg as generic_nwg does; tables upload on s.stream). Its codes
// (slm_plan_engine): 2 line transforms (chirp-z), 3 mixed radix, 4 complex128
// radix plans, 5 complex64 radix plans. Its generic_info is the geometry it
// was created with (slm_plan_generic_info, slm_hip.h): info[0] = code,
// [1] = precision, [2] / [3] = row / column plan key (-1 off the radix-plan
// back ends), [4] = rows per row tile, [5] = columns per column tile,
// [6] = state layout (radix_c128.hpp LAY_RM 0 / LAY_B2 1; 0 = row-major off
// the radix-plan back ends), [7] = column workgroups per hologram. The
// line-transform back end has no tiles: [4] = [5] = 1, [7] = 0.
int generic_create(const PlanState& s, Engine** out);

}  // namespace slm
