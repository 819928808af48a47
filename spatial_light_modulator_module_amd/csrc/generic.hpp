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
//
// Which back end, at which precision and on which tiles is decided once, by
// generic_choose; generic_create builds what that choice says and nothing is
// chosen again afterwards.
#pragma once
#include "plan.hpp"

namespace slm {

// What a plan of one shape, algorithm and requested precision runs on. The
// members are slm_plan_generic_info's (slm_hip.h): info[0] = kind,
// [1] = prec, [2] / [3] = rkey / ckey, [4] = rpw, [5] = cw, [6] = lay,
// [7] = column workgroups per hologram (nwg; 0 on line transforms).
struct AnySizeChoice {
    // the back end, as slm_plan_engine reports it: 2 line transforms (chirp-z),
    // 3 mixed radix, 4 complex128 radix plans, 5 complex64 radix plans
    int kind = 2;
    // the precision the plan runs at: SLM_PRECISION_F32 only on the complex64
    // radix kernels (both sides have one, GS only), else float64
    int prec = SLM_PRECISION_F64;
    // statistics blocks per hologram (PlanState::nwg, the partials' tiling):
    // column tiles of the tiled back ends, element chunks of the line transforms
    int nwg = 0;
    int rkey = -1, ckey = -1;  // radix plans: plan keys (plans.hpp) of the row / column transforms
    int rpw = 1;               // rows per row tile (1 on line transforms: no tiles)
    int cw = 1;                // columns per column tile
    int lay = 0;               // state layout between the passes (radix_c128.hpp LAY_RM 0 / LAY_B2 1); 0 = row-major
    bool big = false;          // mixed radix: a radix outside mr::small_radix in either plan (7, 11, 13)
    bool chirp_all = false;    // line transforms forced ($SLM_GENERIC_ENGINE=bluestein): chirp-z on every side
};

// The choice for a shape, algorithm and requested precision. Reads
// $SLM_GENERIC_ENGINE, $SLM_RZ_* and $SLM_MR_* and queries the tile kernels'
// occupancy (mixed radix), all of it here and nowhere else.
AnySizeChoice generic_choose(int B, int H, int W, int algo, int prec);
// The any-size engine that `c` describes, for the plan s (s.prec = c.prec and
// s.nwg = c.nwg are the caller's to set; tables upload on s.stream).
int generic_create(const PlanState& s, const AnySizeChoice& c, Engine** out);
// the choice an any-size engine was created with
const AnySizeChoice& generic_choice(const Engine& e);

}  // namespace slm
