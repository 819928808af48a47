// What the two kinds of sequence (slm_spots_sequence in spots.hip,
// slm_plan_sequence in slm_capi.hip) share on the host: the check of the
// arguments both take, and where a handle's last sequence left its uint8 frames
// on the device, the one internal door the resident zoom (zoom.hip) reaches
// them through. One accessor per source, defined next to the source's state.
// Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "runtime.hpp"

struct slm_spots;
struct slm_plan;

namespace slm {

// the arguments every sequence takes; max_loops is the handle's
inline int check_sequence_args(int n_frames, int loops_first, int loops, int max_loops, double tol, int rule,
                               double ct2pi) {
    if (n_frames < 1) return fail(SLM_ERR_ARG, "%d frames: a sequence has at least one", n_frames);
    if (loops_first < 1 || loops_first > max_loops || loops < 1 || loops > max_loops)
        return fail(SLM_ERR_ARG, "loops_first %d and loops %d must lie in 1 .. max_loops %d", loops_first, loops,
                    max_loops);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(SLM_ERR_ARG, "tol must be finite and >= 0, got %g", tol);
    if (rule != SLM_QUANT_ASTYPE && rule != SLM_QUANT_PIL) return fail(SLM_ERR_ARG, "unknown rule %d", rule);
    if (!(ct2pi > 0.0) || !std::isfinite(ct2pi))
        return fail(SLM_ERR_ARG, "ct2pi must be finite and positive, got %g", ct2pi);
    return 0;
}

struct SeqFrames {
    const uint8_t* frames = nullptr;  // [n][H][W], flat index f B + b; nullptr: the sequence did not keep them
    hipStream_t stream = nullptr;     // the stream whose chain writes them
    int n = 0, H = 0, W = 0;          // n = F B of the last sequence; 0: there is none
};

SeqFrames spots_seq_frames(const slm_spots* sp);
SeqFrames plan_seq_frames(const slm_plan* p);

}  // namespace slm
