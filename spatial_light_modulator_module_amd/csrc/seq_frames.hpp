// Where a handle's last sequence left its uint8 frames on the device: the one
// internal door the resident zoom (zoom.hip) reaches them through. One accessor
// per source, defined next to the source's state (spots.hip, slm_capi.hip). Not
// part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct slm_spots;
struct slm_plan;

namespace slm {

struct SeqFrames {
    const uint8_t* frames = nullptr;  // [n][H][W], flat index f B + b; nullptr: the sequence did not keep them
    hipStream_t stream = nullptr;     // the stream whose chain writes them
    int n = 0, H = 0, W = 0;          // n = F B of the last sequence; 0: there is none
};

SeqFrames spots_seq_frames(const slm_spots* sp);
SeqFrames plan_seq_frames(const slm_plan* p);

}  // namespace slm
