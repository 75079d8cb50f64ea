// The pieces the histogram kernels share (select.hip, depth_data.hip: wave_count; evaluation.hip, expand_ln_head.hip:
// wave_count_lead): one count per lane into LDS counters, aggregated per wave first.
#pragma once
#include "hs_device.h"

namespace hs {

// lanes with `active` add one to hist[bin].  Keys that agree in the counted digit (all equal, or a few exponents) would send the
// whole wave to one LDS counter, which serialises the adds; so for up to kPeel rounds the first active lane's bin is taken out
// of the wave with ONE add of its population count, and only what is left after that adds lane by lane.  Called by all lanes of
// a wave together (the loop around it has a wave-uniform trip count).
constexpr int kPeel = 4;
__device__ __forceinline__ void wave_count(uint32_t* hist, bool active, uint32_t bin) {
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    unsigned long long left = __ballot(active);
#pragma unroll
    for (int r = 0; r < kPeel; ++r) {
        if (left == 0) return;
        const int leader = __ffsll(left) - 1;
        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
        const unsigned long long same = __ballot(active && bin == b);
        if (lane == leader) atomicAdd(&hist[b], (uint32_t)__popcll(same));
        active = active && bin != b;
        left &= ~same;
    }
    if (active) atomicAdd(&hist[bin], 1u);
}

// The confusion matrices' add (hs_seg_confusion, the decoder tail's seg step): one count into hist[bin] per lane with bin >= 0.
// The lanes that share the FIRST lane's bin -- most of a wave in the uniform regions of a segmentation -- add with one atomic of
// their population count, every other lane on its own: one round, where wave_count peels kPeel.  Contract: called by EVERY lane
// of the wave (the loop around it has a wave-uniform trip count); a lane with nothing to count comes with bin < 0, which counts
// nothing, also when it is the first lane's.  `lane` is the caller's index in its wave.
__device__ __forceinline__ void wave_count_lead(uint32_t* hist, int bin, int lane) {
    const int lead = __builtin_amdgcn_readfirstlane(bin);
    const unsigned long long same = __ballot(bin == lead);
    if (bin == lead) {
        if (lead >= 0 && lane == __ffsll((long long)same) - 1) atomicAdd(&hist[lead], (uint32_t)__popcll(same));
    } else if (bin >= 0) {
        atomicAdd(&hist[bin], 1u);
    }
}

}  // namespace hs
