// The piece the histogram kernels share (select.hip, depth_data.hip): one count per lane into a workgroup's LDS counters,
// aggregated per wave first.
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

}  // namespace hs
