// param_amd/csrc/mean_count.h -- count(t, b) of MEAN pooling as a lane group of G lanes establishes it: the lookups of a bag that are
// not its table's padding index (mean_pool.hip: the scaling kernel; grad_widen.hip: the widening kernel with the scaling fused).
#pragma once

#include "common.h"

namespace pm {

// g: the bag's global number (t * B + b); every lane of the group calls it (the trip count is the group's: its lanes stay together).
// Without a padding row the count is two offset reads; with one, the group's lanes stride over the bag's indices and every round's
// kept lookups are a ballot, masked to the group's lanes, and a population count.
__device__ __forceinline__ int64_t bag_kept_count(const KParams& p, const int64_t* __restrict__ pad_idx, int t, int64_t g, int G, int lig) {
    int64_t s = bag_start_or_end(p, g), e = bag_start_or_end(p, g + 1);
    s = s < 0 ? 0 : s;                         // (an unrepaired request: nothing outside the index array is read)
    e = e > p.N ? p.N : e;
    int64_t count = e > s ? e - s : 0;
    const int64_t pad = pad_idx ? pad_idx[t] : -1;
    if (pad >= 0 && count > 0) {
        const int lane = static_cast<int>(threadIdx.x) & (kWave - 1);
        const int shift = lane & ~(G - 1);     // the group's first lane in its wave
        const uint64_t mask = G == kWave ? ~0ull : ((1ull << G) - 1ull);
        count = 0;
        for (int64_t j0 = s; j0 < e; j0 += G) {
            const int64_t j = j0 + lig;
            const bool keep = j < e && load_index(p.indices, j, p.idx64) != pad;
            count += __popcll((__ballot(keep) >> shift) & mask);
        }
    }
    return count;
}

}  // namespace pm
