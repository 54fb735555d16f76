// param_amd/csrc/embbag_fwd_pad.hip -- batched EmbeddingBag(sum) forward with PADDING: a lookup whose index equals its table's
// padding index contributes nothing (torch's nn.EmbeddingBag(padding_idx=...) rule; pm_embbag_fwd_padded, include/param_amd.h).
//
// A kernel family of its own next to the product forward (embbag_fwd.hip), built from the same device
// pieces: element types, row loads, the accumulate step and the burst of a tile's rows come from fwd_elem.h, the LDS tile layout
// from common.h.  Same tiling -- one
// 256-thread workgroup owns `bags_per_block` consecutive bags of one table, a group of G lanes owns a bag, a lane keeps a
// 16-byte column slice of the fp32 accumulator -- and the same arithmetic: additions in index order from +0.0, one fmaf per
// kept lookup when weighted.  The result is therefore bit-identical to pm_embbag_fwd on the request with the padded lookups
// removed.  What is new:
//   * STAGED tiles (the tile's index range fits the LDS index tile): the indices are COMPACTED while they are staged.  Every
//     round of 256 entries is read from the request with coalesced loads; a lane keeps its entry iff it is not the padding
//     index; its slot is the running count + the kept entries of the waves before it (LDS) + the kept lanes below it in its
//     wave (ballot + mbcnt).  The exclusive kept-count of EVERY entry goes to a 16-bit LDS array, from which the tile's bag
//     bounds are rewritten to compacted positions.  The pooling loop then walks a dense list: a padded lookup costs no row
//     load, no LDS read and no branch.
//   * UNSTAGED tiles (a bag longer than the index tile): indices come from the request, two at a time; a padded one is
//     predicated off -- its row load is not issued and nothing is added.
// The padding row is never read into a sum: what is stored there (NaN, Inf) cannot reach the output.  A bag of padding only
// gives +0.0, like an empty bag.
// Kept small on purpose: two row loads in flight (the product default), bags taken in tile order, lane groups sized for
// max_dim (a narrow table of a mixed request wastes lanes).  3 dtypes x 4 group widths x weighted / not = 24 instantiations.
//
// MEAN pooling (pm_embbag_fwd_mean) is the same kernel with MEAN = true: the pooled sum -- the very
// additions above -- is divided by (float)count before it leaves the registers, count = the bag's kept lookups: e - s of a
// staged tile (the bounds are compacted positions), counted along the walk of an unstaged one.  ONE correctly rounded fp32
// division per element (the compiler's default: no reciprocal, no fast-math); count == 0 skips it, the bag stays +0.0.  A NULL
// pad array is "no table has a padding row" (pad = -1).  Mean is unweighted: 3 dtypes x 4 group widths = 12 more instantiations;
// every MEAN line sits under `if constexpr`, so the 24 above keep their code.
//
// The kernel and its launcher ladder live in embbag_fwd_pad_kernel.inc, which the 16-bit-output translation units share
// (pm_embbag_fwd_out16); this file holds the 36 fp32-output instantiations described above.
#include <type_traits>

#include "common.h"
#include "fwd_elem.h"

namespace pm {
namespace {

#include "embbag_fwd_pad_kernel.inc"      // the kernel and its launcher ladder (shared with the 16-bit-output translation units)

template <bool MEAN>
hipError_t launch_pad_t(const KParams& p, int weight_dtype, int max_dim, const int64_t* pad_idx, hipStream_t stream) {
    switch (weight_dtype) {
        case PM_F32: return launch_pad_g<float, MEAN, float>(p, max_dim, pad_idx, stream);
        case PM_BF16: return launch_pad_g<bf16_t, MEAN, float>(p, max_dim, pad_idx, stream);
        default: return launch_pad_g<f16_t, MEAN, float>(p, max_dim, pad_idx, stream);
    }
}

}  // namespace

// p: plain bag-count tiling (bags_per_block <= 1024, idx_cap <= 4096); stage_out > 0: bags_per_block * stage_out floats of burst buffer
hipError_t launch_embbag_fwd_padded(const KParams& p, int weight_dtype, int max_dim, const int64_t* pad_idx, hipStream_t stream) {
    return launch_pad_t<false>(p, weight_dtype, max_dim, pad_idx, stream);
}

// the same tiling; pad_idx NULL = no table has a padding row
hipError_t launch_embbag_fwd_mean(const KParams& p, int weight_dtype, int max_dim, const int64_t* pad_idx, hipStream_t stream) {
    return launch_pad_t<true>(p, weight_dtype, max_dim, pad_idx, stream);
}

}  // namespace pm
