// param_amd/csrc/embbag_fwd_anyfmt_bf16.hip -- pm_embbag_fwd_anyfmt's kernels with bf16 OUTPUT: one translation unit per output type, so
// that the three compile in parallel.  The kernel and what it computes: embbag_fwd_anyfmt_kernel.inc.
#include "common.h"
#include "fwd_elem.h"
#include "f8s_elem.h"
#include "qrows_elem.h"

namespace pm {
namespace {
#include "embbag_fwd_anyfmt_kernel.inc"
}  // namespace

// p = plan_anyfmt's geometry, p.io = the bf16 output addressed in its elements; table_formats: device int32 [T]; table_exp: device int32 [T] or NULL
hipError_t launch_embbag_fwd_anyfmt_bf16(const KParams& p, const int32_t* table_formats, const int32_t* table_exp, int max_dim, hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, kAnyfmtLaneColumns),
                                [&](auto g) { return launch_any_w<decltype(g)::value, OutBF16>(p, table_formats, table_exp, stream); });
}

}  // namespace pm
