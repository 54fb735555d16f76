// param_amd/csrc/embbag_fwd_f8s_e4m3_table.hip -- pm_embbag_fwd_f8_scaled over e4m3 tables with a table exponent alone: one
// format's and one kind's instantiations of embbag_fwd_f8s_kernel.inc (a translation unit each, as the unscaled FP8 kernels have one per format).
#include <type_traits>

#include "common.h"
#include "fwd_elem.h"
#include "f8s_elem.h"

namespace pm {
namespace {
#include "embbag_fwd_f8s_kernel.inc"
}  // namespace

hipError_t launch_embbag_fwd_f8s_e4m3_table(const KParams& p, int max_dim, int unroll, const F8sArgs& a, bool mean, int out_dtype, hipStream_t stream) {
    return launch_f8s_format<fwd::f8e4m3_t, false>(p, max_dim, unroll, a, mean, out_dtype, stream);
}

}  // namespace pm
