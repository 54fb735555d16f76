// param_amd/csrc/embbag_fwd_f8_e5m2.hip -- pm_embbag_fwd_f8 over e5m2 tables: one format's instantiations of embbag_fwd_f8_kernel.inc
// (a translation unit per format, as the 16-bit-output kernels have one per table dtype).
#include <type_traits>

#include "common.h"
#include "fwd_elem.h"

namespace pm {
namespace {
#include "embbag_fwd_f8_kernel.inc"
}  // namespace

hipError_t launch_embbag_fwd_f8_e5m2(const KParams& p, int max_dim, int unroll, const int64_t* pad_idx, bool mean, int out_dtype, hipStream_t stream) {
    return launch_f8_format<fwd::f8e5m2_t>(p, max_dim, unroll, pad_idx, mean, out_dtype, stream);
}

}  // namespace pm
