// param_amd/csrc/embbag_fwd_out16_bf16.hip -- the padded forward's kernel with bf16 / fp16 OUTPUT (pm_embbag_fwd_out16, DESIGN.md
// section 3.9) for bf16 tables: 4 group widths x {plain, weighted, mean} x {bf16, fp16} = 24 instantiations of pad_fwd_kernel
// (embbag_fwd_pad_kernel.inc).  One translation unit per table dtype, so that the build stays parallel.
#include <type_traits>

#include "common.h"
#include "fwd_elem.h"

namespace pm {
namespace {
#include "embbag_fwd_pad_kernel.inc"
}  // namespace

hipError_t launch_embbag_fwd_out16_bf16(const KParams& p, int max_dim, const int64_t* pad_idx, bool mean, int out_dtype, hipStream_t stream) {
    return launch_pad_out16<bf16_t>(p, max_dim, pad_idx, mean, out_dtype, stream);
}

}  // namespace pm
