// param_amd/csrc/mean_pool.hip -- the gradient side of MEAN pooling (pm_embbag_mean_grad):
//   scaled(t, b)[:] = grad(t, b)[:] * r,   r = 1.0f / (float)count(t, b),   +0.0 everywhere for count == 0
// count(t, b) = the lookups of bag (t, b) that are not table t's padding index.  r is rounded to fp32 FIRST (one correctly rounded
// division per bag), then ONE fp32 multiplication per element: torch's mean backward (not grad / count).  Every backward route --
// sorted, hybrid bag-major, LDS left-over, every optimizer -- is then run unchanged on `scaled`: "mean backward" is "the sum
// backward fed with the scaled gradient".
//
// A lane group per bag, 16 bytes per lane (a wider row takes several rounds), plain loads and stores (the backward reads the buffer
// at once: it should stay in L2).  The count is mean_count.h's (shared with grad_widen.hip).
#include "common.h"
#include "mean_count.h"

namespace pm {
namespace {

// G = 1 << gshift lanes per bag (8 .. 64: a group never straddles a wave); bags of the slice in table-major order
__global__ void __launch_bounds__(kBlock) mean_grad_kernel(const KParams p, const int64_t* __restrict__ pad_idx,
                                                           const float* grad, float* scaled, int gshift) {
    const int G = 1 << gshift;
    const int lig = static_cast<int>(threadIdx.x) & (G - 1);
    const int64_t bag = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) >> gshift;      // kBlock / G bags per workgroup
    if (bag >= static_cast<int64_t>(p.T) * p.bag_count) return;                                   // (whole groups leave together)
    const int t = static_cast<int>(bag / p.bag_count);
    const int64_t b = p.bag_begin + bag % p.bag_count;
    const int64_t g = static_cast<int64_t>(t) * p.B + b;
    const int64_t count = bag_kept_count(p, pad_idx, t, g, G, lig);      // mean_count.h
    const int D = p.dims[t];
    const int64_t row = p.out_offsets[t] + b * p.out_stride;
    const f32x4* src = reinterpret_cast<const f32x4*>(grad + row);
    f32x4* dst = reinterpret_cast<f32x4*>(scaled + row);
    if (count > 0) {
        const float r = 1.0f / static_cast<float>(count);
        for (int c4 = lig; c4 < D / 4; c4 += G) {
            const f32x4 v = src[c4];
            dst[c4] = f32x4{v[0] * r, v[1] * r, v[2] * r, v[3] * r};
        }
    } else {
        for (int c4 = lig; c4 < D / 4; c4 += G) dst[c4] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

}  // namespace

// p: base parameters of the request (any T); grad / scaled addressed like the forward's out (un-blocked layouts)
hipError_t launch_mean_grad(const KParams& p, int max_dim, const int64_t* pad_idx, const float* grad, float* scaled, hipStream_t stream) {
    const int G = group_lanes(max_dim, 4);
    int gshift = 3;
    while ((1 << gshift) < G) ++gshift;
    const int64_t bags = static_cast<int64_t>(p.T) * p.bag_count;
    const int64_t per_block = kBlock >> gshift;
    const int64_t grid = (bags + per_block - 1) / per_block;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(mean_grad_kernel, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0, stream, p, pad_idx, grad, scaled, gshift);
    return hipGetLastError();
}

}  // namespace pm
