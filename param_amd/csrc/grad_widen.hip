// param_amd/csrc/grad_widen.hip -- a bf16 / fp16 gradient as the fp32 gradient every backward route takes (pm_embbag_grad_widen,
// DESIGN.md section 3.9):
//   grad32(t, b)[:] = (float)grad16(t, b)[:]                    mean == 0: the widening is exact
//   grad32(t, b)[:] = (float)grad16(t, b)[:] * r                mean == 1: r = 1.0f / (float)count(t, b), +0.0 everywhere for count == 0
// The second line is pm_embbag_mean_grad (mean_pool.hip) on the widened gradient, bit for bit, in the launch that widens: r is rounded
// to fp32 first, then ONE fp32 multiplication per element.  count(t, b) is mean_count.h's.  The sorted, bag-major and LDS apply
// kernels are then run unchanged on grad32.
//
// The scaling kernel's shape: a lane group per bag, 4 elements per lane and round -- 8 bytes read, 16 bytes written --, plain loads and
// stores (the backward reads grad32 at once: it should stay in L2).  One launch for any number of tables; only the bags of the slice
// are written; grad16 is only read.
#include "common.h"
#include "mean_count.h"

namespace pm {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool BF16>
__device__ __forceinline__ float widen16(uint32_t h) {      // h: the 16 bits, in the low half
    if (BF16) return __uint_as_float(h << 16);
    return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(h)));
}

// G = 1 << gshift lanes per bag (8 .. 64: a group never straddles a wave); bags of the slice in table-major order
template <bool BF16, bool MEAN>
__global__ void __launch_bounds__(kBlock) grad_widen_kernel(const KParams p, const int64_t* __restrict__ pad_idx,
                                                            const uint16_t* __restrict__ grad16, float* __restrict__ grad32, int gshift) {
    const int G = 1 << gshift;
    const int lig = static_cast<int>(threadIdx.x) & (G - 1);
    const int64_t bag = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) >> gshift;      // kBlock / G bags per workgroup
    if (bag >= static_cast<int64_t>(p.T) * p.bag_count) return;                                   // (whole groups leave together)
    const int t = static_cast<int>(bag / p.bag_count);
    const int64_t b = p.bag_begin + bag % p.bag_count;
    int64_t count = 1;
    if constexpr (MEAN) count = bag_kept_count(p, pad_idx, t, static_cast<int64_t>(t) * p.B + b, G, lig);
    const int D = p.dims[t];
    const int64_t row = p.out_offsets[t] + b * p.out_stride;
    const u32x2* src = reinterpret_cast<const u32x2*>(grad16 + row);
    f32x4* dst = reinterpret_cast<f32x4*>(grad32 + row);
    if (count > 0) {
        const float r = MEAN ? 1.0f / static_cast<float>(count) : 1.0f;
        for (int c4 = lig; c4 < D / 4; c4 += G) {
            const u32x2 h = src[c4];
            f32x4 v = {widen16<BF16>(h[0] & 0xffffu), widen16<BF16>(h[0] >> 16), widen16<BF16>(h[1] & 0xffffu), widen16<BF16>(h[1] >> 16)};
            if constexpr (MEAN) v = f32x4{v[0] * r, v[1] * r, v[2] * r, v[3] * r};
            dst[c4] = v;
        }
    } else {
        for (int c4 = lig; c4 < D / 4; c4 += G) dst[c4] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

}  // namespace

// p: base parameters of the request (any T); grad16 / grad32 addressed like the forward's out (un-blocked layouts), in their own elements
hipError_t launch_grad_widen(const KParams& p, int max_dim, const int64_t* pad_idx, bool mean, int grad_dtype, const void* grad16,
                             float* grad32, hipStream_t stream) {
    const int G = group_lanes(max_dim, 4);
    int gshift = 3;
    while ((1 << gshift) < G) ++gshift;
    const int64_t bags = static_cast<int64_t>(p.T) * p.bag_count;
    const int64_t per_block = kBlock >> gshift;
    const int64_t grid = (bags + per_block - 1) / per_block;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const dim3 g(static_cast<unsigned>(grid)), blk(kBlock);
    const uint16_t* src = static_cast<const uint16_t*>(grad16);
    if (grad_dtype == PM_BF16) {
        if (mean) hipLaunchKernelGGL((grad_widen_kernel<true, true>), g, blk, 0, stream, p, pad_idx, src, grad32, gshift);
        else hipLaunchKernelGGL((grad_widen_kernel<true, false>), g, blk, 0, stream, p, pad_idx, src, grad32, gshift);
    } else {
        if (mean) hipLaunchKernelGGL((grad_widen_kernel<false, true>), g, blk, 0, stream, p, pad_idx, src, grad32, gshift);
        else hipLaunchKernelGGL((grad_widen_kernel<false, false>), g, blk, 0, stream, p, pad_idx, src, grad32, gshift);
    }
    return hipGetLastError();
}

}  // namespace pm
