// param_amd/csrc/embbag_max_grad.hip -- the gradient of a MAX-pooled forward as a sequence gradient (pm_embbag_max_grad,
// include/param_amd.h: MAX POOLING):
//   g_seq[j, c] = grad(t, b)[c]   if j is the FIRST position of bag (t, b) with indices[j] == max_indices(t, b)[c]
//               = +0.0            for every other position of the bag
// for the bags of the slice; positions outside it are not written.  The sequence backward (pm_embseq_*) of the same request then
// applies g_seq unchanged: a row a bag looks up twice receives the bag's gradient once, and a table row accumulates its bags'
// contributions in ascending position = ascending bag order.  No arithmetic here: a 16-bit grad is widened exactly in the same launch.
//
// The kernel's shape: a lane group per bag (grad_widen.hip's), a lane holds grad and max_indices of 4 columns per round and walks the
// bag's positions; per position and column hit = !done && index == arg, the store is hit ? g : +0.0, done |= hit.  One 16-byte
// non-temporal store per lane and position: g_seq is written once and read by the apply after the key sort.  max_indices of a bag
// without kept lookups is -1 and matches no index; a padded lookup's index is never a bag's arg-max, so its row is +0.0.
// No atomics.  One launch for any number of tables.
#include "common.h"

namespace pm {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// GD: the gradient's element, 0 fp32 / 1 bf16 / 2 fp16
template <int GD>
__device__ __forceinline__ f32x4 load_grad4(const void* grad, int64_t elem) {
    if constexpr (GD == 0) {
        return *reinterpret_cast<const f32x4*>(static_cast<const float*>(grad) + elem);
    } else {
        const u32x2 h = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(grad) + elem);
        const uint32_t q[4] = {h[0] & 0xffffu, h[0] >> 16, h[1] & 0xffffu, h[1] >> 16};
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = GD == 1 ? __uint_as_float(q[k] << 16) : static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(q[k])));
        return v;
    }
}

// G = 1 << gshift lanes per bag (8 .. 64: a group never straddles a wave); bags of the slice in table-major order
template <int GD>
__global__ void __launch_bounds__(kBlock) max_grad_kernel(const KParams p, const void* __restrict__ grad, const int32_t* __restrict__ arg,
                                                          float* __restrict__ g_seq, int64_t g_stride, int gshift) {
    const int G = 1 << gshift;
    const int lig = static_cast<int>(threadIdx.x) & (G - 1);
    const int64_t bag = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) >> gshift;      // kBlock / G bags per workgroup
    if (bag >= static_cast<int64_t>(p.T) * p.bag_count) return;                                   // (whole groups leave together)
    const int t = static_cast<int>(bag / p.bag_count);
    const int64_t b = p.bag_begin + bag % p.bag_count;
    const int64_t g = static_cast<int64_t>(t) * p.B + b;
    int64_t s = bag_start_or_end(p, g), e = bag_start_or_end(p, g + 1);
    if (s < 0) s = 0;                                   // (a request that was not checked: nothing outside g_seq's N rows is written)
    if (e > p.N) e = p.N;
    const int D = p.dims[t];
    const int64_t row = p.out_offsets[t] + b * p.out_stride;
    for (int c4 = lig; c4 < D / 4; c4 += G) {
        const f32x4 gv = load_grad4<GD>(grad, row + c4 * 4);
        const i32x4 av = *reinterpret_cast<const i32x4*>(arg + row + c4 * 4);
        bool done[4] = {false, false, false, false};
        for (int64_t j = s; j < e; ++j) {
            const int64_t idx = load_index(p.indices, j, p.idx64);
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool hit = !done[k] && idx == static_cast<int64_t>(av[k]);
                v[k] = hit ? gv[k] : 0.0f;
                done[k] = done[k] || hit;
            }
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(g_seq + j * g_stride + c4 * 4));
        }
    }
}

}  // namespace

// p: base parameters of the request (any T, one dim); grad / max_indices addressed like the forward's out (un-blocked layouts), each in
// its own elements; g_seq: fp32 [N, g_stride]
hipError_t launch_max_grad(const KParams& p, int max_dim, const void* grad, int grad_dtype, const int32_t* max_indices, float* g_seq,
                           int64_t g_stride, hipStream_t stream) {
    const int G = group_lanes(max_dim, 4);
    int gshift = 3;
    while ((1 << gshift) < G) ++gshift;
    const int64_t bags = static_cast<int64_t>(p.T) * p.bag_count;
    const int64_t per_block = kBlock >> gshift;
    const int64_t grid = (bags + per_block - 1) / per_block;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const dim3 gr(static_cast<unsigned>(grid)), blk(kBlock);
    if (grad_dtype == PM_F32) hipLaunchKernelGGL((max_grad_kernel<0>), gr, blk, 0, stream, p, grad, max_indices, g_seq, g_stride, gshift);
    else if (grad_dtype == PM_BF16) hipLaunchKernelGGL((max_grad_kernel<1>), gr, blk, 0, stream, p, grad, max_indices, g_seq, g_stride, gshift);
    else hipLaunchKernelGGL((max_grad_kernel<2>), gr, blk, 0, stream, p, grad, max_indices, g_seq, g_stride, gshift);
    return hipGetLastError();
}

}  // namespace pm
