// param_amd/csrc/embedding_gather_f8s.hip -- pm_embedding_gather_f8_scaled: the UN-POOLED lookup over SCALED FP8 tables (include/param_amd.h,
// SCALED FP8 TABLES).  out[j, c] = conv(dec(table_t[indices[j], c]) * 2^(E_t + e_r)) for every lookup position j of the bag slice.
// gfx950 only.
//
// pm_embedding_gather_f8's kernel (embedding_gather_f8.hip, which says what the tiles are) with one more LDS word per position: the
// thread that resolves position j to (table, row) also reads E_t and the row's exponent byte and hands 2^(E_t + e_r), built from its
// bits (f8s_elem.h: pow2, the sum clamped to [-64, 64]), to the lane groups next to the row's address; a lane multiplies its four
// widened columns by it -- exact -- in front of the one rounding of a 16-bit output.  Same geometry: plan_gather_f8's.
// No atomics, no scalar-unit memory writes, no inline assembly.
#include "common.h"
#include "fwd_elem.h"
#include "f8s_elem.h"

namespace pm {
namespace {

using namespace fwd;

__device__ __forceinline__ uint32_t load4(const char* p) { return *as_global<uint32_t>(p); }   // global_load_dword

// p.io = out, p.out_stride = out_row_stride (output elements); p.out_offsets is not read
template <typename WT, typename OT, int G, int U>
__global__ void __launch_bounds__(kBlock) embedding_gather_f8s_kernel(const KParams p, const int col_passes, const int lds_borders, const int xcd_contiguous,
                                                                      const int32_t* __restrict__ table_exp, const int8_t* const* __restrict__ row_exp) {
    constexpr int LC = kF8GatherLaneColumns;   // columns = table bytes per lane and pass
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    constexpr int NG = kBlock / G;
    constexpr int NB = G / U;                  // batches of U rows: a lane group owns kBlock / NG = G positions of the tile
    static_assert(G % U == 0, "the unroll divides the positions of a lane group");
    static_assert(LC == 4, "a lane's columns are one dword");
    __shared__ int64_t s_border[kGatherLdsBorders];
    __shared__ int64_t s_src[kBlock];          // address of the position's row
    __shared__ int32_t s_dim[kBlock];          // its width in columns; 0: the position is not written
    __shared__ float s_scale[kBlock];          // 2^(E_t + e_r) of its row

    const int tid = static_cast<int>(threadIdx.x);
    const int64_t j0 = gather_block_tile(blockIdx.x, gridDim.x, xcd_contiguous != 0) * kBlock;
    const int64_t j = j0 + tid;
    const bool inside = j < p.N;
    int64_t r = 0;
    if (inside) r = load_index(p.indices, j, p.idx64);
    const int t = gather_position_table(p, lds_borders, s_border, j, inside);
    // A position that is not written still gets a readable address (table 0's first row) and width 0: the row loads below are
    // unconditional and only the stores are predicated.
    int D = 0;
    int64_t src = reinterpret_cast<int64_t>(p.tables[0]);
    int e = 0;
    if (t >= 0) {
        D = p.dims[t];
        src = reinterpret_cast<int64_t>(p.tables[t]) + row_offset<true>(r, static_cast<int64_t>(D));
        if (table_exp) e = table_exp[t];
        if (row_exp) e += as_global<int8_t>(row_exp[t])[r];
    }
    s_src[tid] = src;
    s_dim[tid] = D;
    s_scale[tid] = f8s::pow2(f8s::clamp_exp(e));
    __syncthreads();

    const int gid = tid / G;
    const int lig = tid % G;
    char* out = reinterpret_cast<char*>(p.io);
    for (int pass = 0; pass < col_passes; ++pass) {   // rows wider than one group pass (D > 256)
        const int c = (pass * G + lig) * LC;
        // a batch: the U rows' addresses and widths from LDS first, then the U loads back to back (a lane past the row's width reads
        // the row's first dword and stores nothing)
        auto fetch = [&](int b, uint32_t (&raw)[U], int (&dim)[U]) {
            int64_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                a[u] = s_src[q];
                dim[u] = s_dim[q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) raw[u] = load4(reinterpret_cast<const char*>(a[u]) + (c < dim[u] ? c : 0));
        };
        auto emit = [&](int b, const uint32_t (&raw)[U], const int (&dim)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                if (c < dim[u]) {
                    float f[4];
                    widen_f8_dword<WT>(raw[u], f);
                    const float sc = s_scale[q];
#pragma unroll
                    for (int k = 0; k < 4; ++k) f[k] *= sc;
                    char* dst = out + ((j0 + q) * p.out_stride + c) * OB;
                    if constexpr (std::is_same<OT, float>::value) {
                        const f32x4 v = {f[0], f[1], f[2], f[3]};
                        __builtin_nontemporal_store(v, as_global<f32x4>(dst));
                    } else {
                        const u32x2 v = {OT::round(f[0]) | (OT::round(f[1]) << 16), OT::round(f[2]) | (OT::round(f[3]) << 16)};
                        __builtin_nontemporal_store(v, as_global<u32x2>(dst));
                    }
                }
            }
        };
        // two batches ping-pong between two register sets; kept a loop (embedding_gather.hip says why)
        uint32_t ra[U], rb[U];
        int da[U], db[U];
        fetch(0, ra, da);
        if constexpr (NB == 1) {
            emit(0, ra, da);
        } else {
#pragma unroll 1
            for (int b = 0; b + 2 < NB; b += 2) {
                fetch(b + 1, rb, db);
                emit(b, ra, da);
                fetch(b + 2, ra, da);
                emit(b + 1, rb, db);
            }
            fetch(NB - 1, rb, db);
            emit(NB - 2, ra, da);
            emit(NB - 1, rb, db);
        }
    }
}

template <typename WT, typename OT, int G>
hipError_t launch_gather_f8s_u(const KParams& p, const GatherPlan& g, const int32_t* table_exp, const int8_t* const* row_exp, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(g.grid)), block(kBlock);
    auto launch = [&](auto u) {
        hipLaunchKernelGGL((embedding_gather_f8s_kernel<WT, OT, G, decltype(u)::value>), grid, block, 0, stream, p, g.col_passes, g.lds_borders,
                           g.xcd_contiguous, table_exp, row_exp);
    };
    switch (g.unroll) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        default: launch(std::integral_constant<int, 4>{}); break;
    }
    return hipGetLastError();
}

template <typename WT>
hipError_t launch_gather_f8s_o(const KParams& p, int out_dtype, const GatherPlan& g, const int32_t* table_exp, const int8_t* const* row_exp,
                               hipStream_t stream) {
    auto go = [&](auto gl) {
        constexpr int G = decltype(gl)::value;
        if (out_dtype == PM_BF16) return launch_gather_f8s_u<WT, OutBF16, G>(p, g, table_exp, row_exp, stream);
        if (out_dtype == PM_F16) return launch_gather_f8s_u<WT, OutF16, G>(p, g, table_exp, row_exp, stream);
        return launch_gather_f8s_u<WT, float, G>(p, g, table_exp, row_exp, stream);
    };
    return dispatch_group_lanes(g.group_lanes, go);
}

}  // namespace

hipError_t launch_embedding_gather_f8s(const KParams& p, int weight_dtype, int out_dtype, const GatherPlan& g, const int32_t* table_exp,
                                       const int8_t* const* row_exp, hipStream_t stream) {
    if (weight_dtype == PM_F8E5M2) return launch_gather_f8s_o<f8e5m2_t>(p, out_dtype, g, table_exp, row_exp, stream);
    return launch_gather_f8s_o<f8e4m3_t>(p, out_dtype, g, table_exp, row_exp, stream);
}

}  // namespace pm
