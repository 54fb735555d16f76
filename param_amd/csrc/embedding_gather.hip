// param_amd/csrc/embedding_gather.hip -- pm_embedding_gather: the UN-POOLED lookup (nn.Embedding, fbgemm TBE's sequence embeddings).
// out[j] = conv(table_t[indices[j]]) for every lookup position j of the bag slice, t = the table that owns position j.  gfx950 only.
//
// A tile is kBlock consecutive POSITIONS of the index array (launch_plan.h: plan_gather), not a (table, bag) block: the output is
// addressed by position, so a tile may straddle table borders and nothing in it depends on bags.
//   1. every thread loads the index of its own position (one coalesced load) and finds the position's table among the T borders
//      offsets[t * B] -- "the last table whose first bag starts at or before j", bag_start_or_end's rule and the bounds check's --
//      in an LDS copy of the borders (T + 1 <= kGatherLdsBorders) or by a binary search of them in global memory;
//   2. it turns (table, row) into the row's address and width once -- one 32 x 32-bit multiply (row_offset) -- and hands both to the
//      lane groups through LDS; a position outside the bag slice, or outside every table, gets width 0 and is never touched;
//   3. a lane group of G lanes moves one row with 16-byte loads (load16: global_load_dwordx4, plain, so recurring rows stay in L2)
//      and non-temporal stores (the output is written once): 16-byte pieces of fp32, 8-byte pieces of 16-bit output.  It keeps U rows
//      in flight and issues the NEXT batch of row loads before it stores the batch it holds: loads and stores retire through one
//      in-order counter, so a wait for loads that were issued behind a batch of stores would wait for those stores as well.
// Same element type in and out: the 16 bytes leave as they came -- no arithmetic touches them (-0.0, NaN payloads, subnormals).
// Otherwise Elem<WT>::widen (exact) and, for a 16-bit output, the one rounding of OutBF16 / OutF16 (fwd_elem.h).
// No atomics, no scalar-unit memory writes, no inline assembly.
#include "common.h"
#include "fwd_elem.h"

namespace pm {
namespace {

using namespace fwd;

template <typename WT, typename OT>
struct SameBits : std::false_type {};
template <> struct SameBits<float, float> : std::true_type {};
template <> struct SameBits<bf16_t, OutBF16> : std::true_type {};
template <> struct SameBits<f16_t, OutF16> : std::true_type {};

// the VEC elements one lane loaded, converted and stored at dst (VEC output elements: 16-byte aligned fp32, 8-byte aligned 16-bit)
template <typename WT, typename OT>
__device__ __forceinline__ void store_converted(char* dst, const u32x4& raw) {
    constexpr int VEC = Elem<WT>::kVec;
    if constexpr (SameBits<WT, OT>::value && std::is_same<OT, float>::value) {
        __builtin_nontemporal_store(raw, as_global<u32x4>(dst));
    } else if constexpr (SameBits<WT, OT>::value) {
        __builtin_nontemporal_store(u32x2{raw.x, raw.y}, as_global<u32x2>(dst));
        __builtin_nontemporal_store(u32x2{raw.z, raw.w}, as_global<u32x2>(dst) + 1);
    } else {
        float f[VEC];
        Elem<WT>::widen(raw, f);
#pragma unroll
        for (int k = 0; k < VEC; k += 4) {
            if constexpr (std::is_same<OT, float>::value) {
                const f32x4 v = {f[k], f[k + 1], f[k + 2], f[k + 3]};
                __builtin_nontemporal_store(v, as_global<f32x4>(dst) + k / 4);
            } else {
                const u32x2 v = {OT::round(f[k]) | (OT::round(f[k + 1]) << 16), OT::round(f[k + 2]) | (OT::round(f[k + 3]) << 16)};
                __builtin_nontemporal_store(v, as_global<u32x2>(dst) + k / 4);
            }
        }
    }
}

// p.io = out, p.out_stride = out_row_stride (output elements); p.out_offsets is not read
template <typename WT, typename OT, int G, int U>
__global__ void __launch_bounds__(kBlock) embedding_gather_kernel(const KParams p, const int col_passes, const int lds_borders, const int xcd_contiguous) {
    constexpr int VEC = Elem<WT>::kVec;
    constexpr int ES = 16 / VEC;
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    constexpr int NG = kBlock / G;
    constexpr int NB = G / U;                  // batches of U rows: a lane group owns kBlock / NG = G positions of the tile
    static_assert(G % U == 0, "the unroll divides the positions of a lane group");
    __shared__ int64_t s_border[kGatherLdsBorders];
    __shared__ int64_t s_src[kBlock];          // address of the position's row
    __shared__ int32_t s_dim[kBlock];          // its width in elements; 0: the position is not written

    const int tid = static_cast<int>(threadIdx.x);
    const int64_t j0 = gather_block_tile(blockIdx.x, gridDim.x, xcd_contiguous != 0) * kBlock;
    const int64_t j = j0 + tid;
    const bool inside = j < p.N;
    int64_t r = 0;
    if (inside) r = load_index(p.indices, j, p.idx64);

    // the position's table: borders b[t] = offsets[t * B] at or before j, minus one (-1: in front of every table)
    int lo = 0, hi = p.T;
    if (lds_borders) {
        if (tid < p.T) s_border[tid] = load_index(p.offsets, static_cast<int64_t>(tid) * p.B, p.idx64);
        __syncthreads();
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_border[mid] <= j) lo = mid + 1; else hi = mid;
        }
    } else {
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (load_index(p.offsets, static_cast<int64_t>(mid) * p.B, p.idx64) <= j) lo = mid + 1; else hi = mid;
        }
    }
    const int t = lo - 1;
    bool ok = inside && t >= 0;
    if (ok && (p.bag_begin != 0 || p.bag_count != p.B)) {
        const int64_t g0 = static_cast<int64_t>(t) * p.B + p.bag_begin;
        ok = j >= bag_start_or_end(p, g0) && j < bag_start_or_end(p, g0 + p.bag_count);
    }
    // A position that is not written still gets a readable address (table 0's first row) and width 0: the row loads below are
    // unconditional -- straight-line code whose waits the compiler can count -- and only the stores are predicated.
    int D = 0;
    int64_t src = reinterpret_cast<int64_t>(p.tables[0]);
    if (ok) {
        D = p.dims[t];
        src = reinterpret_cast<int64_t>(p.tables[t]) + row_offset<true>(r, static_cast<int64_t>(D) * ES);
    }
    s_src[tid] = src;
    s_dim[tid] = D;
    __syncthreads();

    const int gid = tid / G;
    const int lig = tid % G;
    char* out = reinterpret_cast<char*>(p.io);
    for (int pass = 0; pass < col_passes; ++pass) {   // rows wider than one group pass (fp32 D > 256)
        const int c = (pass * G + lig) * VEC;
        // a batch: the U rows' addresses and widths from LDS first, then the U loads back to back (a lane past the row's width
        // reads the row's first 16 bytes and stores nothing)
        auto fetch = [&](int b, u32x4 (&raw)[U], int (&dim)[U]) {
            int64_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                a[u] = s_src[q];
                dim[u] = s_dim[q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) raw[u] = load16(reinterpret_cast<const char*>(a[u]) + (c < dim[u] ? c * ES : 0), false);
        };
        auto emit = [&](int b, const u32x4 (&raw)[U], const int (&dim)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                if (c < dim[u]) store_converted<WT, OT>(out + ((j0 + q) * p.out_stride + c) * OB, raw[u]);
            }
        };
        // Two batches ping-pong between two register sets, each fetched in front of the other's stores; no set is ever copied (a
        // copy waits for its loads, and through the in-order counter for the stores in front of them).  Kept a loop: unrolled, the
        // compiler hoists every batch's loads to the front -- G rows in flight whatever U says, on 170+ registers.
        u32x4 ra[U], rb[U];
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
hipError_t launch_gather_u(const KParams& p, const GatherPlan& g, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(g.grid)), block(kBlock);
    auto launch = [&](auto u) {
        hipLaunchKernelGGL((embedding_gather_kernel<WT, OT, G, decltype(u)::value>), grid, block, 0, stream, p, g.col_passes, g.lds_borders,
                           g.xcd_contiguous);
    };
    switch (g.unroll) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        default: launch(std::integral_constant<int, 4>{}); break;
    }
    return hipGetLastError();
}

template <typename WT, typename OT>
hipError_t launch_gather_g(const KParams& p, const GatherPlan& g, hipStream_t stream) {
    return dispatch_group_lanes(g.group_lanes, [&](auto gl) { return launch_gather_u<WT, OT, decltype(gl)::value>(p, g, stream); });
}

template <typename WT>
hipError_t launch_gather_o(const KParams& p, int out_dtype, const GatherPlan& g, hipStream_t stream) {
    if (out_dtype == PM_BF16) return launch_gather_g<WT, OutBF16>(p, g, stream);
    if (out_dtype == PM_F16) return launch_gather_g<WT, OutF16>(p, g, stream);
    return launch_gather_g<WT, float>(p, g, stream);
}

}  // namespace

hipError_t launch_embedding_gather(const KParams& p, int weight_dtype, int out_dtype, const GatherPlan& g, hipStream_t stream) {
    if (weight_dtype == PM_BF16) return launch_gather_o<bf16_t>(p, out_dtype, g, stream);
    if (weight_dtype == PM_F16) return launch_gather_o<f16_t>(p, out_dtype, g, stream);
    return launch_gather_o<float>(p, out_dtype, g, stream);
}

}  // namespace pm
