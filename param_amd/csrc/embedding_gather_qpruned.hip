// param_amd/csrc/embedding_gather_qpruned.hip -- pm_embedding_gather_qrows_pruned: the UN-POOLED lookup over ROW-QUANTISED tables of
// per-table format whose rows may be PRUNED (include/param_amd.h "PRUNED TABLES").  table_bits: device int32 [T],
// 8 | 4; remap: device int32, the tables' remaps concatenated; remap_offsets: device int64 [T + 1] -- table t is pruned iff
// remap_offsets[t + 1] > remap_offsets[t], its logical row r is physical row remap[remap_offsets[t] + r], or -1.  gfx950 only.
//
// THE RULE is embedding_gather_qmixed.hip's over the remapped row: for every lookup position j of the bag slice, t the table that owns j,
// r = the physical row of indices[j], per column c < D_t
//     r >= 0:  out[j, c] = conv( fmaf(scale_r, (float)code[r, c], fl32(+0.0f + bias_r)) )
//     r <  0:  out[j, c] = +0.0 of the output dtype          (a pruned row; what fbgemm's nobag kernel writes)
// -- no new arithmetic.  Positions outside the slice are not touched.  The build has -ffp-contract=off.
//
// HOW: qmixed_gather_kernel's tiles and steps (embedding_gather_qmixed.hip -- its sibling: the existing kernels' code objects must not move,
// so the steps stand again under names of their own; a fix to one belongs in the other).  In step 1 each thread has its index and its
// table: the remap load stands there, in front of the row address that goes to LDS.  PRUNED is a third state of a position beside
// "width D" and "width 0, never written": bit 17 of the width word.  The lane group keeps its unconditional loads -- of a pruned position
// they read table 0's first 8 bytes twice, as for a position of width 0 (tables[0] points at 8 readable bytes: the caller's contract) --
// and stores pieces of zeros under the same column predicate.  One instruction stream, selected per lane by values, never by a branch.
// The geometry is plan_gather_qmixed's alone.  No atomics, no inline assembly, no scratch.
#include "common.h"
#include "fwd_elem.h"
#include "qrows_elem.h"

namespace pm {
namespace {

using namespace fwd;

constexpr int CV = kQmixedLaneColumns;     // columns per lane and column pass, whatever the format
constexpr int kFourBit = 1 << 16;          // in a position's width word: the row is 4-bit (widths are at most kQrowsMaxDim = 4096)
constexpr int kPruned = 1 << 17;           // ... the row is pruned: zeros are stored, the address is table 0's first row

// one row's codes of this lane and its tail, as loaded: two dwords each, whatever the format
struct PrunedLoad {
    u32x2_a4 codes, tail;
};
// c: the lane's first column if it lies below the row's width and the row is not pruned, else 0; dimw: the width word
__device__ __forceinline__ PrunedLoad load_pruned(const char* row, int c, int dimw) {
    const int four = (dimw >> 16) & 1;
    const int dim = dimw & 0xffff;
    PrunedLoad q;
    q.codes = *as_global<u32x2_a4>(row + (c >> four));
    // 8-bit: scale, bias at row + D.  4-bit: at row + D / 2 - 4 the last code dword, then the tail.  Width 0 or pruned: the first bytes.
    int toff = four ? (dim >> 1) - 4 : dim;
    if (dimw & kPruned) toff = 0;
    q.tail = *as_global<u32x2_a4>(row + (toff > 0 ? toff : 0));
    return q;
}

// One row's pieces of 4 outputs leave: embedding_gather_qmixed.hip's store_mixed; a pruned row's pieces are +0.0 by value.
// row_out: the position's output row; c0: the pass's first column.
template <typename OT, int G>
__device__ __forceinline__ void store_pruned(char* row_out, const PrunedLoad& q, int lig, int c0, int dimw) {
    constexpr int P = CV / 4;                                  // pieces per lane and pass
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    static_assert(P == 2 && G % P == 0, "a lane group's pieces divide over its stores");
    const bool four = (dimw & kFourBit) != 0;
    const bool pruned = (dimw & kPruned) != 0;
    const int dim = dimw & 0xffff;
    float scale, bias;
    if (four) {
        scale = rq::half_value(static_cast<uint16_t>(q.tail[1] & 0xffffu));
        bias = rq::half_value(static_cast<uint16_t>(q.tail[1] >> 16));
    } else {
        scale = __uint_as_float(q.tail[0]);
        bias = __uint_as_float(q.tail[1]);
    }
    const float t = 0.0f + bias;
    const int slot = lig % P;                                  // which of the source lane's pieces this lane takes
    const uint32_t width = four ? 4u : 8u;                     // bits per code
    const uint32_t mask = four ? 0xfu : 0xffu;
#pragma unroll
    for (int s = 0; s < P; ++s) {
        const int src = s * (G / P) + lig / P;
        const uint32_t v0 = static_cast<uint32_t>(__shfl(static_cast<int>(q.codes[0]), src, G));
        const uint32_t v1 = static_cast<uint32_t>(__shfl(static_cast<int>(q.codes[1]), src, G));
        // the piece's codes in the low 4 * width bits: a dword of an 8-bit row, a 16-bit half of a 4-bit row's first dword
        const uint32_t w = four ? (v0 >> (16 * slot)) : (slot ? v1 : v0);
        float f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = fmaf(scale, static_cast<float>((w >> (k * width)) & mask), t);
            f[k] = pruned ? 0.0f : v;
        }
        const int c = c0 + (s * G + lig) * 4;
        if (c < dim) {
            if constexpr (std::is_same<OT, float>::value) {
                const f32x4 v = {f[0], f[1], f[2], f[3]};
                __builtin_nontemporal_store(v, as_global<f32x4>(row_out + c * OB));
            } else {
                const u32x2 v = {OT::round(f[0]) | (OT::round(f[1]) << 16), OT::round(f[2]) | (OT::round(f[3]) << 16)};
                __builtin_nontemporal_store(v, as_global<u32x2>(row_out + c * OB));
            }
        }
    }
}

// p.io = out, p.out_stride = out_row_stride (output elements); p.out_offsets and p.psw are not read
template <typename OT, int G, int U>
__global__ void __launch_bounds__(kBlock) qpruned_gather_kernel(const KParams p, const int32_t* __restrict__ table_bits, const int32_t* __restrict__ remap,
                                                                const int64_t* __restrict__ remap_offsets, const int col_passes, const int lds_borders,
                                                                const int xcd_contiguous) {
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    constexpr int NG = kBlock / G;
    constexpr int NB = G / U;                  // batches of U rows: a lane group owns kBlock / NG = G positions of the tile
    static_assert(G % U == 0, "the unroll divides the positions of a lane group");
    __shared__ int64_t s_border[kGatherLdsBorders];
    __shared__ int32_t s_bits[kGatherLdsBorders];
    __shared__ int64_t s_src[kBlock];          // address of the position's row
    __shared__ int32_t s_dim[kBlock];          // its width word: columns | kFourBit | kPruned; 0: the position is not written

    const int tid = static_cast<int>(threadIdx.x);
    const int64_t j0 = gather_block_tile(blockIdx.x, gridDim.x, xcd_contiguous != 0) * kBlock;
    const int64_t j = j0 + tid;
    const bool inside = j < p.N;
    int64_t r = 0;
    if (inside) r = load_index(p.indices, j, p.idx64);

    if (lds_borders && tid < p.T) s_bits[tid] = table_bits[tid];      // (gather_position_table's barrier stands behind this)
    const int t = gather_position_table(p, lds_borders, s_border, j, inside);
    // a position that is not written: table 0's first row and width 0 -- the loads below are unconditional, only the stores are predicated
    int dimw = 0;
    int64_t src = reinterpret_cast<int64_t>(p.tables[0]);
    if (t >= 0) {
        // the position's remap: logical -> physical row, in front of the row's address
        const int64_t rbase = as_global<int64_t>(remap_offsets)[t];
        if (as_global<int64_t>(remap_offsets)[t + 1] > rbase) r = as_global<int32_t>(remap)[rbase + r];
        const int D = p.dims[t];
        int bits;                              // (two address spaces, kept apart: an LDS read or a global load, never a flat one)
        if (lds_borders) bits = s_bits[t];
        else bits = *as_global<int32_t>(table_bits + t);
        const bool four = bits != 8;
        dimw = D | (four ? kFourBit : 0);
        if (r >= 0) src = reinterpret_cast<int64_t>(p.tables[t]) + row_offset<true>(r, four ? rq::row_bytes(D, 4) : rq::row_bytes(D, 8));
        else dimw |= kPruned;                  // (src stays table 0's first row)
    }
    s_src[tid] = src;
    s_dim[tid] = dimw;
    __syncthreads();

    const int gid = tid / G;
    const int lig = tid % G;
    char* out = reinterpret_cast<char*>(p.io);
    for (int pass = 0; pass < col_passes; ++pass) {   // rows wider than one group pass (D > 512)
        const int c = (pass * G + lig) * CV;
        // a batch: the U rows' addresses and widths from LDS first, then the U rows' loads back to back (a lane past the row's width, or
        // of a pruned row, reads the row's first dwords; the former stores nothing, the latter zeros)
        auto fetch = [&](int b, PrunedLoad (&raw)[U], int (&dim)[U]) {
            int64_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                a[u] = s_src[q];
                dim[u] = s_dim[q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                raw[u] = load_pruned(reinterpret_cast<const char*>(a[u]), (c < (dim[u] & 0xffff) && !(dim[u] & kPruned)) ? c : 0, dim[u]);
            // nothing moves across this point (embedding_gather_qrows.hip: the scheduler otherwise lifts the first row's code exchange
            // in between the loads)
            __builtin_amdgcn_sched_barrier(0);
        };
        auto emit = [&](int b, const PrunedLoad (&raw)[U], const int (&dim)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                store_pruned<OT, G>(out + (j0 + q) * p.out_stride * OB, raw[u], lig, pass * G * CV, dim[u]);
            }
        };
        // embedding_gather.hip's ping-pong: two register sets, each fetched in front of the other's stores, none ever copied
        PrunedLoad ra[U], rb[U];
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

template <typename OT, int G>
hipError_t launch_qpgather_u(const KParams& p, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, const GatherPlan& g,
                             hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(g.grid)), block(kBlock);
    auto launch = [&](auto u) {
        hipLaunchKernelGGL((qpruned_gather_kernel<OT, G, decltype(u)::value>), grid, block, 0, stream, p, table_bits, remap, remap_offsets, g.col_passes,
                           g.lds_borders, g.xcd_contiguous);
    };
    switch (g.unroll) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        default: launch(std::integral_constant<int, 4>{}); break;
    }
    return hipGetLastError();
}

template <typename OT>
hipError_t launch_qpgather_g(const KParams& p, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, const GatherPlan& g,
                             hipStream_t stream) {
    return dispatch_group_lanes(g.group_lanes,
                                [&](auto gl) { return launch_qpgather_u<OT, decltype(gl)::value>(p, table_bits, remap, remap_offsets, g, stream); });
}

}  // namespace

// p.io = out of out_dtype (PM_F32 | PM_BF16 | PM_F16), p.out_stride = its row stride in elements; table_bits: device int32 [T]; remap: device
// int32; remap_offsets: device int64 [T + 1]; g: plan_gather_qmixed's
hipError_t launch_embedding_gather_qpruned(const KParams& p, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, int out_dtype,
                                           const GatherPlan& g, hipStream_t stream) {
    if (out_dtype == PM_BF16) return launch_qpgather_g<OutBF16>(p, table_bits, remap, remap_offsets, g, stream);
    if (out_dtype == PM_F16) return launch_qpgather_g<OutF16>(p, table_bits, remap, remap_offsets, g, stream);
    return launch_qpgather_g<float>(p, table_bits, remap, remap_offsets, g, stream);
}

}  // namespace pm
