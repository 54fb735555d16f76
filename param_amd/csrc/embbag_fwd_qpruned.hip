// param_amd/csrc/embbag_fwd_qpruned.hip -- pooled lookup over ROW-QUANTISED tables of per-table format whose rows may be PRUNED:
// pm_embbag_fwd_qrows_pruned (include/param_amd.h "PRUNED TABLES").  Table t is embbag_fwd_qmixed.hip's: uint8
// [rows_t, rq::row_bytes(D_t, bits[t])], table_bits a device array of T ints (8 | 4).  A request addresses table t's LOGICAL rows;
// remap (device int32, the tables' remaps concatenated) and remap_offsets (device int64 [T + 1]) map them: table t is pruned iff
// remap_offsets[t + 1] > remap_offsets[t], its logical row r is physical row remap[remap_offsets[t] + r], or -1: the row is pruned.
//
// THE RULE (no new arithmetic): the lookups of a bag whose remap value is -1 are REMOVED -- index and weight alike, whatever the weight's
// value (it is loaded and never multiplied) --, the others take their remap value, and the rest is embbag_fwd_qmixed.hip's rule:
//     acc = fmaf(sc, (float)code[r, c], acc + bi)     in index order from +0.0; an empty or all-pruned bag gives +0.0
// The build has -ffp-contract=off.  A 16-bit output is ONE rounding of the fp32 value, in registers.
//
// HOW: qmixed_fwd_kernel's tile, bag and format structure (embbag_fwd_qmixed.hip -- its sibling: the existing kernels' code objects must
// not move and these kernels carry names of their own, so the row loop stands a third time; a fix to one belongs in the others).
//   * staged tiles: stage_tile_at has put the tile's indices in LDS and a tile belongs to one table, so the workgroup remaps them IN
//     PLACE, s_idx[i] = remap[base_t + s_idx[i]] -- one pass, all of the tile's dependent 4-byte loads in flight together, one barrier,
//     no extra LDS.  A pruned table is a tile-uniform branch; an un-pruned table skips the pass.
//   * unstaged tiles (more lookups than idx_cap): the U indices, then the U remap loads back to back, then the U row loads.
//   * in the row loop a negative entry issues no row load and no accumulate: the lanes of a lane group share the lookup, so the skip is
//     uniform across the group (lane groups of one wave differ: the skip is a predicate, the batch of U loads stays in flight).
// The geometry is plan_qmixed's alone (launch_plan.h).  No atomics, no inline assembly, no scratch memory, no workspace.
#include "common.h"
#include "fwd_elem.h"
#include "qrows_elem.h"

namespace pm {
namespace {

using namespace fwd;

constexpr int CV = kQmixedLaneColumns;     // columns per lane and column pass, whatever the format

// one lookup joins the sum: THE RULE, per column
template <int BITS, bool WEIGHTED>
__device__ __forceinline__ void accumulate_qp(float (&acc)[CV], const QLoadN<BITS, kQmixedDwords<BITS>>& q, float w) {
    constexpr int VEC = QRow<BITS>::kVec;
    float sc = q.tail.scale, bi = q.tail.bias;
    if (WEIGHTED) {
        sc = sc * w;
        bi = bi * w;
    }
#pragma unroll
    for (int h = 0; h < kQmixedDwords<BITS>; ++h) {
        float f[VEC];
        QRow<BITS>::unpack(q.raw[h], f);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float t = acc[h * VEC + k] + bi;
            acc[h * VEC + k] = fmaf(sc, f[k], t);
        }
    }
}

// a batch of U lookups whose PHYSICAL rows are r[u] (< 0: pruned): the rows' loads back to back under their predicates, then the sums
template <int BITS, bool WEIGHTED, bool ST, int U>
__device__ __forceinline__ void pool_batch(float (&acc)[CV], const char* W, const int64_t (&r)[U], const float (&w)[U], int64_t row_bytes, int code_off,
                                           int code_bytes) {
    constexpr int LD = kQmixedDwords<BITS>;
    QLoadN<BITS, LD> q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        q[u] = QLoadN<BITS, LD>{};
        if (r[u] >= 0) q[u] = load_row_n<BITS, LD>(W + row_offset<ST>(r[u], row_bytes), code_off, code_bytes);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (r[u] >= 0) accumulate_qp<BITS, WEIGHTED>(acc, q[u], w[u]);
}

// the tile's bags of table t, whose rows are BITS-bit.  s_idx holds PHYSICAL rows (remapped in place by the kernel, -1: pruned); an
// unstaged tile remaps as it goes: rmap = remap + remap_offsets[t] if the table is pruned, else nullptr.
template <int BITS, int G, bool WEIGHTED, typename OT, int U>
__device__ __forceinline__ void pool_tile(const KParams& p, int t, int64_t bag0, int nb, bool staged, const int32_t* rmap, const int64_t* s_off,
                                          const int32_t* s_idx, const float* s_w, float* s_out) {
    constexpr bool OUT16 = !std::is_same<OT, float>::value;
    constexpr int NG = kBlock / G;
    constexpr int VEC = QRow<BITS>::kVec;
    const int64_t base = s_off[0];
    uint16_t* s_out16 = reinterpret_cast<uint16_t*>(s_out);
    const int gid = threadIdx.x / G;
    const int lig = threadIdx.x % G;
    const int D = p.dims[t];
    const int code_bytes = D * BITS / 8;
    const int64_t row_bytes = rq::row_bytes(D, BITS);
    const char* W = reinterpret_cast<const char*>(p.tables[t]);
    float* out_t = p.io + p.out_offsets[t];
    // OUT16: io is the 16-bit output; offsets and strides count its 2-byte elements
    uint16_t* out16_t = reinterpret_cast<uint16_t*>(p.io) + p.out_offsets[t];
    const bool burst = p.stage_out > 0;

    for (int bg = gid; bg < nb; bg += NG) {
        const int64_t s = s_off[bg];
        const int64_t e = s_off[bg + 1];
        for (int c = lig * CV; c < D; c += G * CV) {
            const int code_off = c / VEC * 4;              // this lane's dword(s) of the row
            float acc[CV];
#pragma unroll
            for (int k = 0; k < CV; ++k) acc[k] = 0.0f;
            if (staged) {
                int j = static_cast<int>(s - base);
                const int je = static_cast<int>(e - base);
                for (; j + U <= je; j += U) {
                    int64_t r[U];
                    float w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        r[u] = s_idx[j + u];
                        w[u] = WEIGHTED ? s_w[j + u] : 1.0f;
                    }
                    pool_batch<BITS, WEIGHTED, true, U>(acc, W, r, w, row_bytes, code_off, code_bytes);
                }
                for (; j < je; ++j) {
                    const int64_t r[1] = {s_idx[j]};
                    const float w[1] = {WEIGHTED ? s_w[j] : 1.0f};
                    pool_batch<BITS, WEIGHTED, true, 1>(acc, W, r, w, row_bytes, code_off, code_bytes);
                }
            } else {
                // the tile's lookups exceed the index tile: indices (and weights) come from the request, then the remap loads back to back
                int64_t j = s;
                for (; j + U <= e; j += U) {
                    int64_t r[U];
                    float w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        r[u] = load_index(p.indices, j + u, p.idx64);
                        w[u] = WEIGHTED ? as_global<float>(p.psw)[j + u] : 1.0f;
                    }
                    if (rmap) {
#pragma unroll
                        for (int u = 0; u < U; ++u) r[u] = as_global<int32_t>(rmap)[r[u]];
                    }
                    pool_batch<BITS, WEIGHTED, false, U>(acc, W, r, w, row_bytes, code_off, code_bytes);
                }
                for (; j < e; ++j) {
                    int64_t r[1] = {load_index(p.indices, j, p.idx64)};
                    const float w[1] = {WEIGHTED ? as_global<float>(p.psw)[j] : 1.0f};
                    if (rmap) r[0] = as_global<int32_t>(rmap)[r[0]];
                    pool_batch<BITS, WEIGHTED, false, 1>(acc, W, r, w, row_bytes, code_off, code_bytes);
                }
            }
            // pieces of 4 outputs: eight columns per lane lie wholly inside the codes (D % 8 == 0)
            if constexpr (OUT16) {
                // the one rounding, in registers; 4 outputs = 8 bytes per piece
                u32x2 piece[CV / 4];
#pragma unroll
                for (int k = 0; k < CV; k += 4)
                    piece[k / 4] = u32x2{OT::round(acc[k]) | (OT::round(acc[k + 1]) << 16), OT::round(acc[k + 2]) | (OT::round(acc[k + 3]) << 16)};
                if (burst) {
                    u32x2* o2 = reinterpret_cast<u32x2*>(s_out16 + static_cast<size_t>(bg) * D + c);
#pragma unroll
                    for (int k = 0; k < CV / 4; ++k) o2[k] = piece[k];
                } else {
                    u32x2* o2 = reinterpret_cast<u32x2*>(out16_t + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                    for (int k = 0; k < CV / 4; ++k) __builtin_nontemporal_store(piece[k], o2 + k);
                }
            } else if (burst) {
                f32x4* o4 = reinterpret_cast<f32x4*>(s_out + static_cast<size_t>(bg) * D + c);
#pragma unroll
                for (int k = 0; k < CV; k += 4) o4[k / 4] = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
            } else {
                f32x4* o4 = reinterpret_cast<f32x4*>(out_t + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                for (int k = 0; k < CV; k += 4) {
                    f32x4 v = {acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
                    __builtin_nontemporal_store(v, o4 + k / 4);
                }
            }
        }
    }
    if (burst) {
        __syncthreads();
        if constexpr (OUT16) {
            const int q = D / 4;               // 8-byte pieces of 4 outputs per row
            for (int i = threadIdx.x; i < nb * q; i += kBlock) {
                const int bg = i / q, c4 = i % q;
                const u32x2 v = *reinterpret_cast<const u32x2*>(s_out16 + static_cast<size_t>(bg) * D + c4 * 4);
                __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(out16_t + (bag0 + bg) * p.out_stride + c4 * 4));
            }
        } else {
            burst_rows(s_out, out_t, bag0, p.out_stride, nb, D);
        }
    }
}

template <int G, bool WEIGHTED, typename OT, int U>
__global__ void __launch_bounds__(kBlock) qpruned_fwd_kernel(const KParams p, const int32_t* __restrict__ table_bits, const int32_t* __restrict__ remap,
                                                             const int64_t* __restrict__ remap_offsets) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    int t, tile;
    block_to_tile(p, t, tile);
    if (t >= p.T) return;
    const int64_t bag0 = p.bag_begin + static_cast<int64_t>(tile) * p.bags_per_block;
    const int64_t left_bags = p.bag_begin + p.bag_count - bag0;
    if (left_bags <= 0) return;
    const int nb = left_bags < p.bags_per_block ? static_cast<int>(left_bags) : p.bags_per_block;

    int64_t* s_off;
    int32_t* s_idx;
    float* s_w;
    const bool staged = stage_tile_at<WEIGHTED>(p, t, bag0, nb, smem, s_off, s_idx, s_w);
    float* s_out = reinterpret_cast<float*>(smem + (tile_lds_bytes(p.bags_per_block, p.idx_cap, WEIGHTED) + 15) / 16 * 16);

    // the tile's remap: one table, two scalar loads, one branch.  Staged: logical -> physical rows in place, the tile's loads in flight
    // together (stage_tile_at's last barrier stands in front: every entry is written; each thread remaps the entries it reads)
    const int64_t rbase = remap_offsets[t];
    const int32_t* rmap = remap_offsets[t + 1] > rbase ? remap + rbase : nullptr;
    if (staged && rmap) {
        const int cnt = static_cast<int>(s_off[nb] - s_off[0]);
        for (int i = threadIdx.x; i < cnt; i += kBlock) s_idx[i] = as_global<int32_t>(rmap)[s_idx[i]];
        __syncthreads();
    }

    // the tile's format: one table, one scalar load, one branch
    if (table_bits[t] == 8)
        pool_tile<8, G, WEIGHTED, OT, U>(p, t, bag0, nb, staged, rmap, s_off, s_idx, s_w, s_out);
    else
        pool_tile<4, G, WEIGHTED, OT, U>(p, t, bag0, nb, staged, rmap, s_off, s_idx, s_w, s_out);
}

// the launcher ladder: group width, weighted, output element, rows in flight
template <int G, typename OT>
hipError_t launch_qp_w(const KParams& p0, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, int unroll, hipStream_t stream) {
    KParams p = p0;
    const bool weighted = p.psw != nullptr;
    const int grid = p.T * p.tiles_per_table;
    const size_t tile_lds = (tile_lds_bytes(p.bags_per_block, p.idx_cap, weighted) + 15) / 16 * 16;
    size_t lds = tile_lds + (p.stage_out > 0 ? static_cast<size_t>(p.bags_per_block) * p.stage_out * sizeof(typename std::conditional<std::is_same<OT, float>::value, float, uint16_t>::type) : 0);
    if (lds > 65536) {                         // (explicit 1024-bag tiles of a weighted request: rows leave one by one)
        p.stage_out = 0;
        lds = tile_lds;
    }
    dispatch_bool(weighted, [&](auto w) {
        dispatch_bool(unroll >= 4, [&](auto deep) {
            constexpr int U = decltype(deep)::value ? 4 : 2;
            hipLaunchKernelGGL((qpruned_fwd_kernel<G, decltype(w)::value, OT, U>), dim3(grid), dim3(kBlock), lds, stream, p, table_bits, remap, remap_offsets);
        });
    });
    return hipGetLastError();
}

template <typename OT>
hipError_t launch_qp_g(const KParams& p, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, int max_dim, int unroll,
                       hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, kQmixedLaneColumns),
                                [&](auto g) { return launch_qp_w<decltype(g)::value, OT>(p, table_bits, remap, remap_offsets, unroll, stream); });
}

}  // namespace

// p.io = out of out_dtype (PM_F32 | PM_BF16 | PM_F16), addressed in its elements; table_bits: device int32 [T], 8 | 4; remap: device int32;
// remap_offsets: device int64 [T + 1]; unroll: plan_qmixed's (2 | 4)
hipError_t launch_embbag_fwd_qpruned(const KParams& p, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, int out_dtype,
                                     int max_dim, int unroll, hipStream_t stream) {
    if (out_dtype == PM_BF16) return launch_qp_g<OutBF16>(p, table_bits, remap, remap_offsets, max_dim, unroll, stream);
    if (out_dtype == PM_F16) return launch_qp_g<OutF16>(p, table_bits, remap, remap_offsets, max_dim, unroll, stream);
    return launch_qp_g<float>(p, table_bits, remap, remap_offsets, max_dim, unroll, stream);
}

}  // namespace pm
