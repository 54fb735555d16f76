// param_amd/csrc/embbag_fwd_qmixed.hip -- pooled lookup over ROW-QUANTISED tables that are EACH stored in the 8- or the 4-bit format:
// pm_embbag_fwd_qrows_mixed (include/param_amd.h).  Table t is uint8 [rows_t, rq::row_bytes(D_t, bits[t])], the
// bytes of embbag_fwd_qrows.hip's tables; table_bits is a device array of T ints (8 | 4), read by the kernel like dims.
//
// THE RULE is embbag_fwd_qrows.hip's, per table with that table's format: the lookups j of a bag in index order, from acc = +0.0, per column
//     sc = scale_r * w_j     bi = bias_r * w_j        (unweighted: sc = scale_r, bi = bias_r; no multiplication happens)
//     acc = fmaf(sc, (float)code[r, c], acc + bi)     r = indices[j]
// -- no new arithmetic: the columns of table t are bit for bit pm_embbag_fwd_qrows' for that table alone with bits = bits[t].  The build
// has -ffp-contract=off.  A 16-bit output is ONE rounding of the fp32 value (OutBF16 / OutF16, fwd_elem.h), in registers.
//
// HOW: qrows_fwd_kernel's tile and bag structure.  A tile's bags belong to one table, so the format is uniform per workgroup: the body
// reads table_bits[t] once (a scalar load) and branches ONCE per tile into the 8-bit or the 4-bit instance of the same row loop.  A lane
// holds EIGHT COLUMNS per row in both (qrows_elem.h: load_row_n -- global_load_dwordx2 of an 8-bit row, global_load_dword of a 4-bit row,
// at dword-aligned addresses), so the lane group G = group_lanes(max_dim, 8), the eight accumulators, the column passes and the output
// pieces are the same for every table; only the load and the unpack differ.  Widths are multiples of 8: a lane's columns are wholly
// inside the codes or the lane has nothing to do -- no lane reads behind a row's codes but for the tail every lane of the group reads.
// Kept from qrows_fwd_kernel: the staged and unstaged index paths, U rows in flight, the LDS output burst, the 16-bit output path,
// 64-bit row offsets, non-temporal output stores.  The geometry is plan_qmixed's alone (launch_plan.h).  No atomics, no scratch memory,
// no workspace.
#include "common.h"
#include "fwd_elem.h"
#include "qrows_elem.h"

namespace pm {
namespace {

using namespace fwd;

// Dwords of codes a lane holds of a row: the product's kQmixedDwords (8 bits: 2, 4 bits: 1 -- eight columns either way).  The experiment
// build -DPM_QMIXED_4BIT_DWORDS=2 gives a 4-bit row two dwords, 16 columns per lane, in lane groups still sized for eight (launch_plan.h
// has both layouts' times): a lane's second dword may then lie behind the codes (D % 16 == 8) -- the row's own tail -- and gives no output.
#ifndef PM_QMIXED_4BIT_DWORDS
#define PM_QMIXED_4BIT_DWORDS 1
#endif
template <int BITS> constexpr int kLD = BITS == 4 ? PM_QMIXED_4BIT_DWORDS : kQmixedDwords<BITS>;
static_assert(kLD<4> == 1 || kLD<4> == 2, "PM_QMIXED_4BIT_DWORDS must be 1 or 2");

// one lookup joins the sum: THE RULE, per column
template <int BITS, bool WEIGHTED>
__device__ __forceinline__ void accumulate_qn(float (&acc)[QRow<BITS>::kVec * kLD<BITS>], const QLoadN<BITS, kLD<BITS>>& q, float w) {
    constexpr int VEC = QRow<BITS>::kVec;
    float sc = q.tail.scale, bi = q.tail.bias;
    if (WEIGHTED) {
        sc = sc * w;
        bi = bi * w;
    }
#pragma unroll
    for (int h = 0; h < kLD<BITS>; ++h) {
        float f[VEC];
        QRow<BITS>::unpack(q.raw[h], f);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float t = acc[h * VEC + k] + bi;
            acc[h * VEC + k] = fmaf(sc, f[k], t);
        }
    }
}

// the tile's bags of table t, whose rows are BITS-bit: qrows_fwd_kernel's row loop (embbag_fwd_qrows.hip -- its TWIN: the existing
// kernels' code objects must not move and these kernels carry names of their own, so the loop stands twice; a fix to one belongs in
// the other) on this file's dwords per lane
template <int BITS, int G, bool WEIGHTED, typename OT, int U>
__device__ __forceinline__ void pool_tile(const KParams& p, int t, int64_t bag0, int nb, bool staged, const int64_t* s_off, const int32_t* s_idx,
                                          const float* s_w, float* s_out) {
    constexpr bool OUT16 = !std::is_same<OT, float>::value;
    constexpr int NG = kBlock / G;
    constexpr int LD = kLD<BITS>;
    constexpr int VEC = QRow<BITS>::kVec;
    constexpr int CV = VEC * LD;               // columns per lane and column pass: 8 in the product
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
            // pieces of 4 outputs: eight columns per lane lie wholly inside the codes (D % 8 == 0); of sixteen the second eight may not
            auto inside = [&](int k) { return CV == kQmixedLaneColumns || c + k < D; };
            if (staged) {
                int j = static_cast<int>(s - base);
                const int je = static_cast<int>(e - base);
                for (; j + U <= je; j += U) {
                    QLoadN<BITS, LD> q[U];
                    float w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        q[u] = load_row_n<BITS, LD>(W + row_offset<true>(static_cast<int64_t>(s_idx[j + u]), row_bytes), code_off, code_bytes);
                        w[u] = WEIGHTED ? s_w[j + u] : 1.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) accumulate_qn<BITS, WEIGHTED>(acc, q[u], w[u]);
                }
                for (; j < je; ++j)
                    accumulate_qn<BITS, WEIGHTED>(acc, load_row_n<BITS, LD>(W + row_offset<true>(static_cast<int64_t>(s_idx[j]), row_bytes), code_off, code_bytes),
                                                  WEIGHTED ? s_w[j] : 1.0f);
            } else {
                // the tile's lookups exceed the index tile: indices (and weights) come from the request
                int64_t j = s;
                for (; j + U <= e; j += U) {
                    QLoadN<BITS, LD> q[U];
                    float w[U];
                    int64_t r[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        r[u] = load_index(p.indices, j + u, p.idx64);
                        w[u] = WEIGHTED ? as_global<float>(p.psw)[j + u] : 1.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) q[u] = load_row_n<BITS, LD>(W + row_offset<false>(r[u], row_bytes), code_off, code_bytes);
#pragma unroll
                    for (int u = 0; u < U; ++u) accumulate_qn<BITS, WEIGHTED>(acc, q[u], w[u]);
                }
                for (; j < e; ++j)
                    accumulate_qn<BITS, WEIGHTED>(acc, load_row_n<BITS, LD>(W + row_offset<false>(load_index(p.indices, j, p.idx64), row_bytes), code_off, code_bytes),
                                                  WEIGHTED ? as_global<float>(p.psw)[j] : 1.0f);
            }
            if constexpr (OUT16) {
                // the one rounding, in registers; 4 outputs = 8 bytes per piece
                u32x2 piece[CV / 4];
#pragma unroll
                for (int k = 0; k < CV; k += 4)
                    piece[k / 4] = u32x2{OT::round(acc[k]) | (OT::round(acc[k + 1]) << 16), OT::round(acc[k + 2]) | (OT::round(acc[k + 3]) << 16)};
                if (burst) {
                    u32x2* o2 = reinterpret_cast<u32x2*>(s_out16 + static_cast<size_t>(bg) * D + c);
#pragma unroll
                    for (int k = 0; k < CV / 4; ++k)
                        if (inside(4 * k)) o2[k] = piece[k];
                } else {
                    u32x2* o2 = reinterpret_cast<u32x2*>(out16_t + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                    for (int k = 0; k < CV / 4; ++k)
                        if (inside(4 * k)) __builtin_nontemporal_store(piece[k], o2 + k);
                }
            } else if (burst) {
                f32x4* o4 = reinterpret_cast<f32x4*>(s_out + static_cast<size_t>(bg) * D + c);
#pragma unroll
                for (int k = 0; k < CV; k += 4)
                    if (inside(k)) o4[k / 4] = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
            } else {
                f32x4* o4 = reinterpret_cast<f32x4*>(out_t + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                for (int k = 0; k < CV; k += 4) {
                    f32x4 v = {acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
                    if (inside(k)) __builtin_nontemporal_store(v, o4 + k / 4);
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
__global__ void __launch_bounds__(kBlock) qmixed_fwd_kernel(const KParams p, const int32_t* __restrict__ table_bits) {
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

    // the tile's format: one table, one scalar load, one branch
    if (table_bits[t] == 8)
        pool_tile<8, G, WEIGHTED, OT, U>(p, t, bag0, nb, staged, s_off, s_idx, s_w, s_out);
    else
        pool_tile<4, G, WEIGHTED, OT, U>(p, t, bag0, nb, staged, s_off, s_idx, s_w, s_out);
}

// the launcher ladder: group width, weighted, output element, rows in flight
template <int G, typename OT>
hipError_t launch_qm_w(const KParams& p0, const int32_t* table_bits, int unroll, hipStream_t stream) {
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
            hipLaunchKernelGGL((qmixed_fwd_kernel<G, decltype(w)::value, OT, U>), dim3(grid), dim3(kBlock), lds, stream, p, table_bits);
        });
    });
    return hipGetLastError();
}

template <typename OT>
hipError_t launch_qm_g(const KParams& p, const int32_t* table_bits, int max_dim, int unroll, hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, kQmixedLaneColumns), [&](auto g) { return launch_qm_w<decltype(g)::value, OT>(p, table_bits, unroll, stream); });
}

}  // namespace

// p.io = out of out_dtype (PM_F32 | PM_BF16 | PM_F16), addressed in its elements; table_bits: device int32 [T], 8 | 4; unroll: plan_qmixed's (2 | 4)
hipError_t launch_embbag_fwd_qmixed(const KParams& p, const int32_t* table_bits, int out_dtype, int max_dim, int unroll, hipStream_t stream) {
    if (out_dtype == PM_BF16) return launch_qm_g<OutBF16>(p, table_bits, max_dim, unroll, stream);
    if (out_dtype == PM_F16) return launch_qm_g<OutF16>(p, table_bits, max_dim, unroll, stream);
    return launch_qm_g<float>(p, table_bits, max_dim, unroll, stream);
}

}  // namespace pm
