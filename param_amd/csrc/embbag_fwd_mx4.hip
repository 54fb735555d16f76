// param_amd/csrc/embbag_fwd_mx4.hip -- pm_embbag_fwd_mx4: the pooled lookup over MXFP4 tables (include/param_amd.h, MXFP4 TABLES).
// gfx950 only.
//
// A sibling of the FP8 kernel (embbag_fwd_f8_kernel.inc) with that kernel's tiling, through plan_mx4 (launch_plan.h): one 256-thread
// workgroup owns bags_per_block consecutive bags of one table; bag offsets, and the tile's indices (and weights) when they fit idx_cap,
// are staged in LDS (stage_tile_at, common.h: there is no padding row, so nothing is compacted); a longer tile reads its indices from the
// request; a group of G lanes owns a bag; the tile's pooled rows leave LDS in one burst.  Per column from +0.0 in index order acc = acc +
// v, or fmaf(w, v, acc) when weighted; MEAN: one correctly rounded fp32 division by the bag's length (none for an empty bag: it stays
// +0.0); a 16-bit output is that fp32 value rounded once, in registers.  What is this kernel's own:
//   * THE LANE owns SIXTEEN COLUMNS = ONE 8-BYTE LOAD of codes (global_load_dwordx2 at a naturally aligned address: rows are multiples
//     of 8 bytes) and half a block: a lane pair shares one scale byte.  G = group_lanes(max_dim, 16): 8 lanes and one pass at D = 128 (the
//     72-byte row is nine 8-byte pieces, eight of them codes), 64 lanes at D = 1024, two passes at D = 2048;
//   * the lane's scale byte (global_load_ubyte at row + D / 2 + c / 32) is issued WITH the row's code load, not after the codes arrive:
//     with U rows in flight (template: 2 / 4) a lane has 2 U loads outstanding;
//   * the decode is 8 x v_cvt_scalef32_pk_f32_fp4 on the two dwords (byte select 0 .. 3) with the scale operand built from the byte, NaN
//     selected for x == 255 (mx4_elem.h; -DPM_MX4_SOFT_DECODE: integer expansion and one exact multiplication), onto 16 accumulators.
// A whole block per lane (32 columns, a 16-byte load at an 8-byte-aligned address) would leave half the group idle at D = 128: not built.
// No atomics, no scratch, no inline assembly.
#include <type_traits>

#include "common.h"
#include "fwd_elem.h"
#include "mx4_elem.h"

namespace pm {
namespace {

using namespace fwd;

constexpr int kLaneColumns = kMx4LaneColumns;   // 16

// what a lane has in flight of one row: two dwords of codes and the scale byte of their block
struct Mx4Load {
    u32x2 w;
    uint32_t x;
};
__device__ __forceinline__ Mx4Load load_row(const char* row, int code_off, int scale_off) {
    Mx4Load q;
    q.w = *as_global<u32x2>(row + code_off);
    q.x = *as_global<uint8_t>(row + scale_off);
    return q;
}

// one lookup joins the sum: the lane's 16 columns decoded to fp32, then one add -- or one fmaf when weighted -- per column
template <bool WEIGHTED>
__device__ __forceinline__ void accumulate_mx4(float (&acc)[kLaneColumns], const Mx4Load& q, float w) {
    float f[kLaneColumns];
    mx4::widen_dword(q.w.x, q.x, f);
    mx4::widen_dword(q.w.y, q.x, f + 8);
#pragma unroll
    for (int k = 0; k < kLaneColumns; ++k) acc[k] = WEIGHTED ? fmaf(w, f[k], acc[k]) : acc[k] + f[k];
}

template <int G, int U, bool WEIGHTED, bool MEAN, typename OT>
__global__ void __launch_bounds__(kBlock) mx4_fwd_kernel(const KParams p) {
    constexpr bool OUT16 = !std::is_same<OT, float>::value;
    constexpr int VEC = kLaneColumns;
    constexpr int NG = kBlock / G;
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
    const int64_t base = s_off[0];
    float* s_out = reinterpret_cast<float*>(smem + (tile_lds_bytes(p.bags_per_block, p.idx_cap, WEIGHTED) + 15) / 16 * 16);
    uint16_t* s_out16 = reinterpret_cast<uint16_t*>(s_out);

    const int gid = threadIdx.x / G;
    const int lig = threadIdx.x % G;
    const int D = p.dims[t];
    const int64_t row_bytes = mx4::row_bytes(D);
    const char* W = reinterpret_cast<const char*>(p.tables[t]);
    float* out_t = p.io + p.out_offsets[t];
    // OUT16: io is the 16-bit output; offsets and strides count its 2-byte elements
    uint16_t* out16_t = reinterpret_cast<uint16_t*>(p.io) + p.out_offsets[t];
    const bool burst = p.stage_out > 0;        // the tile's pooled rows leave LDS together (the launcher sized the buffer for the tile)

    for (int bg = gid; bg < nb; bg += NG) {
        const int64_t s = s_off[bg];
        const int64_t e = s_off[bg + 1];
        for (int c = lig * VEC; c < D; c += G * VEC) {   // (D % 32 == 0: a lane's 8 bytes are codes of one block)
            const int code_off = c / 2;
            const int scale_off = D / 2 + c / mx4::kBlockColumns;
            float acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
            if (staged) {
                // the tile's indices in LDS: U rows' loads back to back, then U accumulate steps in index order
                int j = static_cast<int>(s - base);
                const int je = static_cast<int>(e - base);
                for (; j + U <= je; j += U) {
                    Mx4Load q[U];
                    float w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        q[u] = load_row(W + row_offset<true>(static_cast<int64_t>(s_idx[j + u]), row_bytes), code_off, scale_off);
                        w[u] = WEIGHTED ? s_w[j + u] : 1.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) accumulate_mx4<WEIGHTED>(acc, q[u], w[u]);
                }
                for (; j < je; ++j)
                    accumulate_mx4<WEIGHTED>(acc, load_row(W + row_offset<true>(static_cast<int64_t>(s_idx[j]), row_bytes), code_off, scale_off),
                                             WEIGHTED ? s_w[j] : 1.0f);
            } else {
                // the tile's lookups exceed the index tile: indices (and weights) come from the request; the batch's last positions
                // repeat the bag's last lookup and are not added
                for (int64_t j = s; j < e; j += U) {
                    Mx4Load q[U];
                    float w[U];
                    int64_t r[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t jj = j + u < e ? j + u : e - 1;
                        r[u] = load_index(p.indices, jj, p.idx64);
                        w[u] = WEIGHTED ? as_global<float>(p.psw)[jj] : 1.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) q[u] = load_row(W + row_offset<false>(r[u], row_bytes), code_off, scale_off);
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (j + u < e) accumulate_mx4<WEIGHTED>(acc, q[u], w[u]);
                }
            }
            if constexpr (MEAN) {
                if (e > s) {                   // an empty bag stays +0.0: no division
                    const float n = static_cast<float>(e - s);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = acc[k] / n;
                }
            }
            if constexpr (OUT16) {
                // the one rounding, in registers; 4 outputs = 8 bytes per piece
                u32x2 piece[VEC / 4];
#pragma unroll
                for (int k = 0; k < VEC; k += 4)
                    piece[k / 4] = u32x2{OT::round(acc[k]) | (OT::round(acc[k + 1]) << 16), OT::round(acc[k + 2]) | (OT::round(acc[k + 3]) << 16)};
                if (burst) {
                    u32x2* o2 = reinterpret_cast<u32x2*>(s_out16 + static_cast<size_t>(bg) * D + c);
#pragma unroll
                    for (int k = 0; k < VEC / 4; ++k) o2[k] = piece[k];
                } else {
                    u32x2* o2 = reinterpret_cast<u32x2*>(out16_t + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                    for (int k = 0; k < VEC / 4; ++k) __builtin_nontemporal_store(piece[k], o2 + k);
                }
            } else if (burst) {
                f32x4* o4 = reinterpret_cast<f32x4*>(s_out + static_cast<size_t>(bg) * D + c);
#pragma unroll
                for (int k = 0; k < VEC; k += 4) o4[k / 4] = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
            } else {
                f32x4* o4 = reinterpret_cast<f32x4*>(out_t + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                for (int k = 0; k < VEC; k += 4) {
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

// the launcher ladder: MEAN is unweighted (the entry point has refused weights) ...
template <int G, int U, bool MEAN, typename OT>
hipError_t launch_mx4_w(const KParams& p0, hipStream_t stream) {
    KParams p = p0;
    if (MEAN) p.psw = nullptr;
    const bool weighted = p.psw != nullptr;
    const int grid = p.T * p.tiles_per_table;
    const size_t tile_lds = (tile_lds_bytes(p.bags_per_block, p.idx_cap, weighted) + 15) / 16 * 16;
    size_t lds = tile_lds + (p.stage_out > 0 ? static_cast<size_t>(p.bags_per_block) * p.stage_out * (std::is_same<OT, float>::value ? 4 : 2) : 0);
    if (lds > 65536) {                         // (explicit 1024-bag tiles of a weighted request: rows leave one by one)
        p.stage_out = 0;
        lds = tile_lds;
    }
    auto launch = [&](auto w) {
        hipLaunchKernelGGL((mx4_fwd_kernel<G, U, decltype(w)::value, MEAN, OT>), dim3(grid), dim3(kBlock), lds, stream, p);
    };
    if constexpr (MEAN) launch(std::false_type{});
    else dispatch_bool(weighted, launch);
    return hipGetLastError();
}

// ... rows in flight (plan_mx4: 2 / 4), the lane group, the output type
template <bool MEAN, typename OT>
hipError_t launch_mx4_g(const KParams& p, int max_dim, int unroll, hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, kLaneColumns), [&](auto g) {
        constexpr int G = decltype(g)::value;
        return unroll >= 4 ? launch_mx4_w<G, 4, MEAN, OT>(p, stream) : launch_mx4_w<G, 2, MEAN, OT>(p, stream);
    });
}

}  // namespace

// 4 group widths x 2 depths x {plain, weighted, mean} x {fp32, bf16, fp16} output
hipError_t launch_embbag_fwd_mx4(const KParams& p, int max_dim, int unroll, bool mean, int out_dtype, hipStream_t stream) {
    auto go = [&](auto m) {
        constexpr bool M = decltype(m)::value;
        if (out_dtype == PM_BF16) return launch_mx4_g<M, OutBF16>(p, max_dim, unroll, stream);
        if (out_dtype == PM_F16) return launch_mx4_g<M, OutF16>(p, max_dim, unroll, stream);
        return launch_mx4_g<M, float>(p, max_dim, unroll, stream);
    };
    return dispatch_bool(mean, go);
}

}  // namespace pm
