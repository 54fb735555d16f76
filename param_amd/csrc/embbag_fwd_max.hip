// param_amd/csrc/embbag_fwd_max.hip -- batched EmbeddingBag(MAX) forward (pm_embbag_fwd_max, include/param_amd.h: MAX POOLING;
// DESIGN.md section 3.16): per column the maximum over a bag's lookups that are not its table's padding index, and -- for training --
// the row index that supplied it.
//
// A sibling of the padded forward's kernel (embbag_fwd_pad_kernel.inc), with a compare-and-select where that one adds.  The same
// tiling: one 256-thread workgroup owns `bags_per_block` consecutive bags of one table, a group of G lanes owns a bag, a lane keeps a
// 16-byte column slice.  The same STAGED path: a tile whose index range fits the LDS index tile has its indices compacted while they
// are staged, 256 entries a round (ballot + mbcnt + the waves' counts in LDS), the bags' bounds are rewritten to compacted positions and
// the walk reads a dense list -- the first entry of a bag's list is its first KEPT lookup.  The same UNSTAGED path for a bag longer
// than the index tile: indices from the request, two at a time, a padded one predicated off.  kPadUnroll row loads in flight, the LDS
// output burst, OT = float / OutBF16 / OutF16 (one rounding of the fp32 result in registers) as there.  The geometry is the padded
// forward's plan (launch_plan.h: plan_padded).  The staging lines are that kernel's, copied: its instances keep their code.
//
// The rule per column (fwd_elem.h: max_step): the first kept lookup sets cur = w[r_0, c] whatever it holds; a later one replaces it iff
// w[r_j, c] > cur -- ordered and strict, so a NaN in the first kept lookup stays, a NaN later never enters, and of equal values the
// first wins (-0.0 then +0.0 stays -0.0).  Nothing is seeded with 0.0: a bag of negative rows gives a negative maximum.  A bag
// without kept lookups gives +0.0.  16-bit rows are widened exactly and compared in fp32 (the widening is monotone).
//
// WITH_ARG: the lane keeps the winning row index per owned column and writes it as int32 next to the value, at the value's element
// offset in `max_indices` (-1 for a bag without kept lookups).  The staged path reads the index from s_idx.  The int32 pieces leave
// with direct 16-byte non-temporal stores -- they do not pass the burst buffer, whose LDS the value rows fill.  WITH_ARG = false
// (inference) writes nothing extra.  3 table dtypes x 4 group widths x 3 output types x 2 = 72 instantiations.
#include <type_traits>

#include "common.h"
#include "fwd_elem.h"

namespace pm {
namespace {

#include "embbag_fwd_pad_kernel.inc"      // kPadUnroll, kPadWaves and the LDS layout of a padded tile (no instance of its kernel is made here)

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <typename WT, int G, typename OT, bool WITH_ARG>
__global__ void __launch_bounds__(kBlock) max_fwd_kernel(const KParams p, const int64_t* __restrict__ pad_idx, int32_t* __restrict__ arg_out) {
    constexpr bool OUT16 = !std::is_same<OT, float>::value;
    constexpr int VEC = Elem<WT>::kVec;
    constexpr int NG = kBlock / G;
    constexpr int ES = 16 / VEC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_wave_cnt[kPadWaves];

    int t, tile;
    block_to_tile(p, t, tile);
    if (t >= p.T) return;
    const int64_t bag0 = p.bag_begin + static_cast<int64_t>(tile) * p.bags_per_block;
    const int64_t left_bags = p.bag_begin + p.bag_count - bag0;
    if (left_bags <= 0) return;
    const int nb = left_bags < p.bags_per_block ? static_cast<int>(left_bags) : p.bags_per_block;
    const int64_t pad = pad_idx ? pad_idx[t] : -1;      // -1: the table has no padding row (no index equals it)

    int64_t* s_off = reinterpret_cast<int64_t*>(smem);
    int32_t* s_idx = reinterpret_cast<int32_t*>(smem + tile_idx_offset(p.bags_per_block));
    uint16_t* s_pre = reinterpret_cast<uint16_t*>(smem + pad_pre_offset(p.bags_per_block, p.idx_cap, false));
    float* s_out = reinterpret_cast<float*>(smem + pad_out_offset(p.bags_per_block, p.idx_cap, false));

    const int64_t g0 = static_cast<int64_t>(t) * p.B + bag0;
    for (int i = threadIdx.x; i <= nb; i += kBlock) s_off[i] = bag_start_or_end(p, g0 + i);
    __syncthreads();
    const int64_t base = s_off[0];
    const int64_t cnt64 = s_off[nb] - base;
    const bool staged = cnt64 >= 0 && cnt64 <= p.idx_cap;
    if (staged) {
        // compact the tile's indices into LDS, 256 entries a round (the padded forward's staging)
        const int cnt = static_cast<int>(cnt64);
        const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
        int running = 0;                       // kept entries of the rounds before this one (uniform)
        for (int i0 = 0; i0 < cnt; i0 += kBlock) {
            const int i = i0 + static_cast<int>(threadIdx.x);
            int64_t r = pad;
            if (i < cnt) r = load_index(p.indices, base + i, p.idx64);
            const bool keep = i < cnt && r != pad;
            const uint64_t bal = __ballot(keep);
            const int below = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u)));
            if (lane == 0) s_wave_cnt[wave] = __popcll(bal);
            __syncthreads();
            int before = running, total = running;
#pragma unroll
            for (int w2 = 0; w2 < kPadWaves; ++w2) {
                const int c = s_wave_cnt[w2];
                if (w2 < wave) before += c;
                total += c;
            }
            const int pos = before + below;    // pos <= i < idx_cap
            if (i < cnt) s_pre[i] = static_cast<uint16_t>(pos);
            if (keep) s_idx[pos] = static_cast<int32_t>(r);
            running = total;
            __syncthreads();                   // the next round rewrites s_wave_cnt
        }
        // the bags' bounds as compacted positions (relative to the tile): kept entries in front of the bag's first entry
        int64_t nv[(1024 + kBlock) / kBlock];   // (bags_per_block <= 1024: at most 5 bounds per thread)
#pragma unroll
        for (int k = 0; k < (1024 + kBlock) / kBlock; ++k) {
            const int b = static_cast<int>(threadIdx.x) + k * kBlock;
            nv[k] = 0;
            if (b <= nb) {
                const int64_t rel = s_off[b] - base;
                nv[k] = rel >= cnt ? running : (rel < 0 ? 0 : static_cast<int64_t>(s_pre[rel]));
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < (1024 + kBlock) / kBlock; ++k) {
            const int b = static_cast<int>(threadIdx.x) + k * kBlock;
            if (b <= nb) s_off[b] = nv[k];
        }
        __syncthreads();
    }

    const int gid = threadIdx.x / G;
    const int lig = threadIdx.x % G;
    const int D = p.dims[t];
    const int64_t row_bytes = static_cast<int64_t>(D) * ES;
    const char* W = reinterpret_cast<const char*>(p.tables[t]);
    float* out_t = p.io + p.out_offsets[t];
    // OUT16: io is the 16-bit output; offsets and strides count its 2-byte elements
    uint16_t* out16_t = reinterpret_cast<uint16_t*>(p.io) + p.out_offsets[t];
    uint16_t* s_out16 = reinterpret_cast<uint16_t*>(s_out);
    const bool burst = p.stage_out > 0;        // the tile's pooled rows leave LDS together (the launcher sized the buffer for the tile)

    for (int bg = gid; bg < nb; bg += NG) {
        const int64_t s = s_off[bg];
        const int64_t e = s_off[bg + 1];
        for (int c = lig * VEC; c < D; c += G * VEC) {
            const char* Wc = W + static_cast<int64_t>(c) * ES;
            float cur[VEC];
            int32_t arg[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                cur[k] = 0.0f;                 // what a bag without kept lookups gives; the first kept lookup overwrites it
                arg[k] = -1;
            }
            if (staged) {
                // dense list in LDS: entry s is the bag's first kept lookup
                int j = static_cast<int>(s);
                const int je = static_cast<int>(e);
                for (; j + kPadUnroll <= je; j += kPadUnroll) {
                    u32x4 raw[kPadUnroll];
                    int32_t r[kPadUnroll];
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        r[u] = s_idx[j + u];
                        raw[u] = load16(Wc + row_offset<true>(static_cast<int64_t>(r[u]), row_bytes), false);
                    }
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) max_step<WT, WITH_ARG>(cur, arg, raw[u], r[u], j + u == static_cast<int>(s));
                }
                for (; j < je; ++j) {
                    const int32_t r = s_idx[j];
                    max_step<WT, WITH_ARG>(cur, arg, load16(Wc + row_offset<true>(static_cast<int64_t>(r), row_bytes), false), r, j == static_cast<int>(s));
                }
            } else {
                // indices from the request; a padded lookup's row load is predicated off
                bool have = false;             // a kept lookup has set cur
                for (int64_t j = s; j < e; j += kPadUnroll) {
                    u32x4 raw[kPadUnroll];
                    bool keep[kPadUnroll];
                    int64_t r[kPadUnroll];
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        const int64_t jj = j + u < e ? j + u : e - 1;
                        r[u] = load_index(p.indices, jj, p.idx64);
                        keep[u] = j + u < e && r[u] != pad;
                    }
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        raw[u] = u32x4{0u, 0u, 0u, 0u};
                        if (keep[u]) raw[u] = load16(Wc + row_offset<false>(r[u], row_bytes), false);
                    }
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        if (keep[u]) {
                            max_step<WT, WITH_ARG>(cur, arg, raw[u], static_cast<int32_t>(r[u]), !have);
                            have = true;
                        }
                    }
                }
            }
            if constexpr (WITH_ARG) {
                // the winning rows, at the value's element offset: 4 int32 = 16 bytes per store, past the burst buffer
                i32x4* a4 = reinterpret_cast<i32x4*>(arg_out + p.out_offsets[t] + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                for (int k = 0; k < VEC; k += 4) {
                    i32x4 v = {arg[k], arg[k + 1], arg[k + 2], arg[k + 3]};
                    __builtin_nontemporal_store(v, a4 + k / 4);
                }
            }
            if constexpr (OUT16) {
                // the one rounding, in registers; 4 outputs = 8 bytes per piece
                u32x2 piece[VEC / 4];
#pragma unroll
                for (int k = 0; k < VEC; k += 4)
                    piece[k / 4] = u32x2{OT::round(cur[k]) | (OT::round(cur[k + 1]) << 16), OT::round(cur[k + 2]) | (OT::round(cur[k + 3]) << 16)};
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
                for (int k = 0; k < VEC; k += 4) o4[k / 4] = f32x4{cur[k], cur[k + 1], cur[k + 2], cur[k + 3]};
            } else {
                f32x4* o4 = reinterpret_cast<f32x4*>(out_t + (bag0 + bg) * p.out_stride + c);
#pragma unroll
                for (int k = 0; k < VEC; k += 4) {
                    f32x4 v = {cur[k], cur[k + 1], cur[k + 2], cur[k + 3]};
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

// the launcher ladder: output type -> group width -> with / without arg-max
template <typename WT, int G, typename OT>
hipError_t launch_max_a(const KParams& p0, const int64_t* pad_idx, int32_t* max_indices, hipStream_t stream) {
    KParams p = p0;
    p.psw = nullptr;
    const int grid = p.T * p.tiles_per_table;
    const size_t tile_lds = pad_out_offset(p.bags_per_block, p.idx_cap, false);
    size_t lds = tile_lds + (p.stage_out > 0 ? static_cast<size_t>(p.bags_per_block) * p.stage_out * (std::is_same<OT, float>::value ? 4 : 2) : 0);
    if (lds > 65536) {                         // (explicit 1024-bag tiles: rows leave one by one)
        p.stage_out = 0;
        lds = tile_lds;
    }
    dispatch_bool(max_indices != nullptr, [&](auto a) {
        hipLaunchKernelGGL((max_fwd_kernel<WT, G, OT, decltype(a)::value>), dim3(grid), dim3(kBlock), lds, stream, p, pad_idx, max_indices);
    });
    return hipGetLastError();
}

template <typename WT, typename OT>
hipError_t launch_max_g(const KParams& p, int max_dim, const int64_t* pad_idx, int32_t* max_indices, hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, Elem<WT>::kVec),
                                [&](auto g) { return launch_max_a<WT, decltype(g)::value, OT>(p, pad_idx, max_indices, stream); });
}

template <typename WT>
hipError_t launch_max_o(const KParams& p, int max_dim, const int64_t* pad_idx, int out_dtype, int32_t* max_indices, hipStream_t stream) {
    switch (out_dtype) {
        case PM_F32: return launch_max_g<WT, float>(p, max_dim, pad_idx, max_indices, stream);
        case PM_BF16: return launch_max_g<WT, OutBF16>(p, max_dim, pad_idx, max_indices, stream);
        default: return launch_max_g<WT, OutF16>(p, max_dim, pad_idx, max_indices, stream);
    }
}

}  // namespace

// p: the padded forward's plan for the output element (plan_padded; bags_per_block <= 1024, idx_cap <= 4096); p.io = out of out_dtype;
// pad_idx NULL = no table has a padding row; max_indices NULL = not written
hipError_t launch_embbag_fwd_max(const KParams& p, int weight_dtype, int max_dim, const int64_t* pad_idx, int out_dtype, int32_t* max_indices,
                                 hipStream_t stream) {
    switch (weight_dtype) {
        case PM_F32: return launch_max_o<float>(p, max_dim, pad_idx, out_dtype, max_indices, stream);
        case PM_BF16: return launch_max_o<bf16_t>(p, max_dim, pad_idx, out_dtype, max_indices, stream);
        default: return launch_max_o<f16_t>(p, max_dim, pad_idx, out_dtype, max_indices, stream);
    }
}

}  // namespace pm
