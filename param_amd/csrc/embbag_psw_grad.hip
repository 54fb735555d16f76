// param_amd/csrc/embbag_psw_grad.hip -- gradient of per_sample_weights of the batched EmbeddingBag(sum), CDNA4 / gfx950.
//
//     out[j] = sum_{c < D_t} grad(t, bag(j))[c] * table_t[indices[j], c]        for every lookup j of the requested bag slice
//
// Replaces aten::_embedding_bag_per_sample_weights_backward (autograd of F.embedding_bag(..., per_sample_weights=w)) and the
// indice_weights gradient of fbgemm's TBE backward (split_table_batched_embeddings_ops.py:318-324).
//
// A second gather over the rows the forward read: memory-bound, no MFMA.  The forward's structure (embbag_fwd.hip) with the
// data flow turned round -- the [bags x D] stream is READ (the gradient), and what leaves is 4 bytes per lookup:
//   * one 256-thread workgroup owns a tile of consecutive bags of ONE table; the tile's offsets and its index range are staged
//     in LDS with coalesced loads (indices narrowed to int32).  A tile whose index range exceeds the LDS tile is walked in
//     LDS-tile-sized pieces: every lookup is staged, there is no direct-read path;
//   * a group of g lanes (g x 16 B >= one row, a power of two in 4 .. 64, chosen per table from dims[t]) serves a lookup: lane l
//     loads columns [l V, (l + 1) V) of the row with one global_load_dwordx4 and multiplies them with its slice of the bag's
//     gradient, which it holds in registers (16 B per lane for fp32 tables, 32 B for 16-bit ones); kRows row loads are issued
//     back to back before the first use;
//   * a value does not belong to a bag's sum, so the tile's LOOKUPS -- not its bags -- are dealt out: every lane group walks one
//     contiguous share of the piece and reloads its gradient slice when the walk passes a bag border.  One 9000-lookup bag
//     keeps all lane groups busy, a tile of one-hot bags keeps row loads in flight across bag borders, and ragged tiles
//     need no longest-bag-first order;
//   * arithmetic (the rule of include/param_amd.h): every product and every add rounded to fp32 on its own (no FMA), the lane's V
//     products added in ascending column order from +0, lane partials combined by an xor butterfly with masks 1, 2, 4 .. g / 2;
//     lanes past D / V hold +0.  x + 0 == x: the value does not depend on g, nor on the launch shape.  The butterfly runs in the
//     VALU (DPP adds inside a row, permlane swaps across rows: butterfly_stage below) and the walk is instantiated per group
//     width, so the per-lookup chain has no LDS-crossbar operation and no branch on g;
//   * lane 0 of a group drops the value into an LDS stage; the piece leaves as ONE coalesced non-temporal burst of 4-byte
//     values -- loads and stores share one in-order counter, so no store sits in the row-load loop;
//   * two launch shapes, the forward's rule: requests of one width and >= 12 lookups per bag tile by bag count, T x tiles
//     workgroups in the forward's XCD order; short-bag and mixed-dim requests tile per table by lookups (~256, at most 256 bags)
//     and run as a compact grid over the table-major tile order (tile-count prefix in LDS; more than 1024 tables: T x tiles of
//     the smallest size, surplus workgroups leave).
// No atomics, no workspace, no allocation.
#include <type_traits>

#include "common.h"
#include "fwd_elem.h"

namespace pm {
namespace {

using namespace fwd;

constexpr int kBlockLog2 = 8;
static_assert(kBlock == 1 << kBlockLog2, "lane groups are cut from the workgroup by shifts");
constexpr int kRows = 2;           // row loads in flight per lane group before the first use (the forward's measured optimum)
constexpr int kFlatMinBags = 8;    // smallest per-table tile of the flat shape: sizes the grid where the tile counts are not known

// One stage of the butterfly: v + (the value of the lane's partner half).  After the stages below M every lane of an aligned group
// of M lanes holds the same bits (a + b == b + a), so ANY lane of the other half of the 2 M-group is as good as lane ^ M: the
// stages inside a 16-lane row are DPP modifiers of the add itself (quad permutes for 1 and 2; the half-row and row mirrors reach
// the other quad / the other eight lanes), the stages across rows are gfx950's v_permlane16_swap / v_permlane32_swap, whose two
// results are this lane's own value and its partner's (in either order).  No LDS crossbar (ds_bpermute) on the per-lookup chain:
// five dependent ~100-cycle operations per lookup were as long as the row load itself once the rows come from L2.
template <int M>
__device__ __forceinline__ float butterfly_stage(float v) {
    const int b = __float_as_int(v);
    if constexpr (M == 1) return __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0xB1, 0xF, 0xF, true)));        // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0x4E, 0xF, 0xF, true)));   // quad_perm [2,3,0,1]
    else if constexpr (M == 4) return __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0x141, 0xF, 0xF, true)));  // row_half_mirror
    else if constexpr (M == 8) return __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0x140, 0xF, 0xF, true)));  // row_mirror
    else if constexpr (M == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(b), static_cast<unsigned>(b), false, false);
        return __fadd_rn(__uint_as_float(r[0]), __uint_as_float(r[1]));
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(b), static_cast<unsigned>(b), false, false);
        return __fadd_rn(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
}

// lanes per lookup of a table of D elements: the next power of two >= D / VEC, in [4, 64]
__host__ __device__ inline int psw_group(int D, int vec) {
    int g = 4;
    while (g < 64 && g * vec < D) g <<= 1;
    return g;
}

// bags per tile of table t in the flat shape: ~flat_target lookups by the table's average bag, kFlatMinBags .. flat_bags bags
__device__ __forceinline__ int flat_tile_bags(const KParams& p, int t) {
    const int64_t g0 = static_cast<int64_t>(t) * p.B + p.bag_begin;
    const int64_t lo = bag_start_or_end(p, g0), hi = bag_start_or_end(p, g0 + p.bag_count);
    const int64_t avg = p.bag_count > 0 ? (hi - lo + p.bag_count - 1) / p.bag_count : 1;
    int bags = static_cast<int>(p.flat_target / (avg > 0 ? avg : 1));
    bags = bags > p.flat_bags ? p.flat_bags : bags;
    return bags < kFlatMinBags ? kFlatMinBags : bags;
}

// LDS: int64 s_off[bags_per_block + 2] | int32 s_idx[idx_cap] | float s_val[idx_cap] (| compact: int s_pref[T + 1], uint16 s_bags[T])
// -- common.h's tile layout with the value stage in the weights' place
template <typename WT>
__global__ void __launch_bounds__(kBlock) embbag_psw_grad_kernel(const KParams p, float* __restrict__ out) {
    constexpr int VEC = Elem<WT>::kVec;
    constexpr int ES = 16 / VEC;   // bytes per table element
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int64_t* const s_off = reinterpret_cast<int64_t*>(smem);
    int32_t* const s_idx = reinterpret_cast<int32_t*>(smem + tile_idx_offset(p.bags_per_block));
    float* const s_val = reinterpret_cast<float*>(s_idx + p.idx_cap);
    int* const s_pref = reinterpret_cast<int*>(smem + (tile_lds_bytes(p.bags_per_block, p.idx_cap, true) + 15) / 16 * 16);
    uint16_t* const s_bags = reinterpret_cast<uint16_t*>(s_pref + p.T + 1);
    const float* const grad = p.io;

    auto do_tile = [&](int t, int64_t bag0, int nb) {
        const int D = p.dims[t];
        const int g = psw_group(D, VEC);
        const int64_t gb0 = static_cast<int64_t>(t) * p.B + bag0;
        for (int i = threadIdx.x; i <= nb; i += kBlock) s_off[i] = bag_start_or_end(p, gb0 + i);
        __syncthreads();
        const int64_t base = s_off[0];
        const int64_t end = s_off[nb];

        // the walk of one piece, instantiated per group width: shifts for the lane arithmetic, a straight-line butterfly
        auto walk = [&](auto lg_c, int64_t pbase, int pcnt) {
            constexpr int LG = decltype(lg_c)::value;
            constexpr int G = 1 << LG, NG = kBlock >> LG;
            const int gid = threadIdx.x >> LG;
            const int lig = threadIdx.x & (G - 1);
            const bool live = lig * VEC < D;                          // lanes past D / VEC hold +0: they load column 0 and drop it
            const int c = live ? lig * VEC : 0;
            const int64_t row_bytes = static_cast<int64_t>(D) * ES;
            const char* Wc = reinterpret_cast<const char*>(p.tables[t]) + static_cast<int64_t>(c) * ES;
            const float* grad_t = grad + p.out_offsets[t] + c;
            const bool nt = p.nt_loads != 0;
            const int per = (pcnt + NG - 1) >> (kBlockLog2 - LG);
            const int j_lo = gid * per;
            const int j_hi = j_lo + per < pcnt ? j_lo + per : pcnt;
            if (j_lo >= j_hi) return;
            // the bag that holds the share's first lookup: the last one that starts at or before it (empty bags start where
            // the next one does and are passed over)
            int cur;
            {
                const int64_t pos = pbase + j_lo;
                int lo = 0, hi = nb;                                  // s_off[lo] <= pos < s_off[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_off[mid] <= pos) lo = mid; else hi = mid;
                }
                cur = lo;
            }
            // a bag's end relative to the piece, capped at the piece's end (the walk never reaches that): 32-bit compares
            auto end_of = [&](int bg) { const int64_t d = s_off[bg + 1] - pbase; return d < pcnt ? static_cast<int>(d) : pcnt; };
            int cur_end = end_of(cur);
            float gr[VEC];
            auto load_grad = [&](int bg) {
                const PM_GLOBAL f32x4* q = as_global<f32x4>(grad_t + grad_bag_offset(bag0 + bg, p.out_stride, p.gblk_shift, p.gblk_extra));
#pragma unroll
                for (int k = 0; k < VEC; k += 4) {
                    const f32x4 v = q[k / 4];
                    gr[k] = v.x; gr[k + 1] = v.y; gr[k + 2] = v.z; gr[k + 3] = v.w;
                }
            };
            load_grad(cur);

            for (int j = j_lo; j < j_hi; j += kRows) {
                u32x4 raw[kRows];
                int32_t r[kRows];
#pragma unroll
                for (int u = 0; u < kRows; ++u) r[u] = s_idx[j + u < j_hi ? j + u : j_hi - 1];   // past the share: its last lookup again
#pragma unroll
                for (int u = 0; u < kRows; ++u) raw[u] = load16(Wc + row_offset<true>(r[u], row_bytes), nt);
#pragma unroll
                for (int u = 0; u < kRows; ++u) {
                    if (j + u < j_hi) {
                        if (j + u >= cur_end) {                      // the walk passed the end of bag `cur` (and of any empty bags after it)
                            do { ++cur; cur_end = end_of(cur); } while (j + u >= cur_end);
                            load_grad(cur);
                        }
                        float f[VEC];
                        Elem<WT>::widen(raw[u], f);
                        float acc = 0.0f;
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc = __fadd_rn(acc, __fmul_rn(gr[k], f[k]));
                        acc = live ? acc : 0.0f;
                        // butterfly, masks 1 .. G / 2: a lane's partner lies in its own aligned group of G lanes
                        acc = butterfly_stage<1>(acc);
                        acc = butterfly_stage<2>(acc);
                        if constexpr (G > 4) acc = butterfly_stage<4>(acc);
                        if constexpr (G > 8) acc = butterfly_stage<8>(acc);
                        if constexpr (G > 16) acc = butterfly_stage<16>(acc);
                        if constexpr (G > 32) acc = butterfly_stage<32>(acc);
                        if (lig == 0) s_val[j + u] = acc;
                    }
                }
            }
        };

        for (int64_t pbase = base; pbase < end; pbase += p.idx_cap) {
            const int pcnt = end - pbase < p.idx_cap ? static_cast<int>(end - pbase) : p.idx_cap;
            for (int i = threadIdx.x; i < pcnt; i += kBlock) s_idx[i] = static_cast<int32_t>(load_index(p.indices, pbase + i, p.idx64));
            __syncthreads();
            switch (g) {
                case 4: walk(std::integral_constant<int, 2>{}, pbase, pcnt); break;
                case 8: walk(std::integral_constant<int, 3>{}, pbase, pcnt); break;
                case 16: walk(std::integral_constant<int, 4>{}, pbase, pcnt); break;
                case 32: walk(std::integral_constant<int, 5>{}, pbase, pcnt); break;
                default: walk(std::integral_constant<int, 6>{}, pbase, pcnt); break;
            }
            __syncthreads();
            // the piece's values: one contiguous run of the output, never re-read by this kernel
            for (int i = threadIdx.x; i < pcnt; i += kBlock) __builtin_nontemporal_store(s_val[i], out + pbase + i);
            __syncthreads();                                      // the next piece / tile restages s_idx, s_val and s_off
        }
    };

    // three tile orders, ONE call site of the tile's code:
    //   flat_bags == 0:  tiles of bags_per_block bags, T x tiles_per_table workgroups in the forward's XCD order;
    //   flat, compact:   every table's tile size and count (one thread per table), the prefix of the counts (one wave), then tiles
    //                    blockIdx, + grid, ... of the table-major tile order -- the forward's compact launch;
    //   flat otherwise:  (more than 1024 tables) one workgroup per (table, tile of the smallest size), surplus workgroups leave
    const bool compact = p.flat_compact > 0;
    if (compact) {
        for (int t = threadIdx.x; t < p.T; t += kBlock) {
            const int bags = flat_tile_bags(p, t);
            s_bags[t] = static_cast<uint16_t>(bags);
            s_pref[t + 1] = static_cast<int>((p.bag_count + bags - 1) / bags);
        }
        __syncthreads();
        if (threadIdx.x < kWave) {
            int running = 0;
            for (int b0 = 0; b0 < p.T; b0 += kWave) {
                const int i = b0 + static_cast<int>(threadIdx.x);
                int v = i < p.T ? s_pref[i + 1] : 0;
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) {
                    const int o = __shfl_up(v, d, kWave);
                    if (static_cast<int>(threadIdx.x) >= d) v += o;
                }
                if (i < p.T) s_pref[i + 1] = running + v;
                running += __shfl(v, kWave - 1, kWave);
            }
            if (threadIdx.x == 0) s_pref[0] = 0;
        }
        __syncthreads();
    }
    const int total = compact ? s_pref[p.T] : static_cast<int>(blockIdx.x) + 1;
    const int step = compact ? static_cast<int>(gridDim.x) : 1;
    for (int v = blockIdx.x; v < total; v += step) {
        int t, tile, bags;
        if (compact) {
            int lo = 0, hi = p.T;                                 // the table whose tiles [s_pref[t], s_pref[t + 1]) hold v
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pref[mid] <= v) lo = mid; else hi = mid;
            }
            t = lo;
            tile = v - s_pref[lo];
            bags = s_bags[lo];
        } else {
            block_to_tile(p, t, tile);
            if (t >= p.T) return;
            bags = p.flat_bags > 0 ? flat_tile_bags(p, t) : p.bags_per_block;
        }
        const int64_t bag0 = p.bag_begin + static_cast<int64_t>(tile) * bags;
        const int64_t left = p.bag_begin + p.bag_count - bag0;
        if (left > 0) do_tile(t, bag0, left < bags ? static_cast<int>(left) : bags);      // (uniform: the whole workgroup agrees)
        if (compact) __syncthreads();                             // the next tile restages s_off, which a tile without lookups has just read
    }
}

}  // namespace

// p: make_params' geometry of the request (bag-count tiles, XCD order) with io = the gradient; the flat shape is chosen here
hipError_t launch_embbag_psw_grad(const KParams& p_in, int weight_dtype, int max_dim, int min_dim, float* out, hipStream_t stream) {
    KParams p = p_in;
    const int vec = weight_dtype == PM_F32 ? 4 : 8;
    const int64_t tb = static_cast<int64_t>(p.T) * p.B;
    const int64_t avg_l = tb > 0 ? (p.N + tb - 1) / tb : 0;
    const bool mixed = min_dim > 0 && psw_group(min_dim, vec) < psw_group(max_dim, vec);
    const bool short_bags = tb > 0 && p.N < 12 * tb;
    p.flat_bags = 0;
    p.flat_target = 0;
    p.flat_compact = 0;
    p.stage_out = 0;
    p.stage_bags = 0;
    int64_t grid = static_cast<int64_t>(p.T) * p.tiles_per_table;
    size_t lds;
    if (mixed || short_bags) {
        p.flat_bags = 256;
        p.flat_target = 256;
        p.bags_per_block = p.flat_bags;            // sizes the LDS offsets array
        p.idx_cap = 1024;
        const int64_t tiles_min = (p.bag_count + kFlatMinBags - 1) / kFlatMinBags;
        if (tiles_min * p.T > 0x7fffffffLL) return hipErrorInvalidConfiguration;
        p.tiles_per_table = static_cast<int32_t>(tiles_min);
        if (p.xcd_affine == 3) p.xcd_affine = 0;   // eighths of the tile order assume equal tiles per table
        grid = tiles_min * p.T;
        lds = tile_lds_bytes(p.bags_per_block, p.idx_cap, true);
        if (p.T <= 1024) {
            // about as many workgroups as the request has tiles (the forward's estimate: the true count is on the device); where it
            // falls short workgroups walk on, where it overshoots the surplus leaves after the prologue
            const int64_t n_slice = p.B > 0 ? (p.N * p.bag_count + p.B - 1) / p.B : 0;
            const int64_t by_lookups = (n_slice + p.flat_target - 1) / p.flat_target;
            const int64_t by_bags = static_cast<int64_t>(p.T) * ((p.bag_count + p.flat_bags - 1) / p.flat_bags);
            int64_t est = (by_lookups > by_bags ? by_lookups : by_bags) * 5 / 4 + p.T;
            if (est < 1024) est = 1024;
            if (est > (1 << 20)) est = 1 << 20;
            p.flat_compact = static_cast<int32_t>(est < grid ? est : grid);
            grid = p.flat_compact;
            lds = (lds + 15) / 16 * 16 + static_cast<size_t>(p.T + 1) * 4 + static_cast<size_t>(p.T) * 2;
        }
    } else {
        // index tile: twice what a tile holds on average (8 workgroups per CU keep <= 20 KB of LDS each), 512 .. 4096 entries
        int64_t need = (2 * static_cast<int64_t>(p.bags_per_block) * avg_l + 255) / 256 * 256;
        p.idx_cap = static_cast<int32_t>(need < 512 ? 512 : (need > 4096 ? 4096 : need));
        lds = tile_lds_bytes(p.bags_per_block, p.idx_cap, true);
    }
    if (grid < 1) return hipSuccess;
    const dim3 gd(static_cast<unsigned>(grid)), bd(kBlock);
    switch (weight_dtype) {
        case PM_F32: hipLaunchKernelGGL((embbag_psw_grad_kernel<float>), gd, bd, lds, stream, p, out); break;
        case PM_BF16: hipLaunchKernelGGL((embbag_psw_grad_kernel<bf16_t>), gd, bd, lds, stream, p, out); break;
        default: hipLaunchKernelGGL((embbag_psw_grad_kernel<f16_t>), gd, bd, lds, stream, p, out); break;
    }
    return hipGetLastError();
}

}  // namespace pm
