// param_amd/csrc/embbag_fwd_f8s_kernel.inc -- pm_embbag_fwd_f8_scaled: the pooled lookup over SCALED FP8 tables (include/param_amd.h,
// SCALED FP8 TABLES), included inside `namespace pm { namespace { ... } }` (after common.h, fwd_elem.h and f8s_elem.h) by
// embbag_fwd_f8s_{e4m3,e5m2}_{table,row}.hip: one translation unit per format and per kind of exponent.  gfx950 only.
//
// A sibling of pm_embbag_fwd_f8's kernel (embbag_fwd_f8_kernel.inc, which says what the tiling is): the same tiles, compaction, burst,
// lane groups and rows in flight, with v = dec(code) * 2^(E_t + e_r) in the place of dec(code) in the accumulate step.  v is formed by
// the hardware widening followed by ONE fp32 multiplication by 2^s built from its bits (f8s_elem.h: pow2) -- exact for every non-NaN
// code at every s in [-64, 64], and independent of how v_cvt_scalef32_pk_f32_fp8 / _bf8 treats its scale operand, which nothing here
// relies on.  What differs from the sibling:
//   * E_t (table_exp[t], 0 when the array is absent) is read once per workgroup; with ROW = false its 2^E_t is the one scale of the tile;
//   * ROW = true: a row's exponent byte is loaded WHERE THE TILE'S INDICES ARE STAGED -- the thread that stages index i loads
//     row_exp[t][index] right behind it and the byte is compacted into LDS next to s_idx (s_exp, one byte per index-tile entry, behind
//     s_pre) -- so no lane group waits for a dependent byte load per row; a tile beyond the index tile loads the byte next to the
//     index it reads from the request, predicated like the row load.
// E_t + e_r is clamped to [-64, 64] before 2^s is built (a caller's contract; the clamp keeps a broken one from building a NaN pattern).
// That kernel takes no such arguments, and adding them would rename every kernel of its family; hence a file of its own.
// No atomics, no inline assembly.

using namespace fwd;

constexpr int kF8sWaves = kBlock / kWave;

// LDS: int64 s_off[bags_per_block + 1 (+ 1)] | int32 s_idx[idx_cap] | float s_w[idx_cap] (weighted) | uint16 s_pre[idx_cap] |
// int8 s_exp[idx_cap] (row exponents) | burst -- f8s_pre_offset / f8s_out_offset (common.h), which the plan call shares

// one lookup joins the sum: accumulate (fwd_elem.h) with v = dec(code) * scale
template <typename WT, bool WEIGHTED>
__device__ __forceinline__ void accumulate_scaled(float (&acc)[Elem<WT>::kVec], const u32x4& raw, float w, float scale) {
    constexpr int VEC = Elem<WT>::kVec;
    float f[VEC];
    Elem<WT>::widen(raw, f);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float v = f[k] * scale;
        acc[k] = WEIGHTED ? fmaf(w, v, acc[k]) : acc[k] + v;
    }
}

template <typename WT, int G, int U, bool WEIGHTED, bool MEAN, bool ROW, typename OT>
__global__ void __launch_bounds__(kBlock) f8s_fwd_kernel(const KParams p, const int64_t* __restrict__ pad_idx, const int32_t* __restrict__ table_exp,
                                                         const int8_t* const* __restrict__ row_exp) {
    constexpr bool OUT16 = !std::is_same<OT, float>::value;
    constexpr int VEC = Elem<WT>::kVec;        // 16 columns = 16 bytes per lane and load
    constexpr int NG = kBlock / G;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_wave_cnt[kF8sWaves];

    int t, tile;
    block_to_tile(p, t, tile);
    if (t >= p.T) return;
    const int64_t bag0 = p.bag_begin + static_cast<int64_t>(tile) * p.bags_per_block;
    const int64_t left_bags = p.bag_begin + p.bag_count - bag0;
    if (left_bags <= 0) return;
    const int nb = left_bags < p.bags_per_block ? static_cast<int>(left_bags) : p.bags_per_block;
    const int64_t pad = pad_idx ? pad_idx[t] : -1;   // -1: the table has no padding row (no index equals it)
    const int tab_e = table_exp ? table_exp[t] : 0;
    const PM_GLOBAL int8_t* rexp = ROW ? as_global<int8_t>(row_exp[t]) : nullptr;
    const float tab_scale = f8s::pow2(f8s::clamp_exp(tab_e));
    auto row_scale = [&](int e) { return f8s::pow2(f8s::clamp_exp(tab_e + e)); };

    int64_t* s_off = reinterpret_cast<int64_t*>(smem);
    int32_t* s_idx = reinterpret_cast<int32_t*>(smem + tile_idx_offset(p.bags_per_block));
    float* s_w = reinterpret_cast<float*>(s_idx + p.idx_cap);
    uint16_t* s_pre = reinterpret_cast<uint16_t*>(smem + f8s_pre_offset(p.bags_per_block, p.idx_cap, WEIGHTED));
    int8_t* s_exp = reinterpret_cast<int8_t*>(s_pre + p.idx_cap);
    float* s_out = reinterpret_cast<float*>(smem + f8s_out_offset(p.bags_per_block, p.idx_cap, WEIGHTED, ROW));

    const int64_t g0 = static_cast<int64_t>(t) * p.B + bag0;
    for (int i = threadIdx.x; i <= nb; i += kBlock) s_off[i] = bag_start_or_end(p, g0 + i);
    __syncthreads();
    const int64_t base = s_off[0];
    const int64_t cnt64 = s_off[nb] - base;
    const bool staged = cnt64 >= 0 && cnt64 <= p.idx_cap;
    if (staged) {
        // compact the tile's indices (and weights) into LDS, 256 entries a round
        const int cnt = static_cast<int>(cnt64);
        const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
        int running = 0;                       // kept entries of the rounds before this one (uniform)
        for (int i0 = 0; i0 < cnt; i0 += kBlock) {
            const int i = i0 + static_cast<int>(threadIdx.x);
            int64_t r = pad;
            float w = 0.0f;
            if (i < cnt) {
                r = load_index(p.indices, base + i, p.idx64);
                if (WEIGHTED) w = as_global<float>(p.psw)[base + i];
            }
            const bool keep = i < cnt && r != pad;
            int ex = 0;
            if (ROW && keep) ex = rexp[r];     // the row's exponent, behind its index: in flight across the compaction
            const uint64_t bal = __ballot(keep);
            const int below = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u)));
            if (lane == 0) s_wave_cnt[wave] = __popcll(bal);
            __syncthreads();
            int before = running, total = running;
#pragma unroll
            for (int w2 = 0; w2 < kF8sWaves; ++w2) {
                const int c = s_wave_cnt[w2];
                if (w2 < wave) before += c;
                total += c;
            }
            const int pos = before + below;    // pos <= i < idx_cap
            if (i < cnt) s_pre[i] = static_cast<uint16_t>(pos);
            if (keep) {
                s_idx[pos] = static_cast<int32_t>(r);
                if (WEIGHTED) s_w[pos] = w;
                if (ROW) s_exp[pos] = static_cast<int8_t>(ex);
            }
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
    const int64_t row_bytes = D;               // one byte per column
    const char* W = reinterpret_cast<const char*>(p.tables[t]);
    float* out_t = p.io + p.out_offsets[t];
    // OUT16: io is the 16-bit output; offsets and strides count its 2-byte elements
    uint16_t* out16_t = reinterpret_cast<uint16_t*>(p.io) + p.out_offsets[t];
    uint16_t* s_out16 = reinterpret_cast<uint16_t*>(s_out);
    const bool burst = p.stage_out > 0;        // the tile's pooled rows leave LDS together (the launcher sized the buffer for the tile)

    for (int bg = gid; bg < nb; bg += NG) {
        const int64_t s = s_off[bg];
        const int64_t e = s_off[bg + 1];
        for (int c = lig * VEC; c < D; c += G * VEC) {   // (D % 16 == 0: a lane's 16 bytes end inside the row)
            const char* Wc = W + c;
            float acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
            int64_t kept = 0;                  // MEAN: the bag's kept lookups (staged: e - s, set below)
            auto add = [&](const u32x4& raw, float w, float sc) { accumulate_scaled<WT, WEIGHTED>(acc, raw, w, sc); };
            if (staged) {
                // dense list in LDS: U row loads back to back, then U accumulate steps in index order
                int j = static_cast<int>(s);
                const int je = static_cast<int>(e);
                for (; j + U <= je; j += U) {
                    u32x4 raw[U];
                    float w[U], sc[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        raw[u] = load16(Wc + row_offset<true>(static_cast<int64_t>(s_idx[j + u]), row_bytes), false);
                        w[u] = WEIGHTED ? s_w[j + u] : 1.0f;
                        sc[u] = ROW ? row_scale(s_exp[j + u]) : tab_scale;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) add(raw[u], w[u], sc[u]);
                }
                for (; j < je; ++j)
                    add(load16(Wc + row_offset<true>(static_cast<int64_t>(s_idx[j]), row_bytes), false), WEIGHTED ? s_w[j] : 1.0f,
                        ROW ? row_scale(s_exp[j]) : tab_scale);
            } else {
                // indices from the request; a padded lookup's row load is predicated off
                for (int64_t j = s; j < e; j += U) {
                    u32x4 raw[U];
                    float w[U];
                    bool keep[U];
                    int64_t r[U];
                    int ex[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t jj = j + u < e ? j + u : e - 1;
                        r[u] = load_index(p.indices, jj, p.idx64);
                        w[u] = WEIGHTED ? as_global<float>(p.psw)[jj] : 1.0f;
                        keep[u] = j + u < e && r[u] != pad;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        raw[u] = u32x4{0u, 0u, 0u, 0u};
                        ex[u] = 0;
                        if (keep[u]) raw[u] = load16(Wc + row_offset<false>(r[u], row_bytes), false);
                        if (ROW && keep[u]) ex[u] = rexp[r[u]];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (keep[u]) add(raw[u], w[u], ROW ? row_scale(ex[u]) : tab_scale);
                        if constexpr (MEAN) kept += keep[u] ? 1 : 0;
                    }
                }
            }
            if constexpr (MEAN) {
                if (staged) kept = e - s;
                if (kept > 0) {                // an empty or all-padding bag stays +0.0: no division
                    const float n = static_cast<float>(kept);
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
template <typename WT, int G, int U, bool MEAN, bool ROW, typename OT>
hipError_t launch_f8s_w(const KParams& p0, const F8sArgs& a, hipStream_t stream) {
    KParams p = p0;
    if (MEAN) p.psw = nullptr;
    const bool weighted = p.psw != nullptr;
    const int grid = p.T * p.tiles_per_table;
    // (the burst leaves where the tile's LDS would pass 64 KiB -- explicit tiles of 512 bags and more of a weighted request --: rows
    // then leave one by one; pm_embbag_f8_scaled_plan reports the same stage_out)
    p.stage_out = f8s_stage_out(p.bags_per_block, p.idx_cap, weighted, ROW, p.stage_out, std::is_same<OT, float>::value ? 4 : 2);
    const size_t lds = f8s_lds_bytes(p.bags_per_block, p.idx_cap, weighted, ROW, p.stage_out, std::is_same<OT, float>::value ? 4 : 2);
    auto launch = [&](auto w) {
        hipLaunchKernelGGL((f8s_fwd_kernel<WT, G, U, decltype(w)::value, MEAN, ROW, OT>), dim3(grid), dim3(kBlock), lds, stream, p, a.pad_idx,
                           a.table_exp, a.row_exp);
    };
    if constexpr (MEAN) launch(std::false_type{});
    else dispatch_bool(weighted, launch);
    return hipGetLastError();
}

// ... rows in flight (plan_f8: 2 / 4 / 8), then the lane group
template <typename WT, int G, bool MEAN, bool ROW, typename OT>
hipError_t launch_f8s_u(const KParams& p, int unroll, const F8sArgs& a, hipStream_t stream) {
    if (unroll >= 8) return launch_f8s_w<WT, G, 8, MEAN, ROW, OT>(p, a, stream);
    if (unroll >= 4) return launch_f8s_w<WT, G, 4, MEAN, ROW, OT>(p, a, stream);
    return launch_f8s_w<WT, G, 2, MEAN, ROW, OT>(p, a, stream);
}

template <typename WT, bool MEAN, bool ROW, typename OT>
hipError_t launch_f8s_g(const KParams& p, int max_dim, int unroll, const F8sArgs& a, hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, Elem<WT>::kVec),
                                [&](auto g) { return launch_f8s_u<WT, decltype(g)::value, MEAN, ROW, OT>(p, unroll, a, stream); });
}

// one format's variants of one kind (ROW: row exponents present): 4 group widths x 3 depths x {plain, weighted, mean} x {fp32, bf16, fp16} output
template <typename WT, bool ROW>
hipError_t launch_f8s_format(const KParams& p, int max_dim, int unroll, const F8sArgs& a, bool mean, int out_dtype, hipStream_t stream) {
    auto go = [&](auto m) {
        constexpr bool M = decltype(m)::value;
        if (out_dtype == PM_BF16) return launch_f8s_g<WT, M, ROW, OutBF16>(p, max_dim, unroll, a, stream);
        if (out_dtype == PM_F16) return launch_f8s_g<WT, M, ROW, OutF16>(p, max_dim, unroll, a, stream);
        return launch_f8s_g<WT, M, ROW, float>(p, max_dim, unroll, a, stream);
    };
    return dispatch_bool(mean, go);
}
