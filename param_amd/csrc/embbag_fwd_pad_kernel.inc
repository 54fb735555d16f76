// param_amd/csrc/embbag_fwd_pad_kernel.inc -- the padded forward's kernel and its launcher ladder, included inside
// `namespace pm { namespace { ... } }` (after common.h and fwd_elem.h) by embbag_fwd_pad.hip -- fp32 output: pm_embbag_fwd_padded,
// pm_embbag_fwd_mean -- and by the embbag_fwd_out16_*.hip translation units -- bf16 / fp16 output: pm_embbag_fwd_out16.  What the
// kernel does is described at the top of embbag_fwd_pad.hip; the output element type OT is described below.
//
// OUTPUT DTYPE (include/param_amd.h, DESIGN.md section 3.9): OT = float is the kernel as it always was -- every line that differs sits
// under `if constexpr (OUT16)`.  OT = OutBF16 / OutF16: the pooled fp32 value -- the same additions, the same single division of MEAN --
// is rounded ONCE, to nearest even, in registers, and leaves as 2 bytes: 4 outputs (8 bytes) per store, which is what the request's
// alignment rules guarantee for every table dtype (dims, out_offsets and out_stride are multiples of 4 elements); a lane of a 16-bit
// table holds 8 outputs and stores two such pieces.  The LDS burst buffer then holds 2 bytes per element.  No 16-bit partial sums.
// These variants take a NULL pad array (no table has a padding row) whether MEAN or not.

using namespace fwd;

// (OutBF16 / OutF16 -- the one rounding -- and u32x2, the 8-byte piece of 4 outputs, live in fwd_elem.h: the row gather shares them)

constexpr int kPadUnroll = 2;              // row loads in flight per lane group
constexpr int kPadWaves = kBlock / kWave;

// LDS: int64 s_off[bags_per_block + 1 (+ 1)] | int32 s_idx[idx_cap] | float s_w[idx_cap] (weighted) | uint16 s_pre[idx_cap] | burst
__host__ __device__ inline size_t pad_pre_offset(int bags_per_block, int idx_cap, bool weighted) {
    return tile_lds_bytes(bags_per_block, idx_cap, weighted);
}
__host__ __device__ inline size_t pad_out_offset(int bags_per_block, int idx_cap, bool weighted) {
    return (pad_pre_offset(bags_per_block, idx_cap, weighted) + static_cast<size_t>(idx_cap) * 2 + 15) / 16 * 16;
}

template <typename WT, int G, bool WEIGHTED, bool MEAN = false, typename OT = float>
__global__ void __launch_bounds__(kBlock) pad_fwd_kernel(const KParams p, const int64_t* __restrict__ pad_idx) {
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
    int64_t pad;                               // -1: the table has no padding row (no index equals it)
    if constexpr (MEAN || OUT16) pad = pad_idx ? pad_idx[t] : -1;
    else pad = pad_idx[t];

    int64_t* s_off = reinterpret_cast<int64_t*>(smem);
    int32_t* s_idx = reinterpret_cast<int32_t*>(smem + tile_idx_offset(p.bags_per_block));
    float* s_w = reinterpret_cast<float*>(s_idx + p.idx_cap);
    uint16_t* s_pre = reinterpret_cast<uint16_t*>(smem + pad_pre_offset(p.bags_per_block, p.idx_cap, WEIGHTED));
    float* s_out = reinterpret_cast<float*>(smem + pad_out_offset(p.bags_per_block, p.idx_cap, WEIGHTED));

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
            if (keep) {
                s_idx[pos] = static_cast<int32_t>(r);
                if (WEIGHTED) s_w[pos] = w;
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
            float acc[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
            int64_t kept = 0;                  // MEAN: the bag's kept lookups (staged: e - s, set below)
            auto add = [&](const u32x4& raw, float w) { accumulate<WT, WEIGHTED>(acc, raw, w); };
            if (staged) {
                // dense list in LDS: the product forward's loop
                int j = static_cast<int>(s);
                const int je = static_cast<int>(e);
                for (; j + kPadUnroll <= je; j += kPadUnroll) {
                    u32x4 raw[kPadUnroll];
                    float w[kPadUnroll];
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        raw[u] = load16(Wc + row_offset<true>(static_cast<int64_t>(s_idx[j + u]), row_bytes), false);
                        w[u] = WEIGHTED ? s_w[j + u] : 1.0f;
                    }
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) add(raw[u], w[u]);
                }
                for (; j < je; ++j) add(load16(Wc + row_offset<true>(static_cast<int64_t>(s_idx[j]), row_bytes), false), WEIGHTED ? s_w[j] : 1.0f);
            } else {
                // indices from the request; a padded lookup's row load is predicated off
                for (int64_t j = s; j < e; j += kPadUnroll) {
                    u32x4 raw[kPadUnroll];
                    float w[kPadUnroll];
                    bool keep[kPadUnroll];
                    int64_t r[kPadUnroll];
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        const int64_t jj = j + u < e ? j + u : e - 1;
                        r[u] = load_index(p.indices, jj, p.idx64);
                        w[u] = WEIGHTED ? as_global<float>(p.psw)[jj] : 1.0f;
                        keep[u] = j + u < e && r[u] != pad;
                    }
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        raw[u] = u32x4{0u, 0u, 0u, 0u};
                        if (keep[u]) raw[u] = load16(Wc + row_offset<false>(r[u], row_bytes), false);
                    }
#pragma unroll
                    for (int u = 0; u < kPadUnroll; ++u) {
                        if (keep[u]) add(raw[u], w[u]);
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

// the launcher ladder, once for every pooling and output type: MEAN is unweighted (psw is dropped) and takes a NULL pad_idx
template <typename WT, int G, bool MEAN, typename OT>
hipError_t launch_pad_w(const KParams& p0, const int64_t* pad_idx, hipStream_t stream) {
    KParams p = p0;
    if (MEAN) p.psw = nullptr;
    const bool weighted = p.psw != nullptr;
    const int grid = p.T * p.tiles_per_table;
    const size_t tile_lds = pad_out_offset(p.bags_per_block, p.idx_cap, weighted);
    size_t lds = tile_lds + (p.stage_out > 0 ? static_cast<size_t>(p.bags_per_block) * p.stage_out * (std::is_same<OT, float>::value ? 4 : 2) : 0);
    if (lds > 65536) {                         // (explicit 1024-bag tiles of a weighted request: rows leave one by one)
        p.stage_out = 0;
        lds = tile_lds;
    }
    auto launch = [&](auto w) {
        hipLaunchKernelGGL((pad_fwd_kernel<WT, G, decltype(w)::value, MEAN, OT>), dim3(grid), dim3(kBlock), lds, stream, p, pad_idx);
    };
    if constexpr (MEAN) launch(std::false_type{});   // (mean is unweighted: no WEIGHTED + MEAN instance)
    else dispatch_bool(weighted, launch);
    return hipGetLastError();
}

template <typename WT, bool MEAN, typename OT>
hipError_t launch_pad_g(const KParams& p, int max_dim, const int64_t* pad_idx, hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, Elem<WT>::kVec),
                                [&](auto g) { return launch_pad_w<WT, decltype(g)::value, MEAN, OT>(p, pad_idx, stream); });
}

// the 16-bit-output variants of one table dtype (one translation unit each): 4 group widths x {plain, weighted, mean} x {bf16, fp16}
template <typename WT>
hipError_t launch_pad_out16(const KParams& p, int max_dim, const int64_t* pad_idx, bool mean, int out_dtype, hipStream_t stream) {
    if (out_dtype == PM_BF16)
        return mean ? launch_pad_g<WT, true, OutBF16>(p, max_dim, pad_idx, stream) : launch_pad_g<WT, false, OutBF16>(p, max_dim, pad_idx, stream);
    return mean ? launch_pad_g<WT, true, OutF16>(p, max_dim, pad_idx, stream) : launch_pad_g<WT, false, OutF16>(p, max_dim, pad_idx, stream);
}
