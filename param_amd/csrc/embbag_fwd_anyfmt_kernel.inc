// param_amd/csrc/embbag_fwd_anyfmt_kernel.inc -- pm_embbag_fwd_anyfmt: the pooled lookup over tables that are EACH stored in one of
// seven formats -- fp32, bf16, fp16, OCP FP8 e4m3fn / e5m2 (with a power-of-two table exponent), 8- and 4-bit quantised rows
// (include/param_amd.h, MIXED-FORMAT TABLES; DESIGN.md section 3.19).  Included inside `namespace pm { namespace { ... } }`
// (after common.h, fwd_elem.h, f8s_elem.h and qrows_elem.h) by embbag_fwd_anyfmt_{f32,bf16,f16}.hip, one translation unit per OUTPUT
// type, each of which instantiates launch_any_w with its own output element.  gfx950 only.
//
// THE RULE is, per table, the rule of that format's own kernel -- no new arithmetic.  The lookups j of a bag in index order, from
// acc = +0.0, per column, r = indices[j]:
//     fp32 / bf16 / fp16      f = the element widened exactly          acc = acc + f         weighted: acc = fmaf(w_j, f, acc)
//     FP8                     f = dec(code[r, c]) * 2^E_t              (the same step; E_t = table_exp[t], clamped to [-64, 64])
//     8- / 4-bit rows         sc = scale_r * w_j, bi = bias_r * w_j    acc = fmaf(sc, (float)code[r, c], acc + bi)
//                             (unweighted: sc = scale_r, bi = bias_r; no multiplication happens)
// The build has -ffp-contract=off.  A 16-bit output is ONE rounding of the fp32 value (OutBF16 / OutF16, fwd_elem.h), in registers.
//
// HOW: embbag_fwd_qmixed.hip's tile and bag structure.  A tile's bags belong to one table, so the format is uniform per workgroup: the
// body reads table_formats[t] once and branches ONCE per tile into that format's instance of the same row loop.  A lane holds EIGHT
// COLUMNS of a row whatever the format -- fp32: two 16-byte loads; bf16 / fp16: one; FP8: one 8-byte load; 8-bit rows: two dwords;
// 4-bit rows: one dword -- so the lane group G = group_lanes(max_dim, 8), the eight accumulators, the column passes and the output
// pieces are the same for every table and the plan (plan_qmixed's, launch_plan.h) does not depend on the formats present.  Widths are
// multiples of 8: a lane's columns lie wholly inside the row.  Rows in flight: one compile-time value per format, that format's
// product default (the fp32 forward's 2 for the float formats, kF8Unroll, kQrowsUnroll).
// Kept from qmixed: the staged and unstaged index paths, the LDS output burst, the 16-bit output path, 64-bit row offsets,
// non-temporal output stores.  The row loop is qmixed's (and through it embbag_fwd_qrows.hip's) TWIN: those kernels' code objects must
// not move, so the loop stands again here; a fix to one belongs in the others.
// An unknown format code: the tile's rows are written +0.0 and no table byte is read.
// No atomics, no inline assembly, no scratch memory, no workspace.

using namespace fwd;

constexpr int kAnyCols = kAnyfmtLaneColumns;   // columns per lane and column pass, whatever the format

// ---- one format's pieces: what a lane loads of a row, and how one lookup joins the sum -------------------------------------------------
// load(row, c, D): the lane's eight columns c .. c + 7 of the row at `row` (D: the row's columns).  add<WEIGHTED>(acc, q, w, tab_scale).

// fp32 / bf16 / fp16: Elem<WT>::widen (fwd_elem.h) and accumulate's step
template <typename WT> struct AnyFloat;
template <> struct AnyFloat<float> {
    static constexpr int kUnroll = 2;
    struct Load { u32x4 lo, hi; };
    __device__ static __forceinline__ int64_t row_bytes(int D) { return static_cast<int64_t>(D) * 4; }
    __device__ static __forceinline__ Load load(const char* row, int c, int) { return Load{load16(row + c * 4, false), load16(row + c * 4 + 16, false)}; }
    __device__ static __forceinline__ void widen(const Load& q, float (&f)[8]) {
        float a[4], b[4];
        Elem<float>::widen(q.lo, a);
        Elem<float>::widen(q.hi, b);
#pragma unroll
        for (int k = 0; k < 4; ++k) { f[k] = a[k]; f[4 + k] = b[k]; }
    }
};
template <> struct AnyFloat<bf16_t> {
    static constexpr int kUnroll = 2;
    struct Load { u32x4 v; };
    __device__ static __forceinline__ int64_t row_bytes(int D) { return static_cast<int64_t>(D) * 2; }
    __device__ static __forceinline__ Load load(const char* row, int c, int) { return Load{load16(row + c * 2, false)}; }
    __device__ static __forceinline__ void widen(const Load& q, float (&f)[8]) { Elem<bf16_t>::widen(q.v, f); }
};
template <> struct AnyFloat<f16_t> {
    static constexpr int kUnroll = 2;
    struct Load { u32x4 v; };
    __device__ static __forceinline__ int64_t row_bytes(int D) { return static_cast<int64_t>(D) * 2; }
    __device__ static __forceinline__ Load load(const char* row, int c, int) { return Load{load16(row + c * 2, false)}; }
    __device__ static __forceinline__ void widen(const Load& q, float (&f)[8]) { Elem<f16_t>::widen(q.v, f); }
};
template <typename WT> struct AnyFmtFloat : AnyFloat<WT> {
    template <bool WEIGHTED>
    __device__ static __forceinline__ void add(float (&acc)[kAnyCols], const typename AnyFloat<WT>::Load& q, float w, float) {
        float f[kAnyCols];
        AnyFloat<WT>::widen(q, f);
#pragma unroll
        for (int k = 0; k < kAnyCols; ++k) acc[k] = WEIGHTED ? fmaf(w, f[k], acc[k]) : acc[k] + f[k];
    }
};

// FP8: eight code bytes, widened by the hardware conversion (widen_f8_dword), then embbag_fwd_f8s_kernel.inc's accumulate_scaled
template <typename WT> struct AnyFmtF8 {
    static constexpr int kUnroll = kF8Unroll;
    struct Load { u32x2 v; };
    __device__ static __forceinline__ int64_t row_bytes(int D) { return D; }
    __device__ static __forceinline__ Load load(const char* row, int c, int) { return Load{*as_global<u32x2>(row + c)}; }
    template <bool WEIGHTED>
    __device__ static __forceinline__ void add(float (&acc)[kAnyCols], const Load& q, float w, float scale) {
        float f[kAnyCols];
        widen_f8_dword<WT>(q.v.x, f);
        widen_f8_dword<WT>(q.v.y, f + 4);
#pragma unroll
        for (int k = 0; k < kAnyCols; ++k) {
            const float v = f[k] * scale;
            acc[k] = WEIGHTED ? fmaf(w, v, acc[k]) : acc[k] + v;
        }
    }
};

// 8- / 4-bit rows: load_row_n (qrows_elem.h) and embbag_fwd_qmixed.hip's accumulate_qn
template <int BITS> struct AnyFmtQ {
    static constexpr int kUnroll = kQrowsUnroll;
    static constexpr int LD = kQmixedDwords<BITS>;
    static constexpr int VEC = QRow<BITS>::kVec;
    static_assert(LD * VEC == kAnyCols, "eight columns per lane");
    using Load = QLoadN<BITS, LD>;
    __device__ static __forceinline__ int64_t row_bytes(int D) { return rq::row_bytes(D, BITS); }
    __device__ static __forceinline__ Load load(const char* row, int c, int D) { return load_row_n<BITS, LD>(row, c / VEC * 4, D * BITS / 8); }
    template <bool WEIGHTED>
    __device__ static __forceinline__ void add(float (&acc)[kAnyCols], const Load& q, float w, float) {
        float sc = q.tail.scale, bi = q.tail.bias;
        if (WEIGHTED) {
            sc = sc * w;
            bi = bi * w;
        }
#pragma unroll
        for (int h = 0; h < LD; ++h) {
            float f[VEC];
            QRow<BITS>::unpack(q.raw[h], f);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float t = acc[h * VEC + k] + bi;
                acc[h * VEC + k] = fmaf(sc, f[k], t);
            }
        }
    }
};

// ---- the tile's bags of table t, whose rows are FMT's: embbag_fwd_qmixed.hip's pool_tile on FMT's load and accumulate step ---------------
template <typename FMT, int G, bool WEIGHTED, typename OT>
__device__ __forceinline__ void any_pool_tile(const KParams& p, int t, int64_t bag0, int nb, bool staged, const int64_t* s_off, const int32_t* s_idx,
                                              const float* s_w, float* s_out, float tab_scale) {
    constexpr bool OUT16 = !std::is_same<OT, float>::value;
    constexpr int NG = kBlock / G;
    constexpr int U = FMT::kUnroll;
    constexpr int CV = kAnyCols;
    using Load = typename FMT::Load;
    const int64_t base = s_off[0];
    uint16_t* s_out16 = reinterpret_cast<uint16_t*>(s_out);
    const int gid = threadIdx.x / G;
    const int lig = threadIdx.x % G;
    const int D = p.dims[t];
    const int64_t row_bytes = FMT::row_bytes(D);
    const char* W = reinterpret_cast<const char*>(p.tables[t]);
    float* out_t = p.io + p.out_offsets[t];
    // OUT16: io is the 16-bit output; offsets and strides count its 2-byte elements
    uint16_t* out16_t = reinterpret_cast<uint16_t*>(p.io) + p.out_offsets[t];
    const bool burst = p.stage_out > 0;

    for (int bg = gid; bg < nb; bg += NG) {
        const int64_t s = s_off[bg];
        const int64_t e = s_off[bg + 1];
        for (int c = lig * CV; c < D; c += G * CV) {   // (D % 8 == 0: a lane's eight columns end inside the row)
            float acc[CV];
#pragma unroll
            for (int k = 0; k < CV; ++k) acc[k] = 0.0f;
            if (staged) {
                int j = static_cast<int>(s - base);
                const int je = static_cast<int>(e - base);
                for (; j + U <= je; j += U) {
                    Load q[U];
                    float w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        q[u] = FMT::load(W + row_offset<true>(static_cast<int64_t>(s_idx[j + u]), row_bytes), c, D);
                        w[u] = WEIGHTED ? s_w[j + u] : 1.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) FMT::template add<WEIGHTED>(acc, q[u], w[u], tab_scale);
                }
                for (; j < je; ++j)
                    FMT::template add<WEIGHTED>(acc, FMT::load(W + row_offset<true>(static_cast<int64_t>(s_idx[j]), row_bytes), c, D),
                                                WEIGHTED ? s_w[j] : 1.0f, tab_scale);
            } else {
                // the tile's lookups exceed the index tile: indices (and weights) come from the request
                int64_t j = s;
                for (; j + U <= e; j += U) {
                    Load q[U];
                    float w[U];
                    int64_t r[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        r[u] = load_index(p.indices, j + u, p.idx64);
                        w[u] = WEIGHTED ? as_global<float>(p.psw)[j + u] : 1.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) q[u] = FMT::load(W + row_offset<false>(r[u], row_bytes), c, D);
#pragma unroll
                    for (int u = 0; u < U; ++u) FMT::template add<WEIGHTED>(acc, q[u], w[u], tab_scale);
                }
                for (; j < e; ++j)
                    FMT::template add<WEIGHTED>(acc, FMT::load(W + row_offset<false>(load_index(p.indices, j, p.idx64), row_bytes), c, D),
                                                WEIGHTED ? as_global<float>(p.psw)[j] : 1.0f, tab_scale);
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

// a tile of a table whose format code is none of the seven: its rows are +0.0, in pieces of 4 outputs; no table byte is read
template <typename OT>
__device__ __forceinline__ void any_zero_tile(const KParams& p, int t, int64_t bag0, int nb) {
    constexpr bool OUT16 = !std::is_same<OT, float>::value;
    const int D = p.dims[t];
    const int q = D / 4;
    for (int i = threadIdx.x; i < nb * q; i += kBlock) {
        const int bg = i / q, c4 = i % q;
        if constexpr (OUT16) {
            uint16_t* o = reinterpret_cast<uint16_t*>(p.io) + p.out_offsets[t] + (bag0 + bg) * p.out_stride + c4 * 4;
            __builtin_nontemporal_store(u32x2{0u, 0u}, reinterpret_cast<u32x2*>(o));
        } else {
            float* o = p.io + p.out_offsets[t] + (bag0 + bg) * p.out_stride + c4 * 4;
            __builtin_nontemporal_store(f32x4{0.0f, 0.0f, 0.0f, 0.0f}, reinterpret_cast<f32x4*>(o));
        }
    }
}

template <int G, bool WEIGHTED, typename OT>
__global__ void __launch_bounds__(kBlock) anyfmt_fwd_kernel(const KParams p, const int32_t* __restrict__ table_formats, const int32_t* __restrict__ table_exp) {
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

    // the tile's format: one table, one scalar load, one branch.  2^E_t (f8s_elem.h: pow2 of the clamped exponent) is the FP8 formats'.
    const int fmt = table_formats[t];
    const float tab_scale = f8s::pow2(f8s::clamp_exp(table_exp ? table_exp[t] : 0));
#define PM_ANY_TILE(FMT) any_pool_tile<FMT, G, WEIGHTED, OT>(p, t, bag0, nb, staged, s_off, s_idx, s_w, s_out, tab_scale)
    switch (fmt) {
        case PM_F32: PM_ANY_TILE(AnyFmtFloat<float>); break;
        case PM_BF16: PM_ANY_TILE(AnyFmtFloat<bf16_t>); break;
        case PM_F16: PM_ANY_TILE(AnyFmtFloat<f16_t>); break;
        case PM_F8E4M3: PM_ANY_TILE(AnyFmtF8<f8e4m3_t>); break;
        case PM_F8E5M2: PM_ANY_TILE(AnyFmtF8<f8e5m2_t>); break;
        case PM_Q8: PM_ANY_TILE(AnyFmtQ<8>); break;
        case PM_Q4: PM_ANY_TILE(AnyFmtQ<4>); break;
        default: any_zero_tile<OT>(p, t, bag0, nb); break;
    }
#undef PM_ANY_TILE
}

// the launcher ladder: weighted, then the group width
template <int G, typename OT>
hipError_t launch_any_w(const KParams& p0, const int32_t* table_formats, const int32_t* table_exp, hipStream_t stream) {
    KParams p = p0;
    const bool weighted = p.psw != nullptr;
    const int grid = p.T * p.tiles_per_table;
    const size_t tile_lds = (tile_lds_bytes(p.bags_per_block, p.idx_cap, weighted) + 15) / 16 * 16;
    size_t lds = tile_lds + (p.stage_out > 0 ? static_cast<size_t>(p.bags_per_block) * p.stage_out * (std::is_same<OT, float>::value ? 4 : 2) : 0);
    if (lds > 65536) {                         // (explicit 1024-bag tiles of a weighted request: rows leave one by one)
        p.stage_out = 0;
        lds = tile_lds;
    }
    dispatch_bool(weighted, [&](auto w) {
        hipLaunchKernelGGL((anyfmt_fwd_kernel<G, decltype(w)::value, OT>), dim3(grid), dim3(kBlock), lds, stream, p, table_formats, table_exp);
    });
    return hipGetLastError();
}
