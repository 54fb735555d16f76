// param_amd/csrc/embedding_gather_anyfmt.hip -- pm_embedding_gather_anyfmt: the UN-POOLED lookup over tables that are EACH stored in one
// of seven formats (include/param_amd.h, MIXED-FORMAT TABLES).  table_formats: device int32 [T] of PM_F32 |
// PM_BF16 | PM_F16 | PM_F8E4M3 | PM_F8E5M2 | PM_Q8 | PM_Q4; table_exp: device int32 [T] or NULL, read for FP8 tables.  gfx950 only.
//
// THE RULE is, per position, the un-pooled rule of the format of the table that owns it -- no new arithmetic: for every lookup position j
// of the bag slice, t the table that owns j, r = indices[j], per column c < D_t
//     fp32 / bf16 / fp16      out[j, c] = conv(table_t[r, c])                      (embedding_gather.hip)
//     FP8                     out[j, c] = conv(dec(code[r, c]) * 2^E_t)            (embedding_gather_f8s.hip)
//     8- / 4-bit rows         out[j, c] = conv(fmaf(scale_r, (float)code[r, c], fl32(+0.0f + bias_r)))   (embedding_gather_qrows.hip)
// conv: same element type in and out is a bit copy -- no arithmetic touches the bits; otherwise the exact widening and, for a 16-bit
// output, the one rounding of OutBF16 / OutF16 (fwd_elem.h).  The build has -ffp-contract=off.
//
// HOW: embedding_gather.hip's tiles of kBlock consecutive POSITIONS, whatever tables own them, and its first steps: one index load per
// thread, the position's table from the T borders (gather_position_table), the row's address handed to the lane groups through LDS with
// the row's width and FORMAT in one word and, for an FP8 row, 2^E_t next to it.  The format is a row's, so lane groups of one wave may
// differ in it: this kernel BRANCHES per lane group -- once for the loads of a batch of U rows, once for their conversion -- and accepts
// the divergence (one instruction stream for all seven, as embedding_gather_qmixed.hip has for two, was not built).
// A lane holds EIGHT COLUMNS per row and pass, as TWO PIECES of four: pieces lig and G + lig of the pass's 2 G pieces.  A load and a
// store instruction of the lane group therefore touch consecutive pieces of the row -- 16 bytes of fp32, 8 of a 16-bit type, 4 code
// bytes of FP8 / 8-bit rows, 2 of a 4-bit row -- with no exchange between lanes.  A piece at or behind the row's width is neither read
// nor written, and a position that is not written (or whose format code is none of the seven, which writes +0.0) reads no table byte.
// The geometry is plan_gather_anyfmt's alone.  No atomics, no inline assembly, no scratch.
#include "common.h"
#include "fwd_elem.h"
#include "f8s_elem.h"
#include "qrows_elem.h"

namespace pm {
namespace {

using namespace fwd;

constexpr int kFmtShift = 16;              // a position's width word: columns | (format + 1) << 16; 0: the position is not written
constexpr int kGatherAnyU = kAnyfmtGatherUnroll;

// one row's two pieces of this lane and a quantised row's tail, as loaded
struct AnyRaw {
    u32x4 pc[2];
    u32x2 tail;
};

typedef uint32_t u32x2_a8 __attribute__((ext_vector_type(2)));

// c0, c1: the lane's two pieces' first columns; a piece at or behind the width is not read
__device__ __forceinline__ AnyRaw load_any(const char* row, int fmt, int D, int c0, int c1) {
    AnyRaw q;
    q.pc[0] = u32x4{0u, 0u, 0u, 0u};
    q.pc[1] = u32x4{0u, 0u, 0u, 0u};
    q.tail = u32x2{0u, 0u};
    const int c[2] = {c0, c1};
    switch (fmt) {
        case PM_F32:
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (c[s] < D) q.pc[s] = load16(row + c[s] * 4, false);
            break;
        case PM_BF16:
        case PM_F16:
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (c[s] < D) {
                    const u32x2_a8 v = *as_global<u32x2_a8>(row + c[s] * 2);
                    q.pc[s].x = v.x;
                    q.pc[s].y = v.y;
                }
            break;
        case PM_F8E4M3:
        case PM_F8E5M2:
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (c[s] < D) q.pc[s].x = *as_global<uint32_t>(row + c[s]);
            break;
        case PM_Q8:
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (c[s] < D) q.pc[s].x = *as_global<uint32_t>(row + c[s]);
            if (c0 < D) q.tail = *as_global<u32x2_a4>(row + D);
            break;
        case PM_Q4:
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (c[s] < D) q.pc[s].x = *as_global<uint16_t>(row + c[s] / 2);
            if (c0 < D) q.tail.x = *as_global<uint32_t>(row + D / 2);
            break;
        default: break;
    }
    return q;
}

// the four output values of one piece leave: fp32 as one 16-byte store, 16-bit as one 8-byte store of the once-rounded values
template <typename OT>
__device__ __forceinline__ void store_values(char* dst, const float (&f)[4]) {
    if constexpr (std::is_same<OT, float>::value) {
        const f32x4 v = {f[0], f[1], f[2], f[3]};
        __builtin_nontemporal_store(v, as_global<f32x4>(dst));
    } else {
        const u32x2 v = {OT::round(f[0]) | (OT::round(f[1]) << 16), OT::round(f[2]) | (OT::round(f[3]) << 16)};
        __builtin_nontemporal_store(v, as_global<u32x2>(dst));
    }
}

// a 16-bit piece of element type WT (two dwords of four elements): a bit copy to the same type, else widened and converted
template <typename WT, typename OT, bool SAME>
__device__ __forceinline__ void store_piece16(char* dst, const u32x4& pc) {
    if constexpr (SAME) {
        __builtin_nontemporal_store(u32x2{pc.x, pc.y}, as_global<u32x2>(dst));
    } else {
        float f8[8];
        Elem<WT>::widen(u32x4{pc.x, pc.y, 0u, 0u}, f8);
        const float f[4] = {f8[0], f8[1], f8[2], f8[3]};
        store_values<OT>(dst, f);
    }
}

// row_out: the position's output row; c0, c1 as in load_any; scale: 2^E_t of an FP8 row
template <typename OT>
__device__ __forceinline__ void store_any(char* row_out, const AnyRaw& q, int fmt, int D, int c0, int c1, float scale) {
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    const int c[2] = {c0, c1};
    float qs = 0.0f, qt = 0.0f;            // a quantised row's scale and +0.0 + bias
    if (fmt == PM_Q8) {
        qs = __uint_as_float(q.tail.x);
        qt = 0.0f + __uint_as_float(q.tail.y);
    } else if (fmt == PM_Q4) {
        qs = rq::half_value(static_cast<uint16_t>(q.tail.x & 0xffffu));
        qt = 0.0f + rq::half_value(static_cast<uint16_t>(q.tail.x >> 16));
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (c[s] >= D) continue;
        char* dst = row_out + c[s] * OB;
        const u32x4& pc = q.pc[s];
        float f[4];
        switch (fmt) {
            case PM_F32:
                if constexpr (std::is_same<OT, float>::value) {
                    __builtin_nontemporal_store(pc, as_global<u32x4>(dst));
                } else {
                    Elem<float>::widen(pc, f);
                    store_values<OT>(dst, f);
                }
                break;
            case PM_BF16: store_piece16<bf16_t, OT, std::is_same<OT, OutBF16>::value>(dst, pc); break;
            case PM_F16: store_piece16<f16_t, OT, std::is_same<OT, OutF16>::value>(dst, pc); break;
            case PM_F8E4M3:
                widen_f8_dword<f8e4m3_t>(pc.x, f);
#pragma unroll
                for (int k = 0; k < 4; ++k) f[k] *= scale;
                store_values<OT>(dst, f);
                break;
            case PM_F8E5M2:
                widen_f8_dword<f8e5m2_t>(pc.x, f);
#pragma unroll
                for (int k = 0; k < 4; ++k) f[k] *= scale;
                store_values<OT>(dst, f);
                break;
            case PM_Q8: {
                float code[4];
                QRow<8>::piece(pc.x, code);
#pragma unroll
                for (int k = 0; k < 4; ++k) f[k] = fmaf(qs, code[k], qt);
                store_values<OT>(dst, f);
                break;
            }
            case PM_Q4: {
                float code[4];
                QRow<4>::piece(pc.x, code);
#pragma unroll
                for (int k = 0; k < 4; ++k) f[k] = fmaf(qs, code[k], qt);
                store_values<OT>(dst, f);
                break;
            }
            default:                           // an unknown format code: +0.0
#pragma unroll
                for (int k = 0; k < 4; ++k) f[k] = 0.0f;
                store_values<OT>(dst, f);
                break;
        }
    }
}

// bytes of a row of D columns in format fmt (0 for an unknown code: its row is never read)
__device__ __forceinline__ int64_t any_row_bytes(int fmt, int D) {
    switch (fmt) {
        case PM_F32: return static_cast<int64_t>(D) * 4;
        case PM_BF16:
        case PM_F16: return static_cast<int64_t>(D) * 2;
        case PM_F8E4M3:
        case PM_F8E5M2: return D;
        case PM_Q8: return rq::row_bytes(D, 8);
        case PM_Q4: return rq::row_bytes(D, 4);
        default: return 0;
    }
}

// p.io = out, p.out_stride = out_row_stride (output elements); p.out_offsets and p.psw are not read
template <typename OT, int G>
__global__ void __launch_bounds__(kBlock) anyfmt_gather_kernel(const KParams p, const int32_t* __restrict__ table_formats,
                                                               const int32_t* __restrict__ table_exp, const int col_passes, const int lds_borders,
                                                               const int xcd_contiguous) {
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    constexpr int NG = kBlock / G;
    constexpr int U = kGatherAnyU;
    constexpr int NB = G / U;                  // batches of U rows: a lane group owns kBlock / NG = G positions of the tile
    static_assert(G % U == 0, "the unroll divides the positions of a lane group");
    __shared__ int64_t s_border[kGatherLdsBorders];
    __shared__ int64_t s_src[kBlock];          // address of the position's row
    __shared__ int32_t s_dim[kBlock];          // its width word; 0: the position is not written
    __shared__ float s_scale[kBlock];          // 2^E_t of its table

    const int tid = static_cast<int>(threadIdx.x);
    const int64_t j0 = gather_block_tile(blockIdx.x, gridDim.x, xcd_contiguous != 0) * kBlock;
    const int64_t j = j0 + tid;
    const bool inside = j < p.N;
    int64_t r = 0;
    if (inside) r = load_index(p.indices, j, p.idx64);

    const int t = gather_position_table(p, lds_borders, s_border, j, inside);
    int dimw = 0;
    int64_t src = 0;
    int e = 0;
    if (t >= 0) {
        const int D = p.dims[t];
        int fmt = *as_global<int32_t>(table_formats + t);
        if (fmt < 0 || fmt > PM_Q4) fmt = PM_Q4 + 1;          // every unknown code is one
        if (table_exp) e = *as_global<int32_t>(table_exp + t);
        dimw = D | ((fmt + 1) << kFmtShift);
        src = reinterpret_cast<int64_t>(p.tables[t]) + row_offset<true>(r, any_row_bytes(fmt, D));
    }
    s_src[tid] = src;
    s_dim[tid] = dimw;
    s_scale[tid] = f8s::pow2(f8s::clamp_exp(e));
    __syncthreads();

    const int gid = tid / G;
    const int lig = tid % G;
    char* out = reinterpret_cast<char*>(p.io);
    for (int pass = 0; pass < col_passes; ++pass) {   // rows wider than one group pass (D > 512)
        const int c0 = (pass * 2 * G + lig) * 4;
        const int c1 = c0 + G * 4;
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            // a batch: the U rows' addresses and width words from LDS first, then the U rows' loads, then their stores
            AnyRaw raw[U];
            int dimw_u[U];
            int64_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                a[u] = s_src[q];
                dimw_u[u] = s_dim[q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                raw[u] = load_any(reinterpret_cast<const char*>(a[u]), (dimw_u[u] >> kFmtShift) - 1, dimw_u[u] & 0xffff, c0, c1);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                if (dimw_u[u] != 0)
                    store_any<OT>(out + (j0 + q) * p.out_stride * OB, raw[u], (dimw_u[u] >> kFmtShift) - 1, dimw_u[u] & 0xffff, c0, c1, s_scale[q]);
            }
        }
    }
}

template <typename OT>
hipError_t launch_anygather_g(const KParams& p, const int32_t* table_formats, const int32_t* table_exp, const GatherPlan& g, hipStream_t stream) {
    return dispatch_group_lanes(g.group_lanes, [&](auto gl) {
        hipLaunchKernelGGL((anyfmt_gather_kernel<OT, decltype(gl)::value>), dim3(static_cast<unsigned>(g.grid)), dim3(kBlock), 0, stream, p,
                           table_formats, table_exp, g.col_passes, g.lds_borders, g.xcd_contiguous);
        return hipGetLastError();
    });
}

}  // namespace

// p.io = out of out_dtype (PM_F32 | PM_BF16 | PM_F16), p.out_stride = its row stride in elements; g: plan_gather_anyfmt's
hipError_t launch_embedding_gather_anyfmt(const KParams& p, const int32_t* table_formats, const int32_t* table_exp, int out_dtype, const GatherPlan& g,
                                          hipStream_t stream) {
    if (out_dtype == PM_BF16) return launch_anygather_g<OutBF16>(p, table_formats, table_exp, g, stream);
    if (out_dtype == PM_F16) return launch_anygather_g<OutF16>(p, table_formats, table_exp, g, stream);
    return launch_anygather_g<float>(p, table_formats, table_exp, g, stream);
}

}  // namespace pm
