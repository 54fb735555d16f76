// param_amd/csrc/embedding_gather_qrows.hip -- pm_embedding_gather_qrows: the UN-POOLED lookup over 8- and 4-bit ROW-QUANTISED tables
// (int-nbit TBE's PoolingMode.NONE, torch.ao.nn.quantized.Embedding, quantized::embedding_byte / embedding_4bit).  gfx950 only.
//
// THE RULE (include/param_amd.h, "ROW-QUANTISED TABLES"; tests/qgather_rules.py restates it): for every lookup position j of the bag
// slice, t the table that owns j, r = indices[j], per column c < D_t
//     out[j, c] = conv( fmaf(scale_r, (float)code[r, c], fl32(+0.0f + bias_r)) )
// -- the pooled rule (embbag_fwd_qrows.hip) of one unweighted bag of one lookup, bit for bit: the addition is part of it (a bias of -0.0
// becomes +0.0 before the fused multiply-add).  The build has -ffp-contract=off: the addition is a statement of its own and the fmaf is
// written out.  conv: the identity for fp32, ONE rounding of the fp32 value in registers for bf16 / fp16 (OutBF16 / OutF16, fwd_elem.h).
//
// HOW: the tiles of embedding_gather.hip -- kBlock consecutive POSITIONS of the index array, whatever tables they belong to -- and its
// steps 1 and 2: one coalesced index load per thread, the position's table from the T borders (gather_position_table, fwd_elem.h), the
// row's address tables[t] + r * rq::row_bytes(D_t, BITS) -- 4-byte aligned and no better -- and width handed to the lane groups through
// LDS, width 0 meaning "never written".
//   3. a lane group of G = group_lanes(max_dim, qrows_lane_columns(BITS)) lanes serves one row.  Per row a lane issues ONE load of
//      kQrowsLaneDwords dwords of codes at a dword-aligned address (two dwords: 8 columns of an 8-bit row, 16 of a 4-bit row) and the
//      load of the row's tail (QRow<BITS>::tail, qrows_elem.h: every lane of the group reads that address itself, one request to the
//      memory pipeline); the group's lanes then exchange codes so that each store instruction writes consecutive pieces of the row
//      (store_dequantized below), unpack in registers, apply the rule and store non-temporally in pieces of 4 outputs -- 16 bytes of
//      fp32, 8 bytes of 16-bit output --, each predicated on its first column lying below D_t (D_t is a multiple of 4: a piece never
//      straddles the row's end).
//      U rows are in flight per lane group, in embedding_gather.hip's two ping-pong batches, each fetched in front of the other's stores:
//      loads and stores retire through one in-order counter, so a wait for loads issued behind a batch of stores waits for those stores.
//      Rows wider than G * lane columns take column passes (8-bit D > 512, 4-bit D > 1024).
// EVERY READ STAYS INSIDE A ROW: with two dwords per lane the dwords of a row's last lane that lie behind the codes are the row's own
// tail (qrows_elem.h); a lane wholly past the row's width reads the row's first bytes -- its first kQrowsLaneDwords dwords: the
// narrowest rows are 12 (8-bit D = 4) and 8 bytes (4-bit D = 8) -- and stores nothing; a position of width 0 reads table 0's first row
// only, with "0 columns of codes": its code load and its tail load both start at the row's first byte.
// The geometry is plan_gather_qrows' alone (launch_plan.h).  No atomics, no scalar-unit memory writes, no inline assembly, no scratch.
#include "common.h"
#include "fwd_elem.h"
#include "qrows_elem.h"

namespace pm {
namespace {

using namespace fwd;

// One row's pieces of 4 outputs leave.  A lane LOADED P = CV / 4 adjacent pieces' codes (4 * BITS bits each); stored as they lie in the
// lane, one store instruction would write 16 of every 16 * P bytes of the row -- measured that way the 4-bit table's fp32 rows took
// 1933 us where the pooled route takes 414 (profiles/qgather_probe_lane_major.json).  So the lanes of the group first exchange CODES
// (ds_bpermute through __shfl: registers, no LDS memory): for store s = 0 .. P - 1 lane l takes piece s * G + l of the pass -- it lies in
// lane (s * G + l) / P as that lane's piece l % P -- and every store instruction writes G consecutive pieces of the row.  Then THE RULE
// in registers and the non-temporal store, predicated on the piece's first column lying below the row's width.  Every lane of the wave
// runs the exchange (a lane past the row's width hands on the row's first dwords, which only pieces past the width receive).
// row_out: the position's output row; c0: the pass's first column.
template <int BITS, typename OT, int G>
__device__ __forceinline__ void store_dequantized(char* row_out, const QLoad<BITS>& q, int lig, int c0, int dim) {
    constexpr int P = QRow<BITS>::kVec * kLaneDwords / 4;      // pieces per lane and pass
    constexpr int PPD = QRow<BITS>::kVec / 4;                  // pieces per dword of codes
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    static_assert(G % P == 0, "a lane group's pieces divide over its stores");
    const float t = 0.0f + q.tail.bias;
    const int slot = lig % P;                                  // which of the source lane's pieces this lane takes
#pragma unroll
    for (int s = 0; s < P; ++s) {
        uint32_t w = q.raw[0];
        if constexpr (P > 1) {
            const int src = s * (G / P) + lig / P;
#pragma unroll
            for (int h = 0; h < kLaneDwords; ++h) {
                const uint32_t v = static_cast<uint32_t>(__shfl(static_cast<int>(q.raw[h]), src, G));
                if (h == 0 || slot / PPD == h) w = v;
            }
            if constexpr (PPD > 1) w >>= (32 / PPD) * (slot % PPD);
        }
        float f[4];
        QRow<BITS>::piece(w, f);
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = fmaf(q.tail.scale, f[k], t);
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
template <int BITS, typename OT, int G, int U>
__global__ void __launch_bounds__(kBlock) embedding_gather_qrows_kernel(const KParams p, const int col_passes, const int lds_borders, const int xcd_contiguous) {
    constexpr int VEC = QRow<BITS>::kVec;
    constexpr int CV = VEC * kLaneDwords;      // columns per lane and column pass
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    constexpr int NG = kBlock / G;
    constexpr int NB = G / U;                  // batches of U rows: a lane group owns kBlock / NG = G positions of the tile
    static_assert(G % U == 0, "the unroll divides the positions of a lane group");
    __shared__ int64_t s_border[kGatherLdsBorders];
    __shared__ int64_t s_src[kBlock];          // address of the position's row
    __shared__ int32_t s_dim[kBlock];          // its width in columns; 0: the position is not written

    const int tid = static_cast<int>(threadIdx.x);
    const int64_t j0 = gather_block_tile(blockIdx.x, gridDim.x, xcd_contiguous != 0) * kBlock;
    const int64_t j = j0 + tid;
    const bool inside = j < p.N;
    int64_t r = 0;
    if (inside) r = load_index(p.indices, j, p.idx64);

    const int t = gather_position_table(p, lds_borders, s_border, j, inside);
    // a position that is not written: table 0's first row and width 0 -- the loads below are unconditional, only the stores are predicated
    int D = 0;
    int64_t src = reinterpret_cast<int64_t>(p.tables[0]);
    if (t >= 0) {
        D = p.dims[t];
        src = reinterpret_cast<int64_t>(p.tables[t]) + row_offset<true>(r, rq::row_bytes(D, BITS));
    }
    s_src[tid] = src;
    s_dim[tid] = D;
    __syncthreads();

    const int gid = tid / G;
    const int lig = tid % G;
    char* out = reinterpret_cast<char*>(p.io);
    for (int pass = 0; pass < col_passes; ++pass) {   // rows wider than one group pass (8-bit D > 512, 4-bit D > 1024)
        const int c = (pass * G + lig) * CV;
        // a batch: the U rows' addresses and widths from LDS first, then the U rows' loads back to back (a lane past the row's width
        // reads the row's first dwords and stores nothing)
        auto fetch = [&](int b, QLoad<BITS> (&raw)[U], int (&dim)[U]) {
            int64_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                a[u] = s_src[q];
                dim[u] = s_dim[q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                raw[u] = load_row<BITS>(reinterpret_cast<const char*>(a[u]), c < dim[u] ? c / VEC * 4 : 0, dim[u] * BITS / 8);
            // nothing moves across this point: without it the scheduler lifts the first row's code exchange in between the loads,
            // and with it a full wait for that row's load in front of the batch's other loads (seen in the 4-bit instances' code)
            __builtin_amdgcn_sched_barrier(0);
        };
        auto emit = [&](int b, const QLoad<BITS> (&raw)[U], const int (&dim)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                store_dequantized<BITS, OT, G>(out + (j0 + q) * p.out_stride * OB, raw[u], lig, pass * G * CV, dim[u]);
            }
        };
        // embedding_gather.hip's ping-pong: two register sets, each fetched in front of the other's stores, none ever copied; kept a
        // loop (unrolled, the compiler hoists every batch's loads to the front)
        QLoad<BITS> ra[U], rb[U];
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

template <int BITS, typename OT, int G>
hipError_t launch_qgather_u(const KParams& p, const GatherPlan& g, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(g.grid)), block(kBlock);
    auto launch = [&](auto u) {
        hipLaunchKernelGGL((embedding_gather_qrows_kernel<BITS, OT, G, decltype(u)::value>), grid, block, 0, stream, p, g.col_passes, g.lds_borders,
                           g.xcd_contiguous);
    };
    switch (g.unroll) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        default: launch(std::integral_constant<int, 4>{}); break;
    }
    return hipGetLastError();
}

template <int BITS, typename OT>
hipError_t launch_qgather_g(const KParams& p, const GatherPlan& g, hipStream_t stream) {
    return dispatch_group_lanes(g.group_lanes, [&](auto gl) { return launch_qgather_u<BITS, OT, decltype(gl)::value>(p, g, stream); });
}

template <int BITS>
hipError_t launch_qgather_o(const KParams& p, int out_dtype, const GatherPlan& g, hipStream_t stream) {
    if (out_dtype == PM_BF16) return launch_qgather_g<BITS, OutBF16>(p, g, stream);
    if (out_dtype == PM_F16) return launch_qgather_g<BITS, OutF16>(p, g, stream);
    return launch_qgather_g<BITS, float>(p, g, stream);
}

}  // namespace

// p.io = out of out_dtype (PM_F32 | PM_BF16 | PM_F16), p.out_stride = its row stride in elements; bits 8 | 4; g: plan_gather_qrows'
hipError_t launch_embedding_gather_qrows(const KParams& p, int bits, int out_dtype, const GatherPlan& g, hipStream_t stream) {
    return bits == 8 ? launch_qgather_o<8>(p, out_dtype, g, stream) : launch_qgather_o<4>(p, out_dtype, g, stream);
}

}  // namespace pm
