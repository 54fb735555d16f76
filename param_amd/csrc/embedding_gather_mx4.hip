// param_amd/csrc/embedding_gather_mx4.hip -- pm_embedding_gather_mx4: the UN-POOLED lookup over MXFP4 tables (include/param_amd.h, MXFP4
// TABLES).  out[j, c] = conv(v(table_t[indices[j], c])) for every lookup position j of the bag slice.  gfx950 only.
//
// pm_embedding_gather_f8's kernel (embedding_gather_f8.hip) with another lane: a tile is kBlock consecutive POSITIONS of the index array
// across table borders; every thread finds its position's table among the borders (gather_position_table, fwd_elem.h), turns (table, row)
// into the row's address and width once and hands both to the lane groups through LDS; row loads are unconditional, only the stores are
// predicated; stores are non-temporal; two batches of U rows ping-pong, each fetched in front of the other's stores.
// THE LANE holds FOUR columns (plan_gather_mx4, launch_plan.h): TWO BYTES of codes (one global_load_ushort) and its block's scale byte
// (one global_load_ubyte, issued with it; the eight lanes of a block read the same byte, one request to the memory pipeline), decoded by
// two v_cvt_scalef32_pk_f32_fp4 (mx4_elem.h) to four floats that leave as ONE 16-byte piece (fp32) or one 8-byte piece (bf16 / fp16: the
// one rounding of OutBF16 / OutF16).  A lane group of G = D / 4 lanes (at most 64: column passes of 256 columns above, eight at D = 2048) so
// reads a row's codes contiguously AND writes consecutive pieces of the output row with every store instruction -- the condition the FP8
// and the 4-bit gathers were built to.  Wider loads with a code exchange inside the group: not built.
// No atomics, no scratch, no inline assembly.
#include "common.h"
#include "fwd_elem.h"
#include "mx4_elem.h"

namespace pm {
namespace {

using namespace fwd;

struct Mx4Piece {
    uint32_t w;      // two code bytes
    uint32_t x;      // the block's scale byte
};

// p.io = out, p.out_stride = out_row_stride (output elements); p.out_offsets is not read
template <typename OT, int G, int U>
__global__ void __launch_bounds__(kBlock) embedding_gather_mx4_kernel(const KParams p, const int col_passes, const int lds_borders, const int xcd_contiguous) {
    constexpr int LC = kMx4GatherLaneColumns;  // columns per lane and pass
    constexpr int OB = std::is_same<OT, float>::value ? 4 : 2;
    constexpr int NG = kBlock / G;
    constexpr int NB = G / U;                  // batches of U rows: a lane group owns kBlock / NG = G positions of the tile
    static_assert(G % U == 0, "the unroll divides the positions of a lane group");
    static_assert(LC == 4, "a lane's columns are two bytes of codes");
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
    // A position that is not written still gets a readable address (table 0's first row) and width 0: the row loads below are
    // unconditional and only the stores are predicated.
    int D = 0;
    int64_t src = reinterpret_cast<int64_t>(p.tables[0]);
    if (t >= 0) {
        D = p.dims[t];
        src = reinterpret_cast<int64_t>(p.tables[t]) + row_offset<true>(r, mx4::row_bytes(D));
    }
    s_src[tid] = src;
    s_dim[tid] = D;
    __syncthreads();

    const int gid = tid / G;
    const int lig = tid % G;
    char* out = reinterpret_cast<char*>(p.io);
    for (int pass = 0; pass < col_passes; ++pass) {   // rows wider than one group pass (D > 256)
        const int c = (pass * G + lig) * LC;
        // a batch: the U rows' addresses and widths from LDS first, then the 2 U loads back to back (a lane past the row's width reads
        // the row's first two bytes twice and stores nothing)
        auto fetch = [&](int b, Mx4Piece (&raw)[U], int (&dim)[U]) {
            int64_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                a[u] = s_src[q];
                dim[u] = s_dim[q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = c < dim[u];
                const char* row = reinterpret_cast<const char*>(a[u]);
                raw[u].w = *as_global<uint16_t>(row + (in ? c / 2 : 0));
                raw[u].x = *as_global<uint8_t>(row + (in ? dim[u] / 2 + c / mx4::kBlockColumns : 0));
            }
        };
        auto emit = [&](int b, const Mx4Piece (&raw)[U], const int (&dim)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = (b * U + u) * NG + gid;
                if (c < dim[u]) {
                    float f[4];
                    const float scale = mx4::scale_operand(raw[u].x);
                    mx4::widen_byte<0>(raw[u].w, raw[u].x, scale, f);
                    mx4::widen_byte<1>(raw[u].w, raw[u].x, scale, f + 2);
                    char* dst = out + ((j0 + q) * p.out_stride + c) * OB;
                    if constexpr (std::is_same<OT, float>::value) {
                        const f32x4 v = {f[0], f[1], f[2], f[3]};
                        __builtin_nontemporal_store(v, as_global<f32x4>(dst));
                    } else {
                        const u32x2 v = {OT::round(f[0]) | (OT::round(f[1]) << 16), OT::round(f[2]) | (OT::round(f[3]) << 16)};
                        __builtin_nontemporal_store(v, as_global<u32x2>(dst));
                    }
                }
            }
        };
        // two batches ping-pong between two register sets; kept a loop (embedding_gather.hip says why)
        Mx4Piece ra[U], rb[U];
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

template <typename OT, int G>
hipError_t launch_gather_mx4_u(const KParams& p, const GatherPlan& g, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(g.grid)), block(kBlock);
    auto launch = [&](auto u) {
        hipLaunchKernelGGL((embedding_gather_mx4_kernel<OT, G, decltype(u)::value>), grid, block, 0, stream, p, g.col_passes, g.lds_borders,
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

}  // namespace

hipError_t launch_embedding_gather_mx4(const KParams& p, int out_dtype, const GatherPlan& g, hipStream_t stream) {
    auto go = [&](auto gl) {
        constexpr int G = decltype(gl)::value;
        if (out_dtype == PM_BF16) return launch_gather_mx4_u<OutBF16, G>(p, g, stream);
        if (out_dtype == PM_F16) return launch_gather_mx4_u<OutF16, G>(p, g, stream);
        return launch_gather_mx4_u<float, G>(p, g, stream);
    };
    return dispatch_group_lanes(g.group_lanes, go);
}

}  // namespace pm
