// param_amd/csrc/sparse_rows_adam.hip -- pm_sparse_rows_adam: lazy Adam / AdamW over COALESCED sparse gradients, T tables in one launch.
// gfx950 only.  The gradient is what pm_embbag_sparse_grad writes: per table U_t DISTINCT row ids and a [U_t, D_t] fp32 value block.
// Rows are distinct, so there is no sort, no run and no race: a listed row is read (g, w, m, v) and written (w, m, v) exactly once,
// seven rows of traffic per distinct row; rows that are not listed, and their state, are never touched.
//
// The rule (include/param_amd.h, SPARSE-ROW ADAM; numpy restates it bit for bit: tests/sparse_adam_rules.py) -- every operation one
// fp32 rounding, nothing contracted into an FMA, sqrt and division correctly rounded:
//     w0 = decay ? w * d : w ;  m' = m + (g - m) * c1 ;  v' = v + (g * g - v) * c2 ;  w' = round(w0 - s * (m' / (sqrt(v') + eps)))
//
// A tile is kBlock consecutive ROW SLOTS of the concatenated [0, U) (U = sum U_t), whatever tables they belong to:
//   1. every thread resolves its own slot: the slot's table among the T + 1 prefix entries -- an LDS copy of them (T + 1 <=
//      kAdamLdsPrefix) or a binary search in global memory, the un-pooled gather's scheme (embedding_gather.hip) --, its row id (one
//      coalesced load), and the four row addresses (64-bit: rows_t * D_t may exceed 2^31), which it hands to the lane groups through LDS;
//   2. the tile is walked in RUNS of consecutive tables of one lane-group width G = next_pow2(D_t / 4), capped at 64 (a D = 8 table
//      uses 2 lanes per row, 128 rows per step of the workgroup; wider rows than 256 columns take column passes).  A run of one width
//      is one loop whatever tables it spans: 300 one-row tables of one width are one run, not 300;
//   3. a lane owns four columns: 16-byte loads of g, m, v and of an fp32 w, an 8-byte load of a 16-bit w.  kAdamRows rows are in
//      flight per lane group: all their loads are issued before the first use, then the rule runs in registers and three stores leave.
//      Loads are unconditional -- a lane past the row's width or past the run reads the run's first row, column 0, and stores
//      nothing -- so the batch is straight-line code.  g, m and v are touched once per step: non-temporal when NT (the entry point's
//      cache-policy switch, a speed matter only); w takes plain accesses, the next forward reads it.
// No atomics, no inline assembly, no scratch, no cross-lane operation.
#include "sparse_rows_walk.h"

namespace pm {
namespace {

using namespace rows;

constexpr int kAdamRows = 4;          // rows in flight per lane group (fp32: 4 x 16 VGPRs of row data; no kernel spills)

struct AdamArgs {
    void* const* tables;
    const int64_t* const* row_ids;
    const float* const* values;
    float* const* m;
    float* const* v;
    const int32_t* dims;
    const int64_t* prefix;        // [T + 1]: prefix[t] = U_0 + .. + U_{t-1}
    int64_t U;
    int32_t T;
    int32_t lds_prefix;
    int32_t decay;                // d != 1: w0 = w * d
    int32_t maximize;
    float c1, c2, eps, s, d;
};

template <typename WT, bool NT>
__global__ void __launch_bounds__(kBlock) sparse_rows_adam_kernel(const AdamArgs a) {
    typedef typename AdamW<WT>::raw_t wraw_t;
    constexpr int ES = static_cast<int>(sizeof(wraw_t)) / 4;     // bytes per table element
    __shared__ int64_t s_prefix[kAdamLdsPrefix];
    __shared__ int64_t s_w[kBlock], s_g[kBlock], s_m[kBlock], s_v[kBlock];   // the slot's row addresses
    __shared__ int32_t s_dim[kBlock];                                        // its width in columns
    __shared__ int32_t s_first, s_last;                                      // the tile's first and last table

    const int tid = static_cast<int>(threadIdx.x);
    const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kBlock;
    const int n = a.U - j0 < kBlock ? static_cast<int>(a.U - j0) : kBlock;   // slots of this tile (>= 1: the grid is ceil(U / kBlock))
    const int64_t j = j0 + tid;

    // 1. the slot's table (sparse_rows_walk.h), from the LDS copy of the prefix or from global memory
    int lo;
    if (a.lds_prefix) {
        if (tid <= a.T) s_prefix[tid] = a.prefix[tid];
        __syncthreads();
        lo = slot_table(s_prefix, a.T, j);
    } else {
        lo = slot_table(a.prefix, a.T, j);
    }
    if (tid < n) {
        const int t = lo;
        const int64_t k = j - (a.lds_prefix ? s_prefix[t] : a.prefix[t]);
        const int64_t D = a.dims[t];
        const int64_t at = as_global<int64_t>(a.row_ids[t])[k] * D;          // 64-bit element offset of the row
        s_w[tid] = reinterpret_cast<int64_t>(a.tables[t]) + at * ES;
        s_m[tid] = reinterpret_cast<int64_t>(a.m[t] + at);
        s_v[tid] = reinterpret_cast<int64_t>(a.v[t] + at);
        s_g[tid] = reinterpret_cast<int64_t>(a.values[t] + k * D);
        s_dim[tid] = static_cast<int32_t>(D);
        if (tid == 0) s_first = t;
        if (tid == n - 1) s_last = t;
    }
    __syncthreads();

    // 2. runs of consecutive tables of one lane-group width (every value below is uniform over the workgroup)
    const float sign = a.maximize ? -1.0f : 1.0f;
    const int t_last = s_last;
    int t = s_first;
    int b = 0;                                                               // the next run's first slot of the tile
    while (b < n) {
        const int lg = adam_group_log2(s_dim[b]);
        int d_max = 0;
        const int run0 = b;
        b = a.lds_prefix ? run_end(s_prefix, a.dims, j0, n, t_last, lg, b, t, d_max)   // tables [t, ..) of this width
                         : run_end(a.prefix, a.dims, j0, n, t_last, lg, b, t, d_max);
        const int G = 1 << lg, NG = kBlock >> lg;
        const int gid = tid >> lg, lig = tid & (G - 1);
        const int passes = (d_max + 4 * G - 1) / (4 * G);                    // > 1 only for G = 64 and rows wider than 256 columns
        // 3. batches of kAdamRows rows per lane group: slot run0 + gid + i * NG
        for (int i0 = run0 + gid; i0 < b; i0 += kAdamRows * NG) {
            for (int pass = 0; pass < passes; ++pass) {
                const int c = (pass * G + lig) * 4;
                int64_t aw[kAdamRows], ag[kAdamRows], am[kAdamRows], av[kAdamRows];
                int cc[kAdamRows];
                bool live[kAdamRows];
#pragma unroll
                for (int u = 0; u < kAdamRows; ++u) {
                    const int q = i0 + u * NG;
                    const bool in_run = q < b;
                    const int qq = in_run ? q : run0;
                    live[u] = in_run && c < s_dim[qq];
                    cc[u] = live[u] ? c : 0;
                    aw[u] = s_w[qq]; ag[u] = s_g[qq]; am[u] = s_m[qq]; av[u] = s_v[qq];
                }
                f32x4 g[kAdamRows], m[kAdamRows], v[kAdamRows];
                wraw_t w[kAdamRows];
#pragma unroll
                for (int u = 0; u < kAdamRows; ++u) {
                    g[u] = adam_load4<NT>(ag[u], cc[u]);
                    m[u] = adam_load4<NT>(am[u], cc[u]);
                    v[u] = adam_load4<NT>(av[u], cc[u]);
                    w[u] = *(reinterpret_cast<const PM_GLOBAL wraw_t*>(aw[u]) + (cc[u] >> 2));
                }
#pragma unroll
                for (int u = 0; u < kAdamRows; ++u) {
                    float wn[4];
                    f32x4 mn, vn;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float gk = __fmul_rn(g[u][k], sign);           // exact: -g under maximize
                        const float wk = AdamW<WT>::widen(w[u], k);
                        const float w0 = a.decay ? __fmul_rn(wk, a.d) : wk;
                        mn[k] = __fadd_rn(m[u][k], __fmul_rn(__fsub_rn(gk, m[u][k]), a.c1));
                        vn[k] = __fadd_rn(v[u][k], __fmul_rn(__fsub_rn(__fmul_rn(gk, gk), v[u][k]), a.c2));
                        const float q = mn[k] / __fadd_rn(sqrtf(vn[k]), a.eps);   // correctly rounded sqrt and division
                        wn[k] = __fsub_rn(w0, __fmul_rn(a.s, q));
                    }
                    if (live[u]) {
                        adam_store4<NT>(am[u], c, mn);
                        adam_store4<NT>(av[u], c, vn);
                        *(reinterpret_cast<PM_GLOBAL wraw_t*>(aw[u]) + (c >> 2)) = AdamW<WT>::pack(wn);
                    }
                }
            }
        }
    }
}

template <typename WT>
hipError_t launch_adam_nt(const AdamArgs& a, bool nt, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((a.U + kBlock - 1) / kBlock)), block(kBlock);
    if (nt) hipLaunchKernelGGL((sparse_rows_adam_kernel<WT, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((sparse_rows_adam_kernel<WT, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace

// every array is a device array (see include/param_amd.h); U >= 1, T >= 1, U / kBlock below 2^31: the caller's checks
hipError_t launch_sparse_rows_adam(int T, int64_t U, void* const* tables, int table_dtype, const int64_t* const* row_ids,
                                   const float* const* values, float* const* m, float* const* v, const int32_t* dims,
                                   const int64_t* prefix, const pm_sparse_adam* opt, hipStream_t stream) {
    AdamArgs a;
    a.tables = tables; a.row_ids = row_ids; a.values = values; a.m = m; a.v = v; a.dims = dims; a.prefix = prefix;
    a.U = U; a.T = T;
    a.lds_prefix = T + 1 <= kAdamLdsPrefix ? 1 : 0;
    a.decay = opt->decay != 1.0f ? 1 : 0;      // w * 1 is w: skipping the product changes no bit
    a.maximize = opt->maximize;
    a.c1 = opt->c1; a.c2 = opt->c2; a.eps = opt->eps; a.s = opt->step_size; a.d = opt->decay;
    const bool nt = opt->nontemporal != 0;
    if (table_dtype == PM_BF16) return launch_adam_nt<bf16_t>(a, nt, stream);
    if (table_dtype == PM_F16) return launch_adam_nt<f16_t>(a, nt, stream);
    return launch_adam_nt<float>(a, nt, stream);
}

}  // namespace pm
