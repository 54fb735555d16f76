// param_amd/csrc/sparse_rows_step.hip -- pm_sparse_rows_sgd / pm_sparse_rows_adagrad: SGD, element-wise Adagrad and row-wise Adagrad over
// COALESCED sparse gradients, T tables in one launch.  gfx950 only.  The gradient is what pm_embbag_sparse_grad writes: per table U_t
// DISTINCT row ids and a [U_t, D_t] fp32 value block, so a listed row is read and written exactly once and no other row is touched.
//
// The rules (include/param_amd.h, SPARSE-ROW ADAGRAD AND SGD; numpy restates them bit for bit: tests/sparse_step_rules.py) -- every
// operation one fp32 rounding, fmaf a true fused multiply-add and nothing else contracted, sqrt and division correctly rounded:
//     SGD       w' = conv(fmaf(alpha, g, w))
//     ADAGRAD   s' = s + g * g ;  w' = conv(fmaf(alpha, g / (sqrt(s') + eps), w))                         (s: [rows, D])
//     ROWWISE   s' = s + S / (float)D ;  mult = alpha / (sqrt(s') + eps) ;  w' = conv(fmaf(mult, g, w))   (s: [rows]; S: the row's sum of squares)
//
// The walk from a row slot to its row is Adam's (sparse_rows_walk.h, sparse_rows_adam.hip): tiles of kBlock consecutive row slots of the
// concatenated [0, U), the slot's table from an LDS copy of the prefix (or a search in global memory), the row addresses handed to
// the lane groups through LDS, runs of consecutive tables of one lane-group width G = next_pow2(D / 4) <= 64.  A lane owns four columns
// per column pass; kStepRows rows are in flight per lane group; loads are unconditional (a lane past the row's width or past the run
// reads the run's first row, column 0, and stores nothing), so a batch is straight-line code.
//   SGD, ADAGRAD   no cross-lane operation: the loads of the batch, the rule in registers, the stores.  g and s are touched once per
//                  step: non-temporal when NT.  w takes plain accesses, the next forward reads it.
//   ROWWISE        S is a function of the row, fixed in its order: lane l's partial starts at +0 and adds fl(g * g) with pass ascending,
//                  then column ascending; the G partials meet in an xor butterfly, masks 1, 2, .., G / 2 (__shfl_xor inside the lane group:
//                  the sum is commutative, so every lane ends with the same bits).
//                  Rows of at most 256 columns (one pass): the lane keeps its four g in registers; g, w and a broadcast load of the row's
//                  state value are all issued before the reduction; lane 0 of the group stores s'.
//                  Wider rows: two sweeps over the column passes.  The first accumulates the partial from PLAIN loads of g, so the second,
//                  which re-reads g (non-temporal when NT: its last use) next to w, finds it in L2; g is not held across passes.
// No atomics, no inline assembly, no scratch, no assumption that a row is listed twice.
#include "sparse_rows_walk.h"

namespace pm {
namespace {

using namespace rows;

constexpr int kStepRows = 4;          // rows in flight per lane group
enum { kSgd = 0, kAdagrad = 1, kRowwise = 2 };

struct StepArgs {
    void* const* tables;
    const int64_t* const* row_ids;
    const float* const* values;
    float* const* state;          // ADAGRAD: [rows_t, D_t]; ROWWISE: [rows_t]; SGD: never read
    const int32_t* dims;
    const int64_t* prefix;        // [T + 1]: prefix[t] = U_0 + .. + U_{t-1}
    int64_t U;
    int32_t T;
    int32_t lds_prefix;
    int32_t maximize;
    float alpha, eps;
};

// one batch of SGD / ADAGRAD: rows aw / ag / as at column c (cc: the column the loads use), no cross-lane operation
template <typename WT, int RULE, bool NT>
__device__ __forceinline__ void elementwise_batch(const int64_t (&aw)[kStepRows], const int64_t (&ag)[kStepRows],
                                                  const int64_t (&as)[kStepRows], const int (&cc)[kStepRows],
                                                  const bool (&live)[kStepRows], int c, float sign, float alpha, float eps) {
    f32x4 g[kStepRows], s[kStepRows];
    typename AdamW<WT>::raw_t w[kStepRows];
#pragma unroll
    for (int u = 0; u < kStepRows; ++u) {
        g[u] = adam_load4<NT>(ag[u], cc[u]);
        if (RULE == kAdagrad) s[u] = adam_load4<NT>(as[u], cc[u]);
        w[u] = w_load4<WT>(aw[u], cc[u]);
    }
#pragma unroll
    for (int u = 0; u < kStepRows; ++u) {
        float wn[4];
        f32x4 sn;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = __fmul_rn(g[u][k], sign);                       // exact: -g under maximize
            const float wk = AdamW<WT>::widen(w[u], k);
            if (RULE == kAdagrad) {
                sn[k] = __fadd_rn(s[u][k], __fmul_rn(gk, gk));
                const float q = gk / __fadd_rn(sqrtf(sn[k]), eps);           // correctly rounded sqrt and division
                wn[k] = __fmaf_rn(alpha, q, wk);
            } else {
                wn[k] = __fmaf_rn(alpha, gk, wk);
            }
        }
        if (live[u]) {
            if (RULE == kAdagrad) adam_store4<NT>(as[u], c, sn);
            w_store4<WT>(aw[u], c, wn);
        }
    }
}

// fl(g * g) of the lane's four columns onto its partial, column ascending; a lane that is not live adds nothing
__device__ __forceinline__ float add_squares(float p, const f32x4& g, bool live) {
#pragma unroll
    for (int k = 0; k < 4; ++k) p = __fadd_rn(p, live ? __fmul_rn(g[k], g[k]) : 0.0f);   // p is never -0: p + 0 is p
    return p;
}

// the G = 2^lg partials of each row's lane group -> the row's S in every lane of the group: xor butterfly, low mask first
__device__ __forceinline__ void butterfly(float (&p)[kStepRows], int G) {
    for (int mask = 1; mask < G; mask <<= 1) {
#pragma unroll
        for (int u = 0; u < kStepRows; ++u) p[u] = __fadd_rn(p[u], __shfl_xor(p[u], mask));
    }
}

// s' = s + S / D and the row's multiplier alpha / (sqrt(s') + eps)
__device__ __forceinline__ float rowwise_mult(float s, float S, int D, float alpha, float eps, float& sn) {
    sn = __fadd_rn(s, S / static_cast<float>(D));
    return alpha / __fadd_rn(sqrtf(sn), eps);
}

template <typename WT, int RULE, bool NT>
__global__ void __launch_bounds__(kBlock) sparse_rows_step_kernel(const StepArgs a) {
    constexpr int ES = static_cast<int>(sizeof(typename AdamW<WT>::raw_t)) / 4;   // bytes per table element
    constexpr bool kState = RULE != kSgd;
    __shared__ int64_t s_prefix[kAdamLdsPrefix];
    __shared__ int64_t s_w[kBlock], s_g[kBlock], s_s[kState ? kBlock : 1];   // the slot's row addresses (s_s: its state row / value)
    __shared__ int32_t s_dim[kBlock];                                        // its width in columns
    __shared__ int32_t s_first, s_last;                                      // the tile's first and last table

    const int tid = static_cast<int>(threadIdx.x);
    const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kBlock;
    const int n = a.U - j0 < kBlock ? static_cast<int>(a.U - j0) : kBlock;   // slots of this tile (>= 1: the grid is ceil(U / kBlock))
    const int64_t j = j0 + tid;

    // 1. the slot's table (sparse_rows_walk.h), its row id and the row addresses (64-bit: rows_t * D_t may exceed 2^31)
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
        const int64_t row = as_global<int64_t>(a.row_ids[t])[k];
        s_w[tid] = reinterpret_cast<int64_t>(a.tables[t]) + row * D * ES;
        if (kState) s_s[tid] = reinterpret_cast<int64_t>(a.state[t] + (RULE == kRowwise ? row : row * D));
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
        // 3. batches of kStepRows rows per lane group: slot run0 + gid + i * NG
        for (int i0 = run0 + gid; i0 < b; i0 += kStepRows * NG) {
            int64_t aw[kStepRows], ag[kStepRows], as[kStepRows];
            int dim[kStepRows];
            bool in_run[kStepRows];
#pragma unroll
            for (int u = 0; u < kStepRows; ++u) {
                const int q = i0 + u * NG;
                in_run[u] = q < b;
                const int qq = in_run[u] ? q : run0;
                dim[u] = s_dim[qq];
                aw[u] = s_w[qq]; ag[u] = s_g[qq]; as[u] = kState ? s_s[qq] : 0;
            }
            int cc[kStepRows];
            bool live[kStepRows];
            if (RULE != kRowwise) {
                for (int pass = 0; pass < passes; ++pass) {
                    const int c = (pass * G + lig) * 4;
#pragma unroll
                    for (int u = 0; u < kStepRows; ++u) {
                        live[u] = in_run[u] && c < dim[u];
                        cc[u] = live[u] ? c : 0;
                    }
                    elementwise_batch<WT, RULE, NT>(aw, ag, as, cc, live, c, sign, a.alpha, a.eps);
                }
            } else if (passes == 1) {
                // rows of one pass: g stays in registers between the reduction and the update
                const int c = lig * 4;
                f32x4 g[kStepRows];
                typename AdamW<WT>::raw_t w[kStepRows];
                float s[kStepRows], p[kStepRows];
#pragma unroll
                for (int u = 0; u < kStepRows; ++u) {
                    live[u] = in_run[u] && c < dim[u];
                    cc[u] = live[u] ? c : 0;
                    g[u] = adam_load4<NT>(ag[u], cc[u]);
                    w[u] = w_load4<WT>(aw[u], cc[u]);
                    s[u] = *reinterpret_cast<const PM_GLOBAL float*>(as[u]);  // one address per lane group: a broadcast
                }
#pragma unroll
                for (int u = 0; u < kStepRows; ++u) p[u] = add_squares(0.0f, g[u], live[u]);
                butterfly(p, G);
#pragma unroll
                for (int u = 0; u < kStepRows; ++u) {
                    float sn, wn[4];
                    const float mult = rowwise_mult(s[u], p[u], dim[u], a.alpha, a.eps, sn);
#pragma unroll
                    for (int k = 0; k < 4; ++k) wn[k] = __fmaf_rn(mult, __fmul_rn(g[u][k], sign), AdamW<WT>::widen(w[u], k));
                    if (live[u]) w_store4<WT>(aw[u], c, wn);
                    if (in_run[u] && lig == 0) *reinterpret_cast<PM_GLOBAL float*>(as[u]) = sn;
                }
            } else {
                // wider rows (G = 64, a lane group is a wave): a sweep for S, a sweep for the update
                float s[kStepRows], p[kStepRows], mult[kStepRows];
#pragma unroll
                for (int u = 0; u < kStepRows; ++u) {
                    s[u] = *reinterpret_cast<const PM_GLOBAL float*>(as[u]);
                    p[u] = 0.0f;
                }
                for (int pass = 0; pass < passes; ++pass) {
                    const int c = (pass * G + lig) * 4;
                    f32x4 g[kStepRows];
#pragma unroll
                    for (int u = 0; u < kStepRows; ++u) {
                        live[u] = in_run[u] && c < dim[u];
                        g[u] = adam_load4<false>(ag[u], live[u] ? c : 0);    // plain: the second sweep reads it again
                    }
#pragma unroll
                    for (int u = 0; u < kStepRows; ++u) p[u] = add_squares(p[u], g[u], live[u]);
                }
                butterfly(p, G);
#pragma unroll
                for (int u = 0; u < kStepRows; ++u) {
                    float sn;
                    mult[u] = rowwise_mult(s[u], p[u], dim[u], a.alpha, a.eps, sn);
                    if (in_run[u] && lig == 0) *reinterpret_cast<PM_GLOBAL float*>(as[u]) = sn;
                }
                for (int pass = 0; pass < passes; ++pass) {
                    const int c = (pass * G + lig) * 4;
                    f32x4 g[kStepRows];
                    typename AdamW<WT>::raw_t w[kStepRows];
#pragma unroll
                    for (int u = 0; u < kStepRows; ++u) {
                        live[u] = in_run[u] && c < dim[u];
                        cc[u] = live[u] ? c : 0;
                        g[u] = adam_load4<NT>(ag[u], cc[u]);
                        w[u] = w_load4<WT>(aw[u], cc[u]);
                    }
#pragma unroll
                    for (int u = 0; u < kStepRows; ++u) {
                        float wn[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) wn[k] = __fmaf_rn(mult[u], __fmul_rn(g[u][k], sign), AdamW<WT>::widen(w[u], k));
                        if (live[u]) w_store4<WT>(aw[u], c, wn);
                    }
                }
            }
        }
    }
}

template <typename WT, int RULE>
hipError_t launch_step_nt(const StepArgs& a, bool nt, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((a.U + kBlock - 1) / kBlock)), block(kBlock);
    if (nt) hipLaunchKernelGGL((sparse_rows_step_kernel<WT, RULE, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((sparse_rows_step_kernel<WT, RULE, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

template <int RULE>
hipError_t launch_step_rule(const StepArgs& a, int table_dtype, bool nt, hipStream_t stream) {
    if (table_dtype == PM_BF16) return launch_step_nt<bf16_t, RULE>(a, nt, stream);
    if (table_dtype == PM_F16) return launch_step_nt<f16_t, RULE>(a, nt, stream);
    return launch_step_nt<float, RULE>(a, nt, stream);
}

}  // namespace

// every array is a device array (see include/param_amd.h); U >= 1, T >= 1, U / kBlock below 2^31: the caller's checks.
// state == nullptr: SGD (eps unused); otherwise Adagrad, row-wise when `rowwise`
hipError_t launch_sparse_rows_step(int T, int64_t U, void* const* tables, int table_dtype, const int64_t* const* row_ids,
                                   const float* const* values, float* const* state, const int32_t* dims, const int64_t* prefix,
                                   float alpha, float eps, bool rowwise, bool maximize, bool nontemporal, hipStream_t stream) {
    StepArgs a;
    a.tables = tables; a.row_ids = row_ids; a.values = values; a.state = state; a.dims = dims; a.prefix = prefix;
    a.U = U; a.T = T;
    a.lds_prefix = T + 1 <= kAdamLdsPrefix ? 1 : 0;
    a.maximize = maximize ? 1 : 0;
    a.alpha = alpha; a.eps = eps;
    if (!state) return launch_step_rule<kSgd>(a, table_dtype, nontemporal, stream);
    if (rowwise) return launch_step_rule<kRowwise>(a, table_dtype, nontemporal, stream);
    return launch_step_rule<kAdagrad>(a, table_dtype, nontemporal, stream);
}

}  // namespace pm
