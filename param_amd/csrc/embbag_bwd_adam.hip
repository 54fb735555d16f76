// param_amd/csrc/embbag_bwd_adam.hip -- lazy Adam / AdamW fused into the deterministic backward of a SUM-pooled forward
// (pm_embbag_bwd_adam, include/param_amd.h: FUSED LAZY ADAM).  The summed gradient of a row never leaves the
// chip: it is added up in registers from the [B, sum D]-sized grad and the row's w, exp_avg and exp_avg_sq are updated by the lane
// group that summed it.  No compact [U, D] gradient, no row ids, no host synchronisation, no shared apply kernel.
//
// Input: the pooled, unweighted key sort of the request (pm_embbag_sort_indices): pairs (key = table << tshift | row, value = bag within
// the table), equal keys adjacent -- a RUN -- and ascending bags inside a run; the pair count is on the device.  A bag that holds a row
// twice is two adjacent pairs of one value and counts TWICE (embbag_max_bwd.hip, the template of this file, skips the repeat).
//
// adam_bwd_kernel (one workgroup per tile of kAbTile sorted pairs):
//   1. the tile's keys and values, and the pair in front of it, go into LDS with coalesced loads;
//   2. a run that crosses into the tile has its start found by one lane (a galloping search backwards through the sorted keys);
//   3. every position is tested: a run HEAD (key != the key in front) or a PIECE START (a multiple of kExactRun pairs behind its run's
//      start) becomes a work item in an LDS list;
//   4. lane groups of G = group_lanes(max_dim, 4) lanes take items in turn; a lane owns four columns per pass of 4 G columns.  An item
//      is at most kExactRun pairs of one run; the group walks on in global memory where the item leaves the tile.  Per pair a lane loads
//      grad (16 / 8 bytes) of the pair's bag at its four columns, kAbInFlight pairs' loads in flight; the adds are ordered, from +0.0;
//   5. a head whose run ends within kExactRun pairs is finished by its group: w (16 / 8 bytes), exp_avg and exp_avg_sq (16 bytes each)
//      are loaded BEFORE the walk, the rule runs in registers, three stores leave.  One row, one owner, no atomics on tables or state.
//      A run of the table's padding row is skipped whole: nothing of it is read or written;
//   6. any other item -- a piece of a HOT run -- leaves its fp32 partial in a workspace slot that its position names, and a hot run's
//      head is appended to a list (the one atomic: a counter that orders nothing the result depends on).
// adam_bwd_combine_kernel (second launch, small): a lane group per listed hot run adds the run's pieces in ascending order and
//   applies the rule.
//
// The association is a function of the request alone: the pieces of a run are cut every kExactRun PAIRS from the run's start, whatever
// the tile size, the grid or the order in which workgroups run.  The per-element arithmetic is sparse_rows_adam.hip's expression
// sequence, repeated here (adam_rule4) so that neither file's code depends on the other's.
#include "common.h"
#include "bwd_sorted_apply.h"      // kExactRun
#include "sparse_rows_walk.h"      // AdamW: widen / pack of the three table types; the 16-byte (non-)temporal accesses

namespace pm {
namespace {

using rows::AdamW;
using fwd::u32x2;
using fwd::bf16_t;
using fwd::f16_t;

constexpr int kAbTile = 1024;                    // sorted pairs per workgroup
constexpr int kAbPerThread = kAbTile / kBlock;
constexpr int kAbInFlight = 4;                   // pairs whose gradient loads a lane keeps in flight
constexpr uint64_t kNoKey = ~static_cast<uint64_t>(0);     // a key has one spare bit: no pair has this key

struct AdamBwdArgs {
    const void* keys;            // sorted keys, uint32 or uint64 (key64)
    const uint32_t* vals;        // bag within the table
    const uint32_t* d_count;     // device: pairs in the sorted arrays
    uint32_t* ctl;               // device: hot runs listed -- a word of this call's own area (adam_bwd_clear_kernel zeroes it), NOT the
                                 // sorted apply's control words: the workspace stays a complete sort that a later apply may consume
    uint32_t* hot;               // first sorted position of every hot run, in no particular order
    float* slots;                // a piece's partial: slot_stride floats
    const void* grad;
    void* const* tables;
    float* const* m;
    float* const* v;
    const int64_t* pad_rows;     // device [T], -1: none; NULL: no table has one
    const int32_t* dims;
    const int64_t* out_offsets;
    int64_t out_stride;
    uint32_t n_max;              // num_indices: the pair count is clamped to it
    int32_t key64, tshift, gshift;
    int64_t slot_stride;
    int32_t decay;               // d != 1: w0 = w * d
    float sign;                  // -1 under maximize
    float c1, c2, eps, s, d;
};

__device__ __forceinline__ uint64_t load_key(const void* keys, uint32_t i, int key64) {
    return key64 ? as_global<uint64_t>(keys)[i] : static_cast<uint64_t>(as_global<uint32_t>(keys)[i]);
}

// slot of the piece that starts at sorted position pos: two pieces that start within one window of kExactRun positions are a later piece
// of one run and the head of the next, never two of a kind
__device__ __forceinline__ int64_t piece_slot(uint32_t pos, bool head) { return static_cast<int64_t>(pos / kExactRun) * 2 + (head ? 1 : 0); }

// GD: the gradient's element, 0 fp32 / 1 bf16 / 2 fp16, widened exactly
template <int GD>
__device__ __forceinline__ f32x4 load_grad4(const void* grad, int64_t elem) {
    if constexpr (GD == 0) {
        return *reinterpret_cast<const PM_GLOBAL f32x4*>(as_global<float>(grad) + elem);
    } else {
        const u32x2 h = *reinterpret_cast<const PM_GLOBAL u32x2*>(as_global<uint16_t>(grad) + elem);
        const uint32_t q[4] = {h[0] & 0xffffu, h[0] >> 16, h[1] & 0xffffu, h[1] >> 16};
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = GD == 1 ? __uint_as_float(q[k] << 16) : static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(q[k])));
        return v;
    }
}

// the row's four columns at element offset `elem` of its table and state: what a finishing lane holds between its loads and its stores
template <typename WT>
struct Row4 {
    typename AdamW<WT>::raw_t w;
    f32x4 m, v;
};

template <typename WT, bool NT>
__device__ __forceinline__ Row4<WT> load_row4(const AdamBwdArgs& a, int t, int64_t elem) {
    constexpr int ES = static_cast<int>(sizeof(typename AdamW<WT>::raw_t)) / 4;      // bytes per table element
    Row4<WT> r;
    r.w = rows::w_load4<WT>(reinterpret_cast<int64_t>(a.tables[t]) + elem * ES, 0);
    r.m = rows::adam_load4<NT>(reinterpret_cast<int64_t>(a.m[t] + elem), 0);
    r.v = rows::adam_load4<NT>(reinterpret_cast<int64_t>(a.v[t] + elem), 0);
    return r;
}

// The rule on four columns (include/param_amd.h, SPARSE-ROW ADAM): every operation one fp32 rounding, nothing contracted, sqrt and the
// division correctly rounded -- sparse_rows_adam.hip's expression sequence -- and the three stores.
template <typename WT, bool NT>
__device__ __forceinline__ void adam_rule4(const AdamBwdArgs& a, int t, int64_t elem, const Row4<WT>& r, const f32x4& G) {
    constexpr int ES = static_cast<int>(sizeof(typename AdamW<WT>::raw_t)) / 4;
    float wn[4];
    f32x4 mn, vn;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gk = __fmul_rn(G[k], a.sign);                // exact: -g under maximize
        const float wk = AdamW<WT>::widen(r.w, k);
        const float w0 = a.decay ? __fmul_rn(wk, a.d) : wk;
        mn[k] = __fadd_rn(r.m[k], __fmul_rn(__fsub_rn(gk, r.m[k]), a.c1));
        vn[k] = __fadd_rn(r.v[k], __fmul_rn(__fsub_rn(__fmul_rn(gk, gk), r.v[k]), a.c2));
        const float q = mn[k] / __fadd_rn(sqrtf(vn[k]), a.eps);  // correctly rounded sqrt and division
        wn[k] = __fsub_rn(w0, __fmul_rn(a.s, q));
    }
    rows::adam_store4<NT>(reinterpret_cast<int64_t>(a.m[t] + elem), 0, mn);
    rows::adam_store4<NT>(reinterpret_cast<int64_t>(a.v[t] + elem), 0, vn);
    rows::w_store4<WT>(reinterpret_cast<int64_t>(a.tables[t]) + elem * ES, 0, wn);
}

// the workgroup's view of the sorted pairs: its tile (and the pair in front) from LDS, everything else from global memory
struct PairView {
    const uint64_t* s_key;       // s_key[0] = the key at t0 - 1 (kNoKey in front of the first pair), s_key[1 + i] = the key at t0 + i
    const uint32_t* s_val;       // likewise
    const void* keys;
    const uint32_t* vals;
    uint32_t t0, len;
    int key64;
    __device__ __forceinline__ bool staged(uint32_t pos) const { return pos + 1 >= t0 && pos < t0 + len; }
    __device__ __forceinline__ uint64_t key(uint32_t pos) const { return staged(pos) ? s_key[pos + 1 - t0] : load_key(keys, pos, key64); }
    __device__ __forceinline__ uint32_t val(uint32_t pos) const { return staged(pos) ? s_val[pos + 1 - t0] : as_global<uint32_t>(vals)[pos]; }
};

// first position of the run that holds position `eq` (key0 = its key): gallop backwards, then bisect.  Equal keys are adjacent, so
// "has key0" is monotone on [0, eq].
__device__ __forceinline__ uint32_t run_start(const void* keys, int key64, uint32_t eq, uint64_t key0) {
    uint32_t step = 1, ne = 0;
    for (;;) {
        if (eq < step) {
            if (eq == 0 || load_key(keys, 0, key64) == key0) return 0;
            ne = 0;
            break;
        }
        const uint32_t probe = eq - step;
        if (load_key(keys, probe, key64) != key0) {
            ne = probe;
            break;
        }
        eq = probe;
        step = step < 0x40000000u ? step * 2 : step;
    }
    while (eq - ne > 1) {
        const uint32_t mid = ne + (eq - ne) / 2;
        if (load_key(keys, mid, key64) == key0) eq = mid; else ne = mid;
    }
    return eq;
}

template <typename WT, int GD, bool NT>
__global__ void __launch_bounds__(kBlock) adam_bwd_kernel(const AdamBwdArgs a) {
    __shared__ uint64_t s_key[kAbTile + 1];
    __shared__ uint32_t s_val[kAbTile + 1];
    __shared__ uint32_t s_item[kAbTile];
    __shared__ uint32_t s_nitem, s_cross;
    const uint32_t n_dev = *a.d_count;
    const uint32_t n = n_dev < a.n_max ? n_dev : a.n_max;
    const uint64_t t0_64 = static_cast<uint64_t>(blockIdx.x) * kAbTile;
    if (t0_64 >= n) return;
    const uint32_t t0 = static_cast<uint32_t>(t0_64);
    const uint32_t len = n - t0 < static_cast<uint32_t>(kAbTile) ? n - t0 : kAbTile;
    const int tid = static_cast<int>(threadIdx.x);

    // 1. the tile and the pair in front of it
    for (uint32_t i = tid; i < len; i += kBlock) {
        s_key[1 + i] = load_key(a.keys, t0 + i, a.key64);
        s_val[1 + i] = as_global<uint32_t>(a.vals)[t0 + i];
    }
    if (tid == 0) {
        s_key[0] = t0 > 0 ? load_key(a.keys, t0 - 1, a.key64) : kNoKey;
        s_val[0] = t0 > 0 ? as_global<uint32_t>(a.vals)[t0 - 1] : 0u;
        s_nitem = 0;
    }
    __syncthreads();
    // 2. where the run that crosses into the tile starts
    if (tid == 0) s_cross = s_key[0] == s_key[1] ? run_start(a.keys, a.key64, t0 - 1, s_key[1]) : t0;
    __syncthreads();
    // 3. heads and piece starts
    const bool crossing = s_key[0] == s_key[1];
    const uint32_t cross_start = s_cross;
#pragma unroll
    for (int u = 0; u < kAbPerThread; ++u) {
        const uint32_t i = static_cast<uint32_t>(u) * kBlock + tid;
        if (i >= len) break;
        const uint64_t ki = s_key[1 + i];
        const bool head = ki != s_key[i];
        bool item = head;
        if (!head) {
            if (crossing && ki == s_key[1]) {
                item = (t0 + i - cross_start) % kExactRun == 0;
            } else {
                // the run's head is in the tile: kExactRun-steps back while the key stays
                for (uint32_t q = i; q >= static_cast<uint32_t>(kExactRun) && s_key[1 + q - kExactRun] == ki;) {
                    q -= kExactRun;
                    if (s_key[1 + q] != s_key[q]) {
                        item = true;
                        break;
                    }
                }
            }
        }
        if (item) s_item[atomicAdd(&s_nitem, 1u)] = i | (head ? 0x80000000u : 0u);
    }
    __syncthreads();

    // 4. lane groups take items
    const PairView pv{s_key, s_val, a.keys, a.vals, t0, len, a.key64};
    const int G = 1 << a.gshift;
    const int lig = tid & (G - 1);
    const uint32_t nitem = s_nitem;
    const uint64_t rmask = (static_cast<uint64_t>(1) << a.tshift) - 1;
    for (uint32_t it = static_cast<uint32_t>(tid >> a.gshift); it < nitem; it += static_cast<uint32_t>(kBlock >> a.gshift)) {
        const uint32_t w = s_item[it];
        const bool head = (w & 0x80000000u) != 0;
        const uint32_t gp = t0 + (w & 0x7fffffffu);
        const uint64_t key0 = pv.key(gp);
        const int t = static_cast<int>(key0 >> a.tshift);
        const int64_t row = static_cast<int64_t>(key0 & rmask);
        if (a.pad_rows && a.pad_rows[t] == row) continue;      // the padding row: its run is skipped, head and pieces alike
        uint32_t cnt = 1;
        const uint32_t room = n - gp;      // pairs from gp to the end of the sorted arrays (at least one)
        while (cnt < static_cast<uint32_t>(kExactRun) && cnt < room && pv.key(gp + cnt) == key0) ++cnt;
        const bool more = cnt == static_cast<uint32_t>(kExactRun) && cnt < room && pv.key(gp + cnt) == key0;
        const bool piece = !head || more;      // part of a hot run
        const int D = a.dims[t];
        const int64_t goff = a.out_offsets[t];
        const uint32_t b_first = pv.val(gp);
        if (piece && head && lig == 0) a.hot[atomicAdd(a.ctl, 1u)] = gp;
        for (int c4 = lig; c4 < D / 4; c4 += G) {
            const int64_t elem = row * D + c4 * 4;
            Row4<WT> r{};
            if (!piece) r = load_row4<WT, NT>(a, t, elem);      // in flight during the walk
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (uint32_t j0 = 0; j0 < cnt; j0 += kAbInFlight) {
                f32x4 gv[kAbInFlight];
#pragma unroll
                for (int u = 0; u < kAbInFlight; ++u) {
                    const uint32_t b = j0 + u < cnt ? pv.val(gp + j0 + u) : b_first;      // (past the item: a bag that exists, its load unused)
                    gv[u] = load_grad4<GD>(a.grad, goff + static_cast<int64_t>(b) * a.out_stride + c4 * 4);
                }
#pragma unroll
                for (int u = 0; u < kAbInFlight; ++u) {
                    const bool live = j0 + u < cnt;
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = live ? __fadd_rn(acc[k], gv[u][k]) : acc[k];
                }
            }
            if (!piece) {
                adam_rule4<WT, NT>(a, t, elem, r, acc);
            } else {
                PM_GLOBAL float* s = as_global<float>(a.slots) + piece_slot(gp, head) * a.slot_stride;
                *reinterpret_cast<PM_GLOBAL f32x4*>(s + c4 * 4) = acc;
            }
        }
    }
}

// a lane group per listed hot run: its pieces in ascending order, then the rule
template <typename WT, bool NT>
__global__ void __launch_bounds__(kBlock) adam_bwd_combine_kernel(const AdamBwdArgs a) {
    const uint32_t n_dev = *a.d_count;
    const uint32_t n = n_dev < a.n_max ? n_dev : a.n_max;
    const uint32_t nhot = *a.ctl;
    const int G = 1 << a.gshift;
    const int lig = static_cast<int>(threadIdx.x) & (G - 1);
    const uint64_t rmask = (static_cast<uint64_t>(1) << a.tshift) - 1;
    const uint32_t groups = gridDim.x * static_cast<uint32_t>(kBlock >> a.gshift);
    for (uint32_t h = blockIdx.x * static_cast<uint32_t>(kBlock >> a.gshift) + (threadIdx.x >> a.gshift); h < nhot; h += groups) {
        const uint32_t s0 = a.hot[h];
        const uint64_t key0 = load_key(a.keys, s0, a.key64);
        const int t = static_cast<int>(key0 >> a.tshift);
        const int64_t row = static_cast<int64_t>(key0 & rmask);
        const int D = a.dims[t];
        for (int c4 = lig; c4 < D / 4; c4 += G) {
            const int64_t elem = row * D + c4 * 4;
            const Row4<WT> r = load_row4<WT, NT>(a, t, elem);
            // the head's piece, then the later ones: a hot run has at least two
            f32x4 sum = *reinterpret_cast<const PM_GLOBAL f32x4*>(as_global<float>(a.slots) + piece_slot(s0, true) * a.slot_stride + c4 * 4);
            for (uint64_t pos = static_cast<uint64_t>(s0) + kExactRun;
                 pos < n && load_key(a.keys, static_cast<uint32_t>(pos), a.key64) == key0; pos += kExactRun) {
                const PM_GLOBAL float* s = as_global<float>(a.slots) + piece_slot(static_cast<uint32_t>(pos), false) * a.slot_stride;
                const f32x4 part = *reinterpret_cast<const PM_GLOBAL f32x4*>(s + c4 * 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) sum[k] = __fadd_rn(sum[k], part[k]);
            }
            adam_rule4<WT, NT>(a, t, elem, r, sum);
        }
    }
}

// the hot-run counter starts every call at zero (a kernel, not a memset: the call may be captured into a graph)
__global__ void adam_bwd_clear_kernel(uint32_t* ctl) { *ctl = 0; }

template <typename WT, bool NT>
hipError_t launch_wt(const AdamBwdArgs& a, int grad_dtype, unsigned grid, unsigned combine_grid, hipStream_t stream) {
    const dim3 blk(kBlock);
    hipLaunchKernelGGL(adam_bwd_clear_kernel, dim3(1), dim3(1), 0, stream, a.ctl);
    if (grad_dtype == PM_F32) hipLaunchKernelGGL((adam_bwd_kernel<WT, 0, NT>), dim3(grid), blk, 0, stream, a);
    else if (grad_dtype == PM_BF16) hipLaunchKernelGGL((adam_bwd_kernel<WT, 1, NT>), dim3(grid), blk, 0, stream, a);
    else hipLaunchKernelGGL((adam_bwd_kernel<WT, 2, NT>), dim3(grid), blk, 0, stream, a);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess || combine_grid == 0) return rc;
    hipLaunchKernelGGL((adam_bwd_combine_kernel<WT, NT>), dim3(combine_grid), blk, 0, stream, a);
    return hipGetLastError();
}

template <typename WT>
hipError_t launch_nt(const AdamBwdArgs& a, bool nt, int grad_dtype, unsigned grid, unsigned combine_grid, hipStream_t stream) {
    return nt ? launch_wt<WT, true>(a, grad_dtype, grid, combine_grid, stream) : launch_wt<WT, false>(a, grad_dtype, grid, combine_grid, stream);
}

size_t a256(size_t x) { return (x + 255) / 256 * 256; }
size_t hot_list_bytes(int64_t n) { return a256(4 * (static_cast<size_t>(n) / kExactRun + 2)); }      // the counter, then the list

}  // namespace

// behind the sorted backward's workspace: the hot-run counter and list, then two fp32 slots of max_dim columns per kExactRun sorted positions
size_t adam_bwd_extra_bytes(int64_t n, int max_dim) {
    return hot_list_bytes(n) + a256(2 * (static_cast<size_t>(n) / kExactRun + 1) * static_cast<size_t>(max_dim) * 4);
}

// p: base parameters of the request; mp: the sorted pairs of the request's sort; extra: adam_bwd_extra_bytes
hipError_t launch_adam_bwd(const KParams& p, int max_dim, const MaxBwdPairs& mp, void* extra, const void* grad, int grad_dtype,
                           void* const* tables, int table_dtype, float* const* m, float* const* v, const int64_t* pad_rows,
                           const pm_sparse_adam* opt, hipStream_t stream) {
    const int G = group_lanes(max_dim, 4);
    AdamBwdArgs a;
    a.keys = mp.keys;
    a.vals = mp.vals;
    a.d_count = mp.d_count;
    a.ctl = static_cast<uint32_t*>(extra);
    a.hot = a.ctl + 1;
    a.slots = reinterpret_cast<float*>(static_cast<char*>(extra) + hot_list_bytes(p.N));
    a.grad = grad;
    a.tables = tables;
    a.m = m;
    a.v = v;
    a.pad_rows = pad_rows;
    a.dims = p.dims;
    a.out_offsets = p.out_offsets;
    a.out_stride = p.out_stride;
    a.n_max = static_cast<uint32_t>(p.N);
    a.key64 = mp.key_bytes == 8 ? 1 : 0;
    a.tshift = mp.tshift;
    a.gshift = 3;
    while ((1 << a.gshift) < G) ++a.gshift;
    a.slot_stride = max_dim;
    a.decay = opt->decay != 1.0f ? 1 : 0;      // w * 1 is w: skipping the product changes no bit
    a.sign = opt->maximize ? -1.0f : 1.0f;
    a.c1 = opt->c1; a.c2 = opt->c2; a.eps = opt->eps; a.s = opt->step_size; a.d = opt->decay;
    const int64_t grid = (p.N + kAbTile - 1) / kAbTile;
    if (grid < 1 || grid > kMaxGrid) return hipErrorInvalidConfiguration;
    // a hot run has more than kExactRun pairs: none in a request of at most that many, else a group per possible run up to 1024 workgroups
    const int64_t max_hot = p.N / (kExactRun + 1);
    const int64_t per_block = kBlock >> a.gshift;
    int64_t cgrid = (max_hot + per_block - 1) / per_block;
    if (cgrid > 1024) cgrid = 1024;
    const unsigned g = static_cast<unsigned>(grid), cg = static_cast<unsigned>(cgrid);
    const bool nt = opt->nontemporal != 0;
    if (table_dtype == PM_BF16) return launch_nt<bf16_t>(a, nt, grad_dtype, g, cg, stream);
    if (table_dtype == PM_F16) return launch_nt<f16_t>(a, nt, grad_dtype, g, cg, stream);
    return launch_nt<float>(a, nt, grad_dtype, g, cg, stream);
}

}  // namespace pm
