// param_amd/csrc/sparse_grad.hip -- the coalesced sparse gradient of a batched EmbeddingBag (ABI v8): for every table t the
// distinct rows its lookups hit, ascending, and one fp32 gradient row per distinct row,
//     values_t[k] = sum over lookups j with idx_j = rows_t[k] of psw[j] * grad(t, bag(j))
// -- what torch's EmbeddingBag(sparse=True) backward followed by .coalesce() gives (the autograd backward of the reference's
// dlrm.py:1290-1296 through the tables pytorch_dist_backend.py:924 builds), without a scatter into a table-sized buffer.
//
// It reuses the sorted backward instead of duplicating it:
//   1. pm_embbag_sort_indices (the complete one-phase key sort, seg_sort.hip): keys (t << tshift) | row, table-major, ascending
//      rows within a table, equal keys adjacent and in lookup order;
//   2. pm_embbag_sparse_grad_count: ONE streaming pass over the sorted pairs flags run heads, scans them per table (reduce-then-
//      scan: per-tile counts, one workgroup per table scans its tiles' counts, the tiles relabel -- kernel boundaries as the only
//      synchronisation) and rewrites every key in place to (t << tshift) | slot, slot = the run's index within its table.  The
//      relabelling is monotone and slot < U_t <= rows_t, so the sorted order, the runs and the apply's chunking are unchanged;
//   3. pm_embbag_sparse_grad: the row ids go out, the compact [U_t, D_t] value rows are zeroed, and the UNCHANGED sorted apply
//      (fp32 destination, alpha = 1) sums every run into values_t + slot * D_t -- bit for bit what it writes into row `row` of a
//      zeroed fp32 table.
//
// Kernels (gfx950), all over per-table tiles of kSgTile sorted positions (a tile never spans two tables):
//   sg_plan_kernel     one workgroup: tiles per table from the sort's segment descriptors, their exclusive scan
//   sg_count_kernel    a tile: run heads (key != previous key, or the table's first pair) -> count | first-is-head flag
//   sg_scan_kernel     a table: exclusive scan of its tiles' counts (the tile's first slot), U_t
//   sg_relabel_kernel  a tile: slot of every pair, row id of every run kept in the workspace, keys rewritten
//   sg_rows_kernel     a tile (apply call): row ids of its runs to the caller's arrays, its runs' value rows zeroed
#include "common.h"

namespace pm {
namespace {

constexpr int kSgThreads = 256;
constexpr int kSgItems = 8;                        // sorted positions per thread
constexpr int kSgTile = kSgThreads * kSgItems;     // 2048 per workgroup
constexpr uint32_t kHeadBit = 0x80000000u;         // in a tile's count / base word: the tile's first pair starts a run

__device__ __forceinline__ uint32_t sg_block_excl_scan(uint32_t v, uint32_t* s_tmp, uint32_t* total) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += up;
    }
    if (lane == kWave - 1) s_tmp[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int w = 0; w < static_cast<int>(blockDim.x) / kWave; ++w) {
        if (w < wave) base += s_tmp[w];
        all += s_tmp[w];
    }
    __syncthreads();
    if (total) *total = all;
    return base + incl - v;
}

// table of tile g: the last t with tstart[t] <= g (tables without pairs have no tiles: equal neighbouring starts)
__device__ __forceinline__ int sg_table_of(const uint32_t* tstart, int T, uint32_t g) {
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tstart[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

struct SgTile {
    int t;
    uint32_t i0;     // first sorted position of the tile
    uint32_t len;    // positions in the tile
    bool first;      // the tile is its table's first
};

__device__ __forceinline__ bool sg_tile(const SegDesc* desc, const uint32_t* tstart, int T, uint32_t g, SgTile& tl) {
    if (g >= tstart[T]) return false;
    tl.t = sg_table_of(tstart, T, g);
    const uint32_t k = g - tstart[tl.t];
    const uint32_t cnt = desc[tl.t].count;
    tl.i0 = desc[tl.t].out_start + k * kSgTile;
    tl.len = cnt - k * kSgTile < static_cast<uint32_t>(kSgTile) ? cnt - k * kSgTile : kSgTile;
    tl.first = k == 0;
    return true;
}

// the tile's keys into LDS, coalesced: s_key[0] = the key before the tile (unused for a table's first tile), s_key[1 + k] = key i0 + k
template <typename K>
__device__ __forceinline__ void sg_stage(const K* keys, const SgTile& tl, bool want_prev, K* s_key) {
    for (uint32_t k = threadIdx.x; k < tl.len; k += kSgThreads) s_key[1 + k] = keys[tl.i0 + k];
    if (threadIdx.x == 0) s_key[0] = (want_prev && !tl.first) ? keys[tl.i0 - 1] : static_cast<K>(0);
    __syncthreads();
}

// one workgroup of 1024 threads (T <= kSegSortMaxTables): tstart[t] = first tile of table t, tstart[T] = tiles in all
__global__ void __launch_bounds__(1024) sg_plan_kernel(const SegDesc* desc, int T, uint32_t* tstart) {
    __shared__ uint32_t s_tmp[1024 / kWave];
    const int t = threadIdx.x;
    const uint32_t n = t < T ? (desc[t].count + kSgTile - 1) / kSgTile : 0;
    uint32_t total = 0;
    const uint32_t base = sg_block_excl_scan(n, s_tmp, &total);
    if (t < T) tstart[t] = base;
    if (t == 0) tstart[T] = total;
}

template <typename K>
__global__ void __launch_bounds__(kSgThreads) sg_count_kernel(const K* keys, const SegDesc* desc, const uint32_t* tstart, int T,
                                                              uint32_t* tcnt) {
    __shared__ K s_key[kSgTile + 1];
    __shared__ uint32_t s_tmp[kSgThreads / kWave];
    SgTile tl;
    if (!sg_tile(desc, tstart, T, blockIdx.x, tl)) return;
    sg_stage(keys, tl, true, s_key);
    uint32_t heads = 0;
    const uint32_t k0 = threadIdx.x * kSgItems;
#pragma unroll
    for (int u = 0; u < kSgItems; ++u) {
        const uint32_t k = k0 + u;
        if (k < tl.len) heads += ((k == 0 && tl.first) || s_key[k] != s_key[k + 1]) ? 1u : 0u;
    }
    uint32_t total = 0;
    sg_block_excl_scan(heads, s_tmp, &total);
    if (threadIdx.x == 0) {
        const bool lead = tl.first || s_key[0] != s_key[1];
        tcnt[blockIdx.x] = total | (lead ? kHeadBit : 0u);
    }
}

// grid T: table t's tiles [tstart[t], tstart[t + 1]) get the exclusive prefix of their counts (their first slot), flag kept
__global__ void __launch_bounds__(kSgThreads) sg_scan_kernel(const uint32_t* tstart, uint32_t* tcnt, int64_t* unique_counts) {
    __shared__ uint32_t s_tmp[kSgThreads / kWave];
    const int t = blockIdx.x;
    const uint32_t g0 = tstart[t], g1 = tstart[t + 1];
    uint32_t carry = 0;
    for (uint32_t c = g0; c < g1; c += kSgThreads) {
        const uint32_t g = c + threadIdx.x;
        const uint32_t w = g < g1 ? tcnt[g] : 0u;
        uint32_t total = 0;
        const uint32_t base = sg_block_excl_scan(w & ~kHeadBit, s_tmp, &total);
        if (g < g1) tcnt[g] = (carry + base) | (w & kHeadBit);
        carry += total;
    }
    if (threadIdx.x == 0) unique_counts[t] = static_cast<int64_t>(carry);
}

template <typename K>
__global__ void __launch_bounds__(kSgThreads) sg_relabel_kernel(K* keys, const SegDesc* desc, const uint32_t* tstart, int T,
                                                                const uint32_t* tbase, int tshift, uint32_t* run_rows) {
    __shared__ K s_key[kSgTile + 1];
    __shared__ uint32_t s_tmp[kSgThreads / kWave];
    SgTile tl;
    if (!sg_tile(desc, tstart, T, blockIdx.x, tl)) return;
    // (the key before the tile is not read: the workgroup of the previous tile may have relabelled it already -- whether this
    // tile's first pair starts a run is in its base word, from the count pass)
    sg_stage(keys, tl, false, s_key);
    const uint32_t w = tbase[blockIdx.x];
    const uint32_t base = w & ~kHeadBit;
    const bool lead = (w & kHeadBit) != 0;
    const uint32_t k0 = threadIdx.x * kSgItems;
    bool head[kSgItems];
    uint32_t heads = 0;
#pragma unroll
    for (int u = 0; u < kSgItems; ++u) {
        const uint32_t k = k0 + u;
        head[u] = k < tl.len && (k == 0 ? lead : s_key[k] != s_key[k + 1]);
        heads += head[u] ? 1u : 0u;
    }
    uint32_t run = base + sg_block_excl_scan(heads, s_tmp, nullptr);     // runs begun before this thread's first position
    const K tkey = static_cast<K>(tl.t) << tshift;
    const K rmask = (static_cast<K>(1) << tshift) - 1;
#pragma unroll
    for (int u = 0; u < kSgItems; ++u) {
        const uint32_t k = k0 + u;
        if (k >= tl.len) break;
        if (head[u]) {
            run_rows[tl.i0 + k] = static_cast<uint32_t>(s_key[k + 1] & rmask);
            ++run;
        }
        keys[tl.i0 + k] = tkey | static_cast<K>(run - 1);    // (a tile that continues a run: run = base, slot base - 1)
    }
}

// apply call: a tile's runs are the slots [base, base + heads) of its table -- their row ids leave, their value rows are zeroed
template <typename K>
__global__ void __launch_bounds__(kSgThreads) sg_rows_kernel(const K* keys, const SegDesc* desc, const uint32_t* tstart, int T,
                                                             const uint32_t* tbase, const int32_t* dims, int tshift,
                                                             const uint32_t* run_rows, int64_t* const* row_ids, float* const* values) {
    __shared__ K s_key[kSgTile + 1];
    __shared__ uint32_t s_tmp[kSgThreads / kWave];
    SgTile tl;
    if (!sg_tile(desc, tstart, T, blockIdx.x, tl)) return;
    sg_stage(keys, tl, false, s_key);
    const uint32_t w = tbase[blockIdx.x];
    const uint32_t base = w & ~kHeadBit;
    const bool lead = (w & kHeadBit) != 0;
    const K rmask = (static_cast<K>(1) << tshift) - 1;
    PM_GLOBAL int64_t* rid = as_global<int64_t>(row_ids[tl.t]);
    const uint32_t k0 = threadIdx.x * kSgItems;
    uint32_t heads = 0;
#pragma unroll
    for (int u = 0; u < kSgItems; ++u) {
        const uint32_t k = k0 + u;
        if (k < tl.len && (k == 0 ? lead : s_key[k] != s_key[k + 1])) {
            rid[static_cast<uint32_t>(s_key[k + 1] & rmask)] = static_cast<int64_t>(run_rows[tl.i0 + k]);
            ++heads;
        }
    }
    uint32_t total = 0;
    sg_block_excl_scan(heads, s_tmp, &total);
    // zero the tile's value rows: one contiguous range of total * D floats (D a multiple of 4, rows 16-byte aligned)
    const int64_t D = dims[tl.t];
    PM_GLOBAL f32x4* v = reinterpret_cast<PM_GLOBAL f32x4*>(as_global<float>(values[tl.t]) + static_cast<int64_t>(base) * D);
    const int64_t n4 = static_cast<int64_t>(total) * D / 4;
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t i = threadIdx.x; i < n4; i += kSgThreads) v[i] = z;
}

}  // namespace

size_t sparse_grad_extra_bytes(int64_t n, int T) {
    auto a256 = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t tiles = static_cast<size_t>(sparse_grad_max_tiles(n, T));
    return a256(4 * (static_cast<size_t>(T) + 1)) + a256(4 * tiles) + a256(4 * static_cast<size_t>(n));
}

int64_t sparse_grad_max_tiles(int64_t n, int T) {
    // a table of c > 0 pairs has ceil(c / kSgTile) <= c / kSgTile + 1 tiles
    const int64_t nonempty = n < T ? n : T;
    return n / kSgTile + nonempty;
}

namespace {
struct SgExtra {
    uint32_t* tstart;
    uint32_t* tcnt;
    uint32_t* run_rows;
};
SgExtra sg_extra(void* extra, int64_t n, int T) {
    auto a256 = [](size_t x) { return (x + 255) / 256 * 256; };
    char* p = static_cast<char*>(extra);
    SgExtra e;
    e.tstart = reinterpret_cast<uint32_t*>(p);
    p += a256(4 * (static_cast<size_t>(T) + 1));
    e.tcnt = reinterpret_cast<uint32_t*>(p);
    p += a256(4 * static_cast<size_t>(sparse_grad_max_tiles(n, T)));
    e.run_rows = reinterpret_cast<uint32_t*>(p);
    return e;
}
}  // namespace

hipError_t sparse_grad_count(const SparsePairs& sp, int T, int64_t n, void* extra, int64_t* unique_counts, hipStream_t stream) {
    const SgExtra e = sg_extra(extra, n, T);
    const int64_t grid = sparse_grad_max_tiles(n, T);
    if (T < 1 || T > kSegSortMaxTables || grid < 1 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sg_plan_kernel, dim3(1), dim3(1024), 0, stream, sp.desc, T, e.tstart);
    if (sp.key_bytes == 4)
        hipLaunchKernelGGL(sg_count_kernel<uint32_t>, dim3(static_cast<unsigned>(grid)), dim3(kSgThreads), 0, stream,
                           static_cast<const uint32_t*>(sp.keys), sp.desc, e.tstart, T, e.tcnt);
    else
        hipLaunchKernelGGL(sg_count_kernel<uint64_t>, dim3(static_cast<unsigned>(grid)), dim3(kSgThreads), 0, stream,
                           static_cast<const uint64_t*>(sp.keys), sp.desc, e.tstart, T, e.tcnt);
    hipLaunchKernelGGL(sg_scan_kernel, dim3(T), dim3(kSgThreads), 0, stream, e.tstart, e.tcnt, unique_counts);
    if (sp.key_bytes == 4)
        hipLaunchKernelGGL(sg_relabel_kernel<uint32_t>, dim3(static_cast<unsigned>(grid)), dim3(kSgThreads), 0, stream,
                           static_cast<uint32_t*>(sp.keys), sp.desc, e.tstart, T, e.tcnt, sp.tshift, e.run_rows);
    else
        hipLaunchKernelGGL(sg_relabel_kernel<uint64_t>, dim3(static_cast<unsigned>(grid)), dim3(kSgThreads), 0, stream,
                           static_cast<uint64_t*>(sp.keys), sp.desc, e.tstart, T, e.tcnt, sp.tshift, e.run_rows);
    return hipGetLastError();
}

hipError_t sparse_grad_rows(const SparsePairs& sp, int T, int64_t n, const void* extra, const int32_t* dims, int64_t* const* row_ids,
                            float* const* values, hipStream_t stream) {
    const SgExtra e = sg_extra(const_cast<void*>(extra), n, T);
    const int64_t grid = sparse_grad_max_tiles(n, T);
    if (T < 1 || T > kSegSortMaxTables || grid < 1 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
    if (sp.key_bytes == 4)
        hipLaunchKernelGGL(sg_rows_kernel<uint32_t>, dim3(static_cast<unsigned>(grid)), dim3(kSgThreads), 0, stream,
                           static_cast<const uint32_t*>(sp.keys), sp.desc, e.tstart, T, e.tcnt, dims, sp.tshift, e.run_rows, row_ids, values);
    else
        hipLaunchKernelGGL(sg_rows_kernel<uint64_t>, dim3(static_cast<unsigned>(grid)), dim3(kSgThreads), 0, stream,
                           static_cast<const uint64_t*>(sp.keys), sp.desc, e.tstart, T, e.tcnt, dims, sp.tshift, e.run_rows, row_ids, values);
    return hipGetLastError();
}

}  // namespace pm
