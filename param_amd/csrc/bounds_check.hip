// param_amd/csrc/bounds_check.hip -- repair (or count) out-of-range indices and broken offsets of a batched EmbeddingBag request
// on the device, in front of the lookup kernels, which do not check (pm_embbag_bounds_check; rule: include/param_amd.h).
// Stands in for fbgemm's bounds_check_indices kernel (bounds_check_mode of SplitTableBatchedEmbeddingBagsCodegen).
//
// The rule in short: o'[0] = 0, o'[k] = max(o'[k - 1], clamp(offsets[k], 0, N)) -- a clamp and an inclusive prefix maximum, the
// monotone closure --; lookup j belongs to the last table t with o'[t * B] <= j; an index outside [0, rows[t]) becomes 0.
//
// Four launches on one stream, none of which waits for another workgroup inside a launch (no flags, no look-back, no polling):
//   1  bounds_partial_kernel   one workgroup per PM_BOUNDS_OFFSETS_PER_WG offsets: clamp, maximum -> partials[w]; resets the report
//   2  bounds_scan_kernel      ONE workgroup: exclusive prefix maximum of the partials in place (walks them 256 at a time)
//   3  bounds_apply_kernel     the workgroups of 1 again: prefix maximum inside the workgroup on top of partials[w], changed
//                              entries written (repairing modes) and counted; the repaired table borders o'[t * B] (and N behind
//                              them) go to the scratch -- the dry run needs them too, and finds them there
//   4  bounds_indices_kernel   one coalesced stream over the indices: 16-byte loads over the aligned body (the pointer is
//                              element-aligned only: a scalar head and tail), a workgroup per contiguous chunk.  The chunk's table
//                              range comes from two binary searches over the borders; ONE table (the usual case: a table's
//                              lookups are many chunks long) needs nothing else, a range of up to kBoundsTablesLds tables is
//                              staged in LDS and searched there per vector, a longer one (more than 1024 tables) in global memory.
//                              A table border inside a vector: every element walks on from its predecessor's table.
// An offset is never used as an address before it is clamped, and the indices are read inside [0, N) only: safe on arbitrary
// contents of both arrays.  Counts are reduced per wave and per workgroup before ONE atomic add per workgroup; the first
// positions are 64-bit atomic minima: every field of the report is deterministic.  Memory is written only where a value changes.
#include <type_traits>

#include "common.h"

namespace pm {
namespace {

constexpr int kOffPerThread = PM_BOUNDS_OFFSETS_PER_WG / kBlock;
static_assert(kOffPerThread * kBlock == PM_BOUNDS_OFFSETS_PER_WG, "a thread owns a whole number of consecutive offsets");
constexpr int kWaves = kBlock / kWave;
constexpr int kBoundsTablesLds = 1024;      // table borders + rows of a chunk's table range staged in LDS (16 KB)
constexpr int kIdxVecPerWg = 16 * kBlock;   // 16-byte vectors per workgroup of the index pass: 64 KB of indices
constexpr int kIdxUnroll = 4;               // vector loads in flight per thread
constexpr unsigned long long kNone = static_cast<unsigned long long>(PM_BOUNDS_NONE);

struct BoundsArgs {
    void* indices;
    void* offsets;
    const int64_t* rows;
    unsigned long long* report;   // [4] bad_indices, bad_offsets, first_bad_index, first_bad_offset; NULL: no report
    int64_t* partials;            // [ceil(TB / PM_BOUNDS_OFFSETS_PER_WG)]
    int64_t* borders;             // [T + 1]: o'[t * B], then N
    int64_t TB, B, N;
    int32_t T;
    int32_t idx64;
    int32_t write;                // repairing mode
    int32_t has_last;             // offsets has a TB-th entry, which becomes N
};

__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// clamp(offsets[k], 0, N); entry 0 counts as 0 whatever it holds
__device__ __forceinline__ int64_t clamped(const BoundsArgs& a, int64_t k, int64_t raw) {
    if (k == 0) return 0;
    return raw < 0 ? 0 : (raw > a.N ? a.N : raw);
}

__device__ __forceinline__ void store_index(void* p, int64_t i, int64_t v, int idx64) {
    if (idx64) as_global<int64_t>(p)[i] = v;
    else as_global<int32_t>(p)[i] = static_cast<int32_t>(v);
}

// inclusive prefix maximum over the lanes of a wave (values >= 0: the neutral element is 0)
__device__ __forceinline__ int64_t wave_scan_max(int64_t v) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int64_t o = __shfl_up(v, d, kWave);
        if (lane >= d) v = max64(v, o);
    }
    return v;
}

// the workgroup's count and first position -> one atomic each (threads without a finding pass 0 / kNone)
__device__ __forceinline__ void report_add(unsigned long long* count_word, unsigned long long* first_word, unsigned long long cnt,
                                           unsigned long long first, unsigned long long* s_cnt, unsigned long long* s_first) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        cnt += __shfl_xor(cnt, d, kWave);
        const unsigned long long o = __shfl_xor(first, d, kWave);
        first = o < first ? o : first;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_first[wave] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) {
            cnt += s_cnt[w];
            first = s_first[w] < first ? s_first[w] : first;
        }
        if (cnt) {
            atomicAdd(count_word, cnt);
            atomicMin(first_word, first);
        }
    }
}

__global__ void __launch_bounds__(kBlock) bounds_partial_kernel(const BoundsArgs a) {
    __shared__ int64_t s_w[kWaves];
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.report) {      // every call overwrites the report (launches 3 and 4 add to it)
        a.report[0] = 0;
        a.report[1] = 0;
        a.report[2] = kNone;
        a.report[3] = kNone;
    }
    const int64_t k0 = static_cast<int64_t>(blockIdx.x) * PM_BOUNDS_OFFSETS_PER_WG + static_cast<int64_t>(threadIdx.x) * kOffPerThread;
    int64_t m = 0;
#pragma unroll
    for (int i = 0; i < kOffPerThread; ++i) {
        const int64_t k = k0 + i;
        if (k < a.TB) m = max64(m, clamped(a, k, load_index(a.offsets, k, a.idx64)));
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) m = max64(m, __shfl_xor(m, d, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) m = max64(m, s_w[w]);
        a.partials[blockIdx.x] = m;
    }
}

// partials[w] <- max(partials[0 .. w - 1]) (0 for w = 0): one workgroup, 256 partials at a time with a carry
__global__ void __launch_bounds__(kBlock) bounds_scan_kernel(int64_t* partials, int64_t n) {
    __shared__ int64_t s_w[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const int64_t inc = wave_scan_max(i < n ? partials[i] : 0);
        if (lane == kWave - 1) s_w[wave] = inc;
        __syncthreads();
        int64_t pre = carry, total = carry;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) pre = max64(pre, s_w[w]);
            total = max64(total, s_w[w]);
        }
        const int64_t before = __shfl_up(inc, 1, kWave);
        if (i < n) partials[i] = lane ? max64(pre, before) : pre;
        carry = total;
        __syncthreads();                                        // the next round rewrites s_w
    }
}

__global__ void __launch_bounds__(kBlock) bounds_apply_kernel(const BoundsArgs a) {
    __shared__ int64_t s_w[kWaves];
    __shared__ unsigned long long s_cnt[kWaves], s_first[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t k0 = static_cast<int64_t>(blockIdx.x) * PM_BOUNDS_OFFSETS_PER_WG + static_cast<int64_t>(threadIdx.x) * kOffPerThread;
    int64_t raw[kOffPerThread], loc[kOffPerThread];
    int64_t run = 0;
#pragma unroll
    for (int i = 0; i < kOffPerThread; ++i) {
        const int64_t k = k0 + i;
        raw[i] = 0;
        if (k < a.TB) {
            raw[i] = load_index(a.offsets, k, a.idx64);
            run = max64(run, clamped(a, k, raw[i]));
        }
        loc[i] = run;
    }
    const int64_t inc = wave_scan_max(run);
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    int64_t pre = a.partials[blockIdx.x];                       // everything before this workgroup (launch 2)
    for (int w = 0; w < wave; ++w) pre = max64(pre, s_w[w]);
    const int64_t before = __shfl_up(inc, 1, kWave);
    if (lane) pre = max64(pre, before);

    unsigned long long cnt = 0, first = kNone;
#pragma unroll
    for (int i = 0; i < kOffPerThread; ++i) {
        const int64_t k = k0 + i;
        if (k < a.TB) {
            const int64_t v = max64(pre, loc[i]);
            if (v != raw[i]) {
                ++cnt;
                if (static_cast<unsigned long long>(k) < first) first = static_cast<unsigned long long>(k);
                if (a.write) store_index(a.offsets, k, v, a.idx64);
            }
            if (k % a.B == 0) a.borders[k / a.B] = v;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.borders[a.T] = a.N;
        if (a.has_last && load_index(a.offsets, a.TB, a.idx64) != a.N) {
            ++cnt;
            if (static_cast<unsigned long long>(a.TB) < first) first = static_cast<unsigned long long>(a.TB);
            if (a.write) store_index(a.offsets, a.TB, a.N, a.idx64);
        }
    }
    if (a.report) report_add(a.report + 1, a.report + 3, cnt, first, s_cnt, s_first);
}

// the last table t in [0, nt) with b[t] <= j (b non-decreasing, b[0] <= j)
__device__ __forceinline__ int table_of(const int64_t* b, int nt, int64_t j) {
    int lo = 0, hi = nt;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename IT>
__global__ void __launch_bounds__(kBlock) bounds_indices_kernel(const BoundsArgs a, int64_t head, int64_t nvec) {
    constexpr int VEC = 16 / static_cast<int>(sizeof(IT));
    typedef IT VT __attribute__((ext_vector_type(VEC)));
    __shared__ int64_t s_borders[kBoundsTablesLds + 1];
    __shared__ int64_t s_rows[kBoundsTablesLds];
    __shared__ unsigned long long s_cnt[kWaves], s_first[kWaves];
    PM_GLOBAL IT* const idx = as_global<IT>(a.indices);

    const bool last_wg = blockIdx.x == gridDim.x - 1;
    const int64_t v0 = static_cast<int64_t>(blockIdx.x) * kIdxVecPerWg;
    const int64_t v1 = v0 + kIdxVecPerWg < nvec ? v0 + kIdxVecPerWg : nvec;
    // the workgroup's contiguous chunk of lookups: its vectors, plus the scalar head (first workgroup) and tail (last one)
    const int64_t e0 = blockIdx.x == 0 ? 0 : head + v0 * VEC;
    const int64_t e1 = last_wg ? a.N : head + v1 * VEC;
    if (e0 >= e1) return;
    const int t_lo = table_of(a.borders, a.T, e0);
    const int nt = table_of(a.borders, a.T, e1 - 1) - t_lo + 1;
    // borders b[0 .. nt] and rows r[0 .. nt) of the chunk's tables: LDS copies while they fit, the global arrays otherwise
    const int64_t* b = a.borders + t_lo;
    const int64_t* r = a.rows + t_lo;
    if (nt > 1 && nt <= kBoundsTablesLds) {
        for (int i = threadIdx.x; i <= nt; i += kBlock) s_borders[i] = a.borders[t_lo + i];
        for (int i = threadIdx.x; i < nt; i += kBlock) s_rows[i] = a.rows[t_lo + i];
        __syncthreads();
        b = s_borders;
        r = s_rows;
    }
    const int64_t rows0 = r[0];

    unsigned long long cnt = 0, first = kNone;
    auto fix = [&](int64_t j, int64_t val, int64_t rows) {
        if (val < 0 || val >= rows) {
            ++cnt;
            if (static_cast<unsigned long long>(j) < first) first = static_cast<unsigned long long>(j);
            if (a.write && val != 0) idx[j] = 0;
        }
    };
    // one element whose table is not known: the scalar head and tail
    auto fix_one = [&](int64_t j) { fix(j, static_cast<int64_t>(idx[j]), nt == 1 ? rows0 : r[table_of(b, nt, j)]); };

    for (int64_t v = v0 + threadIdx.x; v < v1; v += kIdxUnroll * kBlock) {
        VT x[kIdxUnroll];
#pragma unroll
        for (int u = 0; u < kIdxUnroll; ++u) {
            const int64_t vu = v + u * kBlock;
            if (vu < v1) x[u] = *reinterpret_cast<const PM_GLOBAL VT*>(idx + head + vu * VEC);
        }
#pragma unroll
        for (int u = 0; u < kIdxUnroll; ++u) {
            const int64_t vu = v + u * kBlock;
            if (vu >= v1) continue;
            const int64_t j0 = head + vu * VEC;
            if (nt == 1) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) fix(j0 + e, static_cast<int64_t>(x[u][e]), rows0);
            } else {
                int t = table_of(b, nt, j0);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    while (t + 1 < nt && b[t + 1] <= j0 + e) ++t;      // a border inside the vector (empty tables: several)
                    fix(j0 + e, static_cast<int64_t>(x[u][e]), r[t]);
                }
            }
        }
    }
    if (blockIdx.x == 0 && static_cast<int64_t>(threadIdx.x) < head) fix_one(threadIdx.x);
    const int64_t tail0 = head + nvec * VEC;
    if (last_wg && tail0 + static_cast<int64_t>(threadIdx.x) < a.N) fix_one(tail0 + threadIdx.x);
    if (a.report) report_add(a.report, a.report + 2, cnt, first, s_cnt, s_first);
}

}  // namespace

int64_t bounds_check_scratch_bytes(int64_t TB, int T) {
    if (TB <= 0) return 0;
    const int64_t nwg = (TB + PM_BOUNDS_OFFSETS_PER_WG - 1) / PM_BOUNDS_OFFSETS_PER_WG;
    return (nwg + T + 1) * static_cast<int64_t>(sizeof(int64_t));
}

// p: the request (T * B > 0; indices / offsets aligned to their element); write: repair in place; report: device int64[4] or NULL
hipError_t launch_bounds_check(const KParams& p, bool write, bool has_last, int64_t* report, void* scratch, hipStream_t stream) {
    BoundsArgs a;
    a.indices = const_cast<void*>(p.indices);
    a.offsets = const_cast<void*>(p.offsets);
    a.rows = p.rows;
    a.report = reinterpret_cast<unsigned long long*>(report);
    a.TB = static_cast<int64_t>(p.T) * p.B;
    a.B = p.B;
    a.N = p.N;
    a.T = p.T;
    a.idx64 = p.idx64;
    a.write = write ? 1 : 0;
    a.has_last = has_last ? 1 : 0;
    const int64_t nwg = (a.TB + PM_BOUNDS_OFFSETS_PER_WG - 1) / PM_BOUNDS_OFFSETS_PER_WG;
    a.partials = static_cast<int64_t*>(scratch);
    a.borders = a.partials + nwg;
    if (nwg > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const dim3 bd(kBlock), gd(static_cast<unsigned>(nwg));
    hipLaunchKernelGGL(bounds_partial_kernel, gd, bd, 0, stream, a);
    hipLaunchKernelGGL(bounds_scan_kernel, dim3(1), bd, 0, stream, a.partials, nwg);
    hipLaunchKernelGGL(bounds_apply_kernel, gd, bd, 0, stream, a);
    if (a.N > 0) {
        const int es = a.idx64 ? 8 : 4, vec = 16 / es;
        // elements in front of the first 16-byte boundary, whole vectors behind it; what is left is the tail
        int64_t head = static_cast<int64_t>((16 - (reinterpret_cast<uintptr_t>(a.indices) & 15)) & 15) / es;
        if (head > a.N) head = a.N;
        const int64_t nvec = (a.N - head) / vec;
        int64_t grid = (nvec + kIdxVecPerWg - 1) / kIdxVecPerWg;
        if (grid < 1) grid = 1;                                 // head and tail alone
        if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
        const dim3 gi(static_cast<unsigned>(grid));
        if (a.idx64) hipLaunchKernelGGL((bounds_indices_kernel<int64_t>), gi, bd, 0, stream, a, head, nvec);
        else hipLaunchKernelGGL((bounds_indices_kernel<int32_t>), gi, bd, 0, stream, a, head, nvec);
    }
    return hipGetLastError();
}

}  // namespace pm
