// param_amd/csrc/sparse_rows_walk.h -- the device pieces the sparse-row optimizer kernels share (sparse_rows_adam.hip, sparse_rows_step.hip):
// how a row slot of the concatenated coalesced gradient finds its table, how a tile is cut into runs of one lane-group width, the
// 4-column accesses and the widen / pack traits of the three table types.  gfx950 only; every function is inlined into its kernel.
#pragma once
#include "common.h"
#include "fwd_elem.h"

namespace pm {
namespace rows {

using namespace fwd;

constexpr int kAdamLdsPrefix = 256;   // prefix entries the LDS copy holds: T + 1 <= 256, i.e. up to 255 tables

// log2 of the lanes a row of D columns takes: next_pow2(D / 4), capped at 64
__device__ __forceinline__ int adam_group_log2(int D) {
    int lg = 0;
    while (lg < 6 && (4 << lg) < D) ++lg;
    return lg;
}

// the slot's table: the first t with prefix[t + 1] > j (tables without rows are passed over: equal neighbouring entries).
// `prefix`: the T + 1 entries, the LDS copy or the global array
template <typename P>
__device__ __forceinline__ int slot_table(const P* prefix, int T, int64_t j) {
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid + 1] <= j) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Grows the run that starts at slot b of the tile (slots are relative to j0, the tile holds n) over the consecutive tables [t, ..) whose
// rows take 2^lg lanes; returns the run's end, leaves t at the first table that did not join and raises d_max to the run's widest row.
// Every value is uniform over the workgroup.  (The table of slot b always joins: the run grows by at least that one.)
template <typename P>
__device__ __forceinline__ int run_end(const P* prefix, const int32_t* dims, int64_t j0, int n, int t_last, int lg, int b, int& t,
                                       int& d_max) {
    for (; t <= t_last; ++t) {
        const int64_t end = prefix[t + 1] - j0;
        if (end <= b) continue;                                              // a table without rows: no slot, whatever its width
        const int D = dims[t];
        if (adam_group_log2(D) != lg) break;
        b = end < n ? static_cast<int>(end) : n;
        d_max = D > d_max ? D : d_max;
    }
    return b;
}

template <bool NT>
__device__ __forceinline__ f32x4 adam_load4(int64_t base, int c) {
    const PM_GLOBAL f32x4* q = reinterpret_cast<const PM_GLOBAL f32x4*>(base) + (c >> 2);
    return NT ? __builtin_nontemporal_load(q) : *q;
}
template <bool NT>
__device__ __forceinline__ void adam_store4(int64_t base, int c, const f32x4& x) {
    PM_GLOBAL f32x4* q = reinterpret_cast<PM_GLOBAL f32x4*>(base) + (c >> 2);
    if (NT) __builtin_nontemporal_store(x, q); else *q = x;
}

// four columns of a weight row, widened exactly, and back with the table type's one rounding (fp32: the identity)
template <typename WT> struct AdamW;
template <> struct AdamW<float> {
    typedef f32x4 raw_t;
    __device__ static __forceinline__ float widen(const raw_t& r, int k) { return r[k]; }
    __device__ static __forceinline__ raw_t pack(const float (&f)[4]) { return raw_t{f[0], f[1], f[2], f[3]}; }
};
template <> struct AdamW<bf16_t> {
    typedef u32x2 raw_t;
    __device__ static __forceinline__ float widen(const raw_t& r, int k) {
        return __uint_as_float((k & 1) ? (r[k >> 1] & 0xffff0000u) : (r[k >> 1] << 16));
    }
    __device__ static __forceinline__ raw_t pack(const float (&f)[4]) {
        return raw_t{f32_to_bf16_rne(f[0]) | (f32_to_bf16_rne(f[1]) << 16), f32_to_bf16_rne(f[2]) | (f32_to_bf16_rne(f[3]) << 16)};
    }
};
template <> struct AdamW<f16_t> {
    typedef u32x2 raw_t;
    __device__ static __forceinline__ float widen(const raw_t& r, int k) {
        return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>((k & 1) ? (r[k >> 1] >> 16) : (r[k >> 1] & 0xffffu))));
    }
    __device__ static __forceinline__ raw_t pack(const float (&f)[4]) {
        return raw_t{OutF16::round(f[0]) | (OutF16::round(f[1]) << 16), OutF16::round(f[2]) | (OutF16::round(f[3]) << 16)};
    }
};

// the table row's four columns at column c (a multiple of 4): a 16-byte access of an fp32 row, an 8-byte access of a 16-bit row; plain
template <typename WT>
__device__ __forceinline__ typename AdamW<WT>::raw_t w_load4(int64_t base, int c) {
    return *(reinterpret_cast<const PM_GLOBAL typename AdamW<WT>::raw_t*>(base) + (c >> 2));
}
template <typename WT>
__device__ __forceinline__ void w_store4(int64_t base, int c, const float (&f)[4]) {
    *(reinterpret_cast<PM_GLOBAL typename AdamW<WT>::raw_t*>(base) + (c >> 2)) = AdamW<WT>::pack(f);
}

}  // namespace rows
}  // namespace pm
