// param_amd/csrc/qrows_elem.h -- the device building blocks both kernels over 8- and 4-bit ROW-QUANTISED tables share: the pooled lookup
// (embbag_fwd_qrows.hip) and the un-pooled one (embedding_gather_qrows.hip), and their siblings over tables of per-table format
// (embbag_fwd_qmixed.hip, embedding_gather_qmixed.hip: the last block below).  A row is uint8 [rq::row_bytes(D, BITS)]: the codes of the D
// columns (a 4-bit code of column c in byte c / 2 at bit 4 * (c % 2)), then the row's tail -- scale and bias (8 bits: two fp32; 4 bits:
// two fp16, widened exactly).  gfx950 only.
#pragma once

#include "common.h"
#include "fwd_elem.h"
#include "rowquant.inc"

namespace pm {
namespace fwd {

template <int BITS> struct QRow;
template <> struct QRow<8> {
    static constexpr int kVec = 4;                       // columns per dword of codes
    struct Tail { float scale, bias; };
    __device__ static __forceinline__ Tail tail(const char* row, int code_bytes) {
        const PM_GLOBAL uint32_t* q = as_global<uint32_t>(row + code_bytes);
        return Tail{__uint_as_float(q[0]), __uint_as_float(q[1])};
    }
    __device__ static __forceinline__ void unpack(uint32_t raw, float (&f)[4]) {
        f[0] = static_cast<float>(raw & 0xffu);
        f[1] = static_cast<float>((raw >> 8) & 0xffu);
        f[2] = static_cast<float>((raw >> 16) & 0xffu);
        f[3] = static_cast<float>(raw >> 24);
    }
    // the 4 codes of a piece of 4 columns: the low 4 * BITS bits of w
    __device__ static __forceinline__ void piece(uint32_t w, float (&f)[4]) { unpack(w, f); }
};
template <> struct QRow<4> {
    static constexpr int kVec = 8;
    struct Tail { float scale, bias; };
    __device__ static __forceinline__ Tail tail(const char* row, int code_bytes) {
        const uint32_t sb = *as_global<uint32_t>(row + code_bytes);
        return Tail{rq::half_value(static_cast<uint16_t>(sb & 0xffffu)), rq::half_value(static_cast<uint16_t>(sb >> 16))};
    }
    __device__ static __forceinline__ void unpack(uint32_t raw, float (&f)[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = static_cast<float>((raw >> (4 * k)) & 0xfu);
    }
    __device__ static __forceinline__ void piece(uint32_t w, float (&f)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = static_cast<float>((w >> (4 * k)) & 0xfu);
    }
};

// kQrowsLaneDwords (launch_plan.h) dwords of codes per lane and row, loaded as ONE instruction at a 4-byte-aligned address: two in the
// product (global_load_dwordx2), 1 and 4 in experiment builds.  The dwords of a row's last lane that lie behind the codes are the
// row's own tail with two dwords per lane (read, never used: 8 tail bytes behind 8-bit codes, 4 behind 4-bit codes, and a lane's
// first dword is always codes); with four they may lie behind the row, which is why four is not a product setting.
constexpr int kLaneDwords = kQrowsLaneDwords;
static_assert(kLaneDwords == 1 || kLaneDwords == 2 || kLaneDwords == 4, "PM_QROWS_LANE_DWORDS must be 1, 2 or 4");
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// one row's codes of this lane and its tail, as loaded
template <int BITS> struct QLoad {
    uint32_t raw[kLaneDwords];
    typename QRow<BITS>::Tail tail;
};
template <int BITS>
__device__ __forceinline__ QLoad<BITS> load_row(const char* row, int code_off, int code_bytes) {
    QLoad<BITS> q;
    if constexpr (kLaneDwords == 4) {
        const u32x4_a4 v = *as_global<u32x4_a4>(row + code_off);
#pragma unroll
        for (int h = 0; h < kLaneDwords; ++h) q.raw[h] = v[h];
    } else if constexpr (kLaneDwords == 2) {
        const u32x2_a4 v = *as_global<u32x2_a4>(row + code_off);
#pragma unroll
        for (int h = 0; h < kLaneDwords; ++h) q.raw[h] = v[h];
    } else {
        q.raw[0] = *as_global<uint32_t>(row + code_off);
    }
    q.tail = QRow<BITS>::tail(row, code_bytes);
    return q;
}

// The kernels over tables of PER-TABLE format (embbag_fwd_qmixed.hip, embedding_gather_qmixed.hip) hold kQmixedLaneColumns = EIGHT
// COLUMNS per lane and row whatever the row's format -- two dwords of an 8-bit row (the load above at its product setting), one dword
// of a 4-bit row -- so that the lane group, the accumulators, the column passes and the output pieces are one for every table of a
// launch (launch_plan.h: plan_qmixed).  Widths are multiples of 8: a lane's columns lie wholly inside the row's codes or wholly behind.
// LD: dwords of codes per lane and row, ONE load instruction at a dword-aligned address.  The product's: kQmixedDwords<BITS> (8 bits: 2,
// 4 bits: 1); the pooled kernel's experiment build -DPM_QMIXED_4BIT_DWORDS=2 gives a 4-bit row two (16 columns: the second dword of a
// row's last lane may be the row's own 4-byte tail, read and never used -- never behind the row).
template <int BITS> constexpr int kQmixedDwords = kQmixedLaneColumns / QRow<BITS>::kVec;
template <int BITS, int LD> struct QLoadN {
    static_assert(LD == 1 || LD == 2, "one or two dwords of codes per lane");
    uint32_t raw[LD];
    typename QRow<BITS>::Tail tail;
};
// code_off: byte offset of the lane's first dword of codes (a multiple of 4, inside the codes)
template <int BITS, int LD>
__device__ __forceinline__ QLoadN<BITS, LD> load_row_n(const char* row, int code_off, int code_bytes) {
    QLoadN<BITS, LD> q;
    if constexpr (LD == 2) {
        const u32x2_a4 v = *as_global<u32x2_a4>(row + code_off);
        q.raw[0] = v[0];
        q.raw[1] = v[1];
    } else {
        q.raw[0] = *as_global<uint32_t>(row + code_off);
    }
    q.tail = QRow<BITS>::tail(row, code_bytes);
    return q;
}

}  // namespace fwd
}  // namespace pm
