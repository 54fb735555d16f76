// param_amd/csrc/mx4_elem.h -- the MXFP4 row format's device pieces (include/param_amd.h, MXFP4 TABLES), shared by the quantiser
// (mx4_quantize.hip), the pooled lookup (embbag_fwd_mx4.hip) and the un-pooled lookup (embedding_gather_mx4.hip).  gfx950 only.
//
// A row of D columns: D / 2 code bytes (e2m1, column c in byte c / 2 at bit 4 * (c % 2)), then D / 32 E8M0 scale bytes (one per block of
// 32 columns, value 2^(x - 127), x == 255: the block is NaN), zero-padded to a multiple of 8 bytes.
// DECODE: gfx950's v_cvt_scalef32_pk_f32_fp4 -- one byte (two columns) of a dword per instruction, times the scale operand, which is
// built from the scale byte as the fp32 pattern x << 23 -- with NaN selected explicitly for x == 255.  -DPM_MX4_SOFT_DECODE: the nibble
// expanded to fp32 bits with integer operations and ONE multiplication by the scale (exact for x in [2, 252]).
// ENCODE: v_cvt_scalef32_pk_fp4_f32 (two columns into one byte of a dword, the same scale operand), or -DPM_MX4_SOFT_ENCODE: the code's
// magnitude is the number of the seven rounding thresholds (the midpoints of neighbouring e2m1 magnitudes, times the block's scale) that
// the element's magnitude BITS pass -- positive fp32 patterns, subnormal ones included, order as integers, every threshold is an fp32
// value, and whether a midpoint itself passes says where its tie goes (to the even code).
#pragma once

#include "common.h"

namespace pm {
namespace mx4 {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kBlockColumns = 32;
constexpr uint32_t kNanScale = 255u;
constexpr uint32_t kQuietNan = 0x7fc00000u;

__host__ __device__ inline int64_t row_bytes(int D) { return (static_cast<int64_t>(D) / 2 + D / kBlockColumns + 7) / 8 * 8; }

// the scale byte as the conversions' scale operand: 2^(x - 127), normal for every x of the contract
__device__ __forceinline__ float scale_operand(uint32_t x) { return __uint_as_float(x << 23); }

// the fp32 pattern of an e2m1 code's magnitude: 0, 0.5, 1, 1.5, 2, 3, 4, 6
__device__ __forceinline__ uint32_t magnitude_bits(uint32_t m3) { return m3 >= 2u ? (m3 + 252u) << 22 : (m3 ? 0x3f000000u : 0u); }

// byte B (two columns) of a dword of codes, low nibble first
template <int B>
__device__ __forceinline__ void widen_byte(uint32_t w, uint32_t x, float scale, float* f) {
#ifndef PM_MX4_SOFT_DECODE
    const f32x2 v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, B);
    f[0] = x == kNanScale ? __uint_as_float(kQuietNan) : v[0];
    f[1] = x == kNanScale ? __uint_as_float(kQuietNan) : v[1];
#else
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t n = (w >> (8 * B + 4 * i)) & 0xfu;
        const float v = __uint_as_float(magnitude_bits(n & 7u)) * scale;      // exact: a power of two times at most two mantissa bits
        f[i] = __uint_as_float(x == kNanScale ? kQuietNan : (__float_as_uint(v) | ((n & 8u) << 28)));
    }
#endif
}

// the eight columns of one dword of codes
__device__ __forceinline__ void widen_dword(uint32_t w, uint32_t x, float* f) {
    const float scale = scale_operand(x);
    widen_byte<0>(w, x, scale, f);
    widen_byte<1>(w, x, scale, f + 2);
    widen_byte<2>(w, x, scale, f + 4);
    widen_byte<3>(w, x, scale, f + 6);
}

// ---- the quantiser's side ----------------------------------------------------------------------------------------------------------
// the block's scale byte from the integer maximum of its elements' magnitude bits: a non-finite element's bits are the maximum whatever
// else the block holds, so the maximum carries the non-finite flag; q = floor(log2 amax) is the exponent field (a subnormal or zero
// amax: field 0, below the clamp anyway), x = clamp(q - 2 + 127, 2, 252) = max(field, 4) - 2
__device__ __forceinline__ uint32_t block_scale(uint32_t amax_bits) {
    if (amax_bits >= 0x7f800000u) return kNanScale;
    const uint32_t field = amax_bits >> 23;
    return (field > 4u ? field : 4u) - 2u;
}

// the seven thresholds T * 2^(x - 127), T = 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, as fp32 patterns (x in [2, 252]): T's pattern with the
// exponent field moved by x - 127 -- but 0.25 * 2^-125 = 2^-127 is subnormal
struct Thresholds { uint32_t t[7]; };
__device__ __forceinline__ Thresholds thresholds(uint32_t x) {
    const uint32_t d = (x - 127u) << 23;
    Thresholds r;
    r.t[0] = x > 2u ? 0x3e800000u + d : 0x00400000u;
    r.t[1] = 0x3f400000u + d;
    r.t[2] = 0x3fa00000u + d;
    r.t[3] = 0x3fe00000u + d;
    r.t[4] = 0x40200000u + d;
    r.t[5] = 0x40600000u + d;
    r.t[6] = 0x40a00000u + d;
    return r;
}
// sign and the nearest e2m1 magnitude of value * 2^(127 - x); ties at 0.25, 1.25, 2.5 and 5 stay below (>), at 0.75, 1.75 and 3.5 go up (>=):
// to the even code each time; above 6 the code is 6's
__device__ __forceinline__ uint32_t encode_soft(float v, const Thresholds& th) {
    const uint32_t u = __float_as_uint(v), m = u & 0x7fffffffu;
    const uint32_t code = (m > th.t[0]) + (m >= th.t[1]) + (m > th.t[2]) + (m >= th.t[3]) + (m > th.t[4]) + (m >= th.t[5]) + (m > th.t[6]);
    return code | ((u >> 28) & 8u);
}

// two columns' codes as one byte, a's in the low nibble
__device__ __forceinline__ uint32_t encode_pair(float a, float b, uint32_t x, const Thresholds& th) {
#ifdef PM_MX4_SOFT_ENCODE
    return encode_soft(a, th) | (encode_soft(b, th) << 4);
#else
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, a, b, scale_operand(x), 0) & 0xffu;
#endif
}

}  // namespace mx4
}  // namespace pm
