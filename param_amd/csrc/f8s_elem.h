// param_amd/csrc/f8s_elem.h -- the pieces of the SCALED FP8 TABLES rule (include/param_amd.h) that are plain integer and fp32 arithmetic:
// the exponent range, 2^s built from its bits, a row's exponent from its largest finite magnitude, and the software encode of one fp32
// value.  Host and device: f8_quantize.hip, embbag_fwd_f8s_kernel.inc and embedding_gather_f8s.hip include it, and it compiles as plain
// C++ (no HIP header) so that the encode can be held to torch's CPU cast without a GPU.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PM_F8S_HD __host__ __device__ __forceinline__
#else
#define PM_F8S_HD inline
#endif

namespace pm {
namespace f8s {

constexpr int kExpMin = -64, kExpMax = 64;     // the range of E_t + e_r (and of each alone, as the quantiser writes them)

PM_F8S_HD float bits_float(uint32_t u) { return __builtin_bit_cast(float, u); }
PM_F8S_HD uint32_t float_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

PM_F8S_HD int clamp_exp(int s) { return s < kExpMin ? kExpMin : (s > kExpMax ? kExpMax : s); }
// 2^s for s in [-64, 64]: a normal fp32 value (exponent field 63 .. 191); a product with it only moves the other factor's exponent
PM_F8S_HD float pow2(int s) { return bits_float(static_cast<uint32_t>(127 + s) << 23); }

// fmax = 1.75 * 2^k: 448 (e4m3fn), 57344 (e5m2)
PM_F8S_HD constexpr int fmax_exp(bool e5m2) { return e5m2 ? 15 : 8; }

// The row's exponent from the magnitude bits of its largest FINITE element (0: no finite element, or all zeros): amax = m * 2^q with
// 1 <= m < 2 read from the exponent and mantissa fields, e = q - k if m <= 1.75 (mantissa field <= 0x600000) else q - k + 1, clamped.
// An fp32 subnormal (exponent field 0) has q <= -127: far below the clamp, like zero.  No logarithm.
PM_F8S_HD int row_exponent(uint32_t amax_bits, int k) {
    const int q = static_cast<int>(amax_bits >> 23) - 127;
    return clamp_exp(q - k + ((amax_bits & 0x7fffffu) > 0x600000u ? 1 : 0));
}

// The software encode: fp32 -> one code, round to nearest even, as torch's CPU `.to(torch.float8_e4m3fn / float8_e5m2)` gives it.
//   e4m3fn: the code after 448's is the NaN code 0x7f: |y| above the midpoint 464 rounds to it by the normal path (the tie stays at 448,
//           the even code), |y| >= 480, +-Inf and NaN are given it;
//   e5m2:   |y| from the midpoint 61440 on (the tie goes up, to the even code) rounds to +-Inf 0x7c by the normal path, NaN gives 0x7f;
//   below the smallest normal (2^-6 / 2^-14) the code is the subnormal count: one fp32 addition of 2^(min_exp - mbits + 23) puts the
//   count, rounded to nearest even by the adder, into the sum's low mantissa bits.
template <bool E5M2>
PM_F8S_HD uint32_t encode_soft(float y) {
    constexpr int MB = E5M2 ? 2 : 3, BIAS = E5M2 ? 15 : 7;
    constexpr uint32_t kInf = 0x7f800000u;
    constexpr uint32_t kOver = E5M2 ? (143u << 23) : 0x43f00000u;          // 65536 | 480
    constexpr uint32_t kMinNormal = static_cast<uint32_t>(127 + 1 - BIAS) << 23;
    constexpr uint32_t kMagic = static_cast<uint32_t>(127 + 1 - BIAS - MB + 23) << 23;
    const uint32_t u = float_bits(y), sign = (u >> 24) & 0x80u;
    uint32_t a = u & 0x7fffffffu, code;
    if (a >= kOver) {
        code = E5M2 ? (a > kInf ? 0x7fu : 0x7cu) : 0x7fu;
    } else if (a < kMinNormal) {
        code = float_bits(bits_float(a) + bits_float(kMagic)) - kMagic;
    } else {
        const uint32_t odd = (a >> (23 - MB)) & 1u;
        a += (static_cast<uint32_t>(BIAS - 127) << 23) + ((1u << (22 - MB)) - 1u) + odd;
        code = a >> (23 - MB);
    }
    return code | sign;
}

}  // namespace f8s
}  // namespace pm
