// param_amd/csrc/f8_quantize.hip -- pm_f8_row_exponents and pm_rows_quantize_f8: the quantiser of SCALED FP8 TABLES (include/param_amd.h).
// gfx950 only.
//
// Both kernels: a 256-thread workgroup, a group of G lanes (8 / 16 / 32 / 64 for the row's 16-byte pieces, a run-time value: the
// butterfly below is the only thing that depends on it) owns a row, workgroups stride over the rows; a lane's load is 16 bytes of the
// source row -- 4 fp32 or 8 bf16 / fp16 columns, widened exactly (fwd_elem.h).
//   * exponents: amax as the INTEGER maximum of the magnitude bits of the row's finite elements (a non-finite element counts as 0),
//     reduced over the lane group by a fixed xor butterfly; lane 0 of the group writes row_exponent(amax) (f8s_elem.h).
//   * codes: s = clamp(E_t + e_r) (either absent = 0), code = cast(x * 2^-s): one fp32 multiplication by a power of two, then the
//     encode; a lane writes its 4 / 8 codes as one 4- / 8-byte piece.
// THE ENCODE: gfx950's v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 for |y| <= fmax (round to nearest even into OCP e4m3fn / e5m2 -- what
// tests/test_gpu_f8s.py holds to torch's cast for every code, every tie and their fp32 neighbours); what lies above fmax is selected
// explicitly, because how the instruction saturates is not torch's business: below the midpoint above fmax the code is fmax's, beyond
// it (and for +-Inf) the next code -- e4m3fn's NaN, e5m2's Inf --, the tie at 464 / 61440 goes to the even one of the two, a NaN gives a
// NaN code.  -DPM_F8S_SOFT_ENCODE takes f8s_elem.h's integer encode
// for every input instead (the experiment build the hardware path was compared with).
// No atomics, no inline assembly, no LDS.
#include "common.h"
#include "fwd_elem.h"
#include "f8s_elem.h"

namespace pm {
namespace {

using namespace fwd;

template <typename ST> struct SrcBytes { static constexpr int value = 2; };
template <> struct SrcBytes<float> { static constexpr int value = 4; };

// the magnitude bits of a finite value, 0 for +-Inf and NaN
__device__ __forceinline__ uint32_t finite_magnitude(float f) {
    const uint32_t a = __float_as_uint(f) & 0x7fffffffu;
    return a < 0x7f800000u ? a : 0u;
}

template <typename ST>
__global__ void __launch_bounds__(kBlock) f8_row_exponents_kernel(const char* __restrict__ src, int64_t n_rows, int dim, int64_t row_bytes, int k, int G,
                                                                  int8_t* __restrict__ row_exp) {
    constexpr int VEC = Elem<ST>::kVec;
    const int lig = static_cast<int>(threadIdx.x) % G;
    const int64_t rows_per_block = kBlock / G;
    for (int64_t r = blockIdx.x * rows_per_block + threadIdx.x / G; r < n_rows; r += gridDim.x * rows_per_block) {
        const char* row = src + r * row_bytes;
        uint32_t amax = 0;
        for (int c = lig * VEC; c < dim; c += G * VEC) {   // (dim % 16 == 0: a lane's 16 bytes end inside the row)
            float f[VEC];
            Elem<ST>::widen(load16(row + static_cast<int64_t>(c) * SrcBytes<ST>::value, false), f);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const uint32_t a = finite_magnitude(f[i]);
                amax = a > amax ? a : amax;
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) {             // the lane group's lanes are all here: r is theirs in common
            const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), m, kWave));
            amax = o > amax ? o : amax;
        }
        if (lig == 0) row_exp[r] = static_cast<int8_t>(f8s::row_exponent(amax, k));
    }
}

template <bool E5M2>
__device__ __forceinline__ uint32_t encode_pair(float a, float b) {      // two codes, a's in the low byte
#ifdef PM_F8S_SOFT_ENCODE
    return f8s::encode_soft<E5M2>(a) | (f8s::encode_soft<E5M2>(b) << 8);
#else
    constexpr uint32_t kFmax = E5M2 ? 0x47600000u : 0x43e00000u;          // 57344 | 448
    // the midpoint between fmax and the value the next code would have: 61440 (the tie goes up, to the even code: Inf) | 464 (the tie goes
    // down: 448's code is the even one; above it the next code, which is e4m3fn's NaN)
    constexpr uint32_t kMid = E5M2 ? 0x47700000u : 0x43e80000u;
    constexpr uint32_t kMaxCode = E5M2 ? 0x7bu : 0x7eu, kOverCode = E5M2 ? 0x7cu : 0x7fu;
    const int hw = E5M2 ? __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false) : __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    uint32_t out = 0;
    const float v[2] = {a, b};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t u = __float_as_uint(v[i]), mag = u & 0x7fffffffu;
        uint32_t code = (static_cast<uint32_t>(hw) >> (8 * i)) & 0xffu;
        if (mag > kFmax) code = ((u >> 24) & 0x80u) | (mag > 0x7f800000u ? 0x7fu : ((E5M2 ? mag >= kMid : mag > kMid) ? kOverCode : kMaxCode));
        out |= code << (8 * i);
    }
    return out;
#endif
}

template <typename ST, bool E5M2>
__global__ void __launch_bounds__(kBlock) f8_rows_quantize_kernel(const char* __restrict__ src, int64_t n_rows, int dim, int64_t row_bytes, int G,
                                                                  const int32_t* __restrict__ table_exp, const int8_t* __restrict__ row_exp,
                                                                  char* __restrict__ dst) {
    constexpr int VEC = Elem<ST>::kVec;
    const int lig = static_cast<int>(threadIdx.x) % G;
    const int64_t rows_per_block = kBlock / G;
    const int base_exp = table_exp ? table_exp[0] : 0;
    for (int64_t r = blockIdx.x * rows_per_block + threadIdx.x / G; r < n_rows; r += gridDim.x * rows_per_block) {
        const char* row = src + r * row_bytes;
        char* out = dst + r * dim;
        const float inv = f8s::pow2(-f8s::clamp_exp(base_exp + (row_exp ? static_cast<int>(row_exp[r]) : 0)));
        for (int c = lig * VEC; c < dim; c += G * VEC) {
            float f[VEC];
            Elem<ST>::widen(load16(row + static_cast<int64_t>(c) * SrcBytes<ST>::value, false), f);
            uint32_t w[VEC / 4];
#pragma unroll
            for (int i = 0; i < VEC; i += 4)
                w[i / 4] = encode_pair<E5M2>(f[i] * inv, f[i + 1] * inv) | (encode_pair<E5M2>(f[i + 2] * inv, f[i + 3] * inv) << 16);
            if constexpr (VEC == 4) *as_global<uint32_t>(out + c) = w[0];
            else *as_global<u32x2>(out + c) = u32x2{w[0], w[1]};
        }
    }
}

// lanes per row and the grid: a row's 16-byte pieces decide the lane group; workgroups stride over the rows beyond 2^20 of them
inline void quantize_geometry(int64_t n_rows, int dim, int vec, int& G, unsigned& grid) {
    G = group_lanes(dim, vec);
    const int64_t blocks = ceil_div(n_rows, static_cast<int64_t>(kBlock / G));
    grid = static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20));
}

template <typename ST>
hipError_t exponents_t(const void* src, int64_t n_rows, int dim, int64_t stride, int f8_dtype, int8_t* row_exp, hipStream_t stream) {
    int G;
    unsigned grid;
    quantize_geometry(n_rows, dim, Elem<ST>::kVec, G, grid);
    hipLaunchKernelGGL((f8_row_exponents_kernel<ST>), dim3(grid), dim3(kBlock), 0, stream, static_cast<const char*>(src), n_rows, dim,
                       stride * SrcBytes<ST>::value, f8s::fmax_exp(f8_dtype == PM_F8E5M2), G, row_exp);
    return hipGetLastError();
}

template <typename ST>
hipError_t quantize_t(const void* src, int64_t n_rows, int dim, int64_t stride, int f8_dtype, const int32_t* table_exp, const int8_t* row_exp,
                      void* dst, hipStream_t stream) {
    int G;
    unsigned grid;
    quantize_geometry(n_rows, dim, Elem<ST>::kVec, G, grid);
    auto launch = [&](auto e5m2) {
        hipLaunchKernelGGL((f8_rows_quantize_kernel<ST, decltype(e5m2)::value>), dim3(grid), dim3(kBlock), 0, stream, static_cast<const char*>(src),
                           n_rows, dim, stride * SrcBytes<ST>::value, G, table_exp, row_exp, static_cast<char*>(dst));
    };
    dispatch_bool(f8_dtype == PM_F8E5M2, launch);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_f8_row_exponents(const void* src, int src_dtype, int64_t n_rows, int dim, int64_t stride, int f8_dtype, int8_t* row_exp,
                                   hipStream_t stream) {
    if (src_dtype == PM_BF16) return exponents_t<bf16_t>(src, n_rows, dim, stride, f8_dtype, row_exp, stream);
    if (src_dtype == PM_F16) return exponents_t<f16_t>(src, n_rows, dim, stride, f8_dtype, row_exp, stream);
    return exponents_t<float>(src, n_rows, dim, stride, f8_dtype, row_exp, stream);
}

hipError_t launch_rows_quantize_f8(const void* src, int src_dtype, int64_t n_rows, int dim, int64_t stride, int f8_dtype, const int32_t* table_exp,
                                   const int8_t* row_exp, void* dst, hipStream_t stream) {
    if (src_dtype == PM_BF16) return quantize_t<bf16_t>(src, n_rows, dim, stride, f8_dtype, table_exp, row_exp, dst, stream);
    if (src_dtype == PM_F16) return quantize_t<f16_t>(src, n_rows, dim, stride, f8_dtype, table_exp, row_exp, dst, stream);
    return quantize_t<float>(src, n_rows, dim, stride, f8_dtype, table_exp, row_exp, dst, stream);
}

}  // namespace pm
