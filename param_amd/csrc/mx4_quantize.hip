// param_amd/csrc/mx4_quantize.hip -- pm_rows_quantize_mx4: the quantiser of MXFP4 TABLES (include/param_amd.h).  gfx950 only.
//
// THE SOURCE IS READ ONCE.  A 256-thread workgroup; a group of G lanes (8 / 16 / 32 / 64 for the row's 16-byte pieces, a run-time value)
// owns a row and the workgroups stride over the rows; a lane's load is 16 bytes of the source row -- 4 fp32 or 8 bf16 / fp16 columns,
// widened exactly (fwd_elem.h) -- and stays in registers from the block maximum to the encode.  A BLOCK of 32 columns is therefore LPB =
// 8 consecutive lanes (fp32) or 4 (16-bit sources), aligned in the wave:
//   * amax: the integer maximum of the magnitude bits over a fixed xor butterfly inside the block's lanes (3 steps / 2 steps).  A
//     non-finite element's bits are above every finite one's, so the maximum IS the non-finite flag (mx4_elem.h: block_scale);
//   * every lane encodes its columns from registers (mx4_elem.h: the hardware conversion, or the integer encode);
//   * the codes travel to every fourth lane (fp32: 2 bytes per lane, two xor steps) or every second lane (16-bit: 4 bytes per lane, one
//     step), which then holds 8 consecutive code bytes: the 16 code bytes of a block leave as TWO 8-byte stores, and the stores of a
//     wave's blocks cover consecutive bytes of the row (a row starts 8-byte aligned and no better: 72 bytes at D = 128);
//   * the block's first lane writes the scale byte; the row's first lane writes the pad bytes (at most 7) as zeros.
// Control flow is uniform over the workgroup (rows past the end and lanes past the row's width load a valid address and store nothing),
// so every lane of a block is there for the exchanges.  No atomics, no LDS, no scratch, no inline assembly.
#include "common.h"
#include "fwd_elem.h"
#include "mx4_elem.h"

namespace pm {
namespace {

using namespace fwd;

template <typename ST> struct SrcBytes { static constexpr int value = 2; };
template <> struct SrcBytes<float> { static constexpr int value = 4; };

__device__ __forceinline__ uint32_t shfl_xor_u32(uint32_t v, int mask) { return static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), mask, kWave)); }

template <typename ST>
__global__ void __launch_bounds__(kBlock) mx4_rows_quantize_kernel(const char* __restrict__ src, int64_t n_rows, int dim, int64_t src_row_bytes, int G,
                                                                   char* __restrict__ dst) {
    constexpr int VEC = Elem<ST>::kVec;                    // columns per lane: 4 | 8
    constexpr int LPB = mx4::kBlockColumns / VEC;          // lanes per block: 8 | 4
    const int lig = static_cast<int>(threadIdx.x) % G;
    const int64_t rows_per_wg = kBlock / G;
    const int64_t dst_row_bytes = mx4::row_bytes(dim);
    const int code_bytes = dim / 2;
    const int tail = code_bytes + dim / mx4::kBlockColumns;   // the row's bytes before its padding
    for (int64_t r0 = blockIdx.x * rows_per_wg; r0 < n_rows; r0 += gridDim.x * rows_per_wg) {
        const int64_t r = r0 + threadIdx.x / G;
        const bool row_ok = r < n_rows;
        const char* row = src + (row_ok ? r : n_rows - 1) * src_row_bytes;
        char* out = dst + r * dst_row_bytes;               // (only dereferenced under row_ok)
        for (int c0 = 0; c0 < dim; c0 += G * VEC) {
            const int c = c0 + lig * VEC;
            const bool ok = row_ok && c < dim;             // (dim % 32 == 0: a block's lanes agree)
            float f[VEC];
            Elem<ST>::widen(load16(row + static_cast<int64_t>(c < dim ? c : 0) * SrcBytes<ST>::value, false), f);
            uint32_t amax = 0;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const uint32_t a = __float_as_uint(f[i]) & 0x7fffffffu;
                amax = a > amax ? a : amax;
            }
#pragma unroll
            for (int m = 1; m < LPB; m <<= 1) {
                const uint32_t o = shfl_xor_u32(amax, m);
                amax = o > amax ? o : amax;
            }
            const uint32_t x = mx4::block_scale(amax);
            // a NaN block's codes are not part of the rule: zeros, encoded at a scale of the contract
            const bool nan_block = x == mx4::kNanScale;
            const uint32_t xe = nan_block ? 127u : x;
            const mx4::Thresholds th = mx4::thresholds(xe);
            uint32_t codes = 0;                            // VEC / 2 bytes, the lane's first column in the low nibble
#pragma unroll
            for (int i = 0; i < VEC; i += 2) codes |= mx4::encode_pair(f[i], f[i + 1], xe, th) << (4 * i);
            if (nan_block) codes = 0;
            // eight consecutive code bytes per storing lane
            uint32_t lo, hi;
            if constexpr (VEC == 4) {
                const uint32_t pair = codes | (shfl_xor_u32(codes, 1) << 16);   // even lanes: 4 bytes
                lo = pair;
                hi = shfl_xor_u32(pair, 2);                                     // lanes 0 and 4 of the block: their neighbour pair's
            } else {
                lo = codes;
                hi = shfl_xor_u32(codes, 1);                                    // even lanes: the next lane's 4 bytes
            }
            constexpr int kStoreEvery = 8 / (VEC / 2);     // lanes per 8-byte store: 4 | 2
            if (ok && lig % kStoreEvery == 0) *as_global<u32x2>(out + c / 2) = u32x2{lo, hi};
            if (ok && lig % LPB == 0) *as_global<uint8_t>(out + code_bytes + c / mx4::kBlockColumns) = static_cast<uint8_t>(x);
        }
        if (row_ok && lig == 0)
            for (int b = tail; b < dst_row_bytes; ++b) *as_global<uint8_t>(out + b) = 0;
    }
}

template <typename ST>
hipError_t quantize_t(const void* src, int64_t n_rows, int dim, int64_t stride, void* dst, hipStream_t stream) {
    const int G = group_lanes(dim, Elem<ST>::kVec);
    const int64_t blocks = ceil_div(n_rows, static_cast<int64_t>(kBlock / G));
    const unsigned grid = static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20));
    hipLaunchKernelGGL((mx4_rows_quantize_kernel<ST>), dim3(grid), dim3(kBlock), 0, stream, static_cast<const char*>(src), n_rows, dim,
                       stride * SrcBytes<ST>::value, G, static_cast<char*>(dst));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rows_quantize_mx4(const void* src, int src_dtype, int64_t n_rows, int dim, int64_t stride, void* dst, hipStream_t stream) {
    if (src_dtype == PM_BF16) return quantize_t<bf16_t>(src, n_rows, dim, stride, dst, stream);
    if (src_dtype == PM_F16) return quantize_t<f16_t>(src, n_rows, dim, stride, dst, stream);
    return quantize_t<float>(src, n_rows, dim, stride, dst, stream);
}

}  // namespace pm
