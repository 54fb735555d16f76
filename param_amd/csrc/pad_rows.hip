// param_amd/csrc/pad_rows.hip -- the two small kernels that keep padding rows out of the backward:
//   pad_guard_kernel   saves / restores every table's padding row (and its optimizer state) around an UNCHANGED backward call
//                      (pm_pad_rows_guard): the apply kernels and the Adagrad update functions keep their code, and whatever they
//                      wrote into a padding row -- scatter-add, decay, stochastic rounding -- is undone bit for bit
//   pad_mask_kernel    writes +0.0 over the per_sample_weights gradient of the padded lookups (pm_embbag_pad_mask)
#include "common.h"

namespace pm {
namespace {

// One wave per table; 16-byte vector copies (a row is a whole number of them: dims[t] is a multiple of 4 fp32 / 8 16-bit
// elements and rows are 16-byte aligned).  Slot t of the stash: [row: dims[t] * elem_bytes][state] with the state at
// row_slot_bytes; state_kind 1: one fp32 (row-wise Adagrad), 2: dims[t] fp32 (element-wise Adagrad).
__global__ void __launch_bounds__(kWave) pad_guard_kernel(void* const* tables, const int32_t* dims, const int64_t* pad_idx,
                                                          float* const* state, int state_kind, int elem_bytes, char* stash,
                                                          int64_t slot_bytes, int64_t row_slot_bytes, int restore) {
    const int t = blockIdx.x;
    const int64_t pad = pad_idx[t];
    if (pad < 0) return;
    const int D = dims[t];
    char* slot = stash + static_cast<int64_t>(t) * slot_bytes;
    {
        const int nvec = D * elem_bytes / 16;
        PM_GLOBAL u32x4* row = as_global<u32x4>(static_cast<char*>(tables[t]) + pad * D * elem_bytes);
        PM_GLOBAL u32x4* keep = as_global<u32x4>(slot);
        for (int i = threadIdx.x; i < nvec; i += kWave) {
            if (restore) row[i] = keep[i]; else keep[i] = row[i];
        }
    }
    if (state_kind == 1) {
        if (threadIdx.x == 0) {
            PM_GLOBAL float* m = as_global<float>(state[t]) + pad;
            PM_GLOBAL float* keep = as_global<float>(slot + row_slot_bytes);
            if (restore) *m = *keep; else *keep = *m;
        }
    } else if (state_kind == 2) {
        const int nvec = D / 4;
        PM_GLOBAL u32x4* row = as_global<u32x4>(state[t] + pad * D);
        PM_GLOBAL u32x4* keep = as_global<u32x4>(slot + row_slot_bytes);
        for (int i = threadIdx.x; i < nvec; i += kWave) {
            if (restore) row[i] = keep[i]; else keep[i] = row[i];
        }
    }
}

// One thread per lookup j: its table is the last t whose first bag starts at or before j (bounds_check.hip's table_of, on the
// request's own offsets); inside the table's bag slice, a lookup of the padding index gets +0.0.
__global__ void __launch_bounds__(kBlock) pad_mask_kernel(const KParams p, const int64_t* pad_idx, float* values) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (j >= p.N) return;
    int lo = 0, hi = p.T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (load_index(p.offsets, static_cast<int64_t>(mid) * p.B, p.idx64) <= j) lo = mid; else hi = mid;
    }
    const int t = lo;
    const int64_t pad = pad_idx[t];
    if (pad < 0) return;
    const int64_t g0 = static_cast<int64_t>(t) * p.B + p.bag_begin;
    if (j < bag_start_or_end(p, g0) || j >= bag_start_or_end(p, g0 + p.bag_count)) return;
    if (load_index(p.indices, j, p.idx64) == pad) values[j] = 0.0f;
}

}  // namespace

hipError_t launch_pad_guard(int T, void* const* tables, const int32_t* dims, int elem_bytes, const int64_t* pad_idx,
                            float* const* state, int state_kind, void* stash, int64_t slot_bytes, int64_t row_slot_bytes,
                            bool restore, hipStream_t stream) {
    hipLaunchKernelGGL(pad_guard_kernel, dim3(static_cast<unsigned>(T)), dim3(kWave), 0, stream, tables, dims, pad_idx, state,
                       state_kind, elem_bytes, static_cast<char*>(stash), slot_bytes, row_slot_bytes, restore ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_pad_mask(const KParams& p, const int64_t* pad_idx, float* values, hipStream_t stream) {
    const int64_t grid = (p.N + kBlock - 1) / kBlock;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(pad_mask_kernel, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0, stream, p, pad_idx, values);
    return hipGetLastError();
}

}  // namespace pm
