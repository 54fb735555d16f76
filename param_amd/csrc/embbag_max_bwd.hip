// param_amd/csrc/embbag_max_bwd.hip -- the DIRECT backward of a MAX-pooled forward (pm_embbag_max_bwd, include/param_amd.h: MAX POOLING,
// DIRECT BACKWARD): grad(t, b)[c] goes to row max_indices(t, b)[c] of table t, read from the [B, sum D]-sized
// gradient through max_indices.  No [N, D] expansion, no bag_of array, no position-to-bag search.
//
// Input: the pooled, unweighted key sort of the request (pm_embbag_sort_indices): pairs (key = table << tshift | row, value = bag within
// the table), equal keys adjacent -- a RUN -- and ascending bags inside a run; the pair count is on the device.  A bag that holds a row
// twice is two adjacent pairs of one value: the repeat is skipped, so a bag counts once.
//
// max_bwd_kernel (one workgroup per tile of kMbTile sorted pairs):
//   1. the tile's keys and values, and the pair in front of it, go into LDS with coalesced loads;
//   2. a run that crosses into the tile has its start found by one lane (a galloping search backwards through the sorted keys);
//   3. every position is tested: a run HEAD (key != the key in front) or a PIECE START (a multiple of kExactRun pairs behind its run's
//      start) becomes a work item in an LDS list;
//   4. lane groups of G = group_lanes(max_dim, 4) lanes take items in turn.  An item is at most kExactRun pairs of one run; the group walks
//      on in global memory where the item leaves the tile.  Per pair a lane loads max_indices (16 bytes) and grad (16 / 8 bytes) of the pair's
//      bag at its four columns, four pairs' loads in flight; the adds are ordered: acc = hit ? (won ? acc + g : g) : acc;
//   5. a head whose run ends within kExactRun pairs is finished by its group: the destination's four columns are loaded, the won columns
//      updated and stored.  One row, one owner, no atomics on a destination.  Any other item -- a piece of a HOT run -- leaves its fp32
//      partial and won mask in a workspace slot that its position names, and a hot run's head is appended to a list (the one atomic: a
//      counter that orders nothing the result depends on).
// max_bwd_combine_kernel (second launch, small): a lane group per listed hot run adds the run's pieces in ascending order and updates
//   the destination the same way.
//
// The association is a function of the request alone: the pieces of a run are cut every kExactRun PAIRS from the run's start, whatever
// the tile size, the grid or the order in which workgroups run.
#include "common.h"
#include "bwd_sorted_apply.h"      // kExactRun; fwd_elem.h: the library's one rounding of a 16-bit destination

namespace pm {
namespace {

constexpr int kMbTile = 1024;                    // sorted pairs per workgroup
constexpr int kMbPerThread = kMbTile / kBlock;
constexpr int kMbInFlight = 4;                   // pairs whose loads a lane keeps in flight
constexpr uint32_t kNoBag = 0xffffffffu;         // batch < 2^32: no bag has this number
constexpr uint64_t kNoKey = ~static_cast<uint64_t>(0);     // a key has one spare bit: no pair has this key

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
using fwd::u32x2;

struct MaxBwdArgs {
    const void* keys;            // sorted keys, uint32 or uint64 (key64)
    const uint32_t* vals;        // bag within the table
    const uint32_t* d_count;     // device: pairs in the sorted arrays
    uint32_t* ctl;               // device: hot runs listed (zeroed by the sort's first kernel)
    uint32_t* hot;               // first sorted position of every hot run, in no particular order
    float* slots;                // a piece's partial: slot_stride words, D floats then D / 4 won masks
    const void* grad;
    const int32_t* arg;
    void* const* dst;
    const int32_t* dims;
    const int64_t* out_offsets;
    int64_t out_stride;
    uint32_t n_max;              // num_indices: the pair count is clamped to it
    int32_t key64, tshift, gshift;
    int64_t slot_stride;
    float alpha;
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

// dst[row, c .. c + 4) of table `base` (row-major, D columns): the won columns become round(widen(dst) + alpha * sum) -- one
// multiplication, one addition --, the others are not stored (fp32) or packed back as read (16-bit).  Nothing won: nothing is read.
// DD: the destination's element, 0 fp32 / 1 bf16 / 2 fp16
template <int DD>
__device__ __forceinline__ void update_row4(void* base, int64_t elem, const f32x4& sum, uint32_t won, float alpha) {
    if (won == 0) return;
    if constexpr (DD == 0) {
        PM_GLOBAL float* d = as_global<float>(base) + elem;
        const f32x4 old = *reinterpret_cast<PM_GLOBAL f32x4*>(d);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float step = alpha * sum[k];
            if (won & (1u << k)) d[k] = old[k] + step;
        }
    } else {
        PM_GLOBAL u32x2* d = reinterpret_cast<PM_GLOBAL u32x2*>(as_global<uint16_t>(base) + elem);
        const u32x2 old = *d;
        uint32_t q[4] = {old[0] & 0xffffu, old[0] >> 16, old[1] & 0xffffu, old[1] >> 16};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float w = DD == 1 ? __uint_as_float(q[k] << 16) : static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(q[k])));
            const float step = alpha * sum[k];
            const float v = w + step;
            const uint32_t r = DD == 1 ? fwd::OutBF16::round(v) : fwd::OutF16::round(v);
            q[k] = (won & (1u << k)) ? (r & 0xffffu) : q[k];
        }
        u32x2 out;
        out[0] = q[0] | (q[1] << 16);
        out[1] = q[2] | (q[3] << 16);
        *d = out;
    }
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

template <int DD, int GD>
__global__ void __launch_bounds__(kBlock) max_bwd_kernel(const MaxBwdArgs a) {
    __shared__ uint64_t s_key[kMbTile + 1];
    __shared__ uint32_t s_val[kMbTile + 1];
    __shared__ uint32_t s_item[kMbTile];
    __shared__ uint32_t s_nitem, s_cross;
    const uint32_t n_dev = *a.d_count;
    const uint32_t n = n_dev < a.n_max ? n_dev : a.n_max;
    const uint64_t t0_64 = static_cast<uint64_t>(blockIdx.x) * kMbTile;
    if (t0_64 >= n) return;
    const uint32_t t0 = static_cast<uint32_t>(t0_64);
    const uint32_t len = n - t0 < static_cast<uint32_t>(kMbTile) ? n - t0 : kMbTile;
    const int tid = static_cast<int>(threadIdx.x);

    // 1. the tile and the pair in front of it
    for (uint32_t i = tid; i < len; i += kBlock) {
        s_key[1 + i] = load_key(a.keys, t0 + i, a.key64);
        s_val[1 + i] = as_global<uint32_t>(a.vals)[t0 + i];
    }
    if (tid == 0) {
        s_key[0] = t0 > 0 ? load_key(a.keys, t0 - 1, a.key64) : kNoKey;
        s_val[0] = t0 > 0 ? as_global<uint32_t>(a.vals)[t0 - 1] : kNoBag;
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
    for (int u = 0; u < kMbPerThread; ++u) {
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
        uint32_t cnt = 1;
        const uint32_t room = n - gp;      // pairs from gp to the end of the sorted arrays (at least one)
        while (cnt < static_cast<uint32_t>(kExactRun) && cnt < room && pv.key(gp + cnt) == key0) ++cnt;
        const bool more = cnt == static_cast<uint32_t>(kExactRun) && cnt < room && pv.key(gp + cnt) == key0;
        const bool piece = !head || more;      // part of a hot run
        const int t = static_cast<int>(key0 >> a.tshift);
        const int64_t row = static_cast<int64_t>(key0 & rmask);
        const int D = a.dims[t];
        const int64_t goff = a.out_offsets[t];
        const uint32_t b_first = pv.val(gp);
        const uint32_t b_before = head ? kNoBag : pv.val(gp - 1);      // a piece's first pair may repeat the bag of the pair in front
        if (piece && head && lig == 0) a.hot[atomicAdd(a.ctl, 1u)] = gp;
        for (int c4 = lig; c4 < D / 4; c4 += G) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            uint32_t won = 0, pb = b_before;
            for (uint32_t j0 = 0; j0 < cnt; j0 += kMbInFlight) {
                uint32_t b[kMbInFlight];
                i32x4 av[kMbInFlight];
                f32x4 gv[kMbInFlight];
#pragma unroll
                for (int u = 0; u < kMbInFlight; ++u) {
                    b[u] = j0 + u < cnt ? pv.val(gp + j0 + u) : b_first;      // (past the item: a bag that exists, its loads unused)
                    const int64_t e = goff + static_cast<int64_t>(b[u]) * a.out_stride + c4 * 4;
                    av[u] = *reinterpret_cast<const PM_GLOBAL i32x4*>(as_global<int32_t>(a.arg) + e);
                    gv[u] = load_grad4<GD>(a.grad, e);
                }
#pragma unroll
                for (int u = 0; u < kMbInFlight; ++u) {
                    const bool fresh = j0 + u < cnt && b[u] != pb;
                    pb = j0 + u < cnt ? b[u] : pb;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool hit = fresh && static_cast<int64_t>(av[u][k]) == row;
                        const float next = (won & (1u << k)) ? acc[k] + gv[u][k] : gv[u][k];
                        acc[k] = hit ? next : acc[k];
                        won |= hit ? (1u << k) : 0u;
                    }
                }
            }
            if (!piece) {
                update_row4<DD>(a.dst[t], row * D + c4 * 4, acc, won, a.alpha);
            } else {
                PM_GLOBAL float* s = as_global<float>(a.slots) + piece_slot(gp, head) * a.slot_stride;
                *reinterpret_cast<PM_GLOBAL f32x4*>(s + c4 * 4) = acc;
                reinterpret_cast<PM_GLOBAL uint32_t*>(s)[D + c4] = won;
            }
        }
    }
}

// a lane group per listed hot run: its pieces in ascending order, then the destination
template <int DD>
__global__ void __launch_bounds__(kBlock) max_bwd_combine_kernel(const MaxBwdArgs a) {
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
            f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
            uint32_t won = 0;
            for (uint64_t pos = s0; pos < n && load_key(a.keys, static_cast<uint32_t>(pos), a.key64) == key0; pos += kExactRun) {
                const PM_GLOBAL float* s = as_global<float>(a.slots) + piece_slot(static_cast<uint32_t>(pos), pos == s0) * a.slot_stride;
                const f32x4 part = *reinterpret_cast<const PM_GLOBAL f32x4*>(s + c4 * 4);
                const uint32_t pw = reinterpret_cast<const PM_GLOBAL uint32_t*>(s)[D + c4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float next = (won & (1u << k)) ? sum[k] + part[k] : part[k];
                    sum[k] = (pw & (1u << k)) ? next : sum[k];
                }
                won |= pw;
            }
            update_row4<DD>(a.dst[t], row * D + c4 * 4, sum, won, a.alpha);
        }
    }
}

template <int DD>
hipError_t launch_dd(const MaxBwdArgs& a, int grad_dtype, unsigned grid, unsigned combine_grid, hipStream_t stream) {
    const dim3 blk(kBlock);
    if (grad_dtype == PM_F32) hipLaunchKernelGGL((max_bwd_kernel<DD, 0>), dim3(grid), blk, 0, stream, a);
    else if (grad_dtype == PM_BF16) hipLaunchKernelGGL((max_bwd_kernel<DD, 1>), dim3(grid), blk, 0, stream, a);
    else hipLaunchKernelGGL((max_bwd_kernel<DD, 2>), dim3(grid), blk, 0, stream, a);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess || combine_grid == 0) return rc;
    hipLaunchKernelGGL((max_bwd_combine_kernel<DD>), dim3(combine_grid), blk, 0, stream, a);
    return hipGetLastError();
}

size_t a256(size_t x) { return (x + 255) / 256 * 256; }
size_t hot_list_bytes(int64_t n) { return a256(4 * (static_cast<size_t>(n) / kExactRun + 1)); }
int64_t slot_words(int max_dim) { return static_cast<int64_t>(max_dim) + max_dim / 4; }

}  // namespace

// behind the sorted backward's workspace: the hot-run list, then two slots per kExactRun sorted positions
size_t max_bwd_extra_bytes(int64_t n, int max_dim) {
    return hot_list_bytes(n) + a256(2 * (static_cast<size_t>(n) / kExactRun + 1) * static_cast<size_t>(slot_words(max_dim)) * 4);
}

// p: base parameters of the request (p.tables = the destinations); mp: the sorted pairs of the request's sort; extra: max_bwd_extra_bytes
hipError_t launch_max_bwd(const KParams& p, int max_dim, const MaxBwdPairs& mp, void* extra, const void* grad, int grad_dtype,
                          const int32_t* max_indices, int dst_dtype, float alpha, hipStream_t stream) {
    const int G = group_lanes(max_dim, 4);
    MaxBwdArgs a;
    a.keys = mp.keys;
    a.vals = mp.vals;
    a.d_count = mp.d_count;
    a.ctl = mp.ctl;
    a.hot = static_cast<uint32_t*>(extra);
    a.slots = reinterpret_cast<float*>(static_cast<char*>(extra) + hot_list_bytes(p.N));
    a.grad = grad;
    a.arg = max_indices;
    a.dst = const_cast<void* const*>(p.tables);
    a.dims = p.dims;
    a.out_offsets = p.out_offsets;
    a.out_stride = p.out_stride;
    a.n_max = static_cast<uint32_t>(p.N);
    a.key64 = mp.key_bytes == 8 ? 1 : 0;
    a.tshift = mp.tshift;
    a.gshift = 3;
    while ((1 << a.gshift) < G) ++a.gshift;
    a.slot_stride = slot_words(max_dim);
    a.alpha = alpha;
    const int64_t grid = (p.N + kMbTile - 1) / kMbTile;
    if (grid < 1 || grid > kMaxGrid) return hipErrorInvalidConfiguration;
    // a hot run has more than kExactRun pairs: none in a request of at most that many, else a group per possible run up to 1024 workgroups
    const int64_t max_hot = p.N / (kExactRun + 1);
    const int64_t per_block = kBlock >> a.gshift;
    int64_t cgrid = (max_hot + per_block - 1) / per_block;
    if (cgrid > 1024) cgrid = 1024;
    const unsigned g = static_cast<unsigned>(grid), cg = static_cast<unsigned>(cgrid);
    if (dst_dtype == PM_F32) return launch_dd<0>(a, grad_dtype, g, cg, stream);
    if (dst_dtype == PM_BF16) return launch_dd<1>(a, grad_dtype, g, cg, stream);
    return launch_dd<2>(a, grad_dtype, g, cg, stream);
}

}  // namespace pm
