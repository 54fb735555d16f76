// param_amd/csrc/bwd_sorted_alt.inc -- the sorted backward's measured alternatives and cross-checks: everything of
// embbag_bwd_sorted.hip that exists in the ALTERNATES build only (make alt, -DPM_ALTERNATES: libparam_amd_alt.so, tests/ and tools/).
// Included by embbag_bwd_sorted.hip, at file scope, from its one PM_ALTERNATES block; the #else of that block holds the product's stubs.
//
// Round 2's pipeline (sort_impl 2; sort_impl 1 swaps its sort for rocPRIM's radix_sort_pairs):
//   1. builds one (table,row) key and one bag value per lookup          (build_keys_kernel)
//   2. sorts the pairs with a stable LSD radix sort by the ROW bits only (radix_sort.hip: own kernels, 3 passes of 8 bits
//      for 10 M-row tables).  The request is table-major, so after a stable sort by row the lookups of one (table, row)
//      are still contiguous and in lookup order -- the order is (row, table, position), which is all step 3 needs: it
//      finds runs by key equality.  (Sorting the table bits too would be a fourth pass for nothing.)
//   3. the sorted apply of embbag_bwd_sorted.hip, unchanged.
// The product library sorts with seg_sort.hip -- per-table segments established on the device -- and forms its keys itself.
#include <rocprim/device/device_radix_sort.hpp>

namespace pm {
namespace {

// step 1: keys / values, same tiling and LDS offset staging as the forward
template <typename K, bool WEIGHTED>
__global__ void __launch_bounds__(kBlock) build_keys_kernel(const KParams p, K* keys, uint32_t* vals,
                                                            uint32_t* bag_of, int rbits, int tshift, int kbits,
                                                            int64_t phase_bags, int64_t slice_begin, int64_t slice_end) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int t, tile;
    block_to_tile(p, t, tile);
    if (t >= p.T) return;
    const int64_t bag0 = static_cast<int64_t>(tile) * p.bags_per_block;  // p.bag_begin == 0 here: whole batch
    const int64_t left = p.B - bag0;
    const int nb = left < p.bags_per_block ? static_cast<int>(left) : p.bags_per_block;
    const int64_t g0 = static_cast<int64_t>(t) * p.B + bag0;
    int64_t* s_off = reinterpret_cast<int64_t*>(smem);
    for (int i = threadIdx.x; i <= nb; i += kBlock) s_off[i] = bag_start_or_end(p, g0 + i);
    __syncthreads();
    const int64_t base = s_off[0];
    const int64_t end = s_off[nb];
    const K pad = static_cast<K>(1) << kbits;
    for (int64_t j = base + threadIdx.x; j < end; j += kBlock) {
        // bag of lookup j: largest b with s_off[b] <= j (binary search over the LDS offsets)
        int lo = 0, hi = nb;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= j) lo = mid; else hi = mid;
        }
        const int64_t bag = bag0 + lo;
        const K row = static_cast<K>(load_index(p.indices, j, p.idx64));
        const bool in_slice = bag >= slice_begin && bag < slice_end;
        // (table, bag phase, row): phase = which run of phase_bags consecutive bags the lookup belongs to (0 everywhere when
        // the apply runs in one phase); the phase sits between table and row so that a (table, phase) segment sorts by row
        const K phase = phase_bags > 0 ? static_cast<K>(bag / phase_bags) : static_cast<K>(0);
        keys[j] = in_slice ? ((static_cast<K>(t) << tshift) | (phase << rbits) | row) : pad;
        if (WEIGHTED) {
            vals[j] = static_cast<uint32_t>(j);
            bag_of[j] = static_cast<uint32_t>(bag);
        } else {
            vals[j] = static_cast<uint32_t>(bag);
        }
    }
}

template <typename K>
hipError_t rocprim_temp_bytes(int64_t n, int kbits_sort, size_t& bytes) {
    bytes = 0;
    K* kn = nullptr;
    uint32_t* vn = nullptr;
    return rocprim::radix_sort_pairs(nullptr, bytes, kn, kn, vn, vn, static_cast<size_t>(n), 0u,
                                     static_cast<unsigned>(kbits_sort), hipStream_t(0));
}

// Backward tuning knobs of the alternatives (pm_set_backward_tuning; -1 = default, which the environment can override once):
//   sort_impl  0 (default) the segmented sort of round 3 (seg_sort.hip: per-table segments established on the device);
//              1 rocPRIM radix_sort_pairs (PARAM_AMD_SORT=rocprim); 2 round 2's own LSD sort with host-side plans (radix_sort.hip,
//              PARAM_AMD_SORT=legacy) -- both kept as measured alternatives and as independent checks of the product's path
//   order      1 (table, [phase,] row, position) -- default --, 0 (row, table, position):   PARAM_AMD_SORT_ORDER=row
//              only the row bits are sorted (one pass fewer; the apply kernel then runs 5 % slower and cannot be XCD-affine)
std::atomic<int> g_sort_impl{-1}, g_sort_order{-1}, g_max_phases{-1};
void set_alt_tuning(int sort_impl, int order, int max_phases_) {
    g_sort_impl.store(sort_impl);
    g_sort_order.store(order);
    g_max_phases.store(max_phases_);
}
int sort_impl_knob() { return knob(g_sort_impl, [] { return env_is("PARAM_AMD_SORT", "rocprim") ? 1 : env_is("PARAM_AMD_SORT", "legacy") ? 2 : 0; }); }
// round 2's sort (sort_impl 2, a measured alternative and cross-check) only: the default segmented sort's make_plan never gets to
// legacy_plan, so no default launch path reads the environment; tests flip it between two plans of one process
bool fused_keys_allowed() { return !env_is("PARAM_AMD_SORT_FUSED_KEYS", "0"); }
bool table_major_order() { return knob(g_sort_order, [] { return env_is("PARAM_AMD_SORT_ORDER", "row") ? 0 : 1; }) == 1; }
//   max_phases 1 (default): one apply launch; 2: a phases = 2 sort lays a fixed-pooling request out for the two-phase
//              apply (measured at benchmark size: uniform indices 1.60 -> 1.58 ms, Zipf 0.97 -> 1.12 ms: rows looked up in
//              both bag halves are read and written twice, and halving the gradient working set does not make it stay in
//              L2 -- 1 KB of row traffic streams through for every 512 B gradient row)              PARAM_AMD_BWD_PHASES=2
int max_phases() { return knob(g_max_phases, [] { return env_is("PARAM_AMD_BWD_PHASES", "2") ? 2 : 1; }); }

// the temp bytes the alternative sorts need behind the pairs (the workspace holds the largest of these and the segmented sort's)
hipError_t alt_temp_bytes(int64_t n, int, int key_bytes, int kbits_sort, size_t& tb) {
    hipError_t rc = key_bytes == 4 ? rocprim_temp_bytes<uint32_t>(n, kbits_sort > 32 ? 32 : kbits_sort, tb)
                                   : rocprim_temp_bytes<uint64_t>(n, kbits_sort, tb);
    if (rc != hipSuccess) return rc;
    const size_t own = rs_scratch_bytes(static_cast<size_t>(n));
    if (own > tb) tb = own;
    return hipSuccess;
}

// The plan of sort_impl 1 / 2 (and of more than kSegSortMaxTables tables), over make_plan's fixed assignments:
// key = (table << tshift) | (phase << rbits) | row, padding keys (batch slices only) = 1 << kbits.
//   fixed pooling (every bag L lookups, op->fixed_pooling = L) and a whole-batch request make the table-major request a
//   sequence of T * H equal segments of seg_len = (B / H) * L lookups, H = bag phases.  If seg_len is a multiple of the
//   sort tile the own sort orders every segment on its own by the ROW bits only (3 passes of 8 bits for 10 M rows: the
//   table and phase bits need no pass); if it is a multiple of the apply tile the apply kernel can run XCD-affine and
//   in H launches.  Everything else (ragged bags, slices, odd sizes) sorts all key bits globally and applies in one launch.
void legacy_plan(const KParams& p, int64_t fixed_pooling, int phases, SortPlan& g) {
    const bool fixed = fixed_pooling > 0 && !g.sliced && p.T >= 1 && p.B > 0 &&
                       fixed_pooling * p.B * static_cast<int64_t>(p.T) == p.N;
    g.H = 1;
    if (phases == 2 && max_phases() >= 2 && fixed && table_major_order() && p.B % 2 == 0 && ((p.B / 2) * fixed_pooling) % kSortTile == 0) g.H = 2;
    g.hbits = g.H == 2 ? 1 : 0;
    g.tshift = g.rbits + g.hbits;
    g.kbits = g.tshift + bits_for(p.T);
    g.key_bytes = (g.kbits + 1 <= 32) ? 4 : 8;
    g.phase_bags = g.H == 2 ? p.B / 2 : 0;
    g.seg_len = fixed ? (p.B / g.H) * fixed_pooling : 0;
    g.seg_tiles = (fixed && table_major_order() && g.seg_len % kSortTile == 0) ? static_cast<int32_t>(g.seg_len / kSortTile) : 0;
    // (one workgroup walks a segment's tile counts: beyond a few thousand tiles per segment the global scan is the faster one)
    g.segmented = fixed && table_major_order() && !g.rocprim && g.seg_len > 0 && g.seg_len % 4096 == 0 && g.seg_len / 4096 <= 4096;
    g.xcd = want_xcd() && g.seg_tiles > 0 && p.T > 1;
    if (g.sliced) g.sort_end_bit = g.kbits + 1;                  // padding keys must end up last
    else if (g.segmented) g.sort_end_bit = g.rbits;              // per (table, phase) segment: rows only
    else g.sort_end_bit = table_major_order() ? g.kbits : g.rbits;
    g.in_b = g.rocprim || (rs_num_passes(0, g.sort_end_bit) % 2 == 1);
    g.fused_keys = g.segmented && g.H == 1 && !g.weighted && !g.sliced && g.sort_end_bit > 0 && fused_keys_allowed();
}

template <typename K>
hipError_t legacy_sort(const KParams& p, const SortPlan& g, SortWs& ws, hipStream_t stream) {
    K* ka = reinterpret_cast<K*>(ws.keys_a);
    K* kb = reinterpret_cast<K*>(ws.keys_b);
    KParams q = p;
    q.bag_begin = 0;
    q.bag_count = p.B;
    q.tiles_per_table = static_cast<int32_t>((p.B + p.bags_per_block - 1) / p.bags_per_block);
    q.xcd_affine = 0;
    const int grid = q.T * q.tiles_per_table;
    const size_t lds = static_cast<size_t>(q.bags_per_block + 2) * sizeof(int64_t);
    // the apply's work-list control words start at zero (the segmented sort's first kernel does this itself)
    hipError_t zrc = hipMemsetAsync(ws.fix_ctl, 0, 4 * sizeof(uint32_t), stream);
    if (zrc != hipSuccess) return zrc;
    const int64_t s0 = p.bag_begin, s1 = p.bag_begin + p.bag_count;
    // per-table segments of a fixed-pooling request, one phase, no weights: bag and table of a lookup follow from its
    // position, so the first radix pass forms the pairs itself from the index array and no key-building kernel runs
    // (33 us and 126 MB of the benchmark step's 190 us sort; PARAM_AMD_SORT_FUSED_KEYS=0 restores it)
    if (g.fused_keys) {
        const RsSource src{p.indices, p.idx64, g.tshift, static_cast<uint32_t>(g.seg_len / p.B)};
        return rs_sort_pairs<K>(ka, kb, ws.vals_a, ws.vals_b, static_cast<size_t>(p.N), nullptr, 0, g.sort_end_bit, ws.temp, stream,
                                static_cast<size_t>(g.seg_len), &src);
    }
    if (g.weighted)
        hipLaunchKernelGGL((build_keys_kernel<K, true>), dim3(grid), dim3(kBlock), lds, stream, q, ka, ws.vals_a,
                           ws.bag_of, g.rbits, g.tshift, g.kbits, g.phase_bags, s0, s1);
    else
        hipLaunchKernelGGL((build_keys_kernel<K, false>), dim3(grid), dim3(kBlock), lds, stream, q, ka, ws.vals_a,
                           ws.bag_of, g.rbits, g.tshift, g.kbits, g.phase_bags, s0, s1);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    size_t tb = ws.temp_bytes;
    // stable LSD radix sort.  rocPRIM leaves the result in keys_b / vals_b, the own sort in the b buffers iff its pass
    // count is odd (plan.in_b).
    if (g.rocprim)
        return rocprim::radix_sort_pairs(ws.temp, tb, ka, kb, ws.vals_a, ws.vals_b, static_cast<size_t>(p.N), 0u,
                                         static_cast<unsigned>(g.sort_end_bit), stream);
    return rs_sort_pairs<K>(ka, kb, ws.vals_a, ws.vals_b, static_cast<size_t>(p.N), nullptr, 0, g.sort_end_bit, ws.temp, stream,
                            g.segmented ? static_cast<size_t>(g.seg_len) : 0);
}

std::string legacy_plan_describe(const SortPlan& g) {
    const int passes = g.rocprim ? -1 : rs_num_passes(0, g.sort_end_bit);
    char buf[640];
    snprintf(buf, sizeof(buf),
             "sort=%s key_bytes=%d rbits=%d hbits=%d kbits=%d sort_bits=%d passes=%d segmented=%d seg_len=%lld phases=%d "
             "apply_seg_tiles=%d xcd=%d sliced=%d weighted=%d result_in_b=%d fused_keys=%d",
             g.rocprim ? "rocprim" : "own", g.key_bytes, g.rbits, g.hbits, g.kbits, g.sort_end_bit, passes, g.segmented ? 1 : 0,
             static_cast<long long>(g.segmented ? g.seg_len : 0), g.H, (g.xcd || g.H > 1) ? g.seg_tiles : 0, g.xcd ? 1 : 0,
             g.sliced ? 1 : 0, g.weighted ? 1 : 0, g.in_b ? 1 : 0, g.fused_keys ? 1 : 0);
    return buf;
}

}  // namespace
}  // namespace pm
