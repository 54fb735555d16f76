// param_amd/csrc/embbag_bwd_sorted_kernels.inc -- step 3 of the sorted backward (included by
// embbag_bwd_sorted.hip inside namespace pm::{anonymous}).
//
// The sorted (key, bag) pairs are cut into CHUNKS of C consecutive positions; one group of G
// lanes owns one chunk and touches exactly its C positions, whatever the skew of the keys
// (a Zipf head row may be looked up thousands of times per step: walking such a run with one
// group serialises thousands of dependent-latency round trips; sweep r1c measured 9.6 ms).
//
//   main kernel    runs lying entirely inside a chunk: destination row read once, the run's
//                  gradient rows added in sorted (= lookup) order in fp32, row written once.
//                  A run of <= kExactRun lookups that crosses a chunk boundary INSIDE the workgroup's tile
//                  is applied the same way by the group holding its head, whose walk runs on past the end
//                  of its chunk; the groups to its right skip their piece.  Other crossing runs (leaving
//                  the tile, or longer) are NOT applied here: each chunk writes the fp32 partial sum of its
//                  piece to a scratch slot (lead / trail) and the piece lengths to a per-chunk record.
//   fix-up kernel  one group per chunk holding the HEAD of such a run: short runs (<= kExactRun lookups)
//                  are re-walked sequentially (bit-identical to the sequential oracle, like in-chunk
//                  runs); longer ones add the chunk partials in chunk order (deterministic; differs from
//                  the sequential order by rounding).
//                  Every short crossing run used to be re-walked here: serial chains that made the fix-up
//                  189 us under Zipf (58 us with none).  Moving them into extra blocks of the main kernel cost
//                  +200 us there (each such run was then read twice); owner-applies-once with scans and
//                  walks through global memory pushed the main kernel past 100 VGPRs (4 waves/SIMD instead
//                  of 5: +85 us).  Keeping it to the tile -- LDS only -- costs neither.  (gpurun s6/s7)
// Both kernels are free of atomics and of inter-workgroup hand-offs (kernel boundary between them).
//
// OPT selects what happens to a row once its gradient is complete:
//   0  scatter-add / SGD:  row += alpha * (sum of psw * g), accumulated ON TOP of the row in lookup order
//   1  exact row-wise Adagrad (the fused optimizer the reference configures for its TBE ops,
//      train/comms/pt/comms_utils.py:2014 EXACT_ROWWISE_ADAGRAD; algorithm as published by fbgemm_gpu):
//          G   = sum over the row's lookups of psw * g            (fp32, lookup order, from zero)
//          m  += (sum_d G[d]^2) / D                                (one fp32 state value per row)
//          row -= lr / (sqrt(m) + eps) * G
//      optional weight decay (L2 / decoupled) and, for 16-bit tables, stochastic rounding of the updated row
//      (the options the reference's TBE operator passes: split_table_batched_embeddings_ops.py:289-300)
//      the sum of squares is a per-lane partial reduced across the G lanes of the group with
//      wave shuffles (xor butterfly), so every lane of the group must take part: one column pass only
//      (max_dim <= G * VEC, checked by the launcher).
//   2  exact element-wise Adagrad (fbgemm's EXACT_ADAGRAD, the optimizer the reference's own TBE unit test builds with;
//      torch.optim.Adagrad's arithmetic): G as for 1, one fp32 state value per WEIGHT ([rows, D] beside the table), finished
//      per lane (adagrad_elem_finish below).  The state's 16 (fp32 tables) / 2 x 16 (16-bit tables) bytes per lane ride with the
//      row's load and leave with its store.  Same launch rules as 1 (one column pass, H == 1, no tile join when weighted).

// (register budget: the fp32 scatter-add instance compiles to 82-86 VGPRs = 5 waves per SIMD without being told to.
//  Forcing 6 waves -- __launch_bounds__(kBlock, 6): 80 VGPRs, 4-38 spilled -- measured Zipf apply 0.97 -> 0.94 ms but
//  uniform 1.60 -> 1.64 ms; forcing 5 on every instance made the 16-bit / Adagrad instances spill: bf16 step 1.39 -> 2.43 ms.)
// finish one row under row-wise Adagrad; called by ALL lanes of the group (acc is zero where c >= D).
// Weight decay as in fbgemm's rowwise_adagrad: L2 adds wd * w to the gradient inside the sum of squares and shrinks
// the row by (1 - mult * wd); decoupled shrinks it by (1 - lr * wd); the raw gradient sum is what gets subtracted.
template <typename DST, int G>
__device__ __forceinline__ void adagrad_finish(char* wptr, float (&wrow)[DST::kVec], const float (&acc)[DST::kVec],
                                               bool any_col, float* mom_row, float mom_prev, int D, const SortedParams& p,
                                               int lig, int nt_rows, uint64_t rowkey, int c) {
    float ss = 0.0f;
    if (p.wd_mode == PM_WD_L2) {
#pragma unroll
        for (int k = 0; k < DST::kVec; ++k) {
            // (a lane past the table's width loaded no row: its wrow is what an earlier, WIDER table's row left there in a
            // mixed-dim request, and counted into this row's sum of squares it inflated the state of every narrower table's rows)
            const float reg = any_col ? p.wd * wrow[k] : 0.0f;
            const float gx = acc[k] + reg;
            ss = ss + gx * gx;
        }
    } else {
#pragma unroll
        for (int k = 0; k < DST::kVec; ++k) ss = ss + acc[k] * acc[k];
    }
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) ss = ss + __shfl_xor(ss, off, G);
    const float m = mom_prev + ss / static_cast<float>(D);   // the state was fetched with the row, not here
    if (lig == 0) hidden_store4(mom_row, m);
    const float mult = p.lr / (sqrtf(m) + p.eps);
    if (any_col) {
        if (p.wd_mode != PM_WD_NONE) {
            const float shrink = p.wd_mode == PM_WD_L2 ? mult * p.wd : p.lr * p.wd;
            const float corr = 1.0f - shrink;
#pragma unroll
            for (int k = 0; k < DST::kVec; ++k) {
                const float kept = corr * wrow[k];
                const float step = mult * acc[k];
                wrow[k] = kept - step;
            }
        } else {
#pragma unroll
            for (int k = 0; k < DST::kVec; ++k) {
                const float step = mult * acc[k];
                wrow[k] = wrow[k] - step;
            }
        }
        if (p.sr) DST::store_sr(wptr, wrow, nt_rows, p.sr_seed, rowkey, c);
        else DST::store(wptr, wrow, nt_rows);
    }
}

// finish one row under exact ELEMENT-wise Adagrad (OPT 2: torch.optim.Adagrad's arithmetic with initial_accumulator_value = 0 and
// lr_decay = 0; fbgemm's EXACT_ADAGRAD): one fp32 state value per weight, so a lane finishes its own VEC columns and nothing
// crosses lanes.  Called only by lanes that hold columns of the row (c < D).  `st` came in with the row's load; it leaves with
// the row's store, under the same cache policy.
//     gx = G + wd * w (L2) | G            s = s_old + gx * gx
//     w  = w - (lr * gx) / (sqrt(s) + eps)                          NONE, L2  (torch: addcdiv_(grad, std, value = -lr))
//     w  = (1 - lr * wd) * w - (lr * G) / (sqrt(s) + eps)           DECOUPLE
// (16-byte state accesses per lane and row: 1 for fp32 tables, 2 for 16-bit tables)
template <typename DST>
__device__ __forceinline__ void adagrad_elem_finish(char* wptr, float (&wrow)[DST::kVec], const float (&acc)[DST::kVec],
                                                    const float (&st)[DST::kVec], float* st_ptr, const SortedParams& p, int nt_rows,
                                                    uint64_t rowkey, int c) {
    const float keep = p.wd_mode == PM_WD_DECOUPLE ? 1.0f - p.lr * p.wd : 1.0f;
    // four columns at a time, their 16 bytes of state stored as soon as they are complete (nothing of the new state stays live)
#pragma unroll
    for (int k4 = 0; k4 < DST::kVec; k4 += 4) {
        float s_new[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k4 + j;
            const float reg = p.wd_mode == PM_WD_L2 ? p.wd * wrow[k] : 0.0f;
            const float gx = acc[k] + reg;
            const float sq = gx * gx;
            s_new[j] = st[k] + sq;
            const float denom = sqrtf(s_new[j]) + p.eps;
            const float num = p.lr * gx;
            const float step = num / denom;
            const float kept = p.wd_mode == PM_WD_DECOUPLE ? keep * wrow[k] : wrow[k];
            wrow[k] = kept - step;
        }
        raw16_store(reinterpret_cast<char*>(st_ptr + k4),
                    u32x4{__float_as_uint(s_new[0]), __float_as_uint(s_new[1]), __float_as_uint(s_new[2]), __float_as_uint(s_new[3])}, nt_rows);
    }
    if (p.sr) DST::store_sr(wptr, wrow, nt_rows, p.sr_seed, rowkey, c);
    else DST::store(wptr, wrow, nt_rows);
}
// the state values of one row's VEC columns as loaded (raw until consumed, like the row: see the main kernel's batch) ...
template <int VEC>
__device__ __forceinline__ void state_load_raw(const void* p, u32x4 (&raw)[VEC / 4], int nt_rows) {
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) raw[k] = raw16_load(reinterpret_cast<const char*>(p) + 16 * k, nt_rows);
}
// ... and as numbers
template <int VEC>
__device__ __forceinline__ void state_widen(const u32x4 (&raw)[VEC / 4], float (&st)[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) {
        st[4 * k] = __uint_as_float(raw[k].x); st[4 * k + 1] = __uint_as_float(raw[k].y);
        st[4 * k + 2] = __uint_as_float(raw[k].z); st[4 * k + 3] = __uint_as_float(raw[k].w);
    }
}

// ---- building blocks of the four apply kernels (main, fix-up, bag-major, rest) --------------------------------
// Where a kernel keeps its own text instead of calling one of these, the spot says which kernel's code the call moved
// (profiles/bwd_refactor_isa.md).
// The row's gradient is complete: the ONE place where OPT selects what happens to it.  `state`: the row's state value (OPT 1) or
// the state of this lane's columns (OPT 2); OPT 1 is called by all lanes of the group, `cols` or not.
template <typename DST, int G, int OPT>
__device__ __forceinline__ void finish_row(char* wptr, float (&wrow)[DST::kVec], float (&acc)[DST::kVec], const float (&srow)[OPT == 2 ? DST::kVec : 1],
                                           bool cols, float* state, float m_prev, int D, const SortedParams& p, int lig, int nt_rows,
                                           uint64_t rowkey, int c) {
    if constexpr (OPT == 2) {
        if (cols) adagrad_elem_finish<DST>(wptr, wrow, acc, srow, state, p, nt_rows, rowkey, c);
    } else
    if (OPT == 1) adagrad_finish<DST, G>(wptr, wrow, acc, cols, state, m_prev, D, p, lig, nt_rows, rowkey, c);
    else if (cols) DST::store(wptr, acc, nt_rows);
}
// a lane's VEC columns of one gradient row, 16 bytes per load; P carries the site's address space (const f32x4*: flat,
// as_global<f32x4>: global)
template <int VEC, typename P>
__device__ __forceinline__ void load_grad(P g, float (&gv)[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC; k += 4) {
        const f32x4 x = g[k / 4];
        gv[k] = x.x; gv[k + 1] = x.y; gv[k + 2] = x.z; gv[k + 3] = x.w;
    }
}
// one lookup joins the row's sum: two roundings (the build has -ffp-contract=off), the sequential oracle's
template <int VEC>
__device__ __forceinline__ void add_scaled(float (&acc)[VEC], float sc, const float (&gv)[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float prod = sc * gv[k];
        acc[k] = acc[k] + prod;
    }
}
// a run opens on the row just loaded: Adagrad holds the row and accumulates the gradient from zero, the plain update accumulates
// on top of the row, in lookup order
template <typename DST, int OPT>
__device__ __forceinline__ void open_row(const u32x4 raw, const u32x4 (&sraw)[OPT == 2 ? DST::kVec / 4 : 1], float (&acc)[DST::kVec],
                                         float (&wrow)[DST::kVec], float (&srow)[OPT == 2 ? DST::kVec : 1]) {
    float wv[DST::kVec];
    DST::widen(raw, wv);
#pragma unroll
    for (int k = 0; k < DST::kVec; ++k) {
        if (OPT != 0) wrow[k] = wv[k];
        else acc[k] = wv[k];
    }
    if constexpr (OPT == 2) state_widen<DST::kVec>(sraw, srow);
}
// A column pass: lane `lig` of a group serves columns c = lig * VEC, + G * VEC, ... < column_pass_end.  Adagrad makes exactly ONE
// pass in which every lane of the group takes part (OPT 1: cross-lane reduction inside adagrad_finish; OPT 2 keeps the rule).
template <int OPT, int VEC>
__device__ __forceinline__ int column_pass_end(int lig, int width) { return OPT != 0 ? lig * VEC + 1 : width; }

// ---- group-wide scans (all G lanes of a lane group call these together) ---------------------------------------
// index of the first lane of this group whose predicate holds, G if none.  Groups of one wave may diverge: the ballot
// only sees active lanes, and only this group's bits are looked at.
template <int G>
__device__ __forceinline__ int group_first(bool pred) {
    const uint64_t m = __ballot(pred);
    if (G == 64) return m ? __builtin_ctzll(m) : G;
    const int sh = (threadIdx.x & 63) / G * G;
    const uint64_t gm = (m >> sh) & ((1ull << (G & 63)) - 1ull);
    return gm ? __builtin_ctzll(gm) : G;
}
// Scans of the tile's LDS key copy (s_key[i + 1] = key of local position i; [0] / [n + 1] hold the neighbours' keys).
// Number of consecutive local positions from, from + 1, ... < to holding `key` ...
template <int G, typename K>
__device__ __forceinline__ int count_same_lds_fwd(const K* s_key, int from, int to, K key) {
    const int lig = threadIdx.x % G;
    for (int j0 = 0; j0 < to - from; j0 += G) {
        const int j = j0 + lig;
        const bool differs = (from + j >= to) || s_key[from + j + 1] != key;
        const int f = group_first<G>(differs);
        if (f < G) return (j0 + f < to - from) ? j0 + f : to - from;
    }
    return to - from;
}
// ... and from to - 1, to - 2, ... >= from
template <int G, typename K>
__device__ __forceinline__ int count_same_lds_bwd(const K* s_key, int from, int to, K key) {
    const int lig = threadIdx.x % G;
    for (int j0 = 0; j0 < to - from; j0 += G) {
        const int j = j0 + lig;
        const bool differs = (to - 1 - j < from) || s_key[to - j] != key;
        const int f = group_first<G>(differs);
        if (f < G) return (j0 + f < to - from) ? j0 + f : to - from;
    }
    return to - from;
}

#ifndef PM_RUN_DEEP
#define PM_RUN_DEEP 2     // batches' worth of gradient rows per trip deep inside a run (1: off)
#endif
template <typename DST, typename K, int G, bool WEIGHTED, int OPT, int TILE>
__global__ void __launch_bounds__(kBlock) bwd_sorted_main_kernel(const SortedParams p) {
    // work list of runs for the fix-up kernel: two counters used in turn.  Which one is this launch's is a device-side
    // generation word that only fix-up kernels advance (fix_ctl[2], read here) -- and the fix-up kernels read theirs
    // (fix_ctl[3]) from the word only main kernels write: no word is written by the kind of kernel that reads it, so no launch
    // needs to know when its last workgroup is done (a ticket per fix-up workgroup measured ~30 ns each, 60 us per launch).
    const uint32_t fix_gen = p.fix_ctl[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) p.fix_ctl[3] = fix_gen;
    PM_STAMP(blockIdx.x, 0);      // (experiment builds: pm_experiments.h; nothing otherwise)
    // positions whose loads a lane group issues together -- for real since late round 3 (see the end of the batch loop).  Measured
    // with the batch real (profiles/r03_bwd_apply_experiments.md; apply ms uniform / Zipf): fp32 tables 2: 1.550 / 0.880, 3: 1.543 /
    // 0.867, 4: 1.504 / 0.830, 6: 1.518 / 0.846, 8: 1.508 / 0.939; 16-bit tables (their per-position registers are twice the fp32
    // instance's: 8 gradient values per lane and position) -- with their rows kept raw until consumed, which is what made THEIR batch
    // real -- 1: 1.365 / 0.964, 2: 1.368 / 0.946, 3: 1.370 / 1.031, 4: 1.381 / 1.026.
    // -DPM_KBATCH_F32= / -DPM_KBATCH_16= rebuild the kernels with another depth.
#ifndef PM_KBATCH_F32
#define PM_KBATCH_F32 4
#endif
#ifndef PM_KBATCH_16
#define PM_KBATCH_16 2
#endif
    // Element-wise Adagrad on 16-bit tables: ONE position per trip of the general path (gradient 2 x 16 B + row + state 2 x 16 B = 5
    // loads in flight) and four per trip deep inside a run (8 loads).  At two positions per trip every fp16 instance and the bf16
    // instances with 64-bit keys came to 129-143 VGPRs -- the open run's 8 state values and the batch's 2 x 8 sit on top of what the
    // row-wise instance holds -- past the 128 this kernel's occupancy counts on (4 waves per SIMD); asking the compiler for 128
    // spilled 12-36 bytes.  One position: at most 115 VGPRs over all 16-bit instances, no scratch.
    constexpr bool kLean = OPT == 2 && DST::kES == 2;
    constexpr int kBatch = DST::kES == 2 ? (kLean ? 1 : PM_KBATCH_16) : PM_KBATCH_F32;
    constexpr int kDeepMul = kLean ? 4 : PM_RUN_DEEP;
    constexpr int VEC = DST::kVec;
    constexpr int NG = kBlock / G;
    constexpr int C = TILE / NG;
    // The workgroup's window of the sorted order: its TILE positions plus up to kOver = kExactRun positions on either side, so
    // that a short run (<= exact_run lookups) which crosses the tile's border is seen WHOLE by both workgroups it touches: the
    // one that holds its head applies it (its last lane group walks on into the overhang), the other skips its piece.  Only
    // runs longer than exact_run are left in pieces for the fix-up kernel -- a short run that reaches the window's edge and
    // goes on is longer than kOver, hence long.  (Before, every short run across a tile border was re-walked by the fix-up
    // kernel: a third of the runs it mended on a Zipf request, and the reason small tiles cost more than they gained.)
    // s_key[i + 1] = key of position base + i for i in [-nb - 1, n_tile + nf]: the ends hold the window's neighbours.
    constexpr int kOver = kExactRun;
    __shared__ K s_keyw[TILE + 2 + 2 * kOver];
    __shared__ uint32_t s_val[TILE + kOver];
    K* const s_key = s_keyw + kOver;
    // per-table arrays staged in LDS (they break a dependent global-load chain); dynamic, sized by the launcher for the
    // request's T tables: [dst T x 8][out_offsets T x 8][state T x 8 if OPT][dims T x 4]
    extern __shared__ __attribute__((aligned(16))) char s_tab[];
    char** s_dst = reinterpret_cast<char**>(s_tab);
    int64_t* s_ooff = reinterpret_cast<int64_t*>(s_tab + static_cast<size_t>(p.T) * 8);
    float** s_mom = reinterpret_cast<float**>(s_tab + static_cast<size_t>(p.T) * 16);
    int32_t* s_dim = reinterpret_cast<int32_t*>(s_tab + static_cast<size_t>(p.T) * (OPT != 0 ? 24 : 16));

    const K* keys = reinterpret_cast<const K*>(p.keys);
    const int nt_rows = p.nt_rows;
    const K pad_bit = static_cast<K>(1) << p.kbits;
    const K row_mask = (static_cast<K>(1) << p.rbits) - 1;
    // blockIdx -> tile of sorted positions.  When the sorted array is a sequence of equal, tile-aligned segments -- one
    // per table, or per (table, bag phase) -- (seg_tiles > 0: every bag has the same number of lookups):
    //   * XCD-affine (xcd != 0): the tiles of table t are served by XCD t % 8 only (blocks are dispatched round-robin
    //     over the 8 XCDs): the ~160 tiles one XCD has in flight then belong to ONE table, whose gradient rows -- each
    //     re-read once per lookup of its bag -- are fetched into one L2 instead of all eight;
    //   * bag phases (H == 2): this launch applies only the segments of phase p.phase (the lookups of the lower / upper
    //     half of the bags; a run never spans two phases, the phase being part of the key), so the gradient rows it
    //     re-reads are half a table's: 2 MB per XCD instead of 4 MB, which is what the 4 MB L2 can actually hold next
    //     to the row traffic streaming through it.  A row looked up in both halves is updated by both launches, in
    //     stream order = lookup order (positions are bag-major).
    const int64_t n_sorted = p.d_n ? static_cast<int64_t>(*p.d_n) : p.n;   // round 3: the pair count lives on the device (batch slices)
    int64_t tile_id = blockIdx.x;
    if (p.xcd == 2) {
        // XCD-contiguous: XCD x (blocks are dispatched round-robin over the 8 XCDs) serves the x-th eighth of the sorted
        // array -- a contiguous run of the table-major order, so the tiles an XCD has in flight belong to one or two tables
        // (whose gradient rows then live in ONE L2) whatever the number of tables or their sizes, and the work per XCD is equal
        // (eighths of the pairs there ARE: with the hybrid backward the sorted arrays hold a few per cent of the request's lookups)
        const int64_t per = ((n_sorted + TILE - 1) / TILE + kXcds - 1) / kXcds;
        const int64_t slot = blockIdx.x / kXcds;
        if (slot >= per) return;
        tile_id = (blockIdx.x % kXcds) * per + slot;
    } else if (p.seg_tiles > 0) {
        int64_t t, i;
        if (p.xcd) {
            const int xcd = blockIdx.x % kXcds;
            const int64_t slot = blockIdx.x / kXcds;
            t = xcd + kXcds * (slot / p.seg_tiles);
            i = slot % p.seg_tiles;
        } else {
            t = blockIdx.x / p.seg_tiles;
            i = blockIdx.x % p.seg_tiles;
        }
        if (t >= p.T) return;
        tile_id = (t * p.H + p.phase) * p.seg_tiles + i;
    }
    const int64_t base = tile_id * TILE;
    if (base >= n_sorted) return;
    const int n_tile = (n_sorted - base) < TILE ? static_cast<int>(n_sorted - base) : TILE;
    const int nb = base < kOver ? static_cast<int>(base) : kOver;                              // positions before the tile
    const int64_t after = n_sorted - (base + n_tile);
    const int nf = after < kOver ? static_cast<int>(after) : kOver;                            // ... and after it
    for (int i = static_cast<int>(threadIdx.x) - nb; i < n_tile + nf; i += kBlock) {
        s_key[i + 1] = keys[base + i];
        if (i >= 0) s_val[i] = p.vals[base + i];
    }
    if (threadIdx.x == 0) {
        s_key[-nb] = base - nb > 0 ? keys[base - nb - 1] : pad_bit;                            // pad never equals a real key
        s_key[n_tile + nf + 1] = (base + n_tile + nf < n_sorted) ? keys[base + n_tile + nf] : pad_bit;
    }
    for (int t = threadIdx.x; t < p.T; t += kBlock) {
        s_dst[t] = reinterpret_cast<char*>(p.dst[t]);
        s_ooff[t] = p.out_offsets ? p.out_offsets[t] : 0;      // NULL (uniform): a sequence apply, gradient rows addressed by position
        s_dim[t] = p.dims[t];
        if (OPT == 1) s_mom[t] = p.mom[t];
        if (OPT == 2) s_mom[t] = p.state[t];      // [rows, D] fp32, one value per weight
    }
    __syncthreads();
    PM_STAMP(blockIdx.x, 1);
    // A tile that lies wholly inside ONE run -- the run comes in from the left and goes on to the right: a Zipf head row at rank
    // shapes (51 K lookups of one row per table at N = 8: 100 tiles), a 3-row Criteo table -- hands the fix-up one partial sum,
    // its chunks' partials added in chunk order here, instead of NG of them: the fix-up's chain of partial-sum round trips and
    // its walk over the chunk records are NG times shorter (119 us -> see HISTORY r5 at the N = 8 Zipf shape).  Uniform over
    // the workgroup (LDS keys); every group of such a tile is in mode 1 from its first position to its last.
    constexpr bool kJoin = !(WEIGHTED && OPT != 0);    // (that instance has no registers to spare: 130 VGPRs with the join; the launcher agrees)
    __shared__ float s_join[kJoin ? kBlock * VEC : 1];
    const bool tile_joined = kJoin && p.join_tiles && n_tile == TILE && s_key[1] == s_key[TILE] && s_key[0] == s_key[1] &&
                             s_key[TILE + 1] == s_key[1] && !(s_key[1] & pad_bit);

    const int gid = threadIdx.x / G;
    const int lig = threadIdx.x % G;
    const int l0 = gid * C;                       // chunk = local positions [l0, l1)
    if (l0 >= n_tile) return;
    const int l1 = (l0 + C < n_tile) ? l0 + C : n_tile;
    const int64_t chunk = (base / TILE) * NG + gid;
    ChunkRec* rec = p.recs + chunk;
    float* lead_slot = p.partials + (chunk * 2) * p.max_dim;
    float* trail_slot = lead_slot + p.max_dim;

    // shape of the chunk's first and last run
    const K first_key = s_key[l0 + 1];
    const K last_key = s_key[l1];
    const bool lead_open = first_key == s_key[l0] && !(first_key & pad_bit);   // continues a run from the left
    const bool trail_open = last_key == s_key[l1 + 1] && !(last_key & pad_bit);  // continues to the right

    // A short run (<= exact_run lookups) across a chunk boundary -- or across the tile's border, see the window above -- is
    // applied exactly and once, by the group whose chunk holds its head: that group's loop runs on past the end of its chunk
    // (own_after positions, still in LDS) and the groups to the right skip their piece (lead_skip).  All groups read the same
    // keys (of their own window or of the neighbour's: the same values), so they agree on every run's extent without
    // exchanging anything.  Longer runs go the partial-sum way (fix-up kernel).
    int lead_skip = 0, own_after = 0;
    bool lead_partial = lead_open, trail_partial = trail_open;
    if (p.exact_run > 0 && (lead_open || trail_open)) {
        bool whole_chunk_in_lead_run = false;
        if (lead_open) {
            const int in_chunk = count_same_lds_fwd<G, K>(s_key, l0, l1, first_key);
            const bool goes_on = in_chunk == l1 - l0 && trail_open;              // then last_key == first_key
            whole_chunk_in_lead_run = goes_on;
            const int right = goes_on ? count_same_lds_fwd<G, K>(s_key, l1, n_tile + nf, first_key) : 0;
            const int before = count_same_lds_bwd<G, K>(s_key, -nb, l0, first_key);
            const bool leaves_tile = (before == l0 + nb && s_key[-nb] == first_key) ||
                                     (goes_on && l1 + right == n_tile + nf && s_key[n_tile + nf + 1] == first_key);
            if (!leaves_tile && before + in_chunk + right <= p.exact_run) {
                lead_skip = in_chunk;
                lead_partial = false;
                if (goes_on) trail_partial = false;                              // a middle chunk: nothing to do here
            }
        }
        if (trail_open && !whole_chunk_in_lead_run) {                            // the trailing run's head is in this chunk
            const int tail = count_same_lds_bwd<G, K>(s_key, l0, l1, last_key);
            const int right = count_same_lds_fwd<G, K>(s_key, l1, n_tile + nf, last_key);
            const bool leaves_tile = l1 + right == n_tile + nf && s_key[n_tile + nf + 1] == last_key;
            if (!leaves_tile && tail + right <= p.exact_run) {
                own_after = right;
                trail_partial = false;
            }
        }
    }

    const int l1e = l1 + own_after;      // end of this group's walk (<= n_tile)
    PM_STAMP(blockIdx.x, 2);

    const int c_end = column_pass_end<OPT, VEC>(lig, p.max_dim);
    for (int c = lig * VEC; c < c_end; c += G * VEC) {
        // mode: 0 closed, 1 leading piece (partial from zero), 2 in-chunk run, 3 trailing piece (partial from zero)
        int mode = 0;
        bool any_col = false, done = false;
        int seg_start = l0;
        uint32_t lead_len = 0, trail_len = 0;
        float acc[VEC];
        float wrow[VEC];                // OPT 1: the destination row, held until the run's gradient is complete
        float cur_mom = 0.0f;           // OPT 1: the open run's optimizer state, fetched together with its row
        constexpr int SV = OPT == 2 ? VEC : 1;
        float srow[SV];                 // OPT 2: the open run's state values of this lane's columns, fetched together with its row
        K cur_key = 0;                  // key of the open run: row pointer, state pointer and row length are re-derived
                                        // from it when the run closes (keeping them live across the batch cost the
                                        // kernel a fifth wave per SIMD)
        // (the zeroing is spelled out in each kernel: as a helper it moved this kernel's element-wise Adagrad instances and was in
        // no combination of lifts that left the benchmark's kernels alone)
#pragma unroll
        for (int k = 0; k < VEC; ++k) { acc[k] = 0.0f; wrow[k] = 0.0f; }
#pragma unroll
        for (int k = 0; k < SV; ++k) srow[k] = 0.0f;
        const char* const dummy_fast = reinterpret_cast<const char*>(p.partials) + static_cast<size_t>(lig) * VEC * sizeof(float);
        auto close_run = [&](K key, float (&a)[VEC], float (&w)[VEC], bool cols, float m_prev) {
            const int t = static_cast<int>(key >> p.tshift);
            const int64_t row = static_cast<int64_t>(key & row_mask);
            const int D = s_dim[t];
            char* wptr = s_dst[t] + (row * D + c) * DST::kES;
            // (finish_row's text, kept: the call moved the benchmark's bf16 plain-update instances of this kernel)
            if constexpr (OPT == 2) {
                if (cols) adagrad_elem_finish<DST>(wptr, w, a, srow, s_mom[t] + row * D + c, p, nt_rows, static_cast<uint64_t>(key), c);
            } else
            if (OPT == 1) adagrad_finish<DST, G>(wptr, w, a, cols, s_mom[t] + row, m_prev, D, p, lig, nt_rows, static_cast<uint64_t>(key), c);
            else if (cols) DST::store(wptr, a, nt_rows);
        };
        for (int pos = l0 + lead_skip; pos < l1e && !done; pos += kBatch) {
            K kk[kBatch + 1];
            uint32_t vv[kBatch];
            bool valid[kBatch], head[kBatch];
            // Inside a run.  When every position of the batch continues the run that is open -- the bulk of a skewed request: a
            // Zipf(1.05) head, the 3- to 155-row Criteo tables -- all there is to do is add kBatch gradient rows: no heads, no row
            // loads, no bookkeeping.  The general path below spends ~125 instructions per position and wave on that and, with
            // every memory operation removed, still took 407 of the Zipf benchmark request's 773 us (round 4, tools/r4_timeline.sh).
            // Same operations in the same order as the general path (prod = alpha * g, acc = acc + prod): same bits.
            if (!WEIGHTED && mode != 0 && pos + kBatch <= l1e) {
                bool same = true;
#pragma unroll
                for (int u = 0; u < kBatch; ++u) same = same && s_key[pos + u + 1] == cur_key;
                if (same) {                                                  // uniform over the lane group
                    const int t = static_cast<int>(cur_key >> p.tshift);
                    const float* gt = any_col ? p.grad + s_ooff[t] + c : reinterpret_cast<const float*>(dummy_fast);
                    const int64_t stride = any_col ? p.out_stride : 0;
                    const int64_t bextra = any_col ? p.gblk_extra : 0;      // blocked gradient layout (0: none)
                    // deep inside a run (the next batch continues it as well): twice the gradient rows per trip
                    constexpr int kDeep = kDeepMul * kBatch;
                    bool deep = kDeepMul > 1 && pos + kDeep <= l1e;
#pragma unroll
                    for (int u = kBatch; u < kDeep; ++u) deep = deep && s_key[pos + (u < kDeep ? u : 0) + 1] == cur_key;
                    // (written twice, for kDeep and for kBatch rows, with load_grad's and add_scaled's text: as one function of the row
                    // count the unweighted instances of this kernel, the benchmark's fp32 plain update among them, moved)
                    if (deep) {
                        float gf[kDeep][VEC];
#pragma unroll
                        for (int u = 0; u < kDeep; ++u) {
                            const float* g = gt + grad_bag_offset(static_cast<int64_t>(s_val[pos + u]), stride, p.gblk_shift, bextra);
#pragma unroll
                            for (int k = 0; k < VEC; k += 4) {
                                const f32x4 x = *reinterpret_cast<const f32x4*>(g + k);
                                gf[u][k] = x.x; gf[u][k + 1] = x.y; gf[u][k + 2] = x.z; gf[u][k + 3] = x.w;
                            }
                        }
                        if (any_col) {
#pragma unroll
                            for (int u = 0; u < kDeep; ++u)
#pragma unroll
                                for (int k = 0; k < VEC; ++k) {
                                    const float prod = p.alpha * gf[u][k];
                                    acc[k] = acc[k] + prod;
                                }
                        }
                        pos += kDeep - kBatch;
                        continue;
                    }
                    float gf[kBatch][VEC];
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) {
                        const float* g = gt + grad_bag_offset(static_cast<int64_t>(s_val[pos + u]), stride, p.gblk_shift, bextra);
#pragma unroll
                        for (int k = 0; k < VEC; k += 4) {
                            const f32x4 x = *reinterpret_cast<const f32x4*>(g + k);
                            gf[u][k] = x.x; gf[u][k + 1] = x.y; gf[u][k + 2] = x.z; gf[u][k + 3] = x.w;
                        }
                    }
                    if (any_col) {
#pragma unroll
                        for (int u = 0; u < kBatch; ++u)
#pragma unroll
                            for (int k = 0; k < VEC; ++k) {
                                const float prod = p.alpha * gf[u][k];
                                acc[k] = acc[k] + prod;
                            }
                    }
                    continue;
                }
            }
            kk[0] = s_key[pos];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const bool in = (pos + u) < l1e;
                kk[u + 1] = in ? s_key[pos + u + 1] : pad_bit;
                valid[u] = in && !(kk[u + 1] & pad_bit);          // padding keys sort last: end of data
                vv[u] = valid[u] ? s_val[pos + u] : 0u;
                head[u] = valid[u] && kk[u + 1] != kk[u];
            }
            // issue every load of the batch before the first add
            float gv[kBatch][VEC];
            u32x4 wraw[kBatch];             // destination rows as loaded: widened when consumed (DST::widen); left unset where no
                                            // row is loaded (a zero there costs a register copy behind a full wait per position)
            float sc[kBatch];
            float mv[kBatch];
            u32x4 sraw[kBatch][OPT == 2 ? VEC / 4 : 1];      // OPT 2: the state values as loaded (unset where no row is loaded)
            bool col_ok[kBatch];
            // Straight-line: every position of the batch issues its gradient load and its row load, whatever it is -- a position
            // that needs none (past the chunk's end, not the head of a run) reads a harmless, cache-resident address instead
            // (the first chunk's partial-sum slot).  No branch stands between two loads of the batch.
            const char* const dummy = reinterpret_cast<const char*>(p.partials) + static_cast<size_t>(lig) * VEC * sizeof(float);
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                mv[u] = 0.0f;
                const K key = kk[u + 1];
                const int t = valid[u] ? static_cast<int>(key >> p.tshift) : 0;
                const int64_t row = static_cast<int64_t>(key & row_mask);
                const int D = s_dim[t];
                col_ok[u] = valid[u] && c < D;
                const bool need_row = col_ok[u] && head[u] && !(trail_partial && key == last_key);
                // row-wise Adagrad: the run's state value rides along with the head's row load (reading it when
                // the run closes put one more memory round trip on every run)
                if (OPT == 1 && valid[u] && head[u] && !(trail_partial && key == last_key)) mv[u] = *as_global<float>(s_mom[t] + row);
                uint32_t bag = vv[u];
                sc[u] = p.alpha;
                if (WEIGHTED) {
                    if (col_ok[u]) {
                        sc[u] = p.alpha * p.psw[vv[u]];
                        bag = p.bag_of[vv[u]];
                    }
                }
                const float* g = col_ok[u] ? p.grad + s_ooff[t] + grad_bag_offset(static_cast<int64_t>(bag), p.out_stride, p.gblk_shift, p.gblk_extra) + c
                                           : reinterpret_cast<const float*>(dummy);
                load_grad<VEC>(reinterpret_cast<const f32x4*>(g), gv[u]);
                // in-chunk runs need the destination row; the trailing open run does not
                wraw[u] = DST::load_raw(need_row ? s_dst[t] + (row * D + c) * DST::kES : dummy, nt_rows);
                // element-wise Adagrad: the state of the lane's columns is issued right behind the row, from the same test
                if constexpr (OPT == 2)
                    state_load_raw<VEC>(need_row ? reinterpret_cast<const char*>(s_mom[t] + row * D + c) : dummy, sraw[u], nt_rows);
            }
            // consume in sorted order
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                if (done) break;
                if (!valid[u]) {
                    done = true;  // end of chunk or of data
                    break;
                }
                const int q = pos + u;
                if (head[u] || (q == l0 && lead_partial)) {
                    // close what was open
                    if (mode == 2) {
                        close_run(cur_key, acc, wrow, any_col, cur_mom);
                    }
                    if (mode == 1) {
                        lead_len = static_cast<uint32_t>(q - l0);
                        if (any_col) {
                            hidden_store_vec<VEC>(lead_slot + c, acc);
                        }
                    }
                    seg_start = q;
                    any_col = col_ok[u];
                    cur_key = kk[u + 1];
                    cur_mom = mv[u];
                    if (!head[u]) {
                        mode = 1;
                    } else if (trail_partial && kk[u + 1] == last_key) {
                        mode = 3;
                    } else {
                        mode = 2;
                    }
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
                    if (mode == 2 && any_col) open_row<DST, OPT>(wraw[u], sraw[u], acc, wrow, srow);
                }
                if (mode != 0 && any_col) add_scaled<VEC>(acc, sc[u], gv[u]);
            }
            // Every register a load of this batch was issued into counts as read here, whichever way the consumption above went
            // (positions past the chunk's end, columns past the table's width and runs without a row load leave theirs unread).
            // Without it such a load is still "pending" for the compiler when the next trip overwrites its register, and -- the
            // pending state of a loop merged over all those paths having no order left -- it guards EVERY position's address
            // arithmetic with `s_waitcnt vmcnt(0)`: one position's loads in flight at a time instead of kBatch.
            // (Spelled out in the three kernels that need it: as a count_as_read(...) helper, together with the other pieces, it
            // moved this kernel's unweighted instances and the left-over kernel's bf16 plain-update instances.)
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) asm volatile("" : : "v"(gv[u][k]));
                asm volatile("" : : "v"(wraw[u]));
                asm volatile("" : : "v"(mv[u]), "v"(sc[u]));
                if constexpr (OPT == 2) {
#pragma unroll
                    for (int k = 0; k < VEC / 4; ++k) asm volatile("" : : "v"(sraw[u][k]));
                }
            }
        }
        // close the last segment of the chunk
        if (mode == 2) {
            close_run(cur_key, acc, wrow, any_col, cur_mom);
        }
        if (mode == 1) {  // the leading piece covers every real position of the chunk
            int real = l1 - l0;
            // count only real (non-pad) positions: pads sit at the very end of the data
            while (real > 0 && (s_key[l0 + real] & pad_bit)) --real;
            lead_len = static_cast<uint32_t>(real);
            if (any_col && !tile_joined) {
                hidden_store_vec<VEC>(lead_slot + c, acc);
            }
        }
        if (tile_joined) {              // (mode == 1 in every group)
            float* const sj = s_join + threadIdx.x * VEC;
#pragma unroll
            for (int k = 0; k < VEC; ++k) sj[k] = acc[k];
            __syncthreads();
            if (gid == 0) {
                float sum[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) sum[k] = acc[k];
#pragma unroll 1
                for (int g = 1; g < NG; ++g) {          // (not unrolled further: NG - 1 partials in registers at once otherwise)
#pragma unroll
                    for (int k = 0; k < VEC; ++k) sum[k] = sum[k] + s_join[(g * G + lig) * VEC + k];
                }
                if (any_col) hidden_store_vec<VEC>(lead_slot + c, sum);
            }
            if (c + G * VEC < c_end) __syncthreads();       // the next pass writes s_join again
        }
        if (mode == 3) {
            trail_len = static_cast<uint32_t>(l1 - seg_start);
            if (any_col) {
                hidden_store_vec<VEC>(trail_slot + c, acc);
            }
        }
        if (c == 0 && lig == 0) {
            rec->lead_len = lead_len | ((tile_joined && gid == 0) ? kJoinedBit : 0u);
            rec->trail_len = trail_len;
            // a chunk that holds the head of a run left in pieces goes on the fix-up's work list (the list order is arbitrary and
            // does not matter: runs are mended independently).  One returning atomic per such chunk, spread over the whole launch.
            if (trail_len > 0) p.fix_list[atomicAdd(p.fix_ctl + (fix_gen & 1u), 1u)] = static_cast<uint32_t>(chunk);
        }
    }
    PM_STAMP_DRAINED(blockIdx.x, 3);      // (lane group 0's end: thread 0 stamps)
}

// one run the main kernel left in pieces, mended by one lane group: `h` = the chunk holding the run's head, `trail` = that
// chunk's trailing piece
template <typename DST, typename K, int G, bool WEIGHTED, int OPT, int TILE>
__device__ __forceinline__ void fixup_one_run(const SortedParams& p, int64_t h, uint32_t trail, int64_t walk_end, uint32_t* my_bag, float* my_sc) {
    constexpr int VEC = DST::kVec;
    constexpr int NG = kBlock / G;
    constexpr int C = TILE / NG;
    // gradient rows in flight per lane in the exact walk: the walk is a chain of memory round trips and nothing else (the few
    // groups that have a run to mend are alone on their CUs), so the batch is as deep as the register file allows -- a run of
    // 250 lookups (the 36- and 108-row Criteo tables) was 32 trips at 8 rows per trip, a third of that kernel's 42 us
    constexpr int kFixBatch = 128 / VEC;
    const int lig = threadIdx.x % G;

    const int nt_rows = p.nt_rows;
    const K* keys = reinterpret_cast<const K*>(p.keys);
    const K row_mask = (static_cast<K>(1) << p.rbits) - 1;
    const int64_t c1 = (h + 1) * C;                    // a trailing piece implies the chunk is full
    const int64_t start = c1 - trail;
    const K key = keys[start];
    const int t = static_cast<int>(key >> p.tshift);
    const int64_t row = static_cast<int64_t>(key & row_mask);
    const int D = p.dims[t];

    // total length and last chunk of the run
    // (G records per round trip: a Zipf head row spans ~100 chunks, and one record per trip was the kernel's floor.  Tiles the
    // main kernel joined -- kJoinedBit on their first chunk's record: contiguous, from the first tile border the run reaches --
    // are walked G TILES per trip.)
    int64_t len = trail, last = h;
    int64_t jt0 = 0;                 // first chunk of the first joined tile
    int64_t njt = 0;                 // joined tiles
    bool tiles_done = !p.join_tiles;
    for (int64_t i0 = h + 1; i0 < walk_end;) {
        if (!tiles_done && i0 % NG == 0) {
            const int64_t i = i0 + static_cast<int64_t>(lig) * NG;
            const uint32_t ll = i < walk_end ? p.recs[i].lead_len : 0u;
            const int f = group_first<G>(!(ll & kJoinedBit));              // first tile that is not joined
            const int full = f < G ? f : G;
            if (njt == 0) jt0 = i0;
            njt += full;
            len += static_cast<int64_t>(full) * TILE;
            i0 += static_cast<int64_t>(full) * NG;
            if (full > 0) last = i0 - 1;
            tiles_done = f < G;
            continue;
        }
        int n = G;                   // chunks this trip looks at: up to the next tile border while joined tiles may follow
        if (!tiles_done) {
            const int64_t to_border = (i0 / NG + 1) * NG - i0;
            if (to_border < n) n = static_cast<int>(to_border);
        }
        const int64_t i = i0 + lig;
        const uint32_t ll = lig >= n ? static_cast<uint32_t>(C) : (i < walk_end ? p.recs[i].lead_len : 0u);
        const int f = group_first<G>(ll < static_cast<uint32_t>(C));   // first chunk the run does not fill
        const int full = f < G ? f : n;
        len += static_cast<int64_t>(full) * C;
        last = i0 + full - 1;
        if (f < G) {
            const uint32_t tail = __shfl(ll, f, G);                     // 0: the run ended with the chunk before
            if (tail > 0) {
                len += tail;
                last = i0 + f;
            }
            break;
        }
        i0 += n;
    }

    // Short run: stage every position's bag (and scale) in LDS first -- all lanes of the group fetch in parallel --
    // so the walk below is a chain of gradient-row round trips only, kFixBatch rows per trip.  (The lanes of a group
    // belong to one wave, whose LDS operations execute in order: a wave-level fence is all the hand-over needs.)
    const bool exact = len <= p.exact_run;
    if (exact) {
        // eight positions per lane and trip, loaded together (positions past the run re-read its last one and are dropped)
        const int n = static_cast<int>(len);
        for (int i0 = lig; i0 < n; i0 += 8 * G) {
            uint32_t v[8];
            float sc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * G;
                v[u] = p.vals[start + (i < n ? i : n - 1)];
            }
            if (WEIGHTED) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    sc[u] = p.psw[v[u]];
                    v[u] = p.bag_of[v[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * G;
                if (i < n) {
                    if (WEIGHTED) my_sc[i] = p.alpha * sc[u];
                    my_bag[i] = v[u];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    const int c_end = column_pass_end<OPT, VEC>(lig, D);
    for (int c = lig * VEC; c < c_end; c += G * VEC) {
        const bool any_col = c < D;
        char* wptr = reinterpret_cast<char*>(p.dst[t]) + (row * D + c) * DST::kES;
        float acc[VEC];
        float wrow[VEC];
        float srow[OPT == 2 ? VEC : 1];      // OPT 2: the state of this lane's columns, loaded with the row
        float* const st_ptr = OPT == 2 ? p.state[t] + row * D + c : nullptr;
#pragma unroll
        for (int k = 0; k < VEC; ++k) { acc[k] = 0.0f; wrow[k] = 0.0f; }
        if (any_col) {
            if (OPT != 0) DST::load(wptr, wrow, nt_rows);
            else DST::load(wptr, acc, nt_rows);
            if constexpr (OPT == 2) {
                u32x4 sraw[VEC / 4];
                state_load_raw<VEC>(st_ptr, sraw, nt_rows);
                state_widen<VEC>(sraw, srow);
            }
        }
        float mom_prev = 0.0f;
        if (OPT == 1) mom_prev = *as_global<float>(p.mom[t] + row);
        if (exact) {
            // exact: re-walk the run in lookup order
            const float* gbase = p.grad + (p.out_offsets ? p.out_offsets[t] : 0) + c;
            for (int q = 0; q < static_cast<int>(len); q += kFixBatch) {
                float gv[kFixBatch][VEC];
                float sc[kFixBatch];
                if (any_col) {
                    // straight-line: positions past the run re-read its last gradient row (dropped below)
#pragma unroll
                    for (int u = 0; u < kFixBatch; ++u) {
                        const int qq = q + u < static_cast<int>(len) ? q + u : static_cast<int>(len) - 1;
                        sc[u] = WEIGHTED ? my_sc[qq] : p.alpha;
                        const float* g = gbase + grad_bag_offset(static_cast<int64_t>(my_bag[qq]), p.out_stride, p.gblk_shift, p.gblk_extra);
                        load_grad<VEC>(reinterpret_cast<const f32x4*>(g), gv[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < kFixBatch; ++u) {
                    if (any_col && q + u < static_cast<int>(len)) add_scaled<VEC>(acc, sc[u], gv[u]);
                }
            }
        } else if (any_col) {
            // long run: chunk partials in chunk order
            const float* part = p.partials + ((h * 2) + 1) * p.max_dim + c;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + part[k];
            // the chunks' leading partials, added in chunk order; kFixBatch loads per round trip (a hot row of a small table spans
            // hundreds of chunks: one load per trip made this kernel a tenth of the Criteo backward).  A joined tile is one element
            // of the sequence (its first chunk's slot holds the tile's sum): chunks h+1 .. jt0-1, the njt tiles, the chunks after them.
            const int64_t n1 = njt > 0 ? jt0 - (h + 1) : last - h;
            const int64_t n_el = (last - h) - njt * (NG - 1);
            auto chunk_of = [&](int64_t e) -> int64_t {
                if (e < n1) return h + 1 + e;
                if (e < n1 + njt) return jt0 + (e - n1) * NG;
                return jt0 + njt * NG + (e - n1 - njt);
            };
            for (int64_t e0 = 0; e0 < n_el; e0 += kFixBatch) {
                float lv[kFixBatch][VEC];
#pragma unroll
                for (int u = 0; u < kFixBatch; ++u) {
                    const int64_t ii = chunk_of(e0 + u < n_el ? e0 + u : n_el - 1);       // straight-line: past the run, its last element again
                    const float* lp = p.partials + (ii * 2) * p.max_dim + c;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) lv[u][k] = lp[k];
                }
#pragma unroll
                for (int u = 0; u < kFixBatch; ++u) {
                    if (e0 + u < n_el) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + lv[u][k];
                    }
                }
            }
        }
        // (the plain update's passes end at D: any_col holds in every one of them)
        finish_row<DST, G, OPT>(wptr, wrow, acc, srow, any_col, OPT == 1 ? p.mom[t] + row : st_ptr, mom_prev, D, p, lig, nt_rows,
                                static_cast<uint64_t>(key), c);
    }
}

// Fix-up: the main kernel listed the chunks that hold the head of a run it left in pieces (one that crosses a TILE boundary,
// or longer than exact_run); a FIXED grid's lane groups take one listed run each (round-robin beyond grid x groups runs), so
// every run is mended concurrently whatever their number and wherever they sit -- the runs of a Zipf head or of a 3-row table
// are neighbours in the sorted order, and both a group per chunk (thousands of workgroups that read one record and leave,
// cycling through the few slots this kernel's registers allow) and a strip of chunks per group (a strip at a table's head
// mends dozens of runs one after the other) cost 40-90 us where the chain of one run is ~15.
// Launched after the main kernel on the same stream (kernel boundary = visibility).
template <typename DST, typename K, int G, bool WEIGHTED, int OPT, int TILE>
__global__ void __launch_bounds__(kBlock) bwd_sorted_fixup_kernel(const SortedParams p, int64_t n_chunks) {
    constexpr int NG = kBlock / G;
    constexpr int C = TILE / NG;
    __shared__ uint32_t s_bag[NG * kExactRun];
    __shared__ float s_sc[WEIGHTED ? NG * kExactRun : 1];
    const int gid = threadIdx.x / G;
    if (p.d_n) n_chunks = (static_cast<int64_t>(*p.d_n) + C - 1) / C;       // chunks past the device-side count hold no records
    const u32x4 ctl = *reinterpret_cast<const u32x4*>(p.fix_ctl);   // one load: both lengths and the generation words
    const uint32_t fix_gen = ctl.w;                         // written by this launch's main kernel
    const uint32_t n_fix = (fix_gen & 1u) ? ctl.y : ctl.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {             // for the next apply: the other counter, emptied
        p.fix_ctl[(fix_gen + 1u) & 1u] = 0u;
        p.fix_ctl[2] = fix_gen + 1u;
    }
    if (blockIdx.x * NG >= n_fix) return;                  // only the workgroups that get a run stay
    uint32_t* my_bag = s_bag + gid * kExactRun;
    float* my_sc = s_sc + (WEIGHTED ? gid * kExactRun : 0);
    const uint32_t groups = gridDim.x * NG;
    for (uint32_t e = blockIdx.x * NG + gid; e < n_fix; e += groups) {
        const int64_t h = p.fix_list[e];
        // bag phases: a run ends inside its segment (the list holds this launch's phase only: it is emptied after every launch)
        const int64_t walk_end = p.H > 1 ? (h / NG / p.seg_tiles + 1) * p.seg_tiles * NG : n_chunks;
        fixup_one_run<DST, K, G, WEIGHTED, OPT, TILE>(p, h, p.recs[h].trail_len, walk_end, my_bag, my_sc);
        // the group's staging rows in LDS are reused by its next run: a group is part of one wave, whose LDS operations
        // execute in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Hybrid backward (round 4; common.h "Hybrid backward", seg_hybrid.inc): the lookups of a HYBRID table whose row no other
// lookup of the step touches -- nearly all of them under uniform indices -- are applied here, bag-major: a lane group owns a
// bag, keeps the bag's gradient slice in registers (loaded ONCE per bag instead of once per lookup) and does one row load, add
// and store per lookup; the sorted apply above moves 3 x D x e bytes per lookup through the CU, this kernel 2 x.  A lookup
// is skipped when all of its row's bits are set in the row's word of the table's dup map: the key sort's emit kernel applied the same test
// to the same maps and handed exactly those lookups to the sorted path, so every lookup is applied exactly once.  A row
// applied here is touched by no other lookup: no order to keep, no atomics, bit-identical to the sequential oracle
// (row + alpha * g is the expression the sorted apply evaluates for a run of one).
// Tiling, LDS staging of offsets / indices and the block -> (table, tile) mapping are the forward's (common.h); the staged
// entry of a lookup is row | dup << 31.  Tables the sort classified "sort" leave at once.
template <typename DST, int G, int OPT>
__global__ void __launch_bounds__(kBlock) bwd_unique_kernel(const SortedParams p, const KParams q, const HybTable* hyb_tab,
                                                            const uint32_t* bloom, void* emit_keys, uint32_t* emit_vals, int key_bytes,
                                                            uint32_t* tile_cnt, size_t tile_cnt_stride, int bloom_wbits_) {
    constexpr int VEC = DST::kVec;
    constexpr int NG = kBlock / G;
#ifndef PM_UNIQUE_UB_F32
#define PM_UNIQUE_UB_F32 4
#endif
#ifndef PM_UNIQUE_UB_16
#define PM_UNIQUE_UB_16 4
#endif
    // row loads a lane group keeps in flight (element-wise Adagrad on 16-bit tables: half as many rows, each with 2 x 16 bytes of state
    // behind it -- 6 loads in flight where the other 16-bit instances have 4, inside the kernel's 128 VGPRs)
    constexpr int UB = (DST::kES == 2 ? PM_UNIQUE_UB_16 : PM_UNIQUE_UB_F32) / (OPT == 2 && DST::kES == 2 ? 2 : 1);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_next;
    // The grid may be smaller than the number of tiles (launcher: PARAM_AMD_UNIQUE_WGS_PER_CU): a workgroup then takes the tiles
    // vb = blockIdx.x, + gridDim.x, ... (gridDim a multiple of 8: the tiles of one workgroup stay on their XCD's tables), and
    // the CUs keep a free workgroup slot for the sort and sorted-apply kernels running beside this one on the second stream.
    const int n_vb = q.T * q.tiles_per_table;
    for (int vb = blockIdx.x; vb < n_vb; vb += gridDim.x) {
    if (vb != static_cast<int>(blockIdx.x)) __syncthreads();       // the previous tile's LDS is free
    int t, tile;
    block_to_tile(q, t, tile, vb);
    if (t >= q.T || t >= kHybMaxTables || hyb_tab[t].mode != 1u) continue;
    const int64_t bag0 = q.bag_begin + static_cast<int64_t>(tile) * q.bags_per_block;
    const int64_t left_bags = q.bag_begin + q.bag_count - bag0;
    if (left_bags <= 0) continue;
    const int nb = left_bags < q.bags_per_block ? static_cast<int>(left_bags) : q.bags_per_block;
    if (threadIdx.x == 0) s_next = NG;
    int64_t* s_off = reinterpret_cast<int64_t*>(smem);
    uint32_t* s_idx = reinterpret_cast<uint32_t*>(smem + tile_idx_offset(q.bags_per_block));
    const int64_t g0 = static_cast<int64_t>(t) * q.B + bag0;
    for (int i = threadIdx.x; i <= nb; i += kBlock) s_off[i] = bag_start_or_end(q, g0 + i);
    __syncthreads();
    const int64_t base = s_off[0];
    const int64_t cnt = s_off[nb] - base;
    const bool staged = cnt <= q.idx_cap;
    const uint32_t* tmap = bloom + (static_cast<size_t>(t) << bloom_wbits_);      // 2^wbits words per table (hyb_slices x 16 384)
    auto flag_of = [&](uint32_t row) -> uint32_t {
        const uint32_t mask = bloom_mask(row);
        return (tmap[bloom_word(row, bloom_wbits_)] & mask) == mask ? 1u : 0u;
    };
    if (staged) {
        // all index loads of a batch first, then their map words (L2-resident: 256 KB per table), then the LDS writes
        constexpr int SU = 4;
        const int n = static_cast<int>(cnt);
        for (int i0 = 0; i0 < n; i0 += kBlock * SU) {
            uint32_t r[SU], f[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int i = i0 + u * kBlock + threadIdx.x;
                r[u] = static_cast<uint32_t>(load_index(q.indices, base + (i < n ? i : n - 1), q.idx64));
            }
#pragma unroll
            for (int u = 0; u < SU; ++u) f[u] = flag_of(r[u]);
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int i = i0 + u * kBlock + threadIdx.x;
                if (i < n) s_idx[i] = r[u] | (f[u] << 31);
            }
        }
        __syncthreads();
    }
    // The flagged lookups of the tile, in order, as (key, bag) pairs into the tile's own request positions of the sort's b
    // buffers, and their number: the input of the sort's compaction (seg_hybrid.inc).  One wave, ballot + prefix popcount per 64
    // entries; the other waves are already pooling.  (A hybrid table has a pooling factor: entry i belongs to bag i / pooling.)
    if (threadIdx.x < kWave) {
        const int lane = threadIdx.x;
        const uint32_t pooling = hyb_tab[t].pooling;
        const uint64_t tkey = static_cast<uint64_t>(t) << p.tshift;
        uint32_t run = 0;
        for (int64_t i0 = 0; i0 < cnt; i0 += kWave) {
            const int64_t i = i0 + lane;
            uint32_t e = 0;
            if (i < cnt) {
                if (staged) {
                    e = s_idx[i];
                } else {
                    const uint32_t r = static_cast<uint32_t>(load_index(q.indices, base + i, q.idx64));
                    e = r | (flag_of(r) << 31);
                }
            }
            const bool hit = (e >> 31) != 0u;
            const uint64_t m = __ballot(hit);
            if (hit) {
                const uint64_t o = static_cast<uint64_t>(base) + run +
                                   __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
                const uint64_t key = tkey | (e & 0x7fffffffu);
                if (key_bytes == 4) static_cast<uint32_t*>(emit_keys)[o] = static_cast<uint32_t>(key);
                else static_cast<uint64_t*>(emit_keys)[o] = key;
                emit_vals[o] = static_cast<uint32_t>(bag0 + i / pooling);
            }
            run += static_cast<uint32_t>(__popcll(m));
        }
        if (lane == 0) tile_cnt[static_cast<size_t>(t) * tile_cnt_stride + tile] = run;
    }
    const int gid = threadIdx.x / G, lig = threadIdx.x % G;
    const int D = q.dims[t];
    const int64_t row_bytes = static_cast<int64_t>(D) * DST::kES;
    char* W = reinterpret_cast<char*>(const_cast<void*>(q.tables[t]));
    const float* grad_t = p.grad + q.out_offsets[t];
    float* mom_t = OPT == 1 ? p.mom[t] : (OPT == 2 ? p.state[t] : nullptr);      // OPT 2: [rows, D], one value per weight
    const int nt_rows = p.nt_rows;
    const char* const dummy = reinterpret_cast<const char*>(p.partials) + static_cast<size_t>(lig) * VEC * sizeof(float);
    const uint64_t tkey = static_cast<uint64_t>(t) << p.tshift;

    for (int slot = gid; slot < nb;) {
        const int64_t s = s_off[slot], e = s_off[slot + 1];
        const float* grow = grad_t + grad_bag_offset(bag0 + slot, q.out_stride, q.gblk_shift, q.gblk_extra);
        auto walk = [&](auto staged_c) {
            constexpr bool ST = decltype(staged_c)::value;
            const int c_end = column_pass_end<OPT, VEC>(lig, D);
            for (int c = lig * VEC; c < c_end; c += G * VEC) {
                const bool any_col = c < D;
                float ga[VEC];      // the bag's gradient, scaled once: alpha * g is every lookup's contribution
                load_grad<VEC>(as_global<f32x4>(any_col ? grow + c : reinterpret_cast<const float*>(dummy)), ga);
#pragma unroll
                for (int k = 0; k < VEC; ++k) ga[k] = p.alpha * ga[k];
                for (int64_t j = s; j < e; j += UB) {
                    uint32_t rr[UB];
                    u32x4 raw[UB];
                    float mv[UB];
                    u32x4 sraw[UB][OPT == 2 ? VEC / 4 : 1];      // OPT 2: the rows' state values, loaded with the rows
                    char* ptr[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u) {      // straight-line: positions past the bag read its last lookup again (dropped below)
                        const int64_t jj = j + u < e ? j + u : e - 1;
                        if (ST) {
                            rr[u] = s_idx[jj - base];
                        } else {
                            const uint32_t r = static_cast<uint32_t>(load_index(q.indices, jj, q.idx64));
                            rr[u] = r | (flag_of(r) << 31);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const bool live = j + u < e && !(rr[u] >> 31);
                        const uint32_t row = rr[u] & 0x7fffffffu;
                        ptr[u] = W + static_cast<uint64_t>(row) * static_cast<uint32_t>(row_bytes) + c * DST::kES;
                        raw[u] = DST::load_raw((live && any_col) ? ptr[u] : dummy, nt_rows);
                        mv[u] = 0.0f;
                        if (OPT == 1) mv[u] = *as_global<float>(live ? mom_t + row : reinterpret_cast<const float*>(dummy));
                        if constexpr (OPT == 2)
                            state_load_raw<VEC>((live && any_col) ? reinterpret_cast<const char*>(mom_t + static_cast<uint64_t>(row) * static_cast<uint32_t>(D) + c) : dummy,
                                                sraw[u], nt_rows);
                    }
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const bool live = j + u < e && !(rr[u] >> 31);     // uniform over the lane group
                        if (live) {
                            // a run of one: the row and its state open it, the bag's gradient is its sum -- "from zero" under Adagrad,
                            // as the sorted apply accumulates it (0.0f + ga: a -0.0 becomes the +0.0 it is there)
                            float acc[VEC], w[VEC], sv[OPT == 2 ? VEC : 1];
#pragma unroll
                            for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
                            open_row<DST, OPT>(raw[u], sraw[u], acc, w, sv);
#pragma unroll
                            for (int k = 0; k < VEC; ++k) acc[k] = (OPT == 0 || any_col) ? acc[k] + ga[k] : 0.0f;
                            const uint32_t row = rr[u] & 0x7fffffffu;
                            float* const state = OPT == 0 ? nullptr : mom_t + (OPT == 2 ? static_cast<uint64_t>(row) * static_cast<uint32_t>(D) + c : row);
                            finish_row<DST, G, OPT>(ptr[u], w, acc, sv, any_col, state, mv[u], D, p, lig, nt_rows, tkey | row, c);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UB; ++u) {      // every loaded register counts as read (see the main kernel's batch)
                        asm volatile("" : : "v"(raw[u]));
                        asm volatile("" : : "v"(mv[u]));
                        if constexpr (OPT == 2) {
#pragma unroll
                            for (int k = 0; k < VEC / 4; ++k) asm volatile("" : : "v"(sraw[u][k]));
                        }
                    }
                }
            }
        };
        if (staged) walk(std::true_type{}); else walk(std::false_type{});
        int nxt = 0;
        if (lig == 0) nxt = atomicAdd(&s_next, 1);
        slot = __shfl(nxt, 0, G);
    }
    }   // tiles of this workgroup
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 6 -- what the bag-major kernel left of a hybrid table, finished inside LDS (common.h: hyb_stage_kernel staged it;
// bwd_sorted_apply.h: RestArgs).  Workgroup (table t, part), for a table with staged pairs (at most kRestCap):
//   1. every workgroup of the table pulls ALL its staged (row, bag) pairs, in list = request-position order, into registers
//      (thread (wave, r, lane) holds position wave * chunk + r * 64 + lane: waves own consecutive runs);
//   2. sorts them in LDS by the row bits, stable 8-bit rounds (per-wave digit counts by ballot matching, as the key sort's tiles):
//      the workgroups of a table hold identical sorted arrays, so they agree on every run without exchanging anything;
//   3. applies the part-th slice of the sorted positions, its lane groups a chunk each: a group owns the runs whose HEAD lies in
//      its chunk (it skips the tail of a run begun before and walks on past the chunk's end to finish its last one -- all in LDS),
//      reads the destination row once, adds the run's gradient rows in list (= lookup) order and writes it once: the expression
//      the sorted apply evaluates for an in-chunk run, and the sequential oracle's bits for ANY run length.
// No atomics on table rows, no inter-workgroup hand-off; LDS: 2 x 32 KB of pairs + 17 KB.
constexpr int kRestAux = (kRestThreads / kWave) * 256 + 256;      // per-wave digit counts + digit starts

// exclusive scan of one value per thread over the workgroup's NW waves; s_tmp[NW] holds the wave totals afterwards (read them
// before the next barrier-separated call)
template <int NW>
__device__ __forceinline__ uint32_t rest_excl_scan(uint32_t v, uint32_t* s_tmp) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += up;
    }
    __syncthreads();                       // the previous call's totals have been read
    if (lane == kWave - 1) s_tmp[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += s_tmp[w];
    return base + incl - v;
}

#ifndef PM_REST_KB_F32
#define PM_REST_KB_F32 8
#endif
#ifndef PM_REST_KB_16
#define PM_REST_KB_16 4
#endif
template <typename DST, int G, int OPT>
__global__ void __launch_bounds__(kRestThreads) hyb_rest_kernel(const SortedParams p, const KParams q, const RestArgs ra) {
    constexpr int VEC = DST::kVec;
    constexpr int NG = kRestThreads / G;
    constexpr int NW = kRestThreads / kWave;
    // sorted positions whose loads a lane group issues together (the Adagrad instances, whose finish keeps the row and the state
    // live, take half: at the full depth they spill)
    constexpr int KB = (DST::kES == 2 ? PM_REST_KB_16 : PM_REST_KB_F32) / (OPT != 0 ? 2 : 1);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* const s_key = reinterpret_cast<uint32_t*>(smem);
    uint32_t* const s_val = s_key + kRestCap;
    uint32_t* const s_aux = s_val + kRestCap;
    __shared__ uint32_t s_tmp[NW];
    const int t = static_cast<int>(blockIdx.x) / ra.parts, part = static_cast<int>(blockIdx.x) % ra.parts;
    if (t >= ra.T_h) return;
    const uint32_t n = ra.rest_n[t];            // 0: not a hybrid table of this request, nothing flagged, or too much for this kernel
    if (n == 0 || n > static_cast<uint32_t>(kRestCap)) return;
    const int bits = static_cast<int>(ra.rbits[static_cast<size_t>(t) * ra.rbits_stride]);
    const unsigned trace_id = 16384u + blockIdx.x;      // (experiment builds: PM_STAMP; nothing otherwise)
    (void)trace_id;
    PM_STAMP(trace_id, 0);
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    // 1. gather
    const uint32_t chunk = ((n + kRestThreads - 1) / kRestThreads) * kWave;      // positions per wave: a multiple of 64, NW * chunk >= n
    uint32_t key[kRestItems], val[kRestItems];
    {
        const PM_GLOBAL uint32_t* sk = as_global<uint32_t>(ra.stage + static_cast<size_t>(t) * 2 * kRestCap);
        const PM_GLOBAL uint32_t* sv = sk + kRestCap;
#pragma unroll
        for (int r = 0; r < kRestItems; ++r) {
            const uint32_t off = static_cast<uint32_t>(r) * kWave + lane, pos = wave * chunk + off;
            const uint32_t e = (off < chunk && pos < n) ? pos : n - 1u;            // straight-line: positions past the end read the last pair again
            key[r] = sk[e];
            val[r] = sv[e];
        }
    }
    PM_STAMP_DRAINED(trace_id, 2);
    // 2. stable LSD sort by the table's row bits
    const int rounds = (bits + 7) / 8;
    uint32_t* const wcnt = s_aux + wave * 256;
    uint32_t* const s_dstart = s_aux + NW * 256;
    for (int rd = 0; rd < rounds; ++rd) {
        const int shift = 8 * rd;
        const int w = (bits - shift) < 8 ? (bits - shift) : 8;
        const uint32_t mask = (1u << w) - 1u;
        for (int i = threadIdx.x; i < NW * 256; i += kRestThreads) s_aux[i] = 0u;
        __syncthreads();
        uint32_t rank[kRestItems];
#pragma unroll
        for (int r = 0; r < kRestItems; ++r) {
            rank[r] = 0;
            if (static_cast<uint32_t>(r) * kWave < chunk) {          // wave-uniform
                const uint32_t off = static_cast<uint32_t>(r) * kWave + lane;
                const bool valid = off < chunk && wave * chunk + off < n;
                const uint32_t d = (key[r] >> shift) & mask;
                uint32_t below, total;
                match_digit<8>(d, valid, below, total);
                const uint32_t b0 = valid ? wcnt[d] : 0u;
                rank[r] = b0 + below;
                // the lowest lane of each match set advances the digit's counter; a wave executes its LDS operations in program order
                if (valid && below == 0) wcnt[d] = b0 + total;
            }
        }
        __syncthreads();
        uint32_t acc_d = 0;
        if (threadIdx.x < 256) {
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                const uint32_t c = s_aux[ww * 256 + threadIdx.x];
                s_aux[ww * 256 + threadIdx.x] = acc_d;                // wave ww's pairs of this digit start this far into the digit's run
                acc_d += c;
            }
        }
        const uint32_t ex = rest_excl_scan<NW>(acc_d, s_tmp);
        if (threadIdx.x < 256) s_dstart[threadIdx.x] = ex;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRestItems; ++r) {
            const uint32_t off = static_cast<uint32_t>(r) * kWave + lane;
            if (off < chunk && wave * chunk + off < n) {
                const uint32_t d = (key[r] >> shift) & mask;
                const uint32_t qp = s_dstart[d] + wcnt[d] + rank[r];
                s_key[qp] = key[r];
                s_val[qp] = val[r];
            }
        }
        __syncthreads();
        if (rd + 1 < rounds) {
#pragma unroll
            for (int r = 0; r < kRestItems; ++r) {
                const uint32_t off = static_cast<uint32_t>(r) * kWave + lane, pos = wave * chunk + off;
                if (off < chunk && pos < n) {
                    key[r] = s_key[pos];
                    val[r] = s_val[pos];
                }
            }
            __syncthreads();                    // everybody has its pairs back before the next round overwrites the staged order
        }
    }
    if (rounds == 0) {                          // a one-row table: list order is the sorted order
#pragma unroll
        for (int r = 0; r < kRestItems; ++r) {
            const uint32_t off = static_cast<uint32_t>(r) * kWave + lane, pos = wave * chunk + off;
            if (off < chunk && pos < n) {
                s_key[pos] = key[r];
                s_val[pos] = val[r];
            }
        }
        __syncthreads();
    }
    // 3. apply this part's slice of the sorted positions (no barrier from here on)
    PM_STAMP(trace_id, 3);
    const int gid = threadIdx.x / G, lig = threadIdx.x % G;
    const uint32_t sa = static_cast<uint32_t>(static_cast<uint64_t>(n) * part / ra.parts);
    const uint32_t sb = static_cast<uint32_t>(static_cast<uint64_t>(n) * (part + 1) / ra.parts);
    const uint32_t C = (sb - sa + NG - 1) / NG;
    const uint32_t l0 = sa + static_cast<uint32_t>(gid) * C;
    if (C == 0 || l0 >= sb) return;
    const uint32_t l1 = l0 + C < sb ? l0 + C : sb;
    uint32_t pos = l0;                          // first head at or after l0 ...
    if (pos > 0) while (pos < n && s_key[pos] == s_key[pos - 1]) ++pos;
    uint32_t end = l1;                          // ... up to the first head at or after l1
    while (end < n && s_key[end] == s_key[end - 1]) ++end;
    if (pos >= end) return;
    const int D = q.dims[t];
    char* const W = reinterpret_cast<char*>(const_cast<void*>(q.tables[t]));
    const float* const grad_t = p.grad + q.out_offsets[t];
    float* const mom_t = OPT == 1 ? p.mom[t] : (OPT == 2 ? p.state[t] : nullptr);
    const int nt_rows = p.nt_rows;
    const uint64_t tkey = static_cast<uint64_t>(t) << p.tshift;
    const char* const dummy = reinterpret_cast<const char*>(p.partials) + static_cast<size_t>(lig) * VEC * sizeof(float);
    PM_STAMP_DRAINED(trace_id, 4);
    const int c_end = column_pass_end<OPT, VEC>(lig, D);
    for (int c = lig * VEC; c < c_end; c += G * VEC) {
        const bool any_col = c < D;
        float acc[VEC], wrow[VEC];
        float srow[OPT == 2 ? VEC : 1];     // OPT 2: the open run's state values of this lane's columns
#pragma unroll
        for (int k = 0; k < VEC; ++k) { acc[k] = 0.0f; wrow[k] = 0.0f; }
#pragma unroll
        for (int k = 0; k < (OPT == 2 ? VEC : 1); ++k) srow[k] = 0.0f;
        float cur_mom = 0.0f;
        uint32_t cur_row = 0;
        bool open = false;
        auto close_run = [&]() {
            char* wptr = W + (static_cast<int64_t>(cur_row) * D + c) * DST::kES;
            float* const state = OPT == 0 ? nullptr : mom_t + (OPT == 2 ? static_cast<int64_t>(cur_row) * D + c : static_cast<int64_t>(cur_row));
            finish_row<DST, G, OPT>(wptr, wrow, acc, srow, any_col, state, cur_mom, D, p, lig, nt_rows, tkey | cur_row, c);
        };
        for (uint32_t q0 = pos; q0 < end; q0 += KB) {
            uint32_t rw[KB], bg[KB];
            bool valid[KB], head[KB];
#pragma unroll
            for (int u = 0; u < KB; ++u) {      // straight-line: positions past the walk read its last pair again (dropped below)
                valid[u] = q0 + u < end;
                const uint32_t qq = valid[u] ? q0 + u : end - 1u;
                rw[u] = s_key[qq];
                bg[u] = s_val[qq];
                head[u] = valid[u] && (qq == 0u || s_key[qq - 1u] != rw[u]);
            }
            float gv[KB][VEC];
            u32x4 wraw[KB];
            float mv[KB];
            u32x4 sraw[KB][OPT == 2 ? VEC / 4 : 1];
#pragma unroll
            for (int u = 0; u < KB; ++u) {      // every load of the batch before the first add; positions that need none read a harmless address
                const float* g = (valid[u] && any_col) ? grad_t + grad_bag_offset(static_cast<int64_t>(bg[u]), q.out_stride, q.gblk_shift, q.gblk_extra) + c
                                                       : reinterpret_cast<const float*>(dummy);
                load_grad<VEC>(as_global<f32x4>(g), gv[u]);
                // (row, state value and element-wise state: the same three lines as in the bag-major kernel; one helper for both moved
                // every instance of this kernel)
                wraw[u] = DST::load_raw((head[u] && any_col) ? W + (static_cast<int64_t>(rw[u]) * D + c) * DST::kES : dummy, nt_rows);
                mv[u] = 0.0f;
                if (OPT == 1) mv[u] = *as_global<float>(head[u] ? mom_t + rw[u] : reinterpret_cast<const float*>(dummy));
                if constexpr (OPT == 2)
                    state_load_raw<VEC>((head[u] && any_col) ? reinterpret_cast<const char*>(mom_t + static_cast<int64_t>(rw[u]) * D + c) : dummy, sraw[u], nt_rows);
            }
#pragma unroll
            for (int u = 0; u < KB; ++u) {
                if (valid[u]) {                 // uniform over the lane group
                    if (head[u]) {
                        if (open) close_run();
                        open = true;
                        cur_row = rw[u];
                        cur_mom = mv[u];
#pragma unroll
                        for (int k = 0; k < VEC; ++k) { acc[k] = 0.0f; wrow[k] = 0.0f; }
                        if (any_col) open_row<DST, OPT>(wraw[u], sraw[u], acc, wrow, srow);
                    }
                    if (any_col) add_scaled<VEC>(acc, p.alpha, gv[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < KB; ++u) {      // every loaded register counts as read (see the main kernel's batch)
#pragma unroll
                for (int k = 0; k < VEC; ++k) asm volatile("" : : "v"(gv[u][k]));
                asm volatile("" : : "v"(wraw[u]));
                asm volatile("" : : "v"(mv[u]));
                if constexpr (OPT == 2) {
#pragma unroll
                    for (int k = 0; k < VEC / 4; ++k) asm volatile("" : : "v"(sraw[u][k]));
                }
            }
        }
        if (open) close_run();
        PM_STAMP(trace_id, 5);                  // (lane group 0's last row loads have returned; its stores are under way)
    }
    PM_STAMP_DRAINED(trace_id, 6);
}
