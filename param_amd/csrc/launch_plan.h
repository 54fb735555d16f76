// param_amd/csrc/launch_plan.h -- a request's launch geometry as pure host functions of (request, element type, knobs).
// No HIP, no atomics, no environment: capi.hip snapshots the knobs once per call (current_knobs) and copies a plan into KParams;
// tests/launch_plan_dump.cpp compiles this header with a plain C++ compiler and tests/test_launch_plan_host.py pins what it plans.
// (The functions are static: the libraries export nothing of them.)
#pragma once

#include <stdint.h>

#include "param_amd.h"

namespace pm {

constexpr int kBlock = 256;  // 4 wave64 per workgroup
constexpr int kXcds = 8;     // MI355X: 8 XCDs, block b is dispatched to XCD b % 8 (speed only)

// lanes per bag for a given widest row: next power of two >= max_dim / vec, clamped to [8, 64]
inline int group_lanes(int max_dim, int vec) {
    int need = (max_dim + vec - 1) / vec;
    int g = 8;
    while (g < need && g < 64) g <<= 1;
    return g;
}

// Row loads a lane group keeps in flight in the forward.  Round 3 found that rounds 1-2 had measured this knob with ONE load
// in flight whatever its value (a wait at the merge of the staged / unstaged index paths, embbag_fwd.hip); with the batch
// real: 1 -> 19.3 G lookups/s Zipf / 0.727 of the HBM peak uniform, 2 -> 22.2 / 0.734, 3 -> 21.5 / 0.712, 4 -> 21.7 / 0.732,
// 6 -> 21.3 / 0.712, 8 -> 21.4 / 0.732 (48 x 10 M x 128 fp32, profiles/r03_fwd_unroll_sweep.txt); Criteo 14.1 / 15.6 / 15.1 at 1 / 2 / 4.
constexpr int kDefaultUnroll = 2;
constexpr int kBurstBytes = 16384;     // the LDS-staged output burst: a tile's pooled rows must fit this
constexpr int64_t kMaxGrid = 0x7fffffffLL;

// ---- knobs --------------------------------------------------------------------------------------------------------------------
// The forward's environment switches (kernel sweeps; every one has a pm_set_* or a default that the product uses); the values
// here are the defaults.
struct FwdEnv {
    int stage = 1;         // PARAM_AMD_FWD_STAGE=0: no LDS-staged output burst
    int flat = 1;          // PARAM_AMD_FWD_FLAT=0: no flat-walk kernel; 2: also for pooling factors up to 4
    int flat_maxl = 0;     // PARAM_AMD_FLAT_MAXL
    int flat_target = 256; // PARAM_AMD_FLAT_TARGET (lookups per flat-walk tile)
    int flat_bags = 256;   // PARAM_AMD_FLAT_BAGS (bags per flat-walk tile at most)
    int tile_major = -1;   // PARAM_AMD_FWD_TILE_MAJOR=1
    int flat_compact = 1;  // PARAM_AMD_FLAT_COMPACT=0: the flat-walk kernel's old grid (T x smallest-tile count); N > 1: exactly N workgroups
    int drain_split = 4;   // PARAM_AMD_FWD_DRAIN_SPLIT=0 (or 1): the last round's tiles are not split; N: by N workgroups each (a power of two)
    int round_wgs = 0;     // PARAM_AMD_FWD_ROUND_WGS=N: N resident workgroups per XCD instead of what the device reports (tests, sweeps)
};
// what pm_set_tuning and pm_set_forward_tuning were last given; the values here are "not set"
struct TuningSetters {
    int unroll = 0, bags_per_block = 0, xcd_affine = -1, nt_loads = -1;   // pm_set_tuning
    int stage_out = -1, flat_grid = -1, flat_target = -1;                 // pm_set_forward_tuning
};
// One call's view of every knob, resolved: a setter value >= 0 (flat_target: > 0) wins, otherwise the environment's, otherwise the
// default.  A plan is a function of this snapshot, so every plan is one that some knob setting describes.
struct PlanKnobs {
    int unroll;          // 0: the library chooses
    int bags_per_block;  // <= 0: the library chooses
    int xcd_affine;      // 0: plain table-major block order
    int nt_loads;        // > 0: non-temporal row loads (< 0: not set -- the sorted backward then has its own default)
    int stage;           // 0: no output burst
    int flat;            // FwdEnv::flat
    int flat_maxl;
    int flat_target;     // >= 1
    int flat_bags;
    int flat_grid;       // 0: grid of T x smallest-tile count; 1: as many resident workgroups as the request has tiles; N > 1: exactly N
    int tile_major;
    int drain_split;     // FwdEnv::drain_split
    int round_wgs;       // FwdEnv::round_wgs
};
static inline PlanKnobs resolve_knobs(const TuningSetters& s, const FwdEnv& e) {
    PlanKnobs k;
    k.unroll = s.unroll;
    k.bags_per_block = s.bags_per_block;
    k.xcd_affine = s.xcd_affine;
    k.nt_loads = s.nt_loads;
    k.stage = s.stage_out >= 0 ? s.stage_out : e.stage;
    k.flat = e.flat;
    k.flat_maxl = e.flat_maxl;
    k.flat_target = s.flat_target > 0 ? s.flat_target : e.flat_target;
    if (k.flat_target < 1) k.flat_target = 1;   // (an environment value of 0 or text: the grid estimate divides by it)
    k.flat_bags = e.flat_bags;
    k.flat_grid = s.flat_grid >= 0 ? s.flat_grid : e.flat_compact;
    k.tile_major = e.tile_major;
    k.drain_split = e.drain_split;
    k.round_wgs = e.round_wgs;
    return k;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------
// The geometry members of KParams (common.h describes each) and the forward's unroll (0 where the launch has none): the twelve members
// pm_embbag_plan reports.  Behind them, unreported: what the plan asks of the launch's last round (with_drain_split); the launcher turns
// it into KParams' members of the same names once it knows the resident workgroups (resolve_drain_split).
struct LaunchPlan {
    int32_t tiles_per_table, bags_per_block, idx_cap, xcd_affine, nt_loads, ordered;
    int32_t stage_out, stage_bags, flat_bags, flat_target, flat_compact;
    int32_t unroll;
    int32_t round_wgs;     // > 0: resident workgroups per XCD given by the knob; 0: the launcher asks the device
    int32_t drain_split;   // > 1: the last round's tiles pooled by this many workgroups each
};

// what the rules below read of a request, derived once
struct PlanShape {
    int vec;             // elements per 16-byte load
    int G, NG;           // lanes per lane group (sized for max_dim), lane groups per workgroup
    int64_t total_bags;  // T * B
    int64_t avg_l;       // lookups per bag, rounded up
    bool even;           // the lookups divide evenly over the bags (fixed pooling: every benchmark shape)
    bool uneven;         // ... they certainly do not: the request is ragged (a request without bags is neither)
    int base_tile;       // bags per tile of the plain bag-count tiling (tile_bags): the host's grid check and every plan start from it
};

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }
// LDS index tile (entries): twice what `bags` bags hold on average, in steps of 256, at least `floor`
static inline int64_t index_tile(int64_t bags, int64_t avg_l, int64_t floor) {
    const int64_t cap = round256(2 * bags * avg_l);
    return cap < floor ? floor : cap;
}
// bags per flat-walk tile at most: the knob in whole lane-group rounds, within [floor, 1024]
// (whole rounds, not a power of two: PARAM_AMD_FLAT_BAGS=48 plans 48-bag tiles)
static inline int flat_bag_cap(int knob, int floor, int NG) { return knob < floor ? floor : (knob > 1024 ? 1024 : knob / NG * NG); }
// the largest tile from `bpb` down (halving, not below one bag per lane group) whose rows of max_dim elem_bytes-elements fit the burst
static inline int burst_tile(int bpb, int NG, int max_dim, int elem_bytes) {
    while (bpb > NG && static_cast<int64_t>(bpb) * max_dim * elem_bytes > kBurstBytes) bpb /= 2;
    return bpb;
}

// bags per tile of the plain bag-count tiling (s: everything of the shape but base_tile)
static inline int tile_bags(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k) {
    const int NG = s.NG;
    int bpb = k.bags_per_block;
    if (bpb <= 0) {
        // 4 bags per lane group amortise the LDS staging; small requests shrink the tile until the
        // grid fills the chip (256 CUs x 8 resident workgroups) -- a 16 K-bag single-table lookup
        // ran 2 workgroups per CU at 49 % of the roofline with the fixed tile (sweep r1e)
        bpb = 4 * NG;
        // Short average bags go with one bag per lane group: requests whose tables have very different bag
        // sizes (Criteo multi-hot 1 .. 100, average 8.2) otherwise leave a few tables' workgroups 100x longer
        // than the rest -- measured 7.2 (32 bags/tile) vs 14.3 G lookups/s (8); with uniform L = 20 the
        // 32-bag tile is 3.5 % faster under Zipf and 2 % slower under uniform indices (sweeps r1f/r1g).
        if (s.total_bags > 0 && op.num_indices < 12 * s.total_bags) bpb = NG;
        const int64_t want_blocks = 256 * 8;
        while (bpb > NG && op.num_tables * ceil_div(op.bag_count, bpb) < want_blocks) bpb /= 2;
    }
    if (bpb < NG) bpb = NG;
    if (bpb > 1024) bpb = 1024;
    return bpb;
}

// A request's shape, derived once per call: capi.hip's validate_request checks the base tile's grid and hands the shape to the plan.
static inline PlanShape plan_shape(const pm_embbag_batch& op, int elem_dtype, const PlanKnobs& k) {
    PlanShape s;
    s.vec = (elem_dtype == PM_F32) ? 4 : 8;
    s.G = group_lanes(op.max_dim, s.vec);
    s.NG = kBlock / s.G;
    s.total_bags = static_cast<int64_t>(op.num_tables) * op.batch;
    s.avg_l = s.total_bags > 0 ? (op.num_indices + s.total_bags - 1) / s.total_bags : 0;
    s.even = s.total_bags > 0 && op.num_indices % s.total_bags == 0;
    s.uneven = s.total_bags > 0 && !s.even;
    s.base_tile = tile_bags(op, s, k);
    return s;
}

// Each kind of plan below comes twice: for a shape the caller has derived already (capi.hip), and for (request, element type, knobs).

// ---- base: the plain bag-count tiling of every backward, check, bounds, psw-grad, split, mean-grad and widen entry ----------------
static inline LaunchPlan plan_base(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k) {
    LaunchPlan p = {};
    p.bags_per_block = s.base_tile;
    p.tiles_per_table = static_cast<int32_t>(ceil_div(op.bag_count, p.bags_per_block));
    // tables of one request can have very different bag sizes (Criteo multi-hot 1 .. 100 at an average of 8): the full 4096 entries
    // (16 KiB of LDS per workgroup) unless the request is weighted -- then twice the tile's average, at least 2048
    const int64_t cap = index_tile(p.bags_per_block, s.avg_l, op.per_sample_weights ? 2048 : 4096);
    p.idx_cap = static_cast<int32_t>(cap > 4096 ? 4096 : cap);
    // T % 8 == 0: table t on XCD t % 8.  Any other table count (26 tables: BASELINE configs[3]): contiguous eighths of the
    // table-major tile order (common.h) -- 26 x 10 M x 128, [B, sum D] output: 0.692 -> 0.700 of the HBM peak under uniform indices,
    // 19.6 -> 21.15 G lookups/s under Zipf (tools/r4_fwd_xcd.py) -- but only where every table has the same lookups per tile: with
    // the Criteo tables' pooling factors of 1 .. 100 the XCD that gets the 100-hot table does a third of the launch (0.70 -> 0.27)
    const bool eighths = op.num_tables > 1 && s.even;
    if (k.xcd_affine == 0) p.xcd_affine = 0;
    // blocked requests (table_group = W consecutive request tables read ONE weight table): contiguous eighths of the
    // table-major tile order keep a weight table's blocks on one XCD; t % 8 would spread them over all eight
    else if (op.table_group > 1 && eighths) p.xcd_affine = 3;
    else p.xcd_affine = op.num_tables % kXcds == 0 ? 1 : (eighths ? 3 : 0);
    p.nt_loads = k.nt_loads > 0 ? k.nt_loads : 0;   // forward: any non-zero = non-temporal row loads; sorted backward: 1 nt, 2 system scope
    // lookups that do not divide evenly over the bags: certainly ragged (fixed-size requests -- every benchmark shape --
    // always divide; a ragged request that happens to divide merely runs the unordered kernel)
    // ... and only where the order can matter: with one bag per lane group (short-bag tiles) nothing is pulled
    p.ordered = (s.uneven && p.bags_per_block > s.NG) ? 1 : 0;
    return p;
}
static inline LaunchPlan plan_base(const pm_embbag_batch& op, int elem_dtype, const PlanKnobs& k) {
    return plan_base(op, plan_shape(op, elem_dtype, k), k);
}

// ---- forward: the steps pm_embbag_fwd's plan takes from the base plan, in this order -------------------------------------------------
// LDS-staged output: the tile's pooled rows leave in one burst at the end of the tile (embbag_fwd.hip).
// Measured at benchmark size: uniform indices 0.69 -> 0.72-0.74 of the HBM peak in both output layouts, Zipf within
// +-2 % -- provided the workgroup's LDS stays small (at 6 workgroups per CU the latency-bound Zipf launch lost 12 %):
// so only for requests whose lookups divide evenly over the bags (fixed pooling: every benchmark shape), whose index
// tile can then be sized for what a tile really holds instead of the 4096-entry default, and only where the staging
// buffer fits 16 KB (the tile is halved until it does; an explicit bags_per_block -- sweeps -- is staged if it fits as it is).
// pm_set_forward_tuning(0) / PARAM_AMD_FWD_STAGE=0 turn it off.
static inline LaunchPlan with_burst_buffer(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, LaunchPlan p) {
    const bool auto_tile = k.bags_per_block <= 0;
    if (k.stage && !p.ordered && s.even) {
        const int bpb = auto_tile ? burst_tile(p.bags_per_block, s.NG, op.max_dim, 4) : p.bags_per_block;
        const int64_t tiles = ceil_div(op.bag_count, bpb);
        if (static_cast<int64_t>(bpb) * op.max_dim * 4 <= kBurstBytes && tiles * op.num_tables <= kMaxGrid) {
            p.bags_per_block = bpb;
            p.tiles_per_table = static_cast<int32_t>(tiles);
            p.stage_out = op.max_dim;
            const int64_t need = index_tile(bpb, s.avg_l, 512);
            if (need < p.idx_cap) p.idx_cap = static_cast<int32_t>(need);
        }
    } else if (k.stage && !p.ordered && auto_tile && static_cast<int64_t>(p.bags_per_block) * op.max_dim * 4 <= 4096) {
        // short-bag tiles of requests with per-table pooling (Criteo multi-hot: one bag per lane group, 8 bags per
        // tile): the staging buffer is 4 KB, the full-size index tile stays -- 20.6 KB per workgroup
        p.stage_out = op.max_dim;
    }
    p.stage_bags = p.bags_per_block;
    return p;
}

// Short-bag requests run the flat-walk kernel (embbag_fwd.hip): tiles sized per table on the device (~256 lookups, up
// to 32 bags for the pooling-1 tables), row loads in flight across bag borders.  tiles_per_table stays the count of the
// smallest tile (one bag per lane group): workgroups past their table's tile count leave.  Criteo tables, visit
// r3_criteo_flat (Zipf G lookups/s / uniform fraction; run-to-run +-1.5 %): 8-bag tiles 15.7-15.9 / 0.69-0.71; flat walk
// target 512 cap 64: 16.4-16.5 / 0.705-0.716; **256 / 32: 16.6 / 0.719**; 128: 16.1 / 0.695; 1024 / 128: 14.1 / 0.64.
// PARAM_AMD_FWD_FLAT=0 turns it off (PARAM_AMD_FLAT_TARGET / _BAGS: sweeps).
// (Round 6: that cap of 32 bags was chosen under round 3's grid, where a larger cap also meant more surplus workgroups.  With
// the compact launch a one-hot table's 32-bag tile is three round trips of set-up around 32 row loads; one process per setting,
// three each, us uniform / Zipf: cap 32: 192-193 / 118; 64: 182 / 114; 128: 186 / 112; **256: 181 / 111.6**
// -- profiles/r06_flat_bags_cap_sweep_all128.jsonl.  The cap is 256 bags on every flat-walk path now.)
// Two kinds of request take it: ragged ones already on one bag per lane group with a staged tile (Criteo multi-hot), and
// fixed-pooling requests of one or two lookups per bag (one-hot tables): bag by bag a lane group has one or
// two row loads in flight.  48 x 10 M x 128 fp32, batch 65536 (tools/r3_shortbags.sh; Zipf G lookups/s / uniform fraction):
// pooling 1: 4.00 / 0.529 -> 5.05 / 0.624; pooling 2: 7.78 / 0.687 -> 8.75 / 0.686; pooling 4: 13.5 / 0.723 -> 13.4 / 0.679
// (not taken; PARAM_AMD_FWD_FLAT=2 extends the rule to 4 for that measurement).
static inline LaunchPlan with_short_bag_flat_walk(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, LaunchPlan p) {
    if (!k.flat || p.ordered || k.bags_per_block > 0 || p.stage_out <= 0) return p;
    const int64_t tiles_ng = ceil_div(op.bag_count, s.NG);
    if (s.even && s.avg_l <= (k.flat_maxl > 0 ? k.flat_maxl : k.flat == 2 ? 4 : 2) && tiles_ng * op.num_tables <= kMaxGrid) {
        p.flat_bags = flat_bag_cap(k.flat_bags, 32, s.NG);
        p.flat_target = k.flat_target;
        p.tiles_per_table = static_cast<int32_t>(tiles_ng);
        p.stage_bags = s.NG;
        p.bags_per_block = p.flat_bags;
        if (p.idx_cap < 1024) p.idx_cap = 1024;
    } else if (!s.even && p.bags_per_block == s.NG) {
        p.flat_bags = flat_bag_cap(k.flat_bags, s.NG, s.NG);
        p.flat_target = k.flat_target;
        p.bags_per_block = p.flat_bags;   // sizes the LDS offsets array; stage_bags (the burst buffer) stays at NG rows
    }
    return p;
}

// ABI v7, mixed embedding dims (min_dim given and its lane group narrower than max_dim's): the flat-walk kernel sizes the lane
// group PER TABLE on the device (embbag_fwd.hip), whatever the bags look like -- tiles are ~flat_target lookups of any pooling
// factor.  Ragged requests keep the ordered kernel (longest bag first matters more there than idle lanes).
static inline LaunchPlan with_mixed_dims(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, LaunchPlan p) {
    if (!k.flat || op.min_dim <= 0 || op.min_dim >= op.max_dim || p.ordered || k.bags_per_block > 0) return p;
    int need = (op.min_dim + s.vec - 1) / s.vec, g_min = 4;          // sub-groups of 4 lanes at least: 64-byte pieces
    while (g_min < need) g_min <<= 1;
    const int64_t tiles_ng = ceil_div(op.bag_count, s.NG);             // the grid of the smallest tile: the widest table's NG bags
    if (g_min >= s.G || tiles_ng * op.num_tables > kMaxGrid) return p;
    const int ng_max = kBlock / g_min;                                 // bags the narrowest table's sub-groups pool at once (64 at most)
    // 256 bags at most per tile (the LDS offsets array): a one-hot narrow table then reaches the ~flat_target lookups per tile the wide
    // tables have -- its 64-bag tiles were three round trips of set-up around 4 KB of rows.  Criteo tables with mixed dims, one
    // process per setting, two each: cap 64: 143.3-143.9 us, 128: 142.3-142.9, 256: 141.5-142.1; the narrow tables alone
    // 24.3 -> 21.6 us: profiles/r06_flat_bags_cap_sweep.jsonl
    if (p.flat_bags < 256) p.flat_bags = 256;
    if (p.flat_target <= 0) p.flat_target = k.flat_target;
    p.tiles_per_table = static_cast<int32_t>(tiles_ng);
    p.bags_per_block = p.flat_bags;
    p.stage_out = op.max_dim;                                          // (staged even with stage_out 0: the flat walk has no unstaged path)
    p.stage_bags = s.NG;                                               // burst buffer: NG rows of max_dim floats (4 KB at D = 128 fp32)
    // index tile: twice what a tile holds on average -- ~flat_target lookups, or the narrowest table's ng_max bags -- within [1024, 4096]
    int64_t cap = index_tile(ng_max, s.avg_l, 1024);
    if (cap < round256(2 * static_cast<int64_t>(p.flat_target))) cap = round256(2 * static_cast<int64_t>(p.flat_target));
    p.idx_cap = static_cast<int32_t>(cap > 4096 ? 4096 : cap);
    if (p.xcd_affine == 3) p.xcd_affine = 0;                           // eighths of the tile order assume equal tiles per table
    return p;
}

// flat-walk launches are one resident set of workgroups walking the tile order (embbag_fwd.hip, round 6)
static inline LaunchPlan with_compact_grid(const pm_embbag_batch& op, const PlanKnobs& k, LaunchPlan p) {
    if (p.flat_bags <= 0 || op.num_tables > 1024 || k.flat_grid <= 0) return p;
    // the tiles the request will have, from its sizes (the tables' own pooling factors are on the device): ~flat_target
    // lookups each, but at most flat_bags bags; a quarter more, because a table's tile is its average bag count rounded DOWN
    // to whole lane-group rounds
    const int64_t n_slice = op.batch > 0 ? ceil_div(op.num_indices * op.bag_count, op.batch) : 0;
    const int64_t by_lookups = ceil_div(n_slice, p.flat_target);
    const int64_t by_bags = op.num_tables * ceil_div(op.bag_count, p.flat_bags);
    int64_t est = (by_lookups > by_bags ? by_lookups : by_bags) * 5 / 4 + op.num_tables;
    if (est < 1024) est = 1024;
    if (est > (1 << 20)) est = 1 << 20;
    p.flat_compact = k.flat_grid > 1 ? k.flat_grid : static_cast<int32_t>(est);
    return p;
}

// Two tilings built and measured in round 3 for requests whose tables have very different pooling factors (Criteo
// multi-hot 1 .. 100) -- both slower than the 8-bag tiles in table-major order, which stay:
//  * WORK tiles (~640 lookups per tile whatever the pooling factor, tile boundaries derived on the device from the
//    tables' lookup counts): 186 us against 120 us under Zipf, 249 against 185 us under uniform indices (caps of
//    32 .. 1024 bags, targets of 320 .. 1280: all slower).  A pooling-1 bag is ONE row load; a lane group walking 16 ..
//    128 of them in turn has one load in flight where 1024 eight-bag workgroups have them all in flight at once -- the
//    small tiles ARE the memory-level parallelism.  Removed again (profiles/r03_criteo_fwd_work_tiles.txt).
//  * tile-major block order (t = b % T, so every table advances at the same rate and the heavy table's long workgroups
//    start throughout the launch): 165 against 120 us under Zipf, 220 against 186 us uniform -- a table's tiles then run
//    on all eight XCDs at once and on every CU next to other tables' rows.  Kept behind PARAM_AMD_FWD_TILE_MAJOR=1.
static inline LaunchPlan with_tile_major(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, LaunchPlan p) {
    if (p.xcd_affine != 1 && op.num_tables > 1 && k.tile_major > 0 && s.uneven) p.xcd_affine = 2;
    return p;
}

// Row loads in flight per lane group when pm_set_tuning leaves the choice to the library.  Two is the measured optimum of a launch
// that fills the chip (eight workgroups per CU: occupancy provides the memory-level parallelism).  A SMALL request -- the reference
// driver's batch 512 .. 4096 rows of one 14 M x 128 table, train/compute/pt/dataset.py:56-82 -- has one or two workgroups per CU,
// each lane group a chain of pooling / 2 dependent round trips: there a deeper batch IS the parallelism.  Additions stay in index
// order: same bits for every value.
static inline int small_request_unroll(const pm_embbag_batch& op, const PlanShape& s, const LaunchPlan& p) {
    if (p.flat_bags > 0 || p.ordered) return kDefaultUnroll;
    const int64_t wgs = static_cast<int64_t>(op.num_tables) * p.tiles_per_table;
    const int64_t avg_l = s.total_bags > 0 ? op.num_indices / s.total_bags : 0;   // (rounded down)
    // kernel us under rocprofv3 --kernel-trace (profiles/r06_small_batch_kernel_us.txt; batch 2 / 4 / 8): 64 workgroups 6.6 / 5.6 / 5.5,
    // 128: 6.9 / 6.0 / 5.6, 256: 9.6 / 7.7 / 6.6, 512: 13.0 / 13.1 / 13.1, 1024: 22.4 / 22.6 / 23.1 -- it pays up to one workgroup per CU
    if (wgs > 384) return kDefaultUnroll;
    return avg_l >= 8 ? 8 : (avg_l >= 4 ? 4 : kDefaultUnroll);
}

static inline LaunchPlan forward_geometry(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k) {
    LaunchPlan p = plan_base(op, s, k);
    p = with_burst_buffer(op, s, k, p);
    p = with_short_bag_flat_walk(op, s, k, p);
    p = with_mixed_dims(op, s, k, p);
    p = with_compact_grid(op, k, p);
    return with_tile_major(op, s, k, p);
}

// ---- forward: pm_embbag_fwd -------------------------------------------------------------------------------------------------------
// A short final drain (drain_block_tile, further down): the tiles of an XCD's last round are pooled by S workgroups each.  Offered where
// the order is t % 8 and the kernel is the staged bag-count one -- fixed pooling, not ordered, not the flat walk -- and left to the
// launcher (embbag_fwd.hip), which knows how many workgroups of the launched instance are resident.  None of the reported members
// moves.  S: a power of two, and a part keeps whole lane-group rounds of bags (S <= bags_per_block / NG).
// Same process, the switch taking turns, medians of 7 windows, spreads <= 0.25 % (profiles/fwd_round_timeline.md; us off -> S = 4):
//   48 x 10 M x 128 fp32 [T, B, D]   Zipf 361.3 -> 358.8 (0.7 %)   uniform 754.4 -> 751.3 (0.4 %)        S = 2: 358.5 / 752.9
//   the same, [B, sum D]              Zipf 364.8 -> 360.7 (1.1 %)   uniform 764.7 -> 760.6 (0.5 %)
//   64 x 10 M x 128 bf16 [T, B, D]   Zipf 277.9 -> 275.5 (0.9 %)   uniform 539.3 -> 537.8 (0.3 %)
// The XCD's last full residency to its last workgroup's end: 44 -> 18 us of the Zipf launch; that it buys 2.6 us says the drain was not
// idle time -- the launch is bound behind L2, and fewer workgroups still keep that path busy.
// Built, measured and removed with it: whole-round table passes (tiles 0 .. R - 1 of each of the XCD's tables in turn, the left-overs
// last).  One table resident 30 -> 63 % of the launch, L2 misses 17.40 M -> 17.13 M (1.5 %), the launch 0.56 % SLOWER (361.3 -> 363.3 us).
static inline LaunchPlan with_drain_split(const PlanShape& s, const PlanKnobs& k, LaunchPlan p) {
    if (p.xcd_affine != 1 || p.stage_out <= 0 || p.ordered || p.flat_bags > 0 || !s.even) return p;
    int split = 1;
    while (split * 2 <= k.drain_split && split * 2 * s.NG <= p.bags_per_block && p.bags_per_block % (split * 2) == 0) split *= 2;
    p.drain_split = split;
    p.round_wgs = split > 1 && k.round_wgs > 0 ? k.round_wgs : 0;
    return p;
}

static inline LaunchPlan plan_forward(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k) {
    LaunchPlan p = forward_geometry(op, s, k);
    p.unroll = k.unroll != 0 ? k.unroll : small_request_unroll(op, s, p);
    return with_drain_split(s, k, p);
}
static inline LaunchPlan plan_forward(const pm_embbag_batch& op, int elem_dtype, const PlanKnobs& k) {
    return plan_forward(op, plan_shape(op, elem_dtype, k), k);
}

// ---- quantized: pm_embbag_fwd_quantized (it refuses a plan that is not staged) -----------------------------------------------------
static inline LaunchPlan plan_quantized(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k) {
    LaunchPlan p = forward_geometry(op, s, k);
    if (p.flat_bags > 0) {   // the quantised burst lives in the bag-per-group kernel: back to its tiles of one bag per lane group
        p.bags_per_block = p.stage_bags;
        p.flat_bags = 0;
    }
    p.unroll = k.unroll != 0 ? k.unroll : kDefaultUnroll;
    return p;
}
static inline LaunchPlan plan_quantized(const pm_embbag_batch& op, int elem_dtype, const PlanKnobs& k) {
    return plan_quantized(op, plan_shape(op, elem_dtype, k), k);
}

// ---- padded: pm_embbag_fwd_padded, pm_embbag_fwd_mean (out_bytes 4) and pm_embbag_fwd_out16 (2) -------------------------------------
// The padded forward keeps the plain bag-count tiling and adds the product forward's output burst where the tile's rows of
// out_bytes-elements fit 16 KB (the tile is halved until they do; it only shrinks, so the base plan's grid check holds); requests whose
// lookups divide evenly over the bags get an index tile sized for what a tile holds, as the product forward's do (a longer tile reads
// its indices from the request).  The kernel has no ordered variant.
static inline LaunchPlan plan_padded(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, int out_bytes) {
    LaunchPlan p = plan_base(op, s, k);
    if (k.bags_per_block <= 0) p.bags_per_block = burst_tile(p.bags_per_block, s.NG, op.max_dim, out_bytes);
    p.tiles_per_table = static_cast<int32_t>(ceil_div(op.bag_count, p.bags_per_block));
    p.stage_out = (k.stage && static_cast<int64_t>(p.bags_per_block) * op.max_dim * out_bytes <= kBurstBytes) ? op.max_dim : 0;
    p.stage_bags = p.bags_per_block;
    if (s.even) {
        const int64_t need = index_tile(p.bags_per_block, s.avg_l, 512);
        if (need < p.idx_cap) p.idx_cap = static_cast<int32_t>(need);
    }
    p.ordered = 0;
    return p;
}
static inline LaunchPlan plan_padded(const pm_embbag_batch& op, int elem_dtype, const PlanKnobs& k, int out_bytes) {
    return plan_padded(op, plan_shape(op, elem_dtype, k), k, out_bytes);
}

// ---- qrows: pm_embbag_fwd_qrows (embbag_fwd_qrows.hip) -- pooled lookup over 8- / 4-bit row-quantised tables ---------------------------
// A lane holds kQrowsLaneDwords DWORDS of a row's codes -- with two: 8 columns of an 8-bit row, 16 of a 4-bit row -- and the lane group
// is sized for max_dim in those units (group_lanes), for every table of the request: a narrower table of a mixed request idles lanes
// (no per-table sub-groups).  Measured, tools/qrows_probe.py (16 x 10 M x 128, batch 8192, pooling 20; us, 8-bit / 4-bit tables, fp32
// output, uniform | Zipf; one process per build, the bf16-table lookup 134.7-136.5 | 71.9-73.5 in all three):
//   1 dword per lane  (global_load_dword)      139.8 / 105.6 | 89.3 / 64.1      profiles/qrows_probe_lane_dwords1.json
//   2 (global_load_dwordx2, dword-aligned)     132.0 / 103.7 | 77.3 / 60.5      profiles/qrows_probe.json -- the product
//   4 (global_load_dwordx4, dword-aligned)     133.1 / 184.2 | 67.4 / 162.9     profiles/qrows_probe_lane_dwords4.json
// Four would be the 8-bit format's optimum (Zipf: 13 % over two) and is the 4-bit format's worst (4 of 8 lanes hold a D = 128 row, on 32
// accumulators); and a lane's 16 bytes reach past the row's END for 8-bit rows of D % 16 == 4 and 4-bit rows of D % 32 == 8 / 16 --
// past the table for its last row.  With two, the dwords behind a row's codes are always the row's own tail.  -DPM_QROWS_LANE_DWORDS=1
// / =4 are experiment builds (4: for widths that are a multiple of 16 / 32 columns only).  A width per format: left as the follow-up.
// The plan is the padded forward's, from the same blocks: the plain bag-count tiling (tile_bags), halved until the tile's rows of
// out_bytes-elements fit the burst buffer (burst_tile; an explicit bags_per_block is kept and bursts only if it fits), and an index tile
// sized for what a tile holds where the lookups divide evenly over the bags (index_tile; a longer tile reads its indices from the
// request).  No ordered variant, no flat walk, plain row loads.
// Rows in flight per lane group: 2 or 4 (pm_set_tuning's unroll: below 4 -> 2, from 4 on -> 4).  Same probe, two dwords per lane, 2 / 4
// rows in flight: 8-bit 134.7 / 132.0 uniform, 79.0 / 77.2 Zipf; 4-bit 104.3 / 103.7, 62.3 / 60.5 -- four is never slower, and the fp32
// forward's optimum of 2 does not carry over: kQrowsUnroll is this kernel's own default.
#ifndef PM_QROWS_LANE_DWORDS
#define PM_QROWS_LANE_DWORDS 2
#endif
constexpr int kQrowsLaneDwords = PM_QROWS_LANE_DWORDS;
constexpr int kQrowsUnroll = 4;
constexpr int kQrowsMaxDim = 4096;     // columns per row at most (8 column passes of the widest lane group over an 8-bit row)
static inline int qrows_elem_dtype(int bits) { return bits == 8 ? PM_F32 : PM_BF16; }   // the element type with the format's column rule (D % 4, D % 8)
static inline int qrows_lane_columns(int bits) { return kQrowsLaneDwords * (bits == 8 ? 4 : 8); }
// the request's shape for this kernel's lane group (plan_shape's, with the columns a lane holds in place of an element type's)
static inline PlanShape lane_columns_shape(const pm_embbag_batch& op, int lane_columns, const PlanKnobs& k) {
    PlanShape s;
    s.vec = lane_columns;
    s.G = group_lanes(op.max_dim, s.vec);
    s.NG = kBlock / s.G;
    s.total_bags = static_cast<int64_t>(op.num_tables) * op.batch;
    s.avg_l = s.total_bags > 0 ? (op.num_indices + s.total_bags - 1) / s.total_bags : 0;
    s.even = s.total_bags > 0 && op.num_indices % s.total_bags == 0;
    s.uneven = s.total_bags > 0 && !s.even;
    s.base_tile = tile_bags(op, s, k);
    return s;
}
static inline PlanShape qrows_shape(const pm_embbag_batch& op, int bits, const PlanKnobs& k) { return lane_columns_shape(op, qrows_lane_columns(bits), k); }
static inline LaunchPlan plan_qrows(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, int out_bytes) {
    LaunchPlan p = plan_base(op, s, k);
    if (k.bags_per_block <= 0) p.bags_per_block = burst_tile(p.bags_per_block, s.NG, op.max_dim, out_bytes);
    p.tiles_per_table = static_cast<int32_t>(ceil_div(op.bag_count, p.bags_per_block));
    p.stage_out = (k.stage && static_cast<int64_t>(p.bags_per_block) * op.max_dim * out_bytes <= kBurstBytes) ? op.max_dim : 0;
    p.stage_bags = p.bags_per_block;
    if (s.even) {
        const int64_t need = index_tile(p.bags_per_block, s.avg_l, 512);
        if (need < p.idx_cap) p.idx_cap = static_cast<int32_t>(need);
    }
    p.ordered = 0;
    p.nt_loads = 0;
    const int u = k.unroll != 0 ? k.unroll : kQrowsUnroll;
    p.unroll = u >= 4 ? 4 : 2;
    return p;
}
static inline LaunchPlan plan_qrows(const pm_embbag_batch& op, int bits, const PlanKnobs& k, int out_bytes) {
    return plan_qrows(op, qrows_shape(op, bits, k), k, out_bytes);
}

// ---- qmixed: pm_embbag_fwd_qrows_mixed (embbag_fwd_qmixed.hip) -- pooled lookup over tables that are EACH 8- or 4-bit ------------------
// A lane holds kQmixedLaneColumns = EIGHT COLUMNS of a row whatever its format: two dwords of an 8-bit row (plan_qrows' product setting)
// and ONE dword of a 4-bit row (measured above for a 4-bit-only launch: 105.6 against 103.7 us uniform, 64.1 against 60.5 us Zipf).  With
// it the lane group G = group_lanes(max_dim, 8), the eight accumulators, the column passes and the output pieces are the same for every
// table of the launch, and the host needs no knowledge of which formats are present: the plan is plan_qrows' for a lane of eight columns,
// a function of the request struct, out_dtype and the knobs alone.  The alternative -- two dwords per lane for both formats, 16 columns of
// a 4-bit row -- idles half the lanes of a 4-bit table of the widest width (G stays sized for the 8-bit rows); the pooled kernel has it as
// the experiment build -DPM_QMIXED_4BIT_DWORDS=2 (embbag_fwd_qmixed.hip).  Measured, tools/qmixed_probe.py (16 x 10 M x 128, tables
// alternately 8- and 4-bit, batch 8192, pooling 20; us, fp32 / fp16 output, uniform | Zipf; one process per build):
//   eight columns per lane for both      121.3 / 117.3 |  78.3 /  72.3      profiles/qmixed_probe.json -- the product
//   two dwords per lane for both         121.5 / 118.8 | 104.2 / 102.7      profiles/qmixed_probe_lane_dwords2.json
// (serving shape 64 x 1 M x 64, batch 256: 10.6 against 11.0).  Two dwords lose a third under Zipf indices: half the lanes of every 4-bit
// tile idle (why that costs so much more under Zipf than under uniform indices has not been looked into: no counters were collected).
constexpr int kQmixedLaneColumns = 8;
static inline PlanShape qmixed_shape(const pm_embbag_batch& op, const PlanKnobs& k) { return lane_columns_shape(op, kQmixedLaneColumns, k); }
static inline LaunchPlan plan_qmixed(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, int out_bytes) { return plan_qrows(op, s, k, out_bytes); }
static inline LaunchPlan plan_qmixed(const pm_embbag_batch& op, const PlanKnobs& k, int out_bytes) { return plan_qmixed(op, qmixed_shape(op, k), k, out_bytes); }

// ---- gather: pm_embedding_gather (embedding_gather.hip) -- un-pooled rows, one output row per lookup POSITION ---------------------------
// A tile is kBlock consecutive positions of the index array, whatever tables they belong to: the output is addressed by position, so
// nothing about a tile depends on bags.  A lane group moves one row at a time and owns kBlock / NG = G of the tile's positions.
// Rows a lane group keeps in flight (two batches of that many ping-pong, embedding_gather.hip).  Nothing depends on a loaded row but its
// own store, so the forward's optimum (kDefaultUnroll = 2) does not carry over: the deepest batch wins although it runs on 230
// registers and two waves per SIMD.  tools/gather_probe.py, 16 x 10 M x 128, 2.6 M lookups, us per call, medians of 5 windows of one
// process, spread <= 1 % (profiles/gather_probe.json); unroll 1 / 2 / 4 / 8:
//   fp32 -> fp32, uniform indices 517.9 / 505.3 / 493.6 / 486.9      Zipf 366.8 / 356.9 / 346.2 / 338.9
//   bf16 -> bf16, uniform indices 252.2 / 245.1 / 241.1 / 239.8      Zipf 181.3 / 175.4 / 171.9 / 160.5
// (the pooled forward of the same rows as bags of one: 557.6 / 394.6 / 402.2 / 408.5 us; an earlier visit, with 4 as the default, ordered
// the four values the same way in every case)
constexpr int kGatherUnroll = 8;
constexpr int kGatherLdsBorders = kBlock;   // T + 1 table borders are staged in LDS up to this many (one load per thread), searched in global memory beyond
struct GatherPlan {
    int32_t vec;             // table elements per 16-byte load
    int32_t group_lanes;     // G: lanes that move one row
    int32_t tile;            // positions per workgroup (= kBlock: the tile's indices are one coalesced load, one per lane)
    int32_t col_passes;      // passes of G * vec columns over the widest row (fp32 D > 256: more than one)
    int32_t unroll;          // rows in flight per lane group: 1, 2, 4 or 8 (divides G)
    int32_t lds_borders;     // 1: the T + 1 table borders are staged in LDS; 0: every position searches them in global memory
    int32_t xcd_contiguous;  // 1: XCD x serves the x-th eighth of the tile order (a table's rows meet in one or two L2s)
    int64_t grid;            // workgroups: ceil(num_indices / tile), every position in exactly one
};
// block -> tile, host and device (constexpr): the identity, or common.h's xcd_contiguous_tile -- a bijection of [0, total) for any total
constexpr int64_t gather_block_tile(int64_t bid, int64_t total, bool xcd_contiguous) {
    return !xcd_contiguous ? bid : (bid % kXcds) * (total / kXcds) + ((bid % kXcds) < (total % kXcds) ? (bid % kXcds) : (total % kXcds)) + bid / kXcds;
}
// ---- the split last round (xcd_affine == 1 launches of the staged bag-count kernel) ----------------------------------------------------
// XCD x = block % 8 serves the n = T / 8 tables x, x + 8, ...; its blocks, in dispatch order, are its SLOTS 0 .. n * tiles_per_table - 1,
// the tiles of its tables in table-major order (what block_to_tile's xcd_affine == 1 branch computes).  With R workgroups resident per
// XCD and S > 1, the XCD's last (slots mod R) slots -- its last round -- are each pooled by S workgroups, part q taking bags
// [q, q + 1) * bags_per_block / S of the tile.  Part 0 is the slot's own block; parts 1 .. S - 1 are blocks appended behind the
// T x tiles_per_table grid, 8 * (slots mod R) * (S - 1) of them, slot-major, on the XCD of their table (T % 8 == 0: the appended blocks
// start at a multiple of 8).
// A bijection of [0, T * tiles_per_table + extra) onto the (table, tile, part) triples for every (T % 8 == 0, tiles_per_table, R, S):
// tests/test_drain_split_host.py.  Host and device (constexpr), 32-bit: resolve_drain_split keeps the grid within kMaxGrid.
struct BlockTile {
    int32_t table, tile;
    int32_t part, parts;   // this block pools part `part` of the tile's `parts` equal runs of bags (1: the whole tile)
};
constexpr BlockTile drain_block_tile(int32_t bid, int32_t T, int32_t tiles_per_table, int32_t R, int32_t S) {
    const int32_t main_grid = T * tiles_per_table;
    const int32_t slots = T / kXcds * tiles_per_table;
    const int32_t drain = S > 1 ? slots % R : 0;
    int32_t xcd = bid % kXcds, slot = bid / kXcds, part = 0;
    if (bid >= main_grid) {
        const int32_t e = bid - main_grid;
        xcd = e % kXcds;
        slot = slots - drain + (e / kXcds) / (S - 1);
        part = 1 + (e / kXcds) % (S - 1);
    }
    return BlockTile{xcd + kXcds * (slot / tiles_per_table), slot % tiles_per_table, part, slot >= slots - drain ? S : 1};
}
// What a launch does with the plan's wish (LaunchPlan::drain_split) once R is known: KParams' members and the blocks to append.  Only
// where it can matter: more than one round per XCD (grid > 8 * R) and a last round that is not a whole one; all zero = the plain order,
// the kernel's plain path.
struct DrainSplit {
    int32_t round_wgs, drain_split;
    int32_t extra_blocks;
};
constexpr DrainSplit resolve_drain_split(int32_t T, int32_t tiles_per_table, int32_t R, int32_t want_split) {
    if (R <= 0 || T % kXcds != 0 || tiles_per_table <= 0 || want_split <= 1) return DrainSplit{0, 0, 0};
    const int64_t slots = static_cast<int64_t>(T / kXcds) * tiles_per_table;
    const int64_t extra = kXcds * (slots % R) * (want_split - 1);
    if (slots <= R || extra == 0 || static_cast<int64_t>(T) * tiles_per_table + extra > kMaxGrid) return DrainSplit{0, 0, 0};
    return DrainSplit{R, want_split, static_cast<int32_t>(extra)};
}

static inline GatherPlan plan_gather(const pm_embbag_batch& op, int elem_dtype, const PlanKnobs& k) {
    GatherPlan g = {};
    g.vec = (elem_dtype == PM_F32) ? 4 : 8;
    g.group_lanes = group_lanes(op.max_dim, g.vec);
    g.tile = kBlock;
    g.col_passes = static_cast<int32_t>(ceil_div(op.max_dim, static_cast<int64_t>(g.group_lanes) * g.vec));
    // pm_set_tuning's unroll (1, 2, 3, 4, 6, 8) rounded down to a divisor of every group width
    const int u = k.unroll != 0 ? k.unroll : kGatherUnroll;
    g.unroll = u >= 8 ? 8 : (u >= 4 ? 4 : (u >= 2 ? 2 : 1));
    g.lds_borders = op.num_tables + 1 <= kGatherLdsBorders ? 1 : 0;
    g.xcd_contiguous = (op.num_tables > 1 && k.xcd_affine != 0) ? 1 : 0;
    g.grid = ceil_div(op.num_indices, g.tile);
    return g;
}

// ---- gather over row-quantised tables: pm_embedding_gather_qrows (embedding_gather_qrows.hip) -------------------------------------------
// The gather's tiles and block order; the lane group is the pooled qrows kernel's: a lane holds kQrowsLaneDwords dwords of a row's codes
// (qrows_lane_columns: 8 columns of an 8-bit row, 16 of a 4-bit row), G = group_lanes(max_dim, that), and rows wider than G such pieces
// take column passes (8-bit D > 512, 4-bit D > 1024; at most 8 at kQrowsMaxDim).  vec: the columns a lane holds per pass.
// Rows in flight per lane group: pm_set_tuning's unroll rounded down to 1 / 2 / 4 / 8, as plan_gather rounds it.  The default is this
// kernel's own, measured: its two parents disagree (kGatherUnroll = 8, kQrowsUnroll = 4).  tools/qgather_probe.py, 16 x 10 M x 128,
// 2.6 M lookups, us per call, medians of 5 windows of one process, spread <= 0.9 % (profiles/qgather_probe.json); unroll 1 / 2 / 4 / 8:
//   8-bit -> fp32, uniform indices 385.4 / 378.6 / 374.7 / 374.9      Zipf 376.4 / 371.2 / 360.7 / 355.4
//   8-bit -> fp16, uniform indices 252.0 / 244.3 / 242.3 / 242.3      Zipf 187.9 / 183.0 / 179.7 / 177.0
//   4-bit -> fp32, uniform indices 353.1 / 345.1 / 341.6 / 341.7      Zipf 335.6 / 318.3 / 327.7 / 327.2
//   4-bit -> fp16, uniform indices 295.8 / 265.6 / 272.1 / 273.0      Zipf 317.4 / 285.2 / 298.7 / 299.0
// (4-bit D = 128 is a group of 8 lanes: 4 and 8 are one batch of 4 / 8 rows).  Eight is the 8-bit format's optimum or within 0.1 % of it
// everywhere; the 4-bit format would take two (up to 4.8 % faster than eight in three of its four cases, 1 % slower in the fourth).  ONE
// default: eight -- with two the 8-bit lookups lose 1 .. 4.4 %.  D = 512 (groups of 64 / 32 lanes, 0.66 M lookups, uniform): 8-bit 359.2 /
// 366.3 / 358.8 / 367.6, 4-bit 312.2 / 311.7 / 322.7 / 319.5 -- within 2.5 % of each other.  A default per format: not built.
constexpr int kQgatherUnroll = 8;
static inline GatherPlan plan_gather_qrows(const pm_embbag_batch& op, int bits, const PlanKnobs& k) {
    GatherPlan g = {};
    g.vec = qrows_lane_columns(bits);
    g.group_lanes = group_lanes(op.max_dim, g.vec);
    g.tile = kBlock;
    g.col_passes = static_cast<int32_t>(ceil_div(op.max_dim, static_cast<int64_t>(g.group_lanes) * g.vec));
    const int u = k.unroll != 0 ? k.unroll : kQgatherUnroll;
    g.unroll = u >= 8 ? 8 : (u >= 4 ? 4 : (u >= 2 ? 2 : 1));
    g.lds_borders = op.num_tables + 1 <= kGatherLdsBorders ? 1 : 0;
    g.xcd_contiguous = (op.num_tables > 1 && k.xcd_affine != 0) ? 1 : 0;
    g.grid = ceil_div(op.num_indices, g.tile);
    return g;
}

// ---- gather over tables that are EACH 8- or 4-bit: pm_embedding_gather_qrows_mixed (embedding_gather_qmixed.hip) -----------------------------
// plan_gather_qrows with plan_qmixed's lane: eight columns per lane and pass for both formats, so rows wider than 512 columns take column
// passes whatever their format (at most 8 at kQrowsMaxDim).  The format is a row's, so lane groups of one wave may differ in it; the
// plan does not know the formats.  Rows in flight: plan_gather_qrows' rounding and default (kQgatherUnroll).
static inline GatherPlan plan_gather_qmixed(const pm_embbag_batch& op, const PlanKnobs& k) {
    GatherPlan g = {};
    g.vec = kQmixedLaneColumns;
    g.group_lanes = group_lanes(op.max_dim, g.vec);
    g.tile = kBlock;
    g.col_passes = static_cast<int32_t>(ceil_div(op.max_dim, static_cast<int64_t>(g.group_lanes) * g.vec));
    const int u = k.unroll != 0 ? k.unroll : kQgatherUnroll;
    g.unroll = u >= 8 ? 8 : (u >= 4 ? 4 : (u >= 2 ? 2 : 1));
    g.lds_borders = op.num_tables + 1 <= kGatherLdsBorders ? 1 : 0;
    g.xcd_contiguous = (op.num_tables > 1 && k.xcd_affine != 0) ? 1 : 0;
    g.grid = ceil_div(op.num_indices, g.tile);
    return g;
}

// ---- MIXED-FORMAT tables: pm_embbag_fwd_anyfmt (embbag_fwd_anyfmt_kernel.inc) and pm_embedding_gather_anyfmt (embedding_gather_anyfmt.hip) --
// Every table of a launch in its own format (fp32, bf16, fp16, FP8 e4m3fn / e5m2, 8- / 4-bit rows).  plan_qmixed's argument, extended: a
// lane holds kAnyfmtLaneColumns = EIGHT COLUMNS of a row whatever its format, so the lane group G = group_lanes(max_dim, 8), the column
// passes (more than one above 512 columns; kAnyfmtMaxDim = 2048: four) and the output pieces are one for every table, and the plan is
// a function of the request struct, out_dtype and the knobs alone -- the host never learns which formats are present.  The pooled plan
// is plan_qmixed's but for the rows in flight: those are a compile-time value per format in the kernel (the format's own product
// default), so `unroll` is reported as 0 and pm_set_tuning's unroll is not read.  The un-pooled kernel branches per lane group and keeps
// kAnyfmtGatherUnroll rows in flight (a compile-time value as well; it divides every group width).
constexpr int kAnyfmtLaneColumns = 8;
constexpr int kAnyfmtMaxDim = 2048;
constexpr int kAnyfmtGatherUnroll = 4;
static inline PlanShape anyfmt_shape(const pm_embbag_batch& op, const PlanKnobs& k) { return lane_columns_shape(op, kAnyfmtLaneColumns, k); }
static inline LaunchPlan plan_anyfmt(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, int out_bytes) {
    LaunchPlan p = plan_qrows(op, s, k, out_bytes);
    p.unroll = 0;
    return p;
}
static inline GatherPlan plan_gather_anyfmt(const pm_embbag_batch& op, const PlanKnobs& k) {
    GatherPlan g = {};
    g.vec = kAnyfmtLaneColumns;
    g.group_lanes = group_lanes(op.max_dim, g.vec);
    g.tile = kBlock;
    g.col_passes = static_cast<int32_t>(ceil_div(op.max_dim, static_cast<int64_t>(g.group_lanes) * g.vec));
    g.unroll = kAnyfmtGatherUnroll;
    g.lds_borders = op.num_tables + 1 <= kGatherLdsBorders ? 1 : 0;
    g.xcd_contiguous = (op.num_tables > 1 && k.xcd_affine != 0) ? 1 : 0;
    g.grid = ceil_div(op.num_indices, g.tile);
    return g;
}

// ---- FP8 tables: pm_embbag_fwd_f8 (embbag_fwd_f8.hip) and pm_embedding_gather_f8 (embedding_gather_f8.hip) ------------------------------
// The 1-byte element: a 16-byte load holds 16 columns (vec = 16, elem_bytes = 1), so the pooled lane group is group_lanes(max_dim, 16) --
// 8 lanes up to D = 128 (one aligned 128-byte line per row), 64 lanes at D = 1024, column passes above (kF8MaxDim = 2048: two).
// The plan is plan_padded's, from the same blocks (tile_bags, burst_tile for out_bytes-elements, index_tile), plus the rows a lane group
// keeps in flight: 2, 4 or 8 (pm_set_tuning's unroll: below 4 -> 2, below 8 -> 4, from 8 on -> 8).  At 128-byte rows two rows in flight
// are a quarter of the fp32 kernel's bytes in flight, and the gather and the qrows kernels both measured better with deeper batches --
// this kernel does not.  tools/f8_probe.py, 16 x 10 M x 128 e4m3, batch 8192, pooling 20, fp32 output, us per call, medians of 5 windows
// of one process, spread <= 0.25 % (profiles/f8_probe.json); 2 / 4 / 8 rows in flight:
//   uniform indices 78.0 / 78.5 / 88.7      Zipf 1.05  48.6 / 50.7 / 64.4
// Two is the default, as in the fp32 forward (kDefaultUnroll): occupancy provides the memory-level parallelism, and the deeper
// instances pay for their registers (70 to 166 VGPRs across the instances).  fp16 output (64-bag tiles, half the workgroups) is
// another matter under Zipf indices: 50.7 us at two, 43.8 us in the earlier run of the probe whose default was four
// (profiles/f8_probe_unroll4_default.json; two processes, not one).  A default per output type: not built.
constexpr int kF8Unroll = 2;
constexpr int kF8MaxDim = 2048;
constexpr int kF8LaneColumns = 16;
static inline PlanShape f8_shape(const pm_embbag_batch& op, const PlanKnobs& k) { return lane_columns_shape(op, kF8LaneColumns, k); }
static inline LaunchPlan plan_f8(const pm_embbag_batch& op, const PlanShape& s, const PlanKnobs& k, int out_bytes) {
    LaunchPlan p = plan_qrows(op, s, k, out_bytes);   // (the same tiling for this shape's lane group; the unroll is this kernel's own)
    const int u = k.unroll != 0 ? k.unroll : kF8Unroll;
    p.unroll = u >= 8 ? 8 : (u >= 4 ? 4 : 2);
    return p;
}
static inline LaunchPlan plan_f8(const pm_embbag_batch& op, const PlanKnobs& k, int out_bytes) { return plan_f8(op, f8_shape(op, k), k, out_bytes); }

// The un-pooled lookup: the gather's tiles and block order with FOUR columns per lane (kF8GatherLaneColumns) -- one global_load_dword per
// lane and row, G = group_lanes(max_dim, 4) lanes (32 at D = 128, 64 from D = 256 on, column passes of 256 columns above).  Stores are the
// point: with the pooled kernel's 16 columns per lane one store instruction of a lane group writes 16 of every 64 output bytes, the layout
// that cost the qrows gather 643.7 against 374.9 us (profiles/qgather_probe_lane_major.json); with four, a lane's widened dword is exactly
// one 16-byte (fp32) / 8-byte (16-bit) piece and a lane group's store instruction writes consecutive pieces of the row, while its loads
// still cover the row contiguously.  The 16-column load with a lane exchange: not built.  Rows in flight: plan_gather's rounding.
constexpr int kF8GatherLaneColumns = 4;
constexpr int kF8GatherUnroll = 8;
static inline GatherPlan plan_gather_f8(const pm_embbag_batch& op, const PlanKnobs& k) {
    GatherPlan g = {};
    g.vec = kF8GatherLaneColumns;
    g.group_lanes = group_lanes(op.max_dim, g.vec);
    g.tile = kBlock;
    g.col_passes = static_cast<int32_t>(ceil_div(op.max_dim, static_cast<int64_t>(g.group_lanes) * g.vec));
    const int u = k.unroll != 0 ? k.unroll : kF8GatherUnroll;
    g.unroll = u >= 8 ? 8 : (u >= 4 ? 4 : (u >= 2 ? 2 : 1));
    g.lds_borders = op.num_tables + 1 <= kGatherLdsBorders ? 1 : 0;
    g.xcd_contiguous = (op.num_tables > 1 && k.xcd_affine != 0) ? 1 : 0;
    g.grid = ceil_div(op.num_indices, g.tile);
    return g;
}

}  // namespace pm
