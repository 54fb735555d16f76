// param_amd/csrc/capi.hip -- extern "C" entry points of libparam_amd.so (include/param_amd.h).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "common.h"

namespace pm {
// row-quantised tables (embbag_fwd_qrows.hip): p.io = out of out_dtype, addressed in its elements; bits 8 | 4; unroll: plan_qrows'
hipError_t launch_embbag_fwd_qrows(const KParams& p, int bits, int out_dtype, int max_dim, int unroll, hipStream_t stream);
// ... of per-table format (embbag_fwd_qmixed.hip): table_bits = device int32 [T], 8 | 4; unroll: plan_qmixed's
hipError_t launch_embbag_fwd_qmixed(const KParams& p, const int32_t* table_bits, int out_dtype, int max_dim, int unroll, hipStream_t stream);
// ... whose rows may be pruned (embbag_fwd_qpruned.hip, embedding_gather_qpruned.hip): remap = device int32, remap_offsets = device int64
// [T + 1]; the geometry is the per-table-format calls' (plan_qmixed, plan_gather_qmixed)
hipError_t launch_embbag_fwd_qpruned(const KParams& p, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, int out_dtype,
                                     int max_dim, int unroll, hipStream_t stream);
hipError_t launch_embedding_gather_qpruned(const KParams& p, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets, int out_dtype,
                                           const GatherPlan& g, hipStream_t stream);
// mixed-format tables (embbag_fwd_anyfmt_{f32,bf16,f16}.hip: one translation unit per output type; embedding_gather_anyfmt.hip):
// table_formats = device int32 [T] of format codes, table_exp = device int32 [T] or NULL; the geometry is plan_anyfmt's / plan_gather_anyfmt's
hipError_t launch_embbag_fwd_anyfmt_f32(const KParams& p, const int32_t* table_formats, const int32_t* table_exp, int max_dim, hipStream_t stream);
hipError_t launch_embbag_fwd_anyfmt_bf16(const KParams& p, const int32_t* table_formats, const int32_t* table_exp, int max_dim, hipStream_t stream);
hipError_t launch_embbag_fwd_anyfmt_f16(const KParams& p, const int32_t* table_formats, const int32_t* table_exp, int max_dim, hipStream_t stream);
hipError_t launch_embedding_gather_anyfmt(const KParams& p, const int32_t* table_formats, const int32_t* table_exp, int out_dtype, const GatherPlan& g,
                                          hipStream_t stream);
}  // namespace pm

namespace {

thread_local std::string g_last_error;

std::atomic<int> g_unroll{0};
std::atomic<int> g_bags_per_block{0};
std::atomic<int> g_xcd_affine{-1};
std::atomic<int> g_nt_loads{-1};
std::atomic<int> g_stage_out{-1};
std::atomic<int> g_flat_target{-1}; // pm_set_forward_tuning: lookups per flat-walk tile (-1: PARAM_AMD_FLAT_TARGET, default 256)
std::atomic<int> g_flat_grid{-1};   // pm_set_forward_tuning: launch shape of the flat-walk forward (-1: PARAM_AMD_FLAT_COMPACT, default 1)
// destination-row cache policy of the sorted backward when pm_set_tuning leaves nt_loads at its default: plain loads,
// agent-scope (sc1) stores.  The store writes through and drops the row's lines from the XCD's L2, so a row occupies L2 only
// between its load and its store and the gradient rows -- re-read once per lookup of their bag -- keep the capacity
// (round 3, 48 x 10 M x 128 fp32, uniform indices: apply 1.58 -> 1.49 ms; Zipf 0.953 -> 0.943 ms).
constexpr int kDefaultRowPolicy = 3;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t rc, const char* what) {
    return fail(PM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(rc));
}

// The forward's environment switches (pm::FwdEnv, launch_plan.h): read ONCE per process, on the first request -- not on the launch
// path (getenv is not thread-safe against setenv, and a value that changes between two calls of one request's sequence is a hazard,
// not a feature).
const pm::FwdEnv& fwd_env() {
    const auto read = [] {
        auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        pm::FwdEnv r;
        const char* st = getenv("PARAM_AMD_FWD_STAGE");
        r.stage = (st && st[0] == '0') ? 0 : 1;
        r.flat = num("PARAM_AMD_FWD_FLAT", r.flat);
        r.flat_maxl = num("PARAM_AMD_FLAT_MAXL", r.flat_maxl);
        r.flat_target = num("PARAM_AMD_FLAT_TARGET", r.flat_target);
        r.flat_bags = num("PARAM_AMD_FLAT_BAGS", r.flat_bags);
        r.tile_major = num("PARAM_AMD_FWD_TILE_MAJOR", r.tile_major);
        r.flat_compact = num("PARAM_AMD_FLAT_COMPACT", r.flat_compact);
        r.drain_split = num("PARAM_AMD_FWD_DRAIN_SPLIT", r.drain_split);
        r.round_wgs = num("PARAM_AMD_FWD_ROUND_WGS", r.round_wgs);
        return r;
    };
#ifdef PM_EXPERIMENTS
    // experiment builds read the switches on every call, so that one process can measure them taking turns (tools/fwd_round_timeline.py)
    static thread_local pm::FwdEnv again;
    again = read();
    return again;
#else
    static const pm::FwdEnv e = read();
    return e;
#endif
}

// Every knob a plan reads, loaded once per call (apply_params alone reads one more, the sorted apply's row policy): a pm_set_* from another thread lands before or after a request's plan, never inside it.
pm::PlanKnobs current_knobs() {
    constexpr auto relaxed = std::memory_order_relaxed;
    pm::TuningSetters s;
    s.unroll = g_unroll.load(relaxed);
    s.bags_per_block = g_bags_per_block.load(relaxed);
    s.xcd_affine = g_xcd_affine.load(relaxed);
    s.nt_loads = g_nt_loads.load(relaxed);
    s.stage_out = g_stage_out.load(relaxed);
    s.flat_grid = g_flat_grid.load(relaxed);
    s.flat_target = g_flat_target.load(relaxed);
    return pm::resolve_knobs(s, fwd_env());
}

bool dtype_is_weight(int d) { return d == PM_F32 || d == PM_BF16 || d == PM_F16; }

const char* const kNoSortRecorded = "no sort has been recorded for this workspace";

// which of launch_plan.h's plans an entry point launches with
enum class PlanKind { base, forward, quantized, padded, padded16 };

// A request's launch parameters in two parts (defined below make_params): what can be refused -- for the element type the call
// reads or writes the tables as; shape: the request's shape, which the grid check derives and a plan starts from --, and the request
// with a plan's geometry as kernel arguments.
int validate_request(const pm_embbag_batch* op, int elem_dtype, const pm::PlanKnobs& knobs, pm::PlanShape* shape = nullptr);
void fill_params(const pm_embbag_batch* op, const pm::LaunchPlan& plan, pm::KParams& p);

// the plan of one kind (make_params for the launching entry points, pm_embbag_plan for the query: one choice, made here)
pm::LaunchPlan plan_of(const pm_embbag_batch& op, const pm::PlanShape& shape, const pm::PlanKnobs& knobs, PlanKind kind) {
    return kind == PlanKind::forward     ? pm::plan_forward(op, shape, knobs)
           : kind == PlanKind::quantized ? pm::plan_quantized(op, shape, knobs)
           : kind == PlanKind::padded    ? pm::plan_padded(op, shape, knobs, 4)
           : kind == PlanKind::padded16  ? pm::plan_padded(op, shape, knobs, 2)
                                         : pm::plan_base(op, shape, knobs);
}

// Validate the host-visible part of a request and derive the launch geometry: the plain bag-count tiling (base) for every entry point
// but the forwards, which name their own plan.  unroll: the plan's (forward, quantized).
int make_params(const pm_embbag_batch* op, int elem_dtype, pm::KParams& p, PlanKind kind = PlanKind::base, int* unroll = nullptr) {
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    const int rc = validate_request(op, elem_dtype, knobs, &shape);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan plan = plan_of(*op, shape, knobs, kind);
    fill_params(op, plan, p);
    if (unroll) *unroll = plan.unroll;
    return PM_OK;
}

// Everything a request can be refused for on the host, in the order the checks have always run: the same input gives the same first
// error.
int validate_request(const pm_embbag_batch* op, int elem_dtype, const pm::PlanKnobs& knobs, pm::PlanShape* shape) {
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    if (op->num_tables < 1) return fail(PM_ERR_INVALID, "num_tables must be >= 1");
    if (!dtype_is_weight(elem_dtype)) return fail(PM_ERR_INVALID, "weight/dst dtype must be PM_F32, PM_BF16 or PM_F16");
    if (op->index_dtype != PM_I64 && op->index_dtype != PM_I32)
        return fail(PM_ERR_INVALID, "index_dtype must be PM_I64 or PM_I32");
    if (op->batch < 0 || op->num_indices < 0) return fail(PM_ERR_INVALID, "negative batch / num_indices");
    if (op->bag_begin < 0 || op->bag_count < 0 || op->bag_begin + op->bag_count > op->batch)
        return fail(PM_ERR_INVALID, "bag_begin/bag_count outside [0, batch]");
    if (!op->tables || !op->rows || !op->dims || !op->out_offsets)
        return fail(PM_ERR_INVALID, "tables/rows/dims/out_offsets must be device pointers");
    if (op->bag_count > 0 && !op->offsets) return fail(PM_ERR_INVALID, "offsets is NULL");
    if (op->num_indices > 0 && !op->indices) return fail(PM_ERR_INVALID, "indices is NULL");
    const int vec = (elem_dtype == PM_F32) ? 4 : 8;
    if (op->max_dim < 1 || op->max_dim % vec != 0)
        return fail(PM_ERR_UNSUPPORTED, "every dims[t] (and max_dim) must be a multiple of " +
                                            std::to_string(vec) + " for this element type");
    if (op->out_stride % 4 != 0) return fail(PM_ERR_UNSUPPORTED, "out_stride must be a multiple of 4 elements");
    if (op->min_dim < 0 || op->min_dim > op->max_dim || (op->min_dim > 0 && op->min_dim % vec != 0))
        return fail(PM_ERR_INVALID, "min_dim must be 0 (not given) or a multiple of the vector width in [1, max_dim]");
    if (op->fixed_pooling < 0 ||
        (op->fixed_pooling > 0 && op->fixed_pooling * op->batch * static_cast<int64_t>(op->num_tables) != op->num_indices))
        return fail(PM_ERR_INVALID, "fixed_pooling must be 0 or num_indices / (num_tables * batch)");
    // the grid of the base plan's tile (the forward plans check their own smaller tiles and keep this one where those do not fit)
    const pm::PlanShape s = pm::plan_shape(*op, elem_dtype, knobs);
    if (shape) *shape = s;
    if ((op->bag_count + s.base_tile - 1) / s.base_tile * op->num_tables > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    if (op->grad_block_shift < 0 || op->grad_block_shift > 31 || op->grad_block_extra < 0 || op->table_group < 0)
        return fail(PM_ERR_INVALID, "grad_block_shift must be in [0, 31], grad_block_extra and table_group >= 0");
    // a blocked gradient needs blocks of at least two bags that tile the batch (shift 0 with a non-zero extra used to read
    // the un-blocked layout without a word, and so did a batch that is not a whole number of blocks)
    if (op->grad_block_shift == 0 && op->grad_block_extra != 0)
        return fail(PM_ERR_INVALID, "grad_block_extra needs grad_block_shift >= 1 (a block of one bag is the un-blocked layout)");
    if (op->grad_block_shift > 0 && (op->batch & ((static_cast<int64_t>(1) << op->grad_block_shift) - 1)) != 0)
        return fail(PM_ERR_INVALID, "batch must be a multiple of 2^grad_block_shift bags");
    return PM_OK;
}

void fill_params(const pm_embbag_batch* op, const pm::LaunchPlan& plan, pm::KParams& p) {
    p.tables = op->tables;
    p.rows = op->rows;
    p.dims = op->dims;
    p.out_offsets = op->out_offsets;
    p.indices = op->indices;
    p.offsets = op->offsets;
    p.psw = op->per_sample_weights;
    p.io = nullptr;
    p.out_stride = op->out_stride;
    p.B = op->batch;
    p.N = op->num_indices;
    p.bag_begin = op->bag_begin;
    p.bag_count = op->bag_count;
    p.T = op->num_tables;
    p.idx64 = op->index_dtype == PM_I64 ? 1 : 0;
    p.alpha = 1.0f;
    p.gblk_shift = op->grad_block_shift > 0 ? op->grad_block_shift : 31;
    p.gblk_extra = op->grad_block_shift > 0 ? op->grad_block_extra : 0;
    p.out_bits = 0;
    p.tiles_per_table = plan.tiles_per_table;
    p.bags_per_block = plan.bags_per_block;
    p.idx_cap = plan.idx_cap;
    p.xcd_affine = plan.xcd_affine;
    p.nt_loads = plan.nt_loads;
    p.ordered = plan.ordered;
    p.stage_out = plan.stage_out;
    p.stage_bags = plan.stage_bags;
    p.flat_bags = plan.flat_bags;
    p.flat_target = plan.flat_target;
    p.flat_compact = plan.flat_compact;
    p.round_wgs = plan.round_wgs;       // (what the plan asks of the launch's last round: the forward's launcher resolves it, embbag_fwd.hip)
    p.drain_split = plan.drain_split;
}

// ---- the sorted backward's entry points: what they share ---------------------------------------------------------------
// the one text of each reason the sort recorded on a workspace does not fit a call; kind: "row-wise" / "element-wise" (Adagrad)
int plan_fail(pm::PlanStatus st, const char* kind, bool sequence = false) {
    switch (st) {
        case pm::PlanStatus::ok: return PM_OK;
        case pm::PlanStatus::none:
            if (sequence)
                return fail(PM_ERR_INVALID, "pm_embseq_sort_indices has not been called for this request on this workspace (same indices / "
                                            "offsets pointers, batch and bag slice as the sort's)");
            return fail(PM_ERR_INVALID, "pm_embbag_sort_indices has not been called for this request on this workspace (same indices / "
                                        "offsets pointers, batch, bag slice and weights as the sort's)");
        case pm::PlanStatus::two_phase:
            return fail(PM_ERR_INVALID, std::string("the request was sorted for a two-phase scatter-add apply; ") + kind + " Adagrad needs "
                                        "pm_embbag_sort_indices (phases = 1)");
        case pm::PlanStatus::relabelled:
            return fail(PM_ERR_INVALID, "the sort on this workspace was relabelled by pm_embbag_sparse_grad_count (its keys hold slots, not "
                                        "rows): sort the request again");
        case pm::PlanStatus::not_complete_segmented:
            return fail(PM_ERR_UNSUPPORTED, "the sparse gradient needs the complete one-phase segmented sort: sort with pm_embbag_sort_indices "
                                            "(sort_impl 0)");
        case pm::PlanStatus::low_digit_order:
            return fail(PM_ERR_UNSUPPORTED, "the sparse gradient needs rows in ascending order within a table: sort mode 1 orders them by "
                                            "their low digit first (pm_set_sort_tuning 0, 2 or 3)");
        case pm::PlanStatus::sequence_sort:
            return fail(PM_ERR_INVALID, "the sort on this workspace is a sequence sort (pm_embseq_sort_indices: its values are lookup positions, "
                                        "not bags): only pm_embseq_bwd_sorted* may follow it; sort the request with pm_embbag_sort_indices");
        case pm::PlanStatus::pooled_sort:
            return fail(PM_ERR_INVALID, "the sort on this workspace is a pooled sort (pm_embbag_sort_indices: its values are bags, not lookup "
                                        "positions): a sequence apply needs pm_embseq_sort_indices");
        case pm::PlanStatus::already_counted:
            return fail(PM_ERR_INVALID, "pm_embbag_sparse_grad_count has been called for this sort already: sort the request again");
        default: return fail(PM_ERR_INVALID, "pm_embbag_sparse_grad needs pm_embbag_sparse_grad_count on this sort first");
    }
}

int sorted_args_ok(const pm_embbag_batch* op, int64_t max_rows) {
    if (max_rows < 1 || max_rows > (1LL << 31)) return fail(PM_ERR_INVALID, "max_rows must be in [1, 2^31]");
    if (op->num_indices >= (1LL << 32) || static_cast<int64_t>(op->batch) >= (1LL << 32))
        return fail(PM_ERR_UNSUPPORTED, "sorted backward needs num_indices and batch below 2^32");
#ifndef PM_ALTERNATES
    if (op->num_tables > pm::kSegSortMaxTables)
        return fail(PM_ERR_UNSUPPORTED, "sorted backward: at most " + std::to_string(pm::kSegSortMaxTables) +
                                            " tables per request (split the request by tables: the calls are independent)");
#endif
    return PM_OK;
}

// The request of a sorted call.  sparse: the coalesced sparse gradient (sparse_grad.hip), whose apply writes fp32 rows: its row-width
// rule (dims multiples of 4) is the fp32 destination's.
int sorted_request(const pm_embbag_batch* op, int dtype, int64_t max_rows, bool sparse, pm::KParams& p) {
    int rc = make_params(op, dtype, p);
    if (rc != PM_OK) return rc;
    if ((rc = sorted_args_ok(op, max_rows)) != PM_OK) return rc;
    return sparse ? validate_request(op, PM_F32, current_knobs()) : PM_OK;
}

// ... and its workspace.  sparse: the sorted backward's, followed by the relabelling's own few words per sorted position and per tile.
int sorted_bytes(const char* who, const pm_embbag_batch* op, int64_t max_rows, bool sparse, const pm::KParams& p, size_t& sorted,
                        size_t& total) {
    const hipError_t h = pm::sorted_workspace_bytes(p, max_rows, op->max_dim, sorted);
    if (h != hipSuccess) return hip_fail(h, who);
    if (sparse) sorted = (sorted + 255) / 256 * 256;
    total = sparse ? sorted + pm::sparse_grad_extra_bytes(p.N, p.T) : sorted;
    return PM_OK;
}

// How every sorted entry point opens, each step written once and in the order they have always run: the request, the caller's own
// argument checks and its nothing-to-do early-out (own_checks: PM_OK to go on, kDone to return PM_OK now), the workspace, and whether
// the sort recorded on it fits (plan: a pm::PlanStatus).  Returns PM_OK to go on, kDone, or the error.
constexpr int kDone = 1;      // (the PM_ERR_* codes are negative)
struct SortedCall {
    const char* who;          // names the call in a HIP error of the workspace size query
    int dtype;                // the element type the call reads or writes the tables as
    bool sparse;              // a sparse-gradient call (sorted_request, sorted_bytes); it sizes the workspace BEFORE its own checks
    const char* kind;         // Adagrad: "row-wise" / "element-wise"
    pm::KParams p;            // out: the request
    size_t sorted;            // out: bytes of the sorted backward's part of the workspace
    bool sequence = false;    // a pm_embseq_* call: names the sequence sort where no sort fits
};
template <typename Own, typename Plan>
int sorted_call_prologue(SortedCall& c, const pm_embbag_batch* op, int64_t max_rows, const void* workspace, int64_t workspace_bytes,
                         Own&& own_checks, Plan&& plan) {
    int rc = sorted_request(op, c.dtype, max_rows, c.sparse, c.p);
    if (rc != PM_OK) return rc;
    size_t need = 0;
    if (c.sparse && (rc = sorted_bytes(c.who, op, max_rows, true, c.p, c.sorted, need)) != PM_OK) return rc;
    if ((rc = own_checks()) != PM_OK) return rc;
    if (!c.sparse && (rc = sorted_bytes(c.who, op, max_rows, false, c.p, c.sorted, need)) != PM_OK) return rc;
    if (!workspace || workspace_bytes < static_cast<int64_t>(need))
        return fail(PM_ERR_INVALID, "workspace too small: need " + std::to_string(need) + " bytes" +
                                        (c.sparse ? " (pm_embbag_sparse_grad_workspace)" : ""));
    return plan_fail(plan(), c.kind, c.sequence);
}

// the sorted apply's view of the request: the gradient, the tables it updates, alpha and the default destination-row policy
// (a cache policy, no geometry: the one knob read outside current_knobs -- "not set" is not a value a plan carries)
void apply_params(pm::KParams& p, const float* grad, const void* tables, float alpha) {
    p.io = const_cast<float*>(grad);
    p.tables = static_cast<const void* const*>(tables);
    p.alpha = alpha;
    if (g_nt_loads.load() < 0) p.nt_loads = kDefaultRowPolicy;
}

// what pm_embbag_fwd_padded, pm_embbag_fwd_mean and pm_embbag_fwd_out16 do behind their own argument rules, on a padded plan
// (launch_plan.h).  out_align: bytes `out` must be aligned to, 0 for no rule beyond its element's; `launch`, `label`: the entry point's own.
template <typename Launch>
int padded_forward(pm::KParams& p, void* out, uintptr_t out_align, pm_stream_t stream, Launch&& launch, const char* label) {
    if (p.bag_count == 0) return PM_OK;
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    if (out_align && reinterpret_cast<uintptr_t>(out) % out_align != 0)
        return fail(PM_ERR_INVALID, "out must be " + std::to_string(out_align) + "-byte aligned");
    p.io = static_cast<float*>(out);           // (the 16-bit kernels address it as 2-byte elements)
    const hipError_t h = launch(p, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, label);
    return PM_OK;
}

}  // namespace

extern "C" {

int pm_abi_version(void) { return PM_ABI_VERSION; }

const char* pm_build_info(void) {
    return "libparam_amd gfx950 (CDNA4, wave64) hip " __VERSION__;
}

const char* pm_last_error(void) { return g_last_error.c_str(); }

int pm_set_tuning(int32_t unroll, int32_t bags_per_block, int32_t xcd_affine, int32_t nt_loads) {
    if (unroll != 0 && unroll != 1 && unroll != 2 && unroll != 3 && unroll != 4 && unroll != 6 && unroll != 8)
        return fail(PM_ERR_INVALID, "unroll must be 0, 1, 2, 3, 4, 6 or 8");
    if (bags_per_block < 0) return fail(PM_ERR_INVALID, "bags_per_block must be >= 0");
    g_unroll.store(unroll);
    g_bags_per_block.store(bags_per_block);
    g_xcd_affine.store(xcd_affine);
    g_nt_loads.store(nt_loads);
    return PM_OK;
}

int pm_set_forward_tuning(int32_t stage_out, int32_t flat_grid, int32_t flat_target) {
    if (stage_out < -1 || stage_out > 1) return fail(PM_ERR_INVALID, "stage_out must be -1, 0 or 1");
    if (flat_grid < -1 || flat_grid > (1 << 20)) return fail(PM_ERR_INVALID, "flat_grid must be -1 (default), 0, 1 or a workgroup count up to 2^20");
    if (flat_target < -1 || flat_target == 0 || flat_target > 4096) return fail(PM_ERR_INVALID, "flat_target must be -1 (default) or 1 .. 4096");
    g_stage_out.store(stage_out);
    g_flat_grid.store(flat_grid);
    g_flat_target.store(flat_target);
    return PM_OK;
}

// ---- the plan queries: what a forward entry point would launch with, from the same validate_request / plan_* calls it makes ------------
int pm_embbag_plan(const pm_embbag_batch* op, int32_t kind, int32_t out[12]) {
    if (kind < PM_PLAN_BASE || kind > PM_PLAN_PADDED16) return fail(PM_ERR_INVALID, "kind must be PM_PLAN_BASE .. PM_PLAN_PADDED16");
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    static_assert(offsetof(pm::LaunchPlan, unroll) == 11 * sizeof(int32_t), "the query copies the twelve reported members in their order");
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    const int rc = validate_request(op, op ? op->weight_dtype : -1, knobs, &shape);
    if (rc != PM_OK) return rc;
    constexpr PlanKind kinds[] = {PlanKind::base, PlanKind::forward, PlanKind::quantized, PlanKind::padded, PlanKind::padded16};
    const pm::LaunchPlan p = plan_of(*op, shape, knobs, kinds[kind]);
    const int32_t v[12] = {p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
                           p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return PM_OK;
}

int pm_embedding_gather_plan(const pm_embbag_batch* op, int64_t out[8]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = validate_request(op, op ? op->weight_dtype : -1, knobs);
    if (rc != PM_OK) return rc;
    const pm::GatherPlan g = pm::plan_gather(*op, op->weight_dtype, knobs);
    const int64_t v[8] = {g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous, g.grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return PM_OK;
}

int pm_set_backward_tuning(int32_t sort_impl, int32_t order, int32_t xcd_affine, int32_t max_phases) {
    if (sort_impl < -1 || sort_impl > 2 || order < -1 || order > 1 || xcd_affine < -1 || xcd_affine > 1)
        return fail(PM_ERR_INVALID, "sort_impl must be -1 .. 2, order / xcd_affine -1, 0 or 1");
#ifndef PM_ALTERNATES
    if (sort_impl > 0)
        return fail(PM_ERR_UNSUPPORTED, "sort_impl 1 (rocPRIM) and 2 (round 2's LSD sort) exist in the alternates build only "
                                        "(libparam_amd_alt.so: make -C param_amd/csrc alt)");
#endif
    if (max_phases != -1 && max_phases != 1 && max_phases != 2) return fail(PM_ERR_INVALID, "max_phases must be -1, 1 or 2");
    pm::set_backward_tuning(sort_impl, order, xcd_affine, max_phases);
    return PM_OK;
}

int pm_set_sort_tuning(int32_t mode) {
    if (mode < -1 || mode > 3) return fail(PM_ERR_INVALID, "mode must be -1, 0, 1, 2 or 3");
    pm::set_sort_tuning(mode);
    return PM_OK;
}

int pm_set_hybrid_tuning(int32_t enable, int64_t lookback_spin_cap) {
    if (enable < -1 || enable > 2) return fail(PM_ERR_INVALID, "enable must be -1 .. 2");
    if (lookback_spin_cap < 0 || lookback_spin_cap > 0xffffffffLL) return fail(PM_ERR_INVALID, "lookback_spin_cap must be in [0, 2^32)");
    pm::set_hybrid_tuning(enable, static_cast<uint32_t>(lookback_spin_cap));
    return PM_OK;
}

int pm_set_hybrid_rest(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(PM_ERR_INVALID, "mode must be -1 (default), 0 or 1");
    pm::set_hybrid_rest(mode);
    return PM_OK;
}

int pm_set_hybrid_min_tiles(int32_t tiles) {
    if (tiles < -1) return fail(PM_ERR_INVALID, "tiles must be -1 (default) or >= 0");
    pm::set_hybrid_min_tiles(tiles);
    return PM_OK;
}

int pm_embbag_sort_status(const pm_embbag_batch* op, int64_t max_rows, const void* workspace, pm_sort_status* out, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if (max_rows < 1 || max_rows > (1LL << 31)) return fail(PM_ERR_INVALID, "max_rows must be in [1, 2^31]");
    if (!workspace || !out) return fail(PM_ERR_INVALID, "NULL argument");
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};
    const hipError_t h = pm::sort_status(p, max_rows, op->max_dim, workspace, static_cast<hipStream_t>(stream), v);
    if (h == hipErrorInvalidValue) return fail(PM_ERR_INVALID, kNoSortRecorded);
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_sort_status");
    out->lookback_fallbacks = v[0];
    out->pairs_sorted = v[1];
    out->hybrid_tables = v[2];
    out->hybrid_launched = v[3];
    out->lds_pairs = v[4];
    out->lds_tables = v[5];
    return PM_OK;
}

#ifdef PM_ALTERNATES
int64_t pm_radix_sort_scratch_bytes(int64_t n_max) {
    if (n_max < 0 || n_max > 0xffffffffLL) return fail(PM_ERR_INVALID, "n_max must be in [0, 2^32)");
    return static_cast<int64_t>(pm::rs_scratch_bytes(static_cast<size_t>(n_max)));
}

int pm_radix_sort_pairs(void* keys_a, void* keys_b, uint32_t* vals_a, uint32_t* vals_b, int64_t n_max,
                        const uint32_t* d_count, int32_t key_bytes, int32_t begin_bit, int32_t end_bit, int64_t segment_len,
                        void* scratch, int64_t scratch_bytes, int32_t* result_in_b, pm_stream_t stream) {
    if (n_max < 0 || n_max > 0xffffffffLL) return fail(PM_ERR_INVALID, "n_max must be in [0, 2^32)");
    if (key_bytes != 4 && key_bytes != 8) return fail(PM_ERR_INVALID, "key_bytes must be 4 or 8");
    if (begin_bit < 0 || end_bit < begin_bit || end_bit > key_bytes * 8) return fail(PM_ERR_INVALID, "bad bit range");
    if (!result_in_b) return fail(PM_ERR_INVALID, "result_in_b is NULL");
    if (segment_len < 0 || (segment_len > 0 && (segment_len % 4096 != 0 || n_max % segment_len != 0 || d_count)))
        return fail(PM_ERR_INVALID, "segment_len must be 0 or a multiple of 4096 dividing n_max (and d_count NULL)");
    *result_in_b = pm::rs_num_passes(begin_bit, end_bit) % 2;
    if (n_max == 0) return PM_OK;
    if (!keys_a || !keys_b || !vals_a || !vals_b) return fail(PM_ERR_INVALID, "key / value buffers are NULL");
    if (!scratch || scratch_bytes < static_cast<int64_t>(pm::rs_scratch_bytes(static_cast<size_t>(n_max))))
        return fail(PM_ERR_INVALID, "scratch too small: need " + std::to_string(pm::rs_scratch_bytes(static_cast<size_t>(n_max))) + " bytes");
    hipError_t h = key_bytes == 4
        ? pm::rs_sort_pairs<uint32_t>(static_cast<uint32_t*>(keys_a), static_cast<uint32_t*>(keys_b), vals_a, vals_b,
                                      static_cast<size_t>(n_max), d_count, begin_bit, end_bit, scratch, static_cast<hipStream_t>(stream),
                                      static_cast<size_t>(segment_len))
        : pm::rs_sort_pairs<uint64_t>(static_cast<uint64_t*>(keys_a), static_cast<uint64_t*>(keys_b), vals_a, vals_b,
                                      static_cast<size_t>(n_max), d_count, begin_bit, end_bit, scratch, static_cast<hipStream_t>(stream),
                                      static_cast<size_t>(segment_len));
    if (h != hipSuccess) return hip_fail(h, "pm_radix_sort_pairs");
    return PM_OK;
}
#endif

static int rowquant_args_ok(int64_t n_rows, int32_t dim, int32_t bitwidth) {
    if (n_rows < 0) return fail(PM_ERR_INVALID, "n_rows is negative");
    if (bitwidth != 16 && bitwidth != 8 && bitwidth != 4 && bitwidth != 2) return fail(PM_ERR_INVALID, "bitwidth must be 16, 8, 4 or 2");
    if (dim < 8 || dim % 8 != 0 || dim > 512) return fail(PM_ERR_UNSUPPORTED, "dim must be a multiple of 8 in [8, 512]");
    return PM_OK;
}

static uintptr_t rowquant_align(int32_t bitwidth) { return bitwidth == 16 ? 16 : static_cast<uintptr_t>(bitwidth); }

int64_t pm_rows_quantized_bytes(int64_t n_rows, int32_t dim, int32_t bitwidth) {
    const int rc = rowquant_args_ok(n_rows, dim, bitwidth);
    if (rc != PM_OK) return rc;
    return n_rows * pm::rows_quantized_row_bytes(dim, bitwidth);
}

int pm_rows_quantize(const float* src, int64_t n_rows, int32_t dim, int32_t bitwidth, void* dst, pm_stream_t stream) {
    const int rc = rowquant_args_ok(n_rows, dim, bitwidth);
    if (rc != PM_OK) return rc;
    if (n_rows == 0) return PM_OK;
    if (!src || !dst) return fail(PM_ERR_INVALID, "src / dst is NULL");
    if (reinterpret_cast<uintptr_t>(src) % 16 != 0 || reinterpret_cast<uintptr_t>(dst) % rowquant_align(bitwidth) != 0)
        return fail(PM_ERR_INVALID, "src must be 16-byte aligned, dst aligned to the format's word (16 / 8 / 4 / 2 bytes for 16 / 8 / 4 / 2 bits)");
    const hipError_t h = pm::launch_rows_quantize(src, n_rows, dim, bitwidth, dst, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_rows_quantize launch");
    return PM_OK;
}

int pm_rows_dequantize(const void* src, int64_t n_rows, int32_t dim, int32_t bitwidth, float* dst, pm_stream_t stream) {
    const int rc = rowquant_args_ok(n_rows, dim, bitwidth);
    if (rc != PM_OK) return rc;
    if (n_rows == 0) return PM_OK;
    if (!src || !dst) return fail(PM_ERR_INVALID, "src / dst is NULL");
    if (reinterpret_cast<uintptr_t>(dst) % 16 != 0 || reinterpret_cast<uintptr_t>(src) % rowquant_align(bitwidth) != 0)
        return fail(PM_ERR_INVALID, "dst must be 16-byte aligned, src aligned to the format's word (16 / 8 / 4 / 2 bytes for 16 / 8 / 4 / 2 bits)");
    const hipError_t h = pm::launch_rows_dequantize(src, n_rows, dim, bitwidth, dst, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_rows_dequantize launch");
    return PM_OK;
}

int pm_embbag_fwd(const pm_embbag_batch* op, float* out, pm_stream_t stream) {
    pm::KParams p;
    int unroll = 0;
    int rc = make_params(op, op ? op->weight_dtype : -1, p, PlanKind::forward, &unroll);
    if (rc != PM_OK) return rc;
    if (p.bag_count == 0) return PM_OK;
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    p.io = out;
    const hipError_t h = pm::launch_embbag_fwd(p, op->weight_dtype, op->max_dim, unroll, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_fwd launch");
    return PM_OK;
}

// ---- padding (embbag_fwd_pad.hip, pad_rows.hip) --------------------------------------------------------------------------
int pm_embbag_fwd_padded(const pm_embbag_batch* op, const int64_t* padding_idx, float* out, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p, PlanKind::padded);
    if (rc != PM_OK) return rc;
    if (!padding_idx) return fail(PM_ERR_INVALID, "padding_idx is NULL (device int64 [num_tables], -1 = no padding row: pm_embbag_fwd takes requests without one)");
    return padded_forward(p, out, 0, stream, [&](const pm::KParams& q, hipStream_t s) {
        return pm::launch_embbag_fwd_padded(q, op->weight_dtype, op->max_dim, padding_idx, s);
    }, "pm_embbag_fwd_padded launch");
}

int pm_embbag_pad_mask(const pm_embbag_batch* op, const int64_t* padding_idx, float* values, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if (!padding_idx) return fail(PM_ERR_INVALID, "padding_idx is NULL");
    if (!values && op->num_indices > 0) return fail(PM_ERR_INVALID, "values is NULL");
    if (p.bag_count == 0 || p.N == 0) return PM_OK;
    const hipError_t h = pm::launch_pad_mask(p, padding_idx, values, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_pad_mask launch");
    return PM_OK;
}

// ---- mean pooling (embbag_fwd_pad.hip with MEAN = true, mean_pool.hip) --------------------------------------------------
// What the mean, 16-bit output and 16-bit gradient calls refuse on the host, behind make_params.  Blocked layouts: the padded family's
// tiling and the scaling / widening kernels address bag b at out_offsets[t] + b * out_stride.
struct Subject { const char* noun; const char* verb; };   // who refuses, in the error text: "<noun> <verb> not take ..."
constexpr Subject kMeanPooling{"mean pooling", "does"}, kOutput16{"16-bit output", "does"}, kGradients16{"16-bit gradients", "do"};
static int blocked_refused(const pm_embbag_batch* op, const Subject& who) {
    if (op->grad_block_shift != 0 || op->table_group != 0)
        return fail(PM_ERR_UNSUPPORTED, std::string(who.noun) + " " + who.verb + " not take blocked layouts (grad_block_shift / table_group must be 0)");
    return PM_OK;
}
static int weighted_mean_refused(const pm_embbag_batch* op) {
    if (op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "mean pooling is unweighted: per_sample_weights must be NULL");
    return PM_OK;
}

int pm_embbag_fwd_mean(const pm_embbag_batch* op, const int64_t* padding_idx, float* out, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p, PlanKind::padded);
    if (rc != PM_OK) return rc;
    if ((rc = blocked_refused(op, kMeanPooling)) != PM_OK || (rc = weighted_mean_refused(op)) != PM_OK) return rc;
    return padded_forward(p, out, 0, stream, [&](const pm::KParams& q, hipStream_t s) {
        return pm::launch_embbag_fwd_mean(q, op->weight_dtype, op->max_dim, padding_idx, s);
    }, "pm_embbag_fwd_mean launch");
}

int pm_embbag_mean_grad(const pm_embbag_batch* op, const int64_t* padding_idx, const float* grad, float* scaled, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if ((rc = blocked_refused(op, kMeanPooling)) != PM_OK) return rc;
    if (p.bag_count == 0) return PM_OK;
    if (!grad || !scaled) return fail(PM_ERR_INVALID, "grad / scaled is NULL");
    if (reinterpret_cast<uintptr_t>(grad) % 16 != 0 || reinterpret_cast<uintptr_t>(scaled) % 16 != 0)
        return fail(PM_ERR_INVALID, "grad and scaled must be 16-byte aligned");
    const hipError_t h = pm::launch_mean_grad(p, op->max_dim, padding_idx, grad, scaled, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_mean_grad launch");
    return PM_OK;
}

// ---- 16-bit output and gradients (embbag_fwd_out16_*.hip, grad_widen.hip) -------------------------------------------------------
// what pm_embbag_fwd_out16 and pm_embbag_grad_widen refuse of their own; what: the dtype argument's name, who: as blocked_refused's
static int out16_args_ok(const pm_embbag_batch* op, int32_t dtype, const char* what, const char* fp32_hint, int32_t mean, const Subject& who) {
    if (dtype != PM_BF16 && dtype != PM_F16) return fail(PM_ERR_INVALID, std::string(what) + " must be PM_BF16 or PM_F16 (" + fp32_hint + ")");
    if (mean != 0 && mean != 1) return fail(PM_ERR_INVALID, "mean must be 0 or 1");
    const int rc = blocked_refused(op, who);
    return rc != PM_OK || !mean ? rc : weighted_mean_refused(op);
}

int pm_embbag_fwd_out16(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t out_dtype, void* out, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p, PlanKind::padded16);
    if (rc != PM_OK) return rc;
    if ((rc = out16_args_ok(op, out_dtype, "out_dtype", "fp32 output is written by pm_embbag_fwd, pm_embbag_fwd_padded and pm_embbag_fwd_mean", mean,
                            kOutput16)) != PM_OK)
        return rc;
    const auto launch = op->weight_dtype == PM_F32 ? pm::launch_embbag_fwd_out16_f32
                        : op->weight_dtype == PM_BF16 ? pm::launch_embbag_fwd_out16_bf16 : pm::launch_embbag_fwd_out16_f16;
    return padded_forward(p, out, 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return launch(q, op->max_dim, padding_idx, mean != 0, out_dtype, s);
    }, "pm_embbag_fwd_out16 launch");
}

int pm_embbag_grad_widen(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t grad_dtype, const void* grad16,
                         float* grad32, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if ((rc = out16_args_ok(op, grad_dtype, "grad_dtype", "an fp32 gradient goes to the backward entry points as it is, or through pm_embbag_mean_grad",
                            mean, kGradients16)) != PM_OK)
        return rc;
    if (p.bag_count == 0) return PM_OK;
    if (!grad16 || !grad32) return fail(PM_ERR_INVALID, "grad16 / grad32 is NULL");
    if (reinterpret_cast<uintptr_t>(grad16) % 8 != 0 || reinterpret_cast<uintptr_t>(grad32) % 16 != 0)
        return fail(PM_ERR_INVALID, "grad16 must be 8-byte aligned and grad32 16-byte aligned");
    if (grad16 == static_cast<const void*>(grad32)) return fail(PM_ERR_INVALID, "grad32 must not be grad16 (the widening is not in place)");
    const hipError_t h = pm::launch_grad_widen(p, op->max_dim, padding_idx, mean != 0, grad_dtype, grad16, grad32, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_grad_widen launch");
    return PM_OK;
}

// ---- max pooling (embbag_fwd_max.hip, embbag_max_grad.hip) -----------------------------------------------------------------------
constexpr Subject kMaxPooling{"max pooling", "does"};
// what the two max calls refuse of their own, behind make_params; what: the dtype argument's name
static int max_args_ok(const pm_embbag_batch* op, int32_t dtype, const char* what) {
    int rc = blocked_refused(op, kMaxPooling);
    if (rc != PM_OK) return rc;
    if (op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "max pooling is unweighted: per_sample_weights must be NULL");
    if (dtype != PM_F32 && dtype != PM_BF16 && dtype != PM_F16) return fail(PM_ERR_INVALID, std::string(what) + " must be PM_F32, PM_BF16 or PM_F16");
    return PM_OK;
}

int pm_embbag_fwd_max(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t out_dtype, void* out, int32_t* max_indices,
                      pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p, out_dtype == PM_F32 ? PlanKind::padded : PlanKind::padded16);
    if (rc != PM_OK) return rc;
    if ((rc = max_args_ok(op, out_dtype, "out_dtype")) != PM_OK) return rc;
    if (reinterpret_cast<uintptr_t>(max_indices) % 16 != 0) return fail(PM_ERR_INVALID, "max_indices must be 16-byte aligned");
    return padded_forward(p, out, out_dtype == PM_F32 ? 16 : 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return pm::launch_embbag_fwd_max(q, op->weight_dtype, op->max_dim, padding_idx, out_dtype, max_indices, s);
    }, "pm_embbag_fwd_max launch");
}

int pm_embbag_max_grad(const pm_embbag_batch* op, const void* grad, int32_t grad_dtype, const int32_t* max_indices, float* g_seq,
                       int64_t g_seq_row_stride, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if ((rc = max_args_ok(op, grad_dtype, "grad_dtype")) != PM_OK) return rc;
    if (op->min_dim != 0 && op->min_dim != op->max_dim)
        return fail(PM_ERR_UNSUPPORTED, "the max gradient needs one common embedding dim (min_dim == max_dim): the sequence backward that "
                                        "applies g_seq takes one");
    if (g_seq_row_stride < op->max_dim || g_seq_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "g_seq_row_stride must be a multiple of 4 elements and at least max_dim");
    if (p.bag_count == 0 || p.N == 0) return PM_OK;
    if (!grad || !max_indices || !g_seq) return fail(PM_ERR_INVALID, "grad / max_indices / g_seq is NULL");
    if (reinterpret_cast<uintptr_t>(grad) % (grad_dtype == PM_F32 ? 16 : 8) != 0 || reinterpret_cast<uintptr_t>(max_indices) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(g_seq) % 16 != 0)
        return fail(PM_ERR_INVALID, "grad must be 16-byte aligned (8-byte for a 16-bit grad_dtype), max_indices and g_seq 16-byte aligned");
    const hipError_t h = pm::launch_max_grad(p, op->max_dim, grad, grad_dtype, max_indices, g_seq, g_seq_row_stride, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_max_grad launch");
    return PM_OK;
}

// ---- row-quantised tables (embbag_fwd_qrows.hip) ---------------------------------------------------------------------------------------
// what the lookup and its plan query refuse on the host, in one order: the request for the element type whose columns per lane the
// format has (qrows_elem_dtype: the column rules D % 4 / D % 8), then the call's own arguments.  out_bytes: of one output element.
static int qrows_request(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, const pm::PlanKnobs& knobs, pm::PlanShape& shape, int& out_bytes) {
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    if (bits == 2 || bits == 16)
        return fail(PM_ERR_UNSUPPORTED, "bits must be 8 or 4: " + std::to_string(bits) + "-bit rows are a payload format of pm_rows_quantize / "
                                        "pm_embbag_fwd_quantized only, no table can be pooled from them");
    if (bits != 8 && bits != 4) return fail(PM_ERR_INVALID, "bits must be 8 or 4");
    const int rc = validate_request(op, pm::qrows_elem_dtype(bits), knobs);
    if (rc != PM_OK) return rc;
    shape = pm::qrows_shape(*op, bits, knobs);      // (lane groups at least as wide in columns as that element type's: no more tiles than validated)
    if (!dtype_is_weight(out_dtype)) return fail(PM_ERR_INVALID, "out_dtype must be PM_F32, PM_BF16 or PM_F16");
    if (op->table_group != 0 || op->grad_block_shift != 0 || op->grad_block_extra != 0)
        return fail(PM_ERR_UNSUPPORTED, "row-quantised tables do not take blocked layouts (table_group / grad_block_shift / grad_block_extra must be 0)");
    if (op->max_dim > pm::kQrowsMaxDim)
        return fail(PM_ERR_UNSUPPORTED, "row-quantised tables: dims[t] (and max_dim) must be at most " + std::to_string(pm::kQrowsMaxDim));
    out_bytes = out_dtype == PM_F32 ? 4 : 2;
    return PM_OK;
}

int pm_embbag_fwd_qrows(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, void* out, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    int out_bytes = 0;
    const int rc = qrows_request(op, bits, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan plan = pm::plan_qrows(*op, shape, knobs, out_bytes);
    pm::KParams p;
    fill_params(op, plan, p);
    return padded_forward(p, out, out_dtype == PM_F32 ? 16 : 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return pm::launch_embbag_fwd_qrows(q, bits, out_dtype, op->max_dim, plan.unroll, s);
    }, "pm_embbag_fwd_qrows launch");
}

int pm_embbag_qrows_plan(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, int32_t out[12]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    int out_bytes = 0;
    const int rc = qrows_request(op, bits, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan p = pm::plan_qrows(*op, shape, knobs, out_bytes);
    const int32_t v[12] = {p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
                           p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return PM_OK;
}

// ---- un-pooled rows (embedding_gather.hip) ---------------------------------------------------------------------------------------------
int pm_embedding_gather(const pm_embbag_batch* op, int32_t out_dtype, void* out, int64_t out_row_stride, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);      // (what pm_embbag_fwd refuses; the base plan's geometry is not used)
    if (rc != PM_OK) return rc;
    if (!dtype_is_weight(out_dtype)) return fail(PM_ERR_INVALID, "out_dtype must be PM_F32, PM_BF16 or PM_F16");
    if (op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "un-pooled rows are unweighted: per_sample_weights must be NULL");
    if (op->table_group != 0 || op->grad_block_shift != 0 || op->grad_block_extra != 0)
        return fail(PM_ERR_UNSUPPORTED, "un-pooled rows do not take blocked layouts (table_group / grad_block_shift / grad_block_extra must be 0)");
    if (out_row_stride < op->max_dim || out_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "out_row_stride must be a multiple of 4 elements and at least max_dim");
    if (!out && op->num_indices > 0) return fail(PM_ERR_INVALID, "out is NULL");
    const uintptr_t align = out_dtype == PM_F32 ? 16 : 8;
    if (reinterpret_cast<uintptr_t>(out) % align != 0) return fail(PM_ERR_INVALID, "out must be " + std::to_string(align) + "-byte aligned");
    if (op->num_indices == 0 || op->bag_count == 0) return PM_OK;
    const pm::GatherPlan g = pm::plan_gather(*op, op->weight_dtype, current_knobs());
    if (g.grid > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    p.io = static_cast<float*>(out);           // (addressed in out_dtype's elements)
    p.out_stride = out_row_stride;
    const hipError_t h = pm::launch_embedding_gather(p, op->weight_dtype, out_dtype, g, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embedding_gather launch");
    return PM_OK;
}

// ---- un-pooled rows of row-quantised tables (embedding_gather_qrows.hip) -----------------------------------------------------------------
// what the lookup and its plan query refuse about the request, in one order: what pm_embbag_fwd_qrows refuses (qrows_request), then
// what pm_embedding_gather refuses about a request
static int qgather_request(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, const pm::PlanKnobs& knobs) {
    pm::PlanShape shape;
    int out_bytes = 0;
    const int rc = qrows_request(op, bits, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    if (op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "un-pooled rows are unweighted: per_sample_weights must be NULL");
    return PM_OK;
}

int pm_embedding_gather_qrows(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, void* out, int64_t out_row_stride, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = qgather_request(op, bits, out_dtype, knobs);
    if (rc != PM_OK) return rc;
    if (out_row_stride < op->max_dim || out_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "out_row_stride must be a multiple of 4 elements and at least max_dim");
    if (op->num_indices == 0 || op->bag_count == 0) return PM_OK;      // nothing to write, whatever `out` is
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const uintptr_t align = out_dtype == PM_F32 ? 16 : 8;
    if (reinterpret_cast<uintptr_t>(out) % align != 0) return fail(PM_ERR_INVALID, "out must be " + std::to_string(align) + "-byte aligned");
    const pm::GatherPlan g = pm::plan_gather_qrows(*op, bits, knobs);
    if (g.grid > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, pm::LaunchPlan{}, p);      // (the request; a gather has no bag tiling)
    p.io = static_cast<float*>(out);           // (addressed in out_dtype's elements)
    p.out_stride = out_row_stride;
    const hipError_t h = pm::launch_embedding_gather_qrows(p, bits, out_dtype, g, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embedding_gather_qrows launch");
    return PM_OK;
}

int pm_embedding_gather_qrows_plan(const pm_embbag_batch* op, int32_t bits, int64_t out[8]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = qgather_request(op, bits, PM_F32, knobs);
    if (rc != PM_OK) return rc;
    const pm::GatherPlan g = pm::plan_gather_qrows(*op, bits, knobs);
    const int64_t v[8] = {g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous, g.grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return PM_OK;
}

// ---- FP8 tables (embbag_fwd_f8_kernel.inc, embedding_gather_f8.hip) -----------------------------------------------------------------------
// what the four calls refuse about a request, in one order: op and its weight_dtype, then what every entry point refuses (for the 16-bit
// element, whose column rule D % 8 the FP8 rule D % 16 contains and whose lane groups are no narrower: no more tiles than validated),
// then the FP8 column rules, blocked layouts and out_dtype.  gather: the un-pooled calls, which are unweighted.
static int f8_request(const pm_embbag_batch* op, int32_t out_dtype, bool gather, const pm::PlanKnobs& knobs) {
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    if (op->weight_dtype != PM_F8E4M3 && op->weight_dtype != PM_F8E5M2)
        return fail(PM_ERR_INVALID, "weight_dtype must be PM_F8E4M3 or PM_F8E5M2 (other tables: pm_embbag_fwd and its family)");
    const int rc = validate_request(op, PM_BF16, knobs);
    if (rc != PM_OK) return rc;
    if (op->max_dim % pm::kF8LaneColumns != 0 || op->min_dim % pm::kF8LaneColumns != 0)
        return fail(PM_ERR_UNSUPPORTED, "FP8 tables: every dims[t] (max_dim, and min_dim where given) must be a multiple of 16");
    if (op->max_dim > pm::kF8MaxDim) return fail(PM_ERR_UNSUPPORTED, "FP8 tables: dims[t] (and max_dim) must be at most " + std::to_string(pm::kF8MaxDim));
    if (op->table_group != 0 || op->grad_block_shift != 0 || op->grad_block_extra != 0)
        return fail(PM_ERR_UNSUPPORTED, "FP8 tables do not take blocked layouts (table_group / grad_block_shift / grad_block_extra must be 0)");
    if (!dtype_is_weight(out_dtype)) return fail(PM_ERR_INVALID, "out_dtype must be PM_F32, PM_BF16 or PM_F16");
    if (gather && op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "un-pooled rows are unweighted: per_sample_weights must be NULL");
    return PM_OK;
}

int pm_embbag_fwd_f8(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t out_dtype, void* out, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    int rc = f8_request(op, out_dtype, false, knobs);
    if (rc != PM_OK) return rc;
    if (mean != 0 && mean != 1) return fail(PM_ERR_INVALID, "mean must be 0 or 1");
    if (mean && (rc = weighted_mean_refused(op)) != PM_OK) return rc;
    const pm::LaunchPlan plan = pm::plan_f8(*op, knobs, out_dtype == PM_F32 ? 4 : 2);
    if (pm::ceil_div(op->bag_count, plan.bags_per_block) * op->num_tables > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, plan, p);
    const auto launch = op->weight_dtype == PM_F8E4M3 ? pm::launch_embbag_fwd_f8_e4m3 : pm::launch_embbag_fwd_f8_e5m2;
    return padded_forward(p, out, out_dtype == PM_F32 ? 16 : 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return launch(q, op->max_dim, plan.unroll, padding_idx, mean != 0, out_dtype, s);
    }, "pm_embbag_fwd_f8 launch");
}

int pm_embbag_f8_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t out[12]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = f8_request(op, out_dtype, false, knobs);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan p = pm::plan_f8(*op, knobs, out_dtype == PM_F32 ? 4 : 2);
    if (pm::ceil_div(op->bag_count, p.bags_per_block) * op->num_tables > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    const int32_t v[12] = {p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
                           p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return PM_OK;
}

int pm_embedding_gather_f8(const pm_embbag_batch* op, int32_t out_dtype, void* out, int64_t out_row_stride, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = f8_request(op, out_dtype, true, knobs);
    if (rc != PM_OK) return rc;
    if (out_row_stride < op->max_dim || out_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "out_row_stride must be a multiple of 4 elements and at least max_dim");
    if (op->num_indices == 0 || op->bag_count == 0) return PM_OK;      // nothing to write, whatever `out` is
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const uintptr_t align = out_dtype == PM_F32 ? 16 : 8;
    if (reinterpret_cast<uintptr_t>(out) % align != 0) return fail(PM_ERR_INVALID, "out must be " + std::to_string(align) + "-byte aligned");
    const pm::GatherPlan g = pm::plan_gather_f8(*op, knobs);
    if (g.grid > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, pm::LaunchPlan{}, p);      // (the request; a gather has no bag tiling)
    p.io = static_cast<float*>(out);           // (addressed in out_dtype's elements)
    p.out_stride = out_row_stride;
    const hipError_t h = pm::launch_embedding_gather_f8(p, op->weight_dtype, out_dtype, g, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embedding_gather_f8 launch");
    return PM_OK;
}

int pm_embedding_gather_f8_plan(const pm_embbag_batch* op, int64_t out[8]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = f8_request(op, PM_F32, true, knobs);
    if (rc != PM_OK) return rc;
    const pm::GatherPlan g = pm::plan_gather_f8(*op, knobs);
    const int64_t v[8] = {g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous, g.grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return PM_OK;
}

// ---- scaled FP8 tables (embbag_fwd_f8s_kernel.inc, embedding_gather_f8s.hip, f8_quantize.hip) ----------------------------------------------
// the lookups: f8_request's refusals, then the exponents -- at least one of the two arrays (none is the unscaled call's request)
static int f8s_request(const pm_embbag_batch* op, int32_t out_dtype, bool gather, const int32_t* table_exp, const int8_t* const* row_exp,
                       const pm::PlanKnobs& knobs) {
    const int rc = f8_request(op, out_dtype, gather, knobs);
    if (rc != PM_OK) return rc;
    if (!table_exp && !row_exp)
        return fail(PM_ERR_INVALID, "table_exp and row_exp are both NULL: an unscaled table is pm_embbag_fwd_f8's / pm_embedding_gather_f8's");
    return PM_OK;
}

// the pooled plan: plan_f8's, with the burst dropped where the row exponents' LDS bytes push the tile past 64 KiB (f8s_stage_out)
static pm::LaunchPlan f8s_plan(const pm_embbag_batch* op, int32_t out_dtype, bool mean, bool row, const pm::PlanKnobs& knobs) {
    const int out_bytes = out_dtype == PM_F32 ? 4 : 2;
    pm::LaunchPlan plan = pm::plan_f8(*op, knobs, out_bytes);
    plan.stage_out = pm::f8s_stage_out(plan.bags_per_block, plan.idx_cap, op->per_sample_weights && !mean, row, plan.stage_out, out_bytes);
    return plan;
}

int pm_embbag_fwd_f8_scaled(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t out_dtype, const int32_t* table_exp,
                            const int8_t* const* row_exp, void* out, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    int rc = f8s_request(op, out_dtype, false, table_exp, row_exp, knobs);
    if (rc != PM_OK) return rc;
    if (mean != 0 && mean != 1) return fail(PM_ERR_INVALID, "mean must be 0 or 1");
    if (mean && (rc = weighted_mean_refused(op)) != PM_OK) return rc;
    const pm::LaunchPlan plan = f8s_plan(op, out_dtype, mean != 0, row_exp != nullptr, knobs);
    if (pm::ceil_div(op->bag_count, plan.bags_per_block) * op->num_tables > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, plan, p);
    const bool e4m3 = op->weight_dtype == PM_F8E4M3;
    const auto launch = row_exp ? (e4m3 ? pm::launch_embbag_fwd_f8s_e4m3_row : pm::launch_embbag_fwd_f8s_e5m2_row)
                                : (e4m3 ? pm::launch_embbag_fwd_f8s_e4m3_table : pm::launch_embbag_fwd_f8s_e5m2_table);
    const pm::F8sArgs args = {padding_idx, table_exp, row_exp};
    return padded_forward(p, out, out_dtype == PM_F32 ? 16 : 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return launch(q, op->max_dim, plan.unroll, args, mean != 0, out_dtype, s);
    }, "pm_embbag_fwd_f8_scaled launch");
}

int pm_embbag_f8_scaled_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t mean, int32_t row_exponents, int32_t out[12]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = f8_request(op, out_dtype, false, knobs);
    if (rc != PM_OK) return rc;
    if ((mean != 0 && mean != 1) || (row_exponents != 0 && row_exponents != 1)) return fail(PM_ERR_INVALID, "mean and row_exponents must be 0 or 1");
    const pm::LaunchPlan p = f8s_plan(op, out_dtype, mean != 0, row_exponents != 0, knobs);
    if (pm::ceil_div(op->bag_count, p.bags_per_block) * op->num_tables > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    const int32_t v[12] = {p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
                           p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return PM_OK;
}

int pm_embedding_gather_f8_scaled(const pm_embbag_batch* op, int32_t out_dtype, const int32_t* table_exp, const int8_t* const* row_exp, void* out,
                                  int64_t out_row_stride, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = f8s_request(op, out_dtype, true, table_exp, row_exp, knobs);
    if (rc != PM_OK) return rc;
    if (out_row_stride < op->max_dim || out_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "out_row_stride must be a multiple of 4 elements and at least max_dim");
    if (op->num_indices == 0 || op->bag_count == 0) return PM_OK;      // nothing to write, whatever `out` is
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const uintptr_t align = out_dtype == PM_F32 ? 16 : 8;
    if (reinterpret_cast<uintptr_t>(out) % align != 0) return fail(PM_ERR_INVALID, "out must be " + std::to_string(align) + "-byte aligned");
    const pm::GatherPlan g = pm::plan_gather_f8(*op, knobs);           // (the unscaled gather's geometry: pm_embedding_gather_f8_plan reports it)
    if (g.grid > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, pm::LaunchPlan{}, p);
    p.io = static_cast<float*>(out);
    p.out_stride = out_row_stride;
    const hipError_t h = pm::launch_embedding_gather_f8s(p, op->weight_dtype, out_dtype, g, table_exp, row_exp, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embedding_gather_f8_scaled launch");
    return PM_OK;
}

// the quantiser's arguments, in one order for both calls (out: row_exp / dst, whose alignment rule is the caller's)
static int f8_quantize_args(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, int64_t src_row_stride, int32_t f8_dtype) {
    if (!dtype_is_weight(src_dtype)) return fail(PM_ERR_INVALID, "src_dtype must be PM_F32, PM_BF16 or PM_F16");
    if (f8_dtype != PM_F8E4M3 && f8_dtype != PM_F8E5M2) return fail(PM_ERR_INVALID, "f8_dtype must be PM_F8E4M3 or PM_F8E5M2");
    if (n_rows < 0) return fail(PM_ERR_INVALID, "n_rows is negative");
    if (dim < 16 || dim % pm::kF8LaneColumns != 0) return fail(PM_ERR_UNSUPPORTED, "FP8 tables: dim must be a multiple of 16");
    if (dim > pm::kF8MaxDim) return fail(PM_ERR_UNSUPPORTED, "FP8 tables: dim must be at most " + std::to_string(pm::kF8MaxDim));
    const int64_t es = src_dtype == PM_F32 ? 4 : 2;
    if (src_row_stride < dim || src_row_stride * es % 16 != 0)
        return fail(PM_ERR_INVALID, "src_row_stride (elements) must be at least dim and a whole number of 16-byte pieces");
    if (n_rows == 0) return PM_OK;
    if (!src) return fail(PM_ERR_INVALID, "src is NULL");
    if (reinterpret_cast<uintptr_t>(src) % 16 != 0) return fail(PM_ERR_INVALID, "src must be 16-byte aligned");
    return PM_OK;
}

int pm_f8_row_exponents(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, int64_t src_row_stride, int32_t f8_dtype, int8_t* row_exp,
                        pm_stream_t stream) {
    const int rc = f8_quantize_args(src, src_dtype, n_rows, dim, src_row_stride, f8_dtype);
    if (rc != PM_OK || n_rows == 0) return rc;
    if (!row_exp) return fail(PM_ERR_INVALID, "row_exp is NULL");
    const hipError_t h = pm::launch_f8_row_exponents(src, src_dtype, n_rows, dim, src_row_stride, f8_dtype, row_exp, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_f8_row_exponents launch");
    return PM_OK;
}

int pm_rows_quantize_f8(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, int64_t src_row_stride, int32_t f8_dtype,
                        const int32_t* table_exp, const int8_t* row_exp, void* dst, pm_stream_t stream) {
    const int rc = f8_quantize_args(src, src_dtype, n_rows, dim, src_row_stride, f8_dtype);
    if (rc != PM_OK || n_rows == 0) return rc;
    if (!dst) return fail(PM_ERR_INVALID, "dst is NULL");
    if (reinterpret_cast<uintptr_t>(dst) % 16 != 0) return fail(PM_ERR_INVALID, "dst must be 16-byte aligned");
    const hipError_t h = pm::launch_rows_quantize_f8(src, src_dtype, n_rows, dim, src_row_stride, f8_dtype, table_exp, row_exp, dst,
                                                     static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_rows_quantize_f8 launch");
    return PM_OK;
}

// ---- row-quantised tables of per-table format (embbag_fwd_qmixed.hip, embedding_gather_qmixed.hip) ---------------------------------------
// what the four calls refuse on the host, in one order: op, table_bits, the eight-column rule (the stricter of the two formats' column
// rules, for every table: a lane holds eight columns whatever the format), then what qrows_request refuses about a request of 4-bit
// tables and the call's out_dtype.  The formats themselves are device data: not read here.
static int qmixed_request(const pm_embbag_batch* op, const int32_t* table_bits, int32_t out_dtype, const pm::PlanKnobs& knobs, pm::PlanShape& shape,
                          int& out_bytes) {
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    if (!table_bits) return fail(PM_ERR_INVALID, "table_bits is NULL (a device array of num_tables ints, each 8 or 4)");
    if (op->max_dim % pm::kQmixedLaneColumns != 0 || op->min_dim % pm::kQmixedLaneColumns != 0)
        return fail(PM_ERR_UNSUPPORTED, "per-table formats: every dims[t] (max_dim and min_dim) must be a multiple of 8");
    const int rc = qrows_request(op, 4, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    shape = pm::qmixed_shape(*op, knobs);          // (lanes of eight columns, as the element type qrows_request validated the grid for)
    return PM_OK;
}

int pm_embbag_fwd_qrows_mixed(const pm_embbag_batch* op, const int32_t* table_bits, int32_t out_dtype, void* out, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    int out_bytes = 0;
    const int rc = qmixed_request(op, table_bits, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan plan = pm::plan_qmixed(*op, shape, knobs, out_bytes);
    pm::KParams p;
    fill_params(op, plan, p);
    return padded_forward(p, out, out_dtype == PM_F32 ? 16 : 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return pm::launch_embbag_fwd_qmixed(q, table_bits, out_dtype, op->max_dim, plan.unroll, s);
    }, "pm_embbag_fwd_qrows_mixed launch");
}

int pm_embbag_qrows_mixed_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t out[12]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    int out_bytes = 0;
    static const int32_t not_read = 0;             // (the plan is a function of the request, out_dtype and the knobs: no formats)
    const int rc = qmixed_request(op, &not_read, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan p = pm::plan_qmixed(*op, shape, knobs, out_bytes);
    const int32_t v[12] = {p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
                           p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return PM_OK;
}

// ... un-pooled: qmixed_request, then what pm_embedding_gather refuses about a request
static int qmixed_gather_request(const pm_embbag_batch* op, const int32_t* table_bits, int32_t out_dtype, const pm::PlanKnobs& knobs) {
    pm::PlanShape shape;
    int out_bytes = 0;
    const int rc = qmixed_request(op, table_bits, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    if (op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "un-pooled rows are unweighted: per_sample_weights must be NULL");
    return PM_OK;
}

int pm_embedding_gather_qrows_mixed(const pm_embbag_batch* op, const int32_t* table_bits, int32_t out_dtype, void* out, int64_t out_row_stride,
                                    pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = qmixed_gather_request(op, table_bits, out_dtype, knobs);
    if (rc != PM_OK) return rc;
    if (out_row_stride < op->max_dim || out_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "out_row_stride must be a multiple of 4 elements and at least max_dim");
    if (op->num_indices == 0 || op->bag_count == 0) return PM_OK;      // nothing to write, whatever `out` is
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const uintptr_t align = out_dtype == PM_F32 ? 16 : 8;
    if (reinterpret_cast<uintptr_t>(out) % align != 0) return fail(PM_ERR_INVALID, "out must be " + std::to_string(align) + "-byte aligned");
    const pm::GatherPlan g = pm::plan_gather_qmixed(*op, knobs);
    if (g.grid > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, pm::LaunchPlan{}, p);      // (the request; a gather has no bag tiling)
    p.io = static_cast<float*>(out);           // (addressed in out_dtype's elements)
    p.out_stride = out_row_stride;
    const hipError_t h = pm::launch_embedding_gather_qmixed(p, table_bits, out_dtype, g, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embedding_gather_qrows_mixed launch");
    return PM_OK;
}

int pm_embedding_gather_qrows_mixed_plan(const pm_embbag_batch* op, int64_t out[8]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    static const int32_t not_read = 0;
    const int rc = qmixed_gather_request(op, &not_read, PM_F32, knobs);
    if (rc != PM_OK) return rc;
    const pm::GatherPlan g = pm::plan_gather_qmixed(*op, knobs);
    const int64_t v[8] = {g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous, g.grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return PM_OK;
}

// ---- mixed-format tables (embbag_fwd_anyfmt_kernel.inc, embedding_gather_anyfmt.hip) ------------------------------------------------------
// what the four calls refuse on the host, in one order: everything the per-table-format calls refuse (op, the eight-column rule, the
// request, out_dtype, blocked layouts), with table_formats in table_bits' place, then this family's width limit.  The formats and
// exponents are device data: not read here.
static int anyfmt_request(const pm_embbag_batch* op, const int32_t* table_formats, int32_t out_dtype, const pm::PlanKnobs& knobs, pm::PlanShape& shape,
                          int& out_bytes) {
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    if (!table_formats)
        return fail(PM_ERR_INVALID, "table_formats is NULL (a device array of num_tables format codes: PM_F32, PM_BF16, PM_F16, PM_F8E4M3, "
                                    "PM_F8E5M2, PM_Q8 or PM_Q4)");
    const int rc = qmixed_request(op, table_formats, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    if (op->max_dim > pm::kAnyfmtMaxDim)
        return fail(PM_ERR_UNSUPPORTED, "mixed-format tables: dims[t] (and max_dim) must be at most " + std::to_string(pm::kAnyfmtMaxDim));
    shape = pm::anyfmt_shape(*op, knobs);
    return PM_OK;
}

int pm_embbag_fwd_anyfmt(const pm_embbag_batch* op, const int32_t* table_formats, const int32_t* table_exp, int32_t out_dtype, void* out,
                         pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    int out_bytes = 0;
    const int rc = anyfmt_request(op, table_formats, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan plan = pm::plan_anyfmt(*op, shape, knobs, out_bytes);
    pm::KParams p;
    fill_params(op, plan, p);
    const auto launch = out_dtype == PM_BF16 ? pm::launch_embbag_fwd_anyfmt_bf16
                                             : (out_dtype == PM_F16 ? pm::launch_embbag_fwd_anyfmt_f16 : pm::launch_embbag_fwd_anyfmt_f32);
    return padded_forward(p, out, out_dtype == PM_F32 ? 16 : 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return launch(q, table_formats, table_exp, op->max_dim, s);
    }, "pm_embbag_fwd_anyfmt launch");
}

int pm_embbag_anyfmt_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t out[12]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    int out_bytes = 0;
    static const int32_t not_read = 0;             // (the plan is a function of the request, out_dtype and the knobs: no formats)
    const int rc = anyfmt_request(op, &not_read, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    const pm::LaunchPlan p = pm::plan_anyfmt(*op, shape, knobs, out_bytes);
    const int32_t v[12] = {p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
                           p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return PM_OK;
}

// ... un-pooled: anyfmt_request, then what pm_embedding_gather refuses about a request
static int anyfmt_gather_request(const pm_embbag_batch* op, const int32_t* table_formats, int32_t out_dtype, const pm::PlanKnobs& knobs) {
    pm::PlanShape shape;
    int out_bytes = 0;
    const int rc = anyfmt_request(op, table_formats, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    if (op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "un-pooled rows are unweighted: per_sample_weights must be NULL");
    return PM_OK;
}

int pm_embedding_gather_anyfmt(const pm_embbag_batch* op, const int32_t* table_formats, const int32_t* table_exp, int32_t out_dtype, void* out,
                               int64_t out_row_stride, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    const int rc = anyfmt_gather_request(op, table_formats, out_dtype, knobs);
    if (rc != PM_OK) return rc;
    if (out_row_stride < op->max_dim || out_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "out_row_stride must be a multiple of 4 elements and at least max_dim");
    if (op->num_indices == 0 || op->bag_count == 0) return PM_OK;      // nothing to write, whatever `out` is
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const uintptr_t align = out_dtype == PM_F32 ? 16 : 8;
    if (reinterpret_cast<uintptr_t>(out) % align != 0) return fail(PM_ERR_INVALID, "out must be " + std::to_string(align) + "-byte aligned");
    const pm::GatherPlan g = pm::plan_gather_anyfmt(*op, knobs);
    if (g.grid > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, pm::LaunchPlan{}, p);      // (the request; a gather has no bag tiling)
    p.io = static_cast<float*>(out);           // (addressed in out_dtype's elements)
    p.out_stride = out_row_stride;
    const hipError_t h = pm::launch_embedding_gather_anyfmt(p, table_formats, table_exp, out_dtype, g, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embedding_gather_anyfmt launch");
    return PM_OK;
}

int pm_embedding_gather_anyfmt_plan(const pm_embbag_batch* op, int64_t out[8]) {
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const pm::PlanKnobs knobs = current_knobs();
    static const int32_t not_read = 0;
    const int rc = anyfmt_gather_request(op, &not_read, PM_F32, knobs);
    if (rc != PM_OK) return rc;
    const pm::GatherPlan g = pm::plan_gather_anyfmt(*op, knobs);
    const int64_t v[8] = {g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous, g.grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return PM_OK;
}

// ---- ... whose rows may be pruned (embbag_fwd_qpruned.hip, embedding_gather_qpruned.hip) -------------------------------------------------
// what the two calls refuse on the host beyond the per-table-format calls' refusals (which come first, in their order): both remap
// arrays are required -- a request without a pruned table goes to the per-table-format calls.  Their contents are device data: not read.
static int qpruned_arrays(const int32_t* remap, const int64_t* remap_offsets) {
    if (!remap_offsets) return fail(PM_ERR_INVALID, "remap_offsets is NULL (a device array of num_tables + 1 int64, non-decreasing)");
    if (!remap)
        return fail(PM_ERR_INVALID, "remap is NULL (a device int32 array, the tables' remaps concatenated; a request without a pruned table goes to "
                                    "pm_embbag_fwd_qrows_mixed / pm_embedding_gather_qrows_mixed)");
    return PM_OK;
}

int pm_embbag_fwd_qrows_pruned(const pm_embbag_batch* op, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets,
                               int32_t out_dtype, void* out, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    pm::PlanShape shape;
    int out_bytes = 0;
    int rc = qmixed_request(op, table_bits, out_dtype, knobs, shape, out_bytes);
    if (rc != PM_OK) return rc;
    if ((rc = qpruned_arrays(remap, remap_offsets)) != PM_OK) return rc;
    const pm::LaunchPlan plan = pm::plan_qmixed(*op, shape, knobs, out_bytes);      // (pm_embbag_qrows_mixed_plan reports it)
    pm::KParams p;
    fill_params(op, plan, p);
    return padded_forward(p, out, out_dtype == PM_F32 ? 16 : 8, stream, [&](const pm::KParams& q, hipStream_t s) {
        return pm::launch_embbag_fwd_qpruned(q, table_bits, remap, remap_offsets, out_dtype, op->max_dim, plan.unroll, s);
    }, "pm_embbag_fwd_qrows_pruned launch");
}

int pm_embedding_gather_qrows_pruned(const pm_embbag_batch* op, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets,
                                     int32_t out_dtype, void* out, int64_t out_row_stride, pm_stream_t stream) {
    const pm::PlanKnobs knobs = current_knobs();
    int rc = qmixed_gather_request(op, table_bits, out_dtype, knobs);
    if (rc != PM_OK) return rc;
    if (out_row_stride < op->max_dim || out_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "out_row_stride must be a multiple of 4 elements and at least max_dim");
    if ((rc = qpruned_arrays(remap, remap_offsets)) != PM_OK) return rc;
    if (op->num_indices == 0 || op->bag_count == 0) return PM_OK;      // nothing to write, whatever `out` is
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    const uintptr_t align = out_dtype == PM_F32 ? 16 : 8;
    if (reinterpret_cast<uintptr_t>(out) % align != 0) return fail(PM_ERR_INVALID, "out must be " + std::to_string(align) + "-byte aligned");
    const pm::GatherPlan g = pm::plan_gather_qmixed(*op, knobs);          // (pm_embedding_gather_qrows_mixed_plan reports it)
    if (g.grid > pm::kMaxGrid) return fail(PM_ERR_UNSUPPORTED, "grid too large");
    pm::KParams p;
    fill_params(op, pm::LaunchPlan{}, p);      // (the request; a gather has no bag tiling)
    p.io = static_cast<float*>(out);           // (addressed in out_dtype's elements)
    p.out_stride = out_row_stride;
    const hipError_t h = pm::launch_embedding_gather_qpruned(p, table_bits, remap, remap_offsets, out_dtype, g, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embedding_gather_qrows_pruned launch");
    return PM_OK;
}

static int pad_guard_layout(int32_t num_tables, int32_t max_dim, int32_t table_dtype, int32_t state_kind, int64_t& row_slot, int64_t& slot) {
    if (num_tables < 1) return fail(PM_ERR_INVALID, "num_tables must be >= 1");
    if (!dtype_is_weight(table_dtype)) return fail(PM_ERR_INVALID, "weight/dst dtype must be PM_F32, PM_BF16 or PM_F16");
    const int vec = (table_dtype == PM_F32) ? 4 : 8;
    if (max_dim < 1 || max_dim % vec != 0)
        return fail(PM_ERR_UNSUPPORTED, "every dims[t] (and max_dim) must be a multiple of " + std::to_string(vec) + " for this element type");
    if (state_kind != PM_PAD_STATE_NONE && state_kind != PM_PAD_STATE_ROW && state_kind != PM_PAD_STATE_ELEM)
        return fail(PM_ERR_INVALID, "state_kind must be PM_PAD_STATE_NONE, PM_PAD_STATE_ROW or PM_PAD_STATE_ELEM");
    row_slot = static_cast<int64_t>(max_dim) * (16 / vec);                      // a multiple of 16 bytes
    slot = row_slot + (state_kind == PM_PAD_STATE_ROW ? 16 : state_kind == PM_PAD_STATE_ELEM ? static_cast<int64_t>(max_dim) * 4 : 0);
    return PM_OK;
}

int64_t pm_pad_rows_guard_bytes(int32_t num_tables, int32_t max_dim, int32_t table_dtype, int32_t state_kind) {
    int64_t row_slot = 0, slot = 0;
    const int rc = pad_guard_layout(num_tables, max_dim, table_dtype, state_kind, row_slot, slot);
    return rc != PM_OK ? rc : slot * num_tables;
}

int pm_pad_rows_guard(int32_t num_tables, int32_t max_dim, void* const* tables, const int32_t* dims, int32_t table_dtype,
                      const int64_t* padding_idx, float* const* state, int32_t state_kind, void* stash, int64_t stash_bytes,
                      int32_t direction, pm_stream_t stream) {
    int64_t row_slot = 0, slot = 0;
    const int rc = pad_guard_layout(num_tables, max_dim, table_dtype, state_kind, row_slot, slot);
    if (rc != PM_OK) return rc;
    if (direction != PM_PAD_SAVE && direction != PM_PAD_RESTORE) return fail(PM_ERR_INVALID, "direction must be PM_PAD_SAVE or PM_PAD_RESTORE");
    if (!tables || !dims || !padding_idx) return fail(PM_ERR_INVALID, "tables / dims / padding_idx is NULL");
    if (state_kind != PM_PAD_STATE_NONE && !state) return fail(PM_ERR_INVALID, "state is NULL");
    if (!stash || stash_bytes < slot * num_tables)
        return fail(PM_ERR_INVALID, "stash is NULL or too small: " + std::to_string(slot * num_tables) + " bytes needed (pm_pad_rows_guard_bytes)");
    if (reinterpret_cast<uintptr_t>(stash) % 16 != 0) return fail(PM_ERR_INVALID, "stash must be 16-byte aligned");
    const hipError_t h = pm::launch_pad_guard(num_tables, tables, dims, table_dtype == PM_F32 ? 4 : 2, padding_idx, state, state_kind, stash,
                                              slot, row_slot, direction == PM_PAD_RESTORE, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_pad_rows_guard launch");
    return PM_OK;
}

int pm_embbag_fwd_quantized(const pm_embbag_batch* op, void* out, int32_t bitwidth, pm_stream_t stream) {
    pm::KParams p;
    int unroll = 0;
    int rc = make_params(op, op ? op->weight_dtype : -1, p, PlanKind::quantized, &unroll);
    if (rc != PM_OK) return rc;
    if ((rc = rowquant_args_ok(0, op->max_dim, bitwidth)) != PM_OK) return rc;
    if (op->out_stride % op->max_dim != 0) return fail(PM_ERR_INVALID, "out_stride must be a whole number of max_dim-element rows");
    if (p.bag_count == 0) return PM_OK;
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    if (reinterpret_cast<uintptr_t>(out) % 16 != 0) return fail(PM_ERR_INVALID, "out must be 16-byte aligned");
    if (!p.stage_out)
        return fail(PM_ERR_UNSUPPORTED, "quantised output needs the staged forward (fixed-pooling requests whose tile fits the staging "
                                        "buffer, staging not disabled): run pm_embbag_fwd and pm_rows_quantize instead");
    p.io = static_cast<float*>(out);
    p.out_bits = bitwidth;
    hipError_t h = pm::launch_embbag_fwd(p, op->weight_dtype, op->max_dim, unroll, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_fwd_quantized launch");
    return PM_OK;
}

int pm_embbag_fwd_split(const pm_embbag_batch* op, float* out, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if (p.bag_count == 0) return PM_OK;
    if (!out) return fail(PM_ERR_INVALID, "out is NULL");
    p.io = out;
    hipError_t h = pm::launch_embbag_fwd_split(p, op->weight_dtype, op->max_dim, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_fwd_split launch");
    return PM_OK;
}

int pm_embbag_psw_grad(const pm_embbag_batch* op, const float* grad, float* out, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);   // (the blocked-gradient rules are make_params' own)
    if (rc != PM_OK) return rc;
    if (!grad) return fail(PM_ERR_INVALID, "grad is NULL");
    if (!out && op->num_indices > 0) return fail(PM_ERR_INVALID, "out is NULL");
    const int vec = op->weight_dtype == PM_F32 ? 4 : 8;
    if (op->max_dim > pm::kWave * vec)
        return fail(PM_ERR_UNSUPPORTED, "pm_embbag_psw_grad: max_dim must be at most " + std::to_string(pm::kWave * vec) +
                                            " for this element type (one 16-byte load per lane of a 64-lane group)");
    if (p.bag_count == 0 || p.N == 0) return PM_OK;
    p.io = const_cast<float*>(grad);
    p.psw = nullptr;                                            // the value does not depend on the weights
    const hipError_t h = pm::launch_embbag_psw_grad(p, op->weight_dtype, op->max_dim, op->min_dim, out, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_psw_grad launch");
    return PM_OK;
}

#ifdef PM_ALTERNATES
int pm_embbag_bwd(const pm_embbag_batch* op, const float* grad, void* const* dst_tables, int32_t dst_dtype,
                  float alpha, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, dst_dtype, p);
    if (rc != PM_OK) return rc;
    if (p.bag_count == 0 || p.N == 0) return PM_OK;
    if (!grad || !dst_tables) return fail(PM_ERR_INVALID, "grad / dst_tables is NULL");
    p.io = const_cast<float*>(grad);
    p.tables = const_cast<const void* const*>(dst_tables);
    p.alpha = alpha;
    hipError_t h = pm::launch_embbag_bwd(p, dst_dtype, op->max_dim, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_bwd launch");
    return PM_OK;
}
#endif

static int64_t workspace_query(const char* who, const pm_embbag_batch* op, int64_t max_rows, bool sparse) {
    pm::KParams p;
    size_t sorted = 0, total = 0;
    int rc = sorted_request(op, op ? op->weight_dtype : -1, max_rows, sparse, p);
    if (rc != PM_OK || (rc = sorted_bytes(who, op, max_rows, sparse, p, sorted, total)) != PM_OK) return rc;
    return static_cast<int64_t>(total);
}

int64_t pm_embbag_bwd_sorted_workspace(const pm_embbag_batch* op, int64_t max_rows) {
    return workspace_query("pm_embbag_bwd_sorted_workspace", op, max_rows, false);
}

int pm_embbag_sort_indices(const pm_embbag_batch* op, int64_t max_rows, void* workspace, int64_t workspace_bytes,
                           pm_stream_t stream) {
    return pm_embbag_sort_indices_ex(op, max_rows, 1, workspace, workspace_bytes, stream);
}

static int sort_request(const pm_embbag_batch* op, int64_t max_rows, int32_t phases, void* workspace, int64_t workspace_bytes,
                        pm_stream_t stream, bool defer_ok) {
    if (phases != 1 && phases != 2) return fail(PM_ERR_INVALID, "phases must be 1 or 2");
    SortedCall c{"pm_embbag_sort_indices", op ? op->weight_dtype : -1, false, ""};
    const pm::KParams& p = c.p;
    const int rc = sorted_call_prologue(c, op, max_rows, workspace, workspace_bytes, [&]() -> int { return p.N == 0 ? kDone : PM_OK; },
                                        [] { return pm::PlanStatus::ok; });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    const hipError_t h = pm::sort_indices(p, max_rows, op->max_dim, op->fixed_pooling, phases, workspace, static_cast<hipStream_t>(stream), defer_ok);
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_sort_indices");
    return PM_OK;
}

int pm_embbag_sort_indices_ex(const pm_embbag_batch* op, int64_t max_rows, int32_t phases, void* workspace,
                              int64_t workspace_bytes, pm_stream_t stream) {
    return sort_request(op, max_rows, phases, workspace, workspace_bytes, stream, false);
}

int pm_embbag_sort_plan(const pm_embbag_batch* op, int64_t max_rows, int32_t phases, char* out, int32_t out_bytes) {
    if (phases != 1 && phases != 2) return fail(PM_ERR_INVALID, "phases must be 1 or 2");
    if (!out || out_bytes < 1) return fail(PM_ERR_INVALID, "out buffer is NULL / empty");
    pm::KParams p;
    int rc = sorted_request(op, op ? op->weight_dtype : -1, max_rows, false, p);
    if (rc != PM_OK) return rc;
    const std::string d = pm::sort_plan_describe(p, max_rows, op->fixed_pooling, phases);
    snprintf(out, static_cast<size_t>(out_bytes), "%s", d.c_str());
    return PM_OK;
}

int pm_embbag_sorted_pairs(const pm_embbag_batch* op, int64_t max_rows, const void* workspace, const void** keys,
                           const uint32_t** vals, const uint32_t** d_count, int32_t* key_bytes, int32_t* tshift) {
    pm::KParams p;
    const int rc = sorted_request(op, op ? op->weight_dtype : -1, max_rows, false, p);
    if (rc != PM_OK) return rc;
    if (!workspace || !keys || !vals || !d_count || !key_bytes || !tshift) return fail(PM_ERR_INVALID, "NULL argument");
    pm::SortedPairsInfo pi;
    if (pm::sorted_pairs_info(p, max_rows, op->max_dim, workspace, pi) != pm::PlanStatus::ok) return fail(PM_ERR_INVALID, kNoSortRecorded);
    if (pi.deferred)
        return fail(PM_ERR_INVALID, "the last sort on this workspace was deferred into its apply (pm_embbag_bwd_fused*, hybrid backward) and no "
                                    "apply has been issued yet: there are no sorted pairs to look at");
    *keys = pi.keys;
    *vals = pi.vals;
    *d_count = pi.d_count;
    *key_bytes = pi.key_bytes;
    *tshift = pi.tshift;
    return PM_OK;
}

int pm_embbag_bwd_sorted(const pm_embbag_batch* op, const float* grad, void* const* dst_tables, int32_t dst_dtype,
                         float alpha, int64_t max_rows, const void* workspace, int64_t workspace_bytes,
                         pm_stream_t stream) {
    SortedCall c{"pm_embbag_bwd_sorted", dst_dtype, false, ""};
    pm::KParams& p = c.p;
    const int rc = sorted_call_prologue(
        c, op, max_rows, workspace, workspace_bytes,
        [&]() -> int {
            if (p.N == 0 || p.bag_count == 0) return kDone;
            return (!grad || !dst_tables) ? fail(PM_ERR_INVALID, "grad / dst_tables is NULL") : PM_OK;
        },
        [&] { return pm::bwd_sorted_plan_check(p, max_rows, workspace, false); });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    apply_params(p, grad, dst_tables, alpha);
    const hipError_t h = pm::bwd_sorted_apply(p, max_rows, dst_dtype, op->max_dim, workspace, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_bwd_sorted launch");
    return PM_OK;
}

// what the Adagrad calls check of their own, in their order (after the options, an empty request is PM_OK: kDone)
static int check_adagrad_args(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype, float* const* state,
                              bool elem, const pm_rowwise_adagrad* opt) {
    if (!opt) return fail(PM_ERR_INVALID, "optimizer options are NULL");
    if (opt->weight_decay_mode != PM_WD_NONE && opt->weight_decay_mode != PM_WD_L2 && opt->weight_decay_mode != PM_WD_DECOUPLE)
        return fail(PM_ERR_INVALID, "weight_decay_mode must be PM_WD_NONE, PM_WD_L2 or PM_WD_DECOUPLE");
    if (op->num_indices == 0 || op->bag_count == 0) return kDone;
    if (!grad || !tables || !state) return fail(PM_ERR_INVALID, elem ? "grad / tables / state is NULL" : "grad / tables / momentum is NULL");
    const int vec = (table_dtype == PM_F32) ? 4 : 8;
    if (op->max_dim > 64 * vec)
        return fail(PM_ERR_UNSUPPORTED, std::string(elem ? "element-wise" : "row-wise") + " Adagrad needs max_dim <= " + std::to_string(64 * vec) +
                                            " for this table dtype");
    return PM_OK;
}

// the Adagrad apply: `elem` = element-wise (state [rows_t, dims_t] per table), else row-wise (one value per row)
static int sorted_adagrad(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype, float* const* momentum,
                          bool elem, const pm_rowwise_adagrad* opt, int64_t max_rows, const void* workspace, int64_t workspace_bytes,
                          pm_stream_t stream) {
    SortedCall c{"pm_embbag_bwd_sorted_adagrad", table_dtype, false, elem ? "element-wise" : "row-wise"};
    pm::KParams& p = c.p;
    const int rc = sorted_call_prologue(c, op, max_rows, workspace, workspace_bytes,
                                        [&] { return check_adagrad_args(op, grad, tables, table_dtype, momentum, elem, opt); },
                                        [&] { return pm::bwd_sorted_plan_check(p, max_rows, workspace, true); });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    apply_params(p, grad, tables, 1.0f);
    const hipError_t h = pm::bwd_sorted_apply(p, max_rows, table_dtype, op->max_dim, workspace, static_cast<hipStream_t>(stream),
                                              pm::ApplyUpdate{opt, momentum, elem});
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_bwd_sorted_adagrad launch");
    return PM_OK;
}

int pm_embbag_bwd_sorted_adagrad_ex(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype,
                                    float* const* momentum, const pm_rowwise_adagrad* opt, int64_t max_rows,
                                    const void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    return sorted_adagrad(op, grad, tables, table_dtype, momentum, false, opt, max_rows, workspace, workspace_bytes, stream);
}

int pm_embbag_bwd_sorted_adagrad_elem(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype,
                                      float* const* state, const pm_rowwise_adagrad* opt, int64_t max_rows,
                                      const void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    return sorted_adagrad(op, grad, tables, table_dtype, state, true, opt, max_rows, workspace, workspace_bytes, stream);
}

int pm_embbag_bwd_sorted_adagrad(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype,
                                 float* const* momentum, float lr, float eps, int64_t max_rows, const void* workspace,
                                 int64_t workspace_bytes, pm_stream_t stream) {
    pm_rowwise_adagrad opt = {lr, eps, 0.0f, PM_WD_NONE, 0, 0, 0};
    return pm_embbag_bwd_sorted_adagrad_ex(op, grad, tables, table_dtype, momentum, &opt, max_rows, workspace,
                                           workspace_bytes, stream);
}

// The fused calls validate what their APPLY half needs before the sort half launches anything (a NULL gradient or a bad
// dtype used to be found after the sort's kernels -- and, on the hybrid path, after a deferred plan -- had been issued).
// (kDone: an empty request.)
static int fused_apply_args_ok(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t dtype) {
    if (op && (op->num_indices == 0 || op->bag_count == 0)) return kDone;
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    if (!dtype_is_weight(dtype)) return fail(PM_ERR_INVALID, "weight/dst dtype must be PM_F32, PM_BF16 or PM_F16");
    if (!grad || !tables) return fail(PM_ERR_INVALID, "grad / dst_tables is NULL");
    return validate_request(op, dtype, current_knobs());      // the apply builds its parameters for the DESTINATION dtype: its row-width rule too
}

int pm_embbag_bwd_fused(const pm_embbag_batch* op, const float* grad, void* const* dst_tables, int32_t dst_dtype, float alpha,
                        int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    int rc = fused_apply_args_ok(op, grad, dst_tables, dst_dtype);
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    if ((rc = sort_request(op, max_rows, 1, workspace, workspace_bytes, stream, true)) != PM_OK) return rc;
    return pm_embbag_bwd_sorted(op, grad, dst_tables, dst_dtype, alpha, max_rows, workspace, workspace_bytes, stream);
}

static int fused_adagrad(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype, float* const* momentum,
                         bool elem, const pm_rowwise_adagrad* opt, int64_t max_rows, void* workspace, int64_t workspace_bytes,
                         pm_stream_t stream) {
    int rc = fused_apply_args_ok(op, grad, tables, table_dtype);
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    if ((rc = check_adagrad_args(op, grad, tables, table_dtype, momentum, elem, opt)) != PM_OK) return rc;      // (before the sort half)
    if ((rc = sort_request(op, max_rows, 1, workspace, workspace_bytes, stream, true)) != PM_OK) return rc;
    return sorted_adagrad(op, grad, tables, table_dtype, momentum, elem, opt, max_rows, workspace, workspace_bytes, stream);
}

int pm_embbag_bwd_fused_adagrad(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype,
                                float* const* momentum, const pm_rowwise_adagrad* opt, int64_t max_rows, void* workspace,
                                int64_t workspace_bytes, pm_stream_t stream) {
    return fused_adagrad(op, grad, tables, table_dtype, momentum, false, opt, max_rows, workspace, workspace_bytes, stream);
}

int pm_embbag_bwd_fused_adagrad_elem(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype,
                                     float* const* state, const pm_rowwise_adagrad* opt, int64_t max_rows, void* workspace,
                                     int64_t workspace_bytes, pm_stream_t stream) {
    return fused_adagrad(op, grad, tables, table_dtype, state, true, opt, max_rows, workspace, workspace_bytes, stream);
}

// ---- sequence (un-pooled) backward: the sorted backward on a sort whose values are lookup positions ------------------------------------
// what the pm_embseq_* calls refuse beyond the pooled calls' rules, before their nothing-to-do early-out; has_grad: the call reads one
static int seq_request_ok(const pm_embbag_batch* op, bool has_grad, const float* grad, int64_t grad_row_stride) {
    if (op->per_sample_weights) return fail(PM_ERR_UNSUPPORTED, "sequence gradients are unweighted: per_sample_weights must be NULL");
    if (op->table_group != 0 || op->grad_block_shift != 0 || op->grad_block_extra != 0)
        return fail(PM_ERR_UNSUPPORTED, "sequence gradients do not take blocked layouts (table_group / grad_block_shift / grad_block_extra must be 0)");
    if (!has_grad) return PM_OK;
    if (grad_row_stride < op->max_dim || grad_row_stride % 4 != 0)
        return fail(PM_ERR_INVALID, "grad_row_stride must be a multiple of 4 elements and at least max_dim");
    if (reinterpret_cast<uintptr_t>(grad) % 16 != 0) return fail(PM_ERR_INVALID, "grad must be 16-byte aligned");
    if (!grad && op->num_indices > 0) return fail(PM_ERR_INVALID, "grad is NULL");
    return PM_OK;
}

// the sequence apply's view of the request: gradient row j at grad + j * grad_row_stride, no per-table offset, no blocking, no weights
static void seq_apply_params(pm::KParams& p, const float* grad, int64_t grad_row_stride, const void* tables, float alpha) {
    apply_params(p, grad, tables, alpha);
    p.out_offsets = nullptr;
    p.out_stride = grad_row_stride;
    p.gblk_extra = 0;
}

int pm_embseq_sort_indices(const pm_embbag_batch* op, int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    SortedCall c{"pm_embseq_sort_indices", op ? op->weight_dtype : -1, false, ""};
    c.sequence = true;
    const pm::KParams& p = c.p;
    const int rc = sorted_call_prologue(
        c, op, max_rows, workspace, workspace_bytes,
        [&]() -> int {
            const int r = seq_request_ok(op, false, nullptr, 0);
            return r != PM_OK ? r : (p.N == 0 || p.bag_count == 0) ? kDone : PM_OK;
        },
        [] { return pm::PlanStatus::ok; });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    const hipError_t h = pm::sort_indices(p, max_rows, op->max_dim, 0, 1, workspace, static_cast<hipStream_t>(stream), false, true);
    if (h != hipSuccess) return hip_fail(h, "pm_embseq_sort_indices");
    return PM_OK;
}

int pm_embseq_bwd_sorted(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* dst_tables, int32_t dst_dtype,
                         float alpha, int64_t max_rows, const void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    SortedCall c{"pm_embseq_bwd_sorted", dst_dtype, false, ""};
    c.sequence = true;
    pm::KParams& p = c.p;
    const int rc = sorted_call_prologue(
        c, op, max_rows, workspace, workspace_bytes,
        [&]() -> int {
            const int r = seq_request_ok(op, true, grad, grad_row_stride);
            if (r != PM_OK) return r;
            if (p.N == 0 || p.bag_count == 0) return kDone;
            return !dst_tables ? fail(PM_ERR_INVALID, "dst_tables is NULL") : PM_OK;
        },
        [&] { return pm::bwd_sorted_plan_check(p, max_rows, workspace, false, true); });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    seq_apply_params(p, grad, grad_row_stride, dst_tables, alpha);
    const hipError_t h = pm::bwd_sorted_apply(p, max_rows, dst_dtype, op->max_dim, workspace, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embseq_bwd_sorted launch");
    return PM_OK;
}

// what the sequence Adagrad calls check of their own, in order (kDone: an empty request, after the options)
static int seq_adagrad_args(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* tables, int32_t table_dtype,
                            float* const* state, int32_t elementwise, const pm_rowwise_adagrad* opt) {
    if (elementwise != 0 && elementwise != 1) return fail(PM_ERR_INVALID, "elementwise must be 0 (row-wise) or 1 (element-wise)");
    const int r = seq_request_ok(op, true, grad, grad_row_stride);
    return r != PM_OK ? r : check_adagrad_args(op, grad, tables, table_dtype, state, elementwise != 0, opt);
}

int pm_embseq_bwd_sorted_adagrad(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* tables,
                                 int32_t table_dtype, float* const* state, const pm_rowwise_adagrad* opt, int32_t elementwise,
                                 int64_t max_rows, const void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    SortedCall c{"pm_embseq_bwd_sorted_adagrad", table_dtype, false, elementwise == 1 ? "element-wise" : "row-wise"};
    c.sequence = true;
    pm::KParams& p = c.p;
    const int rc = sorted_call_prologue(c, op, max_rows, workspace, workspace_bytes,
                                        [&] { return seq_adagrad_args(op, grad, grad_row_stride, tables, table_dtype, state, elementwise, opt); },
                                        [&] { return pm::bwd_sorted_plan_check(p, max_rows, workspace, true, true); });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    seq_apply_params(p, grad, grad_row_stride, tables, 1.0f);
    const hipError_t h = pm::bwd_sorted_apply(p, max_rows, table_dtype, op->max_dim, workspace, static_cast<hipStream_t>(stream),
                                              pm::ApplyUpdate{opt, state, elementwise == 1});
    if (h != hipSuccess) return hip_fail(h, "pm_embseq_bwd_sorted_adagrad launch");
    return PM_OK;
}

// The fused sequence calls, like the pooled ones, validate what their APPLY half needs before the sort half launches anything.
static int seq_fused_args_ok(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* tables, int32_t dtype) {
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    int rc = validate_request(op, dtype, current_knobs());      // (the destination dtype's row-width rule)
    if (rc != PM_OK || (rc = seq_request_ok(op, true, grad, grad_row_stride)) != PM_OK) return rc;
    if (op->num_indices == 0 || op->bag_count == 0) return kDone;
    return !tables ? fail(PM_ERR_INVALID, "dst_tables / tables is NULL") : PM_OK;
}

int pm_embseq_bwd_fused(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* dst_tables, int32_t dst_dtype,
                        float alpha, int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    int rc = seq_fused_args_ok(op, grad, grad_row_stride, dst_tables, dst_dtype);
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    if ((rc = pm_embseq_sort_indices(op, max_rows, workspace, workspace_bytes, stream)) != PM_OK) return rc;
    return pm_embseq_bwd_sorted(op, grad, grad_row_stride, dst_tables, dst_dtype, alpha, max_rows, workspace, workspace_bytes, stream);
}

int pm_embseq_bwd_fused_adagrad(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* tables,
                                int32_t table_dtype, float* const* state, const pm_rowwise_adagrad* opt, int32_t elementwise,
                                int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream) {
    if (!op) return fail(PM_ERR_INVALID, "op is NULL");
    int rc = validate_request(op, table_dtype, current_knobs());
    if (rc != PM_OK) return rc;
    if ((rc = seq_adagrad_args(op, grad, grad_row_stride, tables, table_dtype, state, elementwise, opt)) != PM_OK) return rc == kDone ? PM_OK : rc;
    if ((rc = pm_embseq_sort_indices(op, max_rows, workspace, workspace_bytes, stream)) != PM_OK) return rc;
    return pm_embseq_bwd_sorted_adagrad(op, grad, grad_row_stride, tables, table_dtype, state, opt, elementwise, max_rows, workspace,
                                        workspace_bytes, stream);
}

// ---- ABI v8: coalesced sparse gradient (sparse_grad.hip) ----------------------------------------------------------------
// The workspace is the sorted backward's followed by the relabelling's own few words per sorted position and per tile.
int64_t pm_embbag_sparse_grad_workspace(const pm_embbag_batch* op, int64_t max_rows) {
    return workspace_query("pm_embbag_sparse_grad_workspace", op, max_rows, true);
}

int pm_embbag_sparse_grad_count(const pm_embbag_batch* op, int64_t max_rows, void* workspace, int64_t workspace_bytes,
                                int64_t* unique_counts, pm_stream_t stream) {
    pm::SparsePairs sp;
    SortedCall c{"pm_embbag_sparse_grad_workspace", op ? op->weight_dtype : -1, true, ""};
    const pm::KParams& p = c.p;
    const int rc = sorted_call_prologue(
        c, op, max_rows, workspace, workspace_bytes,
        [&]() -> int {
            if (!unique_counts) return fail(PM_ERR_INVALID, "unique_counts is NULL");
            if (p.N != 0 && p.bag_count != 0) return PM_OK;
            // nothing was sorted: every table is empty
            const hipError_t h = hipMemsetAsync(unique_counts, 0, sizeof(int64_t) * static_cast<size_t>(p.T), static_cast<hipStream_t>(stream));
            return h != hipSuccess ? hip_fail(h, "pm_embbag_sparse_grad_count") : kDone;
        },
        [&] { return pm::sparse_grad_pairs(p, max_rows, op->max_dim, workspace, true, sp); });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    const hipError_t h = pm::sparse_grad_count(sp, p.T, p.N, static_cast<char*>(workspace) + c.sorted, unique_counts,
                                               static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_sparse_grad_count launch");
    return PM_OK;
}

int pm_embbag_sparse_grad(const pm_embbag_batch* op, const float* grad, int64_t max_rows, void* workspace, int64_t workspace_bytes,
                          int64_t* const* row_ids, float* const* values, pm_stream_t stream) {
    pm::SparsePairs sp;
    SortedCall c{"pm_embbag_sparse_grad_workspace", op ? op->weight_dtype : -1, true, ""};
    const pm::KParams& p = c.p;
    int rc = sorted_call_prologue(
        c, op, max_rows, workspace, workspace_bytes,
        [&]() -> int {
            if (p.N == 0 || p.bag_count == 0) return kDone;
            return (!grad || !row_ids || !values) ? fail(PM_ERR_INVALID, "grad / row_ids / values is NULL") : PM_OK;
        },
        [&] { return pm::sparse_grad_pairs(p, max_rows, op->max_dim, workspace, false, sp); });
    if (rc != PM_OK) return rc == kDone ? PM_OK : rc;
    hipError_t h = pm::sparse_grad_rows(sp, p.T, p.N, static_cast<const char*>(workspace) + c.sorted, op->dims, row_ids, values,
                                        static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_sparse_grad launch");
    // the sorted apply, unchanged: fp32 destination, alpha = 1, into the zeroed compact rows (row = slot)
    pm::KParams q;
    if ((rc = make_params(op, PM_F32, q)) != PM_OK) return rc;
    apply_params(q, grad, values, 1.0f);
    h = pm::bwd_sorted_apply(q, max_rows, PM_F32, op->max_dim, workspace, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_sparse_grad apply launch");
    return PM_OK;
}

int pm_dlrm_regroup(const int64_t* lengths, const int64_t* indices, int32_t world_size, int32_t num_tables,
                    int64_t batch, int64_t* out_indices, int64_t* out_offsets, int64_t* scratch, pm_stream_t stream) {
    if (world_size < 1 || num_tables < 1 || batch < 0) return fail(PM_ERR_INVALID, "world_size / num_tables / batch");
    if (static_cast<int64_t>(world_size) * num_tables > 4096) return fail(PM_ERR_UNSUPPORTED, "world_size * num_tables > 4096");
    if (!lengths || !out_offsets || !scratch) return fail(PM_ERR_INVALID, "lengths / out_offsets / scratch is NULL");
    hipError_t h = pm::launch_dlrm_regroup(lengths, indices, world_size, num_tables, batch, out_indices, out_offsets,
                                           scratch, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_dlrm_regroup launch");
    return PM_OK;
}

int pm_embbag_check_ex(const pm_embbag_batch* op, int32_t flags, int32_t* d_error_count, pm_stream_t stream) {
    pm::KParams p;
    int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if (!d_error_count) return fail(PM_ERR_INVALID, "d_error_count is NULL");
    if (flags & ~PM_CHECK_UNIFORM_DIMS) return fail(PM_ERR_INVALID, "unknown check flag");
    hipError_t h = pm::launch_embbag_check(p, d_error_count, op->weight_dtype == PM_F32 ? 4 : 8, op->max_dim, op->fixed_pooling,
                                           (flags & PM_CHECK_UNIFORM_DIMS) ? 1 : 0, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_check launch");
    return PM_OK;
}

int pm_embbag_check(const pm_embbag_batch* op, int32_t* d_error_count, pm_stream_t stream) {
    return pm_embbag_check_ex(op, 0, d_error_count, stream);
}

// what both bounds-check calls refuse beyond make_params: sizes the index type cannot hold, pointers off their element
static int bounds_request(const pm_embbag_batch* op, pm::KParams& p) {
    const int rc = make_params(op, op ? op->weight_dtype : -1, p);
    if (rc != PM_OK) return rc;
    if (op->index_dtype == PM_I32 && op->num_indices > 0x7fffffffLL)
        return fail(PM_ERR_INVALID, "pm_embbag_bounds_check: int32 offsets cannot hold num_indices >= 2^31");
    if (op->batch > 0 && !op->offsets) return fail(PM_ERR_INVALID, "offsets is NULL");
    const uintptr_t es = op->index_dtype == PM_I64 ? 8 : 4;
    if (reinterpret_cast<uintptr_t>(op->indices) % es != 0 || reinterpret_cast<uintptr_t>(op->offsets) % es != 0)
        return fail(PM_ERR_INVALID, "pm_embbag_bounds_check: indices / offsets must be aligned to their element type");
    return PM_OK;
}

int64_t pm_embbag_bounds_check_scratch(const pm_embbag_batch* op) {
    pm::KParams p;
    const int rc = bounds_request(op, p);
    if (rc != PM_OK) return rc;
    return pm::bounds_check_scratch_bytes(static_cast<int64_t>(p.T) * p.B, p.T);
}

int pm_embbag_bounds_check(const pm_embbag_batch* op, int32_t mode, int64_t* d_report, void* d_scratch, int64_t scratch_bytes,
                           pm_stream_t stream) {
    pm::KParams p;
    const int rc = bounds_request(op, p);
    if (rc != PM_OK) return rc;
    const int32_t what = mode & ~PM_BOUNDS_LAST_OFFSET;
    if (what != PM_BOUNDS_FATAL && what != PM_BOUNDS_WARNING && what != PM_BOUNDS_IGNORE)
        return fail(PM_ERR_INVALID, "pm_embbag_bounds_check: unknown mode " + std::to_string(mode) +
                                        " (PM_BOUNDS_FATAL, PM_BOUNDS_WARNING or PM_BOUNDS_IGNORE, optionally | PM_BOUNDS_LAST_OFFSET)");
    if (what == PM_BOUNDS_IGNORE) d_report = nullptr;
    else if (!d_report) return fail(PM_ERR_INVALID, "pm_embbag_bounds_check: d_report is NULL (only PM_BOUNDS_IGNORE goes without a report)");
    if (reinterpret_cast<uintptr_t>(d_report) % 8 != 0) return fail(PM_ERR_INVALID, "pm_embbag_bounds_check: d_report must be 8-byte aligned");
    const int64_t need = pm::bounds_check_scratch_bytes(static_cast<int64_t>(p.T) * p.B, p.T);
    if (need == 0) return PM_OK;                                 // no bags: nothing is repaired, nothing is launched
    if (!d_scratch || scratch_bytes < need)
        return fail(PM_ERR_INVALID, "pm_embbag_bounds_check: scratch is NULL or too small: " + std::to_string(need) +
                                        " bytes needed (pm_embbag_bounds_check_scratch)");
    if (reinterpret_cast<uintptr_t>(d_scratch) % 8 != 0) return fail(PM_ERR_INVALID, "pm_embbag_bounds_check: scratch must be 8-byte aligned");
    const hipError_t h = pm::launch_bounds_check(p, what != PM_BOUNDS_FATAL, (mode & PM_BOUNDS_LAST_OFFSET) != 0, d_report, d_scratch,
                                                 static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_embbag_bounds_check launch");
    return PM_OK;
}

int pm_fill_random(void* dst, int64_t count, int32_t dtype, int32_t dist, float lo, float hi, uint64_t seed,
                   pm_stream_t stream) {
    if (count < 0) return fail(PM_ERR_INVALID, "negative count");
    if (count > 0 && !dst) return fail(PM_ERR_INVALID, "dst is NULL");
    if (!dtype_is_weight(dtype)) return fail(PM_ERR_INVALID, "dtype must be PM_F32, PM_BF16 or PM_F16");
    if (dist != 0 && dist != 1) return fail(PM_ERR_INVALID, "dist must be 0 (uniform) or 1 (normal)");
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) != 0) return fail(PM_ERR_INVALID, "dst must be 16-byte aligned");
    hipError_t h = pm::launch_fill_random(dst, count, dtype, dist, lo, hi, seed, static_cast<hipStream_t>(stream));
    if (h != hipSuccess) return hip_fail(h, "pm_fill_random launch");
    return PM_OK;
}

}  // extern "C"
