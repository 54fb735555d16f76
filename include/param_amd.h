/*
 * include/param_amd.h -- C ABI of libparam_amd.so (MI355X / gfx950).
 *
 * The drop-in boundary of the build.  The reference
 * (facebookresearch/param) is 100 % Python and reaches its kernels through
 * torch / fbgemm_gpu Python calls, so "the reference's FFI for this path" is
 * the set of Python call sites below; each entry point names the call site it
 * replaces (paths relative to the reference root).  Plain pointers and sizes
 * only: no torch types, no allocation inside, stream-ordered and asynchronous,
 * re-entrant across distinct streams.  Every function returns 0 on success or
 * a negative PM_ERR_* code; pm_last_error() gives the message of the calling
 * thread's last failure.
 *
 * All device pointers are caller-owned HBM addresses on the current device.
 * pm_stream_t is a hipStream_t passed as an opaque pointer (NULL = the null
 * stream).
 */
#ifndef PARAM_AMD_H
#define PARAM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_ABI_VERSION 8

typedef void* pm_stream_t;

/* element types */
enum {
    PM_F32 = 0,
    PM_BF16 = 1,
    PM_F16 = 2,
    PM_F8E4M3 = 3,           /* OCP FP8 e4m3fn: table element of pm_embbag_fwd_f8 / pm_embedding_gather_f8 only (FP8 TABLES) */
    PM_F8E5M2 = 4,           /* OCP FP8 e5m2: likewise */
    PM_Q8 = 5,               /* 8-bit quantised rows: a table FORMAT code of pm_embbag_fwd_anyfmt / pm_embedding_gather_anyfmt only (MIXED-FORMAT TABLES) */
    PM_Q4 = 6,               /* 4-bit quantised rows: likewise */
    PM_I32 = 10,
    PM_I64 = 11
};

/* error codes */
enum {
    PM_OK = 0,
    PM_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, bad dtype) */
    PM_ERR_UNSUPPORTED = -2, /* valid but not implemented (e.g. dim not a multiple of the vector width) */
    PM_ERR_HIP = -3,         /* a HIP runtime call failed; message carries hipGetErrorString */
    PM_ERR_INDEX = -4        /* pm_embbag_check found an out-of-range index or a bad offset */
};

/*
 * One batched (multi-table) EmbeddingBag request, TBE layout
 * (train/compute/python/workloads/pytorch/split_table_batched_embeddings_ops.py:93-135,
 * 191-208): `indices` holds the per-table index lists concatenated table-major;
 * `offsets` has num_tables*batch entries (a trailing num_tables*batch+1-th entry
 * equal to num_indices is tolerated and never read); bag (t,b) spans
 * [offsets[t*batch+b], offsets[t*batch+b+1]) and the very last bag ends at
 * num_indices (torch include_last_offset=False rule, train/compute/pt/pytorch_emb.py:172-174).
 * A single nn.EmbeddingBag call is the num_tables == 1 case.
 *
 * Output / gradient addressing: the D_t floats of bag (t,b) live at
 *     base + out_offsets[t] + b * out_stride            (element units)
 * so out_offsets[t] = sum_{u<t} D_u, out_stride = sum_t D_t is the TBE layout
 * [batch, sum D] (pytorch_dist_backend.py:224-228) and out_offsets[t] = t*batch*D,
 * out_stride = D is dlrm.py's torch.stack layout [T, batch, D] (dlrm.py:384-387).
 *
 * [bag_begin, bag_begin+bag_count) selects a slice of the batch dimension so a
 * caller can pipeline chunks of the batch against the all-to-all
 * (pytorch_dist_backend.py:214-234 is the reference's per-op pipelining site).
 */
typedef struct pm_embbag_batch {
    int32_t num_tables;           /* T >= 1 */
    int32_t weight_dtype;         /* PM_F32 | PM_BF16 | PM_F16 : element type of every table */
    int32_t index_dtype;          /* PM_I64 | PM_I32 : element type of indices AND offsets */
    int32_t max_dim;              /* max_t dims[t]; every dims[t] must be a multiple of 4 (f32) / 8 (16-bit) */
    int64_t batch;                /* B: bags per table */
    int64_t num_indices;          /* N: total length of `indices` */
    int64_t bag_begin;            /* first bag (per table) to process, 0 <= bag_begin <= batch */
    int64_t bag_count;            /* bags (per table) to process; bag_begin+bag_count <= batch */
    const void* const* tables;    /* device [T]: base pointer of table t, row-major [rows[t], dims[t]] */
    const int64_t* rows;          /* device [T] */
    const int32_t* dims;          /* device [T] */
    const int64_t* out_offsets;   /* device [T], element units (see above) */
    int64_t out_stride;           /* element units (see above) */
    const void* indices;          /* device [N]; WRITTEN by pm_embbag_bounds_check in its two repairing modes, by nothing else */
    const void* offsets;          /* device [T*B] or [T*B+1]; WRITTEN by pm_embbag_bounds_check in its two repairing modes, by nothing else */
    const float* per_sample_weights; /* device [N] or NULL */
    int64_t fixed_pooling;        /* (ABI v4: only the sort_impl 1 / 2 alternatives read it; the default sort establishes every
                                     table's pooling on the device by reading the offsets.)
                                     L > 0: the caller GUARANTEES every bag has exactly L lookups (offsets[i] == i * L,
                                     num_indices == T * B * L) -- what every benchmark request of the reference looks like;
                                     0: bags may be ragged.  A hint that changes speed only: the sorted backward then knows
                                     where each table's lookups start without reading device memory (per-table sort segments,
                                     XCD-affine and two-phase apply).  pm_embbag_check verifies it; the kernels do not. */
    /* ABI v6: the BLOCKED send layout of a table-wise sharded exchange, [W][T][B_local][D] -- every peer's chunk of the pooled
       output is one contiguous run whose tiles are 16 KB runs (the [B, sum D] layout writes 512-byte pieces 24 KB apart).
       FORWARD: nothing new in the kernels -- the same indices / offsets arrays describe T * W request tables of batch B_local
       (request table t * W + w = the lookups of weight table t for the bags of block w: the arrays are table-major), with
       tables[t * W + w] = table t's pointer and out_offsets[t * W + w] = w * T * B_local * D + t * B_local * D, out_stride = D;
       `table_group` = W tells the launch that W consecutive request tables read ONE weight table, so that they are placed on
       one XCD (speed only).  BACKWARD (pm_embbag_bwd, pm_embbag_bwd_sorted*, pm_embbag_bwd_fused*): the request keeps its T
       weight tables and batch B = W * B_local (a row's lookups must meet in ONE run); the gradient of bag b of table t is read at
       out_offsets[t] + b * out_stride + (b >> grad_block_shift) * grad_block_extra (B_local = 2^grad_block_shift; out_offsets[t] =
       t * B_local * D, out_stride = D, grad_block_extra = (T - 1) * B_local * D).  0 / 0 / 0: no blocking. */
    int32_t table_group;
    int32_t grad_block_shift;
    int64_t grad_block_extra;      /* (needs grad_block_shift >= 1: a block of one bag is the un-blocked layout) */
    /* ABI v7: min_t dims[t] if the caller knows it on the host, 0 = not given (then treated as max_dim).  A hint that changes
       speed only.  The forward sizes its lane groups for max_dim -- G lanes x 16 bytes >= the widest row -- and with one group per
       bag a D = 16 fp32 table of a request whose widest table has D = 128 would keep 4 of every 32 lanes busy.  When
       min_dim says the request is MIXED (its narrowest table needs a smaller power-of-two lane group than its widest) the
       forward runs the flat-walk kernel with the lane group chosen PER TABLE on the device from dims[t] (sub-groups of 4 .. G
       lanes: a D = 16 row is one 64-byte load by 4 lanes, eight bags per 32-lane slot) and tiles sized per table by their lookups
       (~256 lookups, at most 256 bags).
       Results are bit-identical to a max_dim-wide launch (a bag is pooled by one sub-group, additions in index order).  A table
       narrower than min_dim merely wastes lanes.  Reference: mixed embedding dims, train/comms/pt/dlrm.py:384-385 (`mixed_dim`
       -> torch.cat(ly, dim=1)), :506-557. */
    int32_t min_dim;
    int32_t reserved0;             /* 0 */
} pm_embbag_batch;

/* ABI / build identification. */
int pm_abi_version(void);
const char* pm_build_info(void); /* "gfx950 ... " static string */
const char* pm_last_error(void); /* thread-local; "" if none */

/*
 * Forward: out(t,b)[:] = sum_{j in bag (t,b)} psw[j] * table_t[indices[j], :]
 * fp32 accumulation in index order (bit-identical to a sequential fp32 sum;
 * with per_sample_weights each step is one fused multiply-add), fp32 output.
 * Replaces: nn.EmbeddingBag.__call__ at train/compute/pt/pytorch_emb.py:40,61 and
 * train/comms/pt/dlrm.py:380 (T=1 each / one launch for all local tables), and the
 * fbgemm TBE forward at train/comms/pt/pytorch_dist_backend.py:221,845-849 and
 * split_table_batched_embeddings_ops.py:312.
 */
int pm_embbag_fwd(const pm_embbag_batch* op, float* out, pm_stream_t stream);

/*
 * The same lookup for FEW, LONG bags (inference-style requests: a handful of bags of thousands of lookups): one
 * workgroup per bag, the bag's lookups split over the workgroup's lane groups, partial sums combined with wavefront
 * shuffles and through LDS in a fixed order.  Deterministic, but NOT the sequential order: the result agrees with
 * pm_embbag_fwd to fp32 rounding (1e-5 relative to sum |row|), not bit for bit -- hence a separate entry point.
 * Same arguments and layout rules as pm_embbag_fwd; T * bag_count workgroups are launched.
 */
int pm_embbag_fwd_split(const pm_embbag_batch* op, float* out, pm_stream_t stream);

/*
 * ALTERNATES BUILD ONLY (libparam_amd_alt.so, `make alt`, -DPM_ALTERNATES: tests and tools; not in the product library -- the
 * deterministic backward below is the path, and 25 x faster).  Backward scatter-add with hardware atomics:
 *     dst_t[indices[j], :] += alpha * psw[j] * grad(t, bag(j))[:]
 * `grad` is addressed like `out` above.  dst_tables is a device array [T] of
 * destination base pointers with element type dst_dtype and the tables' shapes:
 *   - a dense fp32 gradient buffer with alpha = 1  == torch's dense EmbeddingBag
 *     backward (aten::_embedding_bag_dense_backward; autograd of pytorch_emb.py:179);
 *   - the tables themselves with alpha = -lr       == the fused in-place update the
 *     reference reaches through fbgemm (pytorch_dist_backend.py:854-857,
 *     split_table_batched_embeddings_ops.py:318-324), plain SGD form.
 * Accumulation uses hardware float atomics (order not fixed; duplicates allowed).
 * dst_dtype: PM_F32, or PM_BF16 / PM_F16 (packed 16-bit atomics, one rounding per add).
 */
#ifdef PM_ALTERNATES
int pm_embbag_bwd(const pm_embbag_batch* op, const float* grad, void* const* dst_tables,
                  int32_t dst_dtype, float alpha, pm_stream_t stream);
#endif

/*
 * Deterministic backward without atomics (the default path of the Python modules):
 *   pm_embbag_bwd_sorted_workspace  bytes of caller-owned device scratch for this request
 *                                   (>= 0), or a negative PM_ERR_* code;
 *   pm_embbag_sort_indices          builds one (table,row) key per lookup and sorts them
 *                                   (stable radix sort); depends on indices/offsets only, so
 *                                   it may run on a side stream under the forward pass;
 *   pm_embbag_bwd_sorted            same arithmetic as pm_embbag_bwd, but every destination
 *                                   row is read once, updated in fp32 registers in lookup
 *                                   order and written once: run-to-run reproducible, and
 *                                   bit-identical to a sequential CPU scatter-add for every
 *                                   row looked up at most 256 times in the call (hotter rows
 *                                   are summed as ordered per-chunk partial sums: same value
 *                                   up to fp32 rounding of the association).  Requires
 *                                   pm_embbag_sort_indices on the same workspace and request
 *                                   (stream-ordered before it).  16-bit destinations are
 *                                   widened, accumulated in fp32 and rounded once per row.
 * The apply must be given THE request the sort was issued for, on the same workspace: same indices / offsets POINTERS (the
 * segmented sort leaves its segments and pair counts on the device, keyed to the request's buffers: a copy of the arrays at
 * another address is another request), same batch, bag_begin, bag_count and weights; otherwise PM_ERR_INVALID.
 * max_rows = max_t rows[t] (host value; sizes the sort key).  The request must satisfy
 * num_indices < 2^32 and batch < 2^32.  Replaces the sort + segmented-reduce backward of
 * aten::_embedding_bag_dense_backward and fbgemm's TBE backward (same call sites as
 * pm_embbag_bwd).
 */
int64_t pm_embbag_bwd_sorted_workspace(const pm_embbag_batch* op, int64_t max_rows);
int pm_embbag_sort_indices(const pm_embbag_batch* op, int64_t max_rows, void* workspace,
                           int64_t workspace_bytes, pm_stream_t stream);
/*
 * The same with the number of BAG PHASES the apply may use: phases = 2 lets pm_embbag_bwd_sorted apply the lower and the
 * upper half of the bags in two launches (each re-reads only half a table's gradient rows, which then stay in the L2 of the
 * XCD serving that table) when the request has fixed pooling and its sizes allow; the result is unchanged (a row's
 * lookups are still added in lookup order).  The fused row-wise Adagrad needs every row's lookups in one run: sort with
 * phases = 1 (what pm_embbag_sort_indices does) for pm_embbag_bwd_sorted_adagrad*, which otherwise return PM_ERR_INVALID.
 * The library remembers, per workspace, how the last sort was laid out; the apply call must follow on the same workspace.
 * (`phases` is honoured by sort_impl 2 only: the default segmented sort, sort_impl 0, always lays the request out for a
 * one-launch apply, whatever `phases` says.)
 */
int pm_embbag_sort_indices_ex(const pm_embbag_batch* op, int64_t max_rows, int32_t phases, void* workspace,
                              int64_t workspace_bytes, pm_stream_t stream);
/*
 * Host-only: writes a one-line description of the layout pm_embbag_sort_indices_ex would choose for this request under
 * the current tuning ("sort=own key_bytes=4 ... passes=3 segmented=1 ... xcd=1 ...") into out.  No device access; for
 * tests, sweeps and bug reports.
 */
int pm_embbag_sort_plan(const pm_embbag_batch* op, int64_t max_rows, int32_t phases, char* out, int32_t out_bytes);
int pm_embbag_bwd_sorted(const pm_embbag_batch* op, const float* grad, void* const* dst_tables,
                         int32_t dst_dtype, float alpha, int64_t max_rows, const void* workspace,
                         int64_t workspace_bytes, pm_stream_t stream);
/*
 * ABI v6.  Sort + apply of one request in ONE call (what a backward step that does not hide the sort under other work
 * wants): pm_embbag_sort_indices followed by pm_embbag_bwd_sorted / pm_embbag_bwd_sorted_adagrad_ex on `stream`, same
 * arguments, same results bit for bit.  Because the library itself sequences the two halves, it may DEFER part of the sort
 * into the apply -- the hybrid backward (pm_set_hybrid_tuning): the sort half then only classifies the tables and builds
 * their "looked up twice" maps, and the apply half reads the request's indices and offsets again.  A sort issued on its own
 * (pm_embbag_sort_indices*) never defers: it consumes the request completely, so the caller may reuse the index buffer
 * once the sort has run, as the sort-aside contract above says.
 */
int pm_embbag_bwd_fused(const pm_embbag_batch* op, const float* grad, void* const* dst_tables, int32_t dst_dtype,
                        float alpha, int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream);
/*
 * ABI v4, host-only, for tests and tools: where the last pm_embbag_sort_indices* on this workspace left its pairs.
 * *keys / *vals: device pointers into the workspace (keys of *key_bytes bytes: table << *tshift | row; values: bag within
 * the table, or the lookup position for weighted requests); *d_count: device uint32 holding the number of pairs (batch
 * slices sort only their own lookups), or NULL when it is num_indices.  Valid until the next sort on the workspace.
 * After a sequence sort (pm_embseq_sort_indices, below) the values are lookup positions in the request's index array; this call and
 * pm_embbag_sort_status work there as after any other sort.
 */
int pm_embbag_sorted_pairs(const pm_embbag_batch* op, int64_t max_rows, const void* workspace, const void** keys,
                           const uint32_t** vals, const uint32_t** d_count, int32_t* key_bytes, int32_t* tshift);

/*
 * ABI v5.  What the last sort / apply on this workspace left on the device -- SYNCHRONOUS (copies a few words back and waits
 * for `stream`); for tests, tools and bench lines:
 *   lookback_fallbacks look-back walks of the key sort that stopped waiting for a predecessor tile's published digit counts and
 *                      counted that tile's digits themselves.  Harmless (the result is the same): it is how the one-kernel
 *                      passes make progress without assuming anything about the order in which workgroups are dispatched;
 *                      expected 0 on an otherwise idle device
 *   pairs_sorted       lookups that went through the sort (all of them, or the hybrid path's left-overs)
 *   hybrid_tables      tables whose step took the hybrid path (rows looked up once applied bag-major, see pm_set_hybrid_tuning)
 *   hybrid_launched    0: the hybrid kernels were not launched for this sort (off, weighted or tiny request); else the mode they ran in
 *   lds_pairs          (ABI v7) flagged lookups of hybrid tables that were sorted and applied inside LDS by the left-over kernel
 *                      (pm_set_hybrid_rest) and therefore never reached the sort: a hybrid step applies
 *                      num_indices - pairs_sorted - lds_pairs lookups bag-major
 *   lds_tables         (ABI v7) hybrid tables finished that way
 * Replaces nothing of the reference: it reports on the replacement for the sort inside aten::_embedding_bag_dense_backward
 * (call sites as pm_embbag_bwd_sorted).
 */
typedef struct pm_sort_status {
    uint32_t lookback_fallbacks;
    uint32_t pairs_sorted;
    uint32_t hybrid_tables;
    uint32_t hybrid_launched;
    uint32_t lds_pairs;
    uint32_t lds_tables;
} pm_sort_status;
int pm_embbag_sort_status(const pm_embbag_batch* op, int64_t max_rows, const void* workspace, pm_sort_status* out,
                          pm_stream_t stream);

/*
 * ABI v8.  Coalesced sparse gradient: per table t, the distinct rows its lookups hit and one fp32 gradient row per distinct row,
 *     row_ids[t][k] ascending,   values[t][k * dims[t] .. + dims[t]) = sum_{j : indices[j] == row_ids[t][k]} psw[j] * grad(t, bag(j))
 * (psw[j] = 1 without weights) -- what torch's EmbeddingBag(sparse=True) backward gives after .coalesce(), the gradient the reference's
 * autograd backward (train/comms/pt/dlrm.py:1290-1296) produces for the sparse=True tables of pytorch_dist_backend.py:924, with U_t
 * rows instead of a table-sized dense buffer.  Three stream-ordered calls on one caller-owned workspace, no allocation inside:
 *   pm_embbag_sparse_grad_workspace  bytes of workspace (>= pm_embbag_bwd_sorted_workspace: the sort's, then a few words per
 *                                    lookup and per tile of the relabelling), or a negative PM_ERR_* code;
 *   pm_embbag_sort_indices           the complete one-phase key sort, on that workspace;
 *   pm_embbag_sparse_grad_count      one pass over the sorted pairs: unique_counts[t] = U_t (device int64 [num_tables]), and every
 *                                    sorted key is REWRITTEN IN PLACE from (t << tshift) | row to (t << tshift) | slot, slot = the
 *                                    index of the row's run within its table (the row ids are kept in the workspace).  Until the
 *                                    next sort, pm_embbag_sorted_pairs shows slots, not rows, and pm_embbag_bwd_sorted* refuse the
 *                                    workspace (PM_ERR_INVALID); a second count on the same sort is refused too;
 *   pm_embbag_sparse_grad            row_ids: device array [T] of int64[U_t]; values: device array [T] of float[U_t * dims[t]], 16-byte
 *                                    aligned; both caller-allocated from unique_counts (a table with U_t = 0 is never touched).  Writes
 *                                    the row ids, zeroes the value rows and runs the sorted apply of pm_embbag_bwd_sorted (alpha = 1,
 *                                    fp32 destination) into them: values are bit-identical to that apply into a zeroed fp32 table, read
 *                                    at row_ids[t] -- for any run length.  May be repeated (another `grad`) until the next sort.
 * Same request rules, limits and refusals as the sorted backward (at most 1024 tables: split larger requests by tables, the calls are
 * independent; num_indices and batch below 2^32; dims multiples of 4), checked before anything is launched.  The sort must keep rows
 * ascending within a table: after pm_set_sort_tuning(1) the count call returns PM_ERR_UNSUPPORTED.  The gradient with respect to
 * per_sample_weights is a call of its own: pm_embbag_psw_grad.
 */
int64_t pm_embbag_sparse_grad_workspace(const pm_embbag_batch* op, int64_t max_rows);
int pm_embbag_sparse_grad_count(const pm_embbag_batch* op, int64_t max_rows, void* workspace, int64_t workspace_bytes,
                                int64_t* unique_counts, pm_stream_t stream);
int pm_embbag_sparse_grad(const pm_embbag_batch* op, const float* grad, int64_t max_rows, void* workspace, int64_t workspace_bytes,
                          int64_t* const* row_ids, float* const* values, pm_stream_t stream);

/*
 * Fused backward + exact row-wise Adagrad (the optimizer the reference configures for its TBE ops,
 * train/comms/pt/comms_utils.py:2014 and split_table_batched_embeddings_ops.py:289; algorithm as
 * published by fbgemm_gpu): per touched row r of table t,
 *     G      = sum over the row's lookups of psw[j] * grad(t, bag(j))[:]      (fp32)
 *     m[r]  += (sum_d G[d]^2) / D_t
 *     W[r]  -= lr / (sqrt(m[r]) + eps) * G
 * `momentum` is a device array [T] of fp32 state pointers, one value per row.  Same sort /
 * workspace / determinism contract as pm_embbag_bwd_sorted; max_dim <= 256 (fp32) / 512 (16-bit).
 */
int pm_embbag_bwd_sorted_adagrad(const pm_embbag_batch* op, const float* grad, void* const* tables,
                                 int32_t table_dtype, float* const* momentum, float lr, float eps,
                                 int64_t max_rows, const void* workspace, int64_t workspace_bytes,
                                 pm_stream_t stream);

/*
 * The same with the remaining options the reference's TBE operator passes to the optimizer
 * (train/compute/python/workloads/pytorch/split_table_batched_embeddings_ops.py:289-300: weight_decay,
 * weight_decay_mode, stochastic_rounding=True; algorithm as published by fbgemm_gpu's rowwise_adagrad):
 *     L2        : m[r] += (sum_d (G[d] + wd * W[r,d])^2) / D ;  W[r] = (1 - mult * wd) * W[r] - mult * G
 *     DECOUPLE  : m[r] += (sum_d G[d]^2) / D                 ;  W[r] = (1 - lr * wd)   * W[r] - mult * G
 * with mult = lr / (sqrt(m[r]) + eps).  stochastic_rounding (bf16 / fp16 tables only): the updated row is
 * rounded to the table type with probability proportional to the distance to the two neighbours (unbiased:
 * updates smaller than half an ulp are not lost on average); the random bits are a counter-based function of
 * (seed, table, row, column) -- pass a different seed every step; results are reproducible for a given seed.
 */
enum { PM_WD_NONE = 0, PM_WD_L2 = 1, PM_WD_DECOUPLE = 2 };
/* The options of BOTH fused Adagrad flavours: row-wise (pm_embbag_bwd_*_adagrad*) and element-wise (pm_embbag_bwd_*_adagrad_elem). */
typedef struct pm_rowwise_adagrad {
    float lr;
    float eps;
    float weight_decay;
    int32_t weight_decay_mode;     /* PM_WD_* */
    int32_t stochastic_rounding;   /* 0 / 1 */
    int32_t reserved;
    uint64_t seed;
} pm_rowwise_adagrad;
int pm_embbag_bwd_sorted_adagrad_ex(const pm_embbag_batch* op, const float* grad, void* const* tables,
                                    int32_t table_dtype, float* const* momentum, const pm_rowwise_adagrad* opt,
                                    int64_t max_rows, const void* workspace, int64_t workspace_bytes,
                                    pm_stream_t stream);
/* ABI v6: pm_embbag_sort_indices + pm_embbag_bwd_sorted_adagrad_ex in one call (see pm_embbag_bwd_fused: may take the hybrid path). */
int pm_embbag_bwd_fused_adagrad(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype,
                                float* const* momentum, const pm_rowwise_adagrad* opt, int64_t max_rows, void* workspace,
                                int64_t workspace_bytes, pm_stream_t stream);

/*
 * Fused backward + exact ELEMENT-wise Adagrad (fbgemm's EXACT_ADAGRAD, the optimizer the reference's TBE unit test builds
 * its operator with; the arithmetic of torch.optim.Adagrad with initial_accumulator_value = 0, lr_decay = 0): per touched
 * row r of table t and column d, with G as above,
 *     gx       = G[d] + wd * W[r,d]   (L2)      |   G[d]   (NONE, DECOUPLE)
 *     s[r,d]  += gx * gx
 *     W[r,d]   = W[r,d] - lr * gx / (sqrt(s[r,d]) + eps)                        NONE, L2
 *     W[r,d]   = (1 - lr * wd) * W[r,d] - lr * G[d] / (sqrt(s[r,d]) + eps)      DECOUPLE
 * `state` is a device array [T] of fp32 buffers shaped [rows_t, dims_t]: one value per weight, always fp32.  `opt` is the
 * row-wise calls' options struct (reserved = 0); stochastic_rounding as there.  Contract of pm_embbag_bwd_sorted_adagrad_ex /
 * pm_embbag_bwd_fused_adagrad: same sort and workspace rules, same refusals (a two-phase sort, a relabelled workspace, more
 * than 1024 tables, max_dim > 256 (fp32) / 512 (16-bit)), same determinism (a row's gradient is summed in lookup order for up
 * to 256 lookups, in a fixed chunk order beyond).  NONE and L2 are pinned to torch.optim.Adagrad by the tests; DECOUPLE and
 * stochastic rounding are restated only (no third-party implementation of them is at hand).
 * The ABI version is unchanged (8): a client that needs these two finds out at symbol resolution.
 */
int pm_embbag_bwd_sorted_adagrad_elem(const pm_embbag_batch* op, const float* grad, void* const* tables,
                                      int32_t table_dtype, float* const* state, const pm_rowwise_adagrad* opt,
                                      int64_t max_rows, const void* workspace, int64_t workspace_bytes,
                                      pm_stream_t stream);
/* sort + apply in one call (may take the hybrid path) */
int pm_embbag_bwd_fused_adagrad_elem(const pm_embbag_batch* op, const float* grad, void* const* tables, int32_t table_dtype,
                                     float* const* state, const pm_rowwise_adagrad* opt, int64_t max_rows, void* workspace,
                                     int64_t workspace_bytes, pm_stream_t stream);

/*
 * Gradient of per_sample_weights -- the one piece of mode="sum" autograd the table backwards above do not give: for every
 * lookup j of a bag (t, b) inside [bag_begin, bag_begin + bag_count)
 *     out[j] = sum_{c < D_t} grad(t, b)[c] * table_t[indices[j], c]
 * `grad` is addressed as the sorted backward addresses it: out_offsets[t] + b * out_stride, plus the blocked term
 * (b >> grad_block_shift) * grad_block_extra.  `out` is fp32 [num_indices], indexed like `indices`; lookups of bags outside the
 * slice are not written.  The value does not depend on the weights: op->per_sample_weights is ignored and may be NULL.  Run it
 * BEFORE an in-place update of the tables (the fused backwards): the gradient belongs to the weights the forward read.
 * Arithmetic, fixed so that the result is deterministic and independent of the launch shape (numpy restates it exactly:
 * tests/psw_grad_rules.py): table elements are widened to fp32 (exact); every product and every add is rounded to fp32 on its
 * own -- no fused multiply-add, unlike the weighted forward; lane l of a lookup's lane group owns columns [l V, (l + 1) V), V = 4
 * (fp32 tables) / 8 (16-bit tables), and adds its V products to +0 in ascending column order; the lane partials are combined by
 * an xor butterfly with masks 1, 2, 4, .. up to half the group width, lanes past D_t / V holding +0.  Since x + 0 == x the value
 * is the same for every power-of-two group width >= D_t / V: mixed-dim and max_dim-wide launches give the same bits.
 * One gather over the rows the forward read (D_t * e row bytes, the index and 4 bytes out per lookup; the gradient is read once
 * per bag): no atomics, no workspace, no allocation, stream-ordered.  Tables fp32 / bf16 / fp16, indices int32 / int64, any
 * number of tables.  max_dim <= 256 (fp32) / 512 (16-bit): wider requests get PM_ERR_UNSUPPORTED.  Request rules as
 * pm_embbag_fwd, blocked-gradient rules as pm_embbag_bwd_fused; a NULL grad, or a NULL out with num_indices > 0, is
 * PM_ERR_INVALID; an empty request is PM_OK without touching the device.
 * Replaces aten::_embedding_bag_per_sample_weights_backward (autograd of the weighted lookups at train/compute/pt/pytorch_emb.py:40,61)
 * and the indice_weights gradient of fbgemm's TBE backward (split_table_batched_embeddings_ops.py:318-324; the reference's TBE
 * example, run_op_split_table_batched_embeddings.py, runs weighted).
 * The ABI version is unchanged (8): a client that needs this call finds out at symbol resolution.
 */
int pm_embbag_psw_grad(const pm_embbag_batch* op, const float* grad, float* out, pm_stream_t stream);

/*
 * PADDING -- torch's nn.EmbeddingBag(mode="sum", padding_idx=...) rule, per table: padding_idx is a device array int64 [num_tables],
 * padding_idx[t] in [0, rows[t]) names table t's padding row, -1 says the table has none (a value outside [-1, rows[t]) is the
 * caller's error: the Python modules check it at construction).  A lookup j of table t with indices[j] == padding_idx[t] is PADDED:
 * it contributes nothing to the forward, its row receives no gradient and no optimizer update, and its per_sample_weights gradient
 * is +0.0.  The request struct is unchanged (sizeof 144): the array is an extra argument of the four functions below, and a client
 * that needs them finds out at symbol resolution -- the ABI version stays 8.  tests/padding_rules.py restates the rule in numpy.
 *
 * pm_embbag_fwd_padded   out(t, b)[:] = sum over the lookups j of bag (t, b) with indices[j] != padding_idx[t], in index order from +0.0,
 *                        of psw[j] * table_t[indices[j], :] -- plain fp32 adds unweighted, one fused multiply-add per kept lookup
 *                        weighted: the arithmetic of pm_embbag_fwd, and bit-identical to pm_embbag_fwd on the request with the padded
 *                        lookups removed.  A bag of padding only gives +0.0 everywhere, like an empty bag.  The padding row is never
 *                        read into a sum: a NaN or Inf stored there reaches no output.  Same request, layouts, dtypes, bag slices and
 *                        refusals as pm_embbag_fwd; a NULL padding_idx is PM_ERR_INVALID.  A kernel family of its own
 *                        (csrc/embbag_fwd_pad.hip): a tile's indices are compacted while they are staged into LDS, so a padded lookup
 *                        costs no row load; bags longer than the LDS index tile predicate the load off.
 * pm_embbag_pad_mask     values: fp32 [num_indices], indexed like `indices` (the output of pm_embbag_psw_grad): writes +0.0 at every
 *                        padded lookup of the bags inside [bag_begin, bag_begin + bag_count) and touches nothing else.  Run it behind
 *                        pm_embbag_psw_grad on the same stream.
 * pm_pad_rows_guard      keeps the padding rows out of a backward WITHOUT changing it: called with PM_PAD_SAVE before, and with
 *                        PM_PAD_RESTORE after, any of pm_embbag_bwd_sorted* / pm_embbag_bwd_fused* (one call or several: the table
 *                        ranges of a request of more than 1024 tables), it copies row padding_idx[t] of every table t that has one --
 *                        dims[t] elements of table_dtype at tables[t] -- into slot t of the caller-owned `stash` and back, and with it
 *                        the row's optimizer state: state_kind PM_PAD_STATE_ROW one fp32 at state[t][padding_idx[t]] (row-wise
 *                        Adagrad), PM_PAD_STATE_ELEM dims[t] fp32 at state[t] + padding_idx[t] * dims[t] (element-wise Adagrad),
 *                        PM_PAD_STATE_NONE nothing (state may be NULL).  After the restore the padding rows and their state hold their
 *                        earlier bits whatever the optimizer, decay mode or rounding did to them; every other row is what the backward
 *                        made it.  `tables` may be the weight tables or the fp32 destination buffers of a dense gradient.  One wave per
 *                        table, 16-byte copies, stream-ordered, no synchronisation.  stash: pm_pad_rows_guard_bytes(num_tables, max_dim,
 *                        table_dtype, state_kind) bytes, 16-byte aligned; max_dim >= every dims[t].  The padded lookups are still
 *                        sorted and accumulated by the backward in between -- into a row that is then put back.
 * Null pointers, an unknown dtype, state kind or direction, and a stash that is too small are PM_ERR_INVALID, before any HIP call.
 * Replaces the padding_idx handling inside aten::_embedding_bag / _embedding_bag_dense_backward /
 * _embedding_bag_per_sample_weights_backward (the kernels behind train/compute/pt/pytorch_emb.py:40,61,179).
 */
#define PM_PAD_SAVE    0
#define PM_PAD_RESTORE 1
enum { PM_PAD_STATE_NONE = 0, PM_PAD_STATE_ROW = 1, PM_PAD_STATE_ELEM = 2 };
int pm_embbag_fwd_padded(const pm_embbag_batch* op, const int64_t* padding_idx, float* out, pm_stream_t stream);
int pm_embbag_pad_mask(const pm_embbag_batch* op, const int64_t* padding_idx, float* values, pm_stream_t stream);
int64_t pm_pad_rows_guard_bytes(int32_t num_tables, int32_t max_dim, int32_t table_dtype, int32_t state_kind);
int pm_pad_rows_guard(int32_t num_tables, int32_t max_dim, void* const* tables, const int32_t* dims, int32_t table_dtype,
                      const int64_t* padding_idx, float* const* state, int32_t state_kind, void* stash, int64_t stash_bytes,
                      int32_t direction, pm_stream_t stream);

/*
 * MEAN POOLING -- torch's nn.EmbeddingBag(mode="mean") rule (fbgemm TBE: PoolingMode.MEAN, unweighted).  count(t, b) = the lookups of
 * bag (t, b) whose index is not table t's padding index.  padding_idx is the device array of PADDING above, or NULL when no table has a
 * padding row.  The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs the two calls finds out
 * at symbol resolution.  tests/mean_rules.py restates the rule in numpy.
 *
 * pm_embbag_fwd_mean     out(t, b)[:] = sum(t, b)[:] / (float)count(t, b) for count >= 1: sum is exactly what pm_embbag_fwd_padded gives
 *                        (additions in index order from +0.0, fp32; 16-bit rows widened first), followed by ONE correctly rounded IEEE
 *                        fp32 division per element -- not a multiplication by a reciprocal.  An empty bag or a bag of padding only
 *                        gives +0.0 with no division.  The padded forward's kernel with the division fused in front of its stores
 *                        (csrc/embbag_fwd_pad.hip): same tiling, layouts, dtypes, bag slices and refusals as pm_embbag_fwd_padded.
 *                        Mean is unweighted: per_sample_weights != NULL is PM_ERR_UNSUPPORTED.
 * pm_embbag_mean_grad    scaled(t, b)[:] = grad(t, b)[:] * r with r = 1.0f / (float)count(t, b): r is rounded to fp32 first, then one fp32
 *                        multiplication per element -- not a division of the gradient.  count == 0: +0.0 everywhere.  grad and scaled
 *                        are addressed like out (out_offsets[t] + b * out_stride); only the bags inside [bag_begin, bag_begin +
 *                        bag_count) are written; scaled may be grad itself.  Any number of tables.  The mean backward IS the sum
 *                        backward on `scaled`: pass it as the gradient of any of pm_embbag_bwd_sorted* / pm_embbag_bwd_fused* /
 *                        pm_embbag_sparse_grad (once, in front of the table ranges of a request of more than 1024 tables), with
 *                        pm_pad_rows_guard around it as before.  One launch: a lane group per bag, 16 bytes per lane.
 * Both refuse, before any HIP call: what pm_embbag_fwd refuses; blocked layouts (grad_block_shift != 0 or table_group != 0:
 * PM_ERR_UNSUPPORTED); a NULL out / grad / scaled or a grad / scaled that is not 16-byte aligned (PM_ERR_INVALID).  bag_count == 0 is
 * PM_OK without a launch.
 * Replaces the mode="mean" branches of aten::_embedding_bag and _embedding_bag_dense_backward / _embedding_bag_sparse_backward (the
 * kernels behind nn.EmbeddingBag at train/compute/pt/pytorch_emb.py:179) and PoolingMode.MEAN of fbgemm's TBE forward and backward
 * (split_table_batched_embeddings_ops.py:290), for unweighted requests.
 */
int pm_embbag_fwd_mean(const pm_embbag_batch* op, const int64_t* padding_idx, float* out, pm_stream_t stream);
int pm_embbag_mean_grad(const pm_embbag_batch* op, const int64_t* padding_idx, const float* grad, float* scaled, pm_stream_t stream);

/*
 * OUTPUT DTYPE -- a bf16 / fp16 pooled output and 16-bit gradients (fbgemm TBE: output_dtype = SparseType.BF16 | FP16; torch's
 * nn.EmbeddingBag over a 16-bit table returns 16 bits).  The request struct is unchanged (sizeof 144) and the ABI version stays 8: a
 * client that needs the two calls finds out at symbol resolution.  tests/out16_rules.py restates the rule in numpy.
 *
 * FORWARD   out16 = round16(out32), out32 = exactly what the fp32 forward of the same request gives: the sum (pm_embbag_fwd /
 *           pm_embbag_fwd_padded), the weighted sum or the mean (pm_embbag_fwd_mean), over fp32, bf16 or fp16 tables -- the same fp32
 *           additions in index order from +0.0, mean with the same single division.  ONE rounding follows, per element, in registers,
 *           to nearest even; nothing is rounded before it (no 16-bit partial sums).  fp16 overflow gives +-Inf; fp16 and bf16
 *           subnormals are produced, not flushed; signed zeros are kept.  A NaN becomes a quiet NaN of the same sign: bf16
 *           (u >> 16) | 0x40 of the fp32 bits u, fp16 what the hardware conversion gives (the payload is not part of the rule).
 * BACKWARD  a 16-bit gradient is widened exactly; every backward entry point then does what it does for that fp32 gradient.  With
 *           mean pooling the 1.0f / (float)count scaling happens in the launch that widens, and the result equals
 *           pm_embbag_mean_grad on the widened gradient bit for bit.  The caller's gradient is only read.
 *
 * pm_embbag_fwd_out16    the padded forward's kernel family (csrc/embbag_fwd_pad_kernel.inc) with a 16-bit output element: out is
 *                        out_dtype (PM_BF16 | PM_F16) and addressed like the fp32 out, out_offsets[t] + b * out_stride counted in
 *                        OUTPUT elements (the same numbers as for the fp32 request); only the bags inside [bag_begin, bag_begin +
 *                        bag_count) are written.  padding_idx: the device array of PADDING, or NULL (no table has a padding row).
 *                        mean: 0 = sum (weighted where per_sample_weights is given), 1 = mean.  The value is converted before it
 *                        goes to the LDS burst buffer or to the direct store, and leaves in pieces of 4 outputs (8 bytes: what the
 *                        alignment rules of a request guarantee).  Refused before any HIP call: what pm_embbag_fwd refuses; out_dtype
 *                        PM_F32 or unknown (PM_ERR_INVALID: fp32 output is pm_embbag_fwd / pm_embbag_fwd_padded / pm_embbag_fwd_mean);
 *                        mean not 0 / 1; blocked layouts (PM_ERR_UNSUPPORTED); mean with per_sample_weights (PM_ERR_UNSUPPORTED); a
 *                        NULL out or one that is not 8-byte aligned (PM_ERR_INVALID).  bag_count == 0 is PM_OK without a launch.
 * pm_embbag_grad_widen   grad32(t, b)[:] = (float)grad16(t, b)[:] (mean == 0), times r = 1.0f / (float)count(t, b) with +0.0 everywhere
 *                        for count == 0 (mean == 1: pm_embbag_mean_grad's arithmetic).  grad16 (grad_dtype PM_BF16 | PM_F16) and grad32
 *                        are addressed like out, each in its own elements; only the bags of the slice are written; any number of
 *                        tables, one launch (csrc/grad_widen.hip).  Pass grad32 to any of pm_embbag_bwd_sorted* / pm_embbag_bwd_fused*
 *                        / pm_embbag_sparse_grad / pm_embbag_psw_grad (once, in front of the table ranges of a request of more than
 *                        1024 tables).  Refusals as pm_embbag_mean_grad, plus grad_dtype PM_F32 or unknown, mean not 0 / 1, mean with
 *                        per_sample_weights; grad16 must be 8-byte and grad32 16-byte aligned, and the two must differ.
 * Replaces the output cast behind fbgemm's TBE forward (output_dtype) and the .to(torch.float32) pass in front of its backward.
 */
int pm_embbag_fwd_out16(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t out_dtype, void* out,
                        pm_stream_t stream);
int pm_embbag_grad_widen(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t grad_dtype, const void* grad16,
                         float* grad32, pm_stream_t stream);

/*
 * MAX POOLING -- torch's nn.EmbeddingBag(mode="max") rule, forward, arg-max and gradient.  padding_idx is the device array of PADDING
 * above, or NULL when no table has a padding row.  The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client
 * that needs the two calls finds out at symbol resolution.  tests/max_rules.py restates the rule in numpy.
 *
 * FORWARD   A bag's lookups that equal its table's padding index are removed first (after pm_embbag_bounds_check has repaired the
 *           request, where the caller runs it).  Per column c, over the remaining lookups r_0, r_1, ... in index order: the first sets
 *           cur = w[r_0, c], whatever it holds; every later one replaces it iff w[r_j, c] > cur -- an ordered, strict IEEE comparison,
 *           a compare-and-select and never fmaxf.  So a NaN in the first kept lookup stays; a NaN anywhere later never enters; of
 *           equal values the first wins (-0.0 followed by +0.0 stays -0.0); a bag of negative rows gives a negative maximum -- nothing
 *           is seeded with 0.0.  A bag without kept lookups (empty, or padding only) gives +0.0.  16-bit rows are widened exactly and
 *           compared in fp32; the widening is monotone, so the result is a stored value.  out_dtype PM_BF16 / PM_F16: ONE rounding of
 *           that fp32 result, in registers, as for pm_embbag_fwd_out16.  On fp32, bf16 and fp16 tables this is
 *           torch.nn.functional.embedding_bag(..., mode="max") on the CPU bit for bit (fp32 output of a 16-bit table: torch's widened).
 * ARG-MAX   max_indices(t, b)[c] = the row index that supplied cur, int32, at the element offset of out(t, b)[c] (out_offsets[t] + b *
 *           out_stride + c, counted in int32 elements); -1 for a bag without kept lookups (torch writes 0 there and never reads it).
 * BACKWARD  grad(t, b)[c] goes to row max_indices(t, b)[c] of table t; a row that a bag looks up twice receives it once.  Implemented
 *           as an expansion to a sequence gradient: g_seq[j, c] = grad(t, bag(j))[c] if j is the first position of its bag with
 *           indices[j] == max_indices(t, bag(j))[c], else +0.0; then the sequence backward (pm_embseq_*, below) of the same request
 *           runs unchanged on g_seq.  A table row therefore accumulates its bags' contributions in ascending bag order, which is
 *           torch's _embedding_bag_dense_backward order for max: bit-identical to torch's CPU autograd wherever a row has at most 256
 *           lookups in the request; above that the sequence route's ordered chunk partials apply.  A stated consequence: a looked-up
 *           row that wins no column receives additions of alpha * 0.0 -- nothing in a zeroed dense-gradient buffer, but a scatter-add
 *           with a positive alpha turns a stored -0.0 of such a row into +0.0.
 *
 * pm_embbag_fwd_max      a sibling of the padded forward's kernel (csrc/embbag_fwd_max.hip): same tiling, staging with padding
 *                        compaction, layouts, bag slices.  out is out_dtype (PM_F32 | PM_BF16 | PM_F16), addressed in its own elements;
 *                        max_indices NULL: not written (inference: nothing extra is stored).  Only the bags inside [bag_begin,
 *                        bag_begin + bag_count) are written, in out and in max_indices.
 * pm_embbag_max_grad     the expansion (csrc/embbag_max_grad.hip): grad (grad_dtype PM_F32 | PM_BF16 | PM_F16, widened exactly) and
 *                        max_indices are addressed like out, each in its own elements; g_seq is fp32, row j at g_seq + j *
 *                        g_seq_row_stride.  Only positions of bags inside the slice are written.  One launch, any number of tables:
 *                        a lane group per bag, one 16-byte non-temporal store per lane and position.  Pass g_seq (advanced to a table
 *                        range's first position for requests of more than 1024 tables) to pm_embseq_bwd_fused / pm_embseq_bwd_sorted.
 * Both refuse, before any HIP call: what pm_embbag_fwd refuses; per_sample_weights (PM_ERR_UNSUPPORTED: max is unweighted); blocked
 * layouts (PM_ERR_UNSUPPORTED); an unknown dtype; a NULL out / grad / max_indices (of the gradient call) / g_seq; out or grad not
 * 16-byte aligned (8-byte for a 16-bit dtype), max_indices or g_seq not 16-byte aligned (PM_ERR_INVALID).  pm_embbag_max_grad also
 * refuses mixed dims (min_dim given and != max_dim, PM_ERR_UNSUPPORTED: the sequence route needs one dim) and a g_seq_row_stride below
 * max_dim or not a multiple of 4.  An empty request (bag_count == 0; for the gradient also num_indices == 0) is PM_OK without a launch.
 * Replaces the mode="max" branches of aten::_embedding_bag and _embedding_bag_dense_backward.
 */
int pm_embbag_fwd_max(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t out_dtype, void* out, int32_t* max_indices,
                      pm_stream_t stream);
int pm_embbag_max_grad(const pm_embbag_batch* op, const void* grad, int32_t grad_dtype, const int32_t* max_indices, float* g_seq,
                       int64_t g_seq_row_stride, pm_stream_t stream);

/*
 * UN-POOLED LOOKUPS -- torch's nn.Embedding rule (fbgemm TBE: PoolingMode.NONE, sequence embeddings): one output row per lookup.  For
 * every lookup position j in [0, num_indices) that belongs to a bag inside [bag_begin, bag_begin + bag_count) of its table t
 *     out[j * out_row_stride + c] = conv(table_t[indices[j], c])      for c < dims[t]
 * and nothing else of `out` is touched: not the columns from dims[t] to out_row_stride, not the rows of positions outside the slice.
 * Table t owns the positions [offsets[t * batch], offsets[(t + 1) * batch]), the last table ends at num_indices (the borders the
 * pooled entry points use); the bags inside a table matter for the slice only.  out_offsets and out_stride of the request are not
 * read: `out` is addressed by position, with its own row stride, in elements of out_dtype.  tests/embedding_rules.py restates the rule.
 *   conv   same element type in and out (PM_F32 -> PM_F32, PM_BF16 -> PM_BF16, PM_F16 -> PM_F16): a bit copy -- -0.0, subnormals, Inf
 *          and NaN payloads leave exactly as stored, no arithmetic touches the value (the bag-of-one route through pm_embbag_fwd adds
 *          the row to +0.0, which turns -0.0 into +0.0, and always widens to fp32);
 *          a 16-bit table with out_dtype PM_F32: the exact widening of every pooled forward;
 *          an fp32 table with a 16-bit out_dtype, and bf16 <-> fp16: widened exactly, then rounded ONCE as pm_embbag_fwd_out16 rounds
 *          (OUTPUT DTYPE above; tests/out16_rules.py).
 * One launch for any number of tables (csrc/embedding_gather.hip): a tile is 256 consecutive positions, whatever tables they belong
 * to; a lane group moves one row with 16-byte loads and non-temporal stores, several rows in flight.  Tables fp32 / bf16 / fp16,
 * indices int32 / int64, dims[t] may differ per table.  No atomics, no workspace, no allocation, stream-ordered.
 * Refused on the host, before any HIP call: what pm_embbag_fwd refuses; an unknown out_dtype, a NULL out with num_indices > 0, an out
 * that is not 16-byte (PM_F32) / 8-byte (16-bit) aligned, out_row_stride < max_dim or not a multiple of 4 (PM_ERR_INVALID);
 * per_sample_weights != NULL, a non-zero table_group / grad_block_shift / grad_block_extra (PM_ERR_UNSUPPORTED).  num_indices == 0 or
 * bag_count == 0 is PM_OK without a launch.  The gradient needs no call of its own: it is the sum backward of the request "one bag per
 * lookup" (offsets = 0, 1, 2, ..; batch = num_indices) on the gradient rows.
 * Replaces aten::embedding behind nn.Embedding (the un-pooled sibling of the module at train/compute/pt/pytorch_emb.py:179) and
 * PoolingMode.NONE of fbgemm's TBE forward (split_table_batched_embeddings_ops.py:290 names the pooling mode).
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs this call finds out at symbol resolution.
 */
int pm_embedding_gather(const pm_embbag_batch* op, int32_t out_dtype, void* out, int64_t out_row_stride, pm_stream_t stream);

/*
 * ROW-QUANTISED TABLES -- sum pooling (weighted where per_sample_weights is given) straight from tables stored in the 8- or 4-bit
 * row-wise format: no fp32 copy of a table exists at any point.  op->tables[t] points at uint8 [rows[t], row_bytes(dims[t], bits)],
 * contiguous, 4-byte aligned: the bytes pm_rows_quantize writes and torch's quantized::embedding_bag_{byte,4bit}_prepack produce --
 *   the codes of the dims[t] columns first (a 4-bit code of column c in byte c / 2 at bit 4 * (c % 2)), then the row's tail:
 *   bits 8: fp32 scale, fp32 bias (row_bytes = D + 8); bits 4: fp16 scale, fp16 bias, widened exactly (row_bytes = D / 2 + 4).
 * op->dims[t] is the LOGICAL column count D_t; op->weight_dtype is not read.  Everything else of the request is pm_embbag_fwd's: T
 * tables, out_offsets / out_stride, bag_begin / bag_count, int32 / int64 indices, per_sample_weights.
 * THE RULE, for bag (t, b) and column c, over the bag's lookups j in index order from acc = +0.0:
 *     sc  = fl32(scale_r * w_j)      bi = fl32(bias_r * w_j)       (without per_sample_weights: sc = scale_r, bi = bias_r)
 *     acc = fmaf(sc, (float)code[r, c], fl32(acc + bi))            r = indices[j]
 * one fp32 addition, then one fused multiply-add, per element and lookup; an empty bag gives +0.0.  That is, bit for bit, what torch's
 * CPU operators quantized::embedding_bag_byte_rowwise_offsets and quantized::embedding_bag_4bit_rowwise_offsets compute
 * (tests/qrows_rules.py restates it with exact arithmetic; tests/test_qrows_host.py pins the restatement to the operators).  Two
 * consequences: the result is NOT bit-identical to pm_embbag_fwd over pm_rows_dequantize of the table (that dequantises each element
 * with its own rounding, then adds) -- the two agree within summation rounding, |diff| <= (2L + 2) 2^-24 sum_j |w_j| (|bias_j| + code
 * scale_j) for a bag of L lookups; and a bag of exactly one unweighted lookup equals pm_rows_dequantize of that row as a value
 * (0 + bias is exact).  out_dtype PM_F32, or PM_BF16 / PM_F16: the fp32 value rounded ONCE, in registers, as pm_embbag_fwd_out16
 * rounds (OUTPUT DTYPE above); out is addressed in OUTPUT elements, only the bags of the slice and only the columns below dims[t] are
 * written.
 * One launch for any number of tables (csrc/embbag_fwd_qrows.hip): the padded forward's tile structure, two dwords of codes per lane
 * and row (lane groups sized for max_dim: no per-table sub-groups), loads at dword-aligned addresses -- rows start on 4-byte boundaries
 * and no better.
 * Column rules: dims[t] % 4 == 0 (bits 8), dims[t] % 8 == 0 (bits 4), dims[t] <= 4096.
 * Refused on the host, before any HIP call: what pm_embbag_fwd refuses about the request (the column rules as its "multiple of the
 * vector width" rule: PM_ERR_UNSUPPORTED); bits not 8 or 4 (PM_ERR_INVALID; 2 and 16 -- payload formats of pm_rows_quantize -- are
 * PM_ERR_UNSUPPORTED); an unknown out_dtype (PM_ERR_INVALID); max_dim > 4096, a non-zero table_group / grad_block_shift /
 * grad_block_extra (PM_ERR_UNSUPPORTED); a NULL out or one that is not 16-byte (PM_F32) / 8-byte (16-bit) aligned (PM_ERR_INVALID).
 * bag_count == 0 is PM_OK without a launch.  No gradient: the tables are not trainable.
 * pm_embbag_qrows_plan: the geometry that call WOULD use (plan_qrows, csrc/launch_plan.h) -- the twelve members of pm_embbag_plan in its
 * order; the tile kernel, staged where stage_out > 0; unroll 2 or 4 (pm_set_tuning's unroll: below 4 -> 2, from 4 on -> 4; pm_set_tuning's
 * bags_per_block and pm_set_forward_tuning's stage_out are honoured, nothing else of the knobs is read).  Host only, launches nothing;
 * validates as the launching call does, except for `out` of that call.
 * Replaces torch's two CPU operators named above (behind torch.ao.nn.quantized.EmbeddingBag) and the forward of fbgemm's
 * IntNBitTableBatchedEmbeddingBagsCodegen for INT8 / INT4 tables.  Left out: 2-bit tables, mean, padding_idx, a padded row stride (the
 * un-pooled lookup: below; tables of differing format in one launch: PER-TABLE FORMATS below; pruned rows: PRUNED TABLES below).
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these two finds out at symbol resolution.
 */
int pm_embbag_fwd_qrows(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, void* out, pm_stream_t stream);
int pm_embbag_qrows_plan(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, int32_t out[12]);

/*
 * ROW-QUANTISED TABLES, UN-POOLED -- one output row per lookup from the same tables: the request and the addressing of UN-POOLED
 * LOOKUPS above (table t owns the positions [offsets[t * batch], offsets[(t + 1) * batch]); `out` is addressed by position with its own
 * row stride, in elements of out_dtype; out_offsets / out_stride of the request are not read), the tables and bits of ROW-QUANTISED
 * TABLES.  op->weight_dtype is not read.
 * THE RULE: for every lookup position j that belongs to a bag inside [bag_begin, bag_begin + bag_count) of its table t, r = indices[j],
 * per column c < dims[t]
 *     out[j * out_row_stride + c] = conv( fmaf(scale_r, (float)code[r, c], fl32(+0.0f + bias_r)) )
 * and nothing else of `out` is touched.  conv: the identity for PM_F32; for PM_BF16 / PM_F16 ONE rounding of that fp32 value, in
 * registers, as pm_embbag_fwd_out16 rounds.  It is the pooled rule above for one unweighted bag of one lookup, bit for bit -- and with
 * it what torch's quantized::embedding_bag_{byte,4bit}_rowwise_offsets give for bags of one and quantized::embedding_byte gives
 * (tests/qgather_rules.py restates it, tests/test_qgather_host.py pins it to the operators).  The addition is part of the rule: it is
 * NOT fmaf(scale, code, bias) -- a bias of -0.0 enters the fused multiply-add as +0.0, so a finite row gives no -0.0 (a negative scale,
 * a code of 0 and a bias of -0.0 would give one).  Consequence: the result equals pm_rows_dequantize of the row as a value, not on the sign of zeros.
 * One launch for any number of tables (csrc/embedding_gather_qrows.hip): pm_embedding_gather's tiles of 256 consecutive positions; a
 * lane group serves one row with two dwords of codes per lane (dword-aligned loads that stay inside the row), unpacks and applies the
 * rule in registers and stores non-temporally, several rows in flight.  dims[t] may differ per table: only the columns below dims[t]
 * of a position's row are written.  No atomics, no workspace, no allocation, stream-ordered.
 * Refused on the host, before any HIP call: what pm_embbag_fwd_qrows refuses about the request, bits and out_dtype (bits 2 / 16
 * PM_ERR_UNSUPPORTED, other values PM_ERR_INVALID; the column rules dims[t] % 4 / % 8 and max_dim > 4096 PM_ERR_UNSUPPORTED; a non-zero
 * table_group / grad_block_shift / grad_block_extra PM_ERR_UNSUPPORTED; an unknown out_dtype PM_ERR_INVALID); per_sample_weights !=
 * NULL (PM_ERR_UNSUPPORTED); out_row_stride < max_dim or not a multiple of 4 (PM_ERR_INVALID).  num_indices == 0 or bag_count == 0
 * is then PM_OK without a launch; otherwise a NULL out, or one that is not 16-byte (PM_F32) / 8-byte (16-bit) aligned, is PM_ERR_INVALID.
 * pm_embedding_gather_qrows_plan: the geometry that call WOULD use (plan_gather_qrows, csrc/launch_plan.h) -- the eight members of
 * pm_embedding_gather_plan in its order: vec (columns a lane holds per pass: 8 / 16), group_lanes, tile, col_passes, unroll (pm_set_tuning's
 * unroll rounded down to 1 / 2 / 4 / 8), lds_borders, xcd_contiguous, grid.  Host only, launches nothing; validates the request as the
 * launching call does (`out` and out_row_stride of that call, and an out_dtype, are not part of it).
 * Replaces quantized::embedding_byte / embedding_4bit (behind torch.ao.nn.quantized.Embedding) and PoolingMode.NONE of fbgemm's
 * IntNBitTableBatchedEmbeddingBagsCodegen for INT8 / INT4 tables.  Left out: 2-bit tables, a padded row stride, padding_idx,
 * per-position weights, a lane width per format, any backward (the tables are not trainable).  Tables of
 * differing format in one launch: PER-TABLE FORMATS below; pruned rows / index remapping: PRUNED TABLES below.
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these two finds out at symbol resolution.
 */
int pm_embedding_gather_qrows(const pm_embbag_batch* op, int32_t bits, int32_t out_dtype, void* out, int64_t out_row_stride,
                              pm_stream_t stream);
int pm_embedding_gather_qrows_plan(const pm_embbag_batch* op, int32_t bits, int64_t out[8]);

/*
 * ROW-QUANTISED TABLES, PER-TABLE FORMATS -- the two lookups above in ONE launch over tables that are EACH stored in the 8-bit or the
 * 4-bit row format (a serving model keeps its big tables at 4 bits and its small or sensitive ones at 8): table_bits is a DEVICE array
 * of num_tables ints, table_bits[t] = 8 or 4, read by the kernels like op->dims; its contents are the caller's responsibility, as those
 * of rows and dims are.  op->tables[t] points at uint8 [rows[t], row_bytes(dims[t], table_bits[t])], the bytes of ROW-QUANTISED TABLES:
 * row_bytes = D + 8 (8 bits) or D / 2 + 4 (4 bits).  Everything else of the request and of `out` is the single-format call's.
 * THE RULE: no new arithmetic.  Pooled: the output columns of table t are bit for bit what pm_embbag_fwd_qrows gives for that table alone
 * with bits = table_bits[t] -- acc = fmaf(sc, (float)code, fl32(acc + bi)) in index order from +0.0, weighted or not, fp32 or ONE
 * rounding to bf16 / fp16, an empty bag +0.0.  Un-pooled: row j is bit for bit what pm_embedding_gather_qrows gives with the bits of the
 * table that owns position j -- conv(fmaf(scale, code, fl32(+0.0 + bias))).  (tests/qmixed_rules.py applies tests/qrows_rules.py /
 * tests/qgather_rules.py table by table.)
 * One launch each (csrc/embbag_fwd_qmixed.hip, csrc/embedding_gather_qmixed.hip): a lane holds EIGHT COLUMNS of a row whatever its
 * format -- two dwords of an 8-bit row, one dword of a 4-bit row -- so the lane group (sized for max_dim / 8), the accumulators, the
 * column passes and the output pieces are one for every table, and the plan needs no knowledge of the formats present: it is a function
 * of the request struct, out_dtype and the tuning knobs alone (no further host-side argument).  Pooled: a tile's bags belong to one
 * table, the workgroup branches once per tile into its format's row loop.  Un-pooled: the format is a row's; lane groups of one wave may
 * differ in it and run one instruction stream.  Every read stays inside a row.  No atomics, no workspace, no allocation, stream-ordered.
 * Column rule: dims[t] % 8 == 0 for EVERY table (the stricter of the two formats' rules), dims[t] <= 4096.
 * Refused on the host, before any HIP call: everything the single-format calls refuse about the request, out_dtype, `out` and
 * out_row_stride; a NULL table_bits (PM_ERR_INVALID); max_dim % 8 or min_dim % 8 non-zero (PM_ERR_UNSUPPORTED).  bag_count == 0 (and,
 * un-pooled, num_indices == 0) is PM_OK without a launch.
 * pm_embbag_qrows_mixed_plan / pm_embedding_gather_qrows_mixed_plan: the geometry the two calls WOULD use (plan_qmixed,
 * plan_gather_qmixed, csrc/launch_plan.h) -- the twelve members of pm_embbag_plan / the eight of pm_embedding_gather_plan in their order
 * (vec is 8); host only, nothing is launched, and no table_bits: the plans do not depend on the formats.
 * Measured (tools/qmixed_probe.py, profiles/qmixed_probe.json; tables alternately 8- and 4-bit; us per call, fp32 output, uniform | Zipf
 * 1.05 indices; (a) this call, (b) two single-format launches plus the copies that interleave their results, (c) the two launches alone):
 *   16 x 10 M x 128, batch 8192, pooling 20   pooled     (a) 121.3 |  78.3   (b) 160.4 | 109.3   (c) 123.2 |  78.0
 *                                             un-pooled  (a) 350.1 | 311.2   (b) 811.9 | 786.3   (c) 356.3 | 359.0
 *   64 x 1 M x 64, batch 256, pooling 10      pooled     (a)  10.6 |  10.7   (b)  34.0 |  34.4   (c)  21.0 |  21.3
 *                                             un-pooled  (a)  14.2 |  11.8   (b)  39.2 |  36.4   (c)  22.9 |  23.6
 * (a) is never slower than (b) or, beyond the 0.9 % spread, than (c); fp16 output and the lane layout: README.md, "Per-table formats".
 * Replaces the per-table weights_tys of fbgemm's IntNBitTableBatchedEmbeddingBagsCodegen for INT8 / INT4.  Left out: fp16 / bf16 / fp32
 * rows in the same launch (the format is an int per table so that 16 can follow), 2-bit tables, mean, padding_idx, a padded row stride,
 * per-table lane sub-groups, any backward (pruned rows / index remapping: PRUNED TABLES below).
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these four finds out at symbol resolution.
 */
int pm_embbag_fwd_qrows_mixed(const pm_embbag_batch* op, const int32_t* table_bits, int32_t out_dtype, void* out, pm_stream_t stream);
int pm_embbag_qrows_mixed_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t out[12]);
int pm_embedding_gather_qrows_mixed(const pm_embbag_batch* op, const int32_t* table_bits, int32_t out_dtype, void* out,
                                    int64_t out_row_stride, pm_stream_t stream);
int pm_embedding_gather_qrows_mixed_plan(const pm_embbag_batch* op, int64_t out[8]);

/*
 * ROW-QUANTISED TABLES, PRUNED TABLES -- the two PER-TABLE FORMATS lookups over tables whose rows were pruned: a request addresses table
 * t's LOGICAL rows and an int32 array per table maps each logical row to a physical row or to -1, "pruned" (fbgemm's
 * index_remappings_array / index_remappings_array_offsets; torch's pruned_weights=True / compressed_indices_mapping).  remap is a DEVICE
 * int32 array, the tables' remaps concatenated; remap_offsets a DEVICE int64 array of num_tables + 1 entries, non-decreasing.  Table t is
 * pruned if and only if remap_offsets[t + 1] > remap_offsets[t]; its logical row r is physical row remap[remap_offsets[t] + r], a value in
 * [-1, physical rows of t).  A table that is not pruned is the identity.  op->rows[t] is the table's INDEX SPACE (logical rows): the
 * sanitiser reads it, the lookup kernels do not.  op->tables[t], table_bits and everything else are the per-table-format calls'; the
 * arrays' contents are the caller's responsibility, as those of dims and table_bits are.  The un-pooled call reads 8 bytes at
 * op->tables[0] for a pruned position (as for a position that is not written): tables[0] points at 8 readable bytes even if every row
 * of table 0 is pruned.
 * THE RULE: no new arithmetic.  Pooled: within a bag the lookups whose remap value is -1 are REMOVED -- index and weight alike, whatever
 * the weight's value (a non-finite weight of a pruned lookup does not reach the bag) --, the others take their remap value, and the
 * result is the rule of ROW-QUANTISED TABLES: acc = fmaf(sc, (float)code, fl32(acc + bi)) in index order from +0.0; a bag that is empty
 * or all pruned gives +0.0; a 16-bit output is one rounding.  It is bit for bit what pm_embbag_fwd_qrows_mixed gives over the physical
 * tables for the request with the pruned lookups deleted and the rest remapped -- and what torch's
 * quantized::embedding_bag_{byte,4bit}_rowwise_offsets give with pruned_weights=True (tests/pruned_rules.py restates it,
 * tests/test_pruned_host.py pins it to the operators).  Un-pooled: a position of the bag slice whose remap value is -1 receives +0.0 of
 * out_dtype in the columns [0, dims[t]) of its row (fbgemm's nobag kernel writes zeros); every other position the un-pooled rule over the
 * remapped row; positions outside the slice are not touched.
 * One launch each (csrc/embbag_fwd_qpruned.hip, csrc/embedding_gather_qpruned.hip), kernels of their own beside the per-table-format
 * ones -- also for tables of one format: pass table_bits.  Pooled: the workgroup remaps a staged tile's indices in LDS in place (one
 * pass, the tile's 4-byte loads in flight together, one barrier; a table that is not pruned skips it), a tile beyond the index tile loads
 * its U remap values back to back; a pruned lookup issues no row load.  Un-pooled: the remap load stands with the index load, in front of
 * the row's address.  No atomics, no workspace, no allocation, stream-ordered.  The geometry is the per-table-format calls':
 * pm_embbag_qrows_mixed_plan / pm_embedding_gather_qrows_mixed_plan report it for the same request (there is no plan call of its own).
 * Refused on the host, before any HIP call: everything pm_embbag_fwd_qrows_mixed / pm_embedding_gather_qrows_mixed refuse (dims[t] % 8
 * for every table included), then a NULL remap_offsets or a NULL remap (PM_ERR_INVALID): BOTH arrays are required -- a request without a
 * pruned table goes to the per-table-format calls.  bag_count == 0 (and, un-pooled, num_indices == 0) is PM_OK without a launch.
 * Measured (tools/pruned_probe.py, profiles/pruned_probe.json; half of every table's rows kept, tables alternately 8- and 4-bit; us per
 * call, fp32 output, uniform | Zipf 1.05 indices; (a) this call, (b) the route there was before: one torch gather of the request through
 * the remap with -1 redirected to an all-zero sentinel row, then the per-table-format call, (c) the per-table-format call over the
 * physical tables with no remapping, for context):
 *   16 x 10 M x 128, batch 8192, pooling 20   pooled     (a) 145.2 |  97.5   (b) 155.9 | 105.9   (c) 122.8 |  75.9
 *                                             un-pooled  (a) 344.2 | 350.4   (b) 369.9 | 298.3   (c) 354.4 | 325.8
 *   64 x 1 M x 64, batch 256, pooling 10      pooled     (a)  11.5 |  10.2   (b)  20.1 |  18.3   (c)  10.1 |  10.2
 *                                             un-pooled  (a)  13.6 |  11.4   (b)  19.4 |  19.3   (c)  13.4 |  11.1
 * (a) is not slower than (b) in seven of the eight cases (0.56-0.93 of its time); THE UN-POOLED CALL UNDER ZIPF INDICES AT THE LARGE SHAPE
 * IS 17 % SLOWER THAN (b) (350.4 against 298.3 us; spread 0.1 %): README.md, "Pruned tables".
 * Replaces index_remappings_array of fbgemm's IntNBitTableBatchedEmbeddingBagsCodegen for INT8 / INT4.  Left out: the hash-based remap
 * (pruned_hash_remap), pruned fp32 / bf16 training tables, single-format 8-bit dims that are multiples of 4 but not 8, 2-bit tables, mean,
 * padding_idx, any backward.
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these two finds out at symbol resolution.
 */
int pm_embbag_fwd_qrows_pruned(const pm_embbag_batch* op, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets,
                               int32_t out_dtype, void* out, pm_stream_t stream);
int pm_embedding_gather_qrows_pruned(const pm_embbag_batch* op, const int32_t* table_bits, const int32_t* remap, const int64_t* remap_offsets,
                                     int32_t out_dtype, void* out, int64_t out_row_stride, pm_stream_t stream);

/*
 * FP8 TABLES -- the pooled and the un-pooled lookup over tables stored in OCP FP8: one byte per element, no scale, no bias.
 * op->weight_dtype is PM_F8E4M3 (e4m3fn) or PM_F8E5M2 (e5m2), one format per request; op->tables[t] points at uint8 [rows[t], dims[t]],
 * row-major, rows back to back, 16-byte aligned; dims[t] % 16 == 0, dims[t] <= 2048.  A D = 128 row is one aligned 128-byte line.
 * dec(code), the fp32 value of a byte:
 *   e4m3fn  1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; 0x7f / 0xff are NaN; exponent field 0 is subnormal
 *           (mantissa / 8 * 2^-6); the largest value is 448 (0x7e);
 *   e5m2    1 sign, 5 exponent (bias 15), 2 mantissa bits, IEEE-like: 0x7c / 0xfc are +-Inf, 0x7d-0x7f / 0xfd-0xff are NaN; code << 8 is
 *           the fp16 pattern of the same value.
 * Subnormal codes decode exactly, 0x80 is -0.0, and every non-NaN code is exact in fp32, bf16 and fp16.  A NaN code gives a NaN; its
 * sign and payload are not part of the rule.  (gfx950 converts these two formats in hardware; the fnuz formats of MI300 are others.)
 * THE RULE, pooled (pm_embbag_fwd_f8): the padded family's rule over the decoded table.  Lookups whose index equals padding_idx[t] are
 * removed first (padding_idx: device int64 [num_tables], -1 = the table has no padding row; NULL = no table has one).  Then per column,
 * from acc = +0.0 in index order: acc = acc + dec(code) -- with per_sample_weights acc = fmaf(w_j, dec(code), acc).  mean == 1: one
 * correctly rounded fp32 division by the number of kept lookups; a bag that is empty or all padding gives +0.0 (no division).
 * out_dtype PM_F32, or PM_BF16 / PM_F16: that fp32 value rounded ONCE, in registers, as pm_embbag_fwd_out16 rounds; out is addressed
 * like pm_embbag_fwd's in elements of out_dtype (out_offsets[t] + b * out_stride).  It is what pm_embbag_fwd_padded / _mean / _out16
 * give over the table widened to fp32, and torch.nn.functional.embedding_bag(indices, table.to(torch.float32), ...) on the CPU, bit
 * for bit (tests/f8_rules.py restates it, tests/test_f8_host.py pins it to torch).
 * THE RULE, un-pooled (pm_embedding_gather_f8): the request and the addressing of UN-POOLED LOOKUPS above; for every lookup position j
 * that belongs to a bag inside the slice, out[j * out_row_stride + c] = conv(dec(table_t[indices[j], c])), c < dims[t]; nothing else of
 * out is touched.  The widening is exact for all three out_dtypes: -0.0, subnormals and +-Inf leave as they are stored.  No padding_idx.
 * Kernels: csrc/embbag_fwd_f8_kernel.inc -- the padded forward's tiling (bag offsets and compacted indices in LDS, tiles beyond the
 * index tile read from the request, the LDS output burst), sixteen columns per lane, 2 / 4 / 8 rows in flight per lane group -- and
 * csrc/embedding_gather_f8.hip -- pm_embedding_gather's tiles with four columns per lane, so that every store instruction of a lane
 * group writes consecutive pieces of the row.  No atomics, no workspace, no allocation, stream-ordered; 64-bit row addressing.
 * Refused on the host, before any HIP call: what pm_embbag_fwd / pm_embedding_gather refuse about a request; a weight_dtype other than
 * the two (PM_ERR_INVALID); max_dim or min_dim not a multiple of 16, max_dim > 2048, a non-zero table_group / grad_block_shift /
 * grad_block_extra (PM_ERR_UNSUPPORTED); an unknown out_dtype, mean not 0 / 1 (PM_ERR_INVALID); per_sample_weights with mean == 1 or
 * for the gather (PM_ERR_UNSUPPORTED); out_row_stride < max_dim or not a multiple of 4 (PM_ERR_INVALID).  An empty request (bag_count
 * == 0; the gather: num_indices == 0 as well) is then PM_OK without a launch; otherwise a NULL out, or one that is not 16-byte (PM_F32)
 * / 8-byte (16-bit) aligned, is PM_ERR_INVALID.  Every other entry point keeps refusing the two dtypes.
 * pm_embbag_f8_plan / pm_embedding_gather_f8_plan: the geometry the two calls WOULD use (plan_f8, plan_gather_f8, csrc/launch_plan.h) --
 * the twelve members of pm_embbag_plan (unroll 2 / 4 / 8: pm_set_tuning's unroll, below 4 -> 2, below 8 -> 4; default 2) and the eight of
 * pm_embedding_gather_plan (vec = 4) in their order.  Host only; they validate the request as the launching calls do.
 * Replaces the forward of fbgemm's IntNBitTableBatchedEmbeddingBagsCodegen for SparseType.FP8 tables.  Left out: a quantiser and any
 * scaling (per-row or per-table scales), the fnuz formats, FP8 output, a format per table, FP8 next to 8- / 4-bit tables in one launch,
 * max pooling, pruning, any backward (the tables are not trainable).
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these four finds out at symbol resolution.
 */
int pm_embbag_fwd_f8(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t out_dtype, void* out, pm_stream_t stream);
int pm_embbag_f8_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t out[12]);
int pm_embedding_gather_f8(const pm_embbag_batch* op, int32_t out_dtype, void* out, int64_t out_row_stride, pm_stream_t stream);
int pm_embedding_gather_f8_plan(const pm_embbag_batch* op, int64_t out[8]);

/*
 * SCALED FP8 TABLES -- FP8 TABLES with a power-of-two scale: a quantiser, and the pooled and the un-pooled lookup reading what it writes.
 * A plain cast to FP8 loses a table of small values (|x| <= 3.2e-4, the uniform init of 10 M rows, is all zeros in e4m3fn); fbgemm's FP8
 * int-nbit tables carry an exponent bias per module for the same reason.
 * THE STORED VALUE of element (r, c) of table t is  v = dec(code[r, c]) * 2^(E_t + e_r):  dec as in FP8 TABLES; E_t an int32 per table
 * (table_exp, a device array of num_tables values), e_r an int8 per row (row_exp, a device array of num_tables device pointers to int8
 * [rows[t]]).  Either array may be absent (NULL), which means 0; E_t + e_r lies in [-64, 64] (the caller's contract; the kernels clamp the
 * sum to that range before they build 2^s from it).  In that range v is exact in fp32 for every non-NaN code of both formats and always
 * normal (the smallest magnitude is 2^-16 * 2^-64), so the rule does not depend on how a kernel forms v.
 * THE RULE, pooled (pm_embbag_fwd_f8_scaled): pm_embbag_fwd_f8's with v in the place of dec(code) -- padding lookups removed first; per
 * column from +0.0 in index order acc = acc + v, weighted acc = fmaf(w_j, v, acc); mean: one correctly rounded division by the kept count;
 * an empty or all-padding bag gives +0.0; a 16-bit output is rounded once.  Un-pooled (pm_embedding_gather_f8_scaled): conv(v).  Both are
 * torch's CPU embedding_bag / embedding over the dequantised fp32 table, bit for bit (tests/f8s_rules.py, tests/test_f8s_host.py).
 * THE QUANTISER.  src: n_rows rows of dim columns of src_dtype (PM_F32 | PM_BF16 | PM_F16, widened exactly), src_row_stride elements
 * apart.  fmax = 1.75 * 2^k: k = 8 for e4m3fn (448), k = 15 for e5m2 (57344).
 *   pm_f8_row_exponents: amax = the maximum of |x_c| over the row's FINITE elements; with amax = m * 2^q, 1 <= m < 2, read from the fp32
 *     exponent and mantissa fields with integer arithmetic, e = q - k if m <= 1.75, else q - k + 1, clamped to [-64, 64]; a row with amax == 0
 *     or no finite element gets -64.  e is the smallest exponent at which the row does not overflow.  row_exp[r] = e.
 *   pm_rows_quantize_f8: s = clamp(E + e_r) with E = table_exp[0] (a device int32; NULL = 0) and e_r = row_exp[r] (NULL = 0);
 *     code = cast(x * 2^-s), cast = torch's CPU .to(float8 dtype): round to nearest even, NaN gives a NaN code, +-Inf gives +-Inf in e5m2 and
 *     NaN in e4m3fn, and so does a finite product that rounds past fmax (e4m3fn: above 464; e5m2: from 61440 on).  The product is exact
 *     wherever it matters (what it can lose lies below half the format's smallest subnormal), and a finite element never overflows at its
 *     row's exponent or a larger one: E_t = max_r e_r is the per-table exponent.  The sign and payload of NaN codes are not part of the rule.
 *     dst: uint8 [n_rows, dim], rows back to back.
 * Kernels: csrc/f8_quantize.hip (a lane group per row, 16-byte loads, amax an integer maximum reduced by a fixed butterfly, no atomics; the
 * hardware conversion v_cvt_pk_fp8_f32 / _bf8_f32 up to fmax, explicit selects above), csrc/embbag_fwd_f8s_kernel.inc (the FP8 kernel's
 * tiling; v = the hardware widening times 2^s built from its bits; row exponents are loaded where the tile's indices are staged and
 * compacted into LDS next to them) and csrc/embedding_gather_f8s.hip.  No atomics, no workspace, stream-ordered, 64-bit row addressing.
 * Refused on the host, before any HIP call: what pm_embbag_fwd_f8 / pm_embedding_gather_f8 refuse; table_exp and row_exp both NULL (that
 * request is the unscaled call's; PM_ERR_INVALID).  The quantiser: a src_dtype other than the three, an f8_dtype other than the two, a
 * negative n_rows (PM_ERR_INVALID); dim not a multiple of 16 or above 2048 (PM_ERR_UNSUPPORTED); src_row_stride below dim or not a whole
 * number of 16-byte pieces; then, unless n_rows == 0 (PM_OK without a launch), a NULL or not 16-byte aligned src or dst, a NULL row_exp
 * output (PM_ERR_INVALID).
 * pm_embbag_f8_scaled_plan(op, out_dtype, mean, row_exponents 0 / 1, out[12]): the geometry the pooled call WOULD use: pm_embbag_f8_plan's,
 * except that the row exponents' LDS bytes (one per index-tile entry) drop the output burst (stage_out = 0) where the tile would pass
 * 64 KiB with it -- explicit weighted tiles of 512 bags and more.  The un-pooled call's geometry is pm_embedding_gather_f8_plan's.
 * Left out: scales that are not powers of two, MX block scales, FP8 output, a format per table, max pooling, pruning, any backward.
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these six finds out at symbol resolution.
 */
int pm_f8_row_exponents(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, int64_t src_row_stride, int32_t f8_dtype, int8_t* row_exp,
                        pm_stream_t stream);
int pm_rows_quantize_f8(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, int64_t src_row_stride, int32_t f8_dtype,
                        const int32_t* table_exp, const int8_t* row_exp, void* dst, pm_stream_t stream);
int pm_embbag_fwd_f8_scaled(const pm_embbag_batch* op, const int64_t* padding_idx, int32_t mean, int32_t out_dtype, const int32_t* table_exp,
                            const int8_t* const* row_exp, void* out, pm_stream_t stream);
int pm_embbag_f8_scaled_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t mean, int32_t row_exponents, int32_t out[12]);
int pm_embedding_gather_f8_scaled(const pm_embbag_batch* op, int32_t out_dtype, const int32_t* table_exp, const int8_t* const* row_exp, void* out,
                                  int64_t out_row_stride, pm_stream_t stream);

/*
 * MIXED-FORMAT TABLES -- every table of ONE launch in its own stored format: what a serving model holds (the huge tables at 4 bits or
 * FP8, the mid-size ones at 8 bits, the small or sensitive ones at fp16 or fp32; fbgemm's IntNBitTableBatchedEmbeddingBagsCodegen takes one
 * SparseType per table).  table_formats: a DEVICE array of num_tables format codes --
 *   PM_F32, PM_BF16, PM_F16   [rows[t], dims[t]] elements of that type, rows back to back, tables[t] 16-byte aligned
 *   PM_F8E4M3, PM_F8E5M2      uint8 [rows[t], dims[t]] codes (FP8 TABLES), tables[t] 8-byte aligned
 *   PM_Q8, PM_Q4              uint8 [rows[t], row_bytes(dims[t], 8 | 4)] quantised rows (ROW-QUANTISED TABLES), tables[t] 4-byte aligned
 * -- and op->tables[t] points at that format's bytes exactly as the format's own call takes them.  table_exp: a DEVICE int32 array of
 * num_tables power-of-two table exponents E_t in [-64, 64] (SCALED FP8 TABLES), or NULL meaning all zero; read for FP8 tables only.
 * op->weight_dtype is not read.  The kernels read the formats like dims; the host never does.
 * THE RULE: NO NEW ARITHMETIC.  The columns of table t are bit for bit what that format's own call gives for the table alone:
 *   pooled (pm_embbag_fwd_anyfmt), per column from +0.0 in index order: fp32 / bf16 / fp16 acc = acc + f, weighted fmaf(w_j, f, acc)
 *     (pm_embbag_fwd_padded without padding, pm_embbag_fwd_out16); FP8 the same with f = dec(code) * 2^E_t (pm_embbag_fwd_f8 /
 *     pm_embbag_fwd_f8_scaled); PM_Q8 / PM_Q4 acc = fmaf(scale_r * w_j, code, acc + bias_r * w_j) (pm_embbag_fwd_qrows).  Sum pooling only.
 *   un-pooled (pm_embedding_gather_anyfmt), per position and column: conv(element) (pm_embedding_gather: same type in and out is a bit
 *     copy), conv(dec(code) * 2^E_t) (pm_embedding_gather_f8_scaled), conv(fmaf(scale_r, code, +0.0 + bias_r)) (pm_embedding_gather_qrows).
 *   out_dtype PM_F32, or PM_BF16 / PM_F16: the fp32 value rounded ONCE, in registers.  out is addressed in its own elements, like the
 *   per-table-format calls' (out_offsets / out_stride; the un-pooled call: row j at out + j * out_row_stride).
 *   A format code that is none of the seven is a defined result, not a fault: that table's output rows are +0.0 and none of its bytes is read.
 * Kernels: csrc/embbag_fwd_anyfmt_kernel.inc (the per-table-format kernel's tiles; the workgroup branches once per tile into its table's
 * format; a lane holds eight columns of a row whatever the format) and csrc/embedding_gather_anyfmt.hip (tiles of 256 positions; a lane
 * group branches on its row's format).  No atomics, no workspace, stream-ordered, 64-bit row addressing.
 * Refused on the host, before any HIP call: everything pm_embbag_fwd_qrows_mixed / pm_embedding_gather_qrows_mixed refuse (with a NULL
 * table_formats in a NULL table_bits' place: PM_ERR_INVALID; max_dim or min_dim not a multiple of 8, blocked layouts: PM_ERR_UNSUPPORTED;
 * an out_dtype other than the three: PM_ERR_INVALID); max_dim above 2048 (PM_ERR_UNSUPPORTED); a NULL or misaligned out (16 bytes fp32,
 * 8 bytes 16-bit), an out_row_stride below max_dim or not a multiple of 4 (PM_ERR_INVALID).  An empty request returns PM_OK without a launch.
 * pm_embbag_anyfmt_plan / pm_embedding_gather_anyfmt_plan: the geometry the two calls WOULD use (plan_anyfmt, plan_gather_anyfmt:
 * csrc/launch_plan.h), in pm_embbag_qrows_plan's / pm_embedding_gather_plan's order.  They need no device and no formats: the geometry is
 * a function of the request, out_dtype and the knobs.  The pooled kernel's rows in flight are a compile-time value per format (unroll is
 * reported as 0); the un-pooled kernel's are 4.
 * Left out: FP8 row exponents, pruning, mean and max pooling, padding rows, 2-bit rows, a lane-group width per format, any backward.
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these four finds out at symbol resolution.
 */
int pm_embbag_fwd_anyfmt(const pm_embbag_batch* op, const int32_t* table_formats, const int32_t* table_exp, int32_t out_dtype, void* out,
                         pm_stream_t stream);
int pm_embbag_anyfmt_plan(const pm_embbag_batch* op, int32_t out_dtype, int32_t out[12]);
int pm_embedding_gather_anyfmt(const pm_embbag_batch* op, const int32_t* table_formats, const int32_t* table_exp, int32_t out_dtype, void* out,
                               int64_t out_row_stride, pm_stream_t stream);
int pm_embedding_gather_anyfmt_plan(const pm_embbag_batch* op, int64_t out[8]);

/*
 * SEQUENCE GRADIENTS -- the batched backward of the un-pooled lookup above: the gradient of pm_embedding_gather's rows applied to all
 * num_tables tables by one sort and one apply.  The request is the one pm_embedding_gather takes: table t owns the lookup positions
 * [offsets[t * batch], offsets[(t + 1) * batch]), the last table ends at num_indices; the bags inside a table matter only for the
 * slice [bag_begin, bag_begin + bag_count), whose lookups are the contiguous stretch [offsets[t * batch + bag_begin],
 * offsets[t * batch + bag_begin + bag_count)) of every table.  out_offsets and out_stride of the request are not read.  The gradient
 * is fp32 and addressed by lookup POSITION: row j starts at grad + j * grad_row_stride (elements); columns from dims[t] to the stride
 * and rows of positions outside the slice are never read.
 * The rule: for table t and row r let J(t, r) be the positions j owned by t, inside the slice, with indices[j] == r, ascending.
 *   scatter-add / SGD   dst_t[r] accumulates alpha * grad[j] over J(t, r) in that order: what pm_embbag_bwd_sorted does for a row whose
 *                       bags are those positions;
 *   Adagrad             G = sum of grad[j] over J(t, r) from zero in that order, then the row-wise (elementwise = 0) or element-wise
 *                       (elementwise = 1) finish exactly as documented for pm_embbag_bwd_sorted_adagrad_ex / _adagrad_elem: weight
 *                       decay modes, stochastic rounding (keyed by seed, table, row, column pair), one rounding per 16-bit row.
 * Rows with at most 256 lookups are bit-identical to that sequential loop; hotter rows are summed as ordered chunk partials, as
 * everywhere in the sorted backward.  Deterministic, no atomics; every gradient row is read once.  By construction this is the sum
 * backward of the one-table request "one bag per lookup" (offsets = 0, 1, 2, ..; batch = its lookups) applied per table, without the
 * T sorts, applies and workspaces that route costs, and without a host read of the table borders; tests/sequence_grad_rules.py
 * restates it in numpy.
 * The sort forms every table's keys from the index array in its first radix pass (the path of a pooling-1 table) with the lookup
 * position as the value: no key-building pass, no bag-of array, never the hybrid route -- a sequence sort is always complete, and
 * the fused calls are simply sort then apply.  The apply is the sorted apply of pm_embbag_bwd_sorted*: same kernels, the position
 * in the place of the bag, no per-table gradient offset.
 *   pm_embseq_sort_indices        the key sort (needs the request only; may run on a side stream under the forward);
 *   pm_embseq_bwd_sorted          the scatter-add apply of a sorted request;   pm_embseq_bwd_fused          sort + apply;
 *   pm_embseq_bwd_sorted_adagrad  the Adagrad apply (state: device [T] of fp32 [rows_t] row-wise / [rows_t, dims_t] element-wise);
 *   pm_embseq_bwd_fused_adagrad   sort + apply.
 * Workspace: pm_embbag_bwd_sorted_workspace of the same request with per_sample_weights == NULL (no query of its own).  The workspace
 * remembers which kind of sort it holds: a pooled apply (pm_embbag_bwd_sorted*, pm_embbag_sparse_grad*) after a sequence sort, and a
 * sequence apply after a pooled sort, are PM_ERR_INVALID.  pm_embbag_sorted_pairs / pm_embbag_sort_status work after a sequence sort;
 * the values are then lookup positions.
 * Refused on the host, before any HIP call: everything pm_embbag_bwd_sorted refuses (more than 1024 tables, 2^32 or more lookups, bad
 * dtypes, a workspace that is NULL or too small, a missing or mismatching sort); per_sample_weights != NULL, a non-zero table_group /
 * grad_block_shift / grad_block_extra (PM_ERR_UNSUPPORTED); a NULL grad with num_indices > 0, a grad that is not 16-byte aligned,
 * grad_row_stride < max_dim or not a multiple of 4 (PM_ERR_INVALID); the Adagrad width limits of the pooled calls (max_dim > 256 fp32
 * / 512 16-bit: PM_ERR_UNSUPPORTED); elementwise not 0 or 1 (PM_ERR_INVALID).  num_indices == 0 or bag_count == 0 is PM_OK without a
 * launch.  Padding rows: pm_pad_rows_guard around the call, as for the pooled backwards.
 * Replaces aten::embedding_dense_backward per table (the backward of nn.Embedding, the un-pooled sibling of the module at
 * train/compute/pt/pytorch_emb.py:179) and the sequence (PoolingMode.NONE) backward of fbgemm's TBE with its fused optimizers
 * (split_table_batched_embeddings_ops.py:289-300,318-324).
 * The request struct is unchanged (sizeof 144) and the ABI version stays 8: a client that needs these calls finds out at symbol resolution.
 */
int pm_embseq_sort_indices(const pm_embbag_batch* op, int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream);
int pm_embseq_bwd_sorted(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* dst_tables,
                         int32_t dst_dtype, float alpha, int64_t max_rows, const void* workspace, int64_t workspace_bytes,
                         pm_stream_t stream);
int pm_embseq_bwd_fused(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* dst_tables,
                        int32_t dst_dtype, float alpha, int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream);
int pm_embseq_bwd_sorted_adagrad(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* tables,
                                 int32_t table_dtype, float* const* state, const pm_rowwise_adagrad* opt, int32_t elementwise,
                                 int64_t max_rows, const void* workspace, int64_t workspace_bytes, pm_stream_t stream);
int pm_embseq_bwd_fused_adagrad(const pm_embbag_batch* op, const float* grad, int64_t grad_row_stride, void* const* tables,
                                int32_t table_dtype, float* const* state, const pm_rowwise_adagrad* opt, int32_t elementwise,
                                int64_t max_rows, void* workspace, int64_t workspace_bytes, pm_stream_t stream);

/*
 * DLRM input redistribution on the device: regroup what the lengths / indices all-to-alls deliver
 * (train/comms/pt/dlrm.py:744-855) -- lengths [world][num_tables][batch] int64 and the indices
 * concatenated block by block in that (rank, table) order -- into the TBE request of the batched
 * kernel: out_indices table-major (within a table rank-major = global sample order) and out_offsets
 * [num_tables*world*batch + 1].  Replaces splitPerTable (dlrm.py:430-504: O(world*tables) Python
 * slicing / torch.cat with host syncs) with two launches and no host sync.
 * scratch: world*num_tables int64 (device).  out_indices must hold as many entries as `indices`.
 */
int pm_dlrm_regroup(const int64_t* lengths, const int64_t* indices, int32_t world_size, int32_t num_tables,
                    int64_t batch, int64_t* out_indices, int64_t* out_offsets, int64_t* scratch,
                    pm_stream_t stream);

/*
 * Validate a request on the device: every index in [0, rows[t]) and offsets
 * monotone within [0, num_indices]; plus what the kernels assume about the
 * per-table device arrays: rows[t] in [1, 2^31), dims[t] a multiple of 4 (fp32) /
 * 8 (16-bit) and <= max_dim, out_offsets[t] a multiple of 4 elements, table base
 * pointers 16-byte aligned.  Writes the number of violations to
 * *d_error_count (device int32, caller-zeroed is NOT required: the call zeroes
 * it first).  torch raises on such inputs (CPU) / device-asserts (GPU); the
 * forward/backward kernels themselves do not check.
 */
int pm_embbag_check(const pm_embbag_batch* op, int32_t* d_error_count, pm_stream_t stream);
/* The same with extra requirements.  PM_CHECK_UNIFORM_DIMS: every table has dims[t] == max_dim and out_offsets[t] is a
 * multiple of max_dim -- what pm_embbag_fwd_quantized assumes. */
enum { PM_CHECK_UNIFORM_DIMS = 1 };
int pm_embbag_check_ex(const pm_embbag_batch* op, int32_t flags, int32_t* d_error_count, pm_stream_t stream);

/*
 * Bounds check in front of the lookups: repair (or count) out-of-range indices and broken offsets ON THE DEVICE, stream-ordered, with
 * no host synchronisation -- so that the forward / backward kernels, which do not check, can be handed the arrays of a real input
 * pipeline.  Replaces fbgemm's bounds_check_indices kernel, which SplitTableBatchedEmbeddingBagsCodegen(bounds_check_mode=...) runs in
 * front of every forward (BoundsCheckMode FATAL | WARNING | IGNORE | NONE; the reference builds that module at
 * train/compute/python/workloads/pytorch/split_table_batched_embeddings_ops.py:279-300 and train/comms/pt/comms_utils.py:1994-2017).
 * pm_embbag_check above can only count, walks a bag per thread and is read back by its callers; it stays as the independent verdict.
 *
 * The rule, for T tables, B bags per table, N = num_indices lookups (bag_begin / bag_count are ignored: the whole request is sanitised):
 *   offsets   o = the first T * B entries;  o'[0] = 0,  o'[k] = max(o'[k - 1], clamp(o[k], 0, N))  -- a clamp followed by an inclusive
 *             prefix maximum, the monotone closure.  (fbgemm repairs bag by bag with a benign race between neighbouring bags; this
 *             rule has no race and is idempotent.)  A trailing entry offsets[T * B], present iff PM_BOUNDS_LAST_OFFSET is or'ed
 *             into `mode`, becomes N.
 *   table     lookup j in [0, N) belongs to the last table t with o'[t * B] <= j: every lookup to exactly one table, empty tables own none.
 *   indices   indices[j] outside [0, rows[t]) becomes 0 (fbgemm's replacement value).  per_sample_weights are not touched.
 *   report    d_report, device int64[4], OVERWRITTEN by every call (never accumulated), every field deterministic:
 *             [0] bad_indices       entries replaced                    [2] first_bad_index   smallest such position, or PM_BOUNDS_NONE
 *             [1] bad_offsets       offsets entries whose stored value  [3] first_bad_offset  smallest such position, or PM_BOUNDS_NONE
 *                                   changes (the trailing one included)
 *   writes    memory is written only where a value changes: a clean request stays bit-identical, its report is {0, 0, none, none}.
 * After a repairing call the request satisfies exactly what pm_embbag_check demands.  tests/bounds_rules.py restates the rule in numpy.
 *   mode      PM_BOUNDS_FATAL    dry run: count, write nothing to indices / offsets (the caller reads the report and raises)
 *             PM_BOUNDS_WARNING  repair in place and report
 *             PM_BOUNDS_IGNORE   repair in place, no report (d_report is not used and may be NULL)
 * d_scratch: pm_embbag_bounds_check_scratch(op) bytes of caller-owned device memory, 8-byte aligned (the scan's partial maxima, one per
 * PM_BOUNDS_OFFSETS_PER_WG offsets, and the T + 1 repaired table borders).  indices / offsets need only be aligned to their element.
 * Any number of tables, int32 / int64 (int32: num_indices < 2^31).  Four launches, none waits for another workgroup inside a launch.
 * Safe on arbitrary contents of both arrays: no offset is used as an address before it is clamped, indices are read inside [0, N).
 * Refused on the host, before any HIP call: what every entry point refuses, an unknown mode, a NULL d_report outside IGNORE, a
 * scratch that is NULL or too small.  batch == 0: PM_OK, nothing is launched and nothing written (the report neither: it would be
 * {0, 0, none, none}); num_indices == 0: the offsets are still repaired.
 * The ABI version is unchanged (8): a client that needs these two finds out at symbol resolution.
 */
#define PM_BOUNDS_FATAL   1   /* dry run: count, write nothing            */
#define PM_BOUNDS_WARNING 2   /* repair in place and report               */
#define PM_BOUNDS_IGNORE  3   /* repair in place, no report (may be NULL) */
#define PM_BOUNDS_LAST_OFFSET 0x100          /* or'ed into mode: offsets has T * B + 1 entries; the last one becomes num_indices */
#define PM_BOUNDS_NONE INT64_MAX             /* first_bad_* of a report without a finding */
#define PM_BOUNDS_OFFSETS_PER_WG 2048        /* offsets per workgroup of the scan: sizes the scratch */
int64_t pm_embbag_bounds_check_scratch(const pm_embbag_batch* op);            /* bytes of partials and borders */
int     pm_embbag_bounds_check(const pm_embbag_batch* op, int32_t mode, int64_t* d_report /*[4]*/,
                               void* d_scratch, int64_t scratch_bytes, pm_stream_t stream);

/*
 * Fill a buffer with counter-based pseudo-random values at HBM write speed:
 *   dist 0: uniform in [lo, hi)    (dlrm tables: U(-1/sqrt(n), 1/sqrt(n)),
 *                                   train/comms/pt/pytorch_dist_backend.py:923-934)
 *   dist 1: normal(mean=lo, std=hi) (nn.EmbeddingBag default N(0,1), pytorch_emb.py:179)
 * Element i depends only on (seed, i): reproducible for any launch geometry.
 * The values are the build's own stream, not torch's generator.
 */
int pm_fill_random(void* dst, int64_t count, int32_t dtype, int32_t dist, float lo, float hi,
                   uint64_t seed, pm_stream_t stream);

/*
 * Tuning knobs of the forward/backward launch (process-wide, mainly for bench
 * sweeps): unroll = rows in flight per lane group (1,2,3,4,6,8; 0 = default = 2),
 * bags_per_block (0 = default), xcd_affine = 1 maps table t to XCD t%8 when
 * num_tables%8==0 (keeps each table's hot rows in one L2), -1 = default.  nt_loads: forward -- any value > 0 = non-temporal
 * row loads; sorted backward -- cache policy of the destination-row accesses: 0 plain, 1 non-temporal, 2 system scope,
 * 3 plain load + agent-scope (sc1) store (the default at -1: the written row leaves the L2, the re-read gradient rows keep
 * it), 4 non-temporal load + sc1 store.  Speed only.
 */
int pm_set_tuning(int32_t unroll, int32_t bags_per_block, int32_t xcd_affine, int32_t nt_loads);

/*
 * stage_out = 1 (default; -1 = default, PARAM_AMD_FWD_STAGE=0 in the environment changes it): the forward collects a
 * tile's pooled rows in LDS and writes them in one burst when the tile is done (fixed-pooling requests whose tile of
 * rows fits 16 KB).  Results are bit-identical either way; it changes how the output write stream mixes with the row
 * reads (uniform indices: 0.69 -> 0.72-0.74 of the HBM peak).
 * flat_grid (ABI v7; -1 = default, PARAM_AMD_FLAT_COMPACT in the environment changes it): launch shape of the flat-walk forward
 * (short-bag and mixed-dim requests).  0 = one workgroup per (table, smallest tile): workgroups past their table's tile count
 * leave (round 3's form); 1 = one set of workgroups sized by the library, each walking the table-major tile order b, b + grid, ...
 * after establishing every table's tile count from the offsets (no workgroup is dispatched for a tile that does not exist);
 * N > 1 = exactly N workgroups (sweeps).
 * flat_target (ABI v7; -1 = default 256, PARAM_AMD_FLAT_TARGET in the environment changes it): lookups per tile the flat-walk forward
 * aims at when it sizes a table's tile from the table's average bag (sweeps).  Results are bit-identical in every setting.
 */
int pm_set_forward_tuning(int32_t stage_out, int32_t flat_grid, int32_t flat_target);

/*
 * Which launch geometry a forward entry point WOULD use for a request under the knobs as they stand now (pm_set_tuning,
 * pm_set_forward_tuning and the environment switches, which are read once per process): the status word of the forward.  Host only:
 * nothing is launched, no device memory is touched and no pointer of the request is dereferenced (they are only tested for NULL, as
 * the launching call tests them).  The request is validated exactly as the launching entry point validates it (the same error codes
 * and pm_last_error texts for what every entry point refuses; an entry point's OWN argument rules -- a NULL out, mean with weights --
 * are not part of the plan), and the plan is made by the very functions that call uses (param_amd/csrc/launch_plan.h).
 *   kind  PM_PLAN_BASE       the plain bag-count tiling of every backward, check, bounds, psw-grad, split, mean-grad and widen entry
 *         PM_PLAN_FORWARD    pm_embbag_fwd
 *         PM_PLAN_QUANTIZED  pm_embbag_fwd_quantized
 *         PM_PLAN_PADDED     pm_embbag_fwd_padded, pm_embbag_fwd_mean (4-byte output elements)
 *         PM_PLAN_PADDED16   pm_embbag_fwd_out16 (2-byte output elements)
 *   out   the twelve members of the plan in this order: tiles_per_table, bags_per_block, idx_cap, xcd_affine, nt_loads, ordered,
 *         stage_out, stage_bags, flat_bags, flat_target, flat_compact, unroll (0 where the launch has none).  flat_bags > 0: the
 *         flat-walk kernel; otherwise the tile kernel -- ordered, else staged where stage_out > 0, else plain.
 * pm_embedding_gather_plan is the same for pm_embedding_gather: vec, group_lanes, tile, col_passes, unroll, lds_borders,
 * xcd_contiguous, grid -- in this order.
 * For tests and tools (tests/test_gpu_plan_sweep.py asserts the plan of every launch it compares).  Thread-safe like every call; a
 * pm_set_* from another thread lands before or after the query.  Unknown kind / NULL out: PM_ERR_INVALID.
 * The ABI version is unchanged (8): a client that needs these two finds out at symbol resolution.
 */
#define PM_PLAN_BASE      0
#define PM_PLAN_FORWARD   1
#define PM_PLAN_QUANTIZED 2
#define PM_PLAN_PADDED    3
#define PM_PLAN_PADDED16  4
int pm_embbag_plan(const pm_embbag_batch* op, int32_t kind, int32_t out[12]);
int pm_embedding_gather_plan(const pm_embbag_batch* op, int64_t out[8]);

/*
 * Tuning knobs of the sorted backward (process-wide; -1 = default, which the environment can change:
 * PARAM_AMD_SORT=rocprim, PARAM_AMD_SORT_ORDER=row, PARAM_AMD_BWD_XCD=0, PARAM_AMD_BWD_PHASES=2):
 *   sort_impl   0 (default): the segmented sort of round 3 -- per-table segments, per-table pooling factors and (for batch
 *               slices) the pair count are established ON THE DEVICE from the offsets, so ragged / multi-hot / sliced /
 *               weighted requests take the same fast path as fixed-pooling ones and the fixed_pooling field of the request is
 *               not needed (nor trusted).  The product library has this sort and no other: requests of more than 1024
 *               tables are refused (PM_ERR_UNSUPPORTED: split the request), and sort_impl 1 / 2 are PM_ERR_UNSUPPORTED.
 *               ALTERNATES BUILD ONLY (libparam_amd_alt.so, `make alt`): 1: rocPRIM's radix_sort_pairs; 2: round 2's own LSD
 *               sort with host-side plans (pm_radix_sort_pairs; uses fixed_pooling; also serves more than 1024 tables) --
 *               measured alternatives and independent cross-checks for tests/ and tools/.
 *               order / max_phases below apply to 1 and 2 only; xcd_affine to all (sort_impl 0: XCD-contiguous tiles)
 *   order       1 (default): pairs ordered by (table, [bag phase,] row, position); 0: (row, table, position) -- only
 *               the row bits are sorted, the request being table-major already (one radix pass fewer, a slower apply)
 *   xcd_affine  1 (default; needs order 1 and a fixed-pooling request): the apply kernel's tiles of table t run on
 *               XCD t % 8, so one table's gradient rows are fetched into one L2
 *   max_phases  1 (default): every apply is one launch; 2: pm_embbag_sort_indices_ex(phases = 2) lays a
 *               fixed-pooling request out for the two-phase apply (kept as a measured alternative: it pays under
 *               uniform indices only).
 * Placement, pass count and phases change speed only; every setting gives the same result for rows looked up at
 * most 256 times (longer runs: same value up to fp32 association).
 * Settings are read when a request is SORTED; its apply follows what the sort recorded.
 */
int pm_set_backward_tuning(int32_t sort_impl, int32_t order, int32_t xcd_affine, int32_t max_phases);

/*
 * ABI v4.  How the segmented key sort (sort_impl 0) orders a table's pairs (-1 = default; PARAM_AMD_SORT_MODE in the
 * environment changes the default):
 *   0  LSD passes over all row bits: (table, row, position) order; 8 bits per pass, 9 where that saves a pass (17-18 and
 *      25-27 row bits).  ONE kernel per pass: the digit counts of all passes come from one read of the request, and a
 *      tile learns how many pairs precede it from its predecessors' published counts while the pass runs (look-back)
 *   3  the same order from three kernels per pass (histogram, scan, scatter) -- the cross-check of 0, and what requests
 *      of 2^30 lookups or more get
 *   1  ONE global partition pass on the low row digit, then every (table, digit) bucket is sorted by its remaining bits
 *      inside LDS: (table, row & 255, row >> 8, position) order -- equal rows adjacent and in request order, which is all
 *      the apply kernel needs; buckets stay balanced under any skew
 *   2  the same with the partition on the TOP row digit: ascending rows; a skewed head makes its bucket large
 * Speed only: every mode gives the same tables for rows looked up at most 256 times (longer runs: same value up to fp32
 * association, as documented at pm_embbag_bwd_sorted).
 */
int pm_set_sort_tuning(int32_t mode);

/*
 * ABI v5.  The hybrid backward (sort_impl 0, unweighted requests).  A table whose step touches (nearly) every row once -- the
 * uniform-index benchmark request: 98 % of its lookups -- does not need the sort: pm_embbag_sort_indices* classifies every
 * table on the device (pooling factor present, at most 2^18 lookups, lookups <= rows / 8, and a 2048-lookup sample that does
 * not repeat itself), builds a hashed "looked up twice" bitmap (a blocked Bloom filter, no false negatives) per such table in LDS, and hands only the flagged lookups
 * to the sort; pm_embbag_bwd_sorted* apply the others bag-major (one row read-modify-write per lookup, the bag's gradient slice
 * in registers: 2 x D x e instead of 3 x D x e bytes through the CU per lookup) and the flagged ones through the sorted apply.
 * Same results, bit for bit (a row applied bag-major has no other lookup; the flagged lookups keep their order).
 *   enable   -1 default (= 1); 0 off; 1 on for requests whose lookups divide evenly over the bags (every benchmark shape; ragged
 *            and per-table-pooling requests keep the sorted path): the tables are classified at every sort, on the device, from the request alone (so
 *            the same request always takes the same path: nothing is cached or carried from step to step); 2 every structurally
 *            eligible table goes hybrid whatever its indices look like (tests)                         PARAM_AMD_BWD_HYBRID
 *   lookback_spin_cap  polls before a look-back walk of the key sort stops waiting for a predecessor and counts that tile's digits
 *            itself; 0 = default (2^12).  Tests: 1 = the fallback runs wherever a predecessor is a moment late; 0xFFFFFFFF = it
 *            runs for every predecessor of every tile (nothing published is believed).
 * The path is offered by the FUSED entry points only (pm_embbag_bwd_fused*, ABI v6): its sort half runs the classification and
 * the bitmaps, the rest of the sort (of the flagged lookups, and of every lookup of the tables that did not qualify) runs in the
 * apply half, behind the bag-major kernel, which lists the flagged lookups as a by-product -- and reads the request's indices
 * again.  pm_embbag_sort_indices* on their own always sort completely (round 4 deferred there too: a caller that refilled its
 * index buffer between a side-stream sort and the apply would have had stale dup maps applied to new indices).
 * pm_embbag_sorted_pairs after a fused call shows the pairs that went through the sort; between a deferred sort and its apply
 * (which only the library can be) it returns PM_ERR_INVALID.
 */
int pm_set_hybrid_tuning(int32_t enable, int64_t lookback_spin_cap);

/*
 * ABI v7.  What the bag-major kernel of the hybrid backward leaves of a table -- the lookups its dup map flags, ~3 % of a
 * uniform-index request -- used to go through the whole key sort and the sorted apply: nine small dependent launches for a few
 * thousand pairs per table (7 % of the fp32 benchmark step, 15 % of the bf16 one).  mode 1 (the default at -1; PARAM_AMD_HYB_REST=0
 * in the environment changes it): ONE launch finishes them -- every hybrid table with at most 8192 flagged lookups is sorted
 * by row inside LDS (stable: a row's lookups stay in lookup order) and applied run by run, destination row read once and written
 * once, the arithmetic and order of the sorted apply (bit-identical to the sequential oracle for any run length); tables with
 * more left-overs, and everything when mode is 0, take the round-5 route (lists compacted, key sort, sorted apply).  Which
 * tables were finished is decided on the device from the request alone; the sort's launches follow either way and find no pairs
 * for the tables that were.  Read when the apply is issued.  Same results in either mode for rows looked up at most 256 times.
 */
int pm_set_hybrid_rest(int32_t mode);

/*
 * ABI v7.  The hybrid backward is offered only to requests whose bag-major launch fills the chip: the kernel tiles 128 bags, so a
 * request has num_tables * ceil(bag_count / 128) of its workgroups, and with few of them each workgroup pools its 128 bags' lookups
 * one bag after the other while most of the device idles (ONE 10 M-row table, batch 8192, pooling 20: 254 us against the sorted path's
 * 96).  tiles = the fewest such workgroups for which the path is offered: -1 = default (1024: measured break-even at 768 - 1024,
 * profiles/r06_few_tables_hybrid.jsonl), 0 = no lower bound (tests that drive the hybrid kernels with small requests).  A rule on the
 * request's sizes, read when a request is sorted; results are the same either way (rows looked up at most 256 times: bit for bit).
 */
int pm_set_hybrid_min_tiles(int32_t tiles);

/*
 * Forward with a row-wise QUANTISED output: the pooled vector of (bag b, table t) is written as one quantised row
 * (formats below, bitwidth 16 / 8 / 4 / 2) instead of max_dim floats -- what a quantised all-to-all of pooled embeddings
 * sends (--bitwidth of the reference's comms drivers), produced inside the lookup kernel's output burst so the fp32
 * pooled output never reaches HBM.  Same request as pm_embbag_fwd; the output keeps the fp32 layout with one row per
 * pooled vector: row index b * (out_stride / max_dim) + out_offsets[t] / max_dim, rows packed back to back
 * (pm_rows_quantized_bytes(rows, max_dim, bitwidth) bytes in all; pm_rows_dequantize restores them).  Contract: every
 * table has dims[t] == max_dim (a multiple of 8, <= 512) and out_offsets[t], out_stride are multiples of max_dim
 * (pm_embbag_check_ex(PM_CHECK_UNIFORM_DIMS) verifies the device arrays).  Served by the staged forward only: requests it
 * does not take (ragged bags, staging disabled) get PM_ERR_UNSUPPORTED -- run pm_embbag_fwd + pm_rows_quantize then.
 * Values equal pm_rows_quantize(pm_embbag_fwd(...)) bit for bit.
 */
int pm_embbag_fwd_quantized(const pm_embbag_batch* op, void* out, int32_t bitwidth, pm_stream_t stream);

/*
 * Row-wise quantisation of fp32 rows for the quantised all-to-all of pooled embeddings (the reference's --bitwidth
 * {2,4,8,16} / --quant-a2a-embedding-dim flags, train/comms/pt/comms_utils.py:1788-1806; downcast / restore around the
 * exchange, pytorch_dist_backend.py:48-76 and the unpublished all_to_allv_internal at :273).  src: n_rows x dim fp32,
 * row-major, dim a multiple of 8 in [8, 512].  Quantised row layouts (what torch's
 * quantized::embedding_bag_{byte,4bit,2bit}_prepack produce, i.e. fbgemm's fused row-wise formats):
 *   16: dim x fp16 (round to nearest even)                      2 * dim bytes
 *    8: dim x u8, fp32 scale, fp32 bias                         dim + 8 bytes
 *  4/2: dim * bits / 8 x u8 (low bits first), fp16 scale, bias  dim * bits / 8 + 4 bytes
 * pm_rows_dequantize restores x = fma(code, scale, bias).  Rows are packed back to back; the fp32 buffer is 16-byte aligned,
 * the quantised one aligned to the format's word (16 / 8 / 4 / 2 bytes for 16 / 8 / 4 / 2 bits: any whole number of rows into
 * an aligned buffer qualifies, so per-peer chunks of an exchange buffer can be produced in place).
 * pm_rows_quantized_bytes returns n_rows * row bytes (or a negative PM_ERR_* code).
 */
int64_t pm_rows_quantized_bytes(int64_t n_rows, int32_t dim, int32_t bitwidth);
int pm_rows_quantize(const float* src, int64_t n_rows, int32_t dim, int32_t bitwidth, void* dst, pm_stream_t stream);
int pm_rows_dequantize(const void* src, int64_t n_rows, int32_t dim, int32_t bitwidth, float* dst, pm_stream_t stream);

/*
 * ALTERNATES BUILD ONLY (round 2's sort: the product library sorts per-table segments with csrc/seg_sort.hip).
 * Stable LSD radix sort of (key, uint32 value) pairs by key bits [begin_bit, end_bit) -- the sort the sorted
 * backward ran on its (table,row) keys in round 2 (replaces the sort inside aten::_embedding_bag_dense_backward /
 * fbgemm's TBE backward at the call sites of pm_embbag_bwd_sorted).  key_bytes: 4 or 8.  The pairs start in
 * (keys_a, vals_a); 8-bit passes alternate between the a and b buffers and *result_in_b says where the sorted
 * pairs ended up.  n_max <= 2^32 - 1 elements; if d_count is not NULL the number of elements is read from that
 * device uint32 when the kernels run (clamped to n_max), so a producer kernel can decide it without a host
 * round trip.  segment_len > 0 (a multiple of 4096 dividing n_max, d_count NULL): the array is a sequence of segments of
 * that many pairs, each sorted on its own.  scratch: pm_radix_sort_scratch_bytes(n_max) bytes of device memory.
 */
#ifdef PM_ALTERNATES
int64_t pm_radix_sort_scratch_bytes(int64_t n_max);
int pm_radix_sort_pairs(void* keys_a, void* keys_b, uint32_t* vals_a, uint32_t* vals_b, int64_t n_max,
                        const uint32_t* d_count, int32_t key_bytes, int32_t begin_bit, int32_t end_bit,
                        int64_t segment_len, void* scratch, int64_t scratch_bytes, int32_t* result_in_b,
                        pm_stream_t stream);
#endif


#ifdef __cplusplus
}
#endif
#endif /* PARAM_AMD_H */
