/*
 * dfq_hip.h -- C ABI of libdfq_hip.so, the MI355X (gfx950) engine behind the DFQ calibration
 * hot path of jakc4103/DFQ.
 *
 * This is the drop-in boundary.  The reference is a pure-Python program whose calibration passes
 * are Python loops over channels issuing eager torch-CPU ops; it has no FFI of its own.  Each
 * entry point below replaces one such Python function body (cited as file:line of the reference)
 * and is what a maintainer of the reference would bind from Python with ctypes (see
 * INTEGRATION.md).  The Python package `dfq_amd` is exactly such a binding, keeping the
 * reference's call surface (`cross_layer_equalization`, `bias_correction`,
 * `transform_quant_layer`, `quantize`/`UniformQuantize`, ...).
 *
 * Conventions
 *   - every pointer marked "device" is a HIP device pointer to contiguous float32 (or the stated
 *     type) owned by the caller (in practice: torch-ROCm tensors);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are
 *     asynchronous on that stream unless the comment says "synchronises";
 *   - return value: 0 on success, a negative code on failure; dfq_last_error() gives the
 *     thread-local message.  Nothing aborts, nothing falls back to the CPU;
 *   - weights are OIHW contiguous ([O, I/g, kH, kW]; Linear is [O, I] with kH*kW = 1), float32,
 *     exactly the layout torch gives `nn.Conv2d.weight` / `nn.Linear.weight`.
 *
 * Arithmetic contract (DESIGN.md "Numerics"): all float32 operations are IEEE-754 correctly
 * rounded single operations (no FMA contraction, no fast-math, round-half-even for the
 * quantiser), scalars that the reference computes as Python doubles are computed in float64 on
 * the device.  Integer codes of the fake-quant round trip are bit-exact against the reference.
 */
#ifndef DFQ_HIP_H
#define DFQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFQ_HIP_VERSION 100 /* 0.1.0 */

/* error codes */
#define DFQ_OK 0
#define DFQ_ERR_ARG (-1)     /* invalid argument / unsupported geometry            */
#define DFQ_ERR_HIP (-2)     /* a HIP runtime call failed (message has the details) */
#define DFQ_ERR_STATE (-3)   /* object used in the wrong state                      */
#define DFQ_ERR_ABANDONED (-4) /* a workgroup gave up a bounded in-launch wait (DFQ_SPIN_LIMIT): the tensors the run
                                  rewrites are undefined unless the entry point says otherwise; see *_set_safe_mode */

int dfq_version(void);
const char* dfq_last_error(void);
/* number of visible HIP devices, or a negative error */
int dfq_device_count(void);
/* Destroyed plans park their small device blocks (descriptor tables, statistics arenas: <= DFQ_POOL_MB, default 512 MB per
 * process) in per-device free lists OUTSIDE the caller's allocator so that the next plan costs no hipMalloc.  This returns
 * them to the driver (hipFree) and reports how many bytes that was -- for a host that is about to need the memory itself
 * (torch's caching allocator cannot see these blocks).  No reference counterpart (the reference allocates nothing). */
long long dfq_pool_trim(void);

/* ------------------------------------------------------------------------------------------
 * Layer / relation tables shared by the plans
 * ---------------------------------------------------------------------------------------- */

/* One "targ layer" (Conv2d / Linear family; dfq.py:106, main_cls.py:137-145). */
typedef struct dfq_layer {
    float* weight;         /* device [out_ch, in_per_group, khkw]                       */
    float* bias;           /* device [out_ch] or NULL                                    */
    int32_t out_ch;        /* O                                                          */
    int32_t in_per_group;  /* I / groups                                                 */
    int32_t khkw;          /* kH * kW (1 for Linear)                                     */
    int32_t groups;        /* conv groups (1 for Linear); informational                  */
} dfq_layer;

/* One equalisation pair (utils/relation.py:5-27): layers[first] -> (BN, ReLU...) -> layers[second]. */
typedef struct dfq_relation {
    int32_t first;         /* index into the dfq_layer table                             */
    int32_t second;
    float* bn_weight;      /* device [O1]  BN proxy fake_weight (dfq.py:64-65) or NULL   */
    float* bn_bias;        /* device [O1]  BN proxy fake_bias   (dfq.py:67-68) or NULL   */
    float* scale_cum;      /* device [O1]  cumulative S of Relation.set_scale_vec
                              (relation.py:20-24); must hold 1.0f before the first sweep */
} dfq_relation;

/* ------------------------------------------------------------------------------------------
 * Cross-layer equalisation -- replaces dfq.py:28-75 (_layer_equalization) and the sweep loop
 * dfq.py:78-117 (cross_layer_equalization)
 * ---------------------------------------------------------------------------------------- */
typedef struct dfq_le_plan dfq_le_plan;   /* opaque */

typedef struct dfq_le_config {
    float s_lo, s_hi;          /* s_range (dfq.py:78 default [1e-8, 1e8]) rounded to float32  */
    float inv_lo, inv_hi;      /* float32(1.0 / s_range[k]) computed in double by the caller  */
    int32_t hi_gt_lo;          /* Python `s_range[1] > s_range[0]` (double compare)           */
    float eps;                 /* dfq.py:58 eps                                               */
    int32_t signed_range;      /* 0: max-min (dfq.py:54-55), 1: max|.| (dfq.py:50-51)         */
    double converge_thres;     /* dfq.py:83                                                   */
    int32_t converge_count;    /* dfq.py:83                                                   */
    int32_t max_sweeps;        /* extension: stop after this many sweeps; <0 = reference loop */
} dfq_le_config;

typedef struct dfq_le_result {
    int32_t sweeps;            /* sweeps executed                                             */
    int32_t stall_count;       /* `count` of dfq.py:110-115 at exit                           */
    double diff;               /* `diff` of dfq.py:110-115 at exit                            */
    double last_diff_tmp;      /* diff_tmp of the last sweep                                  */
} dfq_le_result;

/* NaN rule of the channel ranges (every dfq_le_* engine -- resident, streaming, free-running, lazy-scale -- and dfq_row_range /
 * dfq_col_range / dfq_le_pair): a NaN of any sign or payload, quiet or signalling, takes no part in a channel's min / max, the
 * rule of the quantisers' ranges ("Special values" below).  A channel with no non-NaN value gets S = s_hi and 1/S = inv_hi
 * (dfq_row_range / dfq_col_range report -inf for it: the range of the reductions' identities +inf, -inf).  Infinities and
 * denormals are ordinary values.  The NaN element itself stays NaN; the other elements of its row / column are scaled.
 * torch's max() / min() in dfq.py:50-55 PROPAGATE a NaN instead -- the channel's range is NaN and S = s_hi: a documented
 * divergence (one NaN weight does not cost a channel its scale); the oracle states both, channel_ranges(nan=...).
 * The |dW| mean of a tensor that holds a NaN is NaN in every sweep; the loop's comparisons are the reference's (a NaN never
 * resets `count`, the loop ends by converge_count). */
/* Builds the device-side work list: dependency levels of the relation list (Gauss-Seidel order of
 * dfq.py:85 is preserved: of two relations sharing a layer the later one's tiles wait, inside the sweep's
 * single launch, for the tiles of the earlier one they depend on), channel tiles, the per-layer
 * convergence-diff bookkeeping.  `layers` / `relations` are host arrays and
 * are copied.  Allocates a few small device buffers (statistics words, partial sums, descriptors);
 * the weights are processed where they are.  Synchronises. */
int dfq_le_plan_create(const dfq_layer* layers, int32_t n_layers,
                       const dfq_relation* relations, int32_t n_relations,
                       dfq_le_plan** out_plan);
/* Batched form: several independent networks in one plan.  `layer_net[l]` in [0, n_nets) is the network
 * of layer l; layers and relations must be listed network by network.  Every launch then covers all
 * networks (relation descriptors come from a table in global memory instead of the kernarg), each
 * network keeps its own loop state, so networks may converge after different sweep counts.  The sweep
 * loop of the batch runs until every network has stopped. */
int dfq_le_plan_create_batch(const dfq_layer* layers, int32_t n_layers, const int32_t* layer_net, int32_t n_nets,
                             const dfq_relation* relations, int32_t n_relations, dfq_le_plan** out_plan);
/* Replicated form: `n_nets` networks of ONE architecture whose tensors lie at the same offsets from a per-network base
 * address (a batch allocated as one arena with a fixed stride per network -- dfq_amd/arena.py).  `layers` / `relations`
 * describe the FIRST network (its own addresses, indices relative to it); network n's tensors are those addresses moved by
 * bases[n] - bases[0] bytes.  The host then builds one network's tables however large the batch is; everything else is as
 * dfq_le_plan_create_batch.  (Replaces, for a batch, the per-network graph walk of dfq.py:78-82.) */
int dfq_le_plan_create_replicated(const dfq_layer* layers, int32_t n_layers, const dfq_relation* relations, int32_t n_relations,
                                  const void* const* bases, int32_t n_nets, dfq_le_plan** out_plan);
void dfq_le_plan_destroy(dfq_le_plan* plan);
int32_t dfq_le_plan_nets(const dfq_le_plan* plan);

/* introspection (tests, bench byte accounting).  levels: equalisation launches per sweep -- 1 (the whole sweep is one
 * launch whose workgroups wait for the tiles they depend on) or, with DFQ_LE_MERGED=0 in the environment at plan
 * creation, one per dependency level; depth: number of dependency levels of the relation list */
/* 1 when the plan's networks are alike and laid out back to back (a batch from one template): the convergence launch then derives
 * a network's descriptor from its workgroup index instead of fetching it. */
int32_t dfq_le_plan_uniform(const dfq_le_plan* plan);
int32_t dfq_le_plan_levels(const dfq_le_plan* plan);
int32_t dfq_le_plan_depth(const dfq_le_plan* plan);
int64_t dfq_le_plan_paired_elements(const dfq_le_plan* plan);   /* sum over relations of n1+n2  */
/* per sweep: elements read AND written (8 B each) / elements only read by the statistics pass over
 * interior layers (4 B each); algorithmic bytes of a sweep = 8 * rw + 4 * ro */
int64_t dfq_le_plan_rw_elements(const dfq_le_plan* plan);
int64_t dfq_le_plan_ro_elements(const dfq_le_plan* plan);
/* Deferred stores of the streaming engine (DFQ_LE_DEFER = depth D at plan creation: 1 = off, 2 or 4; default 4 for batched
 * plans, 1 for a single network): a layer
 * that is only ever scaled one way is read every sweep but written every D-th one, the sweeps in between re-derive its
 * values from the stored ones and the remembered factors -- the same float32 operations, bit-identical results; every
 * enqueue call ends by bringing the weights up to date.  deferred_elements (a part of rw_elements) are those layers'
 * elements: bytes per sweep as executed, averaged over D sweeps = 8 * rw + 4 * ro - 4 * deferred * (D - 1) / D. */
int64_t dfq_le_plan_deferred_elements(const dfq_le_plan* plan);
int32_t dfq_le_plan_defer_depth(const dfq_le_plan* plan);
/* The store period S of those layers.  D above is the window after which their elements are READ at the latest; a plan that
 * runs lazy sweeps (below) stores them only every S-th sweep, S = DFQ_LE_STORE_DEPTH (4, 8 or 16; default 8 for a plan with
 * 8 Mi deferred elements or more -- the stores of a smaller one do not reach memory that a sweep waits for -- and D below
 * that), a multiple of D -- nobody reads the stores in between.  Its deferred elements then move 4 B per D sweeps read + 4 B per S sweeps written.
 * Every other plan has S = D.  A tile keeps one table of remembered factors per pending sweep in shared memory: a plan with a
 * deferred tile too wide for S - 1 of them gets the largest S that fits, which is what this returns. */
int32_t dfq_le_plan_store_depth(const dfq_le_plan* plan);
/* 1 when the plan runs lazy sweeps: the deferred layers are read only in their storing sweep and in sweeps whose verdict
 * needs their |dW| sums (batched plans with defer > 1; DFQ_LE_LAZY_DW=0 turns them off) */
int32_t dfq_le_plan_lazy(const dfq_le_plan* plan);
/* out3 = (lazy sweeps, uncertain verdicts resolved by the convergence launch, sweeps of the current run), summed over the
 * networks; the first two count since the plan was made.  Synchronises `stream`. */
int dfq_le_plan_lazy_stats(dfq_le_plan* plan, void* stream, int64_t* out3);
/* The convergence launch stages a network's |dW| partials in LDS, as many as the plan's largest network has (6144 at
 * most), and reads what exceeds the stage from memory.  For tests of that second path: lower the stage to `n_partials`
 * (>= 0; a value above the plan's own is ignored).  Returns the stage now in force. */
int32_t dfq_le_plan_set_ctl_stage(dfq_le_plan* plan, int32_t n_partials);
/* Free-running segments of the streaming engine (dfq_le_cf.hpp; DFQ_LE_CF=0 switches them off, DFQ_LE_CF_GROUP = G in
 * {2, 4, 8}, default 8 for a batched plan, 4 for a single network of >= 6 M paired elements, none for a smaller one: its
 * sweep is two launch latencies, and the lean launches only add to them).  A chain of relations whose every consumed range is closed-form -- a chain's first layer (rows * s,
 * dfq.py:62), depthwise layers in between, its last layer (columns * 1/s, dfq.py:73): max_i fl(w_i * s) == fl(max_i w_i * s)
 * -- has the scale factors of ALL its sweeps follow from a few scalars per channel (dfq.py:39-59 without reading a weight).
 * Its layers are not part of a sweep's launch: at the first sweep of every group of G sweeps ONE lean launch reads them, brings
 * them up to date, stores them and leaves sum |W - W_prev| (dfq.py:105-108) of the group's G sweeps; every enqueue call ends by
 * bringing them up to date like the deferred stores.  free_running_elements are NOT part of rw_elements: bytes per sweep as
 * executed = 8 * rw + 4 * ro - 4 * deferred * (D - 1) / D + 8 * free_running / G.  Bit-identical values and sweep counts. */
int64_t dfq_le_plan_free_running_elements(const dfq_le_plan* plan);
int32_t dfq_le_plan_free_running_group(const dfq_le_plan* plan);
/* 1: the lean launches run in the BACKGROUND (opt-in, DFQ_LE_CF_BG=1: bit-identical, measured no faster): a lean launch
 * looks ahead two groups -- it leaves sum |W - W_prev| of the NEXT group's sweeps, this group's were left by the launch before --
 * so its deadline is a whole group away and it runs on a second, low-priority stream of the plan next to the group's sweep
 * launches, in the launch boundaries of the caller's stream (which waits for it where the sums are read and at every
 * write-back; an enqueue call never returns with one in flight).  Same values, same sums, same sweep counts. */
int32_t dfq_le_plan_lean_background(const dfq_le_plan* plan);
int32_t dfq_le_plan_lean_tiles(const dfq_le_plan* plan);
/* Tuning aid: tile `tile` of the lean launch.  out3 = { kind (0 / 1: rows * s in 16-byte vectors / floats, 2: one thread per
 * row, 3 / 4: columns * 1/s, 5: one thread per row of a chain's last layer), rows, floats per row }. */
int dfq_le_plan_lean_info(const dfq_le_plan* plan, int32_t tile, int64_t* out3);
/* the same two counts for one launch level; returns the number of relations in it */
int32_t dfq_le_plan_level_launches(const dfq_le_plan* plan, int32_t level, int64_t* rw_elems,
                                   int64_t* ro_elems, int32_t* n_workgroups);
/* launch geometry of launch `level` of a sweep: grid_x = its workgroups (all of them work), grid_y = 1 */
int dfq_le_plan_level_grid(const dfq_le_plan* plan, int32_t level, int32_t* grid_x, int32_t* grid_y);

/* Single networks whose paired layers fit the chip's LDS run the WHOLE loop as one persistent, cooperative launch (every
 * workgroup keeps one 32 KB tile of one layer in its LDS for all sweeps; dfq_le_resident.hip): the number of its workgroups,
 * or 0 when the plan uses the streaming one-launch-per-sweep kernel (batched plans, networks too large for the
 * chip's resident workgroups, DFQ_LE_RESIDENT=0) -- then dfq_le_plan_resident_reason says why.  Results are
 * bit-identical either way. */
int32_t dfq_le_plan_resident_tiles(const dfq_le_plan* plan);
const char* dfq_le_plan_resident_reason(const dfq_le_plan* plan);
/* The persistent launch stores ALL OR NOTHING (round 5): its tiles write their result back only once every tile has finished
 * the loop.  If a workgroup abandons an in-launch wait (DFQ_SPIN_LIMIT), no tile stores, the caller's tensors are exactly as
 * they were passed, and dfq_le_run repeats the pass on one launch per level -- which waits for nothing inside a launch --
 * instead of returning DFQ_ERR_STATE; the plan then stays on that engine (dfq_le_plan_resident_tiles becomes 0,
 * dfq_le_plan_resident_reason says why).  Number of runs of this plan that were repeated that way (0 in normal operation).
 * The reference's loop (dfq.py:78-117) has no counterpart: it cannot fail half way. */
int32_t dfq_le_plan_degraded(const dfq_le_plan* plan);
/* Launches of the streaming engine in which workgroups wait for other workgroups (the one-launch sweep): 1 if a run of this
 * plan can end with DFQ_ERR_ABANDONED after having rewritten tensors (the persistent launch stores all or nothing and is not
 * counted).  dfq_le_plan_set_safe_mode: from now on the plan runs one launch per dependency level -- no workgroup waits for
 * another one, nothing can be abandoned (parity-tested since round 1, slower) -- and never the persistent launch.  The Python
 * binding's LEPlan.run() uses the pair to repeat an abandoned pass from a device-side snapshot of the tensors (dfq_amd/dfq.py). */
int32_t dfq_le_plan_has_waits(const dfq_le_plan* plan);
int dfq_le_plan_set_safe_mode(dfq_le_plan* plan);
/* The resident launch applies every sweep to its LDS tiles AT ONCE and learns only later (from a reducer workgroup, off every
 * dependency chain) whether dfq.py:105-115 let that sweep happen: a tile may be up to `spec` sweeps past the stopping point
 * and then restores the newest of its checkpoints and replays the logged per-channel factors (bit-identical: the same two
 * rounded multiplications per element and sweep).  Statistics of the LAST launch (tests, tuning; synchronises `stream`):
 * out5 = {tiles that rolled back, sweeps undone in total, most sweeps undone by one tile, speculation depth (DFQ_RES_SPEC,
 * default 2), sweeps between checkpoints (DFQ_RES_CKPT, default 8)}. */
int dfq_le_resident_stats(dfq_le_plan* plan, void* stream, int64_t* out5);
/* Streaming plans built with DFQ_LE_PERSIST=1 (an experiment, off by default): persistent workgroups of a sweep launch
 * (each walks its share of the sweep's tiles with the next tile's data in flight); 0 when a sweep launches one workgroup
 * per tile or the plan is resident.  DFQ_LE_SWEEP_WGS caps the number. */
int32_t dfq_le_plan_sweep_workgroups(const dfq_le_plan* plan);
/* Tuning aid for the persistent launch: restart, run `n_sweeps` sweeps with per-workgroup phase stamps (100 MHz wall
 * clock): out[(tile * 6 + sweep) * 12 + point] for the first 6 sweeps; points: 0 sweep start, 1 s_A solved, 2 row
 * statistics published, 3 s_B solved, 4 new values + statistics published, 5 ticket taken, 6 decision seen; point 7
 * of sweep 0 = layer << 32 | tile rows << 16 | tile columns.  `capacity` >= dfq_le_resident_trace_words().
 * Modifies the weights like an ordinary run.  Synchronises. */
int64_t dfq_le_resident_trace_words(const dfq_le_plan* plan);
int dfq_le_resident_trace(dfq_le_plan* plan, const dfq_le_config* cfg, int32_t n_sweeps, void* stream, int64_t* out,
                          int64_t capacity);

/* Enqueue exactly `n_sweeps` sweeps plus their convergence bookkeeping on `stream`; never
 * synchronises.  The device-side loop state decides whether a sweep still executes (after the
 * reference's exit condition fires the remaining launches are no-ops).  `restart` != 0 resets the
 * loop state (diff = 10, count = 0) first. */
int dfq_le_enqueue(dfq_le_plan* plan, const dfq_le_config* cfg, int32_t n_sweeps, int32_t restart,
                   void* stream);
/* Copy the loop state back (synchronises `stream`).  dfq_le_query: network 0, *done = every network of the
 * plan has stopped; dfq_le_query_all: `out` has dfq_le_plan_nets() entries. */
int dfq_le_query(dfq_le_plan* plan, void* stream, dfq_le_result* out, int32_t* done);
int dfq_le_query_all(dfq_le_plan* plan, void* stream, dfq_le_result* out, int32_t* all_done);
/* A stopping rule that spans several plans -- the sharded pass (dfq_amd/sharded.py), where dfq.py:105-108's sum runs over the
 * layers of ALL ranks.  dfq_le_set_diff_log (single-network plans; synchronises): from now on the plan also leaves diff_tmp of
 * sweep j (sweeps since the last restart) in log_device[j], j < capacity; capacity 0 switches it off.  The caller runs a chunk of
 * sweeps with the plan's own exit test disabled (converge_thres < 0), all-reduces the chunk's log entries in ONE collective and
 * hands the sums to dfq_le_shared_verdict: the (diff, count) state machine of dfq.py:110-115 over `n` values on the device,
 * ext4_device = { diff, count, sweeps, done } as float64 (initialise to { 10, 0, 0, 0 }: dfq.py:81-82); once `done`, the plan's
 * loop state (plan may be NULL for a rank that owns nothing) is stopped so that sweeps enqueued behind it are no-ops.
 * Asynchronous; nothing is read back. */
int dfq_le_set_diff_log(dfq_le_plan* plan, double* log_device, int32_t capacity);
int dfq_le_shared_verdict(dfq_le_plan* plan, const double* reduced_device, int32_t n, double* ext4_device, double converge_thres,
                          int32_t converge_count, int32_t max_sweeps, void* stream);
/* The whole dfq.py:83-115 loop: enqueue in chunks, poll, stop when the device says so.
 * Synchronises. */
int dfq_le_run(dfq_le_plan* plan, const dfq_le_config* cfg, void* stream, dfq_le_result* out);
/* Measurement aid (bench.py roofline): like dfq_le_enqueue(restart=1) for `n_sweeps` sweeps, but every
 * launch is bracketed by a pair of HIP events recorded on `stream`.  level_ms[l] receives the summed
 * duration of the launches of level l (array of dfq_le_plan_levels() doubles), *control_ms the summed
 * duration of the convergence kernel, *n_level_launches the number of level launches timed,
 * *empty_bracket_ms what a pair of event records measures with nothing between them (to subtract),
 * *lean_ms / *n_lean_launches (either may be NULL) the summed duration and number of the lean launches of the
 * free-running layers (one per group of sweeps).  Synchronises. */
int dfq_le_profile(dfq_le_plan* plan, const dfq_le_config* cfg, int32_t n_sweeps, void* stream,
                   double* level_ms, double* control_ms, int32_t* n_level_launches,
                   double* empty_bracket_ms, double* lean_ms, int32_t* n_lean_launches);

/* Tuning aid: run two sweeps and return the shader-clock stamps (s_memtime) that thread 0 of
 * workgroup `block` (= blockIdx.y * grid_x + blockIdx.x) of launch `launch` took at the phase boundaries of its tile during the second
 * sweep: [0] entry, [1] descriptor+state loaded, [2] data loads issued, [3] scales solved,
 * [4] barrier passed, [5] elements stored, [6] stats published, [7] partial written.  Synchronises;
 * modifies the weights like two ordinary sweeps. */
int dfq_le_trace(dfq_le_plan* plan, const dfq_le_config* cfg, int32_t launch, int32_t block, void* stream,
                 int64_t* stamps16);

/* Tuning aid: what workgroup `block` of launch `launch` does.  out8 = { kind (0/1/2: row tile of 16-byte vectors /
 * scalars / one thread per row; 3/4/5: the same for column tiles), rows, columns, elements read and written,
 * elements only read, 1 if it waits for another relation inside the launch, 1 if it publishes statistics,
 * index of its relation in the level-sorted table }. */
int dfq_le_plan_block_info(const dfq_le_plan* plan, int32_t launch, int32_t block, int64_t* out8);

/* Tuning aid: run three sweeps and return, for EVERY workgroup b of launch `launch` during the third one,
 * out[3b] = entry and out[3b+1] = exit time (100 MHz wall clock; 0 for a workgroup that had no tile) and
 * out[3b+2] = XCC_ID << 32 | HW_ID of the compute unit it ran on.  `capacity_blocks` >= grid_x * grid_y of
 * dfq_le_plan_level_grid.  Synchronises; modifies the weights like three ordinary sweeps. */
int dfq_le_trace_blocks(dfq_le_plan* plan, const dfq_le_config* cfg, int32_t launch, void* stream, int64_t* out,
                        int64_t capacity_blocks);

/* ------------------------------------------------------------------------------------------
 * Tensor primitives -- utils/quantize.py:23-76 (UniformQuantize.forward), :102-119 (QuantMeasure)
 * ---------------------------------------------------------------------------------------- */

/* Special values in the reductions of this section, of dfq_quant_plan_* and dfq_row_quant_plan_*, and of the batch plans
 * dfq_batch_quant_plan, dfq_batch_error_plan, dfq_batch_clip_plan and dfq_batch_table_plan (one implementation: csrc/dfq_range.hpp): a
 * NaN of any payload, quiet or signalling, is SKIPPED; a tensor, sample or segment of nothing but NaN gives (NaN, NaN);
 * infinities and denormals are ordinary values; min / max are selections, so every result is exact and only the sign of a
 * zero result is free.  The same on the 16-byte path and on the scalar path (unaligned pointers, tails).  torch's min() /
 * max() would PROPAGATE the NaN instead: a documented divergence -- one NaN weight does not cost a layer its range.
 * tests/test_quant_adversarial.py holds the cases. */

/* out2[0] = min(x), out2[1] = max(x) as float32 (device), NaN skipped (above).  `scratch2` is a device uint32[2] that
 * the call zeroes and uses for the order-preserving atomic reduction. */
int dfq_tensor_minmax(const float* x, int64_t n, float* out2, uint32_t* scratch2, void* stream);

/* Fake-quant round trip y = rint(clip((x + (-min)) / scale, qmin, qmax)) * scale + min
 * (quantize.py:70-74), five separately rounded float32 operations.
 *   range_mode 0: min/max are host doubles (the reference's `float(...)` call sites); the scale
 *                 recipe of quantize.py:49-66 runs in float64.
 *   range_mode 1: min/max are read from the device float32 pair `minmax_dev` and the recipe runs
 *                 in float64 on the device (same values as mode 0 without a host round trip).
 *   range_mode 2: min/max from `minmax_dev`, recipe entirely in float32 -- the `min_value=None`
 *                 tensor path of quantize.py:24-35 (bias fake-quant call sites :198,:226,:311,:335).
 * `codes` (device int32[n]) receives the integer codes when not NULL.  x == y (in place) is allowed.
 * A NaN input gives a NaN output (its integer code is unspecified); an infinite input clamps to qmin / qmax.
 * DFQ_ERR_ARG (and dfq_last_error) for num_bits outside [1, 30] and for symmetric with num_bits == 1: qmax = 2^0 - 1 = 0
 * and the scale would be max / 0 -- the reference raises ZeroDivisionError there (quantize.py:56).  The same refusal in
 * dfq_quant_plan_create, dfq_quant_error and, for per-tensor tensors, dfq_batch_quant_plan_create. */
int dfq_fake_quant(const float* x, float* y, int64_t n, int32_t num_bits, int32_t symmetric,
                   int32_t range_mode, double min_value, double max_value,
                   const float* minmax_dev, int32_t* codes, void* stream);

/* QuantMeasure statistics (quantize.py:103-107): out2[0] = mean_n(min over chw of x[n]),
 * out2[1] = mean_n(max over chw of x[n]).  If `running2` (device float[2] = {running_min,
 * running_max}) is not NULL it is updated in place: running_min = min(running_min, out2[0]),
 * running_max = max(running_max, out2[1]).  `scratch` is a device uint32[2*n_samples].
 * NaN is skipped inside a sample (above); a sample of nothing but NaN has extrema (NaN, NaN), which makes BOTH means NaN and
 * leaves running2 as it was (Python min(r, nan) keeps r). */
int dfq_sample_minmax_mean(const float* x, int32_t n_samples, int64_t sample_len, float* out2,
                           float* running2, uint32_t* scratch, void* stream);
/* QuantMeasure.forward with update_stat (utils/quantize.py:102-119; improve_dfq.py:280-297 runs it for every activation of
 * every distilled batch) in TWO launches: the per-sample extrema, then one kernel in which every workgroup forms their mean
 * (as dfq_sample_minmax_mean does), folds it into running2 = (running_min, running_max) (quantize.py:106-107) and quantises
 * x -> y with the folded range (float64 recipe, asymmetric).  scratch: 4 * n_samples uint32 owned by the caller, ZERO before the
 * first call; parity alternates 0, 1, 0, ... from call to call on the same scratch (each call clears the half the next one
 * accumulates into).  Same numbers as dfq_sample_minmax_mean(running2) + dfq_fake_quant(range_mode 1), special values
 * included: NaN skipped inside a sample, NaN means leave running2 alone and x is quantised with the range it had.  Always
 * asymmetric, so num_bits == 1 is allowed. */
int dfq_quant_measure(const float* x, float* y, int32_t n_samples, int64_t sample_len, int32_t num_bits, float* running2,
                      uint32_t* scratch, int32_t parity, void* stream);
/* The same in ONE launch (round 4 experiment, OPT-IN through DFQ_QM_FUSED=1 in the Python layer: measured slower than the two
 * launches on the MI355X -- 189 vs 148 us on a [64, 96, 112, 112] activation, 3.73 vs 1.71 ms of QuantMeasure time per distilled
 * batch of config 5 -- the grid-wide meeting costs more than the launch boundary it replaces): a
 * grid of persistent workgroups -- dfq_quant_measure_fused_grid(n_samples, sample_len) of them, sized to be co-resident --
 * takes the per-sample extrema, waits (bounded) until the whole grid has arrived, then every workgroup forms the mean, folds
 * the running range and quantises its share of x, which up to the size of the chip's caches has not left them.  Bit-identical
 * to dfq_quant_measure.  scratch: 4 * n_samples + 4 uint32, 8-byte aligned, ZERO before the first call (the last four words
 * hold a monotonic arrival counter and an error word); parity alternates as above; `arrivals_before` = the sum of
 * dfq_quant_measure_fused_grid over all earlier calls on this scratch.  dfq_quant_measure_fused_status synchronises and
 * returns DFQ_ERR_STATE if a workgroup of an earlier call gave up waiting (DFQ_SPIN_LIMIT). */
int32_t dfq_quant_measure_fused_grid(int32_t n_samples, int64_t sample_len);
int dfq_quant_measure_fused(const float* x, float* y, int32_t n_samples, int64_t sample_len, int32_t num_bits, float* running2,
                            uint32_t* scratch, int32_t parity, int64_t arrivals_before, void* stream);
int dfq_quant_measure_fused_status(const uint32_t* scratch, int32_t n_samples, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-layer weight quantisation -- utils/layer_transform.py:279-296 (quantize_targ_layer)
 * ---------------------------------------------------------------------------------------- */
typedef struct dfq_quant_plan dfq_quant_plan;

/* One plan over a table of tensors ("segments"): per-tensor min/max in one launch, fake-quant of
 * all tensors in a second launch.  The min/max of a segment skips NaN (see "Special values" above; a segment of nothing
 * but NaN reports (NaN, NaN) and is quantised to NaN); segments do not see each other.  create: DFQ_ERR_ARG (and
 * dfq_last_error) for a null or empty segment, num_bits outside [1, 30], symmetric with num_bits == 1 (qmax = 0). */
typedef struct dfq_segment {
    float* data;            /* device                                                    */
    int64_t n;
    int32_t num_bits;       /* per segment (weights 8, biases 16 in main_cls.py:181)      */
    int32_t symmetric;
    int32_t* codes;         /* device int32[n] or NULL                                    */
} dfq_segment;

int dfq_quant_plan_create(const dfq_segment* segs, int32_t n_segs, dfq_quant_plan** out_plan);
void dfq_quant_plan_destroy(dfq_quant_plan* plan);
/* min/max of every segment -> quantise every segment in place (range_mode 1 recipe). */
int dfq_quant_plan_run(dfq_quant_plan* plan, void* stream);
/* min/max of every segment only (no quantisation): what a calibration-table writer needs
 * (convert_ncnn.py:183-190) */
int dfq_quant_plan_measure(dfq_quant_plan* plan, void* stream);
/* device float32[2*n_segs] min/max pairs of the last run / measure (valid after the stream reaches it) */
const float* dfq_quant_plan_minmax(const dfq_quant_plan* plan);

/* Per-output-channel weight quantisation (extension; the per-channel counterpart of quantize_targ_layer,
 * utils/layer_transform.py:279-296): every segment is a [rows, row_len] matrix whose row r is fake-quantised in
 * place with its OWN (min, max) -- utils/quantize.py:23-76 UniformQuantize, Python-float min/max recipe, as
 * dfq_fake_quant_rows.  A per-tensor segment (a bias) is a segment of one row.  ONE launch for all segments. */
typedef struct dfq_row_quant_plan dfq_row_quant_plan;
typedef struct dfq_row_segment {
    float* data;            /* device [rows, row_len], quantised in place                 */
    int64_t rows;
    int64_t row_len;
    int32_t num_bits;       /* 2..16                                                      */
    int32_t symmetric;
    int32_t* codes;         /* device int32[rows * row_len] or NULL                       */
    float* ranges;          /* device float32[rows, 2]: (min, max) each row used, or NULL */
} dfq_row_segment;

int dfq_row_quant_plan_create(const dfq_row_segment* segs, int32_t n_segs, dfq_row_quant_plan** out_plan);
void dfq_row_quant_plan_destroy(dfq_row_quant_plan* plan);
int dfq_row_quant_plan_run(dfq_row_quant_plan* plan, void* stream);

/* Weight quantisation of a whole batch of networks of one architecture (extension; quantize_targ_layer,
 * utils/layer_transform.py:279-296, for every network of a batch at once).  The tensor table describes the FIRST of
 * `n_nets` networks; network n's copy of a tensor lies bases[n] - bases[0] bytes further (as the replicated LE / BC
 * plans).  A per-row tensor quantises row r with its own (min, max) -- bit-identical to dfq_row_quant_plan_run; a
 * per-tensor one uses the tensor's (min, max) -- bit-identical to dfq_quant_plan_run.  Integer codes go to a
 * caller-owned block [n_nets, code_stride] of `code_bytes`-wide elements: 4 = int32, 1 = uint8 (asymmetric tensors,
 * 0 .. 2^b-1) / int8 (symmetric, -2^(b-1) .. 2^(b-1)-1), only for tensors of at most 8 bits.  Ranges go to a caller-owned
 * float32 block [n_nets, range_stride]: (min, max) per row of a per-row tensor, one pair for a per-tensor one.
 * Offsets are in elements of their block, -1 = none.  No workgroup waits for another: per-row tensors and per-tensor
 * tensors of at most dfq_batch_quant_register_elements() elements take one launch, longer per-tensor ones a min/max
 * launch in front of it (folding every chunk into one pair of slots per tensor and network, cleared first).  NaN in a
 * range: the rule of Special values above.  Every
 * tensor of network 0 must lie inside network 0's slot: nothing here can check that.  create: DFQ_ERR_ARG (and dfq_last_error) for empty / null arguments, bit widths outside
 * [2, 16] (per row) or [1, 30] (per tensor), a symmetric per-tensor tensor of 1 bit (qmax = 0), 1-byte codes of more than 8 bits, offsets that overflow their stride.
 * Synchronises (create only); run is asynchronous on `stream`. */
typedef struct dfq_batch_quant_plan dfq_batch_quant_plan;
typedef struct dfq_batch_quant_tensor {
    float* data;            /* device, inside network 0's slot; [rows, row_len], quantised in place      */
    int64_t rows;
    int64_t row_len;
    int32_t num_bits;
    int32_t symmetric;
    int32_t per_row;        /* 1: every row its own range; 0: one range for the tensor                   */
    int32_t pad;
    int64_t code_offset;    /* elements into a network's code block, or -1                               */
    int64_t range_offset;   /* floats into a network's range block, or -1                                */
} dfq_batch_quant_tensor;

int dfq_batch_quant_plan_create(const dfq_batch_quant_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                void* codes, int32_t code_bytes, int64_t code_stride, float* ranges, int64_t range_stride,
                                dfq_batch_quant_plan** out_plan);
void dfq_batch_quant_plan_destroy(dfq_batch_quant_plan* plan);
int dfq_batch_quant_plan_run(dfq_batch_quant_plan* plan, void* stream);
/* launches per run (1 or 2) */
int32_t dfq_batch_quant_plan_launches(const dfq_batch_quant_plan* plan);
/* longest row (or per-tensor tensor) kept in registers between its min/max and its quantisation; longer ones are read twice */
int64_t dfq_batch_quant_register_elements(void);

/* Adaptive rounding (extension; SQuant, ICLR 2022 -- nothing of it is in the reference): round to nearest, then flip the few
 * roundings that cost least, so that the rounding errors of every kernel and of every output row sum to at most half a quantum
 * (nearest rounding leaves a row sum of about sqrt(n / 12) quanta, which is what bias correction then has to repair).
 * DEFINITION.  A tensor is [rows, row_len] with row_len = G * K; K = `kernel_len` (kH * kW; 1 for Linear and 1x1 convolutions)
 * and G kernels per row.  The range is the quantisers': the row's own (min, max) or a given pair, NaN skipped (Special values
 * above); QParams by the float64 recipe of dfq_fake_quant (range_mode 0), asymmetric or symmetric, num_bits in [2, 16].  The
 * flip stages work per kernel and per row whichever range is used.  Per element, in the float32 operations of the quantiser:
 *   t  = clamp((w + neg_min) / scale, qmin, qmax);  c0 = rintf(t);  p = c0 - t (exact);  P = llrint((double)p * 2^30),
 *   an integer in [-2^29, 2^29].  ONE = 2^30, HALF = 2^29.  All sums of P are integer sums: a result depends on no order.
 *   stage K (K > 1), per kernel: e = sum P; n = (|e| + HALF) >> 30; s = sign(e); of the elements with s P > 0, ordered by s P
 *            descending, then by index ascending, the first n are flipped: c = c0 - s, P <- P - s ONE.  There are always n
 *            of them, and afterwards |sum P| <= HALF.
 *   stage C, per row: e_j = kernel j's sum after stage K (K = 1: a kernel is one element); E = sum e_j; N = (|E| + HALF) >> 30;
 *            S = sign(E); of the kernels with S e_j > 0, ordered by S e_j descending, then by j ascending, each of the first N
 *            moves one element: c <- c - S, P <- P - S ONE, the element with the largest S P > 0 AFTER stage K, the lowest
 *            index on a tie (an element flipped in stage K may be flipped back).  Such an element always exists.
 *   afterwards |sum_row P| <= HALF, |sum_kernel P| <= ONE, |c - c0| <= 1, qmin <= c <= qmax (an element with p = 0 -- the
 *            row's extremes, every clamped element -- is never a candidate).  Stored: c * scale + min_value, the two float32
 *            roundings of the quantiser.
 *   fallback: a row with an element whose t is NaN, or whose QParams hold a non-finite value, gets no flips and is stored bit
 *            for bit as dfq_fake_quant_rows / dfq_batch_quant_plan_run store it; its stats are (0, 0).  The code of a NaN is 0.
 * dfq_squant_rows: one tensor.  mins / maxs: device [rows], or both NULL for each row's own range (as dfq_fake_quant_rows).
 * codes: device int32 [rows, row_len] or NULL.  stats: device int64 [rows, 2] or NULL = (sum_row P after stage C, number of
 * elements whose code differs from c0).  x == y is allowed.  One launch; rows of up to 256 elements share a wave (4 to 64
 * lanes each), longer ones get a wave, rows above 1536 a workgroup.  DFQ_ERR_ARG (and dfq_last_error) for null or empty
 * arguments, only one of mins / maxs, num_bits outside [2, 16], row_len % kernel_len != 0, row_len above
 * dfq_squant_max_row_len(). */
int dfq_squant_rows(const float* x, float* y, int64_t rows, int64_t row_len, int64_t kernel_len, const float* mins, const float* maxs,
                    int32_t num_bits, int32_t symmetric, int32_t* codes, int64_t* stats, void* stream);
/* longest row the adaptive rounding takes (16384) */
int64_t dfq_squant_max_row_len(void);

/* The same for the weights of a whole batch of networks of one architecture, in the shape of dfq_batch_quant_plan: the table
 * describes the FIRST of `n_nets` networks, network n's copy of a tensor lies bases[n] - bases[0] bytes further.  per_row: each
 * row its own range; else the tensor's (min, max), found by a launch in front (cleared range words, as dfq_batch_quant_plan).
 * Codes go to a caller-owned block [n_nets, code_stride] of `code_bytes`-wide elements (4 = int32; 1 = uint8 / int8, at most 8
 * bits), ranges to a float32 block [n_nets, range_stride] (a pair per row, or one per tensor), stats to an int64 block
 * [n_nets, stats_stride] (a pair per row).  Offsets are in elements of their block, -1 = none.  create: DFQ_ERR_ARG (and
 * dfq_last_error) for null or empty arguments, num_bits outside [2, 16], row_len % kernel_len != 0, row_len above
 * dfq_squant_max_row_len(), 1-byte codes of more than 8 bits, offsets past their stride.  Synchronises (create only); run is
 * asynchronous on `stream`. */
typedef struct dfq_batch_squant_plan dfq_batch_squant_plan;
typedef struct dfq_batch_squant_tensor {
    float* data;            /* device, inside network 0's slot; [rows, row_len], quantised in place      */
    int64_t rows;
    int64_t row_len;
    int32_t num_bits;
    int32_t symmetric;
    int32_t per_row;
    int32_t pad;
    int64_t code_offset;
    int64_t range_offset;
    int64_t kernel_len;     /* K; row_len is a multiple of it                                            */
    int64_t stats_offset;   /* int64 elements into a network's stats block, or -1                        */
} dfq_batch_squant_tensor;

int dfq_batch_squant_plan_create(const dfq_batch_squant_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                 void* codes, int32_t code_bytes, int64_t code_stride, float* ranges, int64_t range_stride,
                                 int64_t* stats, int64_t stats_stride, dfq_batch_squant_plan** out_plan);
int dfq_batch_squant_plan_run(dfq_batch_squant_plan* plan, void* stream);
void dfq_batch_squant_plan_destroy(dfq_batch_squant_plan* plan);
/* kernel launches per run (1 to 3: per-tensor ranges, rows of a wave or less, rows of a workgroup) */
int32_t dfq_batch_squant_plan_launches(const dfq_batch_squant_plan* plan);
/* A width per (network, tensor), read on the device (extension; the widths a dfq_batch_mixed_plan allocation leaves in its
 * `bits` block, so that nothing goes to the host between the allocation and the adaptive rounding).
 * DEFINITION.  With `widths` set -- int32 on the device, [n_nets, width_stride] -- every later run treats tensor t of network n
 * exactly as "Adaptive rounding" above defines it with num_bits = widths[n * width_stride + width_index[t]]: the QParams and so
 * t, P, stage K, stage C, the fallback, the stored weight, the code and the stats are, bit for bit, what a plan created with
 * that num_bits for that tensor stores.  Ranges do not depend on the width: the range launch of the per-tensor tensors and the
 * range block are as without widths.  `width_index` is host memory, [n_tensors] of the plan, read by this call only.
 *   a width that is no width -- outside [2, 16], or above 8 for a tensor that writes one-byte codes -- makes the items of that
 *            (network, tensor) write nothing: no weight, code, range or stats word of it is touched, and status[n] becomes 2
 *            (a plain store of the constant; several items may store it).  Every other tensor of that network and every other
 *            network is processed as usual.  Every run clears `status` -- int32 on the device, [n_nets] -- first, with a memset
 *            on the stream, so status[n] == 0 after a run says that network n was rounded whole.
 * The widths are read by the row launches of a run, so whatever writes them (dfq_batch_mixed_plan_run) goes onto the same
 * stream in front.  The row launches are then other instantiations of the same kernels; dfq_batch_squant_plan_launches is
 * unchanged (the memset is no launch).  NULL `widths`, the default: the table's widths again, every result bit for bit that of
 * a plan that never had widths; `status` is then not touched.  A call with `widths` set synchronises (it replaces the index
 * a run may still read); a NULL call changes host fields only and does not.
 * DFQ_ERR_ARG for a null plan, widths without width_index or status, an index that is negative or >= width_stride. */
int dfq_batch_squant_plan_set_widths(dfq_batch_squant_plan* plan,
                                     const int32_t* widths /* device int32 [n_nets, width_stride], or NULL */, int64_t width_stride,
                                     const int32_t* width_index /* host [n_tensors], read here only */,
                                     int32_t* status /* device int32 [n_nets] */);

/* Bias absorption and weight clipping of a whole batch of networks of one architecture (extension; bias_absorption,
 * dfq.py:121-164, followed by clip_weight, dfq.py:167-170, for every network of a batch at once).  The tables describe the
 * FIRST of `n_nets` networks; network n's copy of a tensor lies bases[n] - bases[0] bytes further.  `relations` lists, in
 * the order bias_absorption would walk them, the relations WITH a ReLU between their layers (the caller skips the others,
 * dfq.py:131-139); one run does for each, in every network, what dfq_bias_absorb does:
 *   c = max(0, bn_bias - n_sigma * bn_weight);  b1 -= c;  bn_bias -= c;  b2[o] += sum_i (sum_k W2[o,i,k]) * c[g*I2/g + i]
 * with c taken ONCE, before anything is shifted, and kept in the caller's float32 block [n_nets, shift_stride] at
 * `shift_offset` (o1 floats).  A bias that is b2 of one relation and b1 of another receives its two updates in the order
 * of the list.  Then every tensor of `clips` becomes clamp(x, lo, hi) as dfq_clamp leaves it (NaN, infinities and signed
 * zeros included); a weight that is both summed and clipped is read once, summed unclipped, and written only where the
 * clamp changed it.  Every result is bit-identical to the dfq_bias_absorb / dfq_clamp calls on that network alone.
 * Two launches (the shifts, then one pass over the weights), none with absorbed relations = one, nothing to do = none; no
 * workgroup waits for another.  create: DFQ_ERR_ARG (and dfq_last_error) for null / empty arguments, a geometry
 * dfq_bias_absorb refuses, a kernel of more than 3136 taps, a non-finite n_sigma, lo > hi or NaN, a shift vector outside
 * its stride or overlapping another, two relations sharing a first or a second layer, a clip tensor listed twice or
 * sized unlike the relation's weight it is.  Every tensor of network 0 must lie inside network 0's slot: nothing here can
 * check that.  Synchronises (create only); run is asynchronous on `stream`. */
typedef struct dfq_batch_absorb_plan dfq_batch_absorb_plan;
typedef struct dfq_batch_absorb_relation {
    const float* w2;        /* second layer's weight [o2, in_per_group, khkw], network 0                   */
    float* b1;              /* first layer's bias [o1]                                                     */
    float* b2;              /* second layer's bias [o2]                                                    */
    const float* bn_weight; /* gamma~ [o1]                                                                 */
    float* bn_bias;         /* beta~ [o1]                                                                  */
    int32_t o2;
    int32_t in_per_group;
    int32_t khkw;
    int32_t o1;
    int64_t shift_offset;   /* floats into a network's shift block                                         */
} dfq_batch_absorb_relation;
typedef struct dfq_batch_absorb_clip {
    float* data;            /* clamped in place, network 0                                                 */
    int64_t n;
} dfq_batch_absorb_clip;

int dfq_batch_absorb_plan_create(const dfq_batch_absorb_relation* relations, int32_t n_relations, const dfq_batch_absorb_clip* clips,
                                 int32_t n_clips, const void* const* bases, int32_t n_nets, float n_sigma, float lo, float hi,
                                 float* shifts, int64_t shift_stride, dfq_batch_absorb_plan** out_plan);
void dfq_batch_absorb_plan_destroy(dfq_batch_absorb_plan* plan);
int dfq_batch_absorb_plan_run(dfq_batch_absorb_plan* plan, void* stream);
/* launches per run (0, 1 or 2) */
int32_t dfq_batch_absorb_plan_launches(const dfq_batch_absorb_plan* plan);
/* weights per network that are read for a row sum, and weights that are only clipped (either pointer may be null) */
int dfq_batch_absorb_plan_elements(const dfq_batch_absorb_plan* plan, int64_t* absorbed, int64_t* clip_only);

/* BatchNorm folding of a whole batch of networks of one architecture (extension; merge_batchnorm,
 * utils/layer_transform.py:246-272, main_cls.py:149, for every network of a batch at once).  `pairs` lists the (layer,
 * BatchNorm) pairs of the FIRST of `n_nets` networks; network n's copy of a tensor lies bases[n] - bases[0] bytes further.
 * One run does for each pair, in every network, what dfq_fold_batchnorm does (utils/layer_transform.py:246-272):
 *   sd = sqrtf(var + eps);  k = gamma / sd;  w[o, :] *= k[o];  b = b * k + (beta - (gamma * mean) / sd);
 *   fake_weight = |gamma|;  fake_bias = beta;  gamma = var = 1;  beta = mean = 0
 * every operation rounded on its own, in that order: bit-identical to dfq_fold_batchnorm on that network alone.  Two
 * launches: one pass over the weights that only reads gamma / var (flat pieces of a tensor, 16-byte accesses, any row
 * length), then a thread per channel; no atomics, no workgroup waits for another.  create: DFQ_ERR_ARG (and dfq_last_error)
 * for a null or empty table, a null tensor, out_ch <= 0 or row_len <= 0, a weight that is not 16-byte aligned, two pairs
 * sharing a weight, a bias or a BatchNorm vector, null bases, networks that are not 16-byte aligned to network 0.  Every
 * tensor of network 0 must lie inside network 0's slot: nothing here can check that.  A second run folds the identity
 * BatchNorms the first one left (the proxies become 1 and 0): the caller runs a plan once.  Synchronises (create only); run
 * is asynchronous on `stream`. */
typedef struct dfq_batch_fold_plan dfq_batch_fold_plan;
typedef struct dfq_batch_fold_pair { /* addresses in network 0 */
    float* w;               /* the layer's weight [out_ch, row_len], scaled in place (layer_transform.py:246-251)   */
    float* b;               /* its bias [out_ch] (:253-261)                                                        */
    float* gamma;           /* bn.weight [out_ch]; 1 afterwards (:268)                                             */
    float* beta;            /* bn.bias; 0 afterwards (:270)                                                        */
    float* mean;            /* bn.running_mean; 0 afterwards (:271)                                                */
    float* var;             /* bn.running_var; 1 afterwards (:269)                                                 */
    float* fake_weight;     /* |gamma| (:264)                                                                      */
    float* fake_bias;       /* beta (:265)                                                                         */
    int64_t row_len;
    int32_t out_ch;
    float eps;              /* bn.eps (:249)                                                                       */
} dfq_batch_fold_pair;

int dfq_batch_fold_plan_create(const dfq_batch_fold_pair* pairs, int32_t n_pairs, const void* const* bases, int32_t n_nets,
                               dfq_batch_fold_plan** out_plan);
int dfq_batch_fold_plan_run(dfq_batch_fold_plan* plan, void* stream);
void dfq_batch_fold_plan_destroy(dfq_batch_fold_plan* plan);
/* launches per run (2) */
int32_t dfq_batch_fold_plan_launches(const dfq_batch_fold_plan* plan);
/* folded weights per network (each is read once and written once: 8 B) */
int64_t dfq_batch_fold_plan_elements(const dfq_batch_fold_plan* plan);

/* Weight statistics of the ncnn int8 calibration table for a whole batch of networks of one architecture (extension; the
 * weight block of model_int8_tensor.table, convert_ncnn.py:178-201, for every network of a batch at once).  `tensors` lists
 * the weights of the FIRST of `n_nets` networks; network n's copy of a tensor lies bases[n] - bases[0] bytes further.  One
 * run reads every weight of every network once, writes no weight, and fills the caller's float32 block [n_nets, stride]:
 * per tensor (min, max) at `range_offset` -- the pair dfq_quant_plan_measure gives, the `mi, ma` of convert_ncnn.py:186-187
 * -- and per output row max|w| at `row_offset` (`rows` floats) -- what dfq_row_range(signed) gives: the per-channel form of
 * the same scale.  Both come from the same read; they are selections, so every value is exact (the sign of a zero is +
 * for a row's maximum and either for a tensor's bound), infinities included.  NaN is skipped (the rule of Special values
 * above); a tensor of nothing but NaN gives (NaN, NaN), a row of nothing but NaN gives 0.  A run clears the WHOLE block, then two launches: one pass over the
 * weights (flat pieces of a tensor, 16-byte loads, any row length; partial results are merged with atomicMax of
 * order-preserving words, which is deterministic for min / max), then a thread per tensor and network that turns the merged
 * words into floats; no workgroup waits for another.  Offsets are in floats from a network's part of the block; the slots of
 * different tensors must not overlap (not checked).  create: DFQ_ERR_ARG (and dfq_last_error) for a null or empty table, a
 * null weight, rows <= 0 or row_len <= 0, a weight that is not 16-byte aligned, a null block, stride <= 0, an offset outside
 * the stride, null bases, networks that are not 16-byte aligned to network 0.  Every tensor of network 0 must lie inside
 * network 0's slot: nothing here can check that.  Synchronises (create only); run is asynchronous on `stream`. */
typedef struct dfq_batch_table_plan dfq_batch_table_plan;
typedef struct dfq_batch_table_tensor { /* addresses in network 0 */
    const float* data;      /* the layer's weight [rows, row_len], only read (convert_ncnn.py:186-187)              */
    int64_t rows;           /* output channels: the scale is written once per row (:194)                            */
    int64_t row_len;
    int64_t range_offset;   /* floats into a network's part of the block: (min, max)                                */
    int64_t row_offset;     /* floats into a network's part of the block: max|w| of every row                       */
} dfq_batch_table_tensor;

int dfq_batch_table_plan_create(const dfq_batch_table_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                float* out, int64_t stride, dfq_batch_table_plan** out_plan);
int dfq_batch_table_plan_run(dfq_batch_table_plan* plan, void* stream);
void dfq_batch_table_plan_destroy(dfq_batch_table_plan* plan);
/* kernel launches per run (2); the clear of the block in front of them is a memset */
int32_t dfq_batch_table_plan_launches(const dfq_batch_table_plan* plan);

/* Weight quantisation error of a whole batch of networks of one architecture (extension; the batch form of
 * _quantize_error(param, num_bits, reduction, signed), dfq.py:8-25, for every weight of every network and up to four
 * quantiser configurations from the same reads).  `tensors` lists the weights of the FIRST of `n_nets` networks; network
 * n's copy of a tensor lies bases[n] - bases[0] bytes further.  A run reads every weight twice (ranges, then errors),
 * writes no weight, and writes, for network n and tensor t, 1 + 3 * n_configs float64 values from
 * out + n * stride + out_offset on: sum w^2, then for every configuration sum e, sum |e|, sum e^2 with
 * e = fake_quant(w; qparams(min, max, num_bits, symmetric)) - w in float32 (dfq.py:15), (min, max) being the tensor's pair,
 * or the row's for a `per_row` configuration: bit for bit the value dfq_batch_quant_plan_run would store, minus w.  A
 * constant tensor or row takes the max(scale, 1e-8) branch of the recipe.  Every sum is a float64 accumulation of float32
 * terms (e^2 and w^2 formed in float64, exactly) in an order of the plan's own that is fixed: two runs are bit-identical,
 * network n's values do not depend on n_nets or on n's place in the batch, no floating-point atomic is used.  NaN is
 * skipped by the ranges (the rule of Special values above); a tensor holding NaN gets NaN sums, nothing else does.  Nothing else in
 * the block is touched.  A clear of the plan's own range words, then three launches (ranges, errors, a fold of the
 * pieces' sums in rising order); no workgroup waits for another.  Offsets are in doubles from a network's part of the
 * block; the slots of different tensors must not overlap (not checked).  create: DFQ_ERR_ARG (and dfq_last_error) for null
 * or empty tables, n_configs outside 1..4, num_bits outside [2, 16] (per row) or [1, 30] (per tensor), symmetric with 1 bit,
 * a null weight, rows <= 0 or row_len <= 0, a weight that is not 16-byte aligned, a null block, stride <= 0, an offset
 * outside the stride, null bases, networks that are not 16-byte aligned to network 0.  Every tensor of network 0 must lie
 * inside network 0's slot: nothing here can check that.  Synchronises (create only); run is asynchronous on `stream`. */
typedef struct dfq_batch_error_plan dfq_batch_error_plan;
typedef struct dfq_batch_error_tensor { /* addresses in network 0 */
    const float* data;      /* the layer's weight [rows, row_len], only read                                        */
    int64_t rows;
    int64_t row_len;
    int64_t out_offset;     /* doubles into a network's part of the block: 1 + 3 * n_configs sums                   */
} dfq_batch_error_tensor;
typedef struct dfq_batch_error_config {
    int32_t num_bits;
    int32_t symmetric;      /* the signed recipe                                                                     */
    int32_t per_row;        /* ranges per output row instead of per tensor                                           */
    int32_t pad;
} dfq_batch_error_config;

int dfq_batch_error_plan_create(const dfq_batch_error_tensor* tensors, int32_t n_tensors, const dfq_batch_error_config* configs,
                                int32_t n_configs, const void* const* bases, int32_t n_nets, double* out, int64_t stride,
                                dfq_batch_error_plan** out_plan);
int dfq_batch_error_plan_run(dfq_batch_error_plan* plan, void* stream);
void dfq_batch_error_plan_destroy(dfq_batch_error_plan* plan);
/* kernel launches per run (3); the clear of the range words in front of them is a memset */
int32_t dfq_batch_error_plan_launches(const dfq_batch_error_plan* plan);

/* MSE-optimal weight clipping of a whole batch of networks of one architecture (extension; the reference's clip_weight,
 * dfq.py:167-170, with a searched bound per unit in place of one constant for the network).  `tensors` lists the weights of
 * the FIRST of `n_nets` networks; network n's copy of a tensor lies bases[n] - bases[0] bytes further.
 * DEFINITION.  A UNIT is a tensor, or an output row with `per_row`.  It has (mn, mx) by the rule of Special values above: NaN
 * skipped, nothing but NaN gives (NaN, NaN).  With K = `candidates` in [1, 64] and `alpha_min` in (0, 1]:
 *   shrink factor   in float64, a_k = 1 for K = 1, else 1 - k (1 - alpha_min) / (K - 1), k = 0 .. K - 1
 *   fixed point     z = min(max(0, mn), mx): the ends shrink toward zero, or toward the end nearest zero of a one-signed
 *                   unit, so a range is never inverted
 *   candidate ends  l_k = (float)(z + a_k (mn - z)), h_k = (float)(z + a_k (mx - z)) in float64; candidate 0 is (mn, mx)
 *   error           err_k = sum_i e_i^2, e_i = fake_quant(c_i; qparams(l_k, h_k, num_bits, symmetric)) - w_i in float32 with
 *                   c_i = w_i clamped to (l_k, h_k) as `apply` clamps it, the recipe of dfq_fake_quant in range_mode 0: bit
 *                   for bit what dfq_batch_quant_plan_run stores for the clamped unit, whose range is then (l_k, h_k), minus
 *                   the weight as it is -- so err_k* is the error of what `apply` and the quantiser leave, and it is never
 *                   above err_0, that of min/max quantisation.  Under the asymmetric recipe the quantiser saturates at
 *                   (l_k, h_k) itself and the clamp inside e_i changes no bit (unless the scale sits at its floor of 1e-8);
 *                   under the symmetric one the grid spans +-max(|l_k|, |h_k|) and only the clamp cuts at the shorter end.
 *                   The square and the sum are float64; the order of the sum depends on
 *                   the tensor's shape alone and no floating-point atomic is used: two runs are bit-identical, and network
 *                   n's values do not depend on n_nets or on n's place in the batch
 *   choice          k* = argmin err_k, the smallest k on a tie: the comparison is err < best starting from candidate 0, so a
 *                   unit whose errors are NaN or all infinite (a NaN or an infinity among its weights, nothing but NaN)
 *                   keeps k* = 0
 *   apply           w <- w < l ? l : (w > h ? h : w) with (l, h) of k*; NaN and -0.0 pass through; where k* = 0 nothing is
 *                   stored, elsewhere only what the clamp changed.  The unit's own (min, max) is then (l, h), which every
 *                   quantiser of this library takes from the weights -- none of them has to know about the search.
 * Outputs per unit, in blocks of the caller [n_nets][stride] units, a tensor's first unit at `out_offset`, its rows behind
 * it: `ranges` float32 [.., 2] = (l, h) of k*; `chosen` int32 = k*; `errors` float64 [.., K] = every err_k (null: not
 * written).  Nothing else in the blocks is touched.  Units of at most dfq_batch_quant_register_elements() elements stay in
 * registers from the min/max through all candidates to the clamp (one launch, one read, at most one write); longer rows get
 * a looping wave; longer per-tensor tensors three launches over flat pieces (ranges, errors per piece, fold and choice) and
 * a fourth with `apply`.  No workgroup waits for another.
 * create: DFQ_ERR_ARG (and dfq_last_error) for null or empty tables, a null configuration, num_bits outside [2, 16],
 * candidates outside [1, 64], alpha_min not in (0, 1] (NaN included), a weight that is null or not 16-byte aligned, rows <= 0
 * or row_len <= 0, a null `ranges` or `chosen` block, stride <= 0, an offset outside the stride, null bases, networks that
 * are not 16-byte aligned to network 0.  Every tensor of network 0 must lie inside network 0's slot: nothing here can check
 * that.  Synchronises (create only); run is asynchronous on `stream`. */
typedef struct dfq_batch_clip_plan dfq_batch_clip_plan;
typedef struct dfq_batch_clip_tensor { /* addresses in network 0 */
    float* data;            /* the layer's weight [rows, row_len], clamped in place with `apply`                     */
    int64_t rows;
    int64_t row_len;
    int64_t out_offset;     /* units into a network's part of the blocks: 1 unit, or `rows` with per_row              */
} dfq_batch_clip_tensor;
typedef struct dfq_batch_clip_config {
    int32_t num_bits;
    int32_t symmetric;      /* the signed recipe                                                                     */
    int32_t per_row;        /* a unit is an output row instead of a tensor                                           */
    int32_t candidates;     /* K                                                                                     */
    double alpha_min;
    int32_t apply;          /* clamp the weights to the chosen ranges                                                */
    int32_t pad;
} dfq_batch_clip_config;

int dfq_batch_clip_plan_create(const dfq_batch_clip_tensor* tensors, int32_t n_tensors, const dfq_batch_clip_config* config,
                               const void* const* bases, int32_t n_nets, float* ranges, int32_t* chosen, double* errors, int64_t stride,
                               dfq_batch_clip_plan** out_plan);
int dfq_batch_clip_plan_run(dfq_batch_clip_plan* plan, void* stream);
void dfq_batch_clip_plan_destroy(dfq_batch_clip_plan* plan);
/* kernel launches per run: 1 for the units in registers and the long rows, 3 (4 with apply) for the flat pieces */
int32_t dfq_batch_clip_plan_launches(const dfq_batch_clip_plan* plan);

/* Mixed-precision weight quantisation of a whole batch of networks of one architecture (extension; a bit width per layer
 * under a size budget, the allocation ZeroQ is known for, joined to the quantiser of dfq_batch_quant_plan).  `tensors` lists
 * the weights of the FIRST of `n_nets` networks; network n's copy of a tensor lies bases[n] - bases[0] bytes further.  One run
 * finds the ranges, the error of every tensor at every candidate width, a width per tensor and network, and quantises every
 * tensor at its own width; nothing goes to the host in between.
 * DEFINITION.  Candidate widths b_0 < b_1 < ... < b_{B-1}, integers in [2, 16], 2 <= B <= 8.  `symmetric` and `per_row`, one
 * pair for the plan, mean what they mean in dfq_batch_quant_tensor.  Tensor t is [rows, row_len], n_t = rows * row_len, with a
 * `sensitivity` s_t (float64, finite, >= 0) and `fixed_bits` (0: free; else one of the candidates, and the tensor is pinned).
 *   errors      E[n][t][j] = sum of e^2 over tensor t of network n, e = fake_quant(w; qparams(min, max, b_j, symmetric)) - w
 *               in float32, (min, max) the tensor's pair, or the row's with per_row: term for term the third sum
 *               dfq_batch_error_plan_run reports for the configuration (b_j, symmetric, per_row).  The square and the sum are
 *               float64; the order of the sum is the plan's own and depends on the tensor's shape alone, no floating-point
 *               atomic is used: two runs are bit-identical, and network n's values do not depend on n_nets or on n's place in
 *               the batch.  NaN is skipped by the ranges (Special values above); a tensor holding NaN gets NaN errors, nothing
 *               else does.  All B errors of a weight come from one read of it.
 *   allocation  per network.  Cost c[t][j] = s_t * E[n][t][j], one float64 multiplication.  Every free tensor starts at
 *               j_t = 0, a pinned one at its width's index; used = sum_t n_t * b_{j_t} in int64.  The NEXT STEP of a free
 *               tensor standing at j: for k > j, g(j, k) = (c[t][j] - c[t][k]) / (double)(n_t * (b_k - b_j)), one float64
 *               subtraction and one float64 division; only k with g > 0 count (false for NaN); the step is the k of greatest
 *               g, the largest such k on a tie; if no k counts the tensor is finished.  LOOP: among the unfinished free
 *               tensors take the one whose next step has the greatest g, the lowest t on a tie; d = n_t * (b_k - b_j); if
 *               used + d > budget_bits the allocation ENDS (it does not skip to a cheaper step); otherwise j_t = k,
 *               used += d, and the loop goes on.  This is the greedy walk along every tensor's lower convex hull in order of
 *               error removed per bit; its result is a Lagrangian minimiser: no allocation of at most `used` bits has a
 *               smaller sum_t c[t][j_t], up to the rounding of g.  If the start alone exceeds the budget the start is the
 *               allocation, and used > budget_bits tells the caller.  At most T (B - 1) steps.
 *   quantise    with `apply`, tensor t of network n is quantised in place at b_{j_t}: the weight and the code are bit for bit
 *               what dfq_batch_quant_plan_run stores for a tensor described with num_bits = b_{j_t} and the plan's symmetric /
 *               per_row.  With apply = 0 no weight and no code is written.
 * Outputs, blocks of the caller: `bits` int32 [n_nets, T] the chosen width; `errors` float64 [n_nets, T, B]; `used` int64
 * [n_nets, 2] = (used bits, steps taken); `cost` float64 [n_nets] = sum_t c[t][j_t] added in rising t; `ranges` float32
 * [n_nets, range_stride], (min, max) per row of a per_row plan, one pair per tensor otherwise -- what the quant plan writes,
 * written with or without `apply`; `codes` [n_nets, code_stride] of code_bytes-wide elements (4 = int32; 1 = uint8, or int8
 * with symmetric, only if b_{B-1} <= 8; 0 = no codes).  code_offset / range_offset are in elements of their block, -1 = none.
 * Rows and tensors of at most dfq_batch_quant_register_elements() elements stay in registers between their range and their
 * errors; a weight is read at most three times and written once.  Launches per run are fixed at creation (2 to 4: ranges of
 * the long per-tensor tensors, errors, allocation -- one workgroup per network --, quantisation); no workgroup waits for
 * another and nothing synchronises with the host.
 * create: DFQ_ERR_ARG (and dfq_last_error) for null or empty tables, a null configuration, B outside 2..8, widths that do not
 * rise or lie outside [2, 16], T * B above 4096, a fixed_bits that is not a candidate, a sensitivity that is negative or not
 * finite, a negative budget, code_bytes other than 0, 1, 4, 1-byte codes with a width above 8, a weight that is null or not
 * 16-byte aligned, rows <= 0 or row_len <= 0, a null bits / errors / used / cost block, a tensor that writes codes or ranges
 * into a null block, offsets outside their strides, null bases, networks that are not 16-byte aligned to network 0.  Every
 * tensor of network 0 must lie inside network 0's slot: nothing here can check that.  Synchronises (create only); run is
 * asynchronous on `stream`. */
typedef struct dfq_batch_mixed_plan dfq_batch_mixed_plan;
typedef struct dfq_batch_mixed_tensor { /* addresses in network 0 */
    float* data;            /* the layer's weight [rows, row_len], quantised in place with `apply`                   */
    int64_t rows;
    int64_t row_len;
    double sensitivity;     /* s_t                                                                                   */
    int32_t fixed_bits;     /* 0: free; else a candidate width the tensor is pinned to                               */
    int32_t pad;
    int64_t code_offset;    /* elements into a network's code block, or -1                                           */
    int64_t range_offset;   /* floats into a network's range block, or -1                                            */
} dfq_batch_mixed_tensor;
typedef struct dfq_batch_mixed_config {
    int32_t widths[8];      /* b_0 < b_1 < ...; the first n_widths count                                             */
    int32_t n_widths;       /* B                                                                                     */
    int32_t symmetric;      /* the signed recipe                                                                     */
    int32_t per_row;        /* ranges per output row instead of per tensor                                           */
    int32_t apply;          /* 0: allocate only                                                                      */
    int32_t code_bytes;     /* 0, 1 or 4                                                                             */
    int32_t pad;
    int64_t budget_bits;    /* the same for every network                                                            */
} dfq_batch_mixed_config;

int dfq_batch_mixed_plan_create(const dfq_batch_mixed_tensor* tensors, int32_t n_tensors, const dfq_batch_mixed_config* config,
                                const void* const* bases, int32_t n_nets, int32_t* bits, double* errors, int64_t* used, double* cost,
                                void* codes, int64_t code_stride, float* ranges, int64_t range_stride, dfq_batch_mixed_plan** out_plan);
int dfq_batch_mixed_plan_run(dfq_batch_mixed_plan* plan, void* stream);
void dfq_batch_mixed_plan_destroy(dfq_batch_mixed_plan* plan);
/* kernel launches per run, fixed at creation: 2 to 4 for a plan of dfq_batch_mixed_plan_create; 3 to 8 for a clipped plan (three
 * for its flat pieces if it has any, one for its units in registers and looping rows if it has any, the allocation, the state
 * and range launch behind it, and with `apply` one quantising launch for each of the two kinds of work present).  The clear
 * of the range words of the long tensors is a memset.  Stages run through dfq_batch_mixed_plan_run_stages are not counted. */
int32_t dfq_batch_mixed_plan_launches(const dfq_batch_mixed_plan* plan);
/* Allocate on given costs (extension): with `costs` set -- float64 on the device, [n_nets, T, B] with the plan's own T and B,
 * which nothing here can check -- the allocation of every later run forms c[t][j] = s_t * costs[n][t][j] in place of
 * s_t * E[n][t][j]; `cost` then reports the sum of those c at the chosen widths.  Everything else of the definition above is
 * unchanged: E is still computed and reported in `errors`, the walk, its ties, the pins, the budget rule and the quantisation
 * are the same.  Every cost must be finite or NaN; a NaN cost takes no step (g > 0 is false), as a NaN error does.  The block
 * is read by the allocation launch of a run, so whatever writes it (dfq_batch_nsr_plan_run) goes onto the same stream in
 * front.  NULL, the default: the plan's own errors again, every result bit for bit that of a plan that never had costs.
 * DFQ_ERR_ARG for a null plan. */
int dfq_batch_mixed_plan_set_costs(dfq_batch_mixed_plan* plan, const double* costs /* device [n_nets, T, B], or NULL */);

/* Clip-aware mixed precision (extension): the MSE-optimal clip of every unit at EVERY candidate width from one read of the
 * weight, the allocation on those errors, and the clamp and the quantisation of every tensor at its own width and at that
 * width's own range; nothing goes to the host in between.  Everything not mentioned here is dfq_batch_mixed_plan_create's
 * definition, unchanged.
 * DEFINITION.  Inputs: the candidate widths b_0 < ... < b_{B-1}, `symmetric`, `per_row`, K = `candidates` in [1, 64] and
 * `alpha_min` in (0, 1].  A UNIT is a tensor, or an output row with `per_row`; its (mn, mx), its shrink factors a_k, its
 * fixed point z and its candidate ends (l_k, h_k) are dfq_batch_clip_plan_create's, word for word: they do not depend on the
 * width.
 *   unit errors   U[n][u][j][k] = err_k of dfq_batch_clip_plan_create with num_bits = b_j: the error of the weight clamped to
 *                 (l_k, h_k) and quantised, minus the weight as it is, in float64.  The order of each sum is the clip plan's
 *                 for a unit of that shape -- the same lane classes, the same register bound, the same 4096-float pieces for
 *                 longer per-tensor tensors, the same fold order -- so every U[n][u][j][k] is BIT FOR BIT the value
 *                 dfq_batch_clip_plan_run reports for (b_j, symmetric, per_row, K, alpha_min).  No floating-point atomic: two
 *                 runs are bit-equal, and a network's values do not depend on the batch or on its place in it.
 *   choice        per width, k*_j = argmin_k U[..][j][k] found with err < best from k = 0 on, the clip plan's rule: a unit whose
 *                 errors are NaN or all infinite keeps 0, and k*_j is exactly what the clip plan chooses at b_j.
 *   tensor error  E[n][t][j] = U[n][u][j][k*_j] for a per-tensor plan; with per_row the float64 sum of U[n][r][j][k*_j(r)] over
 *                 the rows r in rising order (one running sum from +0.0: the order depends on the row count alone).  `errors`
 *                 reports it; the allocation walks on it, or on the costs of dfq_batch_mixed_plan_set_costs, in which case E
 *                 is still reported.  The walk, its ties, the pins, the budget rule, `bits`, `used` and `cost` are unchanged.
 *   clamp stage   every unit of tensor t of network n is clamped to (l, h) of k*_{j_t}, j_t the index of the chosen width:
 *                 w < l ? l : (w > h ? h : w); NaN and -0.0 pass through; only what the clamp changes is stored, nothing
 *                 where k* = 0.
 *   quantise      clamps the same way and quantises in place at b_{j_t} with qparams(l, h, b_{j_t}, symmetric): the weight and
 *                 the code are bit for bit what dfq_batch_clip_plan_run (b_{j_t}, apply) followed by dfq_batch_quant_plan_run
 *                 (b_{j_t}) leave for that tensor of that network; quantising after a clamp stage gives the same bits as
 *                 quantising alone.  `ranges` holds (l, h) of the chosen width for every unit (where that differs from the
 *                 unit's own (min, max) after the clamp only in the sign of a zero, this is the clip plan's value); the
 *                 allocation stage writes it, with or without `apply`.
 * Outputs in blocks of the caller in addition to the mixed plan's, per unit as in the clip plan, a tensor's first unit at
 * unit_offsets[t] and its rows behind it: `clip_ranges` float32 [n_nets, unit_stride, B, 2] = (l, h) of k*_j; `clip_chosen`
 * int32 [n_nets, unit_stride, B] = k*_j; `unit_errors` float64 [n_nets, unit_stride, B] = U at k*_j, or null: not written.
 * Special values follow from the two parent definitions: a unit holding NaN has NaN errors at every width and k* = 0, its
 * tensor's E is NaN and the tensor takes no step.
 * create: DFQ_ERR_ARG (and dfq_last_error) for everything dfq_batch_mixed_plan_create refuses, a null `clip`, candidates
 * outside [1, 64], alpha_min not in (0, 1] (NaN included), B * K above 512, a null clip_ranges or clip_chosen block, null
 * unit_offsets, unit_stride <= 0, units outside the stride, a shape dfq_batch_clip_plan_create refuses.  The plan is a
 * dfq_batch_mixed_plan: run (the allocation stage, and with `apply` the quantising one), run_stages, set_costs, launches and
 * destroy work on it. */
typedef struct dfq_batch_mixed_clip {
    int32_t candidates;          /* K                                                                                */
    int32_t pad;
    double alpha_min;
    float* clip_ranges;          /* device [n_nets, unit_stride, B, 2]                                               */
    int32_t* clip_chosen;        /* device [n_nets, unit_stride, B]                                                  */
    double* unit_errors;         /* device [n_nets, unit_stride, B], or NULL                                         */
    int64_t unit_stride;         /* units of one network in the three blocks                                         */
    const int64_t* unit_offsets; /* host [n_tensors]: a tensor's first unit; read by create only                     */
} dfq_batch_mixed_clip;

int dfq_batch_mixed_plan_create_clipped(const dfq_batch_mixed_tensor* tensors, int32_t n_tensors, const dfq_batch_mixed_config* config,
                                        const void* const* bases, int32_t n_nets, int32_t* bits, double* errors, int64_t* used, double* cost,
                                        void* codes, int64_t code_stride, float* ranges, int64_t range_stride,
                                        const dfq_batch_mixed_clip* clip, dfq_batch_mixed_plan** out_plan);

/* The stages of a mixed plan one by one (extension), valid on every mixed plan; `stages` is a sum of the values below and they
 * run in this order on `stream`:
 *   DFQ_MIXED_ALLOCATE  ranges, errors, allocation; the allocation is also kept in the PLAN'S OWN state, an index j per
 *                       (network, tensor)
 *   DFQ_MIXED_CLAMP     the clamp at the chosen widths; clipped plans only, DFQ_ERR_ARG on others
 *   DFQ_MIXED_QUANTISE  clamp and quantise at the chosen widths, whatever `apply` the plan was made with
 * CLAMP and QUANTISE read the allocation the plan's last ALLOCATE stage (or, for a clipped plan, run) left in the plan's state,
 * not the caller-writable `bits` block: a caller's write there cannot index past the tables (on a plan without clipping
 * QUANTISE first writes the state's widths into `bits` again).  Without an allocation since creation they return
 * DFQ_ERR_STATE; dfq_batch_mixed_plan_run of a plan without clipping is what it always was and leaves no state.  ALLOCATE |
 * QUANTISE gives what run gives with `apply`, bit for bit.  DFQ_ERR_ARG for a null plan and for stages that are 0 or hold
 * another bit. */
#define DFQ_MIXED_ALLOCATE 1
#define DFQ_MIXED_CLAMP 2
#define DFQ_MIXED_QUANTISE 4
int dfq_batch_mixed_plan_run_stages(dfq_batch_mixed_plan* plan, int32_t stages, void* stream);

/* Data-free layer sensitivities of a whole batch of networks of one architecture (extension): the expected noise-to-signal
 * power ratio of every output channel of every layer at every candidate width, from the weights and the BatchNorm proxies
 * alone -- the costs dfq_batch_mixed_plan_set_costs takes.  `tensors` and `sources` describe the FIRST of `n_nets` networks;
 * network n's copy of a tensor or proxy lies bases[n] - bases[0] bytes further.  Nothing is written but the output blocks.
 * DEFINITION.  Layer t of network n has the weight W [O, I/g, K] (rows = O, row_len = I/g * K, kernel_len = K = kH * kW,
 * groups = g); element (o, i, k) of row o reads input channel c(o, i) = (o / (O/g)) * (I/g) + i.
 *   moments     a[n][t][c], float32, c in [0, g * I/g), from the layer's sources [source_begin, source_begin + source_count)
 *               of the dfq_bc_source table: the BatchNorms the bias-correction walk lists for it, in its order.  Per source
 *               (mean, var) is bit for bit what dfq_relu_moments gives at mode 1 if `relu` is set, else mode 0; a source
 *               without fake_weight has mean = beta~ and var = 0.  The first source sets the pair; a source with `concat`
 *               continues at the next channel; any other adds mean and var onto the channels so far, in source order, one
 *               float32 addition each, as `accumulate` of dfq_relu_moments does.  Then, with v = var < 0 ? 0 : var,
 *                 moment = 0 (variance):       a_c = v -- the noise that remains once bias correction has removed the mean
 *                                              term (sum e * mu)^2;
 *                 moment = 1 (second moment):  a_c = (float)((double)mean * (double)mean + (double)v).
 *               NaN stays NaN.  A layer with source_count = 0 -- the first convolution, any layer fed by the data -- gets
 *               a_c = input_moment for every c (float32, finite, >= 0).
 *   rows        per row o and width j, in float64.  e_j = fake_quant(w; qparams(min, max, b_j, symmetric)) - w in float32,
 *               term for term the e of dfq_batch_error_plan and dfq_batch_mixed_plan; (min, max) is the tensor's pair, or
 *               row o's with per_row; NaN is skipped by the ranges.
 *                 Ne[o][j] = sum over (i, k) of (double)a_c(o,i) * (e_j * e_j)    (the square is exact, the product one rounding)
 *                 S[o]     = sum over (i, k) of (double)a_c(o,i) * (w * w)
 *                 R[o][j]  = S[o] == 0 ? 0 : Ne[o][j] / S[o], one division.
 *               The order of the two sums is the plan's own and depends on the row's length alone.  No floating-point atomic
 *               is used: two runs are bit-identical, and network n's values depend neither on n_nets nor on n's place in the
 *               batch.  R is the expected noise-to-signal power ratio of output channel o under independent input channels
 *               and positions with those moments; numerator and denominator share the model, so no BatchNorm behind the
 *               layer is needed.
 *   costs       N[n][t][j] = R[0][j] + R[1][j] + ... in rising o, from 0.0, one float64 addition each.
 * A tensor holding a NaN weight gets NaN in its own slots only; a NaN moment does the same for the rows that read it.
 * Candidate widths b_0 < ... < b_{B-1}, integers in [2, 16], 1 <= B <= 8.
 * Outputs, blocks of the caller: `moments` float32 [n_nets, moment_stride], layer t's a at moment_offset; `rows` float64
 * [n_nets, row_stride, B], R of layer t's row o at (row_offset + o); `signal` float64 [n_nets, row_stride], S, may be NULL;
 * `costs` float64 [n_nets, T, B].  Nothing else in the blocks is touched.
 * Launches per run, fixed at creation (3, or 4 per tensor): the moments, a workgroup per (network, layer); per tensor the
 * tensors' (min, max); the rows; the fold.  A row of at most dfq_batch_quant_register_elements() elements stays in registers
 * from its range through all B errors, L lanes per row with L taken from the row length and B + 1 float64 accumulators per
 * lane; longer rows get a looping wave.  Every weight is read once with per_row, twice per tensor.  No workgroup waits for
 * another and nothing synchronises with the host.
 * create: DFQ_ERR_ARG (and dfq_last_error) for null or empty tables, a null configuration, B outside 1..8, widths that do not
 * rise or lie outside [2, 16], row_len % kernel_len != 0, rows % groups != 0, sources whose channels do not sum to
 * groups * row_len / kernel_len (or an add of another length, or a null proxy), a source range outside the table, an
 * input_moment that is negative or not finite, an unknown `moment`, a weight that is null or not 16-byte aligned, rows <= 0 or
 * row_len <= 0, a null moments / rows / costs block, offsets outside their strides, null bases, networks that are not 16-byte
 * aligned to network 0.  Synchronises (create only); run is asynchronous on `stream`. */
typedef struct dfq_batch_nsr_plan dfq_batch_nsr_plan;
typedef struct dfq_batch_nsr_tensor { /* addresses in network 0 */
    const float* data;      /* the layer's weight [rows, row_len]; read only                                         */
    int64_t rows;           /* O                                                                                     */
    int64_t row_len;        /* I/g * K                                                                               */
    int64_t kernel_len;     /* K = kH * kW                                                                           */
    int32_t groups;         /* g                                                                                     */
    int32_t source_begin;   /* range in the dfq_bc_source table; source_count = 0: input_moment                     */
    int32_t source_count;
    int32_t pad;
    int64_t moment_offset;  /* floats into a network's moment block                                                  */
    int64_t row_offset;     /* rows into a network's row and signal blocks                                           */
} dfq_batch_nsr_tensor;
typedef struct dfq_batch_nsr_config {
    int32_t widths[8];      /* b_0 < b_1 < ...; the first n_widths count                                             */
    int32_t n_widths;       /* B                                                                                     */
    int32_t symmetric;      /* the signed recipe                                                                     */
    int32_t per_row;        /* ranges per output row instead of per tensor                                           */
    int32_t moment;         /* 0: variance, 1: second moment                                                         */
    float input_moment;     /* a_c of a layer without sources                                                        */
    int32_t pad;
} dfq_batch_nsr_config;
struct dfq_bc_source;       /* defined with the bias correction, below */

int dfq_batch_nsr_plan_create(const dfq_batch_nsr_tensor* tensors, int32_t n_tensors, const struct dfq_bc_source* sources,
                              int32_t n_sources, const dfq_batch_nsr_config* config, const void* const* bases, int32_t n_nets,
                              float* moments, int64_t moment_stride, double* rows, double* signal, int64_t row_stride, double* costs,
                              dfq_batch_nsr_plan** out_plan);
int dfq_batch_nsr_plan_run(dfq_batch_nsr_plan* plan, void* stream);
void dfq_batch_nsr_plan_destroy(dfq_batch_nsr_plan* plan);
/* kernel launches per run (3 or 4), fixed at creation; the clear of the range words of a per-tensor plan is a memset */
int32_t dfq_batch_nsr_plan_launches(const dfq_batch_nsr_plan* plan);

/* Dense bit-packing of the integer codes of a whole batch, every tensor of every network at its own width, and the way back
 * (extension; the artefact of a mixed-precision calibration: dfq_batch_quant_plan, dfq_batch_squant_plan and
 * dfq_batch_mixed_plan leave one byte or four per weight, this leaves b / 8).  The tables describe ONE network; every block is
 * [n_nets, stride] and owned by the caller.
 * DEFINITION.
 *   unsigned code  A tensor has a width b in [1, 16] and a `symmetric` flag: qmin = -2^(b-1) if symmetric, else 0.  The unsigned
 *               code of a stored code q is u = (q - qmin) & (2^b - 1).  For the codes the quantisers above write the mask
 *               changes nothing; for a caller's out-of-range codes the mask IS the behaviour, not an error.
 *   stream      Tensor t of network n has n_t elements in the order of its weight (row-major [rows, row_len]) and the width
 *               b = b[n][t].  Its stream is n_t * b bits; element i occupies bits [i b, (i + 1) b), least significant bit first;
 *               uint32 word w holds bits [32 w, 32 w + 32), bit k of the stream at bit k mod 32 of word k div 32.  The stream
 *               takes extent(n, t) = ceil(n_t b / 32) words rounded up to a multiple of 4 (16 bytes); every bit beyond n_t b up
 *               to the end of the extent is written as ZERO, so the packed words of a network are a pure function of its codes
 *               and widths.
 *   offsets     int64 [n_nets, T + 1]: offset[n][0] = 0, offset[n][t + 1] = offset[n][t] + extent(n, t), computed on the device
 *               by one workgroup per network (the widths are on the device; nothing goes to the host).  offset[n][T] is the
 *               network's size in words, and 0 <= 32 offset[n][T] - sum_t n_t b[n][t] < 159 T (at most 31 bits to the word and
 *               three words to the extent, per tensor): a network dfq_batch_mixed_plan allocated in `used` bits packs into
 *               less than used + 159 T bits, so ceil(budget / 32) + 5 T words hold it whenever used <= budget.
 *   widths      per tensor either `num_bits` in [1, 16], or num_bits = 0 and the width is read on the device from an int32 block
 *               [n_nets, width_stride] at width_index -- what dfq_batch_mixed_plan writes as `bits`, and how
 *               dfq_bc_plan_run_widths reads it.  A width read from the device outside [1, 16], or above 8 with one-byte codes,
 *               gives status[n] = 2 and network n is skipped: nothing of its packed row and nothing of its offsets is written.
 *   capacity    the packed block is uint32 [n_nets, word_stride].  offset[n][T] > word_stride gives status[n] = 1: nothing of
 *               network n's packed row is written, its offsets ARE (the caller learns the size it needs).  status[n] = 0
 *               otherwise.  The other networks are not affected, and words at and beyond offset[n][T] are never written.
 *   unpack      from the words, the offsets, the widths and the range block a quantiser wrote ((min, max) float32, a pair per
 *               tensor, or per row with per_row), either or both of
 *                 (a) the codes q = u + qmin into a code block, int32 or one byte (uint8 / int8, the low byte of q, widths <= 8);
 *                 (b) the weights, in place in the batch: y = (float)q * p.scale + p.min_value with
 *                     p = qparams_double((double)min, (double)max, b, symmetric) of csrc/dfq_common.hpp -- two separately rounded
 *                     float32 operations, exactly the last two of the quantisers' fake_quant_one.
 *               It rounds nothing else and reads no weight.  Unpack does not recompute offsets: it reads those pack (or a
 *               loader) left, and skips network n -- status 2 for a bad device width, else status 1 -- if offset[n][0] != 0, if
 *               a tensor's extent as the offsets give it is not extent(n, t), or if offset[n][T] > word_stride.
 *   zero's sign  a quantiser can store -0.0 where the integer code gives +0.0 (a unit whose min is -0.0 and an element whose q
 *               came out as -0.0).  The definition above, from the integer code, is what unpack computes: against the
 *               quantiser's stored weights it is equal in value everywhere, and bit for bit wherever no weight of the unit is a
 *               zero.  Tensors holding NaN are outside the contract (their code is whatever the quantiser left).
 * Launches: pack 2 (offsets, one workgroup per network; then pack), unpack 1.  No workgroup waits for another, no atomic
 * touches a packed word (every word is composed by one lane from the at most ceil(32 / b) + 1 codes that reach into it), the
 * packed block need not be cleared, nothing synchronises with the host outside create.  A tensor is cut into chunks of
 * dfq_batch_pack_chunk_elements() elements, a multiple of 32: every chunk starts on a word boundary at every width, so the
 * grid depends on the element counts alone; a workgroup takes a few consecutive chunks of one tensor, tail and padding included.
 * create (both): DFQ_ERR_ARG (and dfq_last_error) for null or empty tables, code_bytes other than 1 or 4, a num_bits outside
 * {0} and [1, 16] or above 8 with one-byte codes, num_bits = 0 with a null width block, a width_index outside width_stride,
 * offsets outside their strides, numel <= 0, null bases or networks that are not 16-byte aligned to network 0.  pack: a null
 * code, packed, offsets or status block.  unpack: a null words, offsets or status block; neither codes nor any weight to
 * write; a tensor with a weight and no range block or a range_offset < 0, a weight that is not 16-byte aligned, rows * row_len
 * != numel, row_len above 2^31 - 1; with a null code block code_bytes and the code offsets are ignored.  Synchronises (create
 * only); run is asynchronous on `stream`. */
typedef struct dfq_batch_pack_plan dfq_batch_pack_plan;
typedef struct dfq_batch_pack_tensor {
    int64_t code_offset;    /* elements into a network's code row                                                    */
    int64_t numel;          /* n_t                                                                                   */
    int32_t num_bits;       /* 1..16, or 0: read the width block                                                     */
    int32_t width_index;    /* into a network's row of the width block (num_bits == 0)                               */
    int32_t symmetric;
    int32_t pad;
} dfq_batch_pack_tensor;
/* `bases` are taken and checked as by the other batch plans; pack itself reads nothing through them */
int dfq_batch_pack_plan_create(const dfq_batch_pack_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                               const void* codes, int32_t code_bytes, int64_t code_stride, const int32_t* widths, int64_t width_stride,
                               uint32_t* packed, int64_t word_stride, int64_t* offsets, int32_t* status, dfq_batch_pack_plan** out_plan);
int dfq_batch_pack_plan_run(dfq_batch_pack_plan* plan, void* stream);
void dfq_batch_pack_plan_destroy(dfq_batch_pack_plan* plan);
/* kernel launches per run (2) */
int32_t dfq_batch_pack_plan_launches(const dfq_batch_pack_plan* plan);
/* elements of a tensor one workgroup takes (a multiple of 32) */
int64_t dfq_batch_pack_chunk_elements(void);

typedef struct dfq_batch_unpack_plan dfq_batch_unpack_plan;
typedef struct dfq_batch_unpack_tensor {
    float* data;            /* the weight in network 0, [rows, row_len], written in place; NULL: codes only          */
    int64_t rows;
    int64_t row_len;
    int64_t code_offset;    /* elements into a network's code row (ignored with a null code block)                   */
    int64_t numel;
    int64_t range_offset;   /* floats into a network's range block: (min, max), per row with per_row                 */
    int32_t num_bits;
    int32_t width_index;
    int32_t symmetric;
    int32_t per_row;
} dfq_batch_unpack_tensor;
int dfq_batch_unpack_plan_create(const dfq_batch_unpack_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                 const uint32_t* words, int64_t word_stride, const int64_t* offsets, const int32_t* widths,
                                 int64_t width_stride, const float* ranges, int64_t range_stride, void* codes, int32_t code_bytes,
                                 int64_t code_stride, int32_t* status, dfq_batch_unpack_plan** out_plan);
int dfq_batch_unpack_plan_run(dfq_batch_unpack_plan* plan, void* stream);
void dfq_batch_unpack_plan_destroy(dfq_batch_unpack_plan* plan);
/* kernel launches per run (1) */
int32_t dfq_batch_unpack_plan_launches(const dfq_batch_unpack_plan* plan);

/* MX block-scaled FP4 / FP6 / FP8 (extension; the OCP Microscaling formats the block-scaled f8f6f4 MFMA of gfx950 multiplies
 * natively: 32 elements share one E8M0 scale).  Weights of a batch (the plans), and any tensor along any axis (dfq_mx_axis: the
 * activations); no matmul, and no bias correction or adaptive rounding on these grids.
 * DEFINITION.
 *   formats     id, bits, exponent / mantissa bits, bias, largest magnitude, emax:
 *                 DFQ_MX_E2M1 = 0: 4 bits, 2 / 1, bias  1, largest 6,                          emax  2
 *                 DFQ_MX_E2M3 = 1: 6 bits, 2 / 3, bias  1, largest 7.5,                        emax  2
 *                 DFQ_MX_E3M2 = 2: 6 bits, 3 / 2, bias  3, largest 28,                         emax  4
 *                 DFQ_MX_E4M3 = 3: 8 bits, 4 / 3, bias  7, largest 448   = magnitude code 126, emax  8
 *                 DFQ_MX_E5M2 = 4: 8 bits, 5 / 2, bias 15, largest 57344 = magnitude code 123, emax 15
 *               A code is sign bit | exponent | mantissa in the low `bits` bits of a byte.  Subnormals (exponent field 0) are
 *               kept: value(k) = m 2^(1 - bias - M) for exponent field 0, (2^M + m) 2^(x - bias - M) for field x > 0 (M mantissa
 *               bits).  The magnitude codes 0..cmax are monotone in value.  No Inf or NaN code is ever written: conversion
 *               saturates to cmax (the OCP specification leaves overflow implementation-defined for E5M2; this is the choice).
 *   blocks      A tensor is [rows, row_len].  Row r is cut into bpr = ceil(row_len / 32) blocks of DFQ_MX_BLOCK = 32 consecutive
 *               elements; the last block of a row may be short, no block crosses a row.  Block (r, j) has scale byte
 *               s[r * bpr + j].
 *   exponent    amax = max |w| over the block.  E = the unbiased exponent field of amax as a float32, -127 for a zero or
 *               subnormal amax.  e0 = max(E - emax, -127).  search = 0: e = e0.  search = 1: e is the one of {e0, e0 + 1}
 *               with the smaller block error S(e); e0 on a tie or if either S is NaN.  S(e) = sum d^2 with
 *               d = (double)stored - (double)w: one float64 subtraction and one float64 multiplication per element, added as a
 *               balanced binary tree over the element's index in the block -- level m pairs index i with i xor m, for
 *               m = 1, 2, 4, 8, 16, absent elements counting as +0.0 -- so the choice is a pure function of the block.
 *               Scale byte s = e + 127, in [0, 254].
 *   element     v = w 2^(-e) in real arithmetic (|v| < 2^(emax + 1)).  The magnitude code is the code nearest to |v|, a tie going
 *               to the even code (IEEE round to nearest even); everything at or above the largest magnitude goes to cmax.  The
 *               sign bit is w's, so -0.0 and negative values that round to zero keep it.
 *   stored      stored = +-value(code) 2^e, exact in float32 for every format and every e >= -127 down to 2^-143: subnormal
 *               float32 results are exact and no flush mode is relied on (the conversion is integer arithmetic on the bit
 *               pattern).  One corner is not representable: amax in the top binade under e0 + 1 can round up to 2^128; the stored
 *               value is then +-Inf, S(e0 + 1) = Inf, and the search keeps e0 -- no Inf is ever stored.
 *   non-finite  A block holding any NaN or +-Inf gets scale byte 255; its codes are 0, its stored weights all the quiet NaN
 *               0x7fc00000, and its tensor's errors NaN at every format.  No other block or tensor is affected.
 *   errors      E[n][t][f] = sum d^2 over tensor t of network n for candidate format f, float64 -- all candidates from ONE read
 *               of the weight.  The order is the plan's own: a workgroup adds the S of its DFQ_MX_BLOCK-blocks (64 consecutive
 *               ones of one tensor) in a fixed order into one partial sum, a second launch adds a tensor's partial sums in a
 *               fixed order.  It depends on the tensor's shape alone and uses no floating-point atomic: two runs are bit-equal,
 *               and network n's values depend neither on n_nets nor on n's place in the batch.
 *   decode      codes, scale bytes and a width give the stored weights by `stored` above; s = 255 makes the block the quiet NaN.
 *               Magnitude codes above cmax, which the quantiser never writes, decode by the same formula.
 * dfq_mx_rows: one tensor, one launch.  y (float32 [rows, row_len], may be x), codes (uint8, one per element), scales (uint8
 * [rows * bpr]) and err (float64 [rows * bpr]: the S(e) of every block, by the tree above, NaN for a non-finite block) are each
 * written unless NULL.  DFQ_ERR_ARG for a null x, an x that is not 4-byte aligned, rows or row_len <= 0, row_len above 2^31 - 1, more than 2^29 blocks, an
 * unknown format.
 * dfq_mx_axis: the same along any axis, one launch.  x is float32 [outer, len, inner], contiguous, and the blocks run along len:
 * block (o, j, i) holds x[o, 32 j + t, i], t = 0..31; the last block j = bpa - 1 of an (o, i) is short when len % 32 != 0
 * (bpa = ceil(len / 32)); no block crosses an o or an i.  y (float32, may be x), codes (uint8, one per element, in x's layout),
 * scales (uint8 [outer, bpa, inner]) and err (float64 [outer, bpa, inner]: each block's S(e)) are each written unless NULL.
 * `exponent`, `element`, `stored` and `non-finite` above apply word for word; the index in the tree of S(e) is t, absent elements
 * count as +0.0.  EQUIVALENCE: the result is exactly dfq_mx_rows on the tensor with len moved last ([outer * inner, len]), moved
 * back -- stored values, codes, scale bytes and block errors, bit for bit.  inner == 1 IS the row case and takes dfq_mx_rows'
 * launch (rows = outer, row_len = len); otherwise a lane owns a block and no lane waits for another.  DFQ_ERR_ARG for a null x, an
 * x that is not 4-byte aligned, outer, len or inner <= 0, len above 2^31 - 1, more than 2^29 blocks, an unknown format.
 * Asynchronous on `stream`.
 * The batch plan, in the shape of dfq_batch_squant_plan and dfq_batch_mixed_plan: the table describes network 0, network n's copy
 * of a tensor lies bases[n] - bases[0] bytes further.  The blocks are the caller's: errors float64 [n_nets, n_tensors, F]
 * (F = n_widths), codes uint8 [n_nets, code_stride], scales uint8 [n_nets, scale_stride], status int32 [n_nets].
 *   config      widths: the candidates, a rising subset of (4, 6, 8); width 4 is E2M1, widths 6 and 8 are format6 (E2M3 or E3M2)
 *               and format8 (E4M3 or E5M2); `search` as above; `num_bits`: the width to quantise at when no device widths are
 *               set, one of the candidates (read with `apply` only).
 *   stages      DFQ_MX_ERRORS reads every weight once and writes nothing but `errors` (and the plan's own partial sums): two
 *               launches.  DFQ_MX_QUANTISE reads every weight once and writes the stored weight in place, the code byte and the
 *               block's scale byte: one launch.  dfq_batch_mx_plan_run is ERRORS, followed by QUANTISE with `apply`;
 *               dfq_batch_mx_plan_launches counts those (2 or 3).  dfq_batch_mx_plan_run_stages runs any of the two, whatever
 *               `apply` says; the stages keep no state in the plan.
 *   set_widths  dfq_batch_squant_plan_set_widths' contract: with `widths` set -- int32 on the device, [n_nets, width_stride] --
 *               every later QUANTISE treats tensor t of network n at widths[n * width_stride + width_index[t]], bit for bit as a
 *               plan with that num_bits.  A width that is none of the plan's candidates makes the items of that (network, tensor)
 *               write nothing -- no weight, code or scale byte of it is touched -- and status[n] becomes 2; every QUANTISE with
 *               widths set clears `status` first with a memset on the stream.  NULL restores `num_bits`; `status` is then not
 *               touched.  A call with `widths` set synchronises.  DFQ_ERR_ARG for a null plan, widths without width_index or
 *               status, an index that is negative or >= width_stride.
 * No workgroup waits for another; half a wave takes a block, a lane an element.  create: DFQ_ERR_ARG (and dfq_last_error) for
 * null or empty tables, a null configuration, widths that are no rising subset of (4, 6, 8), a format id that does not match
 * its width, `apply` with a num_bits that is no candidate, rows or row_len <= 0, row_len above 2^31 - 1, a weight that is null or
 * not 4-byte aligned, offsets outside their strides, a null errors block (it is what ERRORS writes), a null code or scale block
 * that a tensor's offset >= 0 points into, null bases, networks that are not 16-byte aligned to network 0.  run_stages: a null
 * plan, stages that are 0 or hold an unknown bit.  Synchronises (create only); run is asynchronous on `stream`. */
#define DFQ_MX_E2M1 0
#define DFQ_MX_E2M3 1
#define DFQ_MX_E3M2 2
#define DFQ_MX_E4M3 3
#define DFQ_MX_E5M2 4
#define DFQ_MX_BLOCK 32
#define DFQ_MX_ERRORS 1
#define DFQ_MX_QUANTISE 2
int dfq_mx_rows(const float* x, float* y, int64_t rows, int64_t row_len, int32_t format, int32_t search, uint8_t* codes, uint8_t* scales,
                double* err, void* stream);
int dfq_mx_axis(const float* x, float* y, int64_t outer, int64_t len, int64_t inner, int32_t format, int32_t search,
                uint8_t* codes, uint8_t* scales, double* err, void* stream);

typedef struct dfq_batch_mx_plan dfq_batch_mx_plan;
typedef struct dfq_batch_mx_tensor {
    float* data;            /* device, inside network 0's slot; [rows, row_len], quantised in place                  */
    int64_t rows;
    int64_t row_len;
    int64_t code_offset;    /* bytes into a network's code row (one per element), or -1                              */
    int64_t scale_offset;   /* bytes into a network's scale row (rows * ceil(row_len / 32) of them), or -1           */
} dfq_batch_mx_tensor;
typedef struct dfq_batch_mx_config {
    int32_t widths[3];      /* the candidates: a rising subset of (4, 6, 8)                                          */
    int32_t n_widths;       /* F                                                                                     */
    int32_t format6;        /* DFQ_MX_E2M3 or DFQ_MX_E3M2                                                            */
    int32_t format8;        /* DFQ_MX_E4M3 or DFQ_MX_E5M2                                                            */
    int32_t search;
    int32_t apply;          /* run: QUANTISE behind ERRORS                                                           */
    int32_t num_bits;       /* the width QUANTISE works at without device widths                                     */
    int32_t pad;
} dfq_batch_mx_config;
int dfq_batch_mx_plan_create(const dfq_batch_mx_tensor* tensors, int32_t n_tensors, const dfq_batch_mx_config* config,
                             const void* const* bases, int32_t n_nets, double* errors, uint8_t* codes, int64_t code_stride,
                             uint8_t* scales, int64_t scale_stride, dfq_batch_mx_plan** out_plan);
int dfq_batch_mx_plan_run(dfq_batch_mx_plan* plan, void* stream);
int dfq_batch_mx_plan_run_stages(dfq_batch_mx_plan* plan, int32_t stages, void* stream);
int dfq_batch_mx_plan_set_widths(dfq_batch_mx_plan* plan, const int32_t* widths /* device int32 [n_nets, width_stride], or NULL */,
                                 int64_t width_stride, const int32_t* width_index /* host [n_tensors], read here only */,
                                 int32_t* status /* device int32 [n_nets] */);
void dfq_batch_mx_plan_destroy(dfq_batch_mx_plan* plan);
int32_t dfq_batch_mx_plan_launches(const dfq_batch_mx_plan* plan);

/* The way back: ONE launch that turns one-byte codes and scale bytes into the stored weights, in place in the batch (`decode`
 * above).  Per tensor `num_bits` is 4, 6 or 8, or 0 and the width is read on the device from `widths` [n_nets, width_stride] at
 * width_index.  A device width other than 4, 6 or 8 leaves that (network, tensor) untouched and stores status[n] = 2; with any
 * num_bits = 0 every run clears `status` (int32 [n_nets]) first with a memset on the stream, otherwise `status` may be NULL and
 * is not touched.  `gate`: NULL, or int32 on the device, [n_nets]: a network whose word is not 0 when the launch runs is left
 * untouched, weights and status -- the status block of the unpack launch in front, so that a network unpack skipped is not
 * decoded from codes nobody wrote.  It reads no weight.  create: DFQ_ERR_ARG for null or empty tables, a null code or scale block, a num_bits
 * outside {0, 4, 6, 8}, num_bits = 0 with a null width or status block, a width_index outside width_stride, a format id that
 * does not match its width, rows or row_len <= 0, row_len above 2^31 - 1, a weight that is null or not 4-byte aligned, offsets
 * outside their strides, null bases, networks that are not 16-byte aligned to network 0. */
typedef struct dfq_batch_mx_decode_plan dfq_batch_mx_decode_plan;
typedef struct dfq_batch_mx_decode_tensor {
    float* data;            /* the weight in network 0, [rows, row_len], written in place                            */
    int64_t rows;
    int64_t row_len;
    int64_t code_offset;    /* bytes into a network's code row                                                       */
    int64_t scale_offset;   /* bytes into a network's scale row                                                      */
    int32_t num_bits;       /* 4, 6, 8, or 0: read the width block                                                   */
    int32_t width_index;
} dfq_batch_mx_decode_tensor;
int dfq_batch_mx_decode_plan_create(const dfq_batch_mx_decode_tensor* tensors, int32_t n_tensors, const void* const* bases,
                                    int32_t n_nets, const uint8_t* codes, int64_t code_stride, const uint8_t* scales,
                                    int64_t scale_stride, const int32_t* widths, int64_t width_stride, int32_t format6,
                                    int32_t format8, const int32_t* gate /* device int32 [n_nets], or NULL */, int32_t* status,
                                    dfq_batch_mx_decode_plan** out_plan);
int dfq_batch_mx_decode_plan_run(dfq_batch_mx_decode_plan* plan, void* stream);
void dfq_batch_mx_decode_plan_destroy(dfq_batch_mx_decode_plan* plan);
/* kernel launches per run (1) */
int32_t dfq_batch_mx_decode_plan_launches(const dfq_batch_mx_decode_plan* plan);

/* Analytic activation ranges of a whole batch of networks of one architecture (extension; set_quant_minmax,
 * utils/layer_transform.py:347-609, main_cls.py:188, for every network of a batch at once).  The caller walks the graph of
 * the FIRST network once (find_prev_bn, :299-344, and the branch grouping of :476-580) and hands over what the walk found
 * as a small program: one RESULT per quantiser, each a run of STEPS that one workgroup executes per network.  Network n's
 * copy of a tensor lies bases[n] - bases[0] bytes further.  The steps are the arithmetic of :403-418 and :444-601:
 *   CONST       (min, max) = (lo, hi): the quantiser of the network's input (:443-449)
 *   RANGE       (min, max) = (min_c beta - N gamma, max_c beta + N gamma), min clamped at 0 behind ReLU / ReLU6, max at 6
 *               behind ReLU6 (:403-404, :468-469); what dfq_bn_ranges computes
 *   RANGE_CAT   min = min(min, lo); max = max(max, hi) of another such pair (:560-562)
 *   RANGE_ONE   min += max(0., lo); max += hi (:563-567)
 *   RANGE_DIV   min /= operand; max /= operand (operand = bound + 1, :569-570)
 *   MOM         per-channel (mean, var) of N(beta, gamma^2) behind `relu_mode` (:494-507); what dfq_relu_moments computes
 *   MOM_ADD     mean += mean', var += var' of another BatchNorm (:521-531)
 *   MOM_RELU    (mean, var) of N(mean, var + eps) behind ReLU / ReLU6 (:533-540); what dfq_moments_after_add computes
 *   MOM_RANGE   (min, max) = (min_c mean - N sqrt(var + eps), max_c mean + N sqrt(var + eps)) (:571-573); dfq_moment_range
 *               (both with var + eps clamped at 0, see dfq_moments_after_add)
 * A result is CONST alone, or RANGE followed by RANGE_CAT / RANGE_ONE / RANGE_DIV steps, or MOM followed by MOM_ADD /
 * MOM_RELU steps of the same channel count and closed by MOM_RANGE.  A RANGE* step with `source_weight >= 0` reads its two
 * vectors not from a BatchNorm but from SOURCES (case d, :451-466): a proxy vector pushed through a conv / linear layer that
 * has no BatchNorm of its own, v_out[o] = sum_i (sum_k W[o, i, k]) v_in[g(o) I/g + i] + bias[o], what dfq_bn_through_layer
 * computes; the plan keeps them in a block of its own, written by a first launch.
 * Per-channel arithmetic in float32 in the order of those single-network entry points, the fold over channels with their
 * NaN-propagating min / max and partition, the scalar steps in float64 (Python floats in the reference), rounded to float32
 * once at the store into `out` [n_nets][out_stride] at 2 * result: bit-identical to set_quant_minmax on that network alone.
 * One launch (n_results * n_nets workgroups), two with sources; no workgroup waits for another; nothing but `out` and the
 * plan's own block is written.  create: DFQ_ERR_ARG (and dfq_last_error) for null / empty tables, a result whose steps are
 * not one of the three shapes above, an unknown opcode or ReLU mode, a null vector, channel counts that disagree, a source
 * index out of range, a source geometry dfq_bn_through_layer refuses, a non-finite n_sigma, an `out_stride` below
 * 2 * n_results.  Every tensor of network 0 must lie inside network 0's slot: nothing here can check that.  Synchronises
 * (create only); run is asynchronous on `stream` and copies nothing. */
#define DFQ_ACT_CONST 0
#define DFQ_ACT_RANGE 1
#define DFQ_ACT_RANGE_CAT 2
#define DFQ_ACT_RANGE_ONE 3
#define DFQ_ACT_RANGE_DIV 4
#define DFQ_ACT_MOM 5
#define DFQ_ACT_MOM_ADD 6
#define DFQ_ACT_MOM_RELU 7
#define DFQ_ACT_MOM_RANGE 8
typedef struct dfq_batch_act_plan dfq_batch_act_plan;
typedef struct dfq_batch_act_result {
    int32_t step_begin;     /* into `steps`                                                                */
    int32_t step_count;
} dfq_batch_act_result;
typedef struct dfq_batch_act_step {
    const float* fake_weight;   /* gamma~ [channels], network 0 (RANGE*, MOM, MOM_ADD without sources)        */
    const float* fake_bias;     /* beta~  [channels]                                                          */
    int32_t opcode;             /* DFQ_ACT_*                                                                   */
    int32_t channels;
    int32_t relu_mode;          /* 0 none, 1 ReLU, 2 ReLU6                                                     */
    int32_t operand;            /* RANGE_DIV: the divisor                                                      */
    int32_t source_weight;      /* >= 0: the vectors are sources `source_weight` / `source_bias`, not a BN's   */
    int32_t source_bias;
    float lo;                   /* CONST                                                                       */
    float hi;
} dfq_batch_act_step;
typedef struct dfq_batch_act_source {
    const float* weight;        /* [out_ch, in_per_group, khkw], network 0                                     */
    const float* bias;          /* [out_ch] or null                                                            */
    const float* vector;        /* the proxy vector pushed through the layer [groups * in_per_group]           */
    int32_t out_ch;
    int32_t in_per_group;
    int32_t khkw;
    int32_t groups;
} dfq_batch_act_source;

int dfq_batch_act_plan_create(const dfq_batch_act_result* results, int32_t n_results, const dfq_batch_act_step* steps, int32_t n_steps,
                              const dfq_batch_act_source* sources, int32_t n_sources, const void* const* bases, int32_t n_nets,
                              float n_sigma, float eps, float* out, int64_t out_stride, dfq_batch_act_plan** out_plan);
void dfq_batch_act_plan_destroy(dfq_batch_act_plan* plan);
int dfq_batch_act_plan_run(dfq_batch_act_plan* plan, void* stream);
/* launches per run (1, or 2 with sources) */
int32_t dfq_batch_act_plan_launches(const dfq_batch_act_plan* plan);

/* ------------------------------------------------------------------------------------------
 * Lazy-scale equalisation (opt-in extension): the sweeps of dfq.py:83-101 with a GIVEN sweep count,
 * computed from the pristine weights and the cumulative scale vectors of utils/relation.py:20-24 -- a sweep only READS
 * (4 B per element of the layers it still has to look at, see the byte accounting below), the weights / biases / BN proxies / scale_cum vectors of the relations are written ONCE at the end
 * (W = diag(S_out) W0 diag(1/S_in); 8 B per weight).  Result: within 1e-5 (relative) of the sequentially rescaled tensors of
 * the reference loop run for the same number of sweeps -- NOT bit-identical to them (the default engines are).  The
 * data-dependent exit test of dfq.py:105-115 is not available in this formulation: the caller passes the count (e.g. the one
 * dfq_le_run reports for the same network).  Same layer / relation tables as dfq_le_plan_create_batch.  Asynchronous run.
 * ---------------------------------------------------------------------------------------- */
typedef struct dfq_le_lazy_plan dfq_le_lazy_plan;   /* opaque */
int dfq_le_lazy_plan_create(const dfq_layer* layers, int32_t n_layers, const int32_t* layer_net, int32_t n_nets,
                            const dfq_relation* relations, int32_t n_relations, dfq_le_lazy_plan** out_plan);
void dfq_le_lazy_plan_destroy(dfq_le_lazy_plan* plan);
/* cfg: s_range / eps / signed_range as for dfq_le_run (the convergence fields are ignored); sweeps_per_net[n] >= 0 */
int dfq_le_lazy_run(dfq_le_lazy_plan* plan, const dfq_le_config* cfg, const int32_t* sweeps_per_net, void* stream);
/* byte accounting: passes whose element factors never change run once (chain starts / ends, depthwise layers: their extrema
 * are kept and rescaled per sweep by the solve launch), so the FIRST sweep reads 4 B x paired_elements, every later sweep
 * 4 B x sweep_elements (the non-depthwise layers in the interior of a chain, once per role), and the final materialisation
 * moves 8 B x weight_elements */
int32_t dfq_le_lazy_plan_levels(const dfq_le_lazy_plan* plan);
int64_t dfq_le_lazy_plan_paired_elements(const dfq_le_lazy_plan* plan);
int64_t dfq_le_lazy_plan_sweep_elements(const dfq_le_lazy_plan* plan);
int64_t dfq_le_lazy_plan_weight_elements(const dfq_le_lazy_plan* plan);

/* ------------------------------------------------------------------------------------------
 * Bias correction -- dfq.py:173-293 (bias_correction), :8-25 (_quantize_error)
 * ---------------------------------------------------------------------------------------- */
typedef struct dfq_bc_plan dfq_bc_plan;

/* One BatchNorm contributing to E[x] of a layer (dfq.py:229-270), in the order the reference
 * merges them (depth-sorted, stable). */
typedef struct dfq_bc_source {
    const float* fake_weight;  /* device [channels]  (gamma~)                               */
    const float* fake_bias;    /* device [channels]  (beta~) -- read at the layer's turn    */
    int32_t channels;
    int32_t relu;              /* 1: E = gamma*pdf(-b/g) + b*(1-cdf(-b/g)), clipped at 0    */
    int32_t concat;            /* 1: torch.cat onto the running expectation, 0: add (first
                                  source: ignored)                                          */
} dfq_bc_source;

typedef struct dfq_bc_step {
    int32_t layer;             /* index into the dfq_layer table; bias must be non-NULL     */
    int32_t source_begin;      /* range in the dfq_bc_source table                          */
    int32_t source_count;
    float* next_bn_bias;       /* device [out_ch]: fake_bias of the next BN in graph order,
                                  receives += (-bias) (dfq.py:204-206,293); NULL if none    */
    int32_t net;               /* network of a batched plan (0 for a single network); steps are
                                  listed network by network, each network in graph order: the
                                  j-th steps of all networks share one launch                 */
    int32_t reserved;
} dfq_bc_step;

int dfq_bc_plan_create(const dfq_layer* layers, int32_t n_layers,
                       const dfq_bc_step* steps, int32_t n_steps,
                       const dfq_bc_source* sources, int32_t n_sources,
                       dfq_bc_plan** out_plan);
/* Replicated form (see dfq_le_plan_create_replicated): the three tables describe the FIRST of `n_nets` networks of one
 * architecture (step.net = 0, indices relative to that network), network n's tensors lie bases[n] - bases[0] bytes further.
 * (Replaces, for a batch, the per-network graph walk of dfq.py:194-270.) */
int dfq_bc_plan_create_replicated(const dfq_layer* layers, int32_t n_layers, const dfq_bc_step* steps, int32_t n_steps,
                                  const dfq_bc_source* sources, int32_t n_sources, const void* const* bases, int32_t n_nets,
                                  dfq_bc_plan** out_plan);
void dfq_bc_plan_destroy(dfq_bc_plan* plan);
/* per-tensor min/max of all step layers (one launch) -> the sequential per-layer chain (one launch); a step forms
 * the quant-error row sums eps[o, i] = sum_k (Q(w) - w) of its rows (8 bit, dfq.py:216-219) in registers, straight from
 * the weights: 8 B per weight for the whole pass.  Asynchronous. */
int dfq_bc_plan_run(dfq_bc_plan* plan, int32_t symmetric, void* stream);
/* Per-channel mode (extension; dfq.py:216-219 with a per-output-channel quantiser): the same correction, but the quant
 * error of output row o is Q_o(W) - W with Q_o the recipe of utils/quantize.py:23-76 (Python-float min/max) built from
 * row o's own (min, max) at `num_bits` (2..16) bits.  One more launch in front of the chain reduces every row; every
 * hand-over protocol of the plan is kept.  DFQ_ERR_ARG for a null plan or a bad bit width.  Asynchronous. */
int dfq_bc_plan_run_per_channel(dfq_bc_plan* plan, int32_t symmetric, int32_t num_bits, void* stream);
/* Widths mode (extension): dfq_bc_plan_run (per_row == 0) or dfq_bc_plan_run_per_channel (per_row != 0) with exactly one
 * thing replaced -- the correction step of layer t of network n uses
 *     eps[o, i] = sum_k (fake_quant(w; qparams_double(min, max, b[n][t], symmetric)) - w)[o, i, k],
 * a sequential float32 sum from 0.0f as in the other modes, with b[n][t] that layer's OWN bit width and (min, max) the
 * tensor's pair, or with `per_row` row o's pair (NaN rule: "Special values").  E[x] and its add / cat merges, the grouped
 * matvec, b -= bias, next beta~ += -bias, the chain order, the depthwise folds and every hand-over protocol are untouched, so
 * eps is term for term the error of what a quantisation of that layer at b[n][t] bits (dfq_batch_quant_plan,
 * dfq_batch_mixed_plan with the same per_channel / signed) will store -- computed before it is stored.
 * Widths: `widths` is int32 on the device, the width of step s of network n is widths[n * width_stride + width_index[s]];
 * `width_index` is a HOST table with one entry per step of the plan as created (a replicated plan: network 0's steps; a
 * plain plan: all steps, network 0 throughout, width_stride unused).  It is uploaded when it differs from the last run's.
 * widths == NULL: `uniform_bits` for every step.  Valid widths are 2..16.  A host-given width is checked here; a value read
 * on the device cannot be, so the device CLAMPS it to [2, 16] before any shift is formed from it.
 * One launch (per_row) or two (per tensor: a workgroup per layer merges the rows' pairs into the tensor's -- selections,
 * exact in any order, no atomic -- and writes it to every row) in front of the chain, one read of the weights more than
 * the chain's own.  Never recorded (DFQ_GRAPH=1 runs it directly: its arguments are not fixed per plan).
 * dfq_bc_plan_set_safe_mode / dfq_bc_plan_status as for a per-channel run.  DFQ_ERR_ARG for a null plan, uniform_bits
 * outside [2, 16] when widths is NULL, widths without width_index, a negative index or stride.  Asynchronous. */
int dfq_bc_plan_run_widths(dfq_bc_plan* plan, int32_t symmetric, int32_t per_row,
                           const int32_t* widths /* device, or NULL */, int64_t width_stride,
                           const int32_t* width_index /* host, one per step as created; NULL with widths == NULL */,
                           int32_t uniform_bits /* used when widths == NULL */, void* stream);
/* device pointers into the plan's scratch (tests): the correction vector bias[O] of a step; eps[O*I/g] only for plans
 * created with DFQ_BC_EPS=1 in the environment (debug: one more launch materialises the row sums the chain computes on the
 * fly, same arithmetic) -- NULL otherwise */
/* Synchronises `stream`; DFQ_ERR_STATE if a workgroup of the last run gave up waiting for the correction step it
 * depends on (the chain of all layers is ONE launch whose workgroups wait for the previous layer's; the wait is
 * bounded).  DFQ_BC_MERGED=0 in the environment at plan creation restores one launch per layer. */
int dfq_bc_plan_status(dfq_bc_plan* plan, void* stream);
const float* dfq_bc_plan_eps(const dfq_bc_plan* plan, int32_t step);
const float* dfq_bc_plan_correction(const dfq_bc_plan* plan, int32_t step);
int64_t dfq_bc_plan_weight_elements(const dfq_bc_plan* plan);
/* 1 when the one-launch chain hands values from step to step as tagged 64-bit slots (the default), 0 when it uses per-step
 * counters (DFQ_BC_TAGGED=0, or a graph the tagged scheme does not cover) or one launch per chain position. */
int32_t dfq_bc_plan_tagged(const dfq_bc_plan* plan);
/* 1 if the correction chain runs as ONE launch whose workgroups wait for each other (dfq_bc_plan_status can then report
 * DFQ_ERR_ABANDONED after biases / BN proxies have been rewritten).  dfq_bc_plan_set_safe_mode: one launch per chain position
 * from now on -- nothing waits, nothing can be abandoned (the parity-tested DFQ_BC_MERGED=0 path).  BCPlan.run() of the Python
 * binding uses the pair to repeat an abandoned pass from a device-side snapshot. */
int32_t dfq_bc_plan_has_waits(const dfq_bc_plan* plan);
int dfq_bc_plan_set_safe_mode(dfq_bc_plan* plan);
/* 1 when the LATEST run of the plan used the tagged slots, 0 when it used counters (a run recorded into a graph) or has not run.
 * A run on the NULL stream is an ordinary run (until round 5 it was mistaken for a recording: counters, no guard). */
int32_t dfq_bc_plan_last_run_tagged(const dfq_bc_plan* plan);
/* 1 when a tagged run of the plan is ONE launch: the per-tensor min/max blocks are workgroups of the chain launch, woven in a few chain
 * positions in front of the steps that need them (DFQ_BC_ONE_LAUNCH=0, a kept eps matrix or rows too long for the registers:
 * min/max launch + chain launch).  A never-rewritten BN read through a ReLU does NOT prevent it: the cached moments of such BNs are
 * refreshed by the launch's first blocks and their readers wait for those blocks (cache_arrive). */
int32_t dfq_bc_plan_one_launch(const dfq_bc_plan* plan);
/* Diagnostics.  A library built with -DDFQ_BC_TRACE=1 (tools/bc_trace.py) records five timestamps per workgroup of the one-launch
 * chain; this copies up to `words` 64-bit words of them to `out` and returns the number copied -- 0 from the shipped library. */
int64_t dfq_bc_debug_trace(long long* out, int64_t words);
int64_t dfq_bc_plan_eps_elements(const dfq_bc_plan* plan);
/* Depthwise steps folded into the per-row tail of the step in front of them, and the dependent positions the chain is left
 * with (MobileNetV2: 17 of 52 steps folded -> 35 positions).  A layer with one input channel per group and as many groups as
 * outputs corrects channel o with eps[o] * E[o] alone (dfq.py:281-287 with I/g = 1), and E[o] is what the thread owning row o
 * of the previous step has just produced (dfq.py:204-206, 238-242): that thread performs the depthwise layer's update too --
 * the same operations in the same order, bit-identical -- and one hand-over through the memory system per depthwise layer
 * disappears.  DFQ_BC_FOLD=0 in the environment at plan creation keeps every step. */
int32_t dfq_bc_plan_folded(const dfq_bc_plan* plan);
int32_t dfq_bc_plan_chain_steps(const dfq_bc_plan* plan);

/* _quantize_error (dfq.py:8-25) on one tensor: q(x) - x with per-tensor min/max, 5 reductions:
 *   reduction 0: none   -> out[n]
 *   reduction 1: 'sum'  -> out[0] = sum |eps|
 *   reduction 2: 'mean' -> out[0] = mean eps
 *   reduction 3: 'channel' -> out[0] = sum_o | sum_rest eps |      (rows = shape[0])
 *   reduction 4: 'spatial' -> out[0] = sum_{o,i} | sum_khkw eps |  (rows = shape[0]*shape[1])
 * `rows` is the number of leading-dimension groups for reductions 3/4 (ignored otherwise).
 * `scratch` is device memory of dfq_quant_error_scratch_bytes(n, rows) bytes.  DFQ_ERR_ARG (and dfq_last_error) for
 * symmetric with num_bits == 1 (qmax = 0, see dfq_fake_quant). */
size_t dfq_quant_error_scratch_bytes(int64_t n, int64_t rows);
int dfq_quant_error(const float* x, int64_t n, int64_t rows, int32_t num_bits, int32_t symmetric,
                    int32_t reduction, float* out, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row / column rescale helpers -- utils/layer_transform.py:231-276 (merge_batchnorm),
 * utils/quantize.py:145-174,:269-289 (merge_scale*), dfq.py:121-170 (bias_absorption, clip_weight)
 * ---------------------------------------------------------------------------------------- */

/* w[o, :] = w[o, :] * s[o]   (op 0)   or   w[o, :] / s[o]   (op 1);  row_len = I/g * khkw */
int dfq_scale_rows(float* w, int32_t rows, int64_t row_len, const float* s, int32_t op, void* stream);
/* Input-channel rescale of a grouped conv weight [O, I/g, khkw]: input channel of element
 * (o, i, k) is  (o / (O/groups)) * I/g + i;  w = w * s[ch] (op 0) or w / s[ch] (op 1). */
int dfq_scale_cols(float* w, int32_t out_ch, int32_t in_per_group, int32_t khkw, int32_t groups,
                   const float* s, int32_t op, void* stream);
/* vector helpers on [n]: y = y * s (op 0), y / s (op 1), y + s (op 2), y - s (op 3) */
int dfq_vec_op(float* y, const float* s, int64_t n, int32_t op, void* stream);

/* Batched rebuild from pristine tensors and cumulative scale vectors (utils/relation.py:20-24; the replicated write of
 * the sharded equalisation):  dst[o,i,k] = fl(fl(src[o,i,k] * s_out[o]) / s_in[ch(o,i)])  with
 * ch = (o / (rows/groups)) * cols + i  -- two separately rounded float32 operations in this order; a NULL vector
 * skips its step (both NULL: a copy).  Vectors (bias, BN proxies) are items with cols = khkw = groups = 1.  src may equal
 * dst.  ONE launch covers all items of a plan (8 B per element); identical inputs give bit-identical outputs on every
 * rank.  `items` is a host array and is copied.  Synchronises (create only). */
typedef struct dfq_rebuild_item {
    const float* src;      /* device [rows, cols, khkw]                                   */
    float* dst;            /* device, same shape                                          */
    const float* s_out;    /* device [rows] or NULL                                       */
    const float* s_in;     /* device [groups * cols] or NULL                              */
    int32_t rows;          /* O                                                           */
    int32_t cols;          /* I / groups                                                  */
    int32_t khkw;
    int32_t groups;
    int32_t in_reciprocal; /* 0: divide by s_in[ch]; 1: s_in holds reciprocals: multiply  */
    int32_t reserved;
} dfq_rebuild_item;
typedef struct dfq_rebuild_plan dfq_rebuild_plan;   /* opaque */
int dfq_rebuild_plan_create(const dfq_rebuild_item* items, int32_t n_items, dfq_rebuild_plan** out_plan);
void dfq_rebuild_plan_destroy(dfq_rebuild_plan* plan);
int64_t dfq_rebuild_plan_elements(const dfq_rebuild_plan* plan);
int dfq_rebuild_plan_run(dfq_rebuild_plan* plan, void* stream);
/* x = clamp(x, lo, hi) (dfq.py:170) */
int dfq_clamp(float* x, int64_t n, float lo, float hi, void* stream);

/* BatchNorm folding (layer_transform.py:246-272) for one (conv, bn) pair.  In place:
 *   k = gamma / sqrt(var + bn_eps);  W[o,:] *= k[o];  b = b*k + (beta - gamma*mean/sqrt(var+bn_eps));
 *   fake_weight = |gamma|; fake_bias = beta;  then gamma=1, var=1, beta=0, mean=0. */
int dfq_fold_batchnorm(float* w, float* b, int32_t out_ch, int64_t row_len, float* gamma,
                       float* beta, float* mean, float* var, float bn_eps, float* fake_weight,
                       float* fake_bias, void* stream);

/* Bias absorption for one relation (dfq.py:138-164):  c = max(0, beta~ - N*gamma~);
 * wc[g] = (sum_khkw W2)[g] . c[g];  b1 -= c;  beta~ -= c;  b2 += wc. */
int dfq_bias_absorb(const float* w2, int32_t o2, int32_t in_per_group, int32_t khkw, int32_t o1,
                    float* b1, float* b2, const float* bn_weight, float* bn_bias, float n_sigma,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Stand-alone steps of one equalisation pair / one correction layer: what the
 * plans above fuse, exported one by one.  Composing them reproduces dfq.py:28-75 for one pair bit for bit
 * with the plans (same device arithmetic); they cost two passes over the data and four launches per
 * pair, so the plans are the fast path.  All pointers are device pointers, all calls asynchronous.
 * ---------------------------------------------------------------------------------------- */
/* out[r] = range(W[r, :]): max-min (signed_range 0, dfq.py:54-55) or max|.| (1, dfq.py:50-51); NaN is skipped, a row of
 * nothing but NaN gives -inf ("NaN rule of the channel ranges" at dfq_le_plan_create; torch's max() would propagate) */
int dfq_row_range(const float* w, int64_t rows, int64_t row_len, int32_t signed_range, float* out, void* stream);
/* out[g*I/g + ii] = range over the O/groups rows of pairing group g and the khkw taps of input channel ii
 * of W2 [O, I/g, khkw] (the view of dfq.py:41-46; `groups` = O1 / (I2/g), 1 for an ordinary pair); NaN as in dfq_row_range */
int dfq_col_range(const float* w2, int32_t out_ch, int32_t in_per_group, int32_t khkw, int32_t groups,
                  int32_t signed_range, float* out, void* stream);
/* S[c] = clamp((1/(r1+eps)) * sqrt(r1*r2+eps)) with the Python max/min semantics of dfq.py:58-59 (NaN ->
 * s_hi); Sinv[c] = the float32 value dfq.py:73 multiplies by (1/S, or float32(1/s_range[k]) where the clamp
 * replaced S by a Python float).  Sinv may be NULL. */
int dfq_le_solve(const float* r1, const float* r2, int64_t n, float eps, double s_lo, double s_hi, float* S,
                 float* Sinv, void* stream);
/* dfq.py:62-73: W1[c,:] *= S[c]; b1, bn_weight, bn_bias (each may be NULL) *= S; W2[:, c] *= Sinv[c] */
int dfq_le_apply(float* w1, int32_t o1, int64_t row_len1, float* w2, int32_t o2, int32_t in_per_group2,
                 int32_t khkw2, float* b1, float* bn_weight, float* bn_bias, const float* S, const float* Sinv,
                 void* stream);
/* the four steps above for one pair = _layer_equalization (dfq.py:28-75).  `S` [O1] receives the scale
 * vector, `workspace` is 3*O1 floats of device scratch. */
int dfq_le_pair(float* w1, int32_t o1, int64_t row_len1, float* w2, int32_t o2, int32_t in_per_group2,
                int32_t khkw2, float* b1, float* bn_weight, float* bn_bias, double s_lo, double s_hi,
                int32_t signed_range, float eps, float* S, float* workspace, void* stream);
/* out[0] = float(torch.mean(torch.abs(W - W_prev))) (dfq.py:108): float64 sum in a fixed order, divided by
 * n, rounded once to float32.  `scratch` is dfq_absdiff_mean_scratch_bytes(n) bytes of device memory. */
size_t dfq_absdiff_mean_scratch_bytes(int64_t n);
int dfq_absdiff_mean(const float* w, const float* prev, int64_t n, float* out, void* scratch, void* stream);
/* Per-row (per-output-channel) form of dfq_fake_quant: row r is quantised with its own range -- (mins[r],
 * maxs[r]) if given, its own min/max otherwise (written to minmax_out[2r], [2r+1] if non-NULL).  Same
 * recipe per row as utils/quantize.py:49-74; this is the per-channel weight quantiser of the ncnn table
 * (convert_ncnn.py:178-201: one scale per output channel) and of ZeroQ (quant_utils.py:39-135). */
int dfq_fake_quant_rows(const float* x, float* y, int64_t rows, int64_t row_len, const float* mins,
                        const float* maxs, int32_t num_bits, int32_t symmetric, float* codes, float* minmax_out,
                        void* stream);
/* ZeroQ's per-output-channel asymmetric weight quantiser (ZeroQ/utils/quantization_utils/quant_utils.py:85-135 as
 * used by quant_modules.py:161-171): scale = (1/clamp(max-min, 1e-8)) * (2^k-1) (two roundings, as torch evaluates `n / tensor`), zero point = round(scale*min) + 2^(k-1),
 * q = clamp(round(scale*x - zp), -2^(k-1), 2^(k-1)-1), y = (q + zp)/scale, all in float32.  Row r uses (mins[r],
 * maxs[r]) if given, its own min/max otherwise; `codes` (float, signed integers) and `minmax_out` may be NULL. */
int dfq_zeroq_quant_rows(const float* x, float* y, int64_t rows, int64_t row_len, const float* mins, const float* maxs,
                         int32_t num_bits, float* codes, float* minmax_out, void* stream);
/* out[o] = eps[o, :] . expect[(o / (O/groups)) * I/g ...] (dfq.py:281-287), float64 accumulation */
int dfq_grouped_matvec(const float* eps, const float* expect, int32_t out_ch, int32_t in_per_group,
                       int32_t groups, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Analytic activation ranges -- utils/layer_transform.py:347-609 (set_quant_minmax): the channel arithmetic
 * and reductions behind QuantMeasure.running_min / running_max when no calibration data is used.  The graph
 * walk (find_prev_bn :299-344, branch grouping) stays on the host; see dfq_amd/utils/layer_transform.py.
 * ---------------------------------------------------------------------------------------- */
typedef struct dfq_bn_range_req {
    const float* fake_weight;  /* device [channels]  gamma~ of the BN that feeds the quantiser      */
    const float* fake_bias;    /* device [channels]  beta~                                           */
    int32_t channels;
    int32_t relu_mode;         /* 0: none, 1: ReLU attached, 2: ReLU6 attached                       */
} dfq_bn_range_req;
/* Every "one BN -> one quantiser" case of a network in one launch: out[2i] = min_c(beta~ - N*gamma~)
 * (clamped at 0 if a ReLU/ReLU6 follows), out[2i+1] = max_c(beta~ + N*gamma~) (clamped at 6 for ReLU6)
 * (:403-404, :468-469).  `out` is device [n_reqs][2]; `scratch` is dfq_bn_ranges_scratch_bytes(n_reqs) bytes
 * of device memory.  Copies the request table to the device (synchronises the stream once). */
size_t dfq_bn_ranges_scratch_bytes(int32_t n_reqs);
int dfq_bn_ranges(const dfq_bn_range_req* reqs, int32_t n_reqs, float n_sigma, float* out, void* scratch, void* stream);
/* mean / variance of N(beta~, gamma~^2) after nothing (mode 0: beta~, gamma~^2), ReLU (1, :407-410) or ReLU6
 * (2, :411-418), per channel; accumulate != 0 adds into mean/var (residual adds, :521-531). */
int dfq_relu_moments(const float* weight, const float* bias, int64_t n, int32_t relu_mode, float* mean, float* var,
                     int32_t accumulate, void* stream);
/* Convention for sd = sqrt(var + eps) in dfq_moments_after_add, dfq_moment_range and the MOM_RELU / MOM_RANGE steps of
 * dfq_batch_act_plan_*: the radicand is clamped at 0, sd = sqrt(var + eps < 0 ? 0 : var + eps).  The float32 ReLU6 variance of
 * a narrow channel on the ceiling cancels to a number below -eps (gamma~ = 1.04e-3, beta~ = 5.99877: -6.8e-6, in truth
 * 8.7e-7), where the reference's sqrt is NaN and with it the quantiser's whole range.  Bit-identical to the reference
 * wherever that is finite; a NaN variance still gives NaN.  dfq_relu_moments itself returns the variance as the reference
 * computes it, negative values included. */
/* an add node followed by ReLU (1) / ReLU6 (2): (mean, var) <- moments(sd, mean), sd as above (:533-540); other modes:
 * DFQ_ERR_ARG */
int dfq_moments_after_add(float* mean, float* var, int64_t n, int32_t relu_mode, float eps, void* stream);
/* out2 = (min_c(mean - N*sd), max_c(mean + N*sd)), sd as above (:571-573); NaN propagates as in torch.min / torch.max */
int dfq_moment_range(const float* mean, const float* var, int64_t n, float eps, float n_sigma, float* out2, void* stream);
/* case (d), :455-463: a BN proxy vector pushed through a conv / linear layer without batch norm:
 * v_out[o] = sum_i (sum_k W[o,i,k]) * v_in[group(o)*I/g + i] + bias[o] (bias may be NULL) */
int dfq_bn_through_layer(const float* weight, int32_t out_ch, int32_t in_per_group, int32_t khkw, int32_t groups,
                         const float* bias, const float* v_in, float* v_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm-statistics loss of ZeroQ's data distillation -- ZeroQ/distill_data.py:170-196 (own_loss :40-45):
 * for a BN input x [N, C, H, W] (rows = N*C rows of hw = H*W floats, channel of row r = r % C),
 *   loss2[0] = sum_{n,c} (bn_mean[c] - mean_hw x)^2 / denom,   loss2[1] = sum_{n,c} (bn_std[c] - std_hw(x + eps))^2 / denom
 * (unbiased std; denom = A.size(0) of own_loss: C for the BN terms, N for the input-batch term of :192-196), one read of x; row_mean / row_std [rows] are kept for the backward pass, which writes (or adds
 * into) grad_x = grad_mean_loss * d loss2[0]/dx + grad_std_loss * d loss2[1]/dx with one read of x.
 * `scratch`: dfq_bn_stat_loss_scratch_bytes(rows) bytes.  H*W == 1 follows distill_data.py:181-182: the mean term per
 * (n, c) value, the std term over the contiguous [N, C] block REINTERPRETED as C rows of N values (row r against
 * bn_std[r]); row_std then holds C entries.  The `_dev` backward reads the two upstream gradients from device memory
 * (grad_pair[0] = d/d loss2[0], grad_pair[1] = d/d loss2[1]): no host synchronisation inside an autograd backward.
 * Degenerate rows: the variance comes from float64 sums of (x + eps) minus the row's first (x + eps), so a large common
 * offset cancels exactly and a spatially constant row has row_std == 0 exactly (never NaN; the square root's argument is
 * clamped at 0).  A row whose row_std is 0 gets NO std-term gradient -- torch's std backward, masked_fill_(result == 0, 0),
 * not 0 / 0 -- in both row views of the H*W == 1 branch; its mean-term gradient is unchanged.  A NaN or inf in x stays in
 * its own row's statistics and gradient (and in the losses).
 * ---------------------------------------------------------------------------------------- */
size_t dfq_bn_stat_loss_scratch_bytes(int64_t rows);
int dfq_bn_stat_loss_forward(const float* x, int64_t rows, int64_t hw, int32_t channels, const float* bn_mean,
                             const float* bn_std, float eps, float denom, float* row_mean, float* row_std, float* loss2,
                             void* scratch, void* stream);
int dfq_bn_stat_loss_backward(const float* x, int64_t rows, int64_t hw, int32_t channels, const float* bn_mean,
                              const float* bn_std, float eps, float denom, const float* row_mean, const float* row_std,
                              float grad_mean_loss, float grad_std_loss, float* grad_x, int32_t accumulate, void* stream);
int dfq_bn_stat_loss_backward_dev(const float* x, int64_t rows, int64_t hw, int32_t channels, const float* bn_mean,
                                  const float* bn_std, float eps, float denom, const float* row_mean, const float* row_std,
                                  const float* grad_pair, float* grad_x, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Empirical bias correction on distilled data -- improve_dfq.py:311-371 (bias_correction_distill): the per-channel sums of
 * a hooked output, reduced on the device the moment the hook sees it, and the bias update made of them.
 * ---------------------------------------------------------------------------------------- */
/* improve_dfq.py:349-355 (`outputs.mean(0)` per batch, summed over the batches) and :365 (`.sum(-1)` over H*W), in one
 * read of x [n_samples, channels, hw] (contiguous float32, 16-byte aligned; row r has hw floats and channel r % channels):
 *   acc[c] = acc[c] + weight * sum_n sum_hw x[n, c, hw]
 * in float64 from the first addition on; weight = 1 / n_samples is the reference's mean(0).  No floating-point atomic: the
 * order of the additions depends on (n_samples, channels, hw) alone, so two runs are bit-equal wherever x lies.  NaN and
 * +-inf are data: they reach the sum of their own channel and no other.  `scratch` is device memory of
 * dfq_channel_sum_scratch_bytes(n_samples, channels, hw) bytes (0 for a shape the call refuses), 8-byte aligned; its
 * contents need not survive the call.  DFQ_ERR_ARG: a null pointer, a size < 1, x not 16-byte or acc / scratch not 8-byte
 * aligned, hw above 2^31 - 2^14 or more than 2^31 - 1 pieces of 4096 floats. */
size_t dfq_channel_sum_scratch_bytes(int64_t n_samples, int64_t channels, int64_t hw);
int dfq_channel_sum_accumulate(const float* x, int64_t n_samples, int64_t channels, int64_t hw, double weight, double* acc,
                               void* scratch, void* stream);
/* improve_dfq.py:361-368: bias[c] = bias[c] - (float)((acc_q[c] - acc_ref[c]) * scale) -- the difference and the product
 * in float64, ONE rounding of the shift to float32, then ONE float32 subtraction (`module.bias.add_(-error)`). */
int dfq_bias_sub_channel_delta(float* bias, const double* acc_q, const double* acc_ref, int64_t channels, double scale,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Clipped activation ranges from distilled data (extension: the reference has min / max rules only): the histogram of a
 * quantiser's input, reduced on the device the moment a hook sees it, and the percentile / MSE-optimal range read off it.
 * ---------------------------------------------------------------------------------------- */
/* counts[slot(x[i])] += 1 for every i < n, in one read of x (contiguous float32, 16-byte aligned).  `range2` is a DEVICE
 * float32[2] = (lo, hi): nothing is read on the host and nothing waits.  `counts` is a device uint64[bins + 3]: the bins,
 * then `below` (slot bins), `above` (bins + 1) and `nan` (bins + 2); the call ADDS to it, the caller clears it.
 * The slot of an element, in float32 with no contraction:
 *     w = hi - lo;  degenerate := not (w is finite and w > 0)
 *     x is NaN (either sign, quiet or signalling)  ->  nan
 *     degenerate:  x < lo -> below;  x > hi -> above;  else bin 0
 *     otherwise:   inv = (float)bins / w            (IEEE division)
 *                  t   = (x - lo) * inv             (one subtraction, one multiplication)
 *                  t < 0            -> below
 *                  t >= (float)bins -> x <= hi ? bin bins - 1 : above
 *                  else             -> bin (int)t   (truncation; t is NaN only when bins / w overflowed and x == lo: bin 0)
 * So +-inf land in above / below, denormals and -0.0 are ordinary values, lo > hi and a width that overflows ((-3e38, 3e38))
 * are degenerate, and the sum over all bins + 3 slots grows by exactly n per call.  Counts are integers added with integer
 * atomics: the result does not depend on the order of the additions and is bit-equal from run to run.
 * n == 0 is a no-op (x may then be null: an empty tensor has no address).  DFQ_ERR_ARG: a null pointer, bins outside [2, 4096], n < 0 or more than 2^31 - 1 pieces of 131072
 * floats, x not 16-byte aligned (the Python layer copies such a view), range2 not 4-byte or counts not 8-byte aligned. */
int dfq_act_hist_accumulate(const float* x, int64_t n, const float* range2, int32_t bins, unsigned long long* counts,
                            void* stream);
/* The clipped range of n_hist histograms in ONE launch: counts[n_hist][bins + 3] (layout above), range2[n_hist][2] the
 * (lo, hi) they were counted over, num_bits[n_hist] (device int32), out2[n_hist][2] (device float32).
 *     n_b     = counts[b], `below` added to bin 0 and `above` to bin bins - 1; NaN is ignored.  total = sum n_b
 *     edge(b) = f32(lo + b (hi - lo) / bins) in float64, edge(0) = lo and edge(bins) = hi exactly
 *     rep(b)  = f32(lo + (b + 1/2)(hi - lo) / bins), but rep(0) = lo and rep(bins - 1) = hi: the point masses of ReLU and
 *               ReLU6 sit exactly on the extrema
 * method 0, percentile, param = p in (0.5, 1]: k = clamp(ceil(p total), 1, total) in float64; hi' = edge(b_hi + 1) for the
 *     first b_hi whose inclusive prefix sum is >= k, lo' = edge(b_lo) for the last b_lo whose inclusive suffix sum is >= k.
 * method 1, MSE, candidates = C in [1, bins / 2] (param unused): err(l, h) = sum_b n_b (fq(rep(b); l, h, bits) - rep(b))^2
 *     with fq the asymmetric float64-scale recipe of dfq_fake_quant (scale = max((h - l) / (2^bits - 1), 1e-8) in double);
 *     difference, square and sum in float64, the sum in bin order.  k_h = argmin_{k < C} err(lo, edge(bins - k)), then
 *     k_l = argmin_{k < C} err(edge(k), edge(bins - k_h)), the smallest k on a tie; the result is
 *     (edge(k_l), edge(bins - k_h)).
 * A degenerate range (above) or total == 0 gives (lo, hi) unchanged.
 * DFQ_ERR_ARG: a null or misaligned pointer, n_hist < 0, bins outside [2, 4096], an unknown method, p outside (0.5, 1]
 * (method 0), C outside [1, bins / 2] (method 1).  The bit widths live on the device and are NOT read here: the Python
 * layer (prims.hist_clip_range) refuses a width outside [2, 16]; the kernel leaves the range of such a histogram unchanged. */
int dfq_hist_clip_range(const unsigned long long* counts, const float* range2, int32_t n_hist, int32_t bins,
                        const int32_t* num_bits, int32_t method, double param, int32_t candidates, float* out2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFQ_HIP_H */
