/*
 * hjgpu.h — C-ABI of libhjgpu: MI355X (gfx950) hash-join operators.
 *
 * This is the drop-in boundary for the hot path of xtcyclist/hash_join_codes_KNL.
 * The reference has no plugin/FFI layer: its "interface" is the operator
 * functions that run()/run_hj() call (npj.cpp:769-927, phj.cpp:1646-1949,
 * cpra2.cpp:1697-1986).  Each entry point below names the reference operator(s)
 * it replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - Column layout is hj.h:1-72's: separate uint32 key and payload columns
 *     (inner = build side R, outer = probe side S).  `d_` pointers are DEVICE
 *     pointers (HBM); key and payload columns of one relation must be 16-byte
 *     aligned (the reference requires 64-byte alignment, npj.cpp:118-126).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     `*_async` entry points only enqueue; everything else returns after the
 *     work has completed.
 *   - Every function returns an HJGPU_* status (the reference aborts through
 *     assert(); a library reports).  hjgpu_last_error() has the detail text.
 *   - Hash function everywhere: H(key, f, N) = mulhi32((uint32)(key*f), N)
 *     (npj.cpp:200-201, phj.cpp:83-100, 721-722); factors must be odd.
 *   - Join result = order-free aggregates over the three output columns
 *     join_keys / join_outer_vals / join_inner_vals.
 *   - A context owns one workspace: calls on the SAME context must not overlap in
 *     time from several host threads, and joins enqueued on different streams through
 *     one context would share that workspace - use one context per stream / thread
 *     (contexts are cheap; several may live on one device).  Joins enqueued on ONE
 *     stream may be queued back to back without host synchronisation.
 */
#ifndef HJGPU_H
#define HJGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HJGPU_OK          0
#define HJGPU_EINVAL      1   /* null pointer, even factor, fan-out out of range ...        */
#define HJGPU_EALIGN      2   /* column pointer not 16-byte aligned                         */
#define HJGPU_ENOMEM      3   /* device allocation failed                                   */
#define HJGPU_EHIP        4   /* HIP runtime error (text in hjgpu_last_error)               */
#define HJGPU_EZEROKEY    5   /* NPJ only: key 0 is the empty-bucket sentinel (npj.cpp:583) */
#define HJGPU_EOVERFLOW   6   /* materialised output exceeded its capacity
                                 (reference: assert(o <= block_limit), npj.cpp:245)          */
#define HJGPU_ENODEVICE   7   /* no gfx950-class device visible                             */

/* params->flags */
#define HJGPU_FLAG_UNIQUE 1u      /* the reference's -D_UNIQUE build (npj.cpp:288-290, 436-438; phj.cpp:459,
                                     635; cpra2.cpp:456, 625, 698): a probe tuple reports its FIRST match only
                                     and its walk ends there.  With unique build keys the result is the same
                                     as without the flag; with duplicate build keys count / sum_keys /
                                     sum_outer_vals count every probe tuple that has a match once, and
                                     sum_inner_vals adds the payload of ONE of its build tuples (which one
                                     depends on insertion order, in the reference as here).               */
#define HJGPU_FLAG_SEMI   2u      /* semi-join (EXISTS / IN): ONE result row (key, outer_val) for every probe tuple whose key
                                     equals at least one build key.  hjgpu_phj, hjgpu_cpra, hjgpu_npj, their _async forms and
                                     hjgpu_phj_overlapped_async; every other join entry point refuses it (HJGPU_EINVAL).   */
#define HJGPU_FLAG_ANTI   4u      /* anti-join (NOT EXISTS / NOT IN): ONE result row for every probe tuple whose key equals
                                     no build key (all of them when inner == 0).  Same entry points as HJGPU_FLAG_SEMI.
                                     For both: probe-side duplicates are reported one by one (bag semantics), build-side
                                     duplicates never multiply a row; count / sum_keys / sum_outer_vals are taken over the
                                     reported probe tuples, sum_inner_vals is 0; hjgpu_output::d_inner_vals is neither read
                                     nor written and may be NULL.  SEMI | ANTI: HJGPU_EINVAL.  HJGPU_FLAG_UNIQUE (or option
                                     "unique") beside either is ignored.  PHJ / CPRA: every key value is legal on both sides;
                                     NPJ: a build key 0 is still HJGPU_EZEROKEY, a probe key 0 matches nothing.           */
#define HJGPU_FLAG_LEFT_OUTER 8u  /* left outer join that keeps the probe side (S LEFT JOIN R ON S.key = R.key, S the outer
                                     relation): every inner-join row, exactly as without the flag (build-side duplicates
                                     multiply the rows, probe-side duplicates are reported one by one), plus ONE row
                                     (key, outer_val, HJGPU_NULL_VAL) for every probe tuple whose key equals no build key (every
                                     probe tuple when inner == 0).  count, sum_keys and sum_outer_vals are taken over all rows,
                                     NULL rows included; sum_inner_vals adds the matched rows' payloads only (a NULL adds 0, as
                                     SQL's SUM ignores NULL) - the one case where sum_inner_vals is NOT the sum of the
                                     d_inner_vals column.  Rows have three columns: hjgpu_output::d_inner_vals is required.  A
                                     row cannot tell a NULL from a genuine build payload 0xFFFFFFFF; the aggregates are exact
                                     either way.  With HJGPU_FLAG_UNIQUE (or option "unique"): exactly one row per probe tuple,
                                     its first match or its NULL row (count == outer; which build payload a key with duplicate
                                     build keys gets is unspecified) - the dimension-lookup join.  Same entry points as
                                     HJGPU_FLAG_SEMI; every other join entry point refuses it (HJGPU_EINVAL), as do
                                     LEFT_OUTER | SEMI and LEFT_OUTER | ANTI.  PHJ / CPRA: every key value is legal on both sides;
                                     NPJ: a build key 0 is still HJGPU_EZEROKEY, a probe key 0 matches nothing (a NULL row).   */
#define HJGPU_FLAG_RIGHT_OUTER 16u /* right outer join that keeps the BUILD side (S RIGHT JOIN R ON S.key = R.key, R the inner
                                     relation): every inner-join row, exactly as without the flag, plus ONE row
                                     (key, HJGPU_NULL_VAL, inner_val) for every build tuple whose key equals no probe key
                                     (build-side duplicates one by one; every build tuple when outer == 0; nothing extra when
                                     inner == 0).  count, sum_keys and sum_inner_vals are taken over all rows; sum_outer_vals
                                     adds the matched rows' payloads only.  Rows have three columns: d_outer_vals and
                                     d_inner_vals are both required; hjgpu_output_capacity(rows) holds for the true row count
                                     (at most the inner join's rows + inner).  Same entry points as HJGPU_FLAG_SEMI; every
                                     other join entry point refuses it (HJGPU_EINVAL).  Refused beside HJGPU_FLAG_SEMI, _ANTI and
                                     HJGPU_FLAG_UNIQUE / option "unique" (a first-match walk would leave the other copies of a
                                     duplicated build key neither in a row nor NULL).  Keys as for HJGPU_FLAG_LEFT_OUTER.      */
#define HJGPU_FLAG_FULL_OUTER (HJGPU_FLAG_LEFT_OUTER | HJGPU_FLAG_RIGHT_OUTER)
                                  /* full outer join: the inner join's rows, the left outer join's NULL rows
                                     (key, outer_val, HJGPU_NULL_VAL) and the right outer join's (key, HJGPU_NULL_VAL, inner_val).
                                     sum_outer_vals and sum_inner_vals each skip the rows whose value on that side is the NULL.
                                     inner == 0: identical to LEFT_OUTER; outer == 0: identical to RIGHT_OUTER.  At most the
                                     inner join's rows + inner + outer rows.  Refusals as for HJGPU_FLAG_RIGHT_OUTER.          */
#define HJGPU_FLAG_RIGHT_SEMI 32u  /* right semi-join (the build tuples WITH a partner: "the dimension rows with at least one fact"):
                                     ONE row (key, inner_val) for every build tuple whose key equals at least one probe key.
                                     Build-side duplicates are reported one by one, probe-side duplicates never multiply a row;
                                     empty when inner == 0 or outer == 0.  count, sum_keys and sum_inner_vals are taken over the
                                     reported build tuples, sum_outer_vals is 0.  Rows have two columns, d_keys and d_inner_vals
                                     (required: HJGPU_EINVAL without it); d_outer_vals is neither read nor written and may be
                                     NULL (the _async forms' hjgpu_set_async_output still wants all three).
                                     hjgpu_output_capacity(rows) holds for the true row count (at most inner).  Same entry
                                     points as HJGPU_FLAG_SEMI; every other join entry point refuses it (HJGPU_EINVAL).  Refused
                                     beside HJGPU_FLAG_SEMI, _ANTI, _LEFT_OUTER, _RIGHT_OUTER and _RIGHT_ANTI; HJGPU_FLAG_UNIQUE
                                     (or option "unique") beside it is ignored - no row depends on which copy a walk finds.
                                     Keys as for HJGPU_FLAG_LEFT_OUTER; a payload 0xFFFFFFFF is an ordinary payload here.       */
#define HJGPU_FLAG_RIGHT_ANTI 64u  /* right anti-join (the build tuples WITHOUT a partner: "the dimension rows no fact refers
                                     to"): ONE row (key, inner_val) for every build tuple whose key equals no probe key - every
                                     build tuple when outer == 0, none when inner == 0.  Everything else as for
                                     HJGPU_FLAG_RIGHT_SEMI.                                                                      */
#define HJGPU_NULL_VAL    0xFFFFFFFFu  /* the value on the side without a match in an outer join's NULL row              */

#define HJGPU_MAX_FANOUT  1024u   /* per partitioning pass                                   */
#define HJGPU_MAX_PARTS   32768u  /* fanout1 * fanout2                                       */

typedef struct hjgpu_ctx hjgpu_ctx;

typedef struct {
    uint64_t count;            /* J                                                          */
    uint64_t sum_keys;         /* sum join_keys[j]        mod 2^64                           */
    uint64_t sum_outer_vals;   /* sum join_outer_vals[j]  (probe-side payload)               */
    uint64_t sum_inner_vals;   /* sum join_inner_vals[j]  (build-side payload); left outer
                                  joins (HJGPU_FLAG_LEFT_OUTER): over the matched rows only,
                                  a NULL row's HJGPU_NULL_VAL adds 0                          */
} hjgpu_result;

/* Optional materialised output: three device columns of `capacity` uint32.
 * Blocks of block_size tuples are claimed with one atomic each, exactly the
 * reference's protocol (npj.cpp:244-246, 312-316); after the join the dense
 * prefix [0, count) holds the result (close_gaps, npj.cpp:475-514). */
typedef struct {
    uint32_t *d_keys;
    uint32_t *d_outer_vals;
    uint32_t *d_inner_vals;
    size_t    capacity;        /* in tuples; multiple of block_size                          */
    size_t    block_size;      /* power of two; 0 = 65536 (npj.cpp:945)                      */
} hjgpu_output;

typedef struct {
    uint32_t fanout1, fanout2; /* pass fan-outs; 0 = choose from |R| and the LDS table size  */
    uint32_t factor1, factor2; /* odd pass multipliers; 0 = library defaults                 */
    uint32_t table_factor[2];  /* odd table hash / step multipliers; 0 = defaults            */
    uint32_t chunks;           /* CPRA only: number of independently partitioned chunks
                                  (the reference's #threads, cpra2.cpp:1757-1827, 2023); 0 = 8;
                                  1..256 (HJGPU_EINVAL beyond: the result does not depend on it;
                                  beyond 8 the plan is always two passes)                    */
    uint32_t flags;            /* HJGPU_FLAG_*                                               */
} hjgpu_phj_params;

typedef struct {
    double   load;             /* buckets = inner/load (npj.cpp:944-947); 0 = 0.25           */
    uint32_t factor;           /* odd multiplier; 0 = default                                */
    uint32_t flags;            /* HJGPU_FLAG_*                                               */
} hjgpu_npj_params;

/* Per-phase device times of the last join on this context (hipEvent based).
 * A blocking hjgpu_phj whose build side was partitioned BESIDE its probe side (option "build_beside", below; hjgpu_get_counter
 * "build_beside" counts these joins) has phases on two streams that overlap: they no longer add up to ms_total.  For such a join
 * ms_total is the span from the first to the last event on the caller's stream; ms_scatter1 / ms_scatter2 are the PROBE side's passes
 * on the caller's stream; ms_histogram / ms_plan are the BUILD side's own spans on the side stream (K4 from the fork on; K5 and K5b),
 * whose K6 passes are not reported apart; ms_inner_wait is what the caller's stream then waited for the build side behind the probe
 * side's pass 2. */
typedef struct {
    float    ms_total;         /* first to last event on the caller's stream                 */
    float    ms_histogram;     /* K4: fused two-level histogram, R and S (build beside: R, on the side stream) */
    float    ms_plan;          /* K5: prefix sums / cursors (build beside: on the side stream) */
    float    ms_scatter1;      /* K6 pass 1, R and S (build beside: S alone)                 */
    float    ms_scatter2;      /* K6 pass 2, R and S (build beside: S alone)                 */
    float    ms_join;          /* K7+K8 (PHJ/CPRA) or K3 probe (NPJ)                         */
    float    ms_build;         /* NPJ: K1 clear + K2 build                                   */
    float    ms_close_gaps;    /* K9                                                         */
    float    ms_inner_wait;    /* stream time spent waiting for the build side: to arrive
                                  (hjgpu_phj_overlapped_async), or to be partitioned on the side
                                  stream (build beside); 0 otherwise                         */
    float    ms_upload;        /* hjgpu_join_host: host columns -> HBM (wall clock, pipelined
                                  with the probe side's partitioning for PHJ / CPRA)         */
    float    ms_download;      /* hjgpu_join_host_rows: result columns -> host (wall clock)  */
    float    ms_reserve;       /* wall clock this context has spent growing its workspace so far (hjgpu_reserve / the
                                  first join of a size): allocations plus the placement search for the probe side's
                                  pass-1 twin (option "placement": up to 12 candidate blocks held and filled twice);
                                  never inside a timed join once the workspace is reserved                   */
    uint32_t fanout1, fanout2; /* what was used                                              */
    uint32_t batches;          /* PHJ: batches the probe side was partitioned in (both passes of a batch
                                  back to back, its intermediate copy kept in the Infinity Cache; their
                                  time is reported as ms_scatter1, ms_scatter2 = 0); 0 = unbatched    */
    uint64_t buckets;          /* NPJ table size                                             */
    float    ms_scatter0;      /* grouped plans (a build side of option "group_from" tuples and more, the reference's
                                  third pass, phj.cpp:1791-1808): pass 0, both relations split into `groups`
                                  key-disjoint groups; every other phase is then the SUM over the groups' joins,
                                  ms_total the sum of all of it                                              */
    uint32_t groups;           /* 0 = the plain two-pass plan                                */
    /* the context's last placement search (option "placement": candidate blocks for a buffer of 1 GiB and more that K6's
     * pass 1 scatters into; outside every timed join): blocks allocated and filled, 1 when the search's wall-clock budget
     * (option "placement_ms", default 500) ended it before a fast block was found, the kept block's fill time and size
     * (bytes / ms = its fill rate: >= 5.5 TB/s is the fast kind), and what the search cost: its wall clock
     * beyond the kept block's own hipMalloc (ms_reserve above is ALL growth of the workspace: every allocation, and in a fresh
     * process the first kernel's code-object load) */
    uint32_t placement_tried, placement_timeboxed;
    float    placement_fill_ms;
    float    placement_search_ms;
    uint64_t placement_bytes;
} hjgpu_stats;

typedef struct {
    char     name[128];
    char     arch[64];
    int      compute_units;
    int      lds_bytes_per_block;
    uint64_t hbm_bytes;
} hjgpu_device_info;

/* ---- context ---------------------------------------------------------------- */
/* hash of the kernel sources this library was built from: measurements (profiles/ traffic files) name the
 * kernels they were taken with, bench.py refuses counters of other kernels */
const char *hjgpu_kernel_hash(void);
/* hash of EVERY source of this library (every .hip and .hpp file under csrc, this header): stress / validation logs and the bench line name the
 * library they were taken with - a change of the orchestration changes it, the kernel hash above need not */
const char *hjgpu_library_hash(void);
int  hjgpu_device_count(int *count);                      /* visible GPUs (hosts that do not link HIP) */
int  hjgpu_create(int device, hjgpu_ctx **ctx);           /* device < 0: current device      */
int  hjgpu_destroy(hjgpu_ctx *ctx);
const char *hjgpu_last_error(const hjgpu_ctx *ctx);
const char *hjgpu_status_string(int status);
int  hjgpu_get_device_info(hjgpu_ctx *ctx, hjgpu_device_info *info);
/* Tuning / test switches of ONE context (the reference's compile-time macros and hard-coded constants,
 * SURVEY.md section 5 "Config / flags").  hjgpu_create reads HJGPU_<NAME> from the environment once;
 * nothing else in the library looks at the environment, and nothing on a launch path reads mutable
 * process-wide state.  Names: "unique" (as HJGPU_FLAG_UNIQUE, for every join of the context,
 * including the operator-level hjgpu_npj_probe), "force_chained", "no_broadcast", "dense2", "npj_refhash",
 * "scatter_prof", "merged_plan", "piece_interleave" (0 / 1); "range_tiles" (n); "join_cfg" ("block,log2slots,batch"); "scatter_cfg" /
 * "scatter2_cfg" ("block,vectors[,carry]"); "placement" (candidate allocations for the probe side's pass-1
 * twin, 1..16; "placement_ms": the search's wall-clock budget, default 500, 0 = none; "placement_log" 1: every candidate's fill time on stderr); "batch_tuples" (n, 0 = off); "group_from" / "group_inner" (tuples), "group_always" and "group_device" (0 / 1), "group_slack" (per cent): the
 * grouped plans of hjgpu_phj / hjgpu_cpra (below); "exact_probe_counts" (0 / 1, default 0: a blocking two-pass hjgpu_phj of one chunk
 * partitions its probe side without the histogram pass, into optimistic regions, and joins again exactly when one is full -
 * hjgpu_get_counter; 1: always the exact path) and "probe_slack" (per cent of slack in those regions, default 12, 0 = none: a region is
 * then the mean number of rows in whole 16-tuple lines - rows that fill it to the last tuple are no overflow, one row more is - and
 * with fewer probe rows than partitions it holds no tuple at all: such a join always falls back, and is counted);
 * "build_beside" (0 / 1, default 1: such a join, when both relations have rows, partitions its build side on a second stream of the
 * context while the probe side goes through its passes on the caller's - a fork and a join inside the call; 0: one stream, the build
 * side first; a join under option "solo" never forks: its plain stores rest on the promise of one stream) and "build_cus" (the CUs the
 * build side's kernels get while the probe side's passes keep the others: 0 = the library's choice, which steps aside on small chips,
 * for probe sides below 2^20 rows and for probe sides of fewer than 12 rows per build row; 1 ... CUs - 1: that many, at any size and
 * ratio); "solo" (0 / 1, default 0: the caller promises that nothing else runs on the device beside this context's BLOCKING joins - one process,
 * one stream, as the reference's programs: the joins' partial-line and row stores then stay plain, 4 % faster; without the
 * promise every store that could sit dirty in an L2 is non-temporal, because plain stores ARE lost beside other queues' kernel
 * boundaries: 1.5 in 10^4 steps of the multi-GPU pipeline, DESIGN section 3 "Round 5"); diagnostics: "audit" (0 / 1: every stage of a join leaves a checksum of its output,
 * hjgpu_audit_read below), "hist_min_lds" (bytes of LDS a histogram workgroup asks for at least: nothing else then shares its CU).
 * Unknown names and malformed values: HJGPU_EINVAL. */
int  hjgpu_set_option(hjgpu_ctx *ctx, const char *name, const char *value);
/* Option "audit" (diagnostics; the reference's workers meet at barriers between their phases, phj.cpp:1715-1770,
 * cpra2.cpp:1834-1840 - here the phases are kernels on several streams, and when a step of a pipeline comes out wrong the
 * aggregates do not say which kernel's output lacked the tuples): every PHJ / CPRA / partitioning call of the context is
 * followed, stage by stage and on the call's stream, by read-only kernels that check the stage's output where it lies.
 * A record is 8 stages x {tuples lying in a partition their key does not hash to, sum of keys, sum of payloads, tuples}:
 * 0 probe side as read, 1 after pass 1, 2 final partitions; 3-5 the same for the build side (5 again at every probe of a
 * prepared build side); 6 the join's result; 7 {sequence number, kind (0 whole join, 1 build only, 2 probe only,
 * 3 hjgpu_partition_packed*), build rows, probe rows}.  The context keeps its last 256 records.  *next_seq (may be NULL) =
 * the sequence number the next call will get; records[count][32] = the calls first_seq .. first_seq + count - 1 (waits for
 * `stream`).
 * Which stages a call fills (a stage that is not filled is all zero; the first word of every filled stage 0-5 of a sound call is 0):
 *   0 / 3     whenever the relation has rows - the caller's columns, or the rows [chunk_offsets[0], chunk_offsets[chunks]) of a
 *             pre-partitioned relation's array;
 *   1 / 4     two-pass plans of one chunk over the caller's columns (not hjgpu_cpra's chunks, not pre-partitioned pieces, not a probe
 *             side partitioned in batches, option "batch_tuples"): pass 1's fanout1 partitions;
 *   2 / 5     whenever the relation has rows: fanout1 * fanout2 parts, each holding the partition of its number - chunks * fanout1 *
 *             fanout2 under option "dense2" and of a single pass over chunks, part q then holding partition q % (fanout1 * fanout2);
 *             the partition of a pre-partitioned piece's tuple counts from the layout's first_partition;
 *   6         the four words of the call's hjgpu_result in the order of its fields (count, sum_keys, sum_outer_vals,
 *             sum_inner_vals) when a join ran, whatever its mode;
 *   kind 3    (hjgpu_partition_packed_async, _own_last_async, _counted_async; build rows = n) 0 = the columns as read, 1 = the
 *             packed output where the own-last layout puts it; n == 0 leaves stage 7 alone.
 * Which calls get a sequence number: every call that goes through the PHJ enqueue path or the packed partition operator while
 * the option is set - hjgpu_phj, hjgpu_cpra, their _async forms and hjgpu_phj_overlapped_async (kind 0), hjgpu_phj_build and
 * hjgpu_phj_build_prepartitioned (1), every hjgpu_phj_probe* of them (2), hjgpu_partition_packed* (3).  None: hjgpu_npj*, the
 * look-ups, the column form hjgpu_partition, hjgpu_join_partitions, the column operators, a broadcast join (a small build side
 * without explicit fan-outs, and an anti- or left outer join without build rows), a call that fails its argument checks,
 * hjgpu_audit_recheck, and any call made while the option is off.
 * A grouped plan (see hjgpu_phj; the option selects its host-planned form) leaves ONE kind-0 record PER GROUP that is joined,
 * consecutively and in the order of the groups: the group's rows in stage 7, its own plan's partitions in 1-2 / 4-5, its share of
 * the result in 6 - the stage-0 / stage-3 / stage-6 words of a call's records add up to the whole relations' and the call's result.
 * Pass 0 leaves no record of its own; neither does a group that is skipped (nothing can match) or joined by the broadcast road,
 * nor the grouped plan of hjgpu_phj_overlapped_async, which is planned on the device whatever the option says. */
int  hjgpu_audit_read(hjgpu_ctx *ctx, uint64_t *next_seq, uint64_t first_seq, uint32_t count, uint64_t *records, void *stream);
/* Option "audit", second look (diagnostics): the partition checks of the context's LAST audited call done again with the device quiet
 * (hipDeviceSynchronize first) - by a fresh kernel, and on the host from a copy of the partitions made with hipMemcpy (the copy
 * engine reads memory, not an XCD's L2).  words[checks][9] = {stage, the four words as the fresh kernel counts them, the four words
 * as the host counts them}; *checks = the checks there are, nothing is done when capacity (in checks) is smaller.  A stage whose
 * record was wrong and whose memory is wrong here lost stores; one whose memory is right here was read stale
 * (tools/stress_cpra.py --forensics prints the verdict for every wrong step). */
int  hjgpu_audit_recheck(hjgpu_ctx *ctx, uint64_t *words, size_t capacity, size_t *checks);
/* Pre-size the internal workspace (partition scratch twins = hj.h's [1]
 * columns, NPJ table) so that no allocation happens inside a timed join. */
int  hjgpu_reserve(hjgpu_ctx *ctx, size_t inner_tuples, size_t outer_tuples);
int  hjgpu_get_stats(hjgpu_ctx *ctx, hjgpu_stats *stats);
/* Counters of the context (HJGPU_EINVAL for an unknown name):
 *   "probe_fallbacks"  blocking PHJ joins whose claimed probe side (partitioned without its histogram pass, into optimistic regions)
 *                      overflowed and that were therefore done again on the exact path; their results are the exact path's
 *   "probe_exact"      1 when the context's blocking joins take the exact path (option "exact_probe_counts", or after a fallback)
 *   "build_beside"     blocking PHJ joins whose build side was partitioned on the context's side stream beside the probe side's passes
 *                      (option "build_beside")
 *   "lookup_lds_rows"  the largest build side that hjgpu_lookup answers from LDS tables (0 under option "no_broadcast")
 *   "compact_ranges", "compact_chunk_rows"   hjgpu_compact_selected's geometry: the ranges (= workgroups) its rows are cut into, and the
 *                      rows of a chunk, of which every range holds a whole number
 *   "group_lds_groups" the distinct groups a workgroup's LDS table of hjgpu_group_sum holds before its further groups go straight to the
 *                      merge table in device memory
 *   "filter_step_rows" the rows that hjgpu_filter_selected's whole grid covers in one iteration of its loop (the grid is smaller when the
 *                      rows are fewer)
 *   "gather_step_rows" the same for hjgpu_gather_selected
 *   "agg_step_rows", "agg_scalar_step_rows"   the same for hjgpu_group_agg with key columns and without (nkeys == 0)
 *   "group_by_lds_groups", "group_by_step_rows"   hjgpu_group_by with three and four key columns: the distinct groups a workgroup's wide
 *                      LDS table holds, and the rows its whole grid covers in one iteration of its loop
 *   "lookup_wide_step_rows"   the rows hjgpu_lookup_wide's whole look-up grid covers in one iteration of its loop
 *   "order_lds_rows"   the largest n that hjgpu_order_by sorts in one workgroup's LDS
 *   "order_ranges", "order_chunk_rows"   hjgpu_order_by beyond that: the ranges (= workgroups of a pass's histogram and scatter launches) the
 *                      current permutation is cut into, and the rows of a chunk, of which every range holds a whole number */
int  hjgpu_get_counter(hjgpu_ctx *ctx, const char *name, uint64_t *value);

/* ---- device memory helpers for hosts that do not link HIP (mamalloc/free,
 * npj.cpp:118-126, and the fread targets npj.cpp:1013-1039) ------------------- */
int  hjgpu_malloc(hjgpu_ctx *ctx, void **d_ptr, size_t bytes);
/* hjgpu_malloc with the placement search of the library's own workspace (option "placement": up to 12 candidate blocks
 * are held and filled, the fastest is kept; buffers below 1 GiB: plain hjgpu_malloc): for buffers of a gigabyte and more
 * that a join writes into at many places at once - the result columns of a materialising join (its time differs by up
 * to 13 % between allocations of the same columns).  The search's wall clock is added to hjgpu_stats.ms_reserve. */
int  hjgpu_malloc_placed(hjgpu_ctx *ctx, void **d_ptr, size_t bytes);
int  hjgpu_free(hjgpu_ctx *ctx, void *d_ptr);
int  hjgpu_memcpy_h2d(hjgpu_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int  hjgpu_memcpy_d2h(hjgpu_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int  hjgpu_synchronize(hjgpu_ctx *ctx, void *stream);
/* Page-locked host memory for the fread() targets of the host programs (the reference's
 * mamalloc'd columns, npj.cpp:982-1000): hjgpu_join_host DMAs such columns straight to HBM at
 * the PCIe rate; pageable columns are staged through two pinned buffers instead. */
int  hjgpu_host_alloc(hjgpu_ctx *ctx, void **h_ptr, size_t bytes);
int  hjgpu_host_free(hjgpu_ctx *ctx, void *h_ptr);

/* ---- partition operators ------------------------------------------------------ */
/* histogram(), phj.cpp:693 (shared form 773): d_counts[p] = |{i: H(key_i,f,F)=p}|. */
int  hjgpu_histogram(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n,
                     uint32_t factor, uint32_t fanout, uint64_t *d_counts, void *stream);
/* histogram() + interleave() + partition() (phj.cpp:693, 1263, 1029): permutes
 * (key, payload) so that partition p occupies [d_offsets[p], d_offsets[p+1]);
 * order inside a partition is unspecified, as in the reference.
 * d_offsets: fanout+1 uint64 (64-bit: SURVEY F10). */
int  hjgpu_partition(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                     uint32_t factor, uint32_t fanout,
                     uint32_t *d_keys_out, uint32_t *d_vals_out, uint64_t *d_offsets,
                     void *stream);
/* Enqueue-only form (no host synchronisation; d_offsets is valid once `stream` has reached this point):
 * the exchange-level partitioning of the multi-GPU CPRA keeps several GPUs busy from one host thread. */
int  hjgpu_partition_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                           uint32_t factor, uint32_t fanout,
                           uint32_t *d_keys_out, uint32_t *d_vals_out, uint64_t *d_offsets,
                           void *stream);
/* build()+probe() over co-partitioned relations (phj.cpp:307, 399; the commented
 * join loop phj.cpp:1869-1924 / live cpra2.cpp:1883-1971): for every partition p,
 * R rows [d_inner_offsets[p], [p+1]) are loaded into an LDS hash table and S rows
 * [d_outer_offsets[p], [p+1]) probe it.  (factor1, fanout1, factor2, fanout2)
 * must be the passes that produced the partitions (needed to pick a per-partition
 * empty sentinel, phj.cpp:1886-1897; fanout2 = 1 for a single pass).
 * The offsets need not start at 0 nor end where the columns do: only rows [d_*_offsets[0], d_*_offsets[P]) of a relation take
 * part, whatever lies in front of and behind them (P = fanout1 * fanout2; P + 1 non-decreasing offsets per relation). */
int  hjgpu_join_partitions(hjgpu_ctx *ctx,
                           const uint32_t *d_inner_keys, const uint32_t *d_inner_vals,
                           const uint64_t *d_inner_offsets,
                           const uint32_t *d_outer_keys, const uint32_t *d_outer_vals,
                           const uint64_t *d_outer_offsets,
                           const hjgpu_phj_params *passes,
                           hjgpu_result *result, const hjgpu_output *out, void *stream);

/* ---- NPJ operators ------------------------------------------------------------- */
/* set()+build(), npj.cpp:366, 190: d_table = uint64[buckets] of (val<<32)|key. */
int  hjgpu_npj_build(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                     uint64_t *d_table, size_t buckets, uint32_t factor, void *stream);
/* probe()+close_gaps(), npj.cpp:216, 475. */
int  hjgpu_npj_probe(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                     const uint64_t *d_table, size_t buckets, uint32_t factor,
                     hjgpu_result *result, const hjgpu_output *out, void *stream);

/* ---- NPJ positional look-up (dimension look-up, S.key.map(R)) -------------------------
 * For every probe key d_outer_keys[i], i in [0, outer), IN THE PROBE COLUMN'S ORDER - NPJ never reorders the probe side; no
 * probe payload column is read, nothing goes through the block protocol or close_gaps:
 *   d_vals_out[i]    the payload of a build tuple whose key equals d_outer_keys[i]: the FIRST one the walk meets (with duplicated
 *                    build keys which copy that is depends on insertion order and is unspecified, as under HJGPU_FLAG_UNIQUE);
 *                    HJGPU_NULL_VAL when no build key equals it.  No element at index >= outer is written.
 *   d_match_bits     bit i & 31 (counted from the least significant) of word i >> 5 is 1 exactly when probe key i has a match -
 *                    what tells a NULL from a genuine build payload 0xFFFFFFFF.  (outer + 31) / 32 words: the bits of the last
 *                    word at positions >= outer are written 0, no word at index >= (outer + 31) / 32 is written.
 * Either output may be NULL: the bits alone are the semi-join mask in probe order, the values alone the plain map, and with both
 * NULL the call returns the aggregates only.
 *   result           count = the probe tuples with a match, sum_keys = the sum of their keys, sum_outer_vals = 0 (there is no probe
 *                    payload), sum_inner_vals = the sum of the looked-up payloads (a NULL adds 0).
 * Keys, as for NPJ everywhere: a build key 0 is HJGPU_EZEROKEY (the blocking form returns it; after the _async form
 * hjgpu_get_async_status / hjgpu_accumulate_async_status report it), a probe key 0 matches nothing (NULL, bit 0).  inner == 0: every
 * value NULL, every bit 0, count 0.  outer == 0: nothing is written.
 * Refusals: d_outer_keys, d_vals_out and d_match_bits must be 16-byte aligned (HJGPU_EALIGN), as the build columns; a capturing
 * stream is HJGPU_EINVAL as everywhere.  params->flags: HJGPU_FLAG_UNIQUE is ignored (the look-up is first-match by definition), any
 * join-mode flag (HJGPU_FLAG_SEMI ... HJGPU_FLAG_RIGHT_ANTI) is HJGPU_EINVAL naming the flag.  load and factor mean what they mean
 * for hjgpu_npj; option "npj_refhash" selects the reference-hash table and its walk, as for whole joins.
 * hjgpu_get_stats afterwards: ms_build, ms_join, ms_total and buckets as after hjgpu_npj, ms_close_gaps 0.  The _async form is
 * enqueue-only under hjgpu_npj_async's rules (d_result in device memory, workspace reserved with hjgpu_reserve). */
int  hjgpu_npj_lookup(hjgpu_ctx *ctx,
                      const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                      const uint32_t *d_outer_keys, size_t outer,
                      const hjgpu_npj_params *params,
                      uint32_t *d_vals_out,      /* outer uint32, or NULL */
                      uint32_t *d_match_bits,    /* (outer + 31) / 32 uint32, or NULL */
                      hjgpu_result *result, void *stream);
int  hjgpu_npj_lookup_async(hjgpu_ctx *ctx,
                            const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                            const uint32_t *d_outer_keys, size_t outer,
                            const hjgpu_npj_params *params,
                            uint32_t *d_vals_out, uint32_t *d_match_bits,
                            hjgpu_result *d_result, void *stream);
/* The same look-up in a table that hjgpu_npj_build made (the reference's table format and hash): build once, look up any number
 * of batches.  buckets and factor as given to hjgpu_npj_build (which reports a build key 0 itself); blocking.  The table must hold
 * an empty bucket (hjgpu_npj_build: buckets > n), or the walk of an absent key never ends. */
int  hjgpu_npj_lookup_table(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n,
                            const uint64_t *d_table, size_t buckets, uint32_t factor,
                            uint32_t *d_vals_out, uint32_t *d_match_bits,
                            hjgpu_result *result, void *stream);

/* ---- positional look-up, road chosen by the build side's size ---------------------------
 * hjgpu_npj_lookup's contract, word for word: d_vals_out, d_match_bits, the aggregates, either output may be NULL, nothing is written
 * at index >= outer / at word >= (outer + 31) / 32, the last word's high bits are 0; a build key 0 is HJGPU_EZEROKEY (the blocking
 * form returns it, hjgpu_get_async_status / hjgpu_accumulate_async_status report it after the _async form), a probe key 0 matches
 * nothing, inner == 0 gives all NULL and all bits 0; d_outer_keys, d_vals_out and d_match_bits 16-byte aligned (HJGPU_EALIGN); any
 * join-mode flag is HJGPU_EINVAL naming the flag, HJGPU_FLAG_UNIQUE is ignored; a capturing stream is refused.
 * The road: a build side of at most L rows - L = hjgpu_get_counter(ctx, "lookup_lds_rows"): the largest build side of a
 * broadcast join; 0 under option "no_broadcast" - takes the LDS look-up: every workgroup of one persistent grid keeps the whole
 * build side in a hash table of its own in LDS and streams the probe column once; ONE launch.  params->load and params->factor are
 * ignored there.  Every larger build side is hjgpu_npj_lookup with `params`, exactly.
 * Duplicated build keys: which copy answers is unspecified, as for hjgpu_npj_lookup; on the LDS road two POSITIONS with the same probe
 * key may even receive different copies, because every workgroup fills its own table.
 * hjgpu_get_stats after the LDS road: fanout1 = fanout2 = 1 and buckets = 0 (as after a broadcast join: how a caller sees which road
 * ran), ms_build 0, ms_close_gaps 0, ms_join the kernel; the clear of the device state that precedes the kernel is counted in
 * ms_histogram (a few microseconds, as after a broadcast join) and in ms_total. */
int  hjgpu_lookup(hjgpu_ctx *ctx,
                  const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                  const uint32_t *d_outer_keys, size_t outer,
                  const hjgpu_npj_params *params,
                  uint32_t *d_vals_out,      /* outer uint32, or NULL */
                  uint32_t *d_match_bits,    /* (outer + 31) / 32 uint32, or NULL */
                  hjgpu_result *result, void *stream);
int  hjgpu_lookup_async(hjgpu_ctx *ctx,
                        const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                        const uint32_t *d_outer_keys, size_t outer,
                        const hjgpu_npj_params *params,
                        uint32_t *d_vals_out, uint32_t *d_match_bits,
                        hjgpu_result *d_result, void *stream);

/* ---- selected positional look-up: a bitmap of the rows to look up ----------------------
 * hjgpu_lookup / hjgpu_lookup_async / hjgpu_npj_lookup_table with an input bitmap in d_match_bits' layout - what the next dimension
 * of a star query takes from the one before it: only the rows whose bit is set are looked up, and an unselected row costs no table
 * access.  The contract is the plain entry point's, word for word, plus:
 *   d_select_bits    (outer + 31) / 32 words; bit i & 31 of word i >> 5 says whether row i is selected.  Bits of the last word at
 *                    positions >= outer are ignored (they may hold anything), no word at index >= (outer + 31) / 32 is read.  16-byte
 *                    aligned (HJGPU_EALIGN).  NULL: every row is selected - the call IS the plain entry point, same kernels.
 *   an unselected row i: d_vals_out[i] = HJGPU_NULL_VAL, match bit 0, counted in no aggregate.
 *   a selected row: exactly what the plain look-up gives it.
 *   result           count, sum_keys and sum_inner_vals over the selected rows with a match; sum_outer_vals 0.
 *   in place         d_match_bits may be the very pointer d_select_bits: afterwards the bitmap is select AND match (the last word's high
 *                    bits 0), so a chain of dimensions narrows ONE bitmap.  Any other overlap of the two bitmaps is HJGPU_EINVAL.
 * A build key 0 is HJGPU_EZEROKEY whatever the mask says; outer == 0: nothing is written and nothing is read of the mask.  The road
 * is chosen by `inner` alone, as for hjgpu_lookup; hjgpu_get_stats tells the roads apart as there. */
int  hjgpu_lookup_selected(hjgpu_ctx *ctx,
                           const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                           const uint32_t *d_outer_keys, size_t outer,
                           const hjgpu_npj_params *params,
                           const uint32_t *d_select_bits,   /* (outer + 31) / 32 uint32, or NULL */
                           uint32_t *d_vals_out, uint32_t *d_match_bits,
                           hjgpu_result *result, void *stream);
int  hjgpu_lookup_selected_async(hjgpu_ctx *ctx,
                                 const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                                 const uint32_t *d_outer_keys, size_t outer,
                                 const hjgpu_npj_params *params,
                                 const uint32_t *d_select_bits,
                                 uint32_t *d_vals_out, uint32_t *d_match_bits,
                                 hjgpu_result *d_result, void *stream);
int  hjgpu_npj_lookup_table_selected(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n,
                                     const uint64_t *d_table, size_t buckets, uint32_t factor,
                                     const uint32_t *d_select_bits,
                                     uint32_t *d_vals_out, uint32_t *d_match_bits,
                                     hjgpu_result *result, void *stream);

/* ---- wide positional look-up: two to four key columns -----------------------------------
 * hjgpu_lookup_selected for ON a.k0 = b.k0 AND a.k1 = b.k1 (AND ...): a (partkey, suppkey) dimension, a (year, week) calendar, a
 * (store, item) price list.  With the row number as the build payload and hjgpu_gather_selected behind it, it is a composite-key N:1 join.
 * The contract is hjgpu_lookup_selected's wherever the two meet:
 *   outputs          d_vals_out[i] (NULL: none) = the payload of a build row whose nkeys key values equal probe row i's, position by
 *                    position - (a, b) does not match (b, a) -, bit i of d_match_bits (NULL: none) = there is one; HJGPU_NULL_VAL and bit 0
 *                    for a row that is unselected or unmatched.  No element at index >= outer and no word at index >= (outer + 31) / 32 is
 *                    written; the last word's high bits are 0.
 *   d_select_bits    (outer + 31) / 32 words; bit i & 31 of word i >> 5 says whether row i is selected.  Bits of the last word at
 *                    positions >= outer are ignored (they may hold anything), no word at index >= (outer + 31) / 32 is read.  NULL: every
 *                    row is selected.  An unselected row costs no table access and is counted in no aggregate.
 *   in place         d_match_bits may be the very pointer d_select_bits: afterwards the bitmap is select AND match (the last word's high
 *                    bits 0).  Any other overlap of the two bitmaps is HJGPU_EINVAL.
 *   empty sides      outer == 0: nothing is written and nothing is read.  inner == 0: every row gets HJGPU_NULL_VAL and bit 0, count 0.
 *   stream           a capturing stream is HJGPU_EINVAL.
 *   refusals         every refusal is decided from the arguments alone, before anything is allocated or enqueued.
 * What is the wide look-up's own:
 *   nkeys            2, 3 or 4 (HJGPU_LOOKUP_WIDE_MIN_KEYS .. _MAX_KEYS); 0, 1 and 5 are HJGPU_EINVAL ("nkeys" in hjgpu_last_error; one key
 *                    column is hjgpu_lookup_selected).  d_inner_keys and d_outer_keys are HOST arrays of nkeys device pointers, copied by
 *                    value: build columns of `inner` values, probe columns of `outer` values.  The same column may be given twice.
 *   key values       every value is legal in every key column on both sides, 0 and 0xFFFFFFFF included: this call never returns
 *                    HJGPU_EZEROKEY.
 *   duplicates       which copy of a duplicated build tuple answers is unspecified; within one call every position with the same probe
 *                    tuple receives the SAME copy (one table, one walk).
 *   result           count = the selected rows with a match, sum_keys = the sum of key column 0 over them, sum_outer_vals = 0,
 *                    sum_inner_vals = the sum of the looked-up payloads.  `result` is host memory, `d_result` (the _async form) 32 bytes of
 *                    16-byte aligned device memory; either may be NULL.
 *   params           load sizes the table: slots = max(16, inner + 1, floor(inner / load)) rounded up to a multiple of 8; 0 = 0.5; load >
 *                    0.99 is HJGPU_EINVAL.  factor and HJGPU_FLAG_UNIQUE are ignored.  Any join-mode flag is HJGPU_EINVAL naming the flag.
 *   alignment        every column, the mask, both outputs and d_result are 16-byte aligned (HJGPU_EALIGN).
 *   overlap          a written operand (d_vals_out, d_match_bits, d_result) that shares a byte with a read operand or with another written
 *                    one is HJGPU_EINVAL ("overlaps"); the one declared in-place pair is d_match_bits on d_select_bits.
 *   state            the table and the aggregate words are a workspace of the call's own in the context, grown the first time a size is
 *                    seen (either form; counted in ms_reserve).  The call touches neither the NPJ table, nor a prepared build side
 *                    (hjgpu_phj_build), nor what hjgpu_get_async_status / hjgpu_accumulate_async_status report.  The _async form only
 *                    enqueues and needs no hjgpu_reserve; calls may be queued back to back on one stream of one context.
 *   hjgpu_get_stats  afterwards: ms_histogram = the clear of the table and the build, ms_join = the look-up kernel, ms_total = all of it,
 *                    ms_close_gaps = 0, fanout1 = fanout2 = groups = 0, buckets = the table's slots.  hjgpu_get_counter
 *                    "lookup_wide_step_rows": the rows the look-up's whole grid covers in one iteration of its loop. */
#define HJGPU_LOOKUP_WIDE_MIN_KEYS 2u
#define HJGPU_LOOKUP_WIDE_MAX_KEYS 4u
int  hjgpu_lookup_wide(hjgpu_ctx *ctx, uint32_t nkeys,
                       const uint32_t *const *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                       const uint32_t *const *d_outer_keys, size_t outer,
                       const hjgpu_npj_params *params,
                       const uint32_t *d_select_bits,   /* (outer + 31) / 32 uint32, or NULL: every row */
                       uint32_t *d_vals_out, uint32_t *d_match_bits,   /* either may be NULL */
                       hjgpu_result *result, void *stream);
int  hjgpu_lookup_wide_async(hjgpu_ctx *ctx, uint32_t nkeys,
                             const uint32_t *const *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                             const uint32_t *const *d_outer_keys, size_t outer,
                             const hjgpu_npj_params *params,
                             const uint32_t *d_select_bits,
                             uint32_t *d_vals_out, uint32_t *d_match_bits,
                             hjgpu_result *d_result, void *stream);

/* ---- filter: range predicates over up to 4 columns into a bitmap --------------------------------------------
 * What makes, or narrows, a bitmap in d_match_bits' layout from the fact table's own columns - lo_discount BETWEEN 1 AND 3 AND lo_quantity
 * < 25, a date range, a status code - and from a looked-up value column (d_year BETWEEN 1992 AND 1997): the other half of a star query's
 * WHERE clause, in front of, between and behind the selected look-ups.  Row i < n PASSES when it is selected and every predicate p < npreds
 * holds on d_cols[p][i]:
 *   a predicate      {lo, hi, flags, reserved} holds on x when lo <= x <= hi, BOTH ENDS INCLUSIVE; the compare is unsigned, or - HJGPU_PRED_SIGNED
 *                    - lo, hi and the column are int32 (two's complement order).  HJGPU_PRED_NOT inverts the predicate: the rows outside
 *                    [lo, hi] pass.  lo > hi in the predicate's order is the empty range and is legal: nothing passes, or everything under
 *                    HJGPU_PRED_NOT.  Equality is lo == hi, "x < c" is [0, c - 1] (signed: [INT32_MIN, c - 1]).  A flag bit outside the two
 *                    defined, or reserved != 0, is HJGPU_EINVAL.
 *   HJGPU_NULL_VAL   in a looked-up column is the ordinary value 0xFFFFFFFF: an unsigned range with hi < 0xFFFFFFFF drops the unmatched rows, a
 *                    signed one sees them as -1.
 *   d_bits_out       (n + 31) / 32 words in d_match_bits' layout: bit i & 31 of word i >> 5 is 1 exactly when row i passes.  The last word's
 *                    bits at positions >= n are written 0, no word at index >= (n + 31) / 32 is written.  16-byte aligned (HJGPU_EALIGN).
 *   count            *count (blocking form, host memory) / *d_count (_async form, device memory, 8-byte aligned: HJGPU_EALIGN) = the number
 *                    of passing rows, exact.  Either d_bits_out or the count may be NULL - the count alone, the bitmap alone -; both NULL
 *                    with n > 0 is HJGPU_EINVAL.
 *   d_select_bits    hjgpu_lookup_selected's mask, word for word: (n + 31) / 32 words, bit i & 31 of word i >> 5 selects row i, bits of the
 *                    last word at positions >= n are ignored, no word at index >= (n + 31) / 32 is read.  16-byte aligned (HJGPU_EALIGN).
 *                    NULL selects every row.
 *   in place         d_bits_out may be the very pointer d_select_bits: afterwards the bitmap is select AND pass (the last word's high bits
 *                    0), as the selected look-ups narrow theirs.  Any other overlap of the two bitmaps is HJGPU_EINVAL.
 *   d_cols, preds    HOST arrays of npreds entries, copied by value into the kernel arguments.  npreds is 1 to HJGPU_FILTER_MAX_PREDS; 0,
 *                    more, and a NULL column among the first npreds are HJGPU_EINVAL.  The same column may appear twice (two ranges on one
 *                    column, for example two HJGPU_PRED_NOT ranges).  Columns hold n uint32 and are 16-byte aligned (HJGPU_EALIGN); no row
 *                    at n or beyond is read, except inside a column's last 16-byte vector.  Columns and the mask are never written.
 *   order            the predicates are evaluated in the caller's order, and column p >= 1 is read only where a row of its 128-byte line
 *                    has passed the mask and predicates 0 ... p - 1: MOST SELECTIVE FIRST.  The result does not depend on the order.
 *   overlap          d_bits_out's bytes, or the _async form's count word, that overlap a column's [p, p + 4 * n) or each other (the count
 *                    word: or the mask): HJGPU_EINVAL, "overlaps" in hjgpu_last_error.
 *   n == 0           reads nothing, writes nothing but the count (0), accepts NULL everywhere else.
 * OR between predicates is one elementwise OR of two bitmaps, which the caller has; an IN-list is a look-up.
 * Every refusal is decided from the arguments alone, before anything is enqueued or allocated; a capturing stream is HJGPU_EINVAL.  Neither
 * form touches what hjgpu_get_async_status / hjgpu_accumulate_async_status report.  The _async form only enqueues and needs no
 * hjgpu_reserve: the only workspace is one count word per context, made the first time either form runs, so calls may be queued back to
 * back on one stream of one context.  Two enqueues ordered by the stream - the clear of the count word, then ONE kernel on a persistent grid
 * that streams the mask and the columns once - and no workgroup waits for another.  hjgpu_get_stats afterwards: ms_total = both,
 * ms_histogram = the clear, ms_join = the kernel, every other phase 0, fanout1 = fanout2 = buckets = groups = 0.  hjgpu_get_counter
 * "filter_step_rows": the rows the whole grid covers in one iteration of its loop. */
#define HJGPU_FILTER_MAX_PREDS 4u
#define HJGPU_PRED_NOT    1u   /* the rows OUTSIDE [lo, hi] pass */
#define HJGPU_PRED_SIGNED 2u   /* lo, hi and the column are int32 (two's complement order) */
typedef struct { uint32_t lo, hi, flags, reserved; } hjgpu_predicate;
int  hjgpu_filter_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                           uint32_t npreds, const uint32_t *const *d_cols, const hjgpu_predicate *preds,
                           uint32_t *d_bits_out, uint64_t *count, void *stream);
int  hjgpu_filter_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                                 uint32_t npreds, const uint32_t *const *d_cols, const hjgpu_predicate *preds,
                                 uint32_t *d_bits_out, uint64_t *d_count, void *stream);

/* ---- gather by row number: up to 4 columns fetched by an index column, under a bitmap ------------------------
 * What turns a row number back into column values - the positional look-up whose table is an array.  A look-up or a join carries ONE
 * 32-bit payload per side; when that payload is the row number (a dimension's row in hjgpu_lookup_selected's build payload, a relation's
 * row in hjgpu_phj's payload columns, hjgpu_compact_selected's d_rows_out), this call fetches any further columns of that row: the second
 * attribute of a dimension (filter on c_region, group by c_nation), the other columns of a join's result rows.  Its contract is
 * hjgpu_lookup_selected's wherever the two meet.  For every row i < n, in position (output row i belongs to input row i):
 *   a gathered row   row i is GATHERED when it is selected and d_idx[i] < src_rows.  Then d_cols_out[c][i] = d_src_cols[c][d_idx[i]] for
 *                    every c < ncols, and bit i of d_bits_out is 1.
 *   every other row  gets HJGPU_NULL_VAL in every output column and bit 0, and NO SOURCE ELEMENT IS READ FOR IT: an unselected row,
 *                    whatever its index holds (garbage is legal there and is not counted); a selected row whose index is HJGPU_NULL_VAL -
 *                    the NULL of a look-up or of an outer join passes through -; a selected row whose index is out of range, that is
 *                    >= src_rows and not HJGPU_NULL_VAL.  No index, whatever it holds, makes the call read outside a source column.
 *                    Every element < n of every output column is written, and nothing at n or beyond.
 *   d_bits_out       (n + 31) / 32 words in d_match_bits' layout: bit i & 31 of word i >> 5 is 1 exactly when row i is gathered - what
 *                    tells a NULL from a genuine 0xFFFFFFFF in a source column.  The last word's bits at positions >= n are written 0,
 *                    no word at index >= (n + 31) / 32 is written.  16-byte aligned (HJGPU_EALIGN).  It may be NULL.
 *   counts           counts[0] = the gathered rows, counts[1] = the out-of-range rows, both exact: host memory in the blocking form,
 *                    device memory (two words, 16-byte aligned: HJGPU_EALIGN) in the _async form.  May be NULL.
 *   HJGPU_ERANGE     the blocking form returns it when counts[1] != 0 - also when counts is NULL: it reads the context's own count
 *                    words.  All outputs are still written completely and validly, as HJGPU_EOVERFLOW leaves a valid prefix.  The _async
 *                    form cannot report it: its caller reads d_counts[1].
 *   d_select_bits    hjgpu_lookup_selected's mask, word for word: (n + 31) / 32 words, bit i & 31 of word i >> 5 selects row i, bits of the
 *                    last word at positions >= n are ignored, no word at index >= (n + 31) / 32 is read.  16-byte aligned (HJGPU_EALIGN).
 *                    NULL selects every row.
 *   d_idx            n uint32 row numbers, 16-byte aligned (HJGPU_EALIGN); no row at n or beyond is read, except inside the last 16-byte
 *                    vector.  The 32 rows of a mask word that is 0 are not read at all.
 *   sources          d_src_cols[c] holds src_rows uint32, 16-byte aligned (HJGPU_EALIGN), and is never written.  src_rows <= 0xFFFFFFFF -
 *                    larger is HJGPU_EINVAL: an index is a uint32, and HJGPU_NULL_VAL must never be a legal one.  src_rows == 0 is legal:
 *                    nothing is gathered and no source byte is read.  The same source column may be given twice.
 *   d_src_cols,      HOST arrays of ncols entries, copied by value into the kernel arguments.  ncols is 1 to HJGPU_GATHER_MAX_COLS; 0,
 *   d_cols_out       more, and a NULL entry among the first ncols of either array are HJGPU_EINVAL.  Output columns hold n uint32 and are
 *                    16-byte aligned (HJGPU_EALIGN).
 *   in place         d_bits_out may be the very pointer d_select_bits: afterwards the bitmap is select AND gathered, as the selected
 *                    look-ups narrow theirs.  At most one output column may be the very pointer d_idx: the row numbers are replaced by
 *                    the values.
 *   overlap          any other overlap is HJGPU_EINVAL, "overlaps" in hjgpu_last_error: an output column with the index, another output
 *                    column, a source column or the mask; d_bits_out with anything but the very pointer d_select_bits; the _async
 *                    form's count words with anything.
 *   n == 0           reads nothing, writes nothing but the counts (0, 0), accepts NULL everywhere else.
 * Every refusal is decided from the arguments alone, before anything is enqueued or allocated; a capturing stream is HJGPU_EINVAL.  Neither
 * form touches what hjgpu_get_async_status / hjgpu_accumulate_async_status report.  The _async form only enqueues and needs no
 * hjgpu_reserve: the only workspace is two count words per context, made the first time either form runs, so calls may be queued back to
 * back on one stream of one context.  Two enqueues ordered by the stream - the clear of the count words, then ONE kernel on a persistent
 * grid that streams the mask and the index once and fetches the source elements with ordinary cached loads - and no workgroup waits for
 * another.  hjgpu_get_stats afterwards: ms_total = both, ms_histogram = the clear, ms_join = the kernel, every other phase 0, fanout1 =
 * fanout2 = buckets = groups = 0.  hjgpu_get_counter "gather_step_rows": the rows the whole grid covers in one iteration of its loop.
 * More than HJGPU_GATHER_MAX_COLS columns are further calls, each of which reads the index again. */
#define HJGPU_GATHER_MAX_COLS 4u
#define HJGPU_ERANGE 9   /* gather: a selected row's index is neither HJGPU_NULL_VAL nor below src_rows */
int  hjgpu_gather_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, const uint32_t *d_idx, size_t n,
                           uint32_t ncols, const uint32_t *const *d_src_cols, size_t src_rows,
                           uint32_t *const *d_cols_out, uint32_t *d_bits_out,
                           uint64_t counts[2], void *stream);
int  hjgpu_gather_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, const uint32_t *d_idx, size_t n,
                                 uint32_t ncols, const uint32_t *const *d_src_cols, size_t src_rows,
                                 uint32_t *const *d_cols_out, uint32_t *d_bits_out,
                                 uint64_t *d_counts, void *stream);

/* ---- compaction by bitmap: the selected rows of up to 8 columns, dense and in order ----------------------
 * What turns a bitmap in d_match_bits' layout and full-length columns into dense rows - at the end of a chain of selected look-ups (the
 * bitmap and the K value columns become the result rows) and in front of a join (a filter bitmap and the probe columns become the dense
 * probe columns that hjgpu_phj / hjgpu_npj take; the row numbers can ride along as the payload).  Ordered (stable), so the output is
 * bit-for-bit reproducible.  Let the selected rows be i_0 < i_1 < ... < i_(J-1):
 *   d_cols_out[c][j] = d_cols_in[c][i_j] and d_rows_out[j] = (uint32_t) i_j for j < min(J, capacity); nothing is written at index
 *   >= min(J, capacity) of any output; the mask and the input columns are never written.
 *   d_select_bits    hjgpu_lookup_selected's mask, word for word: (n + 31) / 32 words, bit i & 31 of word i >> 5 selects row i, bits of the
 *                    last word at positions >= n are ignored, no word at index >= (n + 31) / 32 is read.  16-byte aligned (HJGPU_EALIGN).
 *                    NOT NULL when n > 0 (HJGPU_EINVAL; unlike the look-ups: a compaction of every row is a copy, which the caller has).
 *   d_cols_in, d_cols_out   HOST arrays of ncols device pointers, copied by value into the kernel arguments.  ncols may be 0;
 *                    ncols > HJGPU_COMPACT_MAX_COLS and a NULL entry among the first ncols of either array are HJGPU_EINVAL.  The same
 *                    input column may be given twice.  No row at n or beyond is read of any input.
 *   d_rows_out       the selected row numbers, or NULL.  With it, n > 0xFFFFFFFF is HJGPU_EINVAL; without it any n is legal.  ncols == 0
 *                    with d_rows_out: the positions alone; without: the count alone (capacity is then ignored).
 *   count            *count (blocking form, host memory) / *d_count (_async form, device memory, 8-byte aligned: HJGPU_EALIGN) = J, exact
 *                    whatever capacity is.
 *   overflow         J > capacity: the blocking form returns HJGPU_EOVERFLOW with *count = J, and the first `capacity` rows of every output
 *                    are valid (the order makes that well defined).  The _async form cannot report it: its caller compares *d_count with
 *                    capacity.  Neither form touches what hjgpu_get_async_status / hjgpu_accumulate_async_status report: those belong to
 *                    the context's last join.
 *   alignment        every input column, output column and d_rows_out 16-byte aligned (HJGPU_EALIGN).
 *   not in place     an output's bytes [p, p + 4 * capacity) that overlap the mask, an input column's [p, p + 4 * n) or another output:
 *                    HJGPU_EINVAL, "overlaps" in hjgpu_last_error.
 *   n == 0           reads nothing, writes nothing but the count (0), accepts NULL everywhere else.
 * Every refusal is decided from the arguments alone, before anything is enqueued or allocated; a capturing stream is HJGPU_EINVAL.  The
 * _async form only enqueues and needs no hjgpu_reserve: the only workspace is a constant-size buffer of a few KiB per context, made the
 * first time either form runs, so several compactions may be queued back to back on one stream of one context (one context per stream,
 * as everywhere).  Two launches ordered by the stream - a count over the mask alone, then the compaction - and no workgroup waits for
 * another.  hjgpu_get_stats afterwards: ms_total = both launches, ms_histogram = the counting launch, ms_join = the compaction, every
 * other phase 0, fanout1 = fanout2 = buckets = groups = 0.  hjgpu_get_counter "compact_ranges" / "compact_chunk_rows": the geometry -
 * the rows are cut into that many contiguous ranges of whole chunks of that many rows (one workgroup each, the tail in the last
 * non-empty one). */
#define HJGPU_COMPACT_MAX_COLS 8u
int  hjgpu_compact_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                            uint32_t ncols, const uint32_t *const *d_cols_in, uint32_t *const *d_cols_out,
                            uint32_t *d_rows_out, size_t capacity, uint64_t *count, void *stream);
int  hjgpu_compact_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                                  uint32_t ncols, const uint32_t *const *d_cols_in, uint32_t *const *d_cols_out,
                                  uint32_t *d_rows_out, size_t capacity, uint64_t *d_count, void *stream);

/* ---- grouped aggregation: GROUP BY one or two columns, COUNT(*) and up to four SUMs over a bitmap's rows -------
 * What ends a chain of selected look-ups: the bitmap says which rows count, the looked-up value columns are the group keys in place, and
 * the answer is a few thousand rows.  The selected rows i are grouped by the tuple (d_keys_in[0][i] [, d_keys_in[1][i]]); for every
 * distinct tuple there is exactly one output index j < J:
 *   d_keys_out[c][j] = the tuple's column c, d_counts_out[j] = the number of its selected rows, d_sums_out[v][j] = the sum of
 *   d_vals_in[v][i] over them in uint64 modulo 2^64.  The ORDER of the groups is unspecified, as the order of a join's rows is; counts and
 *   sums are exact integers, so the set of (tuple, count, sums) is reproducible bit for bit.
 *   d_select_bits    hjgpu_lookup_selected's mask, word for word: (n + 31) / 32 words, bit i & 31 of word i >> 5 selects row i, bits of the
 *                    last word at positions >= n are ignored, no word at index >= (n + 31) / 32 is read.  16-byte aligned (HJGPU_EALIGN).
 *                    NULL selects every row (unlike the compaction: an aggregate over all rows is a real query).
 *   key values       every key value is legal, 0 and 0xFFFFFFFF included; HJGPU_NULL_VAL from an unmatched but selected row is an
 *                    ordinary group.
 *   d_keys_in, d_vals_in, d_keys_out, d_sums_out   HOST arrays of nkeys / nvals device pointers, copied by value into the kernel
 *                    arguments; input columns hold n uint32, d_keys_out columns capacity uint32, d_sums_out columns capacity uint64.
 *                    nkeys is 1 or 2, nvals 0 to 4 (0: counts only; the value arrays may then be NULL).  nkeys == 0,
 *                    nkeys > HJGPU_GROUP_MAX_KEYS, nvals > HJGPU_GROUP_MAX_VALS and a NULL entry among the first nkeys / nvals of an
 *                    array are HJGPU_EINVAL.  The same input column may be given twice.
 *   d_counts_out     capacity uint64, or NULL: no counts.
 *   count            *ngroups (blocking form, host memory) / *d_ngroups (_async form, device memory, 8-byte aligned: HJGPU_EALIGN) = J.
 *   overflow         J > capacity: the blocking form returns HJGPU_EOVERFLOW, and *ngroups is then a lower bound of J that is greater than
 *                    capacity (J itself while the merge table holds every group: it has at least twice capacity slots).  Nothing at index
 *                    >= capacity is written; the contents below capacity are unspecified.  The _async form's caller compares *d_ngroups
 *                    with capacity.  Neither form touches what hjgpu_get_async_status / hjgpu_accumulate_async_status report.
 *                    capacity == 0 is legal: an overflow unless J is 0.  capacity > 2^40 is HJGPU_EINVAL.
 *   alignment        every input column, every output column and the mask 16-byte aligned (HJGPU_EALIGN).
 *   overlap          an output's byte range (the _async form's count word included) that overlaps the mask, an input column or another
 *                    output: HJGPU_EINVAL, "overlaps" in hjgpu_last_error.  The mask and the inputs are never written; no input row at n
 *                    or beyond is read, except inside the last 16-byte vector of a column.
 *   n == 0           reads nothing, writes nothing but the count (0), accepts NULL everywhere else.
 * Every refusal is decided from the arguments alone, before anything is enqueued or allocated; a capturing stream is HJGPU_EINVAL.  Calls
 * on one stream of one context may be queued back to back.  The workspace is the merge table in the context, sized from capacity (a power
 * of two of at least 2 * capacity and at least 1024 slots of 48 bytes); it grows the first time a capacity is seen (hjgpu_stats.ms_reserve).
 * Three enqueues ordered by the stream - the clears, the aggregation (one pass over the mask, the key and the measure columns; each
 * workgroup pre-aggregates in an LDS table and adds what it holds to the merge table), the emit - and no workgroup waits for another.
 * hjgpu_get_stats afterwards: ms_total = all launches, ms_histogram = the clears, ms_join = the aggregation, ms_close_gaps = the emit,
 * every other phase 0, fanout1 = fanout2 = buckets = groups = 0.  hjgpu_get_counter "group_lds_groups": the distinct groups a
 * workgroup's LDS table holds; correctness never depends on the number of groups. */
#define HJGPU_GROUP_MAX_KEYS 2u
#define HJGPU_GROUP_MAX_VALS 4u
int  hjgpu_group_sum(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                     uint32_t nkeys, const uint32_t *const *d_keys_in, uint32_t nvals, const uint32_t *const *d_vals_in,
                     uint32_t *const *d_keys_out, uint64_t *d_counts_out, uint64_t *const *d_sums_out,
                     size_t capacity, uint64_t *ngroups, void *stream);
int  hjgpu_group_sum_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                           uint32_t nkeys, const uint32_t *const *d_keys_in, uint32_t nvals, const uint32_t *const *d_vals_in,
                           uint32_t *const *d_keys_out, uint64_t *d_counts_out, uint64_t *const *d_sums_out,
                           size_t capacity, uint64_t *d_ngroups, void *stream);

/* ---- aggregate functions: GROUP BY nothing, one or two columns; COUNT(*) and up to four of SUM(a), SUM(a * b), MIN(a), MAX(a) -------
 * hjgpu_group_sum's contract, word for word, wherever the two meet: d_select_bits (and NULL: every row), every key value legal and the
 * groups in unspecified order, n == 0, the count, overflow and *ngroups, alignment, the overlap refusals, the capturing stream, refusals
 * decided from the arguments alone before anything is allocated or enqueued, the untouched async status, calls queued back to back on
 * one stream.  On top of it:
 *   nkeys            0, 1 or 2 (more: HJGPU_EINVAL).  nkeys == 0 is the scalar aggregate - no GROUP BY: J is 1 when at least one row is
 *                    selected and 0 when none is (a group has at least one row, as everywhere in the library), the one row of outputs is
 *                    index 0, d_keys_in and d_keys_out may be NULL, and capacity == 0 with J == 1 is HJGPU_EOVERFLOW.
 *   aggs             a HOST array of naggs hjgpu_aggregate, copied by value; naggs is 0 to HJGPU_AGG_MAX_AGGS (0: the counts alone; aggs
 *                    and d_aggs_out may then be NULL).  HJGPU_EINVAL, each with a text that names the aggregate's index: fn > 3, a flag
 *                    bit outside HJGPU_AGG_SIGNED, d_a == NULL, d_b == NULL under HJGPU_AGG_SUM_MUL, d_b != NULL under any other fn, a
 *                    NULL d_aggs_out entry.  d_a may equal d_b (a sum of squares); a column may appear in several aggregates and also
 *                    as a key.  Columns hold n uint32 (int32 under HJGPU_AGG_SIGNED), 16-byte aligned.
 *   d_aggs_out       a HOST array of naggs device pointers; d_aggs_out[c] holds capacity uint64, and for group j
 *                      HJGPU_AGG_SUM      the sum of a modulo 2^64; a is zero-extended, or sign-extended under HJGPU_AGG_SIGNED (the
 *                                         caller then reads the word as int64);
 *                      HJGPU_AGG_SUM_MUL  the sum modulo 2^64 of the exact product per row: uint32 x uint32 -> uint64, or
 *                                         int32 x int32 -> int64 under HJGPU_AGG_SIGNED;
 *                      HJGPU_AGG_MIN/MAX  the extreme of a in unsigned order, zero-extended; under HJGPU_AGG_SIGNED the extreme in int32
 *                                         order, sign-extended.
 *                    HJGPU_NULL_VAL in a looked-up column is the ordinary value 0xFFFFFFFF, as it is for the filter.
 *   d_counts_out     capacity uint64, or NULL: no counts.
 * The workspace is hjgpu_group_sum's merge table in the context (one context runs one call at a time).  Three enqueues ordered by the
 * stream - the clears, the aggregation, the emit - and no workgroup waits for another; with keys the aggregation is hjgpu_group_sum's
 * (LDS tables, then the merge table), without keys every lane aggregates in registers and a workgroup adds its totals to one slot.
 * hjgpu_get_stats afterwards: hjgpu_group_sum's mapping (ms_histogram = the clears, ms_join = the aggregation, ms_close_gaps = the emit).
 * hjgpu_get_counter "agg_step_rows" / "agg_scalar_step_rows": the rows one loop iteration of the whole grid covers with / without keys.
 * Plain unsigned sums of a GROUP BY are hjgpu_group_sum's job as much as this one's: the results are the same. */
#define HJGPU_AGG_SUM      0u   /* SUM(a)                                                        */
#define HJGPU_AGG_SUM_MUL  1u   /* SUM(a * b): the exact 64-bit product of the two 32-bit values */
#define HJGPU_AGG_MIN      2u   /* MIN(a)                                                        */
#define HJGPU_AGG_MAX      3u   /* MAX(a)                                                        */
#define HJGPU_AGG_SIGNED   1u   /* flags: a (and b) are int32                                    */
#define HJGPU_AGG_MAX_AGGS 4u
typedef struct { uint32_t fn, flags; const uint32_t *d_a, *d_b; } hjgpu_aggregate;
int  hjgpu_group_agg(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                     uint32_t nkeys, const uint32_t *const *d_keys_in, uint32_t naggs, const hjgpu_aggregate *aggs,
                     uint32_t *const *d_keys_out, uint64_t *d_counts_out, uint64_t *const *d_aggs_out,
                     size_t capacity, uint64_t *ngroups, void *stream);
int  hjgpu_group_agg_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                           uint32_t nkeys, const uint32_t *const *d_keys_in, uint32_t naggs, const hjgpu_aggregate *aggs,
                           uint32_t *const *d_keys_out, uint64_t *d_counts_out, uint64_t *const *d_aggs_out,
                           size_t capacity, uint64_t *d_ngroups, void *stream);

/* ---- GROUP BY up to four columns ---------------------------------------------------------------------------------------------------------
 * hjgpu_group_agg's contract, word for word, except that nkeys is 0 to HJGPU_GROUP_BY_MAX_KEYS (4): the mask and NULL, hjgpu_aggregate and
 * its refusals with the aggregate's index in the text, every key value legal - 0 and HJGPU_NULL_VAL included, in every key column -, the
 * groups in unspecified order, n == 0, *ngroups, HJGPU_EOVERFLOW with a lower bound of J above capacity, capacity == 0 and capacity > 2^40,
 * alignment (HJGPU_EALIGN), the "overlaps" refusals, the capturing stream, every refusal decided from the arguments alone before anything
 * is allocated or enqueued, the untouched async status, calls queued back to back on one stream.  nkeys > 4 is HJGPU_EINVAL ("nkeys" in
 * hjgpu_last_error); d_keys_in and d_keys_out are HOST arrays of nkeys device pointers; the same key column may be given more than once.
 * The road is chosen by nkeys, as hjgpu_lookup chooses its road by inner:
 *   nkeys <= 2       hjgpu_group_agg itself: its checks (an error text may name hjgpu_group_agg), its kernels, its results, its stats.
 *   nkeys 3 or 4     the wide road.  A tuple no longer fits one 64-bit word, so a slot of the tables has a 64-bit word per key column,
 *                    key | 1 << 32 - never 0, whatever the key - and insert-or-find goes through a slot's words in order with one 64-bit
 *                    compare-and-swap per word that is still empty; no lane waits for another and no slot is ever left half owned
 *                    (DESIGN.md section 5 "Wide keys").  Everything else is hjgpu_group_agg's: one pass over the mask, the key columns
 *                    and the aggregates' columns, a pre-aggregation per workgroup in LDS, the merge table in the context's workspace (a
 *                    power of two of at least 2 * capacity and at least 1024 slots of 72 bytes; it shares hjgpu_group_sum's buffer and
 *                    grows the first time a capacity is seen: hjgpu_stats.ms_reserve), the emit.  Three enqueues ordered by the stream.
 * hjgpu_get_stats after the wide road: hjgpu_group_agg's mapping - ms_histogram = the clears, ms_join = the aggregation, ms_close_gaps =
 * the emit, ms_total = all of it, every other phase 0, fanout1 = fanout2 = buckets = groups = 0.  hjgpu_get_counter "group_by_lds_groups":
 * the distinct groups a workgroup's wide LDS table holds; "group_by_step_rows": the rows one loop iteration of the whole grid covers.
 * hjgpu_group_sum and hjgpu_group_agg keep refusing nkeys > 2. */
#define HJGPU_GROUP_BY_MAX_KEYS 4u
int  hjgpu_group_by(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                    uint32_t nkeys, const uint32_t *const *d_keys_in, uint32_t naggs, const hjgpu_aggregate *aggs,
                    uint32_t *const *d_keys_out, uint64_t *d_counts_out, uint64_t *const *d_aggs_out,
                    size_t capacity, uint64_t *ngroups, void *stream);
int  hjgpu_group_by_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                          uint32_t nkeys, const uint32_t *const *d_keys_in, uint32_t naggs, const hjgpu_aggregate *aggs,
                          uint32_t *const *d_keys_out, uint64_t *d_counts_out, uint64_t *const *d_aggs_out,
                          size_t capacity, uint64_t *d_ngroups, void *stream);

/* ---- ORDER BY up to four keys with LIMIT over a bitmap's rows -------------------------------------------------------------------------------
 * What ends a chain of column operators: the groups of hjgpu_group_by, the rows of a compaction or of a materialised join come out in
 * unspecified order, and a query ends in ORDER BY ... [LIMIT k].  Let the selected rows be the rows i < n whose bit is set in
 * d_select_bits, J their number and m = min(J, limit).  The selected rows are ordered lexicographically by keys[0], then keys[1], ...,
 * every key in its own direction and signedness, and TIES IN EVERY KEY ARE BROKEN BY ASCENDING ROW NUMBER, whatever the directions: the
 * result is fully determined and bit-for-bit reproducible.  For j < m, with r_j the j-th row of that order:
 *   d_rows_out[j] = (uint32_t) r_j (d_rows_out may be NULL) and cols[c].d_out[j] = cols[c].d_in[r_j], elements of 4 bytes, or of 8 under
 *   HJGPU_ORDER_WIDE.  Nothing is written at index >= m of any output; the mask and the inputs are never written.
 *   d_select_bits    hjgpu_lookup_selected's mask, word for word: (n + 31) / 32 words, bit i & 31 of word i >> 5 selects row i, bits of the
 *                    last word at positions >= n are ignored, no word at index >= (n + 31) / 32 is read.  16-byte aligned (HJGPU_EALIGN).
 *                    NULL selects every row.
 *   keys             a HOST array of nkeys hjgpu_order_key, copied by value.  d_col holds n uint32, or n uint64 under HJGPU_ORDER_WIDE (what
 *                    the grouped operators' counts and aggregates are); HJGPU_ORDER_SIGNED: the column is int32 (int64 with _WIDE), two's
 *                    complement order; HJGPU_ORDER_DESC: this key descending.  nkeys is 1 to HJGPU_ORDER_MAX_KEYS; nkeys == 0 is HJGPU_EINVAL
 *                    ("nkeys" in hjgpu_last_error): with no key the call is hjgpu_compact_selected.
 *   key values       every value is legal.  HJGPU_NULL_VAL in a looked-up column is the ordinary value 0xFFFFFFFF, as it is for the filter:
 *                    last in unsigned ascending order, -1 under HJGPU_ORDER_SIGNED.  There is no NULLS FIRST / NULLS LAST.
 *   cols             a HOST array of ncols hjgpu_order_column, copied by value: the carried columns.  flags is 0 (n uint32 in, limit-or-n
 *                    uint32 out) or HJGPU_ORDER_WIDE (uint64).  ncols is 0 to HJGPU_ORDER_MAX_COLS; a key column may also be carried, and
 *                    the same column may appear several times.  ncols == 0 with d_rows_out == NULL: the count alone.
 *   refusals by index   HJGPU_EINVAL, each with a text that names the entry ("key 2", "column 5"): a flag bit outside those defined,
 *                    reserved != 0, a NULL pointer among the first nkeys / ncols entries.
 *   n                n > 0xFFFFFFFF is HJGPU_EINVAL: a row number is a uint32.
 *   count            *count (blocking form, host memory) / *d_count (_async form, device memory, 8-byte aligned: HJGPU_EALIGN) = J, exact
 *                    whatever limit is.  limit < J is LIMIT, not an error: HJGPU_EOVERFLOW is never returned.
 *   alignment        the mask, every key column, every carried input, every output and d_rows_out 16-byte aligned (HJGPU_EALIGN).
 *   not in place     the first min(limit, n) elements of an output, or the _async form's count word, that share a byte with the mask, a key
 *                    column, a carried input or another output: HJGPU_EINVAL, "overlaps" in hjgpu_last_error.
 *   n == 0           reads nothing, writes nothing but the count (0), accepts NULL everywhere else.
 * Every refusal is decided from the arguments alone, before anything is allocated or enqueued; a capturing stream is HJGPU_EINVAL; what
 * hjgpu_get_async_status reports is untouched.  The _async form only enqueues and needs no hjgpu_reserve; calls may be queued back to
 * back on one stream of one context.  The method is a least-significant-digit radix sort of the PERMUTATION - uint32 row numbers, never
 * the columns - in digits of 8 bits, from the last key's lowest digit to the first key's highest, every pass a stable counting sort; the
 * initial permutation is the selected row numbers ascending, which is where the tie rule comes from.  The road is chosen by n alone, as
 * hjgpu_lookup chooses by inner:
 *   n <= "order_lds_rows"   ONE launch of ONE workgroup: the permutation is made from the mask, sorted and gathered in LDS; a pass whose
 *                    digit is the same for every row is skipped.
 *   beyond           the initial permutation is hjgpu_compact_selected's row numbers (with a NULL mask: an iota); every pass is three
 *                    launches ordered by the stream - a digit histogram per range of the current permutation, an exclusive scan over
 *                    (digit, range), a scatter in which each workgroup ranks its range chunk by chunk - and a last launch gathers the
 *                    outputs.  J stays in device memory.  No workgroup ever waits for another.
 * The workspace is the call's own, in the context, sized from n and never from J: 16 bytes on the LDS road, 8 bytes per row (the two
 * permutation buffers) plus 2,146,320 bytes beyond it; it grows the first time a size is seen (hjgpu_stats.ms_reserve).  hjgpu_get_stats
 * afterwards: ms_histogram = the initial permutation, ms_join = the sorting passes, ms_close_gaps = the final gather, ms_total = all of it
 * (the LDS road's one launch is ms_join), every other phase 0, fanout1 = fanout2 = buckets = groups = 0.  hjgpu_get_counter
 * "order_lds_rows": the rows one workgroup's LDS holds; "order_ranges" / "order_chunk_rows": the device road's geometry - the current
 * permutation is cut into that many contiguous ranges of whole chunks of that many rows, the tail in the last non-empty one.
 * More than four keys or eight carried columns: a further call, or d_rows_out as the index of hjgpu_gather_selected. */
#define HJGPU_ORDER_MAX_KEYS 4u
#define HJGPU_ORDER_MAX_COLS 8u
#define HJGPU_ORDER_DESC   1u   /* this key descending */
#define HJGPU_ORDER_SIGNED 2u   /* the key column is int32 (int64 with _WIDE): two's complement order */
#define HJGPU_ORDER_WIDE   4u   /* the column holds 64-bit words */
typedef struct { const void *d_col; uint32_t flags, reserved; } hjgpu_order_key;
typedef struct { const void *d_in; void *d_out; uint32_t flags /* 0 or HJGPU_ORDER_WIDE */, reserved; } hjgpu_order_column;
int  hjgpu_order_by(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                    uint32_t nkeys, const hjgpu_order_key *keys, uint32_t ncols, const hjgpu_order_column *cols,
                    uint32_t *d_rows_out, size_t limit, uint64_t *count, void *stream);
int  hjgpu_order_by_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n,
                          uint32_t nkeys, const hjgpu_order_key *keys, uint32_t ncols, const hjgpu_order_column *cols,
                          uint32_t *d_rows_out, size_t limit, uint64_t *d_count, void *stream);

/* ---- whole joins on HBM-resident columns (replace run()/run_hj()) ---------------- */
/* run(), npj.cpp:769-927 */
int  hjgpu_npj(hjgpu_ctx *ctx,
               const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
               const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
               const hjgpu_npj_params *params,
               hjgpu_result *result, const hjgpu_output *out, void *stream);
/* run_hj(), phj.cpp:1646-1949.  Passes (phj.cpp:1791-1808 plans 1-4 of equal fan-out from the partition count): one
 * or two passes up to HJGPU_MAX_PARTS partitions; a build side beyond their reach (~228 M tuples) whose probe side is
 * large enough for a further pass to pay is joined by a GROUPED plan - pass 0 splits both relations into key-disjoint
 * groups of about "group_inner" (64 M) build tuples, each joined by the two-pass plan, aggregates and rows added up
 * (hjgpu_stats.groups / ms_scatter0).  The groups are planned ON THE DEVICE (round 6; option "group_device", default 1): pass 0 leaves
 * the groups' offsets in device memory, one small kernel turns them into a descriptor per group (first row and rows of its build and probe
 * columns), and every kernel of a group's join reads its geometry from there - the whole plan is ONE stream-ordered sequence on the
 * caller's stream, exactly like an ungrouped join (phj.cpp:1791-1863 plans and runs its passes inside run_hj).  The *_async forms
 * therefore return at once for grouped plans too, hold no stream in hardware and use no thread of their own.  The workspace of a
 * group's join is planned for up to (1 + "group_slack" / 100) x the mean group (default 50); a group beyond that - heavy duplicates -
 * is SKIPPED and flagged on the device, and the join is then not valid: an *_async call's d_result holds all ones (never a plausible
 * partial count), and the join is done again in the host-planned form (the calling thread waits for pass 0 and plans every group's
 * join from its size) at the caller's next blocking touch point - inside the call for the blocking forms, in hjgpu_get_async_status for
 * the enqueue-only ones (which must therefore be called before d_result or the rows of a grouped plan are trusted; it costs a stream
 * synchronisation when nothing was skipped).  Option "group_device" = 0: always the host-planned form (the *_async forms then wait
 * inside the call); option "audit" implies it.  hjgpu_phj_overlapped_async (the local join of hjgpu_phj_multi / hjgpu_cpra_multi) is
 * always planned on the device; the rank's thread asks for the status after a wait with the communicator's deadline.  Explicit fan-outs in
 * params are never grouped; option "group_from" = 0 turns the plan off. */
int  hjgpu_phj(hjgpu_ctx *ctx,
               const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
               const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
               const hjgpu_phj_params *params,
               hjgpu_result *result, const hjgpu_output *out, void *stream);
/* run_hj(), cpra2.cpp:1697-1986 (chunked partitioning, owner gathers slices) */
int  hjgpu_cpra(hjgpu_ctx *ctx,
                const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
                const hjgpu_phj_params *params,
                hjgpu_result *result, const hjgpu_output *out, void *stream);
/* hjgpu_npj_async cannot report HJGPU_EZEROKEY (a build key of 0 is skipped by the build, npj.cpp:583, and the
 * blocking hjgpu_npj says so): callers of the enqueue-only form must keep key 0 out of the build side themselves.
 * Enqueue-only forms: the aggregates land in d_result (device memory, 32 bytes);
 * no host synchronisation, so a caller can time with its own events and keep several
 * joins in flight on one stream.  Workspace must have been reserved (hjgpu_reserve).
 * Not valid inside a HIP stream capture (HJGPU_EINVAL on a capturing stream): a
 * replayed graph of a join faulted on gfx950 / ROCm 7.0. */
int  hjgpu_npj_async(hjgpu_ctx *ctx,
                     const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                     const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
                     const hjgpu_npj_params *params, hjgpu_result *d_result, void *stream);
int  hjgpu_phj_async(hjgpu_ctx *ctx,
                     const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                     const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
                     const hjgpu_phj_params *params, hjgpu_result *d_result, void *stream);
/* As hjgpu_phj_async, but the build columns only become valid once
 * `inner_ready_event` (a hipEvent_t passed as void*, recorded by the caller on the
 * stream that produces them, e.g. an RCCL broadcast) has fired: the probe side is
 * histogrammed and partitioned first, the wait sits right before the first kernel
 * that reads R.  This is how the multi-GPU PHJ hides the build-side broadcast.
 * (A grouped plan - see hjgpu_phj - reads R first: the stream waits for the event, and the CALLING thread waits for the groups.) */
int  hjgpu_phj_overlapped_async(hjgpu_ctx *ctx,
                     const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                     const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
                     const hjgpu_phj_params *params, hjgpu_result *d_result, void *stream,
                     void *inner_ready_event);
int  hjgpu_cpra_async(hjgpu_ctx *ctx,
                      const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                      const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
                      const hjgpu_phj_params *params, hjgpu_result *d_result, void *stream);
/* Status of an enqueue-only join.  The blocking forms report HJGPU_EZEROKEY (a build key of 0 met by NPJ: the
 * reference's empty-bucket sentinel, npj.cpp:196-210, 583, 867 - such a tuple is not in the table) and
 * HJGPU_EOVERFLOW (the reference's assert(o <= block_limit), npj.cpp:245); an *_async join cannot, so its caller asks:
 *   hjgpu_get_async_status        waits for `stream` and returns what the blocking form of the LAST join enqueued on this
 *                                 context would have returned (HJGPU_OK / HJGPU_EZEROKEY / HJGPU_EOVERFLOW);
 *   hjgpu_accumulate_async_status enqueue-only: d_flags[0] += 1 if that join met a zero build key, d_flags[1] += 1 if
 *                                 its materialised output overflowed (two uint64 in device memory: the multi-GPU joins
 *                                 all-reduce them with the four aggregates, so every rank returns the same status). */
int  hjgpu_get_async_status(hjgpu_ctx *ctx, void *stream);
int  hjgpu_accumulate_async_status(hjgpu_ctx *ctx, uint64_t *d_flags, void *stream);
/* Materialised rows from an enqueue-only join: the NEXT *_async join enqueued on this context (hjgpu_npj_async,
 * hjgpu_phj_async, hjgpu_phj_overlapped_async, hjgpu_cpra_async, hjgpu_phj_probe_async) writes its rows into `out`
 * exactly as the blocking form does (block protocol + close_gaps; the dense prefix [0, d_result->count) holds the
 * result once `stream` has passed the join).  One-shot; out == NULL withdraws it.  Overflow: see above. */
int  hjgpu_set_async_output(hjgpu_ctx *ctx, const hjgpu_output *out);
/* Capacity (in rows, a multiple of block_size) of result columns that are guaranteed to hold `rows` result rows
 * of a join of this context: rows rounded up to whole blocks plus one open block per worker (the reference sizes its
 * output the same way: 1.05 J + 2 T blocks, npj.cpp:997-1000).  algorithm: 0 npj (needs outer_tuples), 1 phj, 2 cpra;
 * block_size 0 = 65536. */
int  hjgpu_output_capacity(hjgpu_ctx *ctx, int algorithm, size_t outer_tuples, size_t rows, size_t block_size,
                           size_t *capacity);

/* ---- PHJ with the build side prepared once and probed by any number of batches -------------------
 * R join S = union over batches S_i of R join S_i, so a probe side that arrives in pieces (slices of a
 * multi-GPU exchange, batches from the host or from an upstream operator) needs the build side
 * histogrammed and partitioned only once: hjgpu_phj_build runs build-side K4/K5/K6 (the reference's
 * run_hj up to the end of the inner relation's passes, phj.cpp:1715-1863) and keeps the partitions in
 * the context's workspace; every hjgpu_phj_probe partitions one batch and runs build+probe per
 * partition (phj.cpp:1869-1924) against them.  `max_outer` sizes the workspace: batches may have up
 * to that many rows.  The prepared state lasts until any other join / partition entry point is called
 * on the context (hjgpu_phj_probe then fails with HJGPU_EINVAL); the caller's build columns are not
 * read again after hjgpu_phj_build has completed on `stream`.  Results are per batch: add them up. */
int  hjgpu_phj_build(hjgpu_ctx *ctx,
                     const uint32_t *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                     size_t max_outer, const hjgpu_phj_params *params, void *stream);
int  hjgpu_phj_probe(hjgpu_ctx *ctx,
                     const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
                     hjgpu_result *result, const hjgpu_output *out, void *stream);
int  hjgpu_phj_probe_async(hjgpu_ctx *ctx,
                           const uint32_t *d_outer_keys, const uint32_t *d_outer_vals, size_t outer,
                           hjgpu_result *d_result, void *stream);

/* ---- PHJ over relations that ARRIVE pass-1-partitioned: the receiving side of the multi-GPU CPRA ---------------------
 * In the reference every worker partitions its own chunk and the owner of a partition gathers that partition's slice
 * from every chunk (cpra2.cpp:1757-1827 own-chunk passes, 1868-1872 ownership, 1891-1959 gather): the own-chunk
 * partitioning IS the join's partitioning.  Across GPUs the same holds when the exchange-level partitioning is pass 1:
 *   sender    hjgpu_partition_packed_async: own chunk -> packed tuples (payload << 32 | key, 8 bytes) partitioned with
 *             fan-out G * k, H(key, factor, G * k); rank g owns partitions [g * k, (g + 1) * k): ONE contiguous message
 *             per destination (keys and payloads travel together: one all-to-all-v instead of two);
 *   receiver  gets `chunks` pieces (one per source rank), each holding its k partitions in order, and runs pass 2 +
 *             build / probe only: hjgpu_phj_build_prepartitioned prepares the received build side once (fused histogram
 *             over the pieces, pass 2 into line-aligned final partitions), hjgpu_phj_probe_prepartitioned_async joins
 *             one received probe batch against it (results add up over the batches).
 * 16 bytes per tuple less HBM traffic on the receiver than partitioning the received tuples from scratch.
 * d_tuples_out of the sender must be 128-byte aligned; d_offsets: fanout + 1 uint64 (rows).  The receiver's pieces are
 * rows [chunk_offsets[c], chunk_offsets[c + 1]) of ONE array (contiguous, e.g. a receive buffer); a batch that is
 * too large for max_outer is passed in several calls, each a contiguous row range cut at any row (a piece of a
 * piece is still sorted by partition): pieces that do not take part have chunk_offsets[c] == chunk_offsets[c + 1]. */
typedef struct {
    uint32_t factor1;           /* the exchange-level pass: p1 = H(key, factor1, fanout1_total)                  */
    uint32_t fanout1_total;     /* G * k, <= 1024                                                                */
    uint32_t first_partition;   /* this rank owns pass-1 partitions [first_partition, first_partition + fanout1) */
    uint32_t fanout1;           /* k                                                                             */
    uint32_t chunks;            /* pieces (source ranks), 1..8                                                   */
    uint32_t reserved;
    uint64_t chunk_offsets[9];  /* rows; non-decreasing; entries beyond [chunks] are ignored                      */
} hjgpu_prepartitioned;
int  hjgpu_partition_packed_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                                  uint32_t factor, uint32_t fanout, uint64_t *d_tuples_out, uint64_t *d_offsets,
                                  void *stream);
/* The same, with the partitions [own_first, own_first + own_count) laid out LAST: rows [n - own_rows, n) of d_tuples_out,
 * behind all other partitions (which keep their order, rows [0, n - own_rows)).  d_offsets is still the plain prefix of
 * the counts (d_offsets[p + 1] - d_offsets[p] rows in partition p); a partition's first row follows from it:
 *   p <  own_first              d_offsets[p]
 *   p in the own range          n - own_rows + d_offsets[p] - d_offsets[own_first]
 *   p >= own_first + own_count  d_offsets[p] - own_rows              (own_rows = the own range's rows).
 * What it is for: a rank of the multi-GPU CPRA keeps its own partitions where they were written - the message to itself
 * (cpra2.cpp:1891-1959 gathers the owner's own chunk with the same memcpy as everybody else's) is never copied: the
 * other ranks' pieces are received right behind row n, and rows [n - own_rows, n + received) are the `chunks` pieces of
 * hjgpu_prepartitioned (the own piece first). */
int  hjgpu_partition_packed_own_last_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                                           uint32_t factor, uint32_t fanout, uint32_t own_first, uint32_t own_count,
                                           uint64_t *d_tuples_out, uint64_t *d_offsets, void *stream);
int  hjgpu_phj_build_prepartitioned(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *layout,
                                    size_t max_outer, const hjgpu_phj_params *params /* fanout2, factor2, table factors, flags */,
                                    void *stream);
int  hjgpu_phj_probe_prepartitioned_async(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *layout,
                                          hjgpu_result *d_result, void *stream);
/* Counts published with the partitions (cpra2.cpp:1783-1840: every worker's histogram of its chunk is what the owners'
 * gather is planned from).  The SENDER's histogram pass can count the receivers' second level in the same read of its keys:
 * hjgpu_partition_packed_counted_async = hjgpu_partition_packed(_own_last)_async (own_count = 0: plain order) that also
 * leaves d_counts2[p1 * fanout2 + p2] = rows of the chunk with H(key, factor, fanout) = p1 and H(key, factor2, fanout2) = p2
 * (fanout * fanout2 <= 32768: the fused histogram lives in LDS).  A receiver that is handed, for every piece c, the rows
 * [first_partition * fanout2, (first_partition + fanout1) * fanout2) of that piece's sender's d_counts2 - d_counts
 * [c * fanout1 * fanout2 + ...], in the order of the pieces - joins the batch without a histogram pass of its own over what
 * arrived (hjgpu_phj_probe_prepartitioned_counted_async; the batch must be whole pieces, as counted).  fanout2 / factor2
 * have to be the prepared build side's: hjgpu_prepartitioned_plan says what hjgpu_phj_build_prepartitioned plans for a
 * build side of `inner` rows (params->fanout2 forces it: all receivers of one exchange need the same). */
int  hjgpu_partition_packed_counted_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                                          uint32_t factor, uint32_t fanout, uint32_t own_first, uint32_t own_count,
                                          uint32_t factor2, uint32_t fanout2, uint64_t *d_tuples_out, uint64_t *d_offsets,
                                          uint64_t *d_counts2, void *stream);
int  hjgpu_phj_probe_prepartitioned_counted_async(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *layout,
                                                  const uint64_t *d_counts, hjgpu_result *d_result, void *stream);
int  hjgpu_prepartitioned_plan(hjgpu_ctx *ctx, size_t inner, uint32_t fanout1, const hjgpu_phj_params *params,
                               uint32_t *fanout2, uint32_t *factor2);
/* The planning rule of hjgpu_phj / hjgpu_cpra for relations of these sizes (the reference plans its passes from the partition
 * count, phj.cpp:1791-1808): *groups = the groups of the grouped plan, 0 = one or two passes.  hjgpu_cpra_multi asks it, with a
 * rank's share of the relations' total sizes, which road its ranks take. */
int  hjgpu_grouped_plan(hjgpu_ctx *ctx, size_t inner, size_t outer, const hjgpu_phj_params *params, uint32_t *groups);

/* ---- whole joins on HOST columns (what the npj/phj/cpra mains call after
 * their fread()s, npj.cpp:1013-1039): upload, join, return aggregates.
 * Batches (option "host_batch": -1 = the default: hjgpu_join_host_rows always, hjgpu_join_host when whole columns and
 * their workspace would not fit the device's free memory; 0 = never; n = always, n rows per batch; a probe side of at
 * least two batches of 64 Mi rows): the build side is uploaded and prepared once, the
 * probe side travels in batches through two device buffers - batch i is joined while batch i + 1 is on the bus (R join S
 * = union over the batches); the device never holds the probe side as a whole (it may be larger than the device's
 * memory), the call costs the upload plus the last batch's join.  stats->batches says how many there were; ms_total is
 * the device time of the whole join - the build side's work plus every batch's join, as after a call without batches -
 * and the phase times are the last batch's scaled to that sum (NPJ: ms_build = the table's build).  hjgpu_join_host_rows works the
 * same way: every batch's rows are made dense on the device and go home - into page-locked columns by a copy kernel, so
 * that the DMA engines carry the upload only - while the next batch is joined; a batch that outgrows its share of
 * rows->capacity (x 1.25: a skewed probe side) is joined once more alone, into device columns made for exactly its rows;
 * only a result beyond rows->capacity sends the call down the whole-column path (it starts over and reports the rows needed).  In batches algorithm 2 (CPRA) joins
 * every batch as ONE chunk of the probe side (cpra2.cpp:1757-1827 partitions every chunk on its own: a batch is one);
 * params->chunks applies to calls without batches.
 * Otherwise (small probe sides, host_batch = 0) the columns are uploaded whole on their own
 * stream, probe side first, build side behind it; PHJ / CPRA partition the probe side while the build side is still
 * arriving.  Page-locked columns (hjgpu_host_alloc) are DMA'd where they are, pageable ones staged
 * through two 32 MiB page-locked buffers the context keeps.
 * stats->ms_upload is the wall-clock time of the upload, ms_total the device time of the join. */
int  hjgpu_join_host(hjgpu_ctx *ctx, int algorithm /* 0 npj, 1 phj, 2 cpra */,
                     const uint32_t *inner_keys, const uint32_t *inner_vals, size_t inner,
                     const uint32_t *outer_keys, const uint32_t *outer_vals, size_t outer,
                     const hjgpu_phj_params *phj_params, const hjgpu_npj_params *npj_params,
                     hjgpu_result *result, hjgpu_stats *stats);

/* As hjgpu_join_host, but the join is materialised (the reference's join_keys / join_outer_vals /
 * join_inner_vals columns, npj.cpp:997-1000, which its mains allocate on the host) and the dense
 * result [0, result->count) is copied back into the caller's three host columns.
 * Page-locked result columns (hjgpu_host_alloc) are filled by DMA, pageable ones through two pinned
 * staging buffers.  Returns HJGPU_EOVERFLOW, with result->count set, when the join has more rows
 * than rows->capacity: call again with columns of at least that many rows.  Row order is
 * unspecified, as in the reference (block claiming, npj.cpp:244-246). */
typedef struct {
    uint32_t *keys, *outer_vals, *inner_vals;   /* host columns of `capacity` uint32 each */
    size_t    capacity;                         /* in rows                                */
} hjgpu_host_rows;
int  hjgpu_join_host_rows(hjgpu_ctx *ctx, int algorithm /* 0 npj, 1 phj, 2 cpra */,
                          const uint32_t *inner_keys, const uint32_t *inner_vals, size_t inner,
                          const uint32_t *outer_keys, const uint32_t *outer_vals, size_t outer,
                          const hjgpu_phj_params *phj_params, const hjgpu_npj_params *npj_params,
                          const hjgpu_host_rows *rows, hjgpu_result *result, hjgpu_stats *stats);
/* hjgpu_join_host_rows into result columns that SEVERAL calls share (one per GPU of a node, each on its own context and
 * host thread: what hjgpu_join_host_rows_multi does for PHJ / NPJ): the rows of this call are appended where an atomic
 * fetch-add on *cursor puts them - a batch's dense rows as soon as they exist, so the calls' rows interleave and
 * [0, *cursor) is dense when all calls have returned (every reference worker appends its blocks to the shared output
 * the same way: npj.cpp:244-246, 312-316).  result = THIS call's aggregates.  Rows that do not fit (rows->capacity, or a
 * skewed batch's device columns) are counted, not written: HJGPU_EOVERFLOW, result->count exact, nothing starts over. */
int  hjgpu_join_host_rows_shared(hjgpu_ctx *ctx, int algorithm,
                                 const uint32_t *inner_keys, const uint32_t *inner_vals, size_t inner,
                                 const uint32_t *outer_keys, const uint32_t *outer_vals, size_t outer,
                                 const hjgpu_phj_params *phj_params, const hjgpu_npj_params *npj_params,
                                 const hjgpu_host_rows *rows, uint64_t *cursor, hjgpu_result *result, hjgpu_stats *stats);

/* ---- multi-GPU joins ------------------------------------------------------------------------------
 * The reference's cross-worker exchange is part of run_hj itself: phj.cpp:1715-1770 (thread-level pass: both
 * relations are exchanged between the threads) and cpra2.cpp:1861-1971 (thread t owns partitions
 * [t*P/T, (t+1)*P/T), cpra2.cpp:1868-1872, and gathers them from every thread's chunk by memcpy).  Here a
 * RANK is one GPU's share of a join and the exchange is RCCL over xGMI, called from this library (C++):
 *   hjgpu_phj_multi / hjgpu_npj_multi   build side replicated from `root` (scatter of 1/G slices over the root's
 *       G-1 links + all-gather, or one ring broadcast), probe side sharded (thread_beg / thread_end ranges with
 *       T = G, npj.cpp:516-529), complete local join per rank - the replication overlaps the probe side's
 *       partitioning -, ncclAllReduce of the four aggregates.  Valid because R join S = union_g (R join S_g).
 *   hjgpu_cpra_multi   both relations chunked over the ranks (cpra2.cpp:1737-1742); every rank partitions its own
 *       chunk with fan-out G (cpra2.cpp:1757-1827), the counts are all-gathered (cpra2.cpp:1834-1840: counts
 *       published, barrier), rank g receives partition g of every chunk by grouped ncclSend / ncclRecv
 *       (all-to-all-v; the memcpy gather cpra2.cpp:1891-1959), local PHJ, ncclAllReduce.  The probe side travels
 *       in `slices` pieces: slice i+1 is partitioned and slice i-1 joined (build side prepared once,
 *       hjgpu_phj_build / hjgpu_phj_probe) while slice i is on the links.
 * A communicator holds one or more LOCAL ranks (one host thread drives them: grouped RCCL calls):
 *   hjgpu_comm_create_local   every rank in this process, ranks[i] on devices[i]: what ./phj and ./cpra use
 *       (all visible GPUs).  transport RCCL = ncclCommInitAll; transport LOOPBACK = exchanges are hipMemcpyAsync
 *       between the ranks' buffers, ranks may share a device: the complete orchestration (ownership, counts,
 *       slicing, reductions) then runs at any world size on ONE GPU with the real kernels (tests), or across
 *       the GPUs of a node by peer copies.
 *   hjgpu_comm_create_rank    one rank per process (torchrun, MPI): ncclCommInitRank with the id that rank 0
 *       got from hjgpu_comm_get_id and passed around (bench.py: over torch.distributed's gloo store).
 * Every process must make the same sequence of *_multi calls with the same `slices` / root / |R| (collectives).
 * The calls return when the result is on the host; it is the GLOBAL result on every rank. */
typedef struct hjgpu_comm hjgpu_comm;
#define HJGPU_TRANSPORT_RCCL      0
#define HJGPU_TRANSPORT_LOOPBACK  1
#define HJGPU_ERCCL               8   /* RCCL error (text in hjgpu_comm_last_error)                */
typedef struct { char bytes[128]; } hjgpu_comm_id;          /* ncclUniqueId */

int  hjgpu_comm_create_local(int nranks, const int *devices, int transport, hjgpu_comm **comm);
int  hjgpu_comm_get_id(hjgpu_comm_id *id);
int  hjgpu_comm_create_rank(int device, int nranks, int rank, const hjgpu_comm_id *id, hjgpu_comm **comm);
int  hjgpu_comm_destroy(hjgpu_comm *comm);
/* comm == NULL: why the last hjgpu_comm_create_* / hjgpu_comm_get_id of THIS thread failed (the communicator that could
 * not be made no longer exists; RCCL's own text, e.g. of ncclCommInitRank, is kept here) */
const char *hjgpu_comm_last_error(const hjgpu_comm *comm);
/* world size, local ranks of this process, global rank of local rank 0 */
int  hjgpu_comm_size(const hjgpu_comm *comm, int *nranks, int *nlocal, int *first_rank);
/* the join context of a local rank: its device memory (hjgpu_malloc), generator, options, per-phase stats */
hjgpu_ctx *hjgpu_comm_ctx(hjgpu_comm *comm, int local_rank);
/* option "ring_broadcast" (0 / 1): replicate the build side with one ncclBroadcast instead of scatter +
 * all-gather; "max_message_bytes" (n): split larger point-to-point messages into pieces; "reserve_cus" (n): CUs
 * that the ranks' partitioning kernels leave free for RCCL's kernels (default 16 with RCCL and > 1 rank, else 0: free, K6 is not CU-bound);
 * "timeout_ms" (n, 0 = none; HJGPU_COMM_TIMEOUT_MS presets it): deadline of every host-side wait of the multi-GPU
 * calls.  The reference's workers meet at pthread barriers (cpra2.cpp:1834-1840, phj.cpp:1715-1770) and a worker
 * that never arrives hangs the program; here the streams are polled, RCCL is asked for asynchronous errors
 * (ncclCommGetAsyncError), and at the deadline the communicator is aborted (ncclCommAbort): the call returns
 * HJGPU_ERCCL naming the rank and stream that did not finish, every later call on the communicator fails fast, and
 * the process can exit.  "stall_rank" (k) / "stall_ms" (n): fault injection for tests, loopback transport only - rank
 * k arrives n ms late at every collective.  "exchange_in_place" (0 / 1, default 1): a CPRA rank keeps its own partitions
 * where its partitioning wrote them and receives the others' pieces behind them (no copy of the message to itself);
 * "cpra_two_level" (0 / 1): round 2's CPRA plan (used automatically beyond 8 ranks); "cpra_grouped" (0 / 1 / 2, default 1; the SAME value on every
 * rank: it decides whether a collective is issued, ranks that differ would mismatch their collectives): the ranks
 * agree, from the relations' total sizes (one all-reduce of two words before the build side's exchange), whether a rank's share needs a
 * grouped plan (hjgpu_grouped_plan on local rank 0's join context: set "group_from" / "group_inner" / "group_always" alike on every
 * rank); if so the exchange has fan-out ranks, the probe side travels in one slice and every rank runs a whole local join whose plan
 * groups.  That road costs one pass more than hjgpu_phj's grouped plan (its exchange is no pass of the join): 1 takes it where it still
 * pays (from ~9 table fills per partition on, e.g. 2 G x 8 G per rank), 2 wherever hjgpu_grouped_plan groups, 0 never; "self_via_rccl" (tests);
 * "debug_forensics" (0 / 1, hjgpu_comm_get_forensics below). */
int  hjgpu_comm_set_option(hjgpu_comm *comm, const char *name, const char *value);
/* What the communicator really is: the transport's own view of the world (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice of local rank 0, ncclGetVersion), so that a result line can prove that N ranks talked over RCCL. */
typedef struct {
    int  nranks, nlocal, first_rank;
    char transport[16];        /* "rccl" | "loopback"                                          */
    int  rccl_version;         /* ncclGetVersion, e.g. 22707; 0 without RCCL                   */
    int  rccl_nranks;          /* ncclCommCount of local rank 0's communicator; -1 without     */
    int  rccl_rank;            /* ncclCommUserRank                                             */
    int  rccl_device;          /* ncclCommCuDevice                                             */
    int  timeout_ms;           /* option "timeout_ms"                                          */
    int  aborted;              /* 1: a deadline expired or RCCL reported an asynchronous error */
} hjgpu_comm_info;
int  hjgpu_comm_get_info(hjgpu_comm *comm, hjgpu_comm_info *info);
/* Preflight ("measure link bandwidth first"): 1 MB through every collective the joins use
 * (all-gather, all-to-all-v with a different count for every pair, all-reduce), each verified word for word on the
 * host; then `link_bytes` from every rank to the peer k places on, for k = 1 .. G-1 (all ranks at once, every
 * pair's own xGMI link), and to all peers at once (the CPRA exchange's shape).  Local rank 0's view.
 * Returns HJGPU_ERCCL when a collective delivered wrong data (ok_* say which). */
typedef struct {
    uint32_t nranks, rank;
    uint32_t ok_all_gather, ok_all_to_all, ok_all_reduce;
    float    ms_all_gather, ms_all_to_all, ms_all_reduce;      /* 1 MB per rank, includes RCCL's lazy set-up */
    uint64_t link_bytes;
    float    link_GBs[64];     /* [peer]: link_bytes sent to `peer` while every other rank sends to ITS peer at the same
                                  distance (second of two rounds); 0 for the rank itself                      */
    float    all_to_all_GBs;   /* bytes this rank SENDS per second when every rank sends link_bytes to every peer at once */
} hjgpu_preflight;
int  hjgpu_comm_preflight(hjgpu_comm *comm, size_t link_bytes, hjgpu_preflight *report);
/* Communicator option "debug_forensics" (0 / 1; diagnostics): option "audit" (hjgpu_audit_read above) on both contexts of
 * every local rank; hjgpu_cpra_multi then keeps the records of the step's exchange-level partitioning calls and of its
 * joins.  words[] = for every local rank {global rank, np, nj} followed by np + nj records of 32 words (the rank's
 * partitioning calls in order: build side, probe slices; then its joins: build, probe batches).  *count = the words there
 * are; nothing is copied when capacity is smaller.  tools/stress_cpra.py --forensics prints them for every wrong step:
 * the stage whose sums differ from its input's is the kernel that lost the tuples. */
int  hjgpu_comm_get_forensics(hjgpu_comm *comm, uint64_t *words, size_t capacity, size_t *count);
/* hjgpu_audit_recheck on both contexts of every local rank: words[] = for every local rank and context {global rank, context
 * (0 exchange-level partitioning, 1 join), n} followed by n x 9 words; *count = the words there are. */
int  hjgpu_comm_recheck(hjgpu_comm *comm, uint64_t *words, size_t capacity, size_t *count);
/* "debug_forensics" = 2: hjgpu_cpra_multi reads every slice's records on the host as soon as the slice's partitioning / join has finished -
 * before the next use of its buffers is enqueued (the overlap of a slice's join with the next slice's partitioning stays) - and a stage
 * whose sums differ from its input's is looked at again on the spot (hjgpu_audit_recheck).  words[] = per event {global rank, context,
 * slice, n, the call's record (32 words)} followed by n x 9 words.  Empty after a step whose records all agreed. */
int  hjgpu_comm_get_frozen(hjgpu_comm *comm, uint64_t *words, size_t capacity, size_t *count);
/* every local rank's streams drained, then a collective over all ranks */
int  hjgpu_comm_barrier(hjgpu_comm *comm);

/* One rank's share of the relations: columns on that rank's device (16-byte aligned).
 * hjgpu_phj_multi / hjgpu_npj_multi: `inner` = |R| on EVERY rank, the build columns are read on `root` only (NULL
 * elsewhere); d_outer_* = the rank's probe shard.  hjgpu_cpra_multi: the rank's chunk of both relations. */
typedef struct {
    const uint32_t *d_inner_keys, *d_inner_vals;
    size_t          inner;
    const uint32_t *d_outer_keys, *d_outer_vals;
    size_t          outer;
} hjgpu_shard;

typedef struct {
    float    ms_wall;            /* host clock around the call                                              */
    float    ms_exchange;        /* local rank 0: device time of its exchanges (replication / all-to-all-v)  */
    float    ms_partition;       /* local rank 0: exchange-level partitioning (CPRA)                         */
    float    ms_exchange_wait;   /* local rank 0: stream time its joins spent waiting for an exchange        */
    uint32_t joins;              /* local rank 0: local join calls whose phase times are in `join`           */
    uint32_t self_copies;        /* local rank 0, CPRA: exchanges whose message to ITSELF had to be copied (0 when every
                                    exchange ran in place: the own partitions stay where the partitioning wrote them)  */
    uint64_t tuples_joined;      /* local rank 0: tuples those joins read                                    */
    uint64_t bytes_sent;         /* local rank 0: bytes sent to OTHER ranks                                  */
    float    ms_upload;          /* hjgpu_join_host_multi: wall clock of the call outside the join step itself (cutting the
                                    columns, enqueueing every rank's uploads); 0 for device-resident shards     */
    float    ms_overlap;         /* hjgpu_join_host_multi, local rank 0: how long BEFORE the last byte of its upload
                                    arrived its first join kernel was already on the device (> 0: the partitioning
                                    of the probe shard overlaps the upload, as in hjgpu_join_host)              */
    hjgpu_stats join;            /* local rank 0: phase times of the MEASURED joins, summed: PHJ / NPJ the one local
                                    join; CPRA the build and the last probe batch (`joins`, `tuples_joined` count
                                    exactly those) - reading every slice's times would hold the host thread back  */
} hjgpu_multi_stats;

/* shards: one entry per LOCAL rank, in rank order */
int  hjgpu_phj_multi(hjgpu_comm *comm, const hjgpu_shard *shards, int root, const hjgpu_phj_params *params,
                     hjgpu_result *result, hjgpu_multi_stats *stats);
int  hjgpu_npj_multi(hjgpu_comm *comm, const hjgpu_shard *shards, int root, const hjgpu_npj_params *params,
                     hjgpu_result *result, hjgpu_multi_stats *stats);
int  hjgpu_cpra_multi(hjgpu_comm *comm, const hjgpu_shard *shards, const hjgpu_phj_params *params,
                      int slices /* 0 = 4 (1 in a world of one) */, hjgpu_result *result, hjgpu_multi_stats *stats);
/* Materialised rows (the reference's join_keys / join_outer_vals / join_inner_vals, which every worker writes:
 * npj.cpp:882-915, cpra2.cpp:1965-1982) through the multi-GPU joins: every rank materialises ITS share of the result
 * into its own three device columns (block protocol + close_gaps; CPRA: slice after slice, each behind the rows of
 * the slices before it) and reports how many dense rows it holds; the concatenation of the ranks' rows is the result
 * (SURVEY.md 8e).  `rows`: one entry per LOCAL rank.  When some rank's columns are too small EVERY rank returns
 * HJGPU_EOVERFLOW (the flags are all-reduced with the aggregates), result->count is the global row count and
 * rows[l].rows what rank l needs: size the columns with hjgpu_output_capacity and call again. */
typedef struct {
    hjgpu_output out;            /* this rank's result columns (device memory of the rank's device)         */
    uint64_t     rows;           /* OUT: rows [0, rows) of them hold the rank's share of the result          */
} hjgpu_shard_rows;
int  hjgpu_phj_multi_rows(hjgpu_comm *comm, const hjgpu_shard *shards, hjgpu_shard_rows *rows, int root,
                          const hjgpu_phj_params *params, hjgpu_result *result, hjgpu_multi_stats *stats);
int  hjgpu_npj_multi_rows(hjgpu_comm *comm, const hjgpu_shard *shards, hjgpu_shard_rows *rows, int root,
                          const hjgpu_npj_params *params, hjgpu_result *result, hjgpu_multi_stats *stats);
int  hjgpu_cpra_multi_rows(hjgpu_comm *comm, const hjgpu_shard *shards, hjgpu_shard_rows *rows,
                           const hjgpu_phj_params *params, int slices, hjgpu_result *result, hjgpu_multi_stats *stats);
/* As hjgpu_join_host on all ranks of a LOCAL communicator (what ./npj ./phj ./cpra call when several GPUs are
 * visible): the host columns are cut into the ranks' shares (thread_beg / thread_end, T = ranks), uploaded, joined.
 * algorithm: 0 npj, 1 phj (build side uploaded to rank 0 and replicated from there), 2 cpra (both sides chunked). */
int  hjgpu_join_host_multi(hjgpu_comm *comm, int algorithm,
                           const uint32_t *inner_keys, const uint32_t *inner_vals, size_t inner,
                           const uint32_t *outer_keys, const uint32_t *outer_vals, size_t outer,
                           const hjgpu_phj_params *phj_params, const hjgpu_npj_params *npj_params,
                           hjgpu_result *result, hjgpu_multi_stats *stats);
/* hjgpu_join_host_rows on all ranks of a local communicator: every rank materialises its share, the shares are copied
 * back to back into the caller's three host columns (rank 0's rows first).  HJGPU_EOVERFLOW with result->count set
 * when the result has more rows than rows->capacity.  (A rank whose own device columns turn out too small is run a
 * second time with exactly the size it reported: not the caller's concern.) */
int  hjgpu_join_host_rows_multi(hjgpu_comm *comm, int algorithm,
                                const uint32_t *inner_keys, const uint32_t *inner_vals, size_t inner,
                                const uint32_t *outer_keys, const uint32_t *outer_vals, size_t outer,
                                const hjgpu_phj_params *phj_params, const hjgpu_npj_params *npj_params,
                                const hjgpu_host_rows *rows, hjgpu_result *result, hjgpu_multi_stats *stats);

/* ---- data generator (write.cpp / generate_data_for_join, cpra2.cpp:1578-1696):
 * statistical contract only — non-zero build keys, unique when outer_total >= inner_total
 * (write.cpp's semantics otherwise: min(inner, outer) distinct keys, the build side repeats
 * them — BASELINE configs[0], 1 M probe x 16 M build, has 16 copies per key), probe keys drawn
 * from them (every build key at least once when outer >= inner), payload = key*factor,
 * both sides in pseudo-random order; counter-based, so any shard
 * [outer_begin, outer_begin+outer_count) of the probe side can be produced
 * independently on its own GPU. */
int  hjgpu_generate(hjgpu_ctx *ctx, uint64_t seed, size_t inner, size_t outer_total,
                    size_t outer_begin, size_t outer_count,
                    uint32_t inner_factor, uint32_t outer_factor,
                    uint32_t *d_inner_keys, uint32_t *d_inner_vals,   /* may be NULL */
                    uint32_t *d_outer_keys, uint32_t *d_outer_vals,   /* may be NULL */
                    void *stream);
/* Same relations, but also the build side in ranges: rows [inner_begin, +inner_count)
 * of the inner_total-tuple build relation (CPRA across GPUs: every GPU owns a chunk of
 * BOTH relations, cpra2.cpp:1737-1742). */
int  hjgpu_generate_range(hjgpu_ctx *ctx, uint64_t seed, size_t inner_total, size_t outer_total,
                          size_t inner_begin, size_t inner_count, size_t outer_begin, size_t outer_count,
                          uint32_t inner_factor, uint32_t outer_factor,
                          uint32_t *d_inner_keys, uint32_t *d_inner_vals,
                          uint32_t *d_outer_keys, uint32_t *d_outer_vals, void *stream);
/* As hjgpu_generate_range, but the repeat picks of the probe side follow a Zipf law of exponent
 * `zipf` over the build keys (0 = uniform): the `zipf` argument of ./write (write.cpp:1685-1686,
 * whose own Zipf walk is unfinished).  Every build key still appears at least once
 * when outer_total >= inner_total, so with unique build keys the join aggregates remain
 * count = |S| and the column sums of S. */
int  hjgpu_generate_zipf(hjgpu_ctx *ctx, uint64_t seed, size_t inner_total, size_t outer_total,
                         size_t inner_begin, size_t inner_count, size_t outer_begin, size_t outer_count,
                         uint32_t inner_factor, uint32_t outer_factor, double zipf,
                         uint32_t *d_inner_keys, uint32_t *d_inner_vals,
                         uint32_t *d_outer_keys, uint32_t *d_outer_vals, void *stream);
/* As hjgpu_generate_zipf, with write.cpp's SELECTIVITY (write.cpp:1685-1689: with d = min(inner, outer) distinct
 * keys per side, join_d = d * selectivity of them are common: the build side draws from unique[0, d), the probe
 * side from unique[d - join_d, 2d - join_d)), so a full-size workload can hold probe tuples WITHOUT a match.
 * `expected` (may be NULL; needs outer_total >= inner_total, i.e. unique build keys): the aggregates that the join
 * of the generated probe range [outer_begin, +outer_count) with the WHOLE build side must return, accumulated
 * while the tuples are generated ("accumulate the expected aggregates during generation");
 * the ranges of several GPUs add up. */
int  hjgpu_generate_select(hjgpu_ctx *ctx, uint64_t seed, size_t inner_total, size_t outer_total,
                           size_t inner_begin, size_t inner_count, size_t outer_begin, size_t outer_count,
                           uint32_t inner_factor, uint32_t outer_factor, double zipf, double selectivity,
                           uint32_t *d_inner_keys, uint32_t *d_inner_vals,
                           uint32_t *d_outer_keys, uint32_t *d_outer_vals, hjgpu_result *expected, void *stream);
/* sum over a column of key, key*f_a, key*f_b (mod 2^32 per term, uint64 sums):
 * the analytic join aggregates of a selectivity-1 workload.
 * The kernel is a plain 16-byte-load streaming read; hjgpu_get_stats().ms_total after
 * the call is its duration (bench.py's empirical streaming-read ceiling). */
int  hjgpu_column_sums(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n,
                       uint32_t f_a, uint32_t f_b, uint64_t sums[3], void *stream);

/* Measurement helper: duration of a plain streaming read (16-byte loads, nothing computed)
 * of `bytes` (a multiple of 64 KiB is read) at d_ptr: the empirical HBM-read ceiling of this
 * device that bench.py reports next to the kernels' rates. */
int  hjgpu_stream_read_ms(hjgpu_ctx *ctx, const void *d_ptr, size_t bytes, float *ms, void *stream);
/* Measurement helper: duration of `reads` independent pseudo-random 64-byte line reads out of the `bytes` at d_ptr
 * (64-byte aligned), four lanes per line and four lines in flight per quad - the NPJ probe's access shape without the
 * join (npj.cpp:216-364 gathers one bucket per lane the same way).  The empirical ceiling bench.py prices NPJ against:
 * out of a table that does not fit the L2 the limit is memory-side requests per second (53-59 G/s for any request size
 * from 16 to 128 bytes, profiles/r03_request_size.txt), not bytes. */
int  hjgpu_random_line_read_ms(hjgpu_ctx *ctx, const void *d_ptr, size_t bytes, size_t reads, float *ms, void *stream);
/* Measurement helper: duration of `ops` independent pseudo-random 8-byte compare-and-swaps (expected 0) into the `bytes` at
 * d_ptr, which are zeroed first (outside the timed span) - the NPJ build's access shape without the join (npj.cpp:196-210:
 * one CAS of an empty bucket per build tuple).  in_flight = 1, 2, 4 or 8 CAS per lane; load_first: a plain load of the
 * bucket before the CAS, as the build skips taken buckets.  The empirical ceiling bench.py prices the NPJ build against. */
int  hjgpu_random_cas_ms(hjgpu_ctx *ctx, void *d_ptr, size_t bytes, size_t ops, int in_flight, int load_first, float *ms, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HJGPU_H */
