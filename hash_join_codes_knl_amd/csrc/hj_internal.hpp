// hj_internal.hpp — launch wrappers shared between the kernel files and the
// C-ABI layer (hjgpu_api.hip).  Everything here is enqueue-only on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/hjgpu.h"
#include "agg_layout.hpp"
#include "compact_layout.hpp"
#include "filter_layout.hpp"
#include "gather_layout.hpp"
#include "group_layout.hpp"
#include "order_layout.hpp"
#include "scatter_layout.hpp"
#include "wide_group_layout.hpp"
#include "wide_lookup_layout.hpp"

typedef unsigned long long u64;

// Geometry constants (also read by the planner on the host side).
// Scatter tile = block * vectors_per_thread * 4 tuples.  Pass 1 of the join pipeline
// (packed output) runs in whole-line mode when its carry buffers fit the LDS beside the
// tile, which decides the tile size from the fan-out; see hj_scatter_config().
// (HJ_LINE_TUPLES, HJ_STREAM_UNIT, HJ_MAX_HEAVY and the LDS layout of a K6 workgroup: scatter_layout.hpp)
struct ScatterConfig { int block, vpt; bool carry; };
struct HjTuning;
ScatterConfig hj_scatter_config(const HjTuning &t, int pass, uint32_t F, bool out_packed);
int hj_scatter_tile(const HjTuning &t, int pass, uint32_t F, bool out_packed);
constexpr int HJ_JOIN_SLICE    = 1 << 16;       // probe tuples per work item (target)
// A build partition larger than one LDS table is joined in several table fills; the fills of such a
// partition are dealt to up to this many work items per probe slice (a heavy build key otherwise leaves
// hundreds of fills, each re-streaming the probe slice, to ONE workgroup).
constexpr int HJ_JOIN_FILL_GROUPS = 64;
// entries of the work-item directory: every partition has >= 1 probe slice, slices of ~HJ_JOIN_SLICE rows
inline size_t hj_join_items_capacity(size_t partitions, size_t outer_rows)
{
    return (partitions + outer_rows / HJ_JOIN_SLICE + 1) * HJ_JOIN_FILL_GROUPS;
}

// Join-kernel geometry: threads per workgroup, log2 of the LDS table slots, and
// probe vectors each lane keeps in flight.  Default 512 / 8192 slots (64 KiB) / 2;
// the "join_cfg" option ("block,log2slots,batch") selects another built variant (tuning).
struct JoinConfig {
    int block, log2slots, batch;
    int slots() const { return 1 << log2slots; }
    int cap() const { return slots() / 2; }      // max build tuples per table fill (load <= 0.5)
};
// 16 K-slot tables (128 KiB of LDS, one 1024-thread workgroup per CU): half the partitions for the same build
// side.  Chosen when the 8 K-slot tables would need more than HJGPU_MAX_PARTS partitions (|R| > ~114 M).
const JoinConfig &hj_join_config_big();
// is this geometry among the built instances of join_kernel (with a _UNIQUE instance, if asked for)?
bool hj_join_config_built(const JoinConfig &c, bool unique);

// Tuning / test switches of ONE context.  They are read from the environment once, in hjgpu_create
// (HJGPU_<NAME>), and can be set per context with hjgpu_set_option; nothing on a launch path looks at
// the environment or at mutable process-wide state, so contexts on different host threads (and on
// different devices) do not share anything.
struct HjTuning {
    int range_tiles = 0;            // "range_tiles": tiles per pass-1 range (0 = planned)
    bool dense2 = false;            // "dense2": dense final layout instead of line-aligned partitions
    bool npj_refhash = false;       // "npj_refhash": whole-join NPJ with the reference's bucket hash
    bool no_broadcast = false;      // "no_broadcast": no broadcast join for tiny build sides
    bool force_chained = false;     // "force_chained": chained fallback tables everywhere (tests)
    bool scatter_prof = false;      // "scatter_prof": K6 phase stamps (diagnostics; synchronises)
    bool unique = false;            // "unique": stop a probe at its first match (_UNIQUE, npj.cpp:288-290)
    bool piece_interleave = true;   // "piece_interleave": pass 2 over arrived pieces takes its tiles partition by partition (PlanArgs::seg_interleave)
    bool merged_plan = true;        // "merged_plan": whole joins on resident columns plan both relations with one set of K5 launches
    int placement = 12;             // "placement": candidate allocations tried for a large pass-1 twin (1 = take the first).  What makes a
                                    // block fast is its physical pages' spread over the memory channels (L2 tag / DRAM-credit stalls,
                                    // profiles/r04_placement_counters.txt): nothing to choose, only to measure.  A cap of 4 was tried in round 4
                                    // and left 3 of 12 fresh processes without a fast block (profiles/r04_placement_log.txt: 10 of 32
                                    // candidates are fast); the search stops at the first fast one, 3 candidates on average.
    int placement_ms = 500;         // "placement_ms": wall-clock budget of one placement search (0 = none): when it is spent the best block so far is
                                    // taken (round 4's driver run spent 3.07 s in a search that found no fast block among twelve)
    bool placement_log = false;     // "placement_log": the search prints every candidate's fill time and its choice to stderr (diagnostics)
    bool exact_probe_counts = false;    // "exact_probe_counts": every join histograms its probe side (K4) - no claimed probe side (A/B, tests)
    int probe_slack = 12;           // "probe_slack": per cent of slack (plus 8 sigma + 64 rows) in the claimed probe side's optimistic regions;
                                    // 0 = none at all (tests: forces the exact fallback)
    bool solo = false;              // "solo": the caller promises that NOTHING else runs on the device beside this context's blocking joins (one
                                    // process, one stream - the reference's programs): their partial-line stores (K6) stay plain,
                                    // 0.34 ms per 64 M x 1 G step faster.  Default 0: every store that may sit dirty in an L2 is non-temporal (round 5:
                                    // plain stores are lost beside other queues' kernel boundaries, 1.5 in 10^4 pipeline steps)
    bool audit = false;             // "audit" (diagnostics): every stage leaves a checksum of its output (audit_kernels.hip, hjgpu_audit_read)
    int hist_min_lds = 0;           // "hist_min_lds" (diagnostics): K4 asks for at least this many bytes of LDS per workgroup (nothing else then shares its CU)
    int reserve_cus = 0;            // "reserve_cus": CUs that K6's persistent grid leaves free (multi-GPU: room for RCCL's kernels)
    // "host_batch": probe rows per batch of the host calls.  -1 (default): the materialising call in batches of 64 Mi rows
    // (its rows go home behind the upload); the aggregate call uploads whole columns while they fit the device's free
    // memory (its device time is then that of ONE join over the whole probe side: 8.5 ms at 64 M x 1 G against 20 ms as the
    // sum of fifteen 64 Mi-row joins - the wall clock is the upload's either way) and falls back to batches when they do not.
    // 0: never batch; n > 0: always, n rows per batch.
    long long host_batch = -1;
    // Grouped plans (a third partitioning pass, hjgpu_api.hip phj_grouped): a build side of "group_from" tuples and more is
    // first split, with the probe side, into key-disjoint groups of about "group_inner" build tuples (64 M: 8 K-slot tables well
    // below their capacity; 1 G x 4 G: 68.1 ms against 72.4 at 100 M and 71.6 at 200 M, profiles/r04_grouped_sweep.txt), each joined by the
    // two-pass plan (the reference plans up to four passes from the partition count, phj.cpp:1791-1808).  group_from 0 = never.
    // "group_always" 1: every build side of group_from tuples and more (tests); 0: only where the cost estimate in
    // grouped_groups() says the extra pass pays (several table fills per partition AND a probe side large enough).
    long long group_from = 300000000, group_inner = 64000000;
    bool group_always = false;
    // "group_device" (default 1): a grouped plan is planned ON THE DEVICE - the groups' sizes and first rows stay in device memory
    // (group_desc_kernel), every kernel of a group's join reads them from there, and the whole plan is one stream-ordered sequence like
    // any other join: enqueue-only calls return at once, nobody waits for pass 0 (phj.cpp:1791-1863 plans and runs its passes inside
    // run_hj).  The workspace is sized for groups of up to (1 + "group_slack" / 100) x the mean group ("group_slack": per cent, default
    // 50); a group beyond that (heavy duplicates) is skipped and flagged, the result marked invalid, and the join is done again by the
    // HOST-planned form (option 0: always that form - the calling thread waits for pass 0 and for every group) at the caller's next
    // blocking touch point (the blocking calls themselves; hjgpu_get_async_status for the enqueue-only ones).
    bool group_device = true;
    int group_slack = 50;
    long long batch_tuples = 0;     // "batch_tuples": probe-side tuples per partitioning batch (0 = no batching, the default)
    JoinConfig join = {512, 13, 2}; // "join_cfg"
    int scatter_cfg[2][3] = {{0, 0, -1}, {0, 0, -1}};   // "scatter_cfg" / "scatter2_cfg": block, vpt, carry; block 0 = planned
};
void hj_tuning_from_env(HjTuning *t);
// returns false for an unknown name or a malformed value
bool hj_tuning_set(HjTuning *t, const char *name, const char *value);
inline const JoinConfig &hj_join_config_of(const HjTuning &t, bool big_tables) { return big_tables ? hj_join_config_big() : t.join; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device only: one flag per
// (kernel instance, device), so a process that drives several GPUs opts in on each of them.
struct HjPerDeviceOnce { unsigned char done[64]; };
int hj_allow_dynamic_lds(const void *kernel, int bytes, HjPerDeviceOnce *once);

// Geometry of partitioning pass 1, known on the host (sizes + alignment only):
// each chunk (segment) is cut into `ranges_per_chunk` contiguous ranges of whole
// tiles.  K4 counts per range, K5 turns the counts into per-range write bases,
// and K6 pass 1 walks the same ranges with private cursors - no global atomics.
constexpr uint32_t HJ_MAX_RANGE_ENTRIES = 1u << 24;   // ranges * F1 kept below this (64 MiB of counts)
// Independently partitioned chunks of a relation (CPRA: the reference's #threads, cpra2.cpp:1757-1827, 2023; its runs used 129
// threads and more - `./cpra 129 ...` is taken as asked -, the result does not depend on the number).  Beyond 8 chunks the plan is always two passes with
// line-aligned final partitions: the join then sees ONE region per partition whatever the number of chunks.
constexpr uint32_t HJ_MAX_CHUNKS = 256;
// work-claim counters inside MetaLayout::tickets (uint32 words, zeroed per join)
constexpr uint32_t HJ_TICKET_K4 = 0;                          // K4: [r * HJ_MAX_CHUNKS + chunk]
constexpr uint32_t HJ_TICKET_K6 = 2 * HJ_MAX_CHUNKS;          // K6: [2 * r + pass - 1]
constexpr uint32_t HJ_TICKET_MULTI_FILL = 2 * HJ_MAX_CHUNKS + 8;
constexpr uint32_t HJ_TICKET_JOIN = 2 * HJ_MAX_CHUNKS + 10;          // K7+K8: two uint64 work counters (8-byte aligned: the block starts on one), the
constexpr uint32_t HJ_TICKET_JOIN2 = 2 * HJ_MAX_CHUNKS + 12;         // second for the multi-fill half of a _UNIQUE join - zeroed with the tickets, per join
constexpr uint32_t HJ_TICKET_JOIN3 = 2 * HJ_MAX_CHUNKS + 14;         // third: the marking launch of a full outer join's multi-fill items
constexpr uint32_t HJ_TICKET_WORDS = 2 * HJ_MAX_CHUNKS + 16;
struct Pass1Geom {
    u64 n, part;                    // chunk c = rows [part * c, c + 1 == chunks ? n : part * (c + 1)): thread_beg / thread_end with
                                    // alignment 16 (npj.cpp:516-529; cpra2.cpp:1737-1742) - computed, not stored: any number of chunks
#if defined(__HIPCC__)
    __host__ __device__
#endif
    u64 beg(uint32_t c) const { return c >= chunks ? n : part * c; }
    uint32_t chunks;
    uint32_t align;                 // (address of the key column / 4) % 4
    uint32_t ranges_per_chunk;      // ceil(tiles of the largest chunk / tiles per range)
    uint32_t tile;
};
#if defined(__HIPCC__)
__host__ __device__
#endif
inline u64 hj_tiles_of(u64 b, u64 e, uint32_t align, uint32_t tile)
{
    if (e <= b) return 0;
    const u64 gb = (align + b) & ~3ull, ge = align + e;
    return (ge - gb + tile - 1) / tile;
}

// One partitioning pass over `nseg` independent input segments.
struct ScatterArgs {
    const uint32_t *kin, *vin;      // input columns (in_packed: kin = packed tuples, vin unused)
    uint32_t *kout, *vout;          // output columns (out_packed: kout = packed tuples, vout unused)
    uint32_t in_packed, out_packed; // packed tuple = payload << 32 | key (8 bytes)
    const u64 *seg_off;             // [nseg+1] element offsets of the segments in kin/vin
    const u64 *tile_prefix;         // [nseg+1] exclusive prefix of tiles per segment
    const uint4 *tile_desc;         // pass 2: [tiles][2] {first row, end row of the segment | first slot of the tile, cursor row}
    u64 *cursors;                   // [nseg*F] pass 2: absolute output positions, advanced atomically;
                                    //          aligned_claims: lines claimed | tail tuples << 32
    const u64 *part_start, *part_end; // pass 2, aligned_claims: [nseg*F] first row / one past the last row of every partition
    uint32_t aligned_claims;
    uint32_t nseg, F, factor;
    uint32_t in_align;              // (address of kin / 4) % 4, same for vin
    // pass 1 only (ranged == 1): per-range bases instead of atomic cursors
    uint32_t ranged;
    uint32_t *work_counter;         // device, zeroed per launch: ticket of the next unclaimed range (pass 1) / tile (pass 2)
    Pass1Geom geom;
    uint32_t range_begin, range_count;   // pass 1: this launch covers ranges [range_begin, +range_count) (0, 0 = all)
    const u64 *range_base;          // [ranges][F] absolute output position of each (range, partition)
    u64 *prof;                      // diagnostics (HJGPU_SCATTER_PROF=1): s_memtime ticks per phase, else NULL
    uint32_t nt_partial;            // 1: the 8-byte (partial-line) stores are non-temporal too (every launch that is not solo: selects the
                                    // NTP instance of the kernel, see k6_store8)
    const u64 *dyn;                 // pass 1 of a device-planned group (else NULL): {first row, rows} of the input inside kin / vin, in device
                                    // memory - geom.n / geom.part are computed from it in the kernel (geom holds the CAPACITY's ranges and tile)
    // claimed pass 1 (the probe side of a blocking join, no K4): partition p writes [p * claim_cap, (p + 1) * claim_cap) of kout, whole
    // lines from the front and the workgroups' last tails from the back; claim_cursors[16 p] = lines | tail tuples << 32 (zeroed per join)
    u64 *claim_cursors;
    u64 claim_cap;
    uint32_t *claim_overflow;       // device flag: an optimistic region (pass 1 claimed, or pass 2 into claimed final regions) was full
};

// What a join reports (HJGPU_FLAG_SEMI / _ANTI / _LEFT_OUTER / _RIGHT_OUTER / _RIGHT_SEMI / _RIGHT_ANTI, derived once by hj_join_mode): every match of a
// probe tuple (inner join), ONE row (key, outer_val) per probe tuple that has a match (semi-join) / that has none (anti-join), every match plus ONE row
// (key, outer_val, HJGPU_NULL_VAL) per probe tuple that has none (left outer join), or ONE row (key, inner_val) per BUILD tuple whose key
// a probe tuple carries (right semi-join) / no probe tuple carries (right anti-join).
enum : uint32_t { HJ_MODE_INNER = 0, HJ_MODE_SEMI = 1, HJ_MODE_ANTI = 2, HJ_MODE_LEFT_OUTER = 3, HJ_MODE_RIGHT_OUTER = 4, HJ_MODE_FULL_OUTER = 5,
                  HJ_MODE_MARK = 6 /* kernels only: a launch that marks and reports nothing - the multi-fill items of a full outer join, every
                                      probe of a right semi- / anti-join -, never a join's mode */,
                  HJ_MODE_RIGHT_SEMI = 7, HJ_MODE_RIGHT_ANTI = 8 };
inline uint32_t hj_join_mode(uint32_t flags)
{
    return (flags & HJGPU_FLAG_RIGHT_SEMI) ? HJ_MODE_RIGHT_SEMI : (flags & HJGPU_FLAG_RIGHT_ANTI) ? HJ_MODE_RIGHT_ANTI
         : (flags & HJGPU_FLAG_SEMI) ? HJ_MODE_SEMI : (flags & HJGPU_FLAG_ANTI) ? HJ_MODE_ANTI
         : (flags & HJGPU_FLAG_FULL_OUTER) == HJGPU_FLAG_FULL_OUTER ? HJ_MODE_FULL_OUTER
         : (flags & HJGPU_FLAG_RIGHT_OUTER) ? HJ_MODE_RIGHT_OUTER
         : (flags & HJGPU_FLAG_LEFT_OUTER) ? HJ_MODE_LEFT_OUTER : HJ_MODE_INNER;
}
// the modes that report probe rows without a match: a partition / group / join without build rows still has work
inline bool hj_mode_keeps_unmatched(uint32_t mode) { return mode == HJ_MODE_ANTI || mode == HJ_MODE_LEFT_OUTER || mode == HJ_MODE_FULL_OUTER; }
// the modes that report BUILD rows without a match (right and full outer joins): the probes mark what they hit - one bit per build row
// (PHJ / CPRA: JoinArgs::build_bits) or bucket (NPJ: NpjProbeArgs::bucket_bits) - and a tail kernel behind them reports the rest, so a
// partition / group / join without probe rows still has build rows to report
inline bool hj_mode_keeps_build(uint32_t mode) { return mode == HJ_MODE_RIGHT_OUTER || mode == HJ_MODE_FULL_OUTER; }
// the modes whose rows are build tuples, (key, inner_val), and nothing else (right semi- and anti-joins): every probe only marks (HJ_MODE_MARK),
// the tail kernel reports the marked rows / buckets (right semi-join) or the clear ones (right anti-join).  d_outer_vals is neither read
// nor written
inline bool hj_mode_reports_build(uint32_t mode) { return mode == HJ_MODE_RIGHT_SEMI || mode == HJ_MODE_RIGHT_ANTI; }
// the modes with marks and a tail kernel: the bitmap is allocated, zeroed per join (and per group), and the tail runs behind the probes
inline bool hj_mode_marks_build(uint32_t mode) { return hj_mode_keeps_build(mode) || hj_mode_reports_build(mode); }
// the modes with rows to report where there are build rows and no probe rows (a join, a group): the tail alone.  Not the right semi-join
inline bool hj_mode_build_alone(uint32_t mode) { return hj_mode_keeps_build(mode) || mode == HJ_MODE_RIGHT_ANTI; }
// what such a join is when one side is empty (right semi- and anti-joins stay what they are: no build rows, no rows): without build rows a full outer join is the left outer join (a right outer join the inner
// join: no rows), without probe rows both are the right outer join (the tail alone)
inline uint32_t hj_mode_for_sides(uint32_t mode, bool inner_rows)
{
    if (inner_rows) return mode;
    return mode == HJ_MODE_FULL_OUTER ? (uint32_t)HJ_MODE_LEFT_OUTER : mode == HJ_MODE_RIGHT_OUTER ? (uint32_t)HJ_MODE_INNER : mode;
}
// the modes whose rows have two columns (key, outer_val): d_inner_vals is neither read nor written
inline bool hj_mode_rows2(uint32_t mode) { return mode == HJ_MODE_SEMI || mode == HJ_MODE_ANTI; }

struct JoinArgs {
    const uint32_t *rk, *rv, *sk, *sv;   // co-partitioned columns (packed: rk / sk = packed tuples)
    uint32_t packed;                     // 1: payload << 32 | key tuples (the library's own passes)
    const u64 *roff, *soff;              // [chunks*P] first row of every partition, chunk-major
    const u64 *rend, *send;              // [chunks*P] one past its last row (dense layouts: roff + 1, soff + 1)
    const u64 *slice_prefix;             // [P+1] exclusive prefix of work items per partition
    const u64 *slices;                   // [P]   probe slices of partition q | fill groups << 32
    const uint32_t *item_part;           // [items] partition of work item w
    uint32_t P, chunks;
    uint32_t f1, F1, f2, F2;             // the passes that produced the partitions
    uint32_t p1_base;                    // pre-partitioned relations: the partitions are pass-1 partitions [p1_base, ...) of F1 (then
                                         // F1 = the exchange's total fan-out; the local partition of a key is
                                         // (H(key, f1, F1) - p1_base) * F2 + H(key, f2, F2))
    uint32_t tf0, tf1;                   // table hash / step multipliers
    uint32_t s_align;                    // (address of sk / 4) % 4
    hjgpu_result *result;                // device, accumulated atomically
    u64 *work_counter;                   // device, zeroed per launch: next unclaimed work item
    // materialised output (NULL keys = aggregate only)
    uint32_t *ok, *oov, *oiv;
    u64 block_size, block_limit;
    u64 *block_counter;                  // device
    u64 *final_offsets;                  // device [gridDim.x] end cursor per workgroup
    uint32_t *overflow;                  // device flag
    uint32_t nt_rows;                    // 1: result rows through non-temporal stores (every join but a solo one: selects the NTROWS instance)
    uint32_t big_tables;                 // hj_join_config_big() instead of hj_join_config()
    // broadcast join (tiny build side, nothing partitioned): P = 1, the relations are the caller's columns, the
    // empty sentinel is *sentinel (a value no build key equals, found by hj_launch_broadcast_meta)
    uint32_t broadcast;
    uint32_t mode;                       // HJ_MODE_*: semi- / anti-joins take exists_probe_kernel, left / right / full outer joins outer_ / right_ / full_probe_kernel (in
                                         // the padding before `sentinel`: the other fields keep their offsets)
    const uint32_t *sentinel;
    uint32_t force_chained;              // tests: skip the cuckoo fast path (option "force_chained")
    uint32_t unique;                     // _UNIQUE (npj.cpp:288-290): a probe key reports its first match only
    // a _UNIQUE join is two launches (join_kernel<.., UNIQUE, DEDUP>): the multi-fill half has its own work counter, goes on
    // in the open output blocks of the single-fill half (same grid, same final_offsets slots) and returns at once when the
    // plan counted no multi-fill partition (multi_fill, may be NULL = unknown)
    u64 *work_counter2;
    const uint32_t *multi_fill;
    uint32_t resume;                     // 1 (device-planned groups): every wave goes on in the output block its slot of final_offsets names (HJ_NO_CURSOR:
                                         // none yet) - the groups' joins share one block counter, one set of open blocks and ONE close_gaps at the end
    uint32_t s_pieces;                   // claimed probe side: 1 - the probe side has 1 + s_pieces pieces per partition in soff / send (front lines,
                                         // back tails) while the build side has `chunks` = 1; else 0
    // right / full outer joins (hj_mode_keeps_build): one bit per row of the partitioned build array `rk` (bit i = tuple i of the array),
    // zeroed per join; the probes OR in the rows whose key a probe tuple carried, hj_launch_build_unmatched reports the others
    uint32_t *build_bits;
    u64 *work_counter3;                  // full outer joins: the work counter of the launch that marks for the multi-fill items (mark_probe_kernel)
};
// The tail of a right semi- / anti-join (build_rows_kernel), launched like hj_launch_build_unmatched: every row of the partitioned build array
// whose bit in a.build_bits is set (a.mode == HJ_MODE_RIGHT_SEMI) / clear (HJ_MODE_RIGHT_ANTI) leaves as (key, inner_val) - a.oiv is the
// second column, a.oov is not touched - and is added to count / sum_keys / sum_inner_vals.
int hj_launch_build_rows(const JoinArgs &a, const HjTuning &t, int cus, hipStream_t stream);
// The tail of a right / full outer join (build_unmatched_kernel), behind the join's launches on the same stream and with the join's grid:
// every row of the partitioned build array (pieces roff / rend of `a`) whose bit in a.build_bits is clear leaves as (key, HJGPU_NULL_VAL,
// inner_val) and is added to count / sum_keys / sum_inner_vals.  Wave w of workgroup b goes on in the output block that wave left open.
int hj_launch_build_unmatched(const JoinArgs &a, const HjTuning &t, int cus, hipStream_t stream);

struct PlanArgs {
    const u64 *counts[2];     // [chunks*P] fused two-level histograms of R (0) and S (1)
    u64 n[2];                 // relation sizes
    u64 chunk_beg[2][9];      // first row of every chunk (host-known: sizes only) - read when the chunks are pieces of any size
                              // (pre-partitioned relations, <= 8 pieces); regular chunks are computed:
    u64 *more[2] = {nullptr, nullptr};   // chunks > 8: [P] the counters of chunks 8 ... chunks - 1 added up (written by hj_launch_plan)
    uint32_t regular[2];      // 1: chunk c of relation r starts at row chunk_part[r] * c (Pass1Geom::part; up to HJ_MAX_CHUNKS chunks)
    u64 chunk_part[2];
    u64 *off2[2];             // [chunks*P + 1] first row of every final partition
    u64 *end2[2];             // [chunks*P] one past its last row
    uint32_t pad2;            // 1: final partitions start on 128-byte lines (two-pass plans)
    u64 *cur2[2];             // [chunks*P]
    u64 *off1[2];             // [chunks*F1 + 1]
    u64 *cur1[2];             // [chunks*F1]
    u64 *tp1[2];              // [chunks + 1] pass-1 tile prefix
    u64 *seg1[2];             // [chunks + 1] chunk boundaries
    u64 *tp2[2];              // [chunks*F1 + 1] pass-2 tile prefix
    uint4 *tdesc[2];          // [pass-2 tiles][2] per-tile descriptors (one independent load per tile in K6)
    uint32_t tdesc_cap;       // tiles the descriptor table holds
    u64 *slice_prefix;        // [P + 1]
    u64 *slices;              // [P]
    uint32_t *item_part;      // [hj_join_items_capacity] partition of every join work item
    uint32_t chunks, F1, F2;
    uint32_t in_align[2];     // alignment of the caller's input columns
    uint32_t tile1, tile2;    // tuples per tile in pass 1 / pass 2
    uint32_t slice;
    uint32_t cap;             // build rows per LDS table fill of the join kernel that will run (JoinConfig::cap)
    uint32_t mask;            // bit 0: plan R, bit 1: plan S, bit 2: join work items
    uint32_t unique;          // _UNIQUE joins: all table fills of a probe slice stay with ONE work item (see join_kernel); also semi- / anti-joins
    uint32_t anti = 0;        // anti- and left outer joins (hj_mode_keeps_unmatched): a partition with probe rows and no build rows has
                              // work items too (its rows are all reported)
    uint32_t *multi_fill = nullptr;   // += partitions with work whose build rows take more than one table fill (zeroed per join)
    // Chunked relations (one-GPU CPRA), line-aligned final layout: the pass-1 output is laid out PARTITION-major - the
    // chunks' regions of a pass-1 partition lie side by side, off1[c * F1 + p] still says where chunk c writes partition
    // p - so pass 2 sees F1 segments [seg2[p], seg2[p + 1]) exactly as after an unchunked pass 1, and pass 1 of every
    // chunk writes across the whole twin (chunk-major: 3.3 + 3.3 ms for the two passes at 2-8 chunks against 3.0 + 3.05)
    uint32_t p_major = 0;
    // Pieces that lie where they arrived (pre-partitioned relations, chunk-major in memory): pass 2 still takes its tiles
    // partition by partition - all pieces of pass-1 partition 0, then of partition 1 ... - so that every final partition
    // is written in one go (tile order only: entry i of the tile prefix is segment (i % chunks) * F1 + i / chunks)
    uint32_t seg_interleave = 0;
    u64 *seg2[2] = {nullptr, nullptr};   // [F1 + 1] p_major: the pass-1 partitions' bounds
    // a device-planned group (else NULL): {first row, rows} of relation r in device memory; n[r] and chunk_part[r] are then computed from it
    const u64 *dyn[2] = {nullptr, nullptr};
    // claimed probe side (else 0): S has no histogram; its final partition q is the optimistic region [q * s_cap2, (q + 1) * s_cap2)
    // (hj_launch_claimed_desc plans pass 2 of S after pass 1), and the join's probe slices are planned for a FULL region: whatever pass 2
    // leaves in it, no work item gets more than HJ_JOIN_SLICE (+ 1 per piece) probe rows - the bound the <UNIQUE, DEDUP> join's
    // per-row `matched` bitmap is sized for
    u64 s_cap2 = 0;
};

// A relation that arrives pass-1-partitioned in pieces (the multi-GPU CPRA's receiving side): piece c = rows
// [b[c], b[c + 1]) of one packed array, c < chunks <= 8 (one piece per source rank).
struct HjChunks {
    u64 b[9];
    uint32_t chunks;
};
int hj_launch_hist_packed(const u64 *tuples, const HjChunks &ch, uint32_t f1, uint32_t F1tot, uint32_t p1_base,
                          uint32_t F1, uint32_t f2, uint32_t F2, u64 *counts, int cus, hipStream_t stream);
int hj_launch_hist2(const uint32_t *keys, const Pass1Geom &geom,
                    uint32_t f1, uint32_t F1, uint32_t f2, uint32_t F2,
                    u64 *counts, uint32_t *range_counts, uint32_t *work_counter /* [chunks], zeroed */,
                    int cus, hipStream_t stream, size_t min_lds = 0, const u64 *dyn = nullptr /* device: {first row, rows}, see ScatterArgs::dyn */);
// Grouped plans on the device: from pass 0's offsets (dense prefixes of the F0 = G * bins counters of both relations) to one descriptor per
// group, desc[g] = {build first row, build rows, probe first row, probe rows} (first rows as pass 0 laid the groups out: hj_group_shift).
// A group with an empty side gets no rows at all (nothing can match; anti / left outer: a group without build rows keeps its probe rows); one beyond
// cap_r / cap_s rows gets none either and raises *skew.
int hj_launch_group_desc(const u64 *roff, const u64 *soff, uint32_t G, uint32_t bins, u64 cap_r, u64 cap_s, u64 n_r, u64 n_s, u64 *desc, uint32_t *skew,
                         hipStream_t stream, bool anti = false, bool keep_build = false /* right / full outer: a group without probe rows keeps its build rows */);
// d_result of a device-planned grouped join: the aggregates, or all ones when a group was skipped (*skew != 0): never a plausible partial count
int hj_launch_group_result(const hjgpu_result *state, const uint32_t *skew, hjgpu_result *d_result, hipStream_t stream);
// own_count > 0 (chunks == 1): partitions [own_first, own_first + own_count) are laid out behind all others
// group_bins > 0 (chunks == 1, own_count == 0): groups of group_bins neighbouring partitions, each group on a 128-byte
// line: group g (whose dense start is row `dense`) starts at row dense + hj_group_shift(dense, g)
int hj_launch_range_base(const uint32_t *range_counts, const u64 *off1, u64 *range_base,
                         uint32_t chunks, uint32_t ranges_per_chunk, uint32_t F1, hipStream_t stream,
                         uint32_t own_first = 0, uint32_t own_count = 0, uint32_t group_bins = 0);
// 32 rows = one 128-byte line of a uint32 column.  Rounding the dense start up and adding one line per group keeps the
// groups apart whatever their sizes: start(g + 1) - start(g) >= rows(g) - 31 + 32.
__host__ __device__ inline u64 hj_group_shift(u64 dense_start, uint32_t g)
{
    return ((dense_start + 31) & ~(u64)31) - dense_start + (u64)32 * g;
}
int hj_launch_plan(const PlanArgs &a, hipStream_t stream);
// Pass 2 of a claimed probe side, planned from pass 1's cursors (claim_cursors[16 p] = lines | back tuples << 32, regions of cap1
// tuples): two segments per pass-1 partition - its front lines and its back tails - cut into tiles of `tile2`; the descriptors go to
// tdesc (at most tdesc_cap) and their number to *total.  A set *overflow (pass 1 found a region full) plans no tile at all.
// The join's view of a claimed probe side after pass 2: partition q's region [off2[q], end2[q]) holds cur2[q] = lines | tails << 32 -
// pieces_beg / pieces_end [2P] = its front lines (q) and its back tails (P + q), clamped to the region (JoinArgs::s_pieces = 1)
int hj_launch_claimed_pieces(const u64 *off2, const u64 *end2, const u64 *cur2, uint32_t P, u64 *pieces_beg, u64 *pieces_end, hipStream_t stream);
int hj_launch_claimed_desc(const u64 *claim_cursors, u64 cap1, uint32_t F1, uint32_t F2, uint32_t tile2, uint4 *tdesc, uint32_t tdesc_cap,
                           u64 *total, uint32_t *overflow, hipStream_t stream);
// Batched partitioning of ONE relation (single chunk): the relation's pass-1 ranges are cut into batches of
// `ranges_per_batch`; pass 1 of a batch writes into a small REUSED buffer (dense layout starting at 0) and pass 2 of
// the batch reads it right away, while it is still in the 256 MiB Infinity Cache - the intermediate copy of the
// relation (16 of PHJ's 44 bytes per probe tuple) then mostly never reaches HBM.  This kernel derives, from K4's
// per-range counts: boff[b][F1 + 1] (the batch's pass-1 layout), range_base[range][F1] (write bases inside the batch
// buffer), tp2b[b][F1 + 1] (pass-2 tile prefix of the batch) and tdesc[b][cap][2] (its pass-2 tile descriptors).
struct BatchPlanArgs {
    const uint32_t *range_counts;   // [ranges][F1]
    u64 *range_base;                // [ranges][F1]
    u64 *boff;                      // [batches][F1 + 1]
    u64 *tp2b;                      // [batches][F1 + 1]
    uint4 *tdesc;                   // [batches][tdesc_cap][2]
    uint32_t tdesc_cap;
    uint32_t ranges, ranges_per_batch, F1, F2, tile2;
};
int hj_launch_batch_plan(const BatchPlanArgs &a, uint32_t batches, hipStream_t stream);
int hj_launch_scatter(const ScatterArgs &a, const HjTuning &t, int cus, hipStream_t stream);
int hj_launch_join(const JoinArgs &a, const HjTuning &t, int cus, hipStream_t stream);
int hj_launch_exscan(const u64 *in, u64 *out, uint32_t n, hipStream_t stream);
int hj_launch_offsets_to_counts(const u64 *off, u64 *counts, uint32_t P, hipStream_t stream);

// a run-time flag as a compile-time one: f(std::true_type) or f(std::false_type) - how the launchers pick a kernel instance
template <class F>
inline void hj_with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// NPJ
int hj_launch_npj_build(const uint32_t *keys, const uint32_t *vals, size_t n, u64 *table,
                        size_t buckets, uint32_t factor, uint32_t *zero_key_flag,
                        int cus, hipStream_t stream, bool line_hash = false);
struct NpjProbeArgs {
    const uint32_t *keys, *vals;
    size_t n;
    const u64 *table;
    size_t buckets;
    uint32_t factor;
    uint32_t line_hash;                  // 1: walks start on 64-byte lines (the library's own tables)
    uint32_t unique;                     // _UNIQUE (npj.cpp:288-290): the walk ends at the key's first match
    uint32_t mode;                       // HJ_MODE_*: semi- / anti-joins take npj_exists_*_kernel (rows without inner_val), left outer
                                         // joins npj_outer_*_kernel
    hjgpu_result *result;
    uint32_t *ok, *oov, *oiv;
    u64 block_size, block_limit;
    u64 *block_counter;
    u64 *final_offsets;
    uint32_t *overflow;
    uint32_t *bucket_bits;               // the modes that mark (hj_mode_marks_build): one bit per bucket, zeroed per join; the probes OR in every bucket they match
};
// The tail of a right / full outer NPJ join (npj_unmatched_kernel), with the probe's grid (`grid`; its waves go on in the probe's open
// output blocks when `resume`): every tuple of the table whose bucket's bit is clear leaves as (key, HJGPU_NULL_VAL, inner_val)
int hj_launch_npj_unmatched(const NpjProbeArgs &a, int grid, bool resume, hipStream_t stream);
// The tail of a right semi- / anti-join (npj_rows_kernel): every tuple of the table whose bucket's bit is set (a.mode == HJ_MODE_RIGHT_SEMI) /
// clear (HJ_MODE_RIGHT_ANTI) leaves as (key, inner_val), a.oiv the second column.  No probe has reported anything: no open blocks to resume
int hj_launch_npj_rows(const NpjProbeArgs &a, int grid, hipStream_t stream);
int hj_launch_npj_probe(const NpjProbeArgs &a, int cus, hipStream_t stream, int *grid_out);
// Positional look-up (hjgpu_npj_lookup*): vals_out[i] = the payload of the first build tuple the walk of keys[i] meets (HJGPU_NULL_VAL: none),
// bit i of match_bits = it met one; either may be NULL.  keys, vals_out and match_bits are 16-byte aligned.  count / sum_keys / sum_inner_vals
// of the matched rows are added to *result.  line_hash: the library's own tables (npj_lookup_line_kernel), else the reference's hash
// (npj_lookup_kernel).  The grid is hj_npj_probe_grid's; n == 0 launches nothing.
struct NpjLookupArgs {
    const uint32_t *keys;
    size_t n;
    const u64 *table;
    size_t buckets;
    uint32_t factor;
    uint32_t line_hash;
    hjgpu_result *result;
    uint32_t *vals_out;
    uint32_t *match_bits;
};
// LDS look-up (hjgpu_lookup*, join_kernels.hip lds_lookup_kernel): NpjLookupArgs' outputs and aggregates for a build side that fits one LDS
// table (inner <= 4096: the 8 K-slot table, two workgroups per CU; up to hj_join_config_big().cap(): the 16 K-slot table, one).  Every
// workgroup of one persistent grid fills its own table from rk / rv, then streams `keys`.  A build key 0 raises *zero_key and is skipped.
// keys, vals_out and match_bits are 16-byte aligned; either output may be NULL.  One launch; inner == 0 && n == 0 launches nothing.
struct LdsLookupArgs {
    const uint32_t *rk, *rv;             // the caller's build columns
    const uint32_t *keys;                // the probe column
    size_t n;
    uint32_t inner;
    uint32_t tf0, tf1;                   // table hash / step multipliers (odd)
    uint32_t force_chained;              // tests: skip the cuckoo fast path (option "force_chained")
    hjgpu_result *result;
    uint32_t *zero_key;                  // DevState::zero_key
    uint32_t *vals_out;
    uint32_t *match_bits;
};
// Selected look-ups (hjgpu_lookup_selected*, hjgpu_npj_lookup_table_selected; DESIGN.md section 5 "Selected look-up"): the two look-ups
// above for the rows whose bit is set in select_bits (match_bits' layout, (n + 31) / 32 words, 16-byte aligned).  An unselected row gets
// HJGPU_NULL_VAL and bit 0, is counted in no aggregate and costs no table access.  match_bits may be select_bits itself: a wave reads the
// words it will store, and before it stores them.  The launchers take these structs; select_bits == NULL launches the plain kernel on the
// base slice (both bases end on a pointer: the mask follows at their size).
struct NpjLookupSelArgs : NpjLookupArgs { const uint32_t *select_bits; };
struct LdsLookupSelArgs : LdsLookupArgs { const uint32_t *select_bits; };
static_assert(sizeof(NpjLookupArgs) == 64 && sizeof(NpjLookupSelArgs) == sizeof(NpjLookupArgs) + sizeof(void *), "kernel argument layout: the mask at offset 64");
static_assert(sizeof(LdsLookupArgs) == 80 && sizeof(LdsLookupSelArgs) == sizeof(LdsLookupArgs) + sizeof(void *), "kernel argument layout: the mask at offset 80");
int hj_launch_npj_lookup(const NpjLookupSelArgs &a, int cus, hipStream_t stream);
int hj_launch_lds_lookup(const LdsLookupSelArgs &a, int cus, hipStream_t stream);

// Compaction by bitmap (hjgpu_compact_selected*, gen_kernels.hip; DESIGN.md section 5 "Compaction by bitmap"): two launches over the ranges of
// compact_layout.hpp.  hj_launch_compact_count: counts[g] = the selected rows of range g (select_bits 16-byte aligned, (n + 31) / 32 words).
// hj_launch_compact: out[c][j] = in[c][i_j], rows_out[j] = i_j for the selected rows i_0 < i_1 < ... and j < capacity, from the counts of
// the count launch; workgroup 0 stores their sum to d_count unless that is NULL (the second launch of a call with more than
// HJ_COMPACT_LAUNCH_COLS columns).  hj_launch_compact_total: the sum alone.  All columns and rows_out 16-byte aligned.
constexpr uint32_t HJ_COMPACT_LAUNCH_COLS = 4;
struct CompactArgs {
    const uint32_t *select_bits;
    hj_compact::Layout lay;
    const u64 *counts;                   // [lay.ranges]
    u64 *d_count;
    u64 capacity;
    const uint32_t *in[HJ_COMPACT_LAUNCH_COLS];
    uint32_t *out[HJ_COMPACT_LAUNCH_COLS];
    uint32_t *rows_out;                  // NULL: no row numbers
};
int hj_launch_compact_count(const uint32_t *select_bits, const hj_compact::Layout &lay, u64 *counts, hipStream_t stream);
int hj_launch_compact(const CompactArgs &a, uint32_t ncols, hipStream_t stream);
int hj_launch_compact_total(const u64 *counts, uint32_t ranges, u64 *d_count, hipStream_t stream);

// Grouped aggregation (hjgpu_group_sum*, hjgpu_group_agg*, hjgpu_group_by*, gen_kernels.hip; DESIGN.md section 5 "Grouped aggregation",
// "Aggregate functions", "Wide keys").  Three roads over one argument shape, one emit body and one host path, which differ in the tables - group_layout.hpp's
// (one 64-bit tuple word: up to two key columns) or wide_group_layout.hpp's (a word per key: three and four) - and in what a row contributes:
// plain 32-bit sums, or agg_layout.hpp's function per slot word.
// The aggregation: one persistent grid; every selected row (select_bits NULL: every row) of the key columns and of vals[c] - aggregate c's
// column a - is combined into its tuple's slot of the merge table.  `merge` holds merge_mask + 1 hashed slots (the narrow tables: and the
// slot of tuple 0 behind them), all zero before the launch, as is *overflow, which is raised when a tuple finds no slot.  The emit: the
// occupied slots go to the dense outputs (rows below capacity only), the words of the extremes turned back into the columns' values, and
// their number is added to *d_ngroups, which is 0 before the launch.  All columns 16-byte aligned.
template <class Slot, uint32_t MAX_KEYS>
struct GroupedArgs {
    const uint32_t *select_bits;         // NULL: every row
    u64 n;
    const uint32_t *keys[MAX_KEYS];
    const uint32_t *vals[hj_agg::MAX_AGGS];
    uint32_t nkeys, nvals;
    Slot *merge;
    u64 merge_mask;
    uint32_t *overflow;
};
template <class Slot, uint32_t MAX_KEYS>
struct GroupedEmitArgs {
    const Slot *merge;
    u64 slots;                           // the hashed slots (the narrow tables: the slot of tuple 0 is merge[slots])
    uint32_t nkeys, nvals;
    uint32_t *keys_out[MAX_KEYS];
    u64 *counts_out;                     // NULL: no counts
    u64 *sums_out[hj_agg::MAX_AGGS];
    u64 capacity;
    u64 *d_ngroups;
};
// the functions of a road with aggregates, behind its tables' arguments g
template <class Head>
struct GroupedKindArgs {
    Head g;
    const uint32_t *b[hj_agg::MAX_AGGS]; // SUM_MUL: the second factor's column
    uint32_t fn[hj_agg::MAX_AGGS], flags[hj_agg::MAX_AGGS];
};
template <class Head>
struct GroupedKindEmitArgs {
    Head g;
    uint32_t fn[hj_agg::MAX_AGGS], flags[hj_agg::MAX_AGGS];
};
// (named structs: the kernels' symbols carry these names)
struct GroupArgs : GroupedArgs<hj_group::Slot, hj_group::MAX_KEYS> {};
struct GroupEmitArgs : GroupedEmitArgs<hj_group::Slot, hj_group::MAX_KEYS> {};
struct AggArgs : GroupedKindArgs<GroupArgs> {};
struct AggEmitArgs : GroupedKindEmitArgs<GroupEmitArgs> {};
struct WideArgs : GroupedKindArgs<GroupedArgs<hj_wide::Slot, hj_wide::MAX_KEYS>> {};
struct WideEmitArgs : GroupedKindEmitArgs<GroupedEmitArgs<hj_wide::Slot, hj_wide::MAX_KEYS>> {};
// A road's two launches.  hj_launch_group_sum / _emit: g.nkeys 1 or 2, every function SUM without flags, which the kernels do not read.
// hj_launch_agg_group / _emit: g.nkeys 0 to 2; with no key column no key is read and every selected row goes to the slot of tuple 0
// (merge[merge_mask + 1]) through agg_layout.hpp's scalar grid.  hj_launch_wide_group / _emit: g.nkeys 3 or 4.
int hj_launch_group_sum(const AggArgs &a, int cus, hipStream_t stream);
int hj_launch_group_emit(const AggEmitArgs &e, int cus, hipStream_t stream);
int hj_launch_agg_group(const AggArgs &a, int cus, hipStream_t stream);
int hj_launch_agg_emit(const AggEmitArgs &e, int cus, hipStream_t stream);
int hj_launch_wide_group(const WideArgs &a, int cus, hipStream_t stream);
int hj_launch_wide_emit(const WideEmitArgs &e, int cus, hipStream_t stream);

// Filter (hjgpu_filter_selected*, gen_kernels.hip; DESIGN.md section 5 "Filter"): one persistent grid of filter_layout.hpp's geometry.  Row
// i < n passes when it is selected (select_bits NULL: every row) and preds[p] holds on cols[p][i] for every p < npreds; bits_out (NULL:
// no bitmap; it may be select_bits itself) receives the passing rows in match_bits' layout, and their number is ADDED to *count (NULL:
// no count), which is 0 before the launch.  The mask and all columns 16-byte aligned; n == 0 launches nothing.
struct FilterArgs {
    const uint32_t *select_bits;         // NULL: every row
    uint32_t *bits_out;                  // NULL: the count alone
    u64 *count;                          // NULL: the bitmap alone
    u64 n;
    const uint32_t *cols[hj_filter::MAX_PREDS];
    hj_filter::Norm preds[hj_filter::MAX_PREDS];
};
int hj_launch_filter(const FilterArgs &a, uint32_t npreds, int cus, hipStream_t stream);

// Gather by row number (hjgpu_gather_selected*, gen_kernels.hip; DESIGN.md section 5 "Gather by row number"): one persistent grid of
// gather_layout.hpp's geometry.  Row i < n is gathered when it is selected (select_bits NULL: every row) and idx[i] < src_rows: then
// out[c][i] = src[c][idx[i]] for every c < ncols and bit i of bits_out (NULL: no bitmap; it may be select_bits itself) is 1; every other
// row gets HJGPU_NULL_VAL and bit 0 and reads no source element.  At most one out[c] may be idx itself.  The gathered rows are ADDED to
// counts[0] and the selected rows whose index is neither below src_rows nor HJGPU_NULL_VAL to counts[1] (NULL: no counts), which are 0
// before the launch.  Every pointer 16-byte aligned; n == 0 launches nothing.
struct GatherArgs {
    const uint32_t *select_bits;         // NULL: every row
    const uint32_t *idx;
    uint32_t *bits_out;                  // NULL: no bitmap
    u64 *counts;                         // NULL: no counts
    u64 n;
    uint32_t src_rows;
    const uint32_t *src[hj_gather::MAX_COLS];
    uint32_t *out[hj_gather::MAX_COLS];
};
int hj_launch_gather(const GatherArgs &a, uint32_t ncols, int cus, hipStream_t stream);

// Wide look-up (hjgpu_lookup_wide*, gen_kernels.hip; DESIGN.md section 5 "Wide look-up"): the table of wide_lookup_layout.hpp - `slots`
// slots of hj_wlk::slot_bytes(nkeys) bytes at `table`, 32-byte aligned.  hj_launch_wide_lookup_build: every build row claims a slot on its
// tuple's path and stores its keys there; the table is all zero before the launch and has more slots than `n` rows.  n == 0 launches nothing.
// hj_launch_wide_lookup: one persistent grid; row i < n that is selected (select_bits NULL: every row) gets the payload of the first slot
// on its tuple's path that holds the tuple and bit 1, every other row HJGPU_NULL_VAL and bit 0; count, the sum of key column 0 and the sum
// of the payloads over the matched rows are ADDED to *result.  slots == 0: no table, no row matches.  match_bits may be select_bits itself.
// Every column, the mask, both outputs and the result 16-byte aligned; either output may be NULL; n == 0 launches nothing.
struct WideLookupBuildArgs {
    const uint32_t *keys[hj_wlk::MAX_KEYS];
    const uint32_t *vals;
    u64 n;
    void *table;
    u64 slots;
};
struct WideLookupArgs {
    const uint32_t *select_bits;         // NULL: every row
    const uint32_t *keys[hj_wlk::MAX_KEYS];
    u64 n;
    const void *table;
    u64 slots;
    hjgpu_result *result;
    uint32_t *vals_out;
    uint32_t *match_bits;
};
int hj_launch_wide_lookup_build(const WideLookupBuildArgs &a, uint32_t nkeys, int cus, hipStream_t stream);
int hj_launch_wide_lookup(const WideLookupArgs &a, uint32_t nkeys, int cus, hipStream_t stream);

// Order by (hjgpu_order_by*, gen_kernels.hip; DESIGN.md section 5 "Order by"): a radix sort of a permutation of row numbers by the digit
// passes of order_layout.hpp.  Every pointer 16-byte aligned, d_count 8-byte.
// The LDS road, hj_launch_order_lds: n <= hj_order::LDS_ROWS, ONE workgroup makes the selected row numbers (select_bits NULL: every row),
// sorts them by keys[0 .. nkeys) and writes *d_count = J and, for j < min(J, limit), rows_out[j] (NULL: none) and out[c][j] = in[c][row],
// 8-byte elements where bit c of wide_cols is set.
struct OrderLdsArgs {
    const uint32_t *select_bits;         // NULL: every row
    uint32_t n, nkeys, ncols, wide_cols;
    const void *keys[hj_order::MAX_KEYS];
    uint32_t key_flags[hj_order::MAX_KEYS];
    const void *in[hj_order::MAX_COLS];
    void *out[hj_order::MAX_COLS];
    uint32_t *rows_out;
    u64 limit;
    u64 *d_count;
};
int hj_launch_order_lds(const OrderLdsArgs &a, hipStream_t stream);
// The device road.  hj_launch_order_iota: perm[i] = i for i < rows, *d_count = count.  One pass over the live permutation [0, *d_count),
// cut into lay's ranges: hj_launch_order_histogram leaves counts[digit * ranges + g] and ADDS the digits' totals to totals[256] (0 before
// the launch); hj_launch_order_scan turns them into bases[digit * ranges + g], where range g's first element of that digit goes;
// hj_launch_order_scatter writes perm_out, stably.  perm_in is not perm_out.  hj_launch_order_gather: rows_out and the columns for
// j < min(*d_count, limit) from the sorted permutation.
struct OrderPassArgs {
    const uint32_t *perm_in;
    uint32_t *perm_out;
    const uint32_t *key_words;           // the pass's key column as 32-bit words
    hj_order::Pass pass;
    hj_order::Layout lay;
    const u64 *d_count;
    uint32_t *counts, *bases, *totals;
};
struct OrderGatherArgs {
    const uint32_t *perm;
    const u64 *d_count;
    u64 limit;
    uint32_t ncols, wide_cols;
    const void *in[hj_order::MAX_COLS];
    void *out[hj_order::MAX_COLS];
    uint32_t *rows_out;                  // NULL: no row numbers
};
int hj_launch_order_iota(uint32_t *perm, u64 rows, u64 count, u64 *d_count, int cus, hipStream_t stream);
int hj_launch_order_histogram(const OrderPassArgs &a, hipStream_t stream);
int hj_launch_order_scan(const OrderPassArgs &a, hipStream_t stream);
int hj_launch_order_scatter(const OrderPassArgs &a, hipStream_t stream);
int hj_launch_order_gather(const OrderGatherArgs &a, u64 n, int cus, hipStream_t stream);

// K9: compact the per-wave partially filled tail blocks (npj.cpp:475-514).
// moves: scratch of 2*HJ_MAX_WORKERS entries of 24 bytes + HJ_MAX_WORKERS entries of 8 bytes.
constexpr uint32_t HJ_MAX_WORKERS = 8192;
int hj_launch_close_gaps_ex(uint32_t *k, uint32_t *ov, uint32_t *iv, const u64 *final_offsets,
                            uint32_t nworkers, u64 block_size, const u64 *block_counter,
                            const uint32_t *overflow, void *moves, uint32_t *nmoves,
                            u64 *dense_count, int cus, hipStream_t stream);
int hj_join_workers(const HjTuning &t, int cus, bool big_tables = false);
// Metadata of a broadcast join, written on the device: one partition holding all of R ([0, inner)) and all of S
// ([0, outer)), `nslices` probe slices x `groups` fill groups (item_part must be zeroed by the caller), and a
// sentinel: a value whose low 14 bits no build key shares (inner <= 16383).
struct BroadcastMeta {
    u64 *roff, *rend, *soff, *send, *slice_prefix, *slices;
    uint32_t *sentinel;
};
int hj_launch_broadcast_meta(const uint32_t *inner_keys, size_t inner, size_t outer, uint32_t nslices,
                             uint32_t groups, const BroadcastMeta &m, hipStream_t stream);
int hj_npj_probe_grid(int cus, size_t n);

// option "audit" (audit_kernels.hip): read-only checks of a stage's output, on the stage's stream.  A record is
// HJ_AUDIT_STAGES x {misplaced tuples, sum of keys, sum of payloads, tuples}; a context keeps its last HJ_AUDIT_RING records.
// PHJ / CPRA calls: stage 0 probe side as read, 1 after pass 1, 2 final partitions; 3-5 the same for the build side (5 is
// checked again by every probe of a prepared build side); 6 the join's result (count, three sums); 7 {sequence number, kind
// (0 whole join, 1 build only, 2 probe only, 3 hjgpu_partition_packed*), build rows, probe rows}.  Partitioning calls: 0 input, 1 output.
constexpr int HJ_AUDIT_STAGES = 8, HJ_AUDIT_RING = 256;
struct HjAuditHash { uint32_t f1, F1, p1_base, f2, F2, modulo; };   // partition of a key: ((H(key, f1, F1) - p1_base) * F2 + H(key, f2, F2)); entry i holds partition i % modulo
int hj_audit_partitions(const u64 *tuples, const u64 *beg, const u64 *end /* NULL: beg + 1 */, uint32_t parts, const HjAuditHash &h,
                        u64 *rec, int cus, hipStream_t stream);
int hj_audit_sums_packed(const u64 *tuples, u64 b, u64 e, u64 *rec, int cus, hipStream_t stream);
int hj_audit_sums_columns(const uint32_t *k, const uint32_t *v, u64 n, u64 *rec, int cus, hipStream_t stream);
int hj_audit_own_last(const u64 *prefix, uint32_t F, uint32_t own_first, uint32_t own_count, u64 n, u64 *beg, u64 *end, hipStream_t stream);
int hj_audit_copy(const u64 *src, u64 *dst, uint32_t words, hipStream_t stream);
int hj_audit_meta(u64 *dst, u64 a, u64 b, u64 c, u64 d, hipStream_t stream);

// generator / checksums
int hj_launch_generate(u64 seed, size_t inner, size_t inner_begin, size_t inner_count,
                       size_t outer_total, size_t outer_begin,
                       size_t outer_count, uint32_t inner_factor, uint32_t outer_factor,
                       uint32_t *ik, uint32_t *iv, uint32_t *ok, uint32_t *ov, hipStream_t stream,
                       double zipf = 0.0, double selectivity = 1.0, u64 *d_expect = nullptr);
int hj_launch_stream_read(const void *p, size_t bytes, void *sink16, int cus, hipStream_t stream);
int hj_launch_copy_to_host(void *host_mapped, const void *d, size_t bytes, hipStream_t stream);
int hj_launch_row_sums(const u64 *counts, uint32_t F1, uint32_t F2, u64 *out, hipStream_t stream);
int hj_launch_random_line_read(const void *p, size_t bytes, size_t reads, void *sink16, int cus, hipStream_t stream);
int hj_launch_random_cas(void *p, size_t bytes, size_t ops, int in_flight, bool load_first, void *sink8, int cus, hipStream_t stream);
int hj_launch_fill_probe(void *p, size_t bytes, hipStream_t stream);
// the library's clears and device-to-device copies (gen_kernels.hip): own kernels with non-temporal stores instead of the runtime's
// hipMemsetAsync / hipMemcpyAsync, whose fill and copy kernels store plainly (the store policy: hj_device.hpp)
hipError_t hj_zero_async(void *p, size_t bytes, hipStream_t stream);
hipError_t hj_fill_async(void *p, uint32_t word, size_t bytes, hipStream_t stream);     // every 4-byte word = `word`
hipError_t hj_copy_async(void *dst, const void *src, size_t bytes, hipStream_t stream);
int hj_launch_column_sums(const uint32_t *keys, size_t n, uint32_t fa, uint32_t fb, u64 *sums3,
                          hipStream_t stream);
