// hjgpu_ctx.hpp - what the translation units behind include/hjgpu.h share: the context, its workspace layout, the plan of a
// PHJ / CPRA join, and the planning / enqueue functions of hjgpu_api.hip that the operator-level entry points (hjgpu_ops.hip), the
// column operators (hjgpu_colops.hip) and the host pipelines (hjgpu_host.hip) call.  Internal: nothing outside csrc/ includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>

#include "hj_internal.hpp"
#include "colop_checks.hpp"
#include "build_beside_layout.hpp"


struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

namespace hjapi {
// a relation on the device: its key and payload columns (a prepared or pre-partitioned relation has none) and its rows
struct Rel { const uint32_t *keys = nullptr, *vals = nullptr; size_t rows = 0; };
}

// Small device-resident state of one join.
struct DevState {
    hjgpu_result result;
    u64 block_counter;
    u64 dense;
    u64 work_counter;
    uint32_t overflow;
    uint32_t zero_key;
    uint32_t nmoves;
    uint32_t pad;
    u64 work_counter2;      // the multi-fill half of a _UNIQUE join (hj_launch_join)
    uint32_t group_skew;    // a device-planned grouped join skipped a group that was larger than its workspace (group_desc_kernel)
    uint32_t probe_overflow;    // a claimed probe side did not fit its optimistic regions (K6 / claimed_desc_kernel): the blocking call joins again exactly
};

// probe side (S) is partitioned first, then the build side (R): a caller can overlap the
// arrival of R (e.g. an RCCL broadcast) with the S passes through `inner_ready`
enum { EV_BEGIN = 0, EV_S_HIST, EV_S_PLAN, EV_S_SC1, EV_S_SC2, EV_WAITED,
       EV_R_HIST, EV_R_PLAN, EV_R_SC1, EV_R_SC2, EV_JOIN, EV_GAPS, EV_COUNT };

// what the context ran last: hjgpu_get_stats reads the events by it.  From ALGO_ONE_KERNEL on, one operator between EV_BEGIN and EV_GAPS
// (begin_span) that records EV_S_HIST and EV_JOIN where it has stages
enum Algo { ALGO_NONE = -1, ALGO_NPJ = 0, ALGO_PHJ = 1,        // (PHJ, CPRA and the LDS-road look-up)
            ALGO_ONE_KERNEL = 2,                               // hjgpu_partition*, hjgpu_column_sums, the hjgpu_*_ms probes
            ALGO_COMPACT = 3, ALGO_GROUP_SUM = 4, ALGO_FILTER = 5, ALGO_GATHER = 6, ALGO_GROUP_AGG = 7,
            ALGO_GROUP_BY = 8,                                 // hjgpu_group_by's wide road (three and four key columns)
            ALGO_LOOKUP_WIDE = 9,                              // hjgpu_lookup_wide: EV_S_HIST behind the clear and the build, stats.buckets = its slots
            ALGO_ORDER_BY = 10 };                              // hjgpu_order_by: EV_S_HIST behind the initial permutation, EV_JOIN behind the passes, then the gather

struct hjgpu_ctx {
    int device = 0;
    int cus = 0;
    hipDeviceProp_t prop;
    char err[512];
    DevBuf tmp[8];          // pass-1 / pass-2 twins of the 4 columns (hj.h's [1] scratch columns)
    DevBuf meta;            // histograms, offsets, cursors, tile / work-item prefixes
    DevBuf table;           // NPJ table
    DevBuf state;           // DevState
    DevBuf moves;           // close_gaps move list
    DevBuf final_offsets;   // per-wave end cursors
    DevBuf compact;         // hjgpu_compact_selected: the ranges' counts and the blocking form's count (constant size, made by the first call)
    DevBuf group;           // hjgpu_group_sum: the blocking form's count word, the overflow word and the merge table (group_layout.hpp; grows with the capacity)
    DevBuf count_words;     // hjgpu_filter_selected (the first word) and hjgpu_gather_selected (both): the count words that the kernel adds to - the blocking
                            // forms read them back (16 bytes, made by the first call of either)
    DevBuf wide_lookup;     // hjgpu_lookup_wide: the call's aggregate words and its table (wide_lookup_layout.hpp; grows with the build side)
    DevBuf order;           // hjgpu_order_by: the blocking form's count word, and on the device road the passes' tables and the two permutation buffers
                            // (order_layout.hpp; grows with n)
    DevBuf build_bits;      // right / full outer joins: one bit per row of the partitioned build array (PHJ / CPRA) or per bucket (NPJ)
    hipEvent_t ev[EV_COUNT];
    bool ev_valid[EV_COUNT];
    hjgpu_stats stats;
    Algo last_algo = ALGO_NONE;
    bool last_lookup = false;   // the last operation was a positional look-up (hjgpu_npj_lookup*): no close_gaps, ms_close_gaps is 0
    // hjgpu_phj_build: the partitioned build side (tmp[0] / tmp[4]) and its plan (meta) stay valid until
    // another entry point uses the workspace
    bool prepared = false;
    size_t prepared_inner = 0, prepared_max_outer = 0;
    unsigned char prepared_plan[128];
    HjTuning tune;          // tuning / test switches: environment at hjgpu_create, hjgpu_set_option afterwards
    // hjgpu_join_host*: two page-locked staging buffers for PAGEABLE host columns, made when the first one is seen and kept
    // (hipHostMalloc + hipHostFree of 2 x 32 MiB cost 22 ms per call; page-locked columns never need them)
    // the batched host calls' three streams (upload / join / download), made once: the runtime binds a stream's copies to a
    // DMA engine when it first uses it, and fresh streams in every call ended up with upload and download on ONE engine
    // from the second call on (one after the other: 430 ms instead of 275 for 8.5 GB up and 12 GB down)
    hipStream_t host_streams[3] = {nullptr, nullptr, nullptr};
    void *host_stage[4] = {nullptr, nullptr, nullptr, nullptr};          // [0..1] uploads, [2..3] downloads (both run at once
    hipEvent_t host_stage_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // when result rows go home behind the upload)
    // hjgpu_set_async_output: the next *_async join of this context materialises into these columns (one-shot)
    hjgpu_output pending_out;
    bool has_pending_out = false;
    bool last_had_output = false;   // hjgpu_get_async_status: the last enqueued join wrote result columns
    // claimed probe side: joins whose optimistic regions overflowed and were done again on the exact path; after the first, every later
    // blocking join of the context takes the exact path at once (hjgpu_get_counter "probe_fallbacks" / "probe_exact")
    uint64_t probe_fallbacks = 0;
    bool probe_exact = false;
    // Build side beside the probe side (PhjRun::partition_beside): the context's side stream (non-blocking, made by the first join
    // that takes the form) and the events of the fork and the join inside one call; option "build_beside" (default 1; 0: the one-stream order)
    // and option "build_cus" (0: hj_beside's choice); joins that took the form (hjgpu_get_counter "build_beside"); and whether the last
    // join did, which is how hjgpu_get_stats reads its events
    enum { BESIDE_FORK = 0, BESIDE_PLAN_DONE, BESIDE_R_DONE, BESIDE_EVENTS };
    hipStream_t side = nullptr;
    hipEvent_t beside_ev[BESIDE_EVENTS] = {nullptr, nullptr, nullptr};
    bool build_beside = true;
    int build_cus = 0;
    uint64_t beside_joins = 0;
    bool last_beside = false;
    bool rows_plain = false;        // the join being enqueued is SOLO - a blocking call of a context with option "solo": plain partial-line stores
                                    // in K6 (k6_store8) and plain result rows (join_kernel<..., NTROWS = false>); every other launch writes them non-temporal
    // grouped plans: pass-0 twins of the four columns, the groups' offsets and (device-planned) descriptors, and the call's accumulated
    // phase times (hjgpu_get_stats returns those while stats_override is set; any later operation's first event clears it)
    DevBuf grp[4], grp_off;
    bool stats_override = false;
    hipStream_t aux = nullptr;      // private non-blocking stream: placement probes of the workspace allocator
    // Device-planned grouped joins (phj_grouped_device): one set of phase events per group - the groups' joins are enqueued back to back
    // and nobody waits in between, so hjgpu_get_stats adds the groups' spans up afterwards - and what hjgpu_get_async_status needs to
    // run the join again, host-planned, when a group turned out larger than its workspace (DevState::group_skew)
    hipEvent_t *ev_cur = nullptr;                        // the set record() writes (NULL: ev)
    std::vector<hipEvent_t> grp_ev;                      // [groups][EV_COUNT]
    uint32_t grp_ev_groups = 0;                          // groups of the last device-planned join (0: hjgpu_get_stats reads ev)
    hipEvent_t grp_ev_pass0[3] = {nullptr, nullptr, nullptr};   // begin, pass 0 done, all done
    struct GroupedCall {
        bool valid = false;
        uint32_t chunks = 1;
        hjapi::Rel R, S;
        bool has_prm = false, has_out = false;
        hjgpu_phj_params prm;
        hjgpu_output out;
        hjgpu_result *d_result = nullptr;
    } grp_last;                                          // the last ENQUEUE-ONLY device-planned grouped join of this context
    // option "audit": the last HJ_AUDIT_RING calls' stage records (audit_kernels.hip), the next call's sequence number, and the
    // explicit partition bounds of an own-last layout
    DevBuf audit, audit_lay;
    uint64_t audit_seq = 0;
    // the partition checks of the LAST audited call, as they were launched: hjgpu_audit_recheck does them again with the device quiet
    struct AuditCheck { int stage; const u64 *tuples, *beg, *end; uint32_t parts; HjAuditHash h; };
    std::vector<AuditCheck> audit_checks;
    float ms_reserve = 0;           // wall clock of the workspace growth so far (allocations + placement probes)
    // the last placement search (ensure_placed): candidate blocks it allocated and filled, the kept block's fill time and size,
    // whether the budget (option "placement_ms") ended it
    uint32_t placement_tried = 0, placement_timeboxed = 0;
    float placement_fill_ms = 0, placement_search_ms = 0;
    size_t placement_bytes = 0;
};

namespace hjapi {

const uint32_t DEFAULT_F1 = 0x9E3779B1u, DEFAULT_F2 = 0x85EBCA6Bu;
const uint32_t DEFAULT_TF0 = 0xC2B2AE35u, DEFAULT_TF1 = 0x27D4EB2Fu;
const uint32_t DEFAULT_NPJ_FACTOR = 0x9E3779B1u;
const uint32_t DEFAULT_F0 = 0x7FEB352Du;      // grouped plans: pass 0 (phj_grouped takes another one when a pass factor of the join equals it)

int fail(hjgpu_ctx *ctx, int status, const char *what, hipError_t e = hipSuccess);
// a check of colop_checks.hpp as the context's error: HJGPU_OK, or its status with its text in hjgpu_last_error
inline int refused(hjgpu_ctx *ctx, const colop::Verdict &v) { return v.status == HJGPU_OK ? HJGPU_OK : fail(ctx, v.status, v.text); }

// The partial-line stores (K6) of a SOLO join - a blocking call of a context with option "solo": the caller waits for it and promises
// that nothing else runs on the device beside it - are plain; every other join (enqueue-only, host batches, multi-GPU slices, and
// every blocking call without the option) writes them non-temporal (DESIGN section 3 "Round 5").  The same for the result rows of PHJ / CPRA
// (join_kernel's NTROWS instances); NPJ's rows are always non-temporal.
struct PlainRows {
    hjgpu_ctx *ctx;
    PlainRows(hjgpu_ctx *c, bool blocking) : ctx(c) { if (ctx) ctx->rows_plain = blocking && ctx->tune.solo; }
    ~PlainRows() { if (ctx) ctx->rows_plain = false; }
};

#define HIPCHK(ctx, call)                                                       \
    do {                                                                        \
        hipError_t e_ = (call);                                                 \
        if (e_ != hipSuccess) return fail((ctx), HJGPU_EHIP, #call, e_);        \
    } while (0)
hipError_t hj_event_synchronize(hipEvent_t ev);
hipError_t hj_stream_synchronize(hipStream_t st);

#define CHK(call)                                                               \
    do {                                                                        \
        int s_ = (call);                                                        \
        if (s_ != HJGPU_OK) return s_;                                          \
    } while (0)

int ensure(hjgpu_ctx *ctx, DevBuf &b, size_t bytes);
int ensure_placed(hjgpu_ctx *ctx, DevBuf &b, size_t bytes);

// Wall clock of workspace growth (hjgpu_stats.ms_reserve): the placement search holds and fills up to 12 candidate
// blocks of the probe side's pass-1 twin; it happens at hjgpu_reserve / the first join of a size, never in a timed join
// afterwards, and its cost is reported instead of being invisible.
struct ReserveClock {
    hjgpu_ctx *ctx;
    size_t before;
    std::chrono::steady_clock::time_point t0;
    static size_t held(const hjgpu_ctx *c)
    {
        size_t n = c->meta.cap + c->table.cap + c->state.cap + c->group.cap + c->wide_lookup.cap + c->order.cap;
        for (const DevBuf &b : c->tmp) n += b.cap;
        return n;
    }
    explicit ReserveClock(hjgpu_ctx *c) : ctx(c), before(held(c)), t0(std::chrono::steady_clock::now()) {}
    ~ReserveClock()
    {
        if (held(ctx) != before)
            ctx->ms_reserve += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

uint32_t grouped_groups(const hjgpu_ctx *ctx, size_t inner, size_t outer, const hjgpu_phj_params *prm);
struct GroupLayout { uint32_t G, bins, F0; };
GroupLayout group_layout(uint32_t G);
int grouped_twins(hjgpu_ctx *ctx, const GroupLayout &l, size_t inner, size_t outer);

// K6 occupies a CU completely (one 1024-thread workgroup with ~155 KiB of LDS that lives until the pass ends): a kernel
// that arrives during a pass - RCCL's, on the multi-GPU path - finds no CU until the pass is over.  "reserve_cus" keeps
// some CUs out of K6's grid (work is claimed from a ticket counter, so any grid size finishes the pass).
inline int scatter_cus(const hjgpu_ctx *ctx)
{
    const int n = ctx->cus - ctx->tune.reserve_cus;
    return n < 1 ? 1 : n;
}

inline uint32_t align_of(const void *p) { return (uint32_t)(((uintptr_t)p >> 2) & 3); }

// Carves the meta buffer; must match between sizing and use.
struct MetaLayout {
    u64 *counts[2], *off2[2], *end2[2], *cur2[2], *off1[2], *cur1[2], *tp1[2], *seg1[2], *tp2[2];
    u64 *claim1;                 // [F1 * 16] claimed probe side: pass 1's cursors, one per 128-byte line (zeroed with the counts)
    u64 *claim_total;            // [1] claimed probe side: pass-2 tiles planned by hj_launch_claimed_desc
    u64 *pieces;                 // [4 P] claimed probe side: the join's two pieces per partition (begins [2 P], ends [2 P])
    u64 *seg2[2];                // [F1 + 1] partition-major pass-1 layout of a chunked relation: bounds of the pass-1 partitions
    u64 *more[2];                // [P] more than 8 chunks: the counters of chunks 8 ... C - 1 added up (PlanArgs::more), else NULL
    u64 *slice_prefix, *slices;
    uint32_t *tickets;           // [HJ_TICKET_WORDS] work-claim counters of K4 / K6, the multi-fill count (inside the block zeroed per join)
    uint32_t *item_part;         // [P + items_extra] partition of every join work item
    uint4 *tdesc[2];             // [tdesc_cap][2] pass-2 tile descriptors (K5 -> K6 pass 2)
    size_t tdesc_cap;
    uint32_t *range_counts[2];   // [ranges][F1] pass-1 counts per range (K4 -> K5b)
    u64 *range_base[2];          // [ranges][F1] pass-1 write bases per range (K5b -> K6)
    // batched probe-side partitioning (hj_launch_batch_plan): per-batch pass-1 layout, pass-2 tile prefix,
    // pass-2 tile descriptors, and one ticket word per launch (pass 1 / pass 2 of every batch)
    u64 *boff, *tp2b;
    uint4 *tdescb;
    uint32_t *btickets;
    size_t btickets_bytes;
    size_t counts_bytes;    // both relations, contiguous (zeroed per join)
    size_t total_bytes;
};
MetaLayout carve(void *base, uint32_t C, uint32_t F1, uint32_t P, size_t ranges, size_t items_extra = 0,
                 size_t tiles2 = 0, size_t batches = 0, size_t tdesc_b_cap = 0);
// Launch arguments that many sites share are built here.  The store policy (PlainRows) is applied by these builders and nowhere else outside
// the kernels: ScatterArgs::nt_partial by the K6 builders, JoinArgs::nt_rows by join_output.
// K6 pass 1 of relation r in ranges (every (range, partition) writes from the base K5b laid out): columns kin / vin -> kout / vout, packed
// tuples when vout is NULL.  The caller adds what is its own: claims, a batch's ranges and ticket, a group's dyn.
ScatterArgs scatter_pass1(const hjgpu_ctx *ctx, const MetaLayout &m, int r, const Pass1Geom &geom, uint32_t F, uint32_t factor,
                          const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout);
// The plan kernels' arguments over the layout m, for C chunks of F1 x F2 partitions.  Everything else is zero / NULL until the caller sets
// it: relation sizes, chunk bounds, input alignment, the two-pass layout (pad2, p_major, seg2, more), multi_fill, dyn, and the pass-2 tile
// descriptors (a non-null tdesc adds a tile_desc_kernel launch).
PlanArgs plan_args(const hjgpu_ctx *ctx, const MetaLayout &m, uint32_t C, uint32_t F1, uint32_t F2, uint32_t tile1, uint32_t tile2, bool unique,
                   uint32_t mask);
// A join's result rows: the block protocol into ja when bs > 0 (setup_output's block size and limit), and close_gaps after the join
void join_output(const hjgpu_ctx *ctx, JoinArgs &ja, const hjgpu_output *out, u64 bs, u64 bl, DevState *st);
// (mode: a semi- / anti-join's rows are key and outer_val only, the inner column is left alone - hj_mode_rows2; a right semi- / anti-join's key
// and inner_val only, the outer column is left alone - hj_mode_reports_build)
int close_gaps(hjgpu_ctx *ctx, const hjgpu_output *out, uint32_t workers, u64 bs, DevState *st, hipStream_t stream, uint32_t mode = HJ_MODE_INNER);
// HJGPU_FLAG_SEMI | HJGPU_FLAG_ANTI together, and the other combinations that name two kinds of join: refused
int check_join_mode(hjgpu_ctx *ctx, uint32_t flags);
// an entry point without semi-, anti- and left outer joins refuses those flags (never an inner join in their place); the text names the flag
int refuse_join_mode(hjgpu_ctx *ctx, uint32_t flags, const char *entry);
void choose_fanout(const HjTuning &tune, size_t inner, const hjgpu_phj_params *prm, uint32_t *F1, uint32_t *F2, bool *big_tables);
void record(hjgpu_ctx *ctx, int which, hipStream_t s);
// an operator's timed span begins: whatever events the last one left are void, hjgpu_get_stats reads the new ones as `op`'s
inline void begin_span(hjgpu_ctx *ctx, Algo op, hipStream_t s)
{
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    ctx->last_algo = op;
    record(ctx, EV_BEGIN, s);
}
int audit_begin(hjgpu_ctx *ctx, int kind, size_t inner, size_t outer, hipStream_t stream, u64 **rec);
// hj_audit_partitions into stage `stage` of the call's record, remembered for hjgpu_audit_recheck
int audit_partitions(hjgpu_ctx *ctx, int stage, const u64 *tuples, const u64 *beg, const u64 *end, uint32_t parts, const HjAuditHash &h, u64 *rec,
                     hipStream_t stream);
int refuse_capture(hjgpu_ctx *ctx, hipStream_t stream);
int check_columns(hjgpu_ctx *ctx, const uint32_t *k, const uint32_t *v, size_t n);
int setup_output(hjgpu_ctx *ctx, const hjgpu_output *out, uint32_t workers, u64 *block_size, u64 *block_limit, uint32_t mode = HJ_MODE_INNER);
uint32_t range_tiles_for(const HjTuning &tune, u64 max_tiles, uint32_t F1);
uint32_t ranges_of(const HjTuning &tune, u64 max_tiles, uint32_t F1);
uint32_t ranges_capacity(const HjTuning &tune, u64 max_tiles, uint32_t F1);
Pass1Geom make_geom(const HjTuning &tune, const void *keys, size_t n, uint32_t C, uint32_t F1, bool out_packed, bool capacity = false);

struct PhjPlan {
    size_t ranges, items_extra, tiles2;
    uint32_t C, F1, F2, P;
    uint32_t f1, f2, tf0, tf1;
    bool big_tables;
    bool unique;             // HJGPU_FLAG_UNIQUE / option "unique"; also set for semi-, anti-, left outer, right semi- and right anti-joins (one fill group per slice)
    uint8_t mode;            // HJ_MODE_*: HJGPU_FLAG_SEMI / _ANTI / _LEFT_OUTER (a byte: beside the flags, the plan keeps its size)
    bool first_match;        // the probe walk ends at a key's first match (JoinArgs::unique): `unique`, except for a left outer join without
                             // HJGPU_FLAG_UNIQUE
    // batched probe-side partitioning: 0 batches = off
    uint32_t batch_ranges;   // pass-1 ranges per batch
    uint32_t batch_cap;      // batches the tables hold
    uint32_t batch_tile_cap; // tiles per range the batch buffers are sized for
    size_t tdesc_b_cap;      // pass-2 tile descriptors per batch
    size_t batch_bytes;      // one batch buffer (packed tuples)
    void no_batches() { batch_ranges = batch_cap = batch_tile_cap = 0; tdesc_b_cap = 0; batch_bytes = 0; }
    // pre-partitioned relations (hjgpu_phj_build_prepartitioned): pass 1 was the exchange-level partitioning of the
    // multi-GPU CPRA; F1 = this rank's share k of its fan-out pre_F1tot, partitions [pre_base, pre_base + k)
    uint32_t pre;            // 1: the relations arrive pass-1-partitioned
    uint32_t pre_f1, pre_F1tot, pre_base;
    // claimed probe side (blocking whole joins, PrepareOpts::claim_s): no K4 of S; pass 1 of S writes regions of cap1 tuples per pass-1
    // partition, pass 2 final regions of cap2 tuples (both optimistic, line multiples)
    uint32_t claim_s;
    u64 cap1, cap2;
};
static_assert(sizeof(PhjPlan) <= sizeof(hjgpu_ctx::prepared_plan), "prepared_plan too small");
// the pieces a pre-partitioned relation arrives in (one per source rank)
struct PrePieces {
    const u64 *tuples[2] = {nullptr, nullptr};      // [0] build side, [1] probe side (packed: payload << 32 | key)
    HjChunks ch[2];
    // [chunks][P] fused (piece, final partition) counts of the relation, counted by the SENDERS' histogram pass and
    // delivered with the exchange (hjgpu_phj_probe_prepartitioned_counted_async): K4p is skipped
    const u64 *counts[2] = {nullptr, nullptr};
};
// which stages a phj_enqueue call runs: the whole join, the build side's partitioning (hjgpu_phj_build*), or the probe side's and the join
enum PhjStages { PHJ_WHOLE = 0, PHJ_BUILD_ONLY = 1, PHJ_PROBE_ONLY = 2 };

struct PrepareOpts {
    bool pre = false;           // the relations arrive pass-1-partitioned: no pass-1 twins
    int big_tables = -1;        // 0 / 1: 16 K-slot tables off / on, whatever the fan-out's choice (-1) would be
    size_t plan_inner = 0;      // > 0: the fan-out is planned for a build side of that many rows while the workspace holds `inner` (device-planned
                                // groups: the mean group decides the partitions, the largest group the plan allows decides the buffers)
    bool claim_s = false;       // the probe side may be partitioned without its histogram pass (a blocking whole join, see
                                // claimed_probe_allowed); the plan says in PhjPlan::claim_s whether it is
};
int phj_prepare(hjgpu_ctx *ctx, size_t inner, size_t outer, const hjgpu_phj_params *prm, uint32_t chunks, PhjPlan *pl, const PrepareOpts &o = {});
// One group of a device-planned grouped join: desc = {build first row, build rows, probe first row, probe rows} in device memory; the
// columns handed to phj_enqueue are the pass-0 twins, their rows the CAPACITY the plan was prepared for.  The join's state
// (aggregates, block counter, open output blocks) is the whole grouped join's: phj_enqueue neither clears it nor closes the gaps.
struct GroupRun { const u64 *desc; };
struct EnqueueOpts {
    PhjStages stages = PHJ_WHOLE;
    const hjgpu_output *out = nullptr;      // result rows (NULL: aggregates only)
    hipEvent_t inner_ready = nullptr;       // the build columns are complete once this event has happened
    const PrePieces *pre = nullptr;         // the relations arrive pass-1-partitioned (a plan with PrepareOpts::pre)
    const GroupRun *grp = nullptr;
};
int phj_enqueue(hjgpu_ctx *ctx, const PhjPlan &pl, const Rel &R, const Rel &S, hipStream_t stream, const EnqueueOpts &o = {});
int finish_blocking(hjgpu_ctx *ctx, hjgpu_result *result, const hjgpu_output *out, hipStream_t stream);
bool npj_unique(const hjgpu_ctx *ctx, const hjgpu_npj_params *prm);
uint32_t npj_mode(const hjgpu_npj_params *prm);
int npj_prepare(hjgpu_ctx *ctx, size_t inner, const hjgpu_npj_params *prm, size_t *buckets, uint32_t *factor);
// a built NPJ table: its buckets, the hash factor, and which hash placed the tuples (line_hash: whole joins' 64-byte lines of 8 buckets;
// else the reference's, hjgpu_npj_build)
struct NpjTable { const u64 *slots; size_t buckets; uint32_t factor; bool line_hash; };
struct NpjProbeOpts {
    bool unique = false;
    uint32_t mode = HJ_MODE_INNER;
    uint32_t *bucket_bits = nullptr;        // right / full outer joins of hjgpu_npj*: the zeroed bucket bitmap; the tail follows the probe
};
int npj_probe_enqueue(hjgpu_ctx *ctx, const Rel &S, const NpjTable &t, const hjgpu_output *out, hipStream_t stream, const NpjProbeOpts &o);
int npj_enqueue(hjgpu_ctx *ctx, const uint32_t *rk, const uint32_t *rv, size_t inner, const uint32_t *sk, const uint32_t *sv, size_t outer,
                size_t buckets, uint32_t factor, const hjgpu_output *out, hipStream_t stream, bool unique, uint32_t mode = HJ_MODE_INNER);
const hjgpu_output *take_async_output(hjgpu_ctx *ctx, const hjgpu_output *given);
// the positional look-up in a built table (hjgpu_npj_lookup*: npj_kernels.hip); ctx->state zeroed by the caller, EV_BEGIN / EV_R_HIST recorded
// select_bits: the mask of a selected look-up (NULL: none, every row is looked up)
int npj_lookup_enqueue(hjgpu_ctx *ctx, const uint32_t *sk, size_t outer, const NpjTable &t, uint32_t *vals_out, uint32_t *match_bits,
                       hipStream_t stream, const uint32_t *select_bits = nullptr);
int check_lookup_columns(hjgpu_ctx *ctx, const uint32_t *sk, size_t outer, const uint32_t *vals_out, const uint32_t *match_bits);
int check_select_bits(hjgpu_ctx *ctx, const uint32_t *select_bits, const uint32_t *match_bits, size_t outer);
// hjgpu_ops.hip: the partition operator on one relation (hjgpu_partition*, hjgpu_partition_packed_*; pass 0 of a grouped plan) - what
// differs between its forms
struct PartitionForm {
    bool packed = false;                    // packed tuples (payload << 32 | key) at keys_out, audited (option "audit"); else the columns keys_out / vals_out
    uint32_t group_bins = 0;                // the partitions in groups of group_bins neighbours, every group on a 128-byte line (hj_group_shift; the
                                            // columns then need room for n + 32 * (groups + 1) rows); the offsets stay the dense prefix of the counts
    uint32_t own_first = 0, own_count = 0;  // partitions [own_first, own_first + own_count) laid out behind all others
    uint32_t factor2 = 0, fanout2 = 0;      // counts2 != NULL: the receivers' second level counted by the same read (bin = p1 * fanout2 + p2)
    uint64_t *counts2 = nullptr;
};
int partition_op(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n, uint32_t factor, uint32_t fanout,
                 uint32_t *keys_out, uint32_t *vals_out, uint64_t *d_offsets, const PartitionForm &form, void *stream_);

}  // namespace hjapi
