// hjgpu_colops.hip - the column operators of include/hjgpu.h over a bitmap's rows: hjgpu_compact_selected, hjgpu_group_sum, hjgpu_group_agg,
// hjgpu_group_by, hjgpu_filter_selected, hjgpu_gather_selected, hjgpu_lookup_wide, hjgpu_order_by and their _async forms.  What they refuse from their arguments alone is
// colop_checks.hpp; their kernels are gen_kernels.hip's.  The blocking and the enqueue-only form of an operator are ONE path (X_call): they
// differ in where the count words lie - the context's, or the caller's in device memory - and in the blocking form's tail.
#include "hjgpu_ctx.hpp"

using namespace hjapi;
using namespace colop;

// what every call does between its checks and its enqueues: nothing is allocated or enqueued for a refused call or on a capturing stream
static int colop_begin(hjgpu_ctx *ctx, const Verdict &checked, hipStream_t stream, DevBuf &workspace, size_t bytes)
{
    CHK(refused(ctx, checked));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    ReserveClock clock(ctx);                             // (hjgpu_stats.ms_reserve: the merge table grows the first time a capacity is seen)
    return ensure(ctx, workspace, bytes);
}

// the blocking forms' tail: k count words come back once the stream is through, to `got` and - if the caller wants them - to `out`
static int read_back(hjgpu_ctx *ctx, const u64 *d_words, uint32_t k, u64 got[2], uint64_t *out, hipStream_t stream)
{
    got[0] = got[1] = 0;
    if (k) HIPCHK(ctx, hipMemcpyAsync(got, d_words, k * sizeof(u64), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    for (uint32_t i = 0; out && i < k; ++i) out[i] = got[i];
    return HJGPU_OK;
}

// ---- compaction by bitmap ---------------------------------------------------------
// the two launches (three beyond HJ_COMPACT_LAUNCH_COLS columns); d_count in device memory.  hjgpu_get_stats afterwards: ms_histogram = the
// counting launch, ms_join = the compaction, ms_total = both
static int compact_enqueue(hjgpu_ctx *ctx, const CompactCall &c, u64 *counts, u64 *d_count, hipStream_t stream)
{
    const hj_compact::Layout lay = hj_compact::layout(c.n, hj_compact::ranges_of(ctx->cus));
    const uint32_t ncols = c.n ? c.ncols : 0;
    uint32_t *rows_out = c.n ? c.rows_out : nullptr;
    begin_span(ctx, ALGO_COMPACT, stream);
    CHK(hj_launch_compact_count(c.bits, lay, counts, stream));
    record(ctx, EV_S_HIST, stream);
    if (ncols == 0 && !rows_out) CHK(hj_launch_compact_total(counts, lay.ranges, d_count, stream));
    for (uint32_t c0 = 0; c0 < ncols || (c0 == 0 && rows_out); c0 += HJ_COMPACT_LAUNCH_COLS) {
        CompactArgs a{};
        a.select_bits = c.bits; a.lay = lay; a.counts = counts; a.capacity = c.capacity;
        a.d_count = c0 == 0 ? d_count : nullptr;
        a.rows_out = c0 == 0 ? rows_out : nullptr;
        const uint32_t k = std::min<uint32_t>(ncols - c0, HJ_COMPACT_LAUNCH_COLS);
        for (uint32_t i = 0; i < k; ++i) { a.in[i] = c.in[c0 + i]; a.out[i] = c.out[c0 + i]; }
        CHK(hj_launch_compact(a, k, stream));
    }
    record(ctx, EV_JOIN, stream);
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// the context's workspace (constant size): the ranges' counts, and the blocking form's count behind them
static int compact_call(hjgpu_ctx *ctx, const CompactCall &c, uint64_t *count, bool device_count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    CHK(colop_begin(ctx, check_compact(c, count, device_count), stream, ctx->compact, ((size_t)hj_compact::MAX_RANGES + 1) * sizeof(u64)));
    u64 *counts = reinterpret_cast<u64 *>(ctx->compact.p);
    u64 *d_count = device_count ? reinterpret_cast<u64 *>(count) : counts + hj_compact::MAX_RANGES;
    CHK(compact_enqueue(ctx, c, counts, d_count, stream));
    if (device_count) return HJGPU_OK;
    u64 got[2];
    CHK(read_back(ctx, d_count, 1, got, count, stream));
    if (c.n && (c.ncols || c.rows_out) && got[0] > c.capacity)
        return fail(ctx, HJGPU_EOVERFLOW, "hjgpu_compact_selected: more selected rows than capacity (*count holds their number, the first capacity rows of every output are valid)");
    return HJGPU_OK;
}

// ---- grouped aggregation: hjgpu_group_sum, hjgpu_group_agg, hjgpu_group_by ----------
// One path for the three entry points.  A road is what it has to know of theirs: the tables (group_layout.hpp's for up to two key columns,
// wide_group_layout.hpp's for three and four) and the two launches over them
template <class Args, class EmitArgs>
struct GroupedRoad {
    Algo algo;
    const char *entry;                                  // the entry point's name in the overflow message
    u64 (*merge_slots)(u64 capacity);
    u64 (*workspace_bytes)(u64 slots);
    int (*aggregate)(const Args &a, int cus, hipStream_t stream);
    int (*emit)(const EmitArgs &e, int cus, hipStream_t stream);
};
static_assert(hj_group::WORKSPACE_HEAD == hj_wide::WORKSPACE_HEAD, "either workspace: the blocking form's count word, the overflow word, the merge table");
static const GroupedRoad<AggArgs, AggEmitArgs> ROAD_SUMS{ALGO_GROUP_SUM, "hjgpu_group_sum", hj_group::merge_slots, hj_group::workspace_bytes, hj_launch_group_sum, hj_launch_group_emit};
// (nkeys 0: the scalar road - every selected row goes to the slot of tuple 0, which the emit turns into J = 0 or 1)
static const GroupedRoad<AggArgs, AggEmitArgs> ROAD_AGGREGATES{ALGO_GROUP_AGG, "hjgpu_group_agg", hj_group::merge_slots, hj_group::workspace_bytes, hj_launch_agg_group, hj_launch_agg_emit};
static const GroupedRoad<WideArgs, WideEmitArgs> ROAD_WIDE{ALGO_GROUP_BY, "hjgpu_group_by", hj_wide::merge_slots, hj_wide::workspace_bytes, hj_launch_wide_group, hj_launch_wide_emit};

// the three enqueues: the clears (the count word; for n > 0 the overflow word and the merge table), the aggregation, the emit.
// hjgpu_get_stats afterwards: ms_histogram = the clears, ms_join = the aggregation, ms_close_gaps = the emit, ms_total = all of them
template <class Args, class EmitArgs>
static int grouped_enqueue(hjgpu_ctx *ctx, const GroupedRoad<Args, EmitArgs> &road, const GroupAggCall &g, u64 *d_ngroups, hipStream_t stream)
{
    const u64 slots = road.merge_slots(g.capacity);
    char *ws = reinterpret_cast<char *>(ctx->group.p);
    begin_span(ctx, road.algo, stream);
    HIPCHK(ctx, hj_zero_async(d_ngroups, sizeof(u64), stream));
    if (g.n) HIPCHK(ctx, hj_zero_async(ws + sizeof(u64), (size_t)(road.workspace_bytes(slots) - sizeof(u64)), stream));
    record(ctx, EV_S_HIST, stream);
    if (g.n) {
        Args a{};
        a.g.select_bits = g.bits; a.g.n = g.n; a.g.nkeys = g.nkeys; a.g.nvals = g.naggs;
        for (uint32_t c = 0; c < g.nkeys; ++c) a.g.keys[c] = g.keys_in[c];
        for (uint32_t c = 0; c < g.naggs; ++c) { a.g.vals[c] = g.aggs[c].d_a; a.b[c] = g.aggs[c].d_b; a.fn[c] = g.aggs[c].fn; a.flags[c] = g.aggs[c].flags; }
        a.g.merge = reinterpret_cast<decltype(a.g.merge)>(ws + hj_group::WORKSPACE_HEAD);
        a.g.merge_mask = slots - 1;
        a.g.overflow = reinterpret_cast<uint32_t *>(ws + sizeof(u64));
        CHK(road.aggregate(a, ctx->cus, stream));
    }
    record(ctx, EV_JOIN, stream);
    if (g.n) {
        EmitArgs e{};
        e.g.merge = reinterpret_cast<decltype(e.g.merge)>(ws + hj_group::WORKSPACE_HEAD);
        e.g.slots = slots; e.g.nkeys = g.nkeys; e.g.nvals = g.naggs; e.g.capacity = g.capacity; e.g.counts_out = reinterpret_cast<u64 *>(g.counts_out);
        for (uint32_t c = 0; c < g.nkeys; ++c) e.g.keys_out[c] = g.keys_out[c];
        for (uint32_t c = 0; c < g.naggs; ++c) { e.g.sums_out[c] = reinterpret_cast<u64 *>(g.aggs_out[c]); e.fn[c] = g.aggs[c].fn; e.flags[c] = g.aggs[c].flags; }
        e.g.d_ngroups = d_ngroups;
        CHK(road.emit(e, ctx->cus, stream));
    }
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// The context's workspace (sized from the capacity by the road's tables): the blocking form's count word first, the overflow word, the
// merge table.  One buffer for every road, grown when needed: one context runs one call at a time, and the clears are ordered by the stream
template <class Args, class EmitArgs>
static int grouped_call(hjgpu_ctx *ctx, const GroupedRoad<Args, EmitArgs> &road, const Verdict &checked, const GroupAggCall &g, uint64_t *ngroups, bool device_count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    CHK(colop_begin(ctx, checked, stream, ctx->group, (size_t)road.workspace_bytes(road.merge_slots(g.capacity))));
    u64 *d_ngroups = reinterpret_cast<u64 *>(device_count ? (void *)ngroups : ctx->group.p);
    CHK(grouped_enqueue(ctx, road, g, d_ngroups, stream));
    if (device_count) return HJGPU_OK;
    u64 got[2];
    CHK(read_back(ctx, d_ngroups, 1, got, ngroups, stream));
    if (got[0] <= g.capacity) return HJGPU_OK;
    char text[256];
    snprintf(text, sizeof(text), "%s: more groups than capacity (*ngroups holds a lower bound of their number that exceeds capacity; the outputs are unspecified)", road.entry);
    return fail(ctx, HJGPU_EOVERFLOW, text);
}

// hjgpu_group_sum: its measures as unsigned sums (the launch takes them for what they are: its kernels read no function)
static int group_call(hjgpu_ctx *ctx, const GroupCall &g, uint64_t *ngroups, bool device_count, void *stream_)
{
    const Verdict checked = check_group(g, ngroups, device_count);
    hjgpu_aggregate sums[HJGPU_GROUP_MAX_VALS] = {};
    if (checked.status == HJGPU_OK && g.n)
        for (uint32_t c = 0; c < g.nvals; ++c) sums[c] = {HJGPU_AGG_SUM, 0, g.vals_in[c], nullptr};
    return grouped_call(ctx, ROAD_SUMS, checked, {g.bits, g.n, g.nkeys, g.nvals, g.keys_in, sums, g.keys_out, g.counts_out, g.sums_out, g.capacity}, ngroups, device_count, stream_);
}

static int group_agg_call(hjgpu_ctx *ctx, const GroupAggCall &g, uint64_t *ngroups, bool device_count, void *stream_)
{
    return grouped_call(ctx, ROAD_AGGREGATES, check_group_agg(g, ngroups, device_count), g, ngroups, device_count, stream_);
}

// The road is chosen by nkeys: up to two key columns are hjgpu_group_agg itself
static int group_by_call(hjgpu_ctx *ctx, const GroupAggCall &g, uint64_t *ngroups, bool device_count, void *stream_)
{
    if (g.nkeys <= HJGPU_GROUP_MAX_KEYS) return group_agg_call(ctx, g, ngroups, device_count, stream_);
    return grouped_call(ctx, ROAD_WIDE, check_group_by(g, ngroups, device_count), g, ngroups, device_count, stream_);
}

// ---- filter -----------------------------------------------------------------------
// the two enqueues: the clear of the count word (d_count NULL: none), the kernel (n == 0: none).  hjgpu_get_stats afterwards: ms_histogram =
// the clear, ms_join = the kernel, ms_total = both
static int filter_enqueue(hjgpu_ctx *ctx, const FilterCall &f, u64 *d_count, hipStream_t stream)
{
    begin_span(ctx, ALGO_FILTER, stream);
    if (d_count) HIPCHK(ctx, hj_zero_async(d_count, sizeof(u64), stream));
    record(ctx, EV_S_HIST, stream);
    if (f.n) {
        FilterArgs a{};
        a.select_bits = f.bits; a.bits_out = f.bits_out; a.count = d_count; a.n = f.n;
        for (uint32_t p = 0; p < f.npreds; ++p) {
            a.cols[p] = f.cols[p];
            a.preds[p] = hj_filter::normalise(f.preds[p].lo, f.preds[p].hi, f.preds[p].flags);
        }
        CHK(hj_launch_filter(a, f.npreds, ctx->cus, stream));
    }
    record(ctx, EV_JOIN, stream);
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// the context's count words (made by the first call of either form, of the filter or of the gather): the blocking form's count is the first
static int filter_call(hjgpu_ctx *ctx, const FilterCall &f, uint64_t *count, bool device_count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    CHK(colop_begin(ctx, check_filter(f, count, device_count), stream, ctx->count_words, 2 * sizeof(u64)));
    u64 *word = reinterpret_cast<u64 *>(ctx->count_words.p);
    if (device_count) return filter_enqueue(ctx, f, reinterpret_cast<u64 *>(count), stream);
    CHK(filter_enqueue(ctx, f, count ? word : nullptr, stream));
    u64 got[2];
    return read_back(ctx, word, count ? 1 : 0, got, count, stream);
}

// ---- gather by row number -----------------------------------------------------------
// the two enqueues: the clear of the count words (d_counts NULL: none), the kernel (n == 0: none).  hjgpu_get_stats afterwards: ms_histogram =
// the clear, ms_join = the kernel, ms_total = both
static int gather_enqueue(hjgpu_ctx *ctx, const GatherCall &g, u64 *d_counts, hipStream_t stream)
{
    begin_span(ctx, ALGO_GATHER, stream);
    if (d_counts) HIPCHK(ctx, hj_zero_async(d_counts, 2 * sizeof(u64), stream));
    record(ctx, EV_S_HIST, stream);
    if (g.n) {
        GatherArgs a{};
        a.select_bits = g.bits; a.idx = g.idx; a.bits_out = g.bits_out; a.counts = d_counts; a.n = g.n; a.src_rows = (uint32_t)g.src_rows;
        for (uint32_t c = 0; c < g.ncols; ++c) { a.src[c] = g.src[c]; a.out[c] = g.out[c]; }
        CHK(hj_launch_gather(a, g.ncols, ctx->cus, stream));
    }
    record(ctx, EV_JOIN, stream);
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// the blocking form counts in the context's words also when counts is NULL: HJGPU_ERANGE is read from them
static int gather_call(hjgpu_ctx *ctx, const GatherCall &g, uint64_t *counts, bool device_count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    CHK(colop_begin(ctx, check_gather(g, device_count ? counts : nullptr), stream, ctx->count_words, 2 * sizeof(u64)));
    u64 *words = reinterpret_cast<u64 *>(ctx->count_words.p);
    CHK(gather_enqueue(ctx, g, device_count ? reinterpret_cast<u64 *>(counts) : words, stream));
    if (device_count) return HJGPU_OK;
    u64 got[2];
    CHK(read_back(ctx, words, 2, got, counts, stream));
    if (got[1])
        return fail(ctx, HJGPU_ERANGE, "hjgpu_gather_selected: selected rows hold an index that is neither below src_rows nor HJGPU_NULL_VAL (counts[1] holds their number; they were written as NULL rows, every output is complete)");
    return HJGPU_OK;
}

// ---- wide look-up: two to four key columns ---------------------------------------------
// the three enqueues: the clear of the aggregate words and the table, the build, the look-up - for an empty build side no table, and
// the two fills that make every row a NULL row in the look-up's place (no key of either side is read); for outer == 0 the clear of the
// aggregate words alone.  hjgpu_get_stats afterwards: ms_histogram = the clear and the build, ms_join = the look-up, ms_total = all of it
// (and, in the device form, the copy of the aggregate words to d_result), buckets = the table's slots
static int lookup_wide_enqueue(hjgpu_ctx *ctx, const LookupWideCall &c, u64 slots, hjgpu_result *d_result, hipStream_t stream)
{
    char *ws = reinterpret_cast<char *>(ctx->wide_lookup.p);
    hjgpu_result *words = reinterpret_cast<hjgpu_result *>(ws);
    void *table = ws + hj_wlk::WORKSPACE_HEAD;
    begin_span(ctx, ALGO_LOOKUP_WIDE, stream);
    ctx->stats.fanout1 = ctx->stats.fanout2 = 0; ctx->stats.buckets = slots; ctx->stats.batches = 0;
    HIPCHK(ctx, hj_zero_async(ws, (size_t)hj_wlk::workspace_bytes(slots, c.nkeys), stream));
    if (slots) {
        WideLookupBuildArgs b{};
        for (uint32_t k = 0; k < c.nkeys; ++k) b.keys[k] = c.inner_keys[k];
        b.vals = c.inner_vals; b.n = c.inner; b.table = table; b.slots = slots;
        CHK(hj_launch_wide_lookup_build(b, c.nkeys, ctx->cus, stream));
    }
    record(ctx, EV_S_HIST, stream);
    if (slots) {
        WideLookupArgs a{};
        a.select_bits = c.select_bits; a.n = c.outer; a.table = table; a.slots = slots; a.result = words;
        for (uint32_t k = 0; k < c.nkeys; ++k) a.keys[k] = c.outer_keys[k];
        a.vals_out = c.vals_out; a.match_bits = c.match_bits;
        CHK(hj_launch_wide_lookup(a, c.nkeys, ctx->cus, stream));
    } else if (c.outer) {
        if (c.vals_out) HIPCHK(ctx, hj_fill_async(c.vals_out, HJGPU_NULL_VAL, c.outer * sizeof(uint32_t), stream));
        if (c.match_bits) HIPCHK(ctx, hj_zero_async(c.match_bits, bitmap_bytes(c.outer), stream));
    }
    record(ctx, EV_JOIN, stream);
    if (d_result) HIPCHK(ctx, hj_copy_async(d_result, words, sizeof(hjgpu_result), stream));
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// the context's workspace (wide_lookup_layout.hpp; sized from the build side and the load): the call's aggregate words, then its table.
// Its own buffer: neither ctx->state nor the NPJ table nor a prepared build side is touched
static int lookup_wide_call(hjgpu_ctx *ctx, const LookupWideCall &c, hjgpu_result *result, bool device_result, void *stream_, const char *entry)
{
    if (!ctx) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    CHK(refused(ctx, check_lookup_wide(c, device_result ? result : nullptr)));
    if (c.params) CHK(refuse_join_mode(ctx, c.params->flags, entry));
    // (outer == 0: nothing is looked up, so nothing is built)
    const u64 slots = c.outer ? hj_wlk::slots_of(c.inner, c.params ? c.params->load : 0.0) : 0;
    CHK(colop_begin(ctx, no_objection(), stream, ctx->wide_lookup, (size_t)hj_wlk::workspace_bytes(slots, c.nkeys)));
    CHK(lookup_wide_enqueue(ctx, c, slots, device_result ? result : nullptr, stream));
    if (device_result) return HJGPU_OK;
    hjgpu_result got;
    HIPCHK(ctx, hipMemcpyAsync(&got, ctx->wide_lookup.p, sizeof(got), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    if (result) *result = got;
    return HJGPU_OK;
}

// ---- order by ----------------------------------------------------------------------------------
// The road is chosen by n alone (order_layout.hpp).  The LDS road is one launch.  The device road: the initial permutation - the
// compaction's row numbers, or an iota under a NULL mask - and the clear of the passes' digit totals; three launches per pass between the
// workspace's two permutation buffers; the gather.  J stays in *d_count, where every kernel reads it.  hjgpu_get_stats afterwards:
// ms_histogram = the initial permutation, ms_join = the passes (the LDS road's one launch), ms_close_gaps = the gather, ms_total = all of it
static int order_enqueue(hjgpu_ctx *ctx, const OrderCall &o, u64 *d_count, hipStream_t stream)
{
    using namespace hj_order;
    char *ws = reinterpret_cast<char *>(ctx->order.p);
    const bool outputs = o.ncols || o.rows_out;
    uint32_t key_flags[MAX_KEYS] = {};
    for (uint32_t k = 0; o.n && k < o.nkeys; ++k) key_flags[k] = o.keys[k].flags;
    begin_span(ctx, ALGO_ORDER_BY, stream);
    if (o.n == 0) HIPCHK(ctx, hj_zero_async(d_count, sizeof(u64), stream));
    else if (lds_road(o.n)) {
        record(ctx, EV_S_HIST, stream);
        OrderLdsArgs a{};
        a.select_bits = o.bits; a.n = (uint32_t)o.n; a.nkeys = o.nkeys; a.ncols = o.ncols;
        for (uint32_t k = 0; k < o.nkeys; ++k) { a.keys[k] = o.keys[k].d_col; a.key_flags[k] = key_flags[k]; }
        for (uint32_t c = 0; c < o.ncols; ++c) { a.in[c] = o.cols[c].d_in; a.out[c] = o.cols[c].d_out; a.wide_cols |= (o.cols[c].flags & HJGPU_ORDER_WIDE ? 1u : 0u) << c; }
        a.rows_out = o.rows_out; a.limit = o.limit; a.d_count = d_count;
        CHK(hj_launch_order_lds(a, stream));
        record(ctx, EV_JOIN, stream);
        record(ctx, EV_GAPS, stream);
        return HJGPU_OK;
    } else {
        uint32_t *perm[2] = {reinterpret_cast<uint32_t *>(ws + WORKSPACE_HEAD), reinterpret_cast<uint32_t *>(ws + WORKSPACE_HEAD + perm_bytes(o.n))};
        u64 *compact_counts = reinterpret_cast<u64 *>(ws + COMPACT_COUNTS_AT);
        uint32_t *totals = reinterpret_cast<uint32_t *>(ws + TOTALS_AT);
        // (the count alone: no permutation is made, let alone sorted)
        if (o.bits) {
            static_assert(COMPACT_COUNTS_BYTES == hj_compact::MAX_RANGES * sizeof(u64), "the compaction's counts");
            CompactArgs c{};
            c.select_bits = o.bits; c.lay = hj_compact::layout(o.n, hj_compact::ranges_of(ctx->cus)); c.counts = compact_counts;
            c.d_count = d_count; c.capacity = o.n; c.rows_out = perm[0];
            CHK(hj_launch_compact_count(o.bits, c.lay, compact_counts, stream));
            if (outputs) CHK(hj_launch_compact(c, 0, stream));
            else CHK(hj_launch_compact_total(compact_counts, c.lay.ranges, d_count, stream));
        } else CHK(hj_launch_order_iota(perm[0], outputs ? o.n : 0, o.n, d_count, ctx->cus, stream));
        record(ctx, EV_S_HIST, stream);
        const uint32_t passes = outputs ? passes_of(o.nkeys, key_flags) : 0;
        if (passes) HIPCHK(ctx, hj_zero_async(totals, TOTALS_BYTES, stream));
        for (uint32_t p = 0; p < passes; ++p) {
            OrderPassArgs a{};
            a.pass = pass_of(o.nkeys, key_flags, p);
            a.perm_in = perm[p & 1]; a.perm_out = perm[(p & 1) ^ 1];
            a.key_words = reinterpret_cast<const uint32_t *>(o.keys[a.pass.key].d_col);
            a.lay = layout(o.n, ranges_of(ctx->cus));
            a.d_count = d_count;
            a.counts = reinterpret_cast<uint32_t *>(ws + COUNTS_AT); a.bases = reinterpret_cast<uint32_t *>(ws + BASES_AT);
            a.totals = totals + (size_t)p * DIGITS;
            CHK(hj_launch_order_histogram(a, stream));
            CHK(hj_launch_order_scan(a, stream));
            CHK(hj_launch_order_scatter(a, stream));
        }
        record(ctx, EV_JOIN, stream);
        if (outputs) {
            OrderGatherArgs g{};
            g.perm = perm[passes & 1]; g.d_count = d_count; g.limit = o.limit; g.ncols = o.ncols; g.rows_out = o.rows_out;
            for (uint32_t c = 0; c < o.ncols; ++c) { g.in[c] = o.cols[c].d_in; g.out[c] = o.cols[c].d_out; g.wide_cols |= (o.cols[c].flags & HJGPU_ORDER_WIDE ? 1u : 0u) << c; }
            CHK(hj_launch_order_gather(g, o.n, ctx->cus, stream));
        }
        record(ctx, EV_GAPS, stream);
        return HJGPU_OK;
    }
    record(ctx, EV_S_HIST, stream);
    record(ctx, EV_JOIN, stream);
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// the context's workspace (order_layout.hpp; sized from n alone): the blocking form's count word first
static int order_call(hjgpu_ctx *ctx, const OrderCall &o, uint64_t *count, bool device_count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    const Verdict checked = check_order_by(o, count, device_count);
    CHK(colop_begin(ctx, checked, stream, ctx->order, (size_t)hj_order::workspace_bytes(checked.status == HJGPU_OK ? o.n : 0)));
    u64 *d_count = reinterpret_cast<u64 *>(device_count ? (void *)count : ctx->order.p);
    CHK(order_enqueue(ctx, o, d_count, stream));
    if (device_count) return HJGPU_OK;
    u64 got[2];
    return read_back(ctx, d_count, 1, got, count, stream);
}

extern "C" {

int hjgpu_order_by_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const hjgpu_order_key *keys, uint32_t ncols,
                         const hjgpu_order_column *cols, uint32_t *d_rows_out, size_t limit, uint64_t *d_count, void *stream)
{
    return order_call(ctx, {d_select_bits, n, nkeys, keys, ncols, cols, d_rows_out, limit}, d_count, true, stream);
}

int hjgpu_order_by(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const hjgpu_order_key *keys, uint32_t ncols,
                   const hjgpu_order_column *cols, uint32_t *d_rows_out, size_t limit, uint64_t *count, void *stream)
{
    return order_call(ctx, {d_select_bits, n, nkeys, keys, ncols, cols, d_rows_out, limit}, count, false, stream);
}

int hjgpu_lookup_wide_async(hjgpu_ctx *ctx, uint32_t nkeys, const uint32_t *const *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                            const uint32_t *const *d_outer_keys, size_t outer, const hjgpu_npj_params *params, const uint32_t *d_select_bits,
                            uint32_t *d_vals_out, uint32_t *d_match_bits, hjgpu_result *d_result, void *stream)
{
    return lookup_wide_call(ctx, {nkeys, d_inner_keys, d_inner_vals, inner, d_outer_keys, outer, params, d_select_bits, d_vals_out, d_match_bits},
                            d_result, true, stream, "hjgpu_lookup_wide_async");
}

int hjgpu_lookup_wide(hjgpu_ctx *ctx, uint32_t nkeys, const uint32_t *const *d_inner_keys, const uint32_t *d_inner_vals, size_t inner,
                      const uint32_t *const *d_outer_keys, size_t outer, const hjgpu_npj_params *params, const uint32_t *d_select_bits,
                      uint32_t *d_vals_out, uint32_t *d_match_bits, hjgpu_result *result, void *stream)
{
    return lookup_wide_call(ctx, {nkeys, d_inner_keys, d_inner_vals, inner, d_outer_keys, outer, params, d_select_bits, d_vals_out, d_match_bits},
                            result, false, stream, "hjgpu_lookup_wide");
}

int hjgpu_compact_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t ncols, const uint32_t *const *d_cols_in,
                                 uint32_t *const *d_cols_out, uint32_t *d_rows_out, size_t capacity, uint64_t *d_count, void *stream)
{
    return compact_call(ctx, {d_select_bits, n, ncols, d_cols_in, d_cols_out, d_rows_out, capacity}, d_count, true, stream);
}

int hjgpu_compact_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t ncols, const uint32_t *const *d_cols_in,
                           uint32_t *const *d_cols_out, uint32_t *d_rows_out, size_t capacity, uint64_t *count, void *stream)
{
    return compact_call(ctx, {d_select_bits, n, ncols, d_cols_in, d_cols_out, d_rows_out, capacity}, count, false, stream);
}

int hjgpu_group_sum_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                          uint32_t nvals, const uint32_t *const *d_vals_in, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                          uint64_t *const *d_sums_out, size_t capacity, uint64_t *d_ngroups, void *stream)
{
    return group_call(ctx, {d_select_bits, n, nkeys, nvals, d_keys_in, d_vals_in, d_keys_out, d_counts_out, d_sums_out, capacity}, d_ngroups, true, stream);
}

int hjgpu_group_sum(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                    uint32_t nvals, const uint32_t *const *d_vals_in, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                    uint64_t *const *d_sums_out, size_t capacity, uint64_t *ngroups, void *stream)
{
    return group_call(ctx, {d_select_bits, n, nkeys, nvals, d_keys_in, d_vals_in, d_keys_out, d_counts_out, d_sums_out, capacity}, ngroups, false, stream);
}

int hjgpu_group_agg_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                          uint32_t naggs, const hjgpu_aggregate *aggs, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                          uint64_t *const *d_aggs_out, size_t capacity, uint64_t *d_ngroups, void *stream)
{
    return group_agg_call(ctx, {d_select_bits, n, nkeys, naggs, d_keys_in, aggs, d_keys_out, d_counts_out, d_aggs_out, capacity}, d_ngroups, true, stream);
}

int hjgpu_group_agg(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                    uint32_t naggs, const hjgpu_aggregate *aggs, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                    uint64_t *const *d_aggs_out, size_t capacity, uint64_t *ngroups, void *stream)
{
    return group_agg_call(ctx, {d_select_bits, n, nkeys, naggs, d_keys_in, aggs, d_keys_out, d_counts_out, d_aggs_out, capacity}, ngroups, false, stream);
}

int hjgpu_group_by_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                         uint32_t naggs, const hjgpu_aggregate *aggs, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                         uint64_t *const *d_aggs_out, size_t capacity, uint64_t *d_ngroups, void *stream)
{
    return group_by_call(ctx, {d_select_bits, n, nkeys, naggs, d_keys_in, aggs, d_keys_out, d_counts_out, d_aggs_out, capacity}, d_ngroups, true, stream);
}

int hjgpu_group_by(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                   uint32_t naggs, const hjgpu_aggregate *aggs, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                   uint64_t *const *d_aggs_out, size_t capacity, uint64_t *ngroups, void *stream)
{
    return group_by_call(ctx, {d_select_bits, n, nkeys, naggs, d_keys_in, aggs, d_keys_out, d_counts_out, d_aggs_out, capacity}, ngroups, false, stream);
}

int hjgpu_filter_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t npreds, const uint32_t *const *d_cols,
                                const hjgpu_predicate *preds, uint32_t *d_bits_out, uint64_t *d_count, void *stream)
{
    return filter_call(ctx, {d_select_bits, n, npreds, d_cols, preds, d_bits_out}, d_count, true, stream);
}

int hjgpu_filter_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t npreds, const uint32_t *const *d_cols,
                          const hjgpu_predicate *preds, uint32_t *d_bits_out, uint64_t *count, void *stream)
{
    return filter_call(ctx, {d_select_bits, n, npreds, d_cols, preds, d_bits_out}, count, false, stream);
}

int hjgpu_gather_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, const uint32_t *d_idx, size_t n, uint32_t ncols,
                                const uint32_t *const *d_src_cols, size_t src_rows, uint32_t *const *d_cols_out, uint32_t *d_bits_out,
                                uint64_t *d_counts, void *stream)
{
    return gather_call(ctx, {d_select_bits, d_idx, n, ncols, d_src_cols, src_rows, d_cols_out, d_bits_out}, d_counts, true, stream);
}

int hjgpu_gather_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, const uint32_t *d_idx, size_t n, uint32_t ncols,
                          const uint32_t *const *d_src_cols, size_t src_rows, uint32_t *const *d_cols_out, uint32_t *d_bits_out,
                          uint64_t counts[2], void *stream)
{
    return gather_call(ctx, {d_select_bits, d_idx, n, ncols, d_src_cols, src_rows, d_cols_out, d_bits_out}, counts, false, stream);
}

}  // extern "C"
