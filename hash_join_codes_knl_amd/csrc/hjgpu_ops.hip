// hjgpu_ops.hip - the operator-level entry points of include/hjgpu.h (the reference's operators one by one: histogram /
// partition / build / probe, phj.cpp:693-1231, npj.cpp:190-364), the relations that arrive pass-1-partitioned (the receiving
// side of the multi-GPU CPRA), and the generator / measurement helpers.  Context, planning and whole joins: hjgpu_api.hip.
#include "hjgpu_ctx.hpp"

using namespace hjapi;

namespace hjapi {


// The partition operator on one relation: K4 -> K5 -> K6 pass 1 of the columns into `fanout` partitions, d_offsets = where they begin
int partition_op(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n, uint32_t factor, uint32_t fanout,
                 uint32_t *keys_out, uint32_t *vals_out, uint64_t *d_offsets, const PartitionForm &form, void *stream_)
{
    if (form.counts2 && (form.fanout2 < 1 || !(form.factor2 & 1) || form.factor2 == factor || (u64)fanout * form.fanout2 > HJGPU_MAX_PARTS))
        return fail(ctx, HJGPU_EINVAL, "fused counts: factor2 odd and different from factor, fanout * fanout2 <= 32768");
    if (!ctx || !d_offsets) return fail(ctx, HJGPU_EINVAL, "null pointer");
    if ((u64)form.own_first + form.own_count > fanout) return fail(ctx, HJGPU_EINVAL, "own_first + own_count must not exceed fanout");
    if (fanout == 0 || fanout > HJGPU_MAX_FANOUT || !(factor & 1))
        return fail(ctx, HJGPU_EINVAL, "fanout must be in [1, 1024] and factor odd");
    if (form.packed) {
        if (n && !keys_out) return fail(ctx, HJGPU_EINVAL, "null output array");
        if ((uintptr_t)keys_out & 127) return fail(ctx, HJGPU_EALIGN, "the packed output must be 128-byte aligned (whole-line writes)");
    } else if (n && (!keys_out || !vals_out)) return fail(ctx, HJGPU_EINVAL, "null output column");
    CHK(check_columns(ctx, d_keys, d_vals, n));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    const Pass1Geom geom = make_geom(ctx->tune, d_keys, n, 1, fanout, form.packed);
    MetaLayout sz = carve(nullptr, 1, fanout, fanout, geom.ranges_per_chunk);
    ctx->prepared = false;                 // the workspace is re-planned below
    CHK(ensure(ctx, ctx->meta, sz.total_bytes));
    MetaLayout m = carve(ctx->meta.p, 1, fanout, fanout, geom.ranges_per_chunk);
    // hjgpu_get_stats().ms_total afterwards = duration of the whole operator (histogram + plan + scatter)
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    ctx->last_algo = 2;
    record(ctx, EV_BEGIN, stream);
    u64 *audit = nullptr;                  // option "audit", packed form: stage 0 the columns as read, stage 1 the packed output where it lies
    if (form.packed) CHK(audit_begin(ctx, 3, n, 0, stream, &audit));
    HIPCHK(ctx, hj_zero_async(m.counts[0], m.counts_bytes, stream));
    if (form.counts2) {
        // the same read of the keys also counts the RECEIVERS' second level (bin = p1 * fanout2 + p2, the join's fused
        // histogram): they then need no histogram pass of their own over what arrives (K4p).  The pass-1 counts of this
        // call are the row sums.
        HIPCHK(ctx, hj_zero_async(form.counts2, (size_t)fanout * form.fanout2 * sizeof(u64), stream));
        if (n) {
            u64 *fused = reinterpret_cast<u64 *>(form.counts2);
            CHK(hj_launch_hist2(d_keys, geom, factor, fanout, form.factor2, form.fanout2, fused, m.range_counts[0], m.tickets, ctx->cus, stream,
                                (size_t)ctx->tune.hist_min_lds));
            CHK(hj_launch_row_sums(fused, fanout, form.fanout2, m.counts[0], stream));
        }
    } else if (n) CHK(hj_launch_hist2(d_keys, geom, factor, fanout, 1u, 1u, m.counts[0], m.range_counts[0], m.tickets, ctx->cus, stream));
    // (the column form plans all three parts, mask 7, the packed form only its relation)
    PlanArgs pa = plan_args(ctx, m, 1, fanout, 1, geom.tile, geom.tile, false, form.packed ? 1u : 7u);
    pa.n[0] = n; pa.in_align[0] = align_of(d_keys);
    for (uint32_t c = 1; c < 9; ++c) pa.chunk_beg[0][c] = n;
    CHK(hj_launch_plan(pa, stream));
    if (n) {
        CHK(hj_launch_range_base(m.range_counts[0], m.off1[0], m.range_base[0], 1, geom.ranges_per_chunk, fanout, stream,
                                 form.own_first, form.own_count, form.group_bins));
        CHK(hj_launch_scatter(scatter_pass1(ctx, m, 0, geom, fanout, factor, d_keys, d_vals, keys_out, vals_out), ctx->tune, scatter_cus(ctx),
                              stream));
    }
    HIPCHK(ctx, hj_copy_async(d_offsets, m.off2[0], ((size_t)fanout + 1) * sizeof(u64), stream));
    if (audit && n) {
        CHK(hj_audit_sums_columns(d_keys, d_vals, n, audit, ctx->cus, stream));
        CHK(ensure(ctx, ctx->audit_lay, (size_t)2 * (HJGPU_MAX_FANOUT + 1) * sizeof(u64)));
        u64 *beg = reinterpret_cast<u64 *>(ctx->audit_lay.p), *end = beg + HJGPU_MAX_FANOUT + 1;
        CHK(hj_audit_own_last(m.off2[0], fanout, form.own_first, form.own_count, n, beg, end, stream));
        const HjAuditHash h = {factor, fanout, 0u, 1u, 1u, fanout};
        CHK(audit_partitions(ctx, 1, reinterpret_cast<const u64 *>(keys_out), beg, end, fanout, h, audit, stream));
    }
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

}  // namespace hjapi

extern "C" {

// ---- partition operators ------------------------------------------------------
int hjgpu_histogram(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n, uint32_t factor,
                    uint32_t fanout, uint64_t *d_counts, void *stream_)
{
    if (!ctx || !d_counts || (n && !d_keys)) return fail(ctx, HJGPU_EINVAL, "null pointer");
    if (fanout == 0 || fanout > HJGPU_MAX_PARTS || !(factor & 1))
        return fail(ctx, HJGPU_EINVAL, "fanout must be in [1, 32768] and factor odd");
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hj_zero_async(d_counts, (size_t)fanout * sizeof(u64), stream));
    if (n) {
        // the per-range counts are a by-product here; they go to scratch
        const Pass1Geom g = make_geom(ctx->tune, d_keys, n, 1, 1, false);
        CHK(ensure(ctx, ctx->moves, ((size_t)g.ranges_per_chunk + 16) * sizeof(uint32_t)));
        uint32_t *ticket = (uint32_t *)ctx->moves.p + g.ranges_per_chunk;
        HIPCHK(ctx, hj_zero_async(ticket, 8 * sizeof(uint32_t), stream));
        CHK(hj_launch_hist2(d_keys, g, 1u, 1u, factor, fanout, (u64 *)d_counts,
                            (uint32_t *)ctx->moves.p, ticket, ctx->cus, stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(stream));
    return HJGPU_OK;
}

int hjgpu_partition_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                          uint32_t factor, uint32_t fanout, uint32_t *d_keys_out, uint32_t *d_vals_out,
                          uint64_t *d_offsets, void *stream_)
{
    return partition_op(ctx, d_keys, d_vals, n, factor, fanout, d_keys_out, d_vals_out, d_offsets, PartitionForm{}, stream_);
}

int hjgpu_partition(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                    uint32_t factor, uint32_t fanout, uint32_t *d_keys_out, uint32_t *d_vals_out,
                    uint64_t *d_offsets, void *stream_)
{
    CHK(hjgpu_partition_async(ctx, d_keys, d_vals, n, factor, fanout, d_keys_out, d_vals_out, d_offsets, stream_));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream_));
    return HJGPU_OK;
}

int hjgpu_join_partitions(hjgpu_ctx *ctx,
                          const uint32_t *rk, const uint32_t *rv, const uint64_t *roff,
                          const uint32_t *sk, const uint32_t *sv, const uint64_t *soff,
                          const hjgpu_phj_params *passes, hjgpu_result *result,
                          const hjgpu_output *out, void *stream_)
{
    if (!ctx || !passes || !roff || !soff || !rk || !rv || !sk || !sv)
        return fail(ctx, HJGPU_EINVAL, "null pointer");
    CHK(refuse_join_mode(ctx, passes->flags, "hjgpu_join_partitions"));
    if (((uintptr_t)sk & 15) || ((uintptr_t)sv & 15))
        return fail(ctx, HJGPU_EALIGN, "probe columns must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PhjPlan pl;
    pl.C = 1;
    pl.F1 = passes->fanout1; pl.F2 = passes->fanout2 ? passes->fanout2 : 1;
    pl.P = pl.F1 * pl.F2;
    if (pl.F1 == 0 || pl.P < 2 || pl.P > HJGPU_MAX_PARTS) return fail(ctx, HJGPU_EINVAL, "fan-out out of range");
    pl.f1 = passes->factor1 ? passes->factor1 : DEFAULT_F1;
    pl.f2 = passes->factor2 ? passes->factor2 : DEFAULT_F2;
    pl.tf0 = passes->table_factor[0] ? passes->table_factor[0] : DEFAULT_TF0;
    pl.tf1 = passes->table_factor[1] ? passes->table_factor[1] : DEFAULT_TF1;
    if (!(pl.f1 & 1) || !(pl.f2 & 1) || !(pl.tf0 & 1) || !(pl.tf1 & 1))
        return fail(ctx, HJGPU_EINVAL, "hash factors must be odd");
    // the work-item directory is sized from the probe rows, which only the device knows here
    u64 s_ends[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(&s_ends[0], soff, sizeof(u64), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipMemcpyAsync(&s_ends[1], soff + pl.P, sizeof(u64), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    const size_t items_extra = hj_join_items_capacity(pl.P, (size_t)(s_ends[1] - s_ends[0])) - pl.P;
    MetaLayout sz = carve(nullptr, 1, pl.F1, pl.P, 1, items_extra);
    ctx->prepared = false;                 // the workspace is re-planned below
    CHK(ensure(ctx, ctx->meta, sz.total_bytes));
    CHK(ensure(ctx, ctx->state, sizeof(DevState)));
    MetaLayout m = carve(ctx->meta.p, 1, pl.F1, pl.P, 1, items_extra);
    DevState *st = reinterpret_cast<DevState *>(ctx->state.p);
    u64 bs = 0, bl = 0;
    const bool unique = ctx->tune.unique || (passes->flags & HJGPU_FLAG_UNIQUE);
    const uint32_t workers = (uint32_t)hj_join_workers(ctx->tune, ctx->cus, false);
    CHK(setup_output(ctx, out, workers, &bs, &bl));
    record(ctx, EV_BEGIN, stream);
    HIPCHK(ctx, hj_zero_async(st, sizeof(DevState), stream));
    // counts = adjacent differences of the caller's offsets, then the usual plan
    // (re-derives identical offsets and the work-item prefix)
    CHK(hj_launch_offsets_to_counts((const u64 *)roff, m.counts[0], pl.P, stream));
    CHK(hj_launch_offsets_to_counts((const u64 *)soff, m.counts[1], pl.P, stream));
    const uint32_t tile = (uint32_t)hj_scatter_tile(ctx->tune, 2, 1, true);
    PlanArgs pa = plan_args(ctx, m, 1, pl.F1, pl.F2, tile, tile, unique, 7u);
    CHK(hj_launch_plan(pa, stream));
    for (int e : {EV_S_HIST, EV_S_PLAN, EV_S_SC1, EV_S_SC2, EV_WAITED, EV_R_HIST, EV_R_PLAN, EV_R_SC1, EV_R_SC2}) record(ctx, e, stream);
    JoinArgs ja{};
    ja.rk = rk; ja.rv = rv; ja.sk = sk; ja.sv = sv;
    ja.roff = (const u64 *)roff; ja.soff = (const u64 *)soff;    // caller's offsets (may start at non-zero)
    ja.rend = ja.roff + 1; ja.send = ja.soff + 1;
    ja.slice_prefix = m.slice_prefix; ja.slices = m.slices; ja.item_part = m.item_part;
    ja.P = pl.P; ja.chunks = 1;
    ja.f1 = pl.f1; ja.F1 = pl.F1; ja.f2 = pl.f2; ja.F2 = pl.F2; ja.tf0 = pl.tf0; ja.tf1 = pl.tf1;
    ja.s_align = 0; ja.result = &st->result; ja.work_counter = &st->work_counter;
    ja.work_counter2 = &st->work_counter2;       // (multi_fill stays NULL: the caller's partitions were not counted)
    ja.unique = unique ? 1u : 0u;
    join_output(ctx, ja, out, bs, bl, st);
    CHK(hj_launch_join(ja, ctx->tune, ctx->cus, stream));
    record(ctx, EV_JOIN, stream);
    if (bs) CHK(close_gaps(ctx, out, workers, bs, st, stream));
    record(ctx, EV_GAPS, stream);
    ctx->last_algo = 1;
    return finish_blocking(ctx, result, out, stream);
}

// ---- NPJ operators ------------------------------------------------------------
int hjgpu_npj_build(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                    uint64_t *d_table, size_t buckets, uint32_t factor, void *stream_)
{
    if (!ctx || !d_table || (n && (!d_keys || !d_vals))) return fail(ctx, HJGPU_EINVAL, "null pointer");
    if (!(factor & 1) || buckets <= n) return fail(ctx, HJGPU_EINVAL, "factor must be odd and buckets > n");
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->state, sizeof(DevState)));
    DevState *st = reinterpret_cast<DevState *>(ctx->state.p);
    HIPCHK(ctx, hj_zero_async(st, sizeof(DevState), stream));
    HIPCHK(ctx, hj_zero_async(d_table, buckets * sizeof(u64), stream));
    if (n) CHK(hj_launch_npj_build(d_keys, d_vals, n, (u64 *)d_table, buckets, factor, &st->zero_key, ctx->cus, stream));
    return finish_blocking(ctx, nullptr, nullptr, stream);
}

int hjgpu_npj_probe(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                    const uint64_t *d_table, size_t buckets, uint32_t factor,
                    hjgpu_result *result, const hjgpu_output *out, void *stream_)
{
    if (!ctx || !d_table || buckets == 0) return fail(ctx, HJGPU_EINVAL, "null pointer");
    CHK(check_columns(ctx, d_keys, d_vals, n));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->state, sizeof(DevState)));
    HIPCHK(ctx, hj_zero_async(ctx->state.p, sizeof(DevState), stream));
    record(ctx, EV_BEGIN, stream); record(ctx, EV_R_HIST, stream);
    const NpjTable table = {.slots = (const u64 *)d_table, .buckets = buckets, .factor = factor, .line_hash = false};      // hjgpu_npj_build's: the reference's hash
    CHK(npj_probe_enqueue(ctx, {d_keys, d_vals, n}, table, out, stream, {.unique = ctx->tune.unique}));
    ctx->last_algo = 0;
    return finish_blocking(ctx, result, out, stream);
}

int hjgpu_npj_lookup_table(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n, const uint64_t *d_table, size_t buckets, uint32_t factor,
                           uint32_t *d_vals_out, uint32_t *d_match_bits, hjgpu_result *result, void *stream_)
{
    return hjgpu_npj_lookup_table_selected(ctx, d_keys, n, d_table, buckets, factor, nullptr, d_vals_out, d_match_bits, result, stream_);
}

// the look-up in a built table for the rows whose bit is set in d_select_bits (NULL: every row - the plain look-up, its kernels)
int hjgpu_npj_lookup_table_selected(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n, const uint64_t *d_table, size_t buckets, uint32_t factor,
                                    const uint32_t *d_select_bits, uint32_t *d_vals_out, uint32_t *d_match_bits, hjgpu_result *result, void *stream_)
{
    if (!ctx || !d_table || buckets == 0) return fail(ctx, HJGPU_EINVAL, "null pointer");
    if ((uintptr_t)d_table & 7) return fail(ctx, HJGPU_EALIGN, "the table must be 8-byte aligned");
    CHK(check_lookup_columns(ctx, d_keys, n, d_vals_out, d_match_bits));
    CHK(check_select_bits(ctx, d_select_bits, d_match_bits, n));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    CHK(ensure(ctx, ctx->state, sizeof(DevState)));
    HIPCHK(ctx, hj_zero_async(ctx->state.p, sizeof(DevState), stream));
    record(ctx, EV_BEGIN, stream); record(ctx, EV_R_HIST, stream);
    const NpjTable table = {.slots = (const u64 *)d_table, .buckets = buckets, .factor = factor, .line_hash = false};      // hjgpu_npj_build's: the reference's hash
    CHK(npj_lookup_enqueue(ctx, d_keys, n, table, d_vals_out, d_match_bits, stream, d_select_bits));
    return finish_blocking(ctx, result, nullptr, stream);
}

// ---- relations that arrive pass-1-partitioned (the receiving side of the multi-GPU CPRA) --------------------
int hjgpu_partition_packed_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                                 uint32_t factor, uint32_t fanout, uint64_t *d_tuples_out, uint64_t *d_offsets, void *stream)
{
    return partition_op(ctx, d_keys, d_vals, n, factor, fanout, reinterpret_cast<uint32_t *>(d_tuples_out), nullptr, d_offsets,
                        PartitionForm{.packed = true}, stream);
}

int hjgpu_partition_packed_own_last_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                                          uint32_t factor, uint32_t fanout, uint32_t own_first, uint32_t own_count,
                                          uint64_t *d_tuples_out, uint64_t *d_offsets, void *stream)
{
    return partition_op(ctx, d_keys, d_vals, n, factor, fanout, reinterpret_cast<uint32_t *>(d_tuples_out), nullptr, d_offsets,
                        PartitionForm{.packed = true, .own_first = own_first, .own_count = own_count}, stream);
}

int hjgpu_partition_packed_counted_async(hjgpu_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, size_t n,
                                         uint32_t factor, uint32_t fanout, uint32_t own_first, uint32_t own_count,
                                         uint32_t factor2, uint32_t fanout2, uint64_t *d_tuples_out, uint64_t *d_offsets,
                                         uint64_t *d_counts2, void *stream)
{
    if (!d_counts2) return fail(ctx, HJGPU_EINVAL, "null counts array");
    return partition_op(ctx, d_keys, d_vals, n, factor, fanout, reinterpret_cast<uint32_t *>(d_tuples_out), nullptr, d_offsets,
                        PartitionForm{.packed = true, .own_first = own_first, .own_count = own_count, .factor2 = factor2, .fanout2 = fanout2,
                                      .counts2 = d_counts2}, stream);
}

// what hjgpu_phj_build_prepartitioned plans for a build side of `inner` rows in `fanout1` pass-1 partitions
static void prepartitioned_plan(const hjgpu_ctx *ctx, size_t inner, uint32_t k, const hjgpu_phj_params *prm, uint32_t *F2, bool *big)
{
    *big = false;
    double parts = ceil((double)inner / (ctx->tune.join.cap() * 0.85));
    if (parts > HJGPU_MAX_PARTS) { *big = true; parts = ceil((double)inner / (hj_join_config_big().cap() * 0.85)); }
    uint32_t f2 = (prm && prm->fanout2) ? prm->fanout2 : (uint32_t)std::max(2.0, ceil(parts / k));
    if (f2 < 2) f2 = 2;
    if (f2 > HJGPU_MAX_FANOUT) f2 = HJGPU_MAX_FANOUT;
    while ((u64)k * f2 > HJGPU_MAX_PARTS && f2 > 2) --f2;
    *F2 = f2;
}

int hjgpu_prepartitioned_plan(hjgpu_ctx *ctx, size_t inner, uint32_t fanout1, const hjgpu_phj_params *params,
                              uint32_t *fanout2, uint32_t *factor2)
{
    if (!ctx || !fanout1 || !fanout2 || !factor2) return HJGPU_EINVAL;
    if (params) CHK(refuse_join_mode(ctx, params->flags, "hjgpu_prepartitioned_plan"));
    bool big = false;
    prepartitioned_plan(ctx, inner, fanout1, params, fanout2, &big);
    *factor2 = (params && params->factor2) ? params->factor2 : DEFAULT_F2;
    return HJGPU_OK;
}

static int check_layout(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *lay, HjChunks *ch, size_t *rows)
{
    if (!lay) return fail(ctx, HJGPU_EINVAL, "null layout");
    if (lay->chunks < 1 || lay->chunks > 8) return fail(ctx, HJGPU_EINVAL, "a pre-partitioned relation arrives in 1 to 8 pieces");
    if (!(lay->factor1 & 1) || lay->fanout1 == 0 || lay->fanout1_total > HJGPU_MAX_FANOUT ||
        (u64)lay->first_partition + lay->fanout1 > lay->fanout1_total)
        return fail(ctx, HJGPU_EINVAL, "pre-partitioned layout: odd factor1, fanout1 >= 1, first_partition + fanout1 <= fanout1_total <= 1024");
    ch->chunks = lay->chunks;
    for (uint32_t c = 0; c < 9; ++c) {
        ch->b[c] = lay->chunk_offsets[c <= lay->chunks ? c : lay->chunks];
        if (c && ch->b[c] < ch->b[c - 1]) return fail(ctx, HJGPU_EINVAL, "pre-partitioned layout: chunk_offsets must not decrease");
    }
    *rows = (size_t)(ch->b[lay->chunks] - ch->b[0]);
    if (*rows && !d_tuples) return fail(ctx, HJGPU_EINVAL, "null tuple array");
    if ((uintptr_t)d_tuples & 15) return fail(ctx, HJGPU_EALIGN, "packed tuples must be 16-byte aligned");
    return HJGPU_OK;
}

int hjgpu_phj_build_prepartitioned(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *lay,
                                   size_t max_outer, const hjgpu_phj_params *prm, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    if (prm) CHK(refuse_join_mode(ctx, prm->flags, "hjgpu_phj_build_prepartitioned"));
    PrePieces pre;
    size_t inner = 0;
    CHK(check_layout(ctx, d_tuples, lay, &pre.ch[0], &inner));
    pre.tuples[0] = reinterpret_cast<const u64 *>(d_tuples);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    // pass 1 is given (fan-out k = lay->fanout1 on this rank): pass 2 brings the build partitions down to one LDS table.
    // Always a second pass (F2 >= 2): the final partitions are then ONE line-aligned region each, whatever the number of pieces.
    hjgpu_phj_params p2;
    memset(&p2, 0, sizeof(p2));
    if (prm) p2 = *prm;
    const uint32_t k = lay->fanout1;
    bool big = false;
    uint32_t F2 = 0;
    prepartitioned_plan(ctx, inner, k, &p2, &F2, &big);
    p2.fanout1 = k; p2.fanout2 = F2;
    PhjPlan pl;
    CHK(phj_prepare(ctx, inner, max_outer, &p2, lay->chunks, &pl, {.pre = true, .big_tables = big ? 1 : 0}));
    pl.pre_f1 = lay->factor1; pl.pre_F1tot = lay->fanout1_total; pl.pre_base = lay->first_partition;
    if (pl.f2 == pl.pre_f1) return fail(ctx, HJGPU_EINVAL, "factor2 must differ from the exchange-level factor1 (same factor: the second pass would not split)");
    CHK(phj_enqueue(ctx, pl, {.rows = inner}, {}, stream, {.stages = PHJ_BUILD_ONLY, .pre = &pre}));
    memcpy(ctx->prepared_plan, &pl, sizeof(pl));
    ctx->prepared_inner = inner; ctx->prepared_max_outer = max_outer;
    ctx->prepared = true;
    return HJGPU_OK;
}

static int probe_prepartitioned(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *lay, const uint64_t *d_counts,
                                hjgpu_result *d_result, void *stream_);

int hjgpu_phj_probe_prepartitioned_async(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *lay,
                                         hjgpu_result *d_result, void *stream_)
{
    return probe_prepartitioned(ctx, d_tuples, lay, nullptr, d_result, stream_);
}

int hjgpu_phj_probe_prepartitioned_counted_async(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *lay,
                                                 const uint64_t *d_counts, hjgpu_result *d_result, void *stream_)
{
    if (ctx && !d_counts) return fail(ctx, HJGPU_EINVAL, "null counts array");
    return probe_prepartitioned(ctx, d_tuples, lay, d_counts, d_result, stream_);
}

static int probe_prepartitioned(hjgpu_ctx *ctx, const uint64_t *d_tuples, const hjgpu_prepartitioned *lay, const uint64_t *d_counts,
                                hjgpu_result *d_result, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    const hjgpu_output *out = take_async_output(ctx, nullptr);   // consumed by this call even if it fails below (see hjgpu_npj_async)
    if (!ctx->prepared) return fail(ctx, HJGPU_EINVAL, "hjgpu_phj_probe_prepartitioned_async: no prepared build side, or another entry point has used the workspace since");
    PhjPlan pl;
    memcpy(&pl, ctx->prepared_plan, sizeof(pl));
    if (!pl.pre) return fail(ctx, HJGPU_EINVAL, "the prepared build side was not pre-partitioned (hjgpu_phj_build_prepartitioned)");
    PrePieces pre;
    size_t outer = 0;
    CHK(check_layout(ctx, d_tuples, lay, &pre.ch[1], &outer));
    if (lay->chunks != pl.C || lay->factor1 != pl.pre_f1 || lay->fanout1_total != pl.pre_F1tot ||
        lay->first_partition != pl.pre_base || lay->fanout1 != pl.F1)
        return fail(ctx, HJGPU_EINVAL, "the probe batch's layout differs from the prepared build side's (pieces, factor1, fan-outs, first partition)");
    if (outer > ctx->prepared_max_outer) return fail(ctx, HJGPU_EINVAL, "batch larger than the max_outer given to hjgpu_phj_build_prepartitioned");
    pre.tuples[1] = reinterpret_cast<const u64 *>(d_tuples);
    pre.counts[1] = reinterpret_cast<const u64 *>(d_counts);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->last_had_output = out && out->d_keys;
    CHK(phj_enqueue(ctx, pl, {.rows = ctx->prepared_inner}, {.rows = outer}, stream, {.stages = PHJ_PROBE_ONLY, .out = out, .pre = &pre}));
    if (d_result)
        HIPCHK(ctx, hj_copy_async(d_result, ctx->state.p, sizeof(hjgpu_result), stream));
    return HJGPU_OK;
}

// ---- generator ------------------------------------------------------------------
int hjgpu_generate_range(hjgpu_ctx *ctx, uint64_t seed, size_t inner_total, size_t outer_total,
                         size_t inner_begin, size_t inner_count, size_t outer_begin, size_t outer_count,
                         uint32_t inner_factor, uint32_t outer_factor,
                         uint32_t *ik, uint32_t *iv, uint32_t *ok, uint32_t *ov, void *stream_)
{
    return hjgpu_generate_zipf(ctx, seed, inner_total, outer_total, inner_begin, inner_count, outer_begin,
                               outer_count, inner_factor, outer_factor, 0.0, ik, iv, ok, ov, stream_);
}

int hjgpu_generate_zipf(hjgpu_ctx *ctx, uint64_t seed, size_t inner_total, size_t outer_total,
                        size_t inner_begin, size_t inner_count, size_t outer_begin, size_t outer_count,
                        uint32_t inner_factor, uint32_t outer_factor, double zipf,
                        uint32_t *ik, uint32_t *iv, uint32_t *ok, uint32_t *ov, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    if (!(zipf >= 0.0) || zipf > 8.0) return fail(ctx, HJGPU_EINVAL, "zipf exponent must be in [0, 8]");
    if ((ik && !iv) || (ok && !ov)) return fail(ctx, HJGPU_EINVAL, "key column without payload column");
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = hj_launch_generate(seed, inner_total, inner_begin, inner_count, outer_total, outer_begin,
                                outer_count, inner_factor, outer_factor, ik, iv, ok, ov, stream, zipf);
    if (rc != HJGPU_OK) return fail(ctx, rc, "generate: bad sizes or launch failure");
    HIPCHK(ctx, hipStreamSynchronize(stream));
    return HJGPU_OK;
}

int hjgpu_generate_select(hjgpu_ctx *ctx, uint64_t seed, size_t inner_total, size_t outer_total,
                          size_t inner_begin, size_t inner_count, size_t outer_begin, size_t outer_count,
                          uint32_t inner_factor, uint32_t outer_factor, double zipf, double selectivity,
                          uint32_t *ik, uint32_t *iv, uint32_t *ok, uint32_t *ov, hjgpu_result *expected, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    if (!(zipf >= 0.0) || zipf > 8.0) return fail(ctx, HJGPU_EINVAL, "zipf exponent must be in [0, 8]");
    if (!(selectivity >= 0.0) || selectivity > 1.0) return fail(ctx, HJGPU_EINVAL, "selectivity must be in [0, 1]");
    if ((ik && !iv) || (ok && !ov)) return fail(ctx, HJGPU_EINVAL, "key column without payload column");
    if (expected && outer_total < inner_total)
        return fail(ctx, HJGPU_EINVAL, "analytic aggregates need unique build keys (outer_total >= inner_total)");
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    u64 *d_expect = nullptr;
    if (expected) {
        memset(expected, 0, sizeof(*expected));
        CHK(ensure(ctx, ctx->moves, 64));
        d_expect = (u64 *)ctx->moves.p;
        HIPCHK(ctx, hj_zero_async(d_expect, 4 * sizeof(u64), stream));
    }
    int rc = hj_launch_generate(seed, inner_total, inner_begin, inner_count, outer_total, outer_begin,
                                outer_count, inner_factor, outer_factor, ik, iv, ok, ov, stream, zipf, selectivity,
                                ok ? d_expect : nullptr);
    if (rc != HJGPU_OK) return fail(ctx, rc, "generate: bad sizes or launch failure");
    if (expected) HIPCHK(ctx, hipMemcpyAsync(expected, d_expect, sizeof(*expected), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    return HJGPU_OK;
}

int hjgpu_generate(hjgpu_ctx *ctx, uint64_t seed, size_t inner, size_t outer_total,
                   size_t outer_begin, size_t outer_count, uint32_t inner_factor, uint32_t outer_factor,
                   uint32_t *ik, uint32_t *iv, uint32_t *ok, uint32_t *ov, void *stream_)
{
    return hjgpu_generate_range(ctx, seed, inner, outer_total, 0, inner, outer_begin, outer_count,
                                inner_factor, outer_factor, ik, iv, ok, ov, stream_);
}

int hjgpu_column_sums(hjgpu_ctx *ctx, const uint32_t *d_keys, size_t n, uint32_t fa, uint32_t fb,
                      uint64_t sums[3], void *stream_)
{
    if (!ctx || !sums || (n && !d_keys)) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->moves, 64));
    u64 *d = (u64 *)ctx->moves.p;
    // hjgpu_get_stats().ms_total afterwards = duration of this one streaming read
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    ctx->last_algo = 2;
    record(ctx, EV_BEGIN, stream);
    CHK(hj_launch_column_sums(d_keys, n, fa, fb, d, stream));
    record(ctx, EV_GAPS, stream);
    HIPCHK(ctx, hipMemcpyAsync(sums, d, 3 * sizeof(u64), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    return HJGPU_OK;
}

// ---- compaction by bitmap ---------------------------------------------------------
// hjgpu_compact_selected / _async (DESIGN.md section 5 "Compaction by bitmap").  Every refusal is decided here, from the arguments alone, before
// anything is allocated or enqueued.
static bool ranges_overlap(const void *p, size_t pbytes, const void *q, size_t qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pbytes && qbytes && a < b + qbytes && b < a + pbytes;
}

static int check_compact(hjgpu_ctx *ctx, const uint32_t *bits, size_t n, uint32_t ncols, const uint32_t *const *in, uint32_t *const *out,
                         const uint32_t *rows_out, size_t capacity, const uint64_t *count, bool device_count)
{
    if (!count) return fail(ctx, HJGPU_EINVAL, "null count pointer");
    if (device_count && ((uintptr_t)count & 7)) return fail(ctx, HJGPU_EALIGN, "d_count must be 8-byte aligned");
    if (ncols > HJGPU_COMPACT_MAX_COLS) return fail(ctx, HJGPU_EINVAL, "ncols must not exceed HJGPU_COMPACT_MAX_COLS (8)");
    if (n == 0) return HJGPU_OK;                         // nothing is read, nothing but the count is written: anything else may be NULL
    if (!bits) return fail(ctx, HJGPU_EINVAL, "null d_select_bits (a compaction of every row is a copy)");
    if ((uintptr_t)bits & 15) return fail(ctx, HJGPU_EALIGN, "d_select_bits must be 16-byte aligned");
    if (ncols && (!in || !out)) return fail(ctx, HJGPU_EINVAL, "null column array");
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!in[c] || !out[c]) return fail(ctx, HJGPU_EINVAL, "null column pointer");
        if (((uintptr_t)in[c] & 15) || ((uintptr_t)out[c] & 15)) return fail(ctx, HJGPU_EALIGN, "input and output columns must be 16-byte aligned");
    }
    if ((uintptr_t)rows_out & 15) return fail(ctx, HJGPU_EALIGN, "d_rows_out must be 16-byte aligned");
    if (rows_out && n > 0xFFFFFFFFull) return fail(ctx, HJGPU_EINVAL, "d_rows_out holds 32-bit row numbers: n must not exceed 0xFFFFFFFF");
    // not in place: no output may share a byte with the mask, an input column or another output
    const void *outs[HJGPU_COMPACT_MAX_COLS + 1];
    uint32_t nouts = 0;
    for (uint32_t c = 0; c < ncols; ++c) outs[nouts++] = out[c];
    if (rows_out) outs[nouts++] = rows_out;
    const size_t obytes = capacity * sizeof(uint32_t), mbytes = (n + 31) / 32 * sizeof(uint32_t);
    for (uint32_t o = 0; o < nouts; ++o) {
        if (ranges_overlap(outs[o], obytes, bits, mbytes)) return fail(ctx, HJGPU_EINVAL, "an output overlaps d_select_bits (the compaction is not in place)");
        for (uint32_t c = 0; c < ncols; ++c)
            if (ranges_overlap(outs[o], obytes, in[c], n * sizeof(uint32_t)))
                return fail(ctx, HJGPU_EINVAL, "an output overlaps an input column (the compaction is not in place)");
        for (uint32_t q = 0; q < o; ++q)
            if (ranges_overlap(outs[o], obytes, outs[q], obytes)) return fail(ctx, HJGPU_EINVAL, "an output overlaps another output");
    }
    return HJGPU_OK;
}

// the two launches (three beyond HJ_COMPACT_LAUNCH_COLS columns) behind the checks; d_count in device memory
static int compact_enqueue(hjgpu_ctx *ctx, const uint32_t *bits, size_t n, uint32_t ncols, const uint32_t *const *in, uint32_t *const *out,
                           uint32_t *rows_out, size_t capacity, u64 *counts, u64 *d_count, hipStream_t stream)
{
    const hj_compact::Layout lay = hj_compact::layout(n, hj_compact::ranges_of(ctx->cus));
    if (n == 0) { ncols = 0; rows_out = nullptr; }
    // hjgpu_get_stats afterwards: ms_histogram = the counting launch, ms_join = the compaction, ms_total = both
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    ctx->last_algo = 3;
    record(ctx, EV_BEGIN, stream);
    CHK(hj_launch_compact_count(bits, lay, counts, stream));
    record(ctx, EV_S_HIST, stream);
    if (ncols == 0 && !rows_out) CHK(hj_launch_compact_total(counts, lay.ranges, d_count, stream));
    for (uint32_t c0 = 0; c0 < ncols || (c0 == 0 && rows_out); c0 += HJ_COMPACT_LAUNCH_COLS) {
        CompactArgs a{};
        a.select_bits = bits; a.lay = lay; a.counts = counts; a.capacity = capacity;
        a.d_count = c0 == 0 ? d_count : nullptr;
        a.rows_out = c0 == 0 ? rows_out : nullptr;
        const uint32_t k = std::min<uint32_t>(ncols - c0, HJ_COMPACT_LAUNCH_COLS);
        for (uint32_t c = 0; c < k; ++c) { a.in[c] = in[c0 + c]; a.out[c] = out[c0 + c]; }
        CHK(hj_launch_compact(a, k, stream));
    }
    record(ctx, EV_JOIN, stream);
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// the context's constant-size workspace of the compaction: the ranges' counts, and the blocking form's count behind them
static int compact_workspace(hjgpu_ctx *ctx, u64 **counts)
{
    CHK(ensure(ctx, ctx->compact, ((size_t)hj_compact::MAX_RANGES + 1) * sizeof(u64)));
    *counts = reinterpret_cast<u64 *>(ctx->compact.p);
    return HJGPU_OK;
}

int hjgpu_compact_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t ncols, const uint32_t *const *d_cols_in,
                                 uint32_t *const *d_cols_out, uint32_t *d_rows_out, size_t capacity, uint64_t *d_count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    CHK(check_compact(ctx, d_select_bits, n, ncols, d_cols_in, d_cols_out, d_rows_out, capacity, d_count, true));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    u64 *counts = nullptr;
    CHK(compact_workspace(ctx, &counts));
    return compact_enqueue(ctx, d_select_bits, n, ncols, d_cols_in, d_cols_out, d_rows_out, capacity, counts, reinterpret_cast<u64 *>(d_count), stream);
}

int hjgpu_compact_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t ncols, const uint32_t *const *d_cols_in,
                           uint32_t *const *d_cols_out, uint32_t *d_rows_out, size_t capacity, uint64_t *count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    CHK(check_compact(ctx, d_select_bits, n, ncols, d_cols_in, d_cols_out, d_rows_out, capacity, count, false));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    u64 *counts = nullptr;
    CHK(compact_workspace(ctx, &counts));
    u64 *d_count = counts + hj_compact::MAX_RANGES;
    CHK(compact_enqueue(ctx, d_select_bits, n, ncols, d_cols_in, d_cols_out, d_rows_out, capacity, counts, d_count, stream));
    u64 got = 0;
    HIPCHK(ctx, hipMemcpyAsync(&got, d_count, sizeof(got), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    *count = got;
    if (n && (ncols || d_rows_out) && got > capacity)
        return fail(ctx, HJGPU_EOVERFLOW, "hjgpu_compact_selected: more selected rows than capacity (*count holds their number, the first capacity rows of every output are valid)");
    return HJGPU_OK;
}

// ---- grouped aggregation ----------------------------------------------------------
// hjgpu_group_sum / _async (DESIGN.md section 5 "Grouped aggregation").  Every refusal is decided here, from the arguments alone, before
// anything is allocated or enqueued.
struct GroupCall {
    const uint32_t *bits;
    size_t n;
    uint32_t nkeys, nvals;
    const uint32_t *const *keys_in, *const *vals_in;
    uint32_t *const *keys_out;
    uint64_t *counts_out;
    uint64_t *const *sums_out;
    size_t capacity;
};

static int check_group(hjgpu_ctx *ctx, const GroupCall &g, const uint64_t *ngroups, bool device_count)
{
    if (!ngroups) return fail(ctx, HJGPU_EINVAL, "null group count pointer");
    if (device_count && ((uintptr_t)ngroups & 7)) return fail(ctx, HJGPU_EALIGN, "d_ngroups must be 8-byte aligned");
    if (g.nkeys == 0 || g.nkeys > HJGPU_GROUP_MAX_KEYS) return fail(ctx, HJGPU_EINVAL, "nkeys must be 1 to HJGPU_GROUP_MAX_KEYS (2)");
    if (g.nvals > HJGPU_GROUP_MAX_VALS) return fail(ctx, HJGPU_EINVAL, "nvals must not exceed HJGPU_GROUP_MAX_VALS (4)");
    if (hj_group::merge_slots(g.capacity) == 0) return fail(ctx, HJGPU_EINVAL, "capacity must not exceed 2^40 groups");
    if (g.n == 0) return HJGPU_OK;                       // nothing is read, nothing but the count is written: anything else may be NULL
    if ((uintptr_t)g.bits & 15) return fail(ctx, HJGPU_EALIGN, "d_select_bits must be 16-byte aligned");
    if (!g.keys_in || !g.keys_out || (g.nvals && (!g.vals_in || !g.sums_out))) return fail(ctx, HJGPU_EINVAL, "null column array");
    for (uint32_t c = 0; c < g.nkeys; ++c) {
        if (!g.keys_in[c] || !g.keys_out[c]) return fail(ctx, HJGPU_EINVAL, "null key column pointer");
        if (((uintptr_t)g.keys_in[c] | (uintptr_t)g.keys_out[c]) & 15) return fail(ctx, HJGPU_EALIGN, "key columns must be 16-byte aligned");
    }
    for (uint32_t c = 0; c < g.nvals; ++c) {
        if (!g.vals_in[c] || !g.sums_out[c]) return fail(ctx, HJGPU_EINVAL, "null measure column pointer");
        if (((uintptr_t)g.vals_in[c] | (uintptr_t)g.sums_out[c]) & 15) return fail(ctx, HJGPU_EALIGN, "measure and sum columns must be 16-byte aligned");
    }
    if ((uintptr_t)g.counts_out & 15) return fail(ctx, HJGPU_EALIGN, "d_counts_out must be 16-byte aligned");
    // no output may share a byte with the mask, an input column or another output (the device count word is an output)
    struct Range { const void *p; size_t bytes; };
    Range outs[HJGPU_GROUP_MAX_KEYS + HJGPU_GROUP_MAX_VALS + 2], ins[HJGPU_GROUP_MAX_KEYS + HJGPU_GROUP_MAX_VALS + 1];
    uint32_t nouts = 0, nins = 0;
    for (uint32_t c = 0; c < g.nkeys; ++c) { outs[nouts++] = {g.keys_out[c], g.capacity * sizeof(uint32_t)}; ins[nins++] = {g.keys_in[c], g.n * sizeof(uint32_t)}; }
    for (uint32_t c = 0; c < g.nvals; ++c) { outs[nouts++] = {g.sums_out[c], g.capacity * sizeof(uint64_t)}; ins[nins++] = {g.vals_in[c], g.n * sizeof(uint32_t)}; }
    if (g.counts_out) outs[nouts++] = {g.counts_out, g.capacity * sizeof(uint64_t)};
    if (device_count) outs[nouts++] = {ngroups, sizeof(uint64_t)};
    if (g.bits) ins[nins++] = {g.bits, (g.n + 31) / 32 * sizeof(uint32_t)};
    for (uint32_t o = 0; o < nouts; ++o) {
        for (uint32_t i = 0; i < nins; ++i)
            if (ranges_overlap(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes))
                return fail(ctx, HJGPU_EINVAL, i + 1 == nins && g.bits ? "an output overlaps d_select_bits" : "an output overlaps an input column");
        for (uint32_t q = 0; q < o; ++q)
            if (ranges_overlap(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes)) return fail(ctx, HJGPU_EINVAL, "an output overlaps another output");
    }
    return HJGPU_OK;
}

// the three enqueues behind the checks: the clears (the count word; for n > 0 the overflow word and the merge table), the aggregation, the
// emit.  hjgpu_get_stats afterwards: ms_histogram = the clears, ms_join = the aggregation, ms_close_gaps = the emit, ms_total = all of them
static int group_enqueue(hjgpu_ctx *ctx, const GroupCall &g, u64 *d_ngroups, hipStream_t stream)
{
    const u64 slots = hj_group::merge_slots(g.capacity);
    char *ws = reinterpret_cast<char *>(ctx->group.p);
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    ctx->last_algo = 4;
    record(ctx, EV_BEGIN, stream);
    HIPCHK(ctx, hj_zero_async(d_ngroups, sizeof(u64), stream));
    if (g.n) HIPCHK(ctx, hj_zero_async(ws + sizeof(u64), (size_t)(hj_group::workspace_bytes(slots) - sizeof(u64)), stream));
    record(ctx, EV_S_HIST, stream);
    if (g.n) {
        GroupArgs a{};
        a.select_bits = g.bits; a.n = g.n; a.nkeys = g.nkeys; a.nvals = g.nvals;
        for (uint32_t c = 0; c < g.nkeys; ++c) a.keys[c] = g.keys_in[c];
        for (uint32_t c = 0; c < g.nvals; ++c) a.vals[c] = g.vals_in[c];
        a.merge = reinterpret_cast<hj_group::Slot *>(ws + hj_group::WORKSPACE_HEAD);
        a.merge_mask = slots - 1;
        a.overflow = reinterpret_cast<uint32_t *>(ws + sizeof(u64));
        CHK(hj_launch_group_sum(a, ctx->cus, stream));
    }
    record(ctx, EV_JOIN, stream);
    if (g.n) {
        GroupEmitArgs e{};
        e.merge = reinterpret_cast<const hj_group::Slot *>(ws + hj_group::WORKSPACE_HEAD);
        e.slots = slots; e.nkeys = g.nkeys; e.nvals = g.nvals; e.capacity = g.capacity; e.counts_out = reinterpret_cast<u64 *>(g.counts_out);
        for (uint32_t c = 0; c < g.nkeys; ++c) e.keys_out[c] = g.keys_out[c];
        for (uint32_t c = 0; c < g.nvals; ++c) e.sums_out[c] = reinterpret_cast<u64 *>(g.sums_out[c]);
        e.d_ngroups = d_ngroups;
        CHK(hj_launch_group_emit(e, ctx->cus, stream));
    }
    record(ctx, EV_GAPS, stream);
    return HJGPU_OK;
}

// the context's merge table, sized from the capacity: it grows the first time a capacity is seen (hjgpu_stats.ms_reserve)
static int group_workspace(hjgpu_ctx *ctx, size_t capacity)
{
    ReserveClock clock(ctx);
    return ensure(ctx, ctx->group, (size_t)hj_group::workspace_bytes(hj_group::merge_slots(capacity)));
}

int hjgpu_group_sum_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                          uint32_t nvals, const uint32_t *const *d_vals_in, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                          uint64_t *const *d_sums_out, size_t capacity, uint64_t *d_ngroups, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    const GroupCall g{d_select_bits, n, nkeys, nvals, d_keys_in, d_vals_in, d_keys_out, d_counts_out, d_sums_out, capacity};
    CHK(check_group(ctx, g, d_ngroups, true));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    CHK(group_workspace(ctx, capacity));
    return group_enqueue(ctx, g, reinterpret_cast<u64 *>(d_ngroups), stream);
}

int hjgpu_group_sum(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t nkeys, const uint32_t *const *d_keys_in,
                    uint32_t nvals, const uint32_t *const *d_vals_in, uint32_t *const *d_keys_out, uint64_t *d_counts_out,
                    uint64_t *const *d_sums_out, size_t capacity, uint64_t *ngroups, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    const GroupCall g{d_select_bits, n, nkeys, nvals, d_keys_in, d_vals_in, d_keys_out, d_counts_out, d_sums_out, capacity};
    CHK(check_group(ctx, g, ngroups, false));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    CHK(group_workspace(ctx, capacity));
    u64 *d_ngroups = reinterpret_cast<u64 *>(ctx->group.p);           // the workspace's first word
    CHK(group_enqueue(ctx, g, d_ngroups, stream));
    u64 got = 0;
    HIPCHK(ctx, hipMemcpyAsync(&got, d_ngroups, sizeof(got), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    *ngroups = got;
    if (got > capacity)
        return fail(ctx, HJGPU_EOVERFLOW, "hjgpu_group_sum: more groups than capacity (*ngroups holds a lower bound of their number that exceeds capacity; the outputs are unspecified)");
    return HJGPU_OK;
}

// ---- filter -----------------------------------------------------------------------
// hjgpu_filter_selected / _async (DESIGN.md section 5 "Filter").  Every refusal is decided here, from the arguments alone, before anything is
// allocated or enqueued.
struct FilterCall {
    const uint32_t *bits;
    size_t n;
    uint32_t npreds;
    const uint32_t *const *cols;
    const hjgpu_predicate *preds;
    uint32_t *bits_out;
};

static int check_filter(hjgpu_ctx *ctx, const FilterCall &f, const uint64_t *count, bool device_count)
{
    if (device_count && ((uintptr_t)count & 7)) return fail(ctx, HJGPU_EALIGN, "d_count must be 8-byte aligned");
    if (f.npreds == 0 || f.npreds > HJGPU_FILTER_MAX_PREDS) return fail(ctx, HJGPU_EINVAL, "npreds must be 1 to HJGPU_FILTER_MAX_PREDS (4)");
    if (f.n == 0) return HJGPU_OK;                       // nothing is read, nothing but the count is written: anything else may be NULL
    if (!f.bits_out && !count) return fail(ctx, HJGPU_EINVAL, "d_bits_out and the count are both null: nothing to compute");
    if ((uintptr_t)f.bits & 15) return fail(ctx, HJGPU_EALIGN, "d_select_bits must be 16-byte aligned");
    if ((uintptr_t)f.bits_out & 15) return fail(ctx, HJGPU_EALIGN, "d_bits_out must be 16-byte aligned");
    if (!f.cols || !f.preds) return fail(ctx, HJGPU_EINVAL, "null column or predicate array");
    for (uint32_t p = 0; p < f.npreds; ++p) {
        if (!f.cols[p]) return fail(ctx, HJGPU_EINVAL, "null column pointer");
        if ((uintptr_t)f.cols[p] & 15) return fail(ctx, HJGPU_EALIGN, "columns must be 16-byte aligned");
        if (f.preds[p].flags & ~(HJGPU_PRED_NOT | HJGPU_PRED_SIGNED)) return fail(ctx, HJGPU_EINVAL, "unknown predicate flag (HJGPU_PRED_NOT and HJGPU_PRED_SIGNED are defined)");
        if (f.preds[p].reserved) return fail(ctx, HJGPU_EINVAL, "a predicate's reserved word must be 0");
    }
    // in place: d_bits_out may be the very pointer d_select_bits - the kernel reads a word of the mask in the wave that stores it, before
    // it stores it -; two bitmaps that overlap in any other way would be read after they were written
    const size_t mbytes = (f.n + 31) / 32 * sizeof(uint32_t), cbytes = f.n * sizeof(uint32_t);
    if (f.bits && f.bits_out && f.bits != f.bits_out && ranges_overlap(f.bits_out, mbytes, f.bits, mbytes))
        return fail(ctx, HJGPU_EINVAL, "d_bits_out overlaps d_select_bits: it may be the very pointer d_select_bits (in place), any other overlap of the two bitmaps is refused");
    // no output may share a byte with a column or with the other output; the device count word none with the mask either
    for (uint32_t p = 0; p < f.npreds; ++p) {
        if (ranges_overlap(f.bits_out, f.bits_out ? mbytes : 0, f.cols[p], cbytes)) return fail(ctx, HJGPU_EINVAL, "d_bits_out overlaps a column");
        if (device_count && ranges_overlap(count, count ? sizeof(uint64_t) : 0, f.cols[p], cbytes)) return fail(ctx, HJGPU_EINVAL, "d_count overlaps a column");
    }
    if (device_count && count) {
        if (ranges_overlap(count, sizeof(uint64_t), f.bits_out, f.bits_out ? mbytes : 0)) return fail(ctx, HJGPU_EINVAL, "d_count overlaps d_bits_out");
        if (ranges_overlap(count, sizeof(uint64_t), f.bits, f.bits ? mbytes : 0)) return fail(ctx, HJGPU_EINVAL, "d_count overlaps d_select_bits");
    }
    return HJGPU_OK;
}

// the context's count word (the blocking form's; made by the first call of either form)
static int filter_workspace(hjgpu_ctx *ctx, u64 **word)
{
    CHK(ensure(ctx, ctx->filter, sizeof(u64)));
    *word = reinterpret_cast<u64 *>(ctx->filter.p);
    return HJGPU_OK;
}

// the two enqueues behind the checks: the clear of the count word (d_count NULL: none), the kernel (n == 0: none).  hjgpu_get_stats
// afterwards: ms_histogram = the clear, ms_join = the kernel, ms_total = both
static int filter_enqueue(hjgpu_ctx *ctx, const FilterCall &f, u64 *d_count, hipStream_t stream)
{
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    ctx->last_algo = 5;
    record(ctx, EV_BEGIN, stream);
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

int hjgpu_filter_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t npreds, const uint32_t *const *d_cols,
                                const hjgpu_predicate *preds, uint32_t *d_bits_out, uint64_t *d_count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    const FilterCall f{d_select_bits, n, npreds, d_cols, preds, d_bits_out};
    CHK(check_filter(ctx, f, d_count, true));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    u64 *word = nullptr;
    CHK(filter_workspace(ctx, &word));
    return filter_enqueue(ctx, f, reinterpret_cast<u64 *>(d_count), stream);
}

int hjgpu_filter_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, size_t n, uint32_t npreds, const uint32_t *const *d_cols,
                          const hjgpu_predicate *preds, uint32_t *d_bits_out, uint64_t *count, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    const FilterCall f{d_select_bits, n, npreds, d_cols, preds, d_bits_out};
    CHK(check_filter(ctx, f, count, false));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    u64 *word = nullptr;
    CHK(filter_workspace(ctx, &word));
    CHK(filter_enqueue(ctx, f, count ? word : nullptr, stream));
    u64 got = 0;
    if (count) HIPCHK(ctx, hipMemcpyAsync(&got, word, sizeof(got), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    if (count) *count = got;
    return HJGPU_OK;
}

// ---- gather by row number -----------------------------------------------------------
// hjgpu_gather_selected / _async (DESIGN.md section 5 "Gather by row number").  Every refusal is decided here, from the arguments alone, before
// anything is allocated or enqueued.
struct GatherCall {
    const uint32_t *bits;
    const uint32_t *idx;
    size_t n;
    uint32_t ncols;
    const uint32_t *const *src;
    size_t src_rows;
    uint32_t *const *out;
    uint32_t *bits_out;
};

static int check_gather(hjgpu_ctx *ctx, const GatherCall &g, const uint64_t *d_counts)
{
    if ((uintptr_t)d_counts & 15) return fail(ctx, HJGPU_EALIGN, "d_counts must be 16-byte aligned");
    if (g.ncols == 0 || g.ncols > HJGPU_GATHER_MAX_COLS) return fail(ctx, HJGPU_EINVAL, "ncols must be 1 to HJGPU_GATHER_MAX_COLS (4)");
    if (g.src_rows > 0xFFFFFFFFull) return fail(ctx, HJGPU_EINVAL, "src_rows must not exceed 0xFFFFFFFF: an index is a uint32 and HJGPU_NULL_VAL is never a legal one");
    if (g.n == 0) return HJGPU_OK;                       // nothing is read, nothing but the counts is written: anything else may be NULL
    if (!g.idx) return fail(ctx, HJGPU_EINVAL, "null d_idx");
    if ((uintptr_t)g.bits & 15) return fail(ctx, HJGPU_EALIGN, "d_select_bits must be 16-byte aligned");
    if ((uintptr_t)g.idx & 15) return fail(ctx, HJGPU_EALIGN, "d_idx must be 16-byte aligned");
    if ((uintptr_t)g.bits_out & 15) return fail(ctx, HJGPU_EALIGN, "d_bits_out must be 16-byte aligned");
    if (!g.src || !g.out) return fail(ctx, HJGPU_EINVAL, "null column array");
    for (uint32_t c = 0; c < g.ncols; ++c) {
        if (!g.src[c] || !g.out[c]) return fail(ctx, HJGPU_EINVAL, "null column pointer");
        if ((uintptr_t)g.src[c] & 15) return fail(ctx, HJGPU_EALIGN, "source columns must be 16-byte aligned");
        if ((uintptr_t)g.out[c] & 15) return fail(ctx, HJGPU_EALIGN, "output columns must be 16-byte aligned");
    }
    const size_t mbytes = (g.n + 31) / 32 * sizeof(uint32_t), cbytes = g.n * sizeof(uint32_t), sbytes = g.src_rows * sizeof(uint32_t);
    // in place: an output column may be the very pointer d_idx - a lane reads its index vector before it stores the same vector - and, being
    // an output, only one can; d_bits_out may be the very pointer d_select_bits (hj_lookup.hpp's IN-PLACE RULE).  Every other shared byte
    // between an output and anything else would be read after it was written, or written twice
    for (uint32_t c = 0; c < g.ncols; ++c) {
        if (g.out[c] != g.idx && ranges_overlap(g.out[c], cbytes, g.idx, cbytes))
            return fail(ctx, HJGPU_EINVAL, "an output column overlaps d_idx: it may be the very pointer d_idx (in place), any other overlap is refused");
        for (uint32_t q = 0; q < c; ++q)
            if (ranges_overlap(g.out[c], cbytes, g.out[q], cbytes)) return fail(ctx, HJGPU_EINVAL, "an output column overlaps another output column");
        for (uint32_t q = 0; q < g.ncols; ++q)
            if (ranges_overlap(g.out[c], cbytes, g.src[q], sbytes)) return fail(ctx, HJGPU_EINVAL, "an output column overlaps a source column");
        if (ranges_overlap(g.out[c], cbytes, g.bits, g.bits ? mbytes : 0)) return fail(ctx, HJGPU_EINVAL, "an output column overlaps d_select_bits");
    }
    if (g.bits_out) {
        if (g.bits && g.bits != g.bits_out && ranges_overlap(g.bits_out, mbytes, g.bits, mbytes))
            return fail(ctx, HJGPU_EINVAL, "d_bits_out overlaps d_select_bits: it may be the very pointer d_select_bits (in place), any other overlap of the two bitmaps is refused");
        if (ranges_overlap(g.bits_out, mbytes, g.idx, cbytes)) return fail(ctx, HJGPU_EINVAL, "d_bits_out overlaps d_idx");
        for (uint32_t c = 0; c < g.ncols; ++c) {
            if (ranges_overlap(g.bits_out, mbytes, g.out[c], cbytes)) return fail(ctx, HJGPU_EINVAL, "d_bits_out overlaps an output column");
            if (ranges_overlap(g.bits_out, mbytes, g.src[c], sbytes)) return fail(ctx, HJGPU_EINVAL, "d_bits_out overlaps a source column");
        }
    }
    if (d_counts) {
        const size_t wbytes = 2 * sizeof(uint64_t);
        if (ranges_overlap(d_counts, wbytes, g.bits, g.bits ? mbytes : 0)) return fail(ctx, HJGPU_EINVAL, "d_counts overlaps d_select_bits");
        if (ranges_overlap(d_counts, wbytes, g.idx, cbytes)) return fail(ctx, HJGPU_EINVAL, "d_counts overlaps d_idx");
        if (ranges_overlap(d_counts, wbytes, g.bits_out, g.bits_out ? mbytes : 0)) return fail(ctx, HJGPU_EINVAL, "d_counts overlaps d_bits_out");
        for (uint32_t c = 0; c < g.ncols; ++c) {
            if (ranges_overlap(d_counts, wbytes, g.out[c], cbytes)) return fail(ctx, HJGPU_EINVAL, "d_counts overlaps an output column");
            if (ranges_overlap(d_counts, wbytes, g.src[c], sbytes)) return fail(ctx, HJGPU_EINVAL, "d_counts overlaps a source column");
        }
    }
    return HJGPU_OK;
}

// the context's two count words (the blocking form's; made by the first call of either form)
static int gather_workspace(hjgpu_ctx *ctx, u64 **words)
{
    CHK(ensure(ctx, ctx->gather, 2 * sizeof(u64)));
    *words = reinterpret_cast<u64 *>(ctx->gather.p);
    return HJGPU_OK;
}

// the two enqueues behind the checks: the clear of the count words (d_counts NULL: none), the kernel (n == 0: none).  hjgpu_get_stats
// afterwards: ms_histogram = the clear, ms_join = the kernel, ms_total = both
static int gather_enqueue(hjgpu_ctx *ctx, const GatherCall &g, u64 *d_counts, hipStream_t stream)
{
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    ctx->last_algo = 6;
    record(ctx, EV_BEGIN, stream);
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

int hjgpu_gather_selected_async(hjgpu_ctx *ctx, const uint32_t *d_select_bits, const uint32_t *d_idx, size_t n, uint32_t ncols,
                                const uint32_t *const *d_src_cols, size_t src_rows, uint32_t *const *d_cols_out, uint32_t *d_bits_out,
                                uint64_t *d_counts, void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    const GatherCall g{d_select_bits, d_idx, n, ncols, d_src_cols, src_rows, d_cols_out, d_bits_out};
    CHK(check_gather(ctx, g, d_counts));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    u64 *words = nullptr;
    CHK(gather_workspace(ctx, &words));
    return gather_enqueue(ctx, g, reinterpret_cast<u64 *>(d_counts), stream);
}

int hjgpu_gather_selected(hjgpu_ctx *ctx, const uint32_t *d_select_bits, const uint32_t *d_idx, size_t n, uint32_t ncols,
                          const uint32_t *const *d_src_cols, size_t src_rows, uint32_t *const *d_cols_out, uint32_t *d_bits_out,
                          uint64_t counts[2], void *stream_)
{
    if (!ctx) return HJGPU_EINVAL;
    const GatherCall g{d_select_bits, d_idx, n, ncols, d_src_cols, src_rows, d_cols_out, d_bits_out};
    CHK(check_gather(ctx, g, nullptr));
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(refuse_capture(ctx, stream));
    u64 *words = nullptr;
    CHK(gather_workspace(ctx, &words));
    CHK(gather_enqueue(ctx, g, words, stream));          // (the context's words also when counts is NULL: HJGPU_ERANGE is read from them)
    u64 got[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(got, words, sizeof(got), hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    if (counts) { counts[0] = got[0]; counts[1] = got[1]; }
    if (got[1])
        return fail(ctx, HJGPU_ERANGE, "hjgpu_gather_selected: selected rows hold an index that is neither below src_rows nor HJGPU_NULL_VAL (counts[1] holds their number; they were written as NULL rows, every output is complete)");
    return HJGPU_OK;
}

int hjgpu_stream_read_ms(hjgpu_ctx *ctx, const void *d_ptr, size_t bytes, float *ms, void *stream_)
{
    if (!ctx || !d_ptr || !ms) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->moves, 64));
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    record(ctx, EV_BEGIN, stream);
    CHK(hj_launch_stream_read(d_ptr, bytes, ctx->moves.p, ctx->cus, stream));
    record(ctx, EV_GAPS, stream);
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[EV_GAPS]));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev[EV_BEGIN], ctx->ev[EV_GAPS]));
    ctx->last_algo = 2;
    return HJGPU_OK;
}

int hjgpu_random_line_read_ms(hjgpu_ctx *ctx, const void *d_ptr, size_t bytes, size_t reads, float *ms, void *stream_)
{
    if (!ctx || !d_ptr || !ms) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->moves, 64));
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    record(ctx, EV_BEGIN, stream);
    CHK(hj_launch_random_line_read(d_ptr, bytes, reads, ctx->moves.p, ctx->cus, stream));
    record(ctx, EV_GAPS, stream);
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[EV_GAPS]));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev[EV_BEGIN], ctx->ev[EV_GAPS]));
    ctx->last_algo = 2;
    return HJGPU_OK;
}

int hjgpu_random_cas_ms(hjgpu_ctx *ctx, void *d_ptr, size_t bytes, size_t ops, int in_flight, int load_first, float *ms, void *stream_)
{
    if (!ctx || !d_ptr || !ms) return HJGPU_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure(ctx, ctx->moves, 64));
    HIPCHK(ctx, hj_zero_async(d_ptr, bytes, stream));              // every bucket empty: outside the timed span
    for (int i = 0; i < EV_COUNT; ++i) ctx->ev_valid[i] = false;
    record(ctx, EV_BEGIN, stream);
    CHK(hj_launch_random_cas(d_ptr, bytes, ops, in_flight, load_first != 0, ctx->moves.p, ctx->cus, stream));
    record(ctx, EV_GAPS, stream);
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[EV_GAPS]));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev[EV_BEGIN], ctx->ev[EV_GAPS]));
    ctx->last_algo = 2;
    return HJGPU_OK;
}

}  // extern "C"
