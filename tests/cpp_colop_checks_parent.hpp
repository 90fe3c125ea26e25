// cpp_colop_checks_parent.hpp - the four hand-written argument checkers of the column operators (csrc/hjgpu_ops.hip) and check_select_bits
// (csrc/hjgpu_api.hip) as they stood before csrc/colop_checks.hpp replaced them, verbatim but for one change: fail(ctx, status, text) is a
// return of {status, text}.  tests/cpp_colop_checks.cpp compares every decision of the new checks with these: they are the definition.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../include/hjgpu.h"
#include "group_layout.hpp"

namespace parent {

struct Verdict { int status; const char *text; };
static const Verdict OK = {HJGPU_OK, ""};

static bool ranges_overlap(const void *p, size_t pbytes, const void *q, size_t qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pbytes && qbytes && a < b + qbytes && b < a + pbytes;
}

static Verdict check_compact(const uint32_t *bits, size_t n, uint32_t ncols, const uint32_t *const *in, uint32_t *const *out,
                             const uint32_t *rows_out, size_t capacity, const uint64_t *count, bool device_count)
{
    if (!count) return {HJGPU_EINVAL, "null count pointer"};
    if (device_count && ((uintptr_t)count & 7)) return {HJGPU_EALIGN, "d_count must be 8-byte aligned"};
    if (ncols > HJGPU_COMPACT_MAX_COLS) return {HJGPU_EINVAL, "ncols must not exceed HJGPU_COMPACT_MAX_COLS (8)"};
    if (n == 0) return OK;                               // nothing is read, nothing but the count is written: anything else may be NULL
    if (!bits) return {HJGPU_EINVAL, "null d_select_bits (a compaction of every row is a copy)"};
    if ((uintptr_t)bits & 15) return {HJGPU_EALIGN, "d_select_bits must be 16-byte aligned"};
    if (ncols && (!in || !out)) return {HJGPU_EINVAL, "null column array"};
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!in[c] || !out[c]) return {HJGPU_EINVAL, "null column pointer"};
        if (((uintptr_t)in[c] & 15) || ((uintptr_t)out[c] & 15)) return {HJGPU_EALIGN, "input and output columns must be 16-byte aligned"};
    }
    if ((uintptr_t)rows_out & 15) return {HJGPU_EALIGN, "d_rows_out must be 16-byte aligned"};
    if (rows_out && n > 0xFFFFFFFFull) return {HJGPU_EINVAL, "d_rows_out holds 32-bit row numbers: n must not exceed 0xFFFFFFFF"};
    // not in place: no output may share a byte with the mask, an input column or another output
    const void *outs[HJGPU_COMPACT_MAX_COLS + 1];
    uint32_t nouts = 0;
    for (uint32_t c = 0; c < ncols; ++c) outs[nouts++] = out[c];
    if (rows_out) outs[nouts++] = rows_out;
    const size_t obytes = capacity * sizeof(uint32_t), mbytes = (n + 31) / 32 * sizeof(uint32_t);
    for (uint32_t o = 0; o < nouts; ++o) {
        if (ranges_overlap(outs[o], obytes, bits, mbytes)) return {HJGPU_EINVAL, "an output overlaps d_select_bits (the compaction is not in place)"};
        for (uint32_t c = 0; c < ncols; ++c)
            if (ranges_overlap(outs[o], obytes, in[c], n * sizeof(uint32_t)))
                return {HJGPU_EINVAL, "an output overlaps an input column (the compaction is not in place)"};
        for (uint32_t q = 0; q < o; ++q)
            if (ranges_overlap(outs[o], obytes, outs[q], obytes)) return {HJGPU_EINVAL, "an output overlaps another output"};
    }
    return OK;
}

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

static Verdict check_group(const GroupCall &g, const uint64_t *ngroups, bool device_count)
{
    if (!ngroups) return {HJGPU_EINVAL, "null group count pointer"};
    if (device_count && ((uintptr_t)ngroups & 7)) return {HJGPU_EALIGN, "d_ngroups must be 8-byte aligned"};
    if (g.nkeys == 0 || g.nkeys > HJGPU_GROUP_MAX_KEYS) return {HJGPU_EINVAL, "nkeys must be 1 to HJGPU_GROUP_MAX_KEYS (2)"};
    if (g.nvals > HJGPU_GROUP_MAX_VALS) return {HJGPU_EINVAL, "nvals must not exceed HJGPU_GROUP_MAX_VALS (4)"};
    if (hj_group::merge_slots(g.capacity) == 0) return {HJGPU_EINVAL, "capacity must not exceed 2^40 groups"};
    if (g.n == 0) return OK;                             // nothing is read, nothing but the count is written: anything else may be NULL
    if ((uintptr_t)g.bits & 15) return {HJGPU_EALIGN, "d_select_bits must be 16-byte aligned"};
    if (!g.keys_in || !g.keys_out || (g.nvals && (!g.vals_in || !g.sums_out))) return {HJGPU_EINVAL, "null column array"};
    for (uint32_t c = 0; c < g.nkeys; ++c) {
        if (!g.keys_in[c] || !g.keys_out[c]) return {HJGPU_EINVAL, "null key column pointer"};
        if (((uintptr_t)g.keys_in[c] | (uintptr_t)g.keys_out[c]) & 15) return {HJGPU_EALIGN, "key columns must be 16-byte aligned"};
    }
    for (uint32_t c = 0; c < g.nvals; ++c) {
        if (!g.vals_in[c] || !g.sums_out[c]) return {HJGPU_EINVAL, "null measure column pointer"};
        if (((uintptr_t)g.vals_in[c] | (uintptr_t)g.sums_out[c]) & 15) return {HJGPU_EALIGN, "measure and sum columns must be 16-byte aligned"};
    }
    if ((uintptr_t)g.counts_out & 15) return {HJGPU_EALIGN, "d_counts_out must be 16-byte aligned"};
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
                return {HJGPU_EINVAL, i + 1 == nins && g.bits ? "an output overlaps d_select_bits" : "an output overlaps an input column"};
        for (uint32_t q = 0; q < o; ++q)
            if (ranges_overlap(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes)) return {HJGPU_EINVAL, "an output overlaps another output"};
    }
    return OK;
}

struct FilterCall {
    const uint32_t *bits;
    size_t n;
    uint32_t npreds;
    const uint32_t *const *cols;
    const hjgpu_predicate *preds;
    uint32_t *bits_out;
};

static Verdict check_filter(const FilterCall &f, const uint64_t *count, bool device_count)
{
    if (device_count && ((uintptr_t)count & 7)) return {HJGPU_EALIGN, "d_count must be 8-byte aligned"};
    if (f.npreds == 0 || f.npreds > HJGPU_FILTER_MAX_PREDS) return {HJGPU_EINVAL, "npreds must be 1 to HJGPU_FILTER_MAX_PREDS (4)"};
    if (f.n == 0) return OK;                             // nothing is read, nothing but the count is written: anything else may be NULL
    if (!f.bits_out && !count) return {HJGPU_EINVAL, "d_bits_out and the count are both null: nothing to compute"};
    if ((uintptr_t)f.bits & 15) return {HJGPU_EALIGN, "d_select_bits must be 16-byte aligned"};
    if ((uintptr_t)f.bits_out & 15) return {HJGPU_EALIGN, "d_bits_out must be 16-byte aligned"};
    if (!f.cols || !f.preds) return {HJGPU_EINVAL, "null column or predicate array"};
    for (uint32_t p = 0; p < f.npreds; ++p) {
        if (!f.cols[p]) return {HJGPU_EINVAL, "null column pointer"};
        if ((uintptr_t)f.cols[p] & 15) return {HJGPU_EALIGN, "columns must be 16-byte aligned"};
        if (f.preds[p].flags & ~(HJGPU_PRED_NOT | HJGPU_PRED_SIGNED)) return {HJGPU_EINVAL, "unknown predicate flag (HJGPU_PRED_NOT and HJGPU_PRED_SIGNED are defined)"};
        if (f.preds[p].reserved) return {HJGPU_EINVAL, "a predicate's reserved word must be 0"};
    }
    // in place: d_bits_out may be the very pointer d_select_bits - the kernel reads a word of the mask in the wave that stores it, before
    // it stores it -; two bitmaps that overlap in any other way would be read after they were written
    const size_t mbytes = (f.n + 31) / 32 * sizeof(uint32_t), cbytes = f.n * sizeof(uint32_t);
    if (f.bits && f.bits_out && f.bits != f.bits_out && ranges_overlap(f.bits_out, mbytes, f.bits, mbytes))
        return {HJGPU_EINVAL, "d_bits_out overlaps d_select_bits: it may be the very pointer d_select_bits (in place), any other overlap of the two bitmaps is refused"};
    // no output may share a byte with a column or with the other output; the device count word none with the mask either
    for (uint32_t p = 0; p < f.npreds; ++p) {
        if (ranges_overlap(f.bits_out, f.bits_out ? mbytes : 0, f.cols[p], cbytes)) return {HJGPU_EINVAL, "d_bits_out overlaps a column"};
        if (device_count && ranges_overlap(count, count ? sizeof(uint64_t) : 0, f.cols[p], cbytes)) return {HJGPU_EINVAL, "d_count overlaps a column"};
    }
    if (device_count && count) {
        if (ranges_overlap(count, sizeof(uint64_t), f.bits_out, f.bits_out ? mbytes : 0)) return {HJGPU_EINVAL, "d_count overlaps d_bits_out"};
        if (ranges_overlap(count, sizeof(uint64_t), f.bits, f.bits ? mbytes : 0)) return {HJGPU_EINVAL, "d_count overlaps d_select_bits"};
    }
    return OK;
}

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

static Verdict check_gather(const GatherCall &g, const uint64_t *d_counts)
{
    if ((uintptr_t)d_counts & 15) return {HJGPU_EALIGN, "d_counts must be 16-byte aligned"};
    if (g.ncols == 0 || g.ncols > HJGPU_GATHER_MAX_COLS) return {HJGPU_EINVAL, "ncols must be 1 to HJGPU_GATHER_MAX_COLS (4)"};
    if (g.src_rows > 0xFFFFFFFFull) return {HJGPU_EINVAL, "src_rows must not exceed 0xFFFFFFFF: an index is a uint32 and HJGPU_NULL_VAL is never a legal one"};
    if (g.n == 0) return OK;                             // nothing is read, nothing but the counts is written: anything else may be NULL
    if (!g.idx) return {HJGPU_EINVAL, "null d_idx"};
    if ((uintptr_t)g.bits & 15) return {HJGPU_EALIGN, "d_select_bits must be 16-byte aligned"};
    if ((uintptr_t)g.idx & 15) return {HJGPU_EALIGN, "d_idx must be 16-byte aligned"};
    if ((uintptr_t)g.bits_out & 15) return {HJGPU_EALIGN, "d_bits_out must be 16-byte aligned"};
    if (!g.src || !g.out) return {HJGPU_EINVAL, "null column array"};
    for (uint32_t c = 0; c < g.ncols; ++c) {
        if (!g.src[c] || !g.out[c]) return {HJGPU_EINVAL, "null column pointer"};
        if ((uintptr_t)g.src[c] & 15) return {HJGPU_EALIGN, "source columns must be 16-byte aligned"};
        if ((uintptr_t)g.out[c] & 15) return {HJGPU_EALIGN, "output columns must be 16-byte aligned"};
    }
    const size_t mbytes = (g.n + 31) / 32 * sizeof(uint32_t), cbytes = g.n * sizeof(uint32_t), sbytes = g.src_rows * sizeof(uint32_t);
    // in place: an output column may be the very pointer d_idx - a lane reads its index vector before it stores the same vector - and, being
    // an output, only one can; d_bits_out may be the very pointer d_select_bits (hj_lookup.hpp's IN-PLACE RULE).  Every other shared byte
    // between an output and anything else would be read after it was written, or written twice
    for (uint32_t c = 0; c < g.ncols; ++c) {
        if (g.out[c] != g.idx && ranges_overlap(g.out[c], cbytes, g.idx, cbytes))
            return {HJGPU_EINVAL, "an output column overlaps d_idx: it may be the very pointer d_idx (in place), any other overlap is refused"};
        for (uint32_t q = 0; q < c; ++q)
            if (ranges_overlap(g.out[c], cbytes, g.out[q], cbytes)) return {HJGPU_EINVAL, "an output column overlaps another output column"};
        for (uint32_t q = 0; q < g.ncols; ++q)
            if (ranges_overlap(g.out[c], cbytes, g.src[q], sbytes)) return {HJGPU_EINVAL, "an output column overlaps a source column"};
        if (ranges_overlap(g.out[c], cbytes, g.bits, g.bits ? mbytes : 0)) return {HJGPU_EINVAL, "an output column overlaps d_select_bits"};
    }
    if (g.bits_out) {
        if (g.bits && g.bits != g.bits_out && ranges_overlap(g.bits_out, mbytes, g.bits, mbytes))
            return {HJGPU_EINVAL, "d_bits_out overlaps d_select_bits: it may be the very pointer d_select_bits (in place), any other overlap of the two bitmaps is refused"};
        if (ranges_overlap(g.bits_out, mbytes, g.idx, cbytes)) return {HJGPU_EINVAL, "d_bits_out overlaps d_idx"};
        for (uint32_t c = 0; c < g.ncols; ++c) {
            if (ranges_overlap(g.bits_out, mbytes, g.out[c], cbytes)) return {HJGPU_EINVAL, "d_bits_out overlaps an output column"};
            if (ranges_overlap(g.bits_out, mbytes, g.src[c], sbytes)) return {HJGPU_EINVAL, "d_bits_out overlaps a source column"};
        }
    }
    if (d_counts) {
        const size_t wbytes = 2 * sizeof(uint64_t);
        if (ranges_overlap(d_counts, wbytes, g.bits, g.bits ? mbytes : 0)) return {HJGPU_EINVAL, "d_counts overlaps d_select_bits"};
        if (ranges_overlap(d_counts, wbytes, g.idx, cbytes)) return {HJGPU_EINVAL, "d_counts overlaps d_idx"};
        if (ranges_overlap(d_counts, wbytes, g.bits_out, g.bits_out ? mbytes : 0)) return {HJGPU_EINVAL, "d_counts overlaps d_bits_out"};
        for (uint32_t c = 0; c < g.ncols; ++c) {
            if (ranges_overlap(d_counts, wbytes, g.out[c], cbytes)) return {HJGPU_EINVAL, "d_counts overlaps an output column"};
            if (ranges_overlap(d_counts, wbytes, g.src[c], sbytes)) return {HJGPU_EINVAL, "d_counts overlaps a source column"};
        }
    }
    return OK;
}

static Verdict check_select_bits(const uint32_t *select_bits, const uint32_t *match_bits, size_t outer)
{
    if ((uintptr_t)select_bits & 15) return {HJGPU_EALIGN, "d_select_bits must be 16-byte aligned"};
    const uintptr_t s = (uintptr_t)select_bits, m = (uintptr_t)match_bits, bytes = (outer + 31) / 32 * sizeof(uint32_t);
    if (select_bits && match_bits && s != m && s < m + bytes && m < s + bytes)
        return {HJGPU_EINVAL, "d_match_bits overlaps d_select_bits: it may be the very pointer d_select_bits (in place), any other overlap of the two bitmaps is refused"};
    return OK;
}

}  // namespace parent
