// colop_checks.hpp - what the column operators (hjgpu_compact_selected, hjgpu_group_sum, hjgpu_group_agg, hjgpu_group_by, hjgpu_filter_selected, hjgpu_gather_selected, hjgpu_lookup_wide, hjgpu_order_by: hjgpu_colops.hip)
// and the selected look-ups refuse from their arguments alone, before anything is allocated or enqueued (DESIGN.md section 5 "Argument checks
// of the column operators").  Plain host C++, no HIP and no context: a check returns {status, text}, its caller hands that to fail().
// tests/test_colop_checks.py compiles it with g++ and compares every decision with the hand-written checkers it replaced.
//
// A check is its operator's own head - the count pointer, the limits, the n == 0 accept, the required pointers - and then ONE rule over a
// table of the pointers the kernels will read and write: every one aligned, and no written range shares a byte with any other range, except
// that a written operand may be the very pointer of the one read operand it names (in place).  No device pointer is dereferenced.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/hjgpu.h"
#include "group_layout.hpp"
#include "wide_group_layout.hpp"
#include "wide_lookup_layout.hpp"
#include "order_layout.hpp"

namespace colop {

struct Verdict {
    int status;
    char text[192];                                     // (inside the value: fail() copies it)
};

inline Verdict no_objection()
{
    Verdict v;
    v.status = HJGPU_OK; v.text[0] = 0;
    return v;
}

#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline Verdict refuse(int status, const char *fmt, ...)
{
    Verdict v;
    v.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(v.text, sizeof(v.text), fmt, ap);
    va_end(ap);
    return v;
}

struct Operand {
    const void *p;                                      // NULL: an absent optional operand, it takes no part
    size_t bytes;
    bool written;
    uint32_t align;
    const char *name;
    int in_place;                                       // a written operand: the read operand it may coincide with exactly, or -1
};

// the largest table, hjgpu_group_by_async's: the mask, 4 keys, 4 aggregates' a and b, 4 key outputs, 4 aggregate outputs, the counts and
// the count word (23; a compaction has the mask, 8 inputs, 8 outputs and the row numbers: 18)
constexpr int MAX_OPERANDS = 1 + 2 * HJGPU_GROUP_BY_MAX_KEYS + 3 * HJGPU_AGG_MAX_AGGS + 2;
static_assert(MAX_OPERANDS >= 2 * HJGPU_COMPACT_MAX_COLS + 2, "the operand table holds a compaction's operands");

struct Operands {
    Operand v[MAX_OPERANDS];
    int n = 0;
    int read(const void *p, size_t bytes, uint32_t align, const char *name) { v[n] = {p, bytes, false, align, name, -1}; return n++; }
    int write(const void *p, size_t bytes, uint32_t align, const char *name, int in_place = -1) { v[n] = {p, bytes, true, align, name, in_place}; return n++; }
};

inline bool ranges_overlap(const void *p, size_t pbytes, const void *q, size_t qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && pbytes && qbytes && a < b + qbytes && b < a + pbytes;
}

// The one rule.  All alignments first; then every written operand against every read operand and every earlier written one.  In place: a
// kernel reads a vector (a bitmap word, an index vector) in the lane that stores it, before it stores it, so the very pointer is safe - any
// other shared byte would be read after it was written, or written twice.
inline Verdict check_operands(const Operands &t)
{
    for (int i = 0; i < t.n; ++i)
        if ((uintptr_t)t.v[i].p & (t.v[i].align - 1)) return refuse(HJGPU_EALIGN, "%s must be %u-byte aligned", t.v[i].name, t.v[i].align);
    for (int i = 0; i < t.n; ++i) {
        const Operand &w = t.v[i];
        if (!w.written) continue;
        for (int j = 0; j < t.n; ++j) {
            const Operand &o = t.v[j];
            if (j == i || (o.written && j > i) || !ranges_overlap(w.p, w.bytes, o.p, o.bytes)) continue;
            if (w.in_place != j) return refuse(HJGPU_EINVAL, "%s overlaps %s", w.name, o.name);
            if (w.p != o.p)
                return refuse(HJGPU_EINVAL, "%s overlaps %s: it may be the very pointer %s (in place), any other overlap is refused", w.name, o.name, o.name);
        }
    }
    return no_objection();
}

inline size_t bitmap_bytes(size_t n) { return (n + 31) / 32 * sizeof(uint32_t); }

// ---- the selected look-ups' mask (NULL: no mask): d_match_bits may be d_select_bits itself ---------------------------------------------
inline Verdict check_select_bits(const uint32_t *select_bits, const uint32_t *match_bits, size_t outer)
{
    Operands t;
    const int mask = t.read(select_bits, bitmap_bytes(outer), 16, "d_select_bits");
    t.write(match_bits, bitmap_bytes(outer), 1, "d_match_bits", mask);       // (its alignment: check_lookup_columns)
    return check_operands(t);
}

// ---- hjgpu_compact_selected ---------------------------------------------------------------------------------------------------------------
struct CompactCall {
    const uint32_t *bits;
    size_t n;
    uint32_t ncols;
    const uint32_t *const *in;
    uint32_t *const *out;
    uint32_t *rows_out;
    size_t capacity;
};

inline Verdict check_compact(const CompactCall &c, const uint64_t *count, bool device_count)
{
    if (!count) return refuse(HJGPU_EINVAL, "null count pointer");
    if (device_count && ((uintptr_t)count & 7)) return refuse(HJGPU_EALIGN, "d_count must be 8-byte aligned");
    if (c.ncols > HJGPU_COMPACT_MAX_COLS) return refuse(HJGPU_EINVAL, "ncols must not exceed HJGPU_COMPACT_MAX_COLS (8)");
    if (c.n == 0) return no_objection();                      // nothing is read, nothing but the count is written: anything else may be NULL
    if (!c.bits) return refuse(HJGPU_EINVAL, "null d_select_bits (a compaction of every row is a copy)");
    if (c.ncols && (!c.in || !c.out)) return refuse(HJGPU_EINVAL, "null column array");
    for (uint32_t k = 0; k < c.ncols; ++k)
        if (!c.in[k] || !c.out[k]) return refuse(HJGPU_EINVAL, "null column pointer");
    if (c.rows_out && c.n > 0xFFFFFFFFull) return refuse(HJGPU_EINVAL, "d_rows_out holds 32-bit row numbers: n must not exceed 0xFFFFFFFF");
    // not in place.  (d_count is not in the table: the other three operators refuse a device count word that overlaps an operand, this one
    // never has - a follow-up, it would refuse calls that are accepted today)
    Operands t;
    const size_t obytes = c.capacity * sizeof(uint32_t);
    t.read(c.bits, bitmap_bytes(c.n), 16, "d_select_bits");
    for (uint32_t k = 0; k < c.ncols; ++k) t.read(c.in[k], c.n * sizeof(uint32_t), 16, "an input column");
    for (uint32_t k = 0; k < c.ncols; ++k) t.write(c.out[k], obytes, 16, "an output column");
    t.write(c.rows_out, obytes, 16, "d_rows_out");
    return check_operands(t);
}

// ---- hjgpu_group_sum ------------------------------------------------------------------------------------------------------------------------
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

inline Verdict check_group(const GroupCall &g, const uint64_t *ngroups, bool device_count)
{
    if (!ngroups) return refuse(HJGPU_EINVAL, "null group count pointer");
    if (device_count && ((uintptr_t)ngroups & 7)) return refuse(HJGPU_EALIGN, "d_ngroups must be 8-byte aligned");
    if (g.nkeys == 0 || g.nkeys > HJGPU_GROUP_MAX_KEYS) return refuse(HJGPU_EINVAL, "nkeys must be 1 to HJGPU_GROUP_MAX_KEYS (2)");
    if (g.nvals > HJGPU_GROUP_MAX_VALS) return refuse(HJGPU_EINVAL, "nvals must not exceed HJGPU_GROUP_MAX_VALS (4)");
    if (hj_group::merge_slots(g.capacity) == 0) return refuse(HJGPU_EINVAL, "capacity must not exceed 2^40 groups");
    if (g.n == 0) return no_objection();                      // nothing is read, nothing but the count is written: anything else may be NULL
    if (!g.keys_in || !g.keys_out || (g.nvals && (!g.vals_in || !g.sums_out))) return refuse(HJGPU_EINVAL, "null column array");
    for (uint32_t k = 0; k < g.nkeys; ++k)
        if (!g.keys_in[k] || !g.keys_out[k]) return refuse(HJGPU_EINVAL, "null key column pointer");
    for (uint32_t k = 0; k < g.nvals; ++k)
        if (!g.vals_in[k] || !g.sums_out[k]) return refuse(HJGPU_EINVAL, "null measure column pointer");
    Operands t;
    t.read(g.bits, bitmap_bytes(g.n), 16, "d_select_bits");
    for (uint32_t k = 0; k < g.nkeys; ++k) t.read(g.keys_in[k], g.n * sizeof(uint32_t), 16, "a key column");
    for (uint32_t k = 0; k < g.nvals; ++k) t.read(g.vals_in[k], g.n * sizeof(uint32_t), 16, "a measure column");
    for (uint32_t k = 0; k < g.nkeys; ++k) t.write(g.keys_out[k], g.capacity * sizeof(uint32_t), 16, "a key output column");
    for (uint32_t k = 0; k < g.nvals; ++k) t.write(g.sums_out[k], g.capacity * sizeof(uint64_t), 16, "a sum column");
    t.write(g.counts_out, g.capacity * sizeof(uint64_t), 16, "d_counts_out");
    if (device_count) t.write(ngroups, sizeof(uint64_t), 8, "d_ngroups");
    return check_operands(t);
}

// ---- hjgpu_group_agg ------------------------------------------------------------------------------------------------------------------------
struct GroupAggCall {
    const uint32_t *bits;
    size_t n;
    uint32_t nkeys, naggs;
    const uint32_t *const *keys_in;
    const hjgpu_aggregate *aggs;                        // a host array, copied by value
    uint32_t *const *keys_out;
    uint64_t *counts_out;
    uint64_t *const *aggs_out;
    size_t capacity;
};

// check_group's head with nkeys == 0 legal (the scalar aggregate: the key arrays may then be NULL) and no more than max_keys key columns
// (too_many_keys: the refusal's text), then every aggregate by its index
inline Verdict check_keys_and_aggregates(const GroupAggCall &g, const uint64_t *ngroups, bool device_count, uint32_t max_keys, const char *too_many_keys)
{
    if (!ngroups) return refuse(HJGPU_EINVAL, "null group count pointer");
    if (device_count && ((uintptr_t)ngroups & 7)) return refuse(HJGPU_EALIGN, "d_ngroups must be 8-byte aligned");
    if (g.nkeys > max_keys) return refuse(HJGPU_EINVAL, "%s", too_many_keys);
    if (g.naggs > HJGPU_AGG_MAX_AGGS) return refuse(HJGPU_EINVAL, "naggs must not exceed HJGPU_AGG_MAX_AGGS (4)");
    if (hj_group::merge_slots(g.capacity) == 0) return refuse(HJGPU_EINVAL, "capacity must not exceed 2^40 groups");
    if (g.n == 0) return no_objection();                      // nothing is read, nothing but the count is written: anything else may be NULL
    if ((g.nkeys && (!g.keys_in || !g.keys_out)) || (g.naggs && !g.aggs_out)) return refuse(HJGPU_EINVAL, "null column array");
    if (g.naggs && !g.aggs) return refuse(HJGPU_EINVAL, "null aggregate array");
    for (uint32_t k = 0; k < g.nkeys; ++k)
        if (!g.keys_in[k] || !g.keys_out[k]) return refuse(HJGPU_EINVAL, "null key column pointer");
    for (uint32_t c = 0; c < g.naggs; ++c) {
        const hjgpu_aggregate &a = g.aggs[c];
        if (a.fn > HJGPU_AGG_MAX) return refuse(HJGPU_EINVAL, "aggregate %u: unknown function %u (HJGPU_AGG_SUM, _SUM_MUL, _MIN and _MAX are defined)", c, a.fn);
        if (a.flags & ~HJGPU_AGG_SIGNED) return refuse(HJGPU_EINVAL, "aggregate %u: unknown flag (HJGPU_AGG_SIGNED is defined)", c);
        if (!a.d_a) return refuse(HJGPU_EINVAL, "aggregate %u: null d_a", c);
        if (a.fn == HJGPU_AGG_SUM_MUL && !a.d_b) return refuse(HJGPU_EINVAL, "aggregate %u: null d_b under HJGPU_AGG_SUM_MUL", c);
        if (a.fn != HJGPU_AGG_SUM_MUL && a.d_b) return refuse(HJGPU_EINVAL, "aggregate %u: d_b must be NULL unless the function is HJGPU_AGG_SUM_MUL", c);
        if (!g.aggs_out[c]) return refuse(HJGPU_EINVAL, "aggregate %u: null output column pointer", c);
    }
    Operands t;
    t.read(g.bits, bitmap_bytes(g.n), 16, "d_select_bits");
    for (uint32_t k = 0; k < g.nkeys; ++k) t.read(g.keys_in[k], g.n * sizeof(uint32_t), 16, "a key column");
    for (uint32_t c = 0; c < g.naggs; ++c) t.read(g.aggs[c].d_a, g.n * sizeof(uint32_t), 16, "an aggregate's column d_a");
    for (uint32_t c = 0; c < g.naggs; ++c) t.read(g.aggs[c].d_b, g.n * sizeof(uint32_t), 16, "an aggregate's column d_b");
    for (uint32_t k = 0; k < g.nkeys; ++k) t.write(g.keys_out[k], g.capacity * sizeof(uint32_t), 16, "a key output column");
    for (uint32_t c = 0; c < g.naggs; ++c) t.write(g.aggs_out[c], g.capacity * sizeof(uint64_t), 16, "an aggregate output column");
    t.write(g.counts_out, g.capacity * sizeof(uint64_t), 16, "d_counts_out");
    if (device_count) t.write(ngroups, sizeof(uint64_t), 8, "d_ngroups");
    return check_operands(t);
}

inline Verdict check_group_agg(const GroupAggCall &g, const uint64_t *ngroups, bool device_count)
{
    return check_keys_and_aggregates(g, ngroups, device_count, HJGPU_GROUP_MAX_KEYS, "nkeys must not exceed HJGPU_GROUP_MAX_KEYS (2)");
}

// ---- hjgpu_group_by -------------------------------------------------------------------------------------------------------------------------
// check_group_agg with up to four key inputs and four key outputs (the capacity rule is the same for both table layouts)
inline Verdict check_group_by(const GroupAggCall &g, const uint64_t *ngroups, bool device_count)
{
    static_assert(hj_wide::MAX_KEYS == HJGPU_GROUP_BY_MAX_KEYS && hj_wide::MAX_CAPACITY == hj_group::MAX_CAPACITY, "one capacity rule, four key words");
    return check_keys_and_aggregates(g, ngroups, device_count, HJGPU_GROUP_BY_MAX_KEYS, "nkeys must not exceed HJGPU_GROUP_BY_MAX_KEYS (4)");
}

// ---- hjgpu_filter_selected ------------------------------------------------------------------------------------------------------------------
struct FilterCall {
    const uint32_t *bits;
    size_t n;
    uint32_t npreds;
    const uint32_t *const *cols;
    const hjgpu_predicate *preds;
    uint32_t *bits_out;
};

inline Verdict check_filter(const FilterCall &f, const uint64_t *count, bool device_count)
{
    if (device_count && ((uintptr_t)count & 7)) return refuse(HJGPU_EALIGN, "d_count must be 8-byte aligned");
    if (f.npreds == 0 || f.npreds > HJGPU_FILTER_MAX_PREDS) return refuse(HJGPU_EINVAL, "npreds must be 1 to HJGPU_FILTER_MAX_PREDS (4)");
    if (f.n == 0) return no_objection();                      // nothing is read, nothing but the count is written: anything else may be NULL
    if (!f.bits_out && !count) return refuse(HJGPU_EINVAL, "d_bits_out and the count are both null: nothing to compute");
    if (!f.cols || !f.preds) return refuse(HJGPU_EINVAL, "null column or predicate array");
    for (uint32_t p = 0; p < f.npreds; ++p) {
        if (!f.cols[p]) return refuse(HJGPU_EINVAL, "null column pointer");
        if (f.preds[p].flags & ~(HJGPU_PRED_NOT | HJGPU_PRED_SIGNED)) return refuse(HJGPU_EINVAL, "unknown predicate flag (HJGPU_PRED_NOT and HJGPU_PRED_SIGNED are defined)");
        if (f.preds[p].reserved) return refuse(HJGPU_EINVAL, "a predicate's reserved word must be 0");
    }
    Operands t;
    const int mask = t.read(f.bits, bitmap_bytes(f.n), 16, "d_select_bits");
    for (uint32_t p = 0; p < f.npreds; ++p) t.read(f.cols[p], f.n * sizeof(uint32_t), 16, "a column");
    t.write(f.bits_out, bitmap_bytes(f.n), 16, "d_bits_out", mask);
    if (device_count) t.write(count, sizeof(uint64_t), 8, "d_count");        // (the blocking form's count is the caller's own word in host memory)
    return check_operands(t);
}

// ---- hjgpu_gather_selected ------------------------------------------------------------------------------------------------------------------
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

// d_counts: the device form's two count words (NULL: none, and the blocking form, whose words are the context's)
inline Verdict check_gather(const GatherCall &g, const uint64_t *d_counts)
{
    if ((uintptr_t)d_counts & 15) return refuse(HJGPU_EALIGN, "d_counts must be 16-byte aligned");
    if (g.ncols == 0 || g.ncols > HJGPU_GATHER_MAX_COLS) return refuse(HJGPU_EINVAL, "ncols must be 1 to HJGPU_GATHER_MAX_COLS (4)");
    if (g.src_rows > 0xFFFFFFFFull) return refuse(HJGPU_EINVAL, "src_rows must not exceed 0xFFFFFFFF: an index is a uint32 and HJGPU_NULL_VAL is never a legal one");
    if (g.n == 0) return no_objection();                      // nothing is read, nothing but the counts is written: anything else may be NULL
    if (!g.idx) return refuse(HJGPU_EINVAL, "null d_idx");
    if (!g.src || !g.out) return refuse(HJGPU_EINVAL, "null column array");
    for (uint32_t k = 0; k < g.ncols; ++k)
        if (!g.src[k] || !g.out[k]) return refuse(HJGPU_EINVAL, "null column pointer");
    // (every output column names d_idx; being outputs, only one of them can be it)
    Operands t;
    const size_t cbytes = g.n * sizeof(uint32_t);
    const int mask = t.read(g.bits, bitmap_bytes(g.n), 16, "d_select_bits");
    const int idx = t.read(g.idx, cbytes, 16, "d_idx");
    for (uint32_t k = 0; k < g.ncols; ++k) t.read(g.src[k], g.src_rows * sizeof(uint32_t), 16, "a source column");
    for (uint32_t k = 0; k < g.ncols; ++k) t.write(g.out[k], cbytes, 16, "an output column", idx);
    t.write(g.bits_out, bitmap_bytes(g.n), 16, "d_bits_out", mask);
    t.write(d_counts, 2 * sizeof(uint64_t), 16, "d_counts");
    return check_operands(t);
}

// ---- hjgpu_lookup_wide ------------------------------------------------------------------------------------------------------------------------
struct LookupWideCall {
    uint32_t nkeys;
    const uint32_t *const *inner_keys;                  // host arrays of nkeys device pointers, copied by value
    const uint32_t *inner_vals;
    size_t inner;
    const uint32_t *const *outer_keys;
    size_t outer;
    const hjgpu_npj_params *params;                     // NULL: the defaults
    const uint32_t *select_bits;
    uint32_t *vals_out, *match_bits;
};

// d_result: the device form's result words (NULL: none, and the blocking form, whose words are the context's).  The join-mode flags are
// the entry point's to refuse (refuse_join_mode names them).  outer == 0: nothing is read, not even the build side; inner == 0: no key of
// either side is read
inline Verdict check_lookup_wide(const LookupWideCall &c, const hjgpu_result *d_result)
{
    static_assert(hj_wlk::MIN_KEYS == HJGPU_LOOKUP_WIDE_MIN_KEYS && hj_wlk::MAX_KEYS == HJGPU_LOOKUP_WIDE_MAX_KEYS, "two to four key words");
    if (c.nkeys == 1) return refuse(HJGPU_EINVAL, "nkeys must be 2 to HJGPU_LOOKUP_WIDE_MAX_KEYS (4): one key column is hjgpu_lookup_selected");
    if (c.nkeys < HJGPU_LOOKUP_WIDE_MIN_KEYS || c.nkeys > HJGPU_LOOKUP_WIDE_MAX_KEYS) return refuse(HJGPU_EINVAL, "nkeys must be 2 to HJGPU_LOOKUP_WIDE_MAX_KEYS (4)");
    if (c.params && !(c.params->load >= 0 && c.params->load <= hj_wlk::MAX_LOAD)) return refuse(HJGPU_EINVAL, "load must be 0 (the default, 0.5) or in (0, 0.99]");
    if ((uintptr_t)d_result & 15) return refuse(HJGPU_EALIGN, "d_result must be 16-byte aligned");
    if (c.outer == 0) return no_objection();                  // nothing is read, nothing but the result is written: anything else may be NULL
    if (c.inner) {
        if (!c.inner_keys || !c.outer_keys) return refuse(HJGPU_EINVAL, "null key column array");
        for (uint32_t k = 0; k < c.nkeys; ++k)
            if (!c.inner_keys[k] || !c.outer_keys[k]) return refuse(HJGPU_EINVAL, "null key column pointer");
        if (!c.inner_vals) return refuse(HJGPU_EINVAL, "null d_inner_vals");
    }
    Operands t;
    const size_t obytes = c.outer * sizeof(uint32_t), ibytes = c.inner * sizeof(uint32_t);
    const int mask = t.read(c.select_bits, bitmap_bytes(c.outer), 16, "d_select_bits");
    for (uint32_t k = 0; c.inner && k < c.nkeys; ++k) t.read(c.outer_keys[k], obytes, 16, "a probe key column");
    for (uint32_t k = 0; c.inner && k < c.nkeys; ++k) t.read(c.inner_keys[k], ibytes, 16, "a build key column");
    t.read(c.inner_vals, ibytes, 16, "d_inner_vals");
    t.write(c.vals_out, obytes, 16, "d_vals_out");
    t.write(c.match_bits, bitmap_bytes(c.outer), 16, "d_match_bits", mask);
    t.write(d_result, sizeof(hjgpu_result), 16, "d_result");
    return check_operands(t);
}

// ---- hjgpu_order_by ---------------------------------------------------------------------------------------------------------------------------
struct OrderCall {
    const uint32_t *bits;                               // NULL: every row
    size_t n;
    uint32_t nkeys;
    const hjgpu_order_key *keys;                        // host arrays, copied by value
    uint32_t ncols;
    const hjgpu_order_column *cols;
    uint32_t *rows_out;
    size_t limit;
};

static_assert(MAX_OPERANDS >= 1 + HJGPU_ORDER_MAX_KEYS + 2 * HJGPU_ORDER_MAX_COLS + 2, "the operand table holds an ordering's operands");
static_assert(hj_order::MAX_KEYS == HJGPU_ORDER_MAX_KEYS && hj_order::MAX_COLS == HJGPU_ORDER_MAX_COLS && hj_order::DESC == HJGPU_ORDER_DESC &&
              hj_order::SIGNED == HJGPU_ORDER_SIGNED && hj_order::WIDE == HJGPU_ORDER_WIDE, "order_layout.hpp speaks the header's flags");

// not in place: an output is checked over its first min(limit, n) elements
inline Verdict check_order_by(const OrderCall &o, const uint64_t *count, bool device_count)
{
    if (!count) return refuse(HJGPU_EINVAL, "null count pointer");
    if (device_count && ((uintptr_t)count & 7)) return refuse(HJGPU_EALIGN, "d_count must be 8-byte aligned");
    if (o.nkeys == 0) return refuse(HJGPU_EINVAL, "nkeys must be 1 to HJGPU_ORDER_MAX_KEYS (4): with no key the call is hjgpu_compact_selected");
    if (o.nkeys > HJGPU_ORDER_MAX_KEYS) return refuse(HJGPU_EINVAL, "nkeys must be 1 to HJGPU_ORDER_MAX_KEYS (4)");
    if (o.ncols > HJGPU_ORDER_MAX_COLS) return refuse(HJGPU_EINVAL, "ncols must not exceed HJGPU_ORDER_MAX_COLS (8)");
    if (o.n > 0xFFFFFFFFull) return refuse(HJGPU_EINVAL, "n must not exceed 0xFFFFFFFF: a row number is a uint32");
    if (o.n == 0) return no_objection();                      // nothing is read, nothing but the count is written: anything else may be NULL
    if (!o.keys) return refuse(HJGPU_EINVAL, "null key array");
    if (o.ncols && !o.cols) return refuse(HJGPU_EINVAL, "null column array");
    for (uint32_t k = 0; k < o.nkeys; ++k) {
        const hjgpu_order_key &key = o.keys[k];
        if (key.flags & ~(HJGPU_ORDER_DESC | HJGPU_ORDER_SIGNED | HJGPU_ORDER_WIDE))
            return refuse(HJGPU_EINVAL, "key %u: unknown flag (HJGPU_ORDER_DESC, _SIGNED and _WIDE are defined)", k);
        if (key.reserved) return refuse(HJGPU_EINVAL, "key %u: the reserved word must be 0", k);
        if (!key.d_col) return refuse(HJGPU_EINVAL, "key %u: null d_col", k);
    }
    for (uint32_t c = 0; c < o.ncols; ++c) {
        const hjgpu_order_column &col = o.cols[c];
        if (col.flags & ~HJGPU_ORDER_WIDE) return refuse(HJGPU_EINVAL, "column %u: unknown flag (HJGPU_ORDER_WIDE is defined)", c);
        if (col.reserved) return refuse(HJGPU_EINVAL, "column %u: the reserved word must be 0", c);
        if (!col.d_in) return refuse(HJGPU_EINVAL, "column %u: null d_in", c);
        if (!col.d_out) return refuse(HJGPU_EINVAL, "column %u: null d_out", c);
    }
    Operands t;
    const size_t m = o.limit < o.n ? o.limit : o.n;
    auto width = [](uint32_t flags) -> size_t { return (flags & HJGPU_ORDER_WIDE) ? sizeof(uint64_t) : sizeof(uint32_t); };
    t.read(o.bits, bitmap_bytes(o.n), 16, "d_select_bits");
    for (uint32_t k = 0; k < o.nkeys; ++k) t.read(o.keys[k].d_col, o.n * width(o.keys[k].flags), 16, "a key column");
    for (uint32_t c = 0; c < o.ncols; ++c) t.read(o.cols[c].d_in, o.n * width(o.cols[c].flags), 16, "a carried input column");
    for (uint32_t c = 0; c < o.ncols; ++c) t.write(o.cols[c].d_out, m * width(o.cols[c].flags), 16, "an output column");
    t.write(o.rows_out, m * sizeof(uint32_t), 16, "d_rows_out");
    if (device_count) t.write(count, sizeof(uint64_t), 8, "d_count");
    return check_operands(t);
}

}  // namespace colop
