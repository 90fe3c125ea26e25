// cpp_group_agg_checks.cpp - csrc/colop_checks.hpp check_group_agg and csrc/agg_layout.hpp's transform, on the CPU.
// Device pointers are fabricated integers in a fake arena - the check dereferences none; only the host arrays of pointers and aggregates are
// real.  Both forms (blocking, device count): one valid call, then every single deviation from it must give the stated status and text.
// The transform: term / combine / result over edge values against the definition of SUM, SUM(a * b), MIN and MAX, starting from the
// tables' initial word 0.  Prints "ok: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "agg_layout.hpp"
#include "colop_checks.hpp"

static const uintptr_t ARENA = 0x40000000u, STRIDE = 0x10000u;       // every operand in a region of its own, far from its neighbours
static long cases = 0;

// the operands of the valid call, in the order of the check's table
enum { BITS, KEY0, KEY1, A0, A1, A2, A3, B1, KOUT0, KOUT1, OUT0, OUT1, OUT2, OUT3, COUNTS, NGROUPS, NOPS };
static const char *const NAME[NOPS] = {"mask", "key 0", "key 1", "a 0", "a 1", "a 2", "a 3", "b 1", "key out 0", "key out 1", "out 0", "out 1", "out 2", "out 3",
                                       "counts", "d_ngroups"};

struct Call {
    uintptr_t p[NOPS];
    size_t n, capacity;
    uint32_t nkeys, naggs;
    hjgpu_aggregate aggs[5];
    bool null_keys_in, null_keys_out, null_aggs, null_aggs_out;
    bool device;
};

static Call base(bool device)
{
    Call c;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < NOPS; ++i) c.p[i] = ARENA + (uintptr_t)i * STRIDE;
    c.n = 1000; c.capacity = 1000; c.nkeys = 2; c.naggs = 4; c.device = device;
    c.aggs[0] = {HJGPU_AGG_SUM, 0, nullptr, nullptr};
    c.aggs[1] = {HJGPU_AGG_SUM_MUL, HJGPU_AGG_SIGNED, nullptr, nullptr};
    c.aggs[2] = {HJGPU_AGG_MIN, 0, nullptr, nullptr};
    c.aggs[3] = {HJGPU_AGG_MAX, HJGPU_AGG_SIGNED, nullptr, nullptr};
    c.aggs[4] = {HJGPU_AGG_SUM, 0, nullptr, nullptr};
    return c;
}

static size_t bytes_of(const Call &c, int i)
{
    if (i == BITS) return (c.n + 31) / 32 * 4;
    if (i <= B1) return c.n * 4;
    if (i <= KOUT1) return c.capacity * 4;
    if (i <= COUNTS) return c.capacity * 8;
    return 8;
}

// the aggregates' pointers: an entry of `set` that is not ~0 replaces what the operand table gives
struct Override { uintptr_t a[5], b[5]; };
static Override no_override()
{
    Override o;
    for (int i = 0; i < 5; ++i) o.a[i] = o.b[i] = ~(uintptr_t)0;
    return o;
}

static colop::Verdict run(const Call &c, const Override &o = no_override())
{
    const uint32_t *keys_in[3] = {(const uint32_t *)c.p[KEY0], (const uint32_t *)c.p[KEY1], (const uint32_t *)(ARENA + 40 * STRIDE)};
    uint32_t *keys_out[3] = {(uint32_t *)c.p[KOUT0], (uint32_t *)c.p[KOUT1], (uint32_t *)(ARENA + 41 * STRIDE)};
    uint64_t *aggs_out[5] = {(uint64_t *)c.p[OUT0], (uint64_t *)c.p[OUT1], (uint64_t *)c.p[OUT2], (uint64_t *)c.p[OUT3], (uint64_t *)(ARENA + 42 * STRIDE)};
    hjgpu_aggregate aggs[5];
    for (int i = 0; i < 5; ++i) {
        aggs[i] = c.aggs[i];
        aggs[i].d_a = (const uint32_t *)(i < 4 ? c.p[A0 + i] : ARENA + 43 * STRIDE);
        aggs[i].d_b = i == 1 ? (const uint32_t *)c.p[B1] : nullptr;
        if (o.a[i] != ~(uintptr_t)0) aggs[i].d_a = (const uint32_t *)o.a[i];
        if (o.b[i] != ~(uintptr_t)0) aggs[i].d_b = (const uint32_t *)o.b[i];
    }
    ++cases;
    return colop::check_group_agg({(const uint32_t *)c.p[BITS], c.n, c.nkeys, c.naggs, c.null_keys_in ? nullptr : keys_in, c.null_aggs ? nullptr : aggs,
                                   c.null_keys_out ? nullptr : keys_out, (uint64_t *)c.p[COUNTS], c.null_aggs_out ? nullptr : aggs_out, c.capacity},
                                  (const uint64_t *)c.p[NGROUPS], c.device);
}

static void expect(const colop::Verdict &v, int status, const char *text, const char *what, const char *detail = "")
{
    if (v.status == status && (!text || strstr(v.text, text))) return;
    printf("FAILED %s %s: status %d \"%s\", want status %d%s%s\n", what, detail, v.status, v.text, status, text ? " with " : "", text ? text : "");
    exit(1);
}

static void checks(bool device)
{
    const Call c0 = base(device);
    expect(run(c0), HJGPU_OK, nullptr, "the valid call");
    char idx[32];
    // the aggregates: function, flags, d_a, d_b - each refusal names the aggregate's index
    for (uint32_t a = 0; a < 4; ++a) {
        snprintf(idx, sizeof(idx), "aggregate %u:", a);
        for (uint32_t fn : {4u, 5u, 0x80000000u, 0xFFFFFFFFu}) {
            Call c = c0; c.aggs[a].fn = fn;
            Override o = no_override(); o.b[a] = 0;
            expect(run(c, o), HJGPU_EINVAL, idx, "fn > 3");
            expect(run(c), HJGPU_EINVAL, idx, "fn > 3");
        }
        for (int bit = 1; bit < 32; ++bit) { Call c = c0; c.aggs[a].flags |= 1u << bit; expect(run(c), HJGPU_EINVAL, idx, "a flag bit outside HJGPU_AGG_SIGNED"); }
        { Call c = c0; c.aggs[a].flags ^= HJGPU_AGG_SIGNED; expect(run(c), HJGPU_OK, nullptr, "HJGPU_AGG_SIGNED flipped"); }
        { Override o = no_override(); o.a[a] = 0; expect(run(c0, o), HJGPU_EINVAL, idx, "d_a == NULL"); }
        Override o = no_override();
        if (c0.aggs[a].fn == HJGPU_AGG_SUM_MUL) { o.b[a] = 0; expect(run(c0, o), HJGPU_EINVAL, idx, "d_b == NULL under SUM_MUL"); }
        else { o.b[a] = ARENA + 50 * STRIDE; expect(run(c0, o), HJGPU_EINVAL, idx, "d_b != NULL under another fn"); }
        for (uint32_t fn = 0; fn < 4; ++fn) {                           // every function on every index, with the d_b it asks for
            Call c = c0; c.aggs[a].fn = fn;
            Override ok = no_override(); ok.b[a] = fn == HJGPU_AGG_SUM_MUL ? ARENA + 50 * STRIDE : 0;
            expect(run(c, ok), HJGPU_OK, nullptr, "a legal function");
        }
    }
    { Override o = no_override(); o.b[1] = c0.p[A1]; expect(run(c0, o), HJGPU_OK, nullptr, "d_a == d_b"); }
    { Override o = no_override(); o.a[0] = o.a[2] = o.a[3] = c0.p[KEY0]; o.b[1] = c0.p[KEY0]; expect(run(c0, o), HJGPU_OK, nullptr, "one column in several aggregates and as a key"); }
    // the limits
    for (uint32_t k = 0; k <= 4; ++k) { Call c = c0; c.naggs = k; expect(run(c), HJGPU_OK, nullptr, "naggs 0 to 4"); }
    { Call c = c0; c.naggs = 5; expect(run(c), HJGPU_EINVAL, "naggs", "naggs 5"); c.n = 0; expect(run(c), HJGPU_EINVAL, "naggs", "naggs 5, n 0"); }
    { Call c = c0; c.naggs = 0; c.null_aggs = c.null_aggs_out = true; expect(run(c), HJGPU_OK, nullptr, "naggs 0 with NULL arrays"); }
    for (uint32_t k = 0; k <= 2; ++k) { Call c = c0; c.nkeys = k; expect(run(c), HJGPU_OK, nullptr, "nkeys 0 to 2"); }
    { Call c = c0; c.nkeys = 3; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 3"); c.n = 0; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 3, n 0"); }
    { Call c = c0; c.nkeys = 0; c.null_keys_in = c.null_keys_out = true; expect(run(c), HJGPU_OK, nullptr, "nkeys 0 with NULL key arrays"); }
    { Call c = c0; c.nkeys = 0; c.naggs = 0; c.null_keys_in = c.null_keys_out = c.null_aggs = c.null_aggs_out = true; c.p[COUNTS] = 0; expect(run(c), HJGPU_OK, nullptr, "nothing but the count"); }
    for (size_t cap : {(size_t)0, (size_t)1, (size_t)hj_group::MAX_CAPACITY}) { Call c = c0; c.capacity = cap; c.n = 0; expect(run(c), HJGPU_OK, nullptr, "a legal capacity"); }
    { Call c = c0; c.capacity = 0; expect(run(c), HJGPU_OK, nullptr, "capacity 0"); }
    { Call c = c0; c.capacity = (size_t)hj_group::MAX_CAPACITY + 1; expect(run(c), HJGPU_EINVAL, "capacity", "capacity beyond 2^40"); c.n = 0; expect(run(c), HJGPU_EINVAL, "capacity", "capacity beyond 2^40, n 0"); }
    // the host arrays and their entries
    { Call c = c0; c.null_keys_in = true; expect(run(c), HJGPU_EINVAL, "null", "d_keys_in NULL"); }
    { Call c = c0; c.null_keys_out = true; expect(run(c), HJGPU_EINVAL, "null", "d_keys_out NULL"); }
    { Call c = c0; c.null_aggs = true; expect(run(c), HJGPU_EINVAL, "null", "aggs NULL"); }
    { Call c = c0; c.null_aggs_out = true; expect(run(c), HJGPU_EINVAL, "null", "d_aggs_out NULL"); }
    for (int i : {KEY0, KEY1, KOUT0, KOUT1}) { Call c = c0; c.p[i] = 0; expect(run(c), HJGPU_EINVAL, "null key column", "a NULL key entry", NAME[i]); }
    for (int i : {OUT0, OUT1, OUT2, OUT3}) {
        Call c = c0; c.p[i] = 0;
        snprintf(idx, sizeof(idx), "aggregate %d:", i - OUT0);
        expect(run(c), HJGPU_EINVAL, idx, "a NULL d_aggs_out entry", NAME[i]);
    }
    { Call c = c0; c.p[COUNTS] = 0; expect(run(c), HJGPU_OK, nullptr, "d_counts_out NULL"); }
    { Call c = c0; c.p[BITS] = 0; expect(run(c), HJGPU_OK, nullptr, "d_select_bits NULL"); }
    { Call c = c0; c.p[NGROUPS] = 0; expect(run(c), HJGPU_EINVAL, "null group count", "the count pointer NULL"); c.n = 0; expect(run(c), HJGPU_EINVAL, "null group count", "the count pointer NULL, n 0"); }
    // n == 0: nothing but the count
    {
        Call c = c0; c.n = 0;
        for (int i = 0; i < NGROUPS; ++i) c.p[i] = 0;
        c.null_keys_in = c.null_keys_out = c.null_aggs = c.null_aggs_out = true;
        expect(run(c), HJGPU_OK, nullptr, "n = 0 with everything NULL");
        c.nkeys = 0; expect(run(c), HJGPU_OK, nullptr, "n = 0, nkeys = 0, everything NULL");
    }
    // every alignment
    for (int i = 0; i < NOPS; ++i) {
        for (uintptr_t d : {(uintptr_t)4, (uintptr_t)8, (uintptr_t)12, (uintptr_t)1}) {
            Call c = c0; c.p[i] += d;
            if (i == NGROUPS) {
                if (!device || d == 8) expect(run(c), HJGPU_OK, nullptr, "a count word that is aligned, or in host memory", NAME[i]);
                else expect(run(c), HJGPU_EALIGN, "d_ngroups", "a misaligned count word");
            } else expect(run(c), HJGPU_EALIGN, "16-byte aligned", "a misaligned operand", NAME[i]);
        }
    }
    // every overlap of a written operand with any other operand; a read operand onto a read operand is legal
    for (int w = 0; w < NOPS; ++w) {
        for (int j = 0; j < NOPS; ++j) {
            if (j == w) continue;
            const uintptr_t q = c0.p[j], theirs = bytes_of(c0, j), mine = bytes_of(c0, w);
            for (uintptr_t to : {q, q + 16, q + (theirs - 1) / 16 * 16, q - (mine - 1) / 16 * 16}) {
                if (theirs <= 16 && to == q + 16) continue;                 // (behind a count word: no overlap)
                Call c = c0; c.p[w] = to;
                // (the blocking form's count word is the caller's own, in host memory: it takes no part)
                const bool both_operands = device || (w != NGROUPS && j != NGROUPS);
                if (both_operands && (w >= KOUT0 || j >= KOUT0)) expect(run(c), HJGPU_EINVAL, "overlaps", NAME[w], NAME[j]);
                else expect(run(c), HJGPU_OK, nullptr, NAME[w], NAME[j]);
            }
        }
    }
    if (device) {                                                          // the count word inside an output, 8-byte aligned only
        for (int j = KOUT0; j <= COUNTS; ++j) { Call c = c0; c.p[NGROUPS] = c0.p[j] + 8; expect(run(c), HJGPU_EINVAL, "overlaps", "d_ngroups inside", NAME[j]); }
        for (int j = BITS; j <= B1; ++j) { Call c = c0; c.p[NGROUPS] = c0.p[j] + 8; expect(run(c), HJGPU_EINVAL, "overlaps", "d_ngroups inside", NAME[j]); }
    }
}

// agg_layout.hpp: the fold of any non-empty multiset of rows, from the initial word 0, is the definition's value
static void transform()
{
    using namespace hj_agg;
    const uint32_t edge[] = {0u, 1u, 2u, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu, 12345u, 0xA5A5A5A5u};
    const int E = sizeof(edge) / sizeof(edge[0]);
    for (uint32_t flags = 0; flags < 2; ++flags)
        for (int i = 0; i < E; ++i)
            for (int j = 0; j < E; ++j)
                for (int k = 0; k < E; ++k) {
                    const uint32_t x[3] = {edge[i], edge[j], edge[k]}, y[3] = {edge[k], edge[i], edge[j]};
                    for (int rows = 1; rows <= 3; ++rows) {
                        for (uint32_t fn = 0; fn < 4; ++fn) {
                            u64 word = 0;
                            for (int r = 0; r < rows; ++r) word = combine(fn, word, term(fn, flags, x[r], y[r]));
                            u64 want = 0;
                            if (fn == SUM) for (int r = 0; r < rows; ++r) want += flags ? (u64)(long long)(int32_t)x[r] : (u64)x[r];
                            else if (fn == SUM_MUL) for (int r = 0; r < rows; ++r) want += flags ? (u64)((long long)(int32_t)x[r] * (long long)(int32_t)y[r]) : (u64)x[r] * (u64)y[r];
                            else if (flags) {
                                int32_t e = (int32_t)x[0];
                                for (int r = 1; r < rows; ++r) e = fn == MIN ? ((int32_t)x[r] < e ? (int32_t)x[r] : e) : ((int32_t)x[r] > e ? (int32_t)x[r] : e);
                                want = (u64)(long long)e;
                            } else {
                                uint32_t e = x[0];
                                for (int r = 1; r < rows; ++r) e = fn == MIN ? (x[r] < e ? x[r] : e) : (x[r] > e ? x[r] : e);
                                want = e;
                            }
                            ++cases;
                            if (is_extreme(fn) && (word >> 32)) { printf("FAILED: an extreme's word is not zero-extended\n"); exit(1); }
                            if (result(fn, flags, word) != want) {
                                printf("FAILED transform fn %u flags %u rows %d (%08x %08x %08x): %llx, want %llx\n", fn, flags, rows, x[0], x[1], x[2], result(fn, flags, word), want);
                                exit(1);
                            }
                        }
                    }
                }
}

int main()
{
    static_assert(sizeof(hjgpu_aggregate) == 24 && offsetof(hjgpu_aggregate, d_a) == 8 && offsetof(hjgpu_aggregate, d_b) == 16, "hjgpu_aggregate's layout");
    static_assert(colop::MAX_OPERANDS >= NOPS + 3, "the operand table holds the call's 19 operands");
    checks(false);
    checks(true);
    transform();
    printf("ok: %ld cases\n", cases);
    return 0;
}
