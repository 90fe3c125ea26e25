// cpp_group_by_checks.cpp - csrc/colop_checks.hpp check_group_by, on the CPU: check_group_agg's rules with up to four key inputs and four key
// outputs.  Device pointers are fabricated integers in a fake arena - the check dereferences none; only the host arrays of pointers and
// aggregates are real.  Both forms (blocking, device count): one valid call with four keys and four aggregates, then every single deviation
// from it must give the stated status and text.  Prints "ok: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>

#include "colop_checks.hpp"

static const uintptr_t ARENA = 0x40000000u, STRIDE = 0x10000u;       // every operand in a region of its own, far from its neighbours
static long cases = 0;

// the operands of the valid call, in the order of the check's table
enum { BITS, KEY0, KEY1, KEY2, KEY3, A0, A1, A2, A3, B1, KOUT0, KOUT1, KOUT2, KOUT3, OUT0, OUT1, OUT2, OUT3, COUNTS, NGROUPS, NOPS };
static const char *const NAME[NOPS] = {"mask", "key 0", "key 1", "key 2", "key 3", "a 0", "a 1", "a 2", "a 3", "b 1", "key out 0", "key out 1", "key out 2", "key out 3",
                                       "out 0", "out 1", "out 2", "out 3", "counts", "d_ngroups"};

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
    c.n = 1000; c.capacity = 1000; c.nkeys = 4; c.naggs = 4; c.device = device;
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
    if (i <= KOUT3) return c.capacity * 4;
    if (i <= COUNTS) return c.capacity * 8;
    return 8;
}

static colop::Verdict run(const Call &c, uintptr_t b_of_0 = 0)
{
    const uint32_t *keys_in[5] = {(const uint32_t *)c.p[KEY0], (const uint32_t *)c.p[KEY1], (const uint32_t *)c.p[KEY2], (const uint32_t *)c.p[KEY3],
                                  (const uint32_t *)(ARENA + 40 * STRIDE)};
    uint32_t *keys_out[5] = {(uint32_t *)c.p[KOUT0], (uint32_t *)c.p[KOUT1], (uint32_t *)c.p[KOUT2], (uint32_t *)c.p[KOUT3], (uint32_t *)(ARENA + 41 * STRIDE)};
    uint64_t *aggs_out[5] = {(uint64_t *)c.p[OUT0], (uint64_t *)c.p[OUT1], (uint64_t *)c.p[OUT2], (uint64_t *)c.p[OUT3], (uint64_t *)(ARENA + 42 * STRIDE)};
    hjgpu_aggregate aggs[5];
    for (int i = 0; i < 5; ++i) {
        aggs[i] = c.aggs[i];
        aggs[i].d_a = (const uint32_t *)(i < 4 ? c.p[A0 + i] : ARENA + 43 * STRIDE);
        aggs[i].d_b = i == 1 ? (const uint32_t *)c.p[B1] : i == 0 ? (const uint32_t *)b_of_0 : nullptr;
    }
    ++cases;
    return colop::check_group_by({(const uint32_t *)c.p[BITS], c.n, c.nkeys, c.naggs, c.null_keys_in ? nullptr : keys_in, c.null_aggs ? nullptr : aggs,
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
    // the limits: nkeys 0 to 4, five refused - also at n == 0
    for (uint32_t k = 0; k <= 4; ++k) {
        Call c = c0; c.nkeys = k; expect(run(c), HJGPU_OK, nullptr, "nkeys 0 to 4");
        c.n = 0; expect(run(c), HJGPU_OK, nullptr, "nkeys 0 to 4, n 0");
    }
    for (uint32_t k : {5u, 6u, 0xFFFFFFFFu}) {
        Call c = c0; c.nkeys = k; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 5 and more");
        c.n = 0; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 5 and more, n 0");
    }
    { Call c = c0; c.nkeys = 0; c.null_keys_in = c.null_keys_out = true; expect(run(c), HJGPU_OK, nullptr, "nkeys 0 with NULL key arrays"); }
    for (uint32_t k = 0; k <= 4; ++k) { Call c = c0; c.naggs = k; expect(run(c), HJGPU_OK, nullptr, "naggs 0 to 4"); }
    { Call c = c0; c.naggs = 5; expect(run(c), HJGPU_EINVAL, "naggs", "naggs 5"); c.n = 0; expect(run(c), HJGPU_EINVAL, "naggs", "naggs 5, n 0"); }
    for (size_t cap : {(size_t)0, (size_t)1, (size_t)hj_wide::MAX_CAPACITY}) { Call c = c0; c.capacity = cap; c.n = 0; expect(run(c), HJGPU_OK, nullptr, "a legal capacity"); }
    { Call c = c0; c.capacity = 0; expect(run(c), HJGPU_OK, nullptr, "capacity 0"); }
    { Call c = c0; c.capacity = (size_t)hj_wide::MAX_CAPACITY + 1; expect(run(c), HJGPU_EINVAL, "capacity", "capacity beyond 2^40"); c.n = 0; expect(run(c), HJGPU_EINVAL, "capacity", "capacity beyond 2^40, n 0"); }
    // the aggregates' refusals carry the aggregate's index, as hjgpu_group_agg's do
    for (uint32_t a = 0; a < 4; ++a) {
        char idx[32];
        snprintf(idx, sizeof(idx), "aggregate %u:", a);
        { Call c = c0; c.aggs[a].fn = 4; expect(run(c), HJGPU_EINVAL, idx, "fn > 3"); }
        { Call c = c0; c.aggs[a].flags = 2; expect(run(c), HJGPU_EINVAL, idx, "an unknown flag"); }
    }
    expect(run(c0, ARENA + 50 * STRIDE), HJGPU_EINVAL, "aggregate 0:", "d_b != NULL under SUM");
    // the host arrays and their entries: a NULL entry among the first nkeys of either key array, for every nkeys
    { Call c = c0; c.null_keys_in = true; expect(run(c), HJGPU_EINVAL, "null", "d_keys_in NULL"); }
    { Call c = c0; c.null_keys_out = true; expect(run(c), HJGPU_EINVAL, "null", "d_keys_out NULL"); }
    { Call c = c0; c.null_aggs = true; expect(run(c), HJGPU_EINVAL, "null", "aggs NULL"); }
    { Call c = c0; c.null_aggs_out = true; expect(run(c), HJGPU_EINVAL, "null", "d_aggs_out NULL"); }
    for (uint32_t k = 1; k <= 4; ++k)
        for (int side : {KEY0, KOUT0})
            for (uint32_t e = 0; e < 4; ++e) {
                Call c = c0; c.nkeys = k; c.p[side + e] = 0;
                if (e < k) expect(run(c), HJGPU_EINVAL, "null key column", "a NULL key entry", NAME[side + e]);
                else expect(run(c), HJGPU_OK, nullptr, "a NULL entry behind the first nkeys", NAME[side + e]);
            }
    for (int i : {OUT0, OUT1, OUT2, OUT3}) {
        char idx[32];
        Call c = c0; c.p[i] = 0;
        snprintf(idx, sizeof(idx), "aggregate %d:", i - OUT0);
        expect(run(c), HJGPU_EINVAL, idx, "a NULL d_aggs_out entry", NAME[i]);
    }
    { Call c = c0; c.p[COUNTS] = 0; expect(run(c), HJGPU_OK, nullptr, "d_counts_out NULL"); }
    { Call c = c0; c.p[BITS] = 0; expect(run(c), HJGPU_OK, nullptr, "d_select_bits NULL"); }
    { Call c = c0; c.p[NGROUPS] = 0; expect(run(c), HJGPU_EINVAL, "null group count", "the count pointer NULL"); c.n = 0; expect(run(c), HJGPU_EINVAL, "null group count", "the count pointer NULL, n 0"); }
    // n == 0: nothing but the count
    for (uint32_t k = 0; k <= 4; ++k) {
        Call c = c0; c.n = 0; c.nkeys = k;
        for (int i = 0; i < NGROUPS; ++i) c.p[i] = 0;
        c.null_keys_in = c.null_keys_out = c.null_aggs = c.null_aggs_out = true;
        expect(run(c), HJGPU_OK, nullptr, "n = 0 with everything NULL");
    }
    // the same key column more than once
    { Call c = c0; c.p[KEY1] = c.p[KEY2] = c.p[KEY3] = c.p[KEY0]; expect(run(c), HJGPU_OK, nullptr, "one key column four times"); }
    { Call c = c0; c.p[A0] = c.p[A2] = c.p[KEY3]; expect(run(c), HJGPU_OK, nullptr, "a key column as an aggregate's column"); }
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
    // with three keys the fourth pair of key pointers takes no part
    { Call c = c0; c.nkeys = 3; c.p[KOUT3] = c0.p[BITS]; c.p[KEY3] = c0.p[OUT0]; expect(run(c), HJGPU_OK, nullptr, "the fourth key pointers of a three-key call"); }
    if (device) {                                                          // the _async form's count word inside an operand, 8-byte aligned only
        for (int j = KOUT0; j <= COUNTS; ++j) { Call c = c0; c.p[NGROUPS] = c0.p[j] + 8; expect(run(c), HJGPU_EINVAL, "overlaps", "d_ngroups inside", NAME[j]); }
        for (int j = BITS; j <= B1; ++j) { Call c = c0; c.p[NGROUPS] = c0.p[j] + 8; expect(run(c), HJGPU_EINVAL, "overlaps", "d_ngroups inside", NAME[j]); }
    }
}

int main()
{
    static_assert(HJGPU_GROUP_BY_MAX_KEYS == 4 && HJGPU_GROUP_MAX_KEYS == 2, "the two limits");
    static_assert(colop::MAX_OPERANDS == 23 && colop::MAX_OPERANDS >= NOPS + 3, "the operand table holds the call's 23 operands");
    checks(false);
    checks(true);
    // hjgpu_group_agg's own limit stays where it was
    {
        const uint32_t *keys_in[3] = {(const uint32_t *)ARENA, (const uint32_t *)(ARENA + STRIDE), (const uint32_t *)(ARENA + 2 * STRIDE)};
        uint32_t *keys_out[3] = {(uint32_t *)(ARENA + 3 * STRIDE), (uint32_t *)(ARENA + 4 * STRIDE), (uint32_t *)(ARENA + 5 * STRIDE)};
        uint64_t count = 0;
        const colop::GroupAggCall g = {nullptr, 1000, 3, 0, keys_in, nullptr, keys_out, nullptr, nullptr, 1000};
        expect(colop::check_group_agg(g, &count, false), HJGPU_EINVAL, "HJGPU_GROUP_MAX_KEYS (2)", "check_group_agg with three keys");
        expect(colop::check_group_by(g, &count, false), HJGPU_OK, nullptr, "check_group_by with three keys");
        cases += 2;
    }
    printf("ok: %ld cases\n", cases);
    return 0;
}
