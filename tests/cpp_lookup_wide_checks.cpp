// cpp_lookup_wide_checks.cpp - csrc/colop_checks.hpp check_lookup_wide, on the CPU.  Device pointers are fabricated integers in a fake arena -
// the check dereferences none; only the host arrays of pointers are real.  Both forms (blocking, device result): one valid call with four
// keys, a mask and both outputs, then every single deviation from it must give the stated status and text.  Prints "ok: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>

#include "colop_checks.hpp"

static const uintptr_t ARENA = 0x40000000u, STRIDE = 0x10000u;       // every operand in a region of its own, far from its neighbours
static long cases = 0;

// the operands of the valid call, in the order of the check's table
enum { MASK, SK0, SK1, SK2, SK3, RK0, RK1, RK2, RK3, RV, VALS, BITS, RESULT, NOPS };
static const char *const NAME[NOPS] = {"mask", "probe key 0", "probe key 1", "probe key 2", "probe key 3", "build key 0", "build key 1", "build key 2",
                                       "build key 3", "payloads", "d_vals_out", "d_match_bits", "d_result"};

struct Call {
    uintptr_t p[NOPS];
    size_t inner, outer;
    uint32_t nkeys;
    bool null_inner_keys, null_outer_keys, has_params;
    hjgpu_npj_params params;
    bool device;
};

static Call base(bool device)
{
    Call c;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < NOPS; ++i) c.p[i] = ARENA + (uintptr_t)i * STRIDE;
    c.inner = 900; c.outer = 1000; c.nkeys = 4; c.device = device;
    return c;
}

static bool is_written(int i) { return i >= VALS; }
static bool exists(const Call &c, int i) { return c.device || i != RESULT; }      // (the blocking form's result is host memory: not an operand)

static size_t bytes_of(const Call &c, int i)
{
    if (i == MASK || i == BITS) return (c.outer + 31) / 32 * 4;
    if (i <= SK3 || i == VALS) return c.outer * 4;
    if (i <= RV) return c.inner * 4;
    return 32;
}

static colop::Verdict run(const Call &c)
{
    const uint32_t *outer_keys[5] = {(const uint32_t *)c.p[SK0], (const uint32_t *)c.p[SK1], (const uint32_t *)c.p[SK2], (const uint32_t *)c.p[SK3],
                                     (const uint32_t *)(ARENA + 40 * STRIDE)};
    const uint32_t *inner_keys[5] = {(const uint32_t *)c.p[RK0], (const uint32_t *)c.p[RK1], (const uint32_t *)c.p[RK2], (const uint32_t *)c.p[RK3],
                                     (const uint32_t *)(ARENA + 41 * STRIDE)};
    ++cases;
    return colop::check_lookup_wide({c.nkeys, c.null_inner_keys ? nullptr : inner_keys, (const uint32_t *)c.p[RV], c.inner, c.null_outer_keys ? nullptr : outer_keys,
                                     c.outer, c.has_params ? &c.params : nullptr, (const uint32_t *)c.p[MASK], (uint32_t *)c.p[VALS], (uint32_t *)c.p[BITS]},
                                    c.device ? (const hjgpu_result *)c.p[RESULT] : nullptr);
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
    // nkeys: 2, 3 and 4; 0, 1 and 5 refused - also with empty sides -, and 1 points to the one-column look-up
    for (uint32_t k = 2; k <= 4; ++k) { Call c = c0; c.nkeys = k; expect(run(c), HJGPU_OK, nullptr, "nkeys 2 to 4"); }
    for (uint32_t k : {0u, 1u, 5u, 6u, 0xFFFFFFFFu}) {
        Call c = c0; c.nkeys = k; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 0, 1, 5 and more");
        if (k == 1) expect(run(c), HJGPU_EINVAL, "hjgpu_lookup_selected", "nkeys 1 names the one-column look-up");
        c.outer = 0; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 0, 1, 5 and more, outer 0");
        c = c0; c.nkeys = k; c.inner = 0; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 0, 1, 5 and more, inner 0");
    }
    // only the first nkeys entries of a key array are looked at
    for (uint32_t k = 2; k <= 4; ++k) {
        for (uint32_t e = 0; e < 4; ++e) {
            Call c = c0; c.nkeys = k; c.p[SK0 + e] = 0;
            expect(run(c), e < k ? HJGPU_EINVAL : HJGPU_OK, e < k ? "null key column pointer" : nullptr, "a NULL probe key column");
            c = c0; c.nkeys = k; c.p[RK0 + e] = 0;
            expect(run(c), e < k ? HJGPU_EINVAL : HJGPU_OK, e < k ? "null key column pointer" : nullptr, "a NULL build key column");
        }
    }
    { Call c = c0; c.null_inner_keys = true; expect(run(c), HJGPU_EINVAL, "null key column array", "a NULL build key array"); }
    { Call c = c0; c.null_outer_keys = true; expect(run(c), HJGPU_EINVAL, "null key column array", "a NULL probe key array"); }
    { Call c = c0; c.p[RV] = 0; expect(run(c), HJGPU_EINVAL, "d_inner_vals", "a NULL payload column with inner > 0"); }
    // the optional operands
    for (int i : {MASK, VALS, BITS, RESULT}) { Call c = c0; c.p[i] = 0; expect(run(c), HJGPU_OK, nullptr, "an absent optional operand", NAME[i]); }
    { Call c = c0; c.p[MASK] = c.p[VALS] = c.p[BITS] = c.p[RESULT] = 0; expect(run(c), HJGPU_OK, nullptr, "no optional operand at all"); }
    // the same column twice, on either side
    { Call c = c0; c.p[SK1] = c.p[SK0]; c.p[RK3] = c.p[RK2]; expect(run(c), HJGPU_OK, nullptr, "the same key column twice"); }
    // params: the load, and nothing else (the join-mode flags are refused by the entry point, by name)
    for (double load : {0.0, 0.05, 0.5, 0.99}) { Call c = c0; c.has_params = true; c.params.load = load; expect(run(c), HJGPU_OK, nullptr, "a legal load"); }
    for (double load : {0.991, 1.0, 4.0, -0.5}) {
        Call c = c0; c.has_params = true; c.params.load = load; expect(run(c), HJGPU_EINVAL, "load", "load beyond 0.99 or negative");
        c.outer = 0; expect(run(c), HJGPU_EINVAL, "load", "load beyond 0.99 or negative, outer 0");
    }
    { Call c = c0; c.has_params = true; c.params.factor = 12; c.params.flags = HJGPU_FLAG_UNIQUE; expect(run(c), HJGPU_OK, nullptr, "factor and HJGPU_FLAG_UNIQUE are ignored"); }
    // every alignment
    for (int i = 0; i < NOPS; ++i) {
        if (!exists(c0, i)) continue;
        for (uintptr_t off : {4u, 8u, 12u}) {
            Call c = c0; c.p[i] += off;
            expect(run(c), HJGPU_EALIGN, "16-byte aligned", "a misaligned operand", NAME[i]);
        }
    }
    if (device) { Call c = c0; c.p[RESULT] += 8; c.outer = 0; expect(run(c), HJGPU_EALIGN, "d_result", "a misaligned d_result at outer 0"); }
    // every overlap of a written operand with every other operand: its first bytes, its last bytes, and the very pointer
    for (int w = 0; w < NOPS; ++w) {
        if (!is_written(w) || !exists(c0, w)) continue;
        for (int o = 0; o < NOPS; ++o) {
            if (o == w || !exists(c0, o)) continue;
            const bool pair = (w == BITS && o == MASK);
            for (int how = 0; how < 3; ++how) {
                Call c = c0;
                if (how == 0) c.p[w] = c.p[o];                                                    // the very pointer
                else if (how == 1) c.p[w] = c.p[o] + ((bytes_of(c, o) - 1) & ~(uintptr_t)15);     // w begins inside o's last vector
                else c.p[w] = c.p[o] - ((bytes_of(c, w) - 1) & ~(uintptr_t)15);                   // w ends inside o's first vector
                if (how != 0 && bytes_of(c, w) <= 16 && bytes_of(c, o) <= 16) continue;
                if (pair && how == 0) expect(run(c), HJGPU_OK, nullptr, "d_match_bits on d_select_bits (in place)");
                else expect(run(c), HJGPU_EINVAL, "overlaps", NAME[w], NAME[o]);
                if (pair && how != 0) expect(run(c), HJGPU_EINVAL, "in place", "any other overlap of the two bitmaps");
            }
        }
    }
    // a mask given as d_match_bits while another mask is read: no in-place pair with a NULL mask, and none needed
    { Call c = c0; c.p[MASK] = 0; expect(run(c), HJGPU_OK, nullptr, "match bits without a mask"); }
    // the empty sides: NULL wherever nothing is read
    {
        Call c = c0; c.outer = 0;
        expect(run(c), HJGPU_OK, nullptr, "outer 0");
        for (int i = 0; i < NOPS; ++i) c.p[i] = 0;
        c.null_inner_keys = c.null_outer_keys = true;
        expect(run(c), HJGPU_OK, nullptr, "outer 0 with NULL everywhere");
        c.inner = 0; expect(run(c), HJGPU_OK, nullptr, "both sides empty with NULL everywhere");
    }
    {
        Call c = c0; c.inner = 0;
        expect(run(c), HJGPU_OK, nullptr, "inner 0");
        c.null_inner_keys = c.null_outer_keys = true; c.p[RV] = 0;
        for (int i = SK0; i <= RK3; ++i) c.p[i] = 0;
        expect(run(c), HJGPU_OK, nullptr, "inner 0 with NULL key arrays and payloads");
        // ... and the outputs of an empty build side are still written: their rules hold
        c.p[VALS] += 4; expect(run(c), HJGPU_EALIGN, "d_vals_out", "inner 0, a misaligned output");
        c = c0; c.inner = 0; c.p[VALS] = c.p[MASK]; expect(run(c), HJGPU_EINVAL, "overlaps", "inner 0, d_vals_out on the mask");
        c = c0; c.inner = 0; c.p[BITS] = c.p[MASK]; expect(run(c), HJGPU_OK, nullptr, "inner 0, in place");
    }
}

int main()
{
    checks(false);
    checks(true);
    printf("ok: %ld cases\n", cases);
    return 0;
}
