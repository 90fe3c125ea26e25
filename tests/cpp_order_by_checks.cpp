// cpp_order_by_checks.cpp - csrc/colop_checks.hpp check_order_by, on the CPU.  Device pointers are fabricated integers in a fake arena -
// the check dereferences none; only the host arrays of keys and columns are real.  Both forms (blocking, device count): one valid call with
// four keys, eight carried columns, a mask and the row numbers, then every single deviation from it must give the stated status and text.
// Prints "ok: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>

#include "colop_checks.hpp"

static const uintptr_t ARENA = 0x40000000u, STRIDE = 0x100000u;      // every operand in a region of its own, far from its neighbours
static long cases = 0;

// the operands of the valid call, in the order of the check's table
enum { MASK, KEY0, IN0 = KEY0 + 4, OUT0 = IN0 + 8, ROWS = OUT0 + 8, COUNT, NOPS };

struct Call {
    uintptr_t p[NOPS];
    uint32_t key_flags[4], key_reserved[4], col_flags[8], col_reserved[8];
    size_t n, limit;
    uint32_t nkeys, ncols;
    bool null_keys, null_cols, null_count;
    bool device;
};

static Call base(bool device)
{
    Call c;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < NOPS; ++i) c.p[i] = ARENA + (uintptr_t)i * STRIDE;
    c.n = 1000; c.limit = 700; c.nkeys = 4; c.ncols = 8; c.device = device;
    // mixed widths, directions and signedness
    c.key_flags[0] = 0; c.key_flags[1] = HJGPU_ORDER_DESC | HJGPU_ORDER_WIDE; c.key_flags[2] = HJGPU_ORDER_SIGNED;
    c.key_flags[3] = HJGPU_ORDER_DESC | HJGPU_ORDER_SIGNED | HJGPU_ORDER_WIDE;
    for (int k = 0; k < 8; ++k) c.col_flags[k] = (k & 1) ? HJGPU_ORDER_WIDE : 0;
    return c;
}

static const char *name_of(int i)
{
    static char text[32];
    if (i == MASK) return "mask";
    if (i == ROWS) return "d_rows_out";
    if (i == COUNT) return "d_count";
    if (i < IN0) snprintf(text, sizeof(text), "key %d", i - KEY0);
    else if (i < OUT0) snprintf(text, sizeof(text), "input %d", i - IN0);
    else snprintf(text, sizeof(text), "output %d", i - OUT0);
    return text;
}

static bool is_written(int i) { return i >= OUT0; }
static bool exists(const Call &c, int i) { return c.device || i != COUNT; }       // (the blocking form's count is host memory: not an operand)

static size_t bytes_of(const Call &c, int i)
{
    const size_t m = c.limit < c.n ? c.limit : c.n;
    if (i == MASK) return (c.n + 31) / 32 * 4;
    if (i < IN0) return c.n * ((c.key_flags[i - KEY0] & HJGPU_ORDER_WIDE) ? 8 : 4);
    if (i < OUT0) return c.n * ((c.col_flags[i - IN0] & HJGPU_ORDER_WIDE) ? 8 : 4);
    if (i < ROWS) return m * ((c.col_flags[i - OUT0] & HJGPU_ORDER_WIDE) ? 8 : 4);
    if (i == ROWS) return m * 4;
    return 8;
}

static colop::Verdict run(const Call &c)
{
    hjgpu_order_key keys[5];
    hjgpu_order_column cols[9];
    for (int k = 0; k < 4; ++k) keys[k] = {(const void *)c.p[KEY0 + k], c.key_flags[k], c.key_reserved[k]};
    keys[4] = {nullptr, 0xFFu, 7u};                                               // behind nkeys: never looked at
    for (int k = 0; k < 8; ++k) cols[k] = {(const void *)c.p[IN0 + k], (void *)c.p[OUT0 + k], c.col_flags[k], c.col_reserved[k]};
    cols[8] = {nullptr, nullptr, 0xFFu, 7u};
    uint64_t host_count = 0;
    const uint64_t *count = c.null_count ? nullptr : c.device ? (const uint64_t *)c.p[COUNT] : &host_count;
    ++cases;
    return colop::check_order_by({(const uint32_t *)c.p[MASK], c.n, c.nkeys, c.null_keys ? nullptr : keys, c.ncols, c.null_cols ? nullptr : cols,
                                  (uint32_t *)c.p[ROWS], c.limit}, count, c.device);
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
    char index[32];
    expect(run(c0), HJGPU_OK, nullptr, "the valid call");
    // nkeys 1 to 4; 0 and 5 refused - also with no rows -, and 0 points to the compaction
    for (uint32_t k = 1; k <= 4; ++k) { Call c = c0; c.nkeys = k; expect(run(c), HJGPU_OK, nullptr, "nkeys 1 to 4"); }
    for (uint32_t k : {0u, 5u, 6u, 0xFFFFFFFFu}) {
        Call c = c0; c.nkeys = k; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 0, 5 and more");
        if (k == 0) expect(run(c), HJGPU_EINVAL, "hjgpu_compact_selected", "nkeys 0 names the compaction");
        c.n = 0; expect(run(c), HJGPU_EINVAL, "nkeys", "nkeys 0, 5 and more, n 0");
    }
    // ncols 0 to 8; 9 refused
    for (uint32_t k = 0; k <= 8; ++k) { Call c = c0; c.ncols = k; expect(run(c), HJGPU_OK, nullptr, "ncols 0 to 8"); }
    for (uint32_t k : {9u, 10u, 0xFFFFFFFFu}) {
        Call c = c0; c.ncols = k; expect(run(c), HJGPU_EINVAL, "ncols", "ncols 9 and more");
        c.n = 0; expect(run(c), HJGPU_EINVAL, "ncols", "ncols 9 and more, n 0");
    }
    { Call c = c0; c.ncols = 0; c.null_cols = true; expect(run(c), HJGPU_OK, nullptr, "no columns, a NULL column array"); }
    { Call c = c0; c.ncols = 0; c.null_cols = true; c.p[ROWS] = 0; expect(run(c), HJGPU_OK, nullptr, "the count alone"); }
    { Call c = c0; c.p[ROWS] = 0; expect(run(c), HJGPU_OK, nullptr, "no row numbers"); }
    { Call c = c0; c.p[MASK] = 0; expect(run(c), HJGPU_OK, nullptr, "a NULL mask selects every row"); }
    // each NULL: the arrays, the count, and the pointers among the first nkeys / ncols entries, by index
    { Call c = c0; c.null_keys = true; expect(run(c), HJGPU_EINVAL, "null key array", "a NULL key array"); }
    { Call c = c0; c.null_cols = true; expect(run(c), HJGPU_EINVAL, "null column array", "a NULL column array"); }
    { Call c = c0; c.null_count = true; expect(run(c), HJGPU_EINVAL, "null count pointer", "a NULL count"); c.n = 0; expect(run(c), HJGPU_EINVAL, "null count pointer", "a NULL count, n 0"); }
    for (uint32_t nk = 1; nk <= 4; ++nk)
        for (uint32_t e = 0; e < 4; ++e) {
            Call c = c0; c.nkeys = nk; c.p[KEY0 + e] = 0;
            snprintf(index, sizeof(index), "key %u: null d_col", e);
            expect(run(c), e < nk ? HJGPU_EINVAL : HJGPU_OK, e < nk ? index : nullptr, "a NULL key column");
        }
    for (uint32_t nc : {1u, 5u, 8u})
        for (uint32_t e = 0; e < 8; ++e) {
            Call c = c0; c.ncols = nc; c.p[IN0 + e] = 0;
            snprintf(index, sizeof(index), "column %u: null d_in", e);
            expect(run(c), e < nc ? HJGPU_EINVAL : HJGPU_OK, e < nc ? index : nullptr, "a NULL carried input");
            c = c0; c.ncols = nc; c.p[OUT0 + e] = 0;
            snprintf(index, sizeof(index), "column %u: null d_out", e);
            expect(run(c), e < nc ? HJGPU_EINVAL : HJGPU_OK, e < nc ? index : nullptr, "a NULL output");
        }
    // each flag: every defined combination accepted, every bit outside refused by index; reserved
    for (uint32_t e = 0; e < 4; ++e) {
        for (uint32_t f = 0; f < 8; ++f) { Call c = c0; c.key_flags[e] = f; expect(run(c), HJGPU_OK, nullptr, "every defined key flag"); }
        for (uint32_t bit = 3; bit < 32; ++bit) {
            Call c = c0; c.key_flags[e] |= 1u << bit;
            snprintf(index, sizeof(index), "key %u: unknown flag", e);
            expect(run(c), HJGPU_EINVAL, index, "an undefined key flag");
        }
        Call c = c0; c.key_reserved[e] = 1;
        snprintf(index, sizeof(index), "key %u: the reserved", e);
        expect(run(c), HJGPU_EINVAL, index, "a key's reserved word");
    }
    for (uint32_t e = 0; e < 8; ++e) {
        for (uint32_t f : {0u, (uint32_t)HJGPU_ORDER_WIDE}) { Call c = c0; c.col_flags[e] = f; expect(run(c), HJGPU_OK, nullptr, "every defined column flag"); }
        for (uint32_t bit = 0; bit < 32; ++bit) {
            if ((1u << bit) == HJGPU_ORDER_WIDE) continue;
            Call c = c0; c.col_flags[e] |= 1u << bit;
            snprintf(index, sizeof(index), "column %u: unknown flag", e);
            expect(run(c), HJGPU_EINVAL, index, "an undefined column flag");
        }
        Call c = c0; c.col_reserved[e] = 0x80000000u;
        snprintf(index, sizeof(index), "column %u: the reserved", e);
        expect(run(c), HJGPU_EINVAL, index, "a column's reserved word");
    }
    // n: a row number is a uint32
    // (columns of that many rows reach across the arena: what is written lies in front of it)
    { Call c = c0; c.n = 0xFFFFFFFFull; c.limit = 10; c.ncols = 0; c.p[ROWS] = 0x10000; c.p[COUNT] = 0x20000; expect(run(c), HJGPU_OK, nullptr, "n 0xFFFFFFFF"); }
    for (size_t n : {(size_t)0x100000000ull, (size_t)0x100000001ull, (size_t)1 << 40}) {
        Call c = c0; c.n = n; expect(run(c), HJGPU_EINVAL, "0xFFFFFFFF", "n beyond 0xFFFFFFFF");
        c.p[ROWS] = 0; c.ncols = 0; expect(run(c), HJGPU_EINVAL, "0xFFFFFFFF", "n beyond 0xFFFFFFFF, the count alone");
    }
    // limit: anything
    for (size_t limit : {(size_t)0, (size_t)1, (size_t)999, (size_t)1000, (size_t)1001, ~(size_t)0}) { Call c = c0; c.limit = limit; expect(run(c), HJGPU_OK, nullptr, "any limit"); }
    // every alignment
    for (int i = 0; i < NOPS; ++i) {
        if (!exists(c0, i)) continue;
        for (uintptr_t off : {4u, 8u, 12u}) {
            if (i == COUNT && off == 8) continue;                                 // (the count word is 8-byte aligned)
            Call c = c0; c.p[i] += off;
            expect(run(c), HJGPU_EALIGN, i == COUNT ? "8-byte aligned" : "16-byte aligned", "a misaligned operand", name_of(i));
        }
    }
    if (device) { Call c = c0; c.p[COUNT] += 8; expect(run(c), HJGPU_OK, nullptr, "a count word at 8 modulo 16"); }
    if (device) { Call c = c0; c.p[COUNT] += 4; c.n = 0; expect(run(c), HJGPU_EALIGN, "d_count", "a misaligned d_count at n 0"); }
    { Call c = c0; c.limit = 0; c.p[OUT0] += 4; expect(run(c), HJGPU_EALIGN, "16-byte aligned", "a misaligned output under limit 0"); }
    // every overlap of a written operand with every other operand: the very pointer, its first bytes, its last bytes
    for (int w = 0; w < NOPS; ++w) {
        if (!is_written(w) || !exists(c0, w)) continue;
        for (int o = 0; o < NOPS; ++o) {
            if (o == w || !exists(c0, o)) continue;
            for (int how = 0; how < 3; ++how) {
                Call c = c0;
                const uintptr_t grain = (w == COUNT || o == COUNT) ? 7 : 15;
                if (how == 0) c.p[w] = c.p[o];                                                    // the very pointer
                else if (how == 1) c.p[w] = c.p[o] + ((bytes_of(c, o) - 1) & ~grain);             // w begins inside o's last vector
                else c.p[w] = c.p[o] - ((bytes_of(c, w) - 1) & ~grain);                           // w ends inside o's first vector
                if (how != 0 && bytes_of(c, w) <= 8 && bytes_of(c, o) <= 8) continue;
                if (c.p[w] & (w == COUNT ? 7 : 15)) continue;                                     // (an alignment case, above)
                expect(run(c), HJGPU_EINVAL, "overlaps", name_of(w), name_of(o));
            }
        }
    }
    // the overlap check covers the first min(limit, n) elements of an output: an output that ends in front of a read operand is fine,
    // however long the column it was cut from
    {
        Call c = c0; c.limit = 16;
        c.p[OUT0] = c.p[MASK] - 64; expect(run(c), HJGPU_OK, nullptr, "16 rows of an output in front of the mask");
        c.limit = 17; expect(run(c), HJGPU_EINVAL, "overlaps", "17 rows of an output reach the mask");
        c = c0; c.limit = 0; c.p[ROWS] = c.p[KEY0]; expect(run(c), HJGPU_OK, nullptr, "limit 0: no output byte");
        c = c0; c.limit = ~(size_t)0; c.p[ROWS] = c.p[MASK] - 4000; expect(run(c), HJGPU_OK, nullptr, "limit beyond n counts as n");
        c.p[ROWS] = c.p[MASK] - 3984; expect(run(c), HJGPU_EINVAL, "overlaps", "limit beyond n counts as n, one vector further");
    }
    // a key column may be carried, and the same column may appear several times
    { Call c = c0; c.p[IN0] = c.p[KEY0]; c.p[IN0 + 2] = c.p[KEY0]; c.p[KEY0 + 2] = c.p[KEY0]; c.p[IN0 + 4] = c.p[IN0 + 6]; expect(run(c), HJGPU_OK, nullptr, "shared read operands"); }
    // n == 0: NULL everywhere else
    {
        Call c = c0; c.n = 0;
        expect(run(c), HJGPU_OK, nullptr, "n 0");
        for (int i = 0; i < NOPS; ++i) if (i != COUNT) c.p[i] = 0;
        c.null_keys = c.null_cols = true;
        expect(run(c), HJGPU_OK, nullptr, "n 0 with NULL everywhere");
        for (int k = 0; k < 4; ++k) c.key_flags[k] = 0xFFFFFFFFu;
        expect(run(c), HJGPU_OK, nullptr, "n 0: nothing is looked at");
    }
}

int main()
{
    checks(false);
    checks(true);
    printf("ok: %ld cases\n", cases);
    return 0;
}
