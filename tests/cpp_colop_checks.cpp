// cpp_colop_checks.cpp - csrc/colop_checks.hpp against the hand-written checkers it replaced (cpp_colop_checks_parent.hpp), on the CPU.
// Device pointers are fabricated integers in a fake arena - neither version dereferences one; only the host arrays of pointers and predicates
// are real.  For every operator, both forms (blocking, device count) and the largest and the smallest legal shape: a valid base call, every
// single deviation from it (same status, "overlaps" in the new text exactly when it is in the old one), every pair of deviations on two
// different operands (same accept / refuse decision), and the legal in-place calls (accepted; moved by one vector, refused).
// Prints "ok: N cases"; fails if an operand of an operator was never moved, or never moved onto.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "colop_checks.hpp"
#include "cpp_colop_checks_parent.hpp"

enum Op { COMPACT, GROUP, FILTER, GATHER, LOOKUP, OPS };
// an operand's part in its call: the mask, the index column, the columns read (A: inputs / keys / predicate columns / sources, B: measures),
// the columns written (A: outputs / key outputs, B: sums), the one further output (row numbers / group counts / the bitmap), the count word(s)
enum Role { BITS, IDX, IN_A, IN_B, OUT_A, OUT_B, EXTRA, COUNT, ROLES };
static const char *const OP_NAME[OPS] = {"compact", "group", "filter", "gather", "lookup"};
static const char *const ROLE_NAME[ROLES] = {"mask", "index", "input A", "input B", "output A", "output B", "further output", "count"};
static const uint32_t MAX_A[OPS] = {HJGPU_COMPACT_MAX_COLS, HJGPU_GROUP_MAX_KEYS, HJGPU_FILTER_MAX_PREDS, HJGPU_GATHER_MAX_COLS, 0};
static const uint32_t MAX_B[OPS] = {0, HJGPU_GROUP_MAX_VALS, 0, 0, 0};

static const uintptr_t ARENA = 0x40000000u, STRIDE = 0x10000u;       // every operand in a region of its own, far from its neighbours
static const int MAX_LIST = 9;                                       // entries of a host array: the largest limit + 1

struct Operand { Role role; uintptr_t p; };
struct State {
    Op op;
    bool device;
    size_t n, capacity, src_rows;
    uint32_t na, nb;                        // the counts the call states
    int nv;
    Operand v[24];
    bool null_list[4];                      // a host array passed as NULL: inputs A, inputs B, outputs A, outputs B
    bool null_preds;
    hjgpu_predicate preds[MAX_LIST];
};

static size_t bytes_of(const State &s, Role r)
{
    const size_t mask = (s.n + 31) / 32 * 4;
    switch (r) {
    case BITS: return mask;
    case IDX: return s.n * 4;
    case IN_A: return (s.op == GATHER ? s.src_rows : s.n) * 4;
    case IN_B: return s.n * 4;
    case OUT_A: return (s.op == GATHER ? s.n : s.capacity) * 4;
    case OUT_B: return s.capacity * 8;
    case EXTRA: return s.op == COMPACT ? s.capacity * 4 : s.op == GROUP ? s.capacity * 8 : mask;
    default: return s.op == GATHER ? 16 : 8;
    }
}

static State base(Op op, bool device, uint32_t a, uint32_t b)
{
    State s;
    memset(&s, 0, sizeof(s));
    s.op = op; s.device = device; s.n = 1000; s.capacity = 1000; s.src_rows = 2000; s.na = a; s.nb = b;
    auto add = [&](Role r, uint32_t k) { for (uint32_t i = 0; i < k; ++i) { s.v[s.nv] = {r, ARENA + (uintptr_t)s.nv * STRIDE}; ++s.nv; } };
    add(BITS, 1);
    if (op == GATHER) add(IDX, 1);
    if (op != LOOKUP) { add(IN_A, a); add(IN_B, b); }
    if (op != FILTER && op != LOOKUP) { add(OUT_A, a); add(OUT_B, b); }
    add(EXTRA, 1);
    if (op != LOOKUP && !(op == GATHER && !device)) add(COUNT, 1);       // (the blocking gather passes no count operand)
    for (int p = 0; p < MAX_LIST; ++p) s.preds[p] = {1u + p, 7u + p, (uint32_t)p & 3u, 0u};
    return s;
}

struct Decision { int status; bool overlaps; };

// the host arrays of a call: the state's operands first, then spare valid columns up to the largest count a deviation states
struct Lists {
    const uint32_t *in_a[MAX_LIST], *in_b[MAX_LIST];
    uint32_t *out_a[MAX_LIST];
    uint64_t *out_b[MAX_LIST];
    const uint32_t *bits, *idx;
    void *extra, *count;
    explicit Lists(const State &s)
    {
        int n[ROLES] = {0};
        bits = idx = nullptr; extra = count = nullptr;
        for (int i = 0; i < s.nv; ++i) {
            const uintptr_t p = s.v[i].p;
            switch (s.v[i].role) {
            case BITS: bits = (const uint32_t *)p; break;
            case IDX: idx = (const uint32_t *)p; break;
            case IN_A: in_a[n[IN_A]++] = (const uint32_t *)p; break;
            case IN_B: in_b[n[IN_B]++] = (const uint32_t *)p; break;
            case OUT_A: out_a[n[OUT_A]++] = (uint32_t *)p; break;
            case OUT_B: out_b[n[OUT_B]++] = (uint64_t *)p; break;
            case EXTRA: extra = (void *)p; break;
            default: count = (void *)p; break;
            }
        }
        uintptr_t spare = ARENA + 64 * STRIDE;
        for (int i = n[IN_A]; i < MAX_LIST; ++i, spare += STRIDE) in_a[i] = (const uint32_t *)spare;
        for (int i = n[IN_B]; i < MAX_LIST; ++i, spare += STRIDE) in_b[i] = (const uint32_t *)spare;
        for (int i = n[OUT_A]; i < MAX_LIST; ++i, spare += STRIDE) out_a[i] = (uint32_t *)spare;
        for (int i = n[OUT_B]; i < MAX_LIST; ++i, spare += STRIDE) out_b[i] = (uint64_t *)spare;
    }
};

static void both(const State &s, Decision *was, Decision *is)
{
    const Lists l(s);
    const uint32_t *const *in_a = s.null_list[0] ? nullptr : l.in_a, *const *in_b = s.null_list[1] ? nullptr : l.in_b;
    uint32_t *const *out_a = s.null_list[2] ? nullptr : l.out_a;
    uint64_t *const *out_b = s.null_list[3] ? nullptr : l.out_b;
    const uint64_t *count = (const uint64_t *)l.count;
    parent::Verdict o = parent::OK;
    colop::Verdict v = colop::no_objection();
    switch (s.op) {
    case COMPACT:
        o = parent::check_compact(l.bits, s.n, s.na, in_a, out_a, (const uint32_t *)l.extra, s.capacity, count, s.device);
        v = colop::check_compact({l.bits, s.n, s.na, in_a, out_a, (uint32_t *)l.extra, s.capacity}, count, s.device);
        break;
    case GROUP:
        o = parent::check_group({l.bits, s.n, s.na, s.nb, in_a, in_b, out_a, (uint64_t *)l.extra, out_b, s.capacity}, count, s.device);
        v = colop::check_group({l.bits, s.n, s.na, s.nb, in_a, in_b, out_a, (uint64_t *)l.extra, out_b, s.capacity}, count, s.device);
        break;
    case FILTER:
        o = parent::check_filter({l.bits, s.n, s.na, in_a, s.null_preds ? nullptr : s.preds, (uint32_t *)l.extra}, count, s.device);
        v = colop::check_filter({l.bits, s.n, s.na, in_a, s.null_preds ? nullptr : s.preds, (uint32_t *)l.extra}, count, s.device);
        break;
    case GATHER:
        o = parent::check_gather({l.bits, l.idx, s.n, s.na, in_a, s.src_rows, out_a, (uint32_t *)l.extra}, s.device ? count : nullptr);
        v = colop::check_gather({l.bits, l.idx, s.n, s.na, in_a, s.src_rows, out_a, (uint32_t *)l.extra}, s.device ? count : nullptr);
        break;
    default:
        o = parent::check_select_bits(l.bits, (const uint32_t *)l.extra, s.n);
        v = colop::check_select_bits(l.bits, (const uint32_t *)l.extra, s.n);
        break;
    }
    *was = {o.status, strstr(o.text, "overlaps") != nullptr};
    *is = {v.status, strstr(v.text, "overlaps") != nullptr};
}

static long cases = 0;
static bool moved[OPS][ROLES], moved_onto[OPS][ROLES];

static void fail_case(const State &s, const char *what, const char *detail, Decision was, Decision is)
{
    printf("FAILED %s (%s form, %u + %u columns): %s, %s: was status %d%s, is status %d%s\n", OP_NAME[s.op], s.device ? "device-count" : "blocking",
           s.na, s.nb, what, detail, was.status, was.overlaps ? " (overlaps)" : "", is.status, is.overlaps ? " (overlaps)" : "");
    exit(1);
}

static void same_status(const State &s, const char *what, const char *detail = "")
{
    Decision was, is;
    both(s, &was, &is);
    ++cases;
    if (was.status != is.status || was.overlaps != is.overlaps) fail_case(s, what, detail, was, is);
}

static void expect(const State &s, bool accepted, const char *what)
{
    Decision was, is;
    both(s, &was, &is);
    ++cases;
    if ((was.status == HJGPU_OK) != accepted || (is.status == HJGPU_OK) != accepted) fail_case(s, what, accepted ? "must be accepted" : "must be refused", was, is);
    if (was.status != is.status || was.overlaps != is.overlaps) fail_case(s, what, "", was, is);
}

struct Move { int operand; uintptr_t to; };

static void one_shape(Op op, bool device, uint32_t a, uint32_t b)
{
    const State s0 = base(op, device, a, b);
    expect(s0, true, "the base call");
    // every operand in turn: NULL, misaligned, and onto every other operand
    std::vector<Move> moves;
    for (int i = 0; i < s0.nv; ++i) {
        const uintptr_t p = s0.v[i].p, mine = bytes_of(s0, s0.v[i].role);
        moves.push_back({i, 0});
        moves.push_back({i, p + 4});
        moves.push_back({i, p + 8});
        moved[op][s0.v[i].role] = true;
        for (int j = 0; j < s0.nv; ++j) {
            if (j == i) continue;
            const uintptr_t q = s0.v[j].p, theirs = bytes_of(s0, s0.v[j].role);
            moves.push_back({i, q});                                 // the very pointer
            moves.push_back({i, q + 16});                            // behind its first vector
            moves.push_back({i, q + (theirs - 1) / 16 * 16});        // its last vector
            moves.push_back({i, q - (mine - 1) / 16 * 16});          // before its start: only the moved operand's own last vector reaches in
            moved_onto[op][s0.v[j].role] = true;
        }
    }
    for (const Move &m : moves) {
        State s = s0;
        s.v[m.operand].p = m.to;
        same_status(s, "one operand moved", ROLE_NAME[s0.v[m.operand].role]);
    }
    for (size_t x = 0; x < moves.size(); ++x)
        for (size_t y = x + 1; y < moves.size(); ++y) {
            if (moves[x].operand == moves[y].operand) continue;
            State s = s0;
            s.v[moves[x].operand].p = moves[x].to;
            s.v[moves[y].operand].p = moves[y].to;
            Decision was, is;
            both(s, &was, &is);
            ++cases;
            if ((was.status == HJGPU_OK) != (is.status == HJGPU_OK)) fail_case(s, "two operands moved", ROLE_NAME[s0.v[moves[x].operand].role], was, is);
        }
    // the host arrays
    for (int l = 0; l < 4; ++l) { State s = s0; s.null_list[l] = true; same_status(s, "a null host array"); }
    { State s = s0; s.null_preds = true; same_status(s, "a null predicate array"); }
    // the counts and the limits
    for (uint32_t k : {0u, MAX_A[op], MAX_A[op] + 1}) { State s = s0; s.na = k; same_status(s, "the first count at 0, max, max + 1"); }
    for (uint32_t k : {0u, MAX_B[op], MAX_B[op] + 1}) { State s = s0; s.nb = k; same_status(s, "the second count at 0, max, max + 1"); }
    for (int keep_count = 0; keep_count < 2; ++keep_count) {
        State s = s0;
        s.n = 0;
        for (int i = 0; i < s.nv; ++i) if (!(keep_count && s.v[i].role == COUNT)) s.v[i].p = 0;
        for (int l = 0; l < 4; ++l) s.null_list[l] = true;
        s.null_preds = true;
        same_status(s, "n = 0 with everything NULL");
    }
    { State s = s0; s.n = 1ull << 32; same_status(s, "n = 2^32"); }
    { State s = s0; s.src_rows = 1ull << 32; same_status(s, "src_rows = 2^32"); }
    { State s = s0; s.capacity = 0; same_status(s, "capacity = 0"); }
    { State s = s0; s.capacity = (size_t)hj_group::MAX_CAPACITY + 1; same_status(s, "a capacity without merge slots"); }
    if (hj_group::merge_slots(hj_group::MAX_CAPACITY + 1) != 0) { printf("FAILED: merge_slots(2^40 + 1) is not 0\n"); exit(1); }
    // the predicates
    for (uint32_t p = 0; p < a && op == FILTER; ++p) {
        for (int bit = 2; bit < 32; ++bit) { State s = s0; s.preds[p].flags |= 1u << bit; same_status(s, "an unknown predicate flag"); }
        State s = s0; s.preds[p].reserved = 1; same_status(s, "a non-zero reserved word");
    }
}

static int find(const State &s, Role r, int nth = 0)
{
    for (int i = 0; i < s.nv; ++i) if (s.v[i].role == r && nth-- == 0) return i;
    printf("FAILED: %s has no %s\n", OP_NAME[s.op], ROLE_NAME[r]);
    exit(1);
}

// an output on the very pointer of the input it may replace: accepted; one vector further: refused
static void in_place(Op op, bool device, uint32_t a, Role written, int nth, Role read)
{
    State s = base(op, device, a, 0);
    const int w = find(s, written, nth), r = find(s, read);
    s.v[w].p = s.v[r].p;
    expect(s, true, "in place");
    s.v[w].p = s.v[r].p + 16;
    expect(s, false, "in place, moved by one vector");
}

int main()
{
    for (int device = 0; device < 2; ++device) {
        one_shape(COMPACT, device, HJGPU_COMPACT_MAX_COLS, 0);
        one_shape(COMPACT, device, 0, 0);
        one_shape(GROUP, device, HJGPU_GROUP_MAX_KEYS, HJGPU_GROUP_MAX_VALS);
        one_shape(GROUP, device, 1, 0);
        one_shape(FILTER, device, HJGPU_FILTER_MAX_PREDS, 0);
        one_shape(FILTER, device, 1, 0);
        one_shape(GATHER, device, HJGPU_GATHER_MAX_COLS, 0);
        one_shape(GATHER, device, 1, 0);
        for (uint32_t a : {1u, HJGPU_FILTER_MAX_PREDS}) in_place(FILTER, device, a, EXTRA, 0, BITS);
        for (uint32_t a : {1u, HJGPU_GATHER_MAX_COLS}) {
            in_place(GATHER, device, a, EXTRA, 0, BITS);
            for (uint32_t c = 0; c < a; ++c) in_place(GATHER, device, a, OUT_A, c, IDX);
        }
    }
    one_shape(LOOKUP, false, 0, 0);
    in_place(LOOKUP, false, 0, EXTRA, 0, BITS);
    // every operand of every operator was moved, and was moved onto
    const State full[OPS] = {base(COMPACT, true, 8, 0), base(GROUP, true, 2, 4), base(FILTER, true, 4, 0), base(GATHER, true, 4, 0), base(LOOKUP, false, 0, 0)};
    for (const State &s : full)
        for (int i = 0; i < s.nv; ++i)
            if (!moved[s.op][s.v[i].role] || !moved_onto[s.op][s.v[i].role]) {
                printf("FAILED: the %s of %s was never exercised\n", ROLE_NAME[s.v[i].role], OP_NAME[s.op]);
                return 1;
            }
    printf("ok: %ld cases\n", cases);
    return 0;
}
