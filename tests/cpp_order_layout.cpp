// cpp_order_layout.cpp - csrc/order_layout.hpp on the CPU: the ranges of the device road, the key normalisation, and a host emulation of
// the whole pass sequence - both roads' arithmetic, the header's digit functions - against std::stable_sort with the composite comparator.
// Prints "ok: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "order_layout.hpp"

using namespace hj_order;
static long cases = 0;

#define REQUIRE(cond, ...)                                                      \
    do {                                                                        \
        if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } \
    } while (0)

// ---- the ranges: they tile [0, n), start on chunk boundaries, and the tail is in the last non-empty one ------------------------------------
static void check_ranges(u64 n, uint32_t ranges)
{
    const Layout l = layout(n, ranges);
    REQUIRE(l.ranges == ranges && l.n == n && l.range_rows % CHUNK_ROWS == 0, "n %llu ranges %u", n, ranges);
    REQUIRE((n == 0) == (l.range_rows == 0), "n %llu", n);
    u64 at = 0;
    bool ended = false;
    for (uint32_t g = 0; g < ranges; ++g) {
        const u64 b = l.begin(g), e = l.end(g);
        REQUIRE(b <= e && e <= n, "n %llu range %u: [%llu, %llu)", n, g, b, e);
        if (b == e) { ended = true; REQUIRE(b == n, "an empty range lies at n (n %llu range %u)", n, g); continue; }
        REQUIRE(!ended, "a non-empty range behind an empty one (n %llu range %u)", n, g);
        REQUIRE(b == at && b % CHUNK_ROWS == 0, "n %llu range %u begins at %llu, want %llu", n, g, b, at);
        REQUIRE(e == n || (e - b) % CHUNK_ROWS == 0, "only the last non-empty range holds a partial chunk (n %llu range %u)", n, g);
        REQUIRE(e - b <= l.range_rows, "n %llu range %u", n, g);
        at = e;
    }
    REQUIRE(at == n, "the ranges end at %llu, n %llu", at, n);
    ++cases;
}

// ---- the normalisation orders as the plain comparison does -------------------------------------------------------------------------------------
static bool before32(uint32_t a, uint32_t b, uint32_t flags)
{
    if (flags & SIGNED) return (flags & DESC) ? (int32_t)a > (int32_t)b : (int32_t)a < (int32_t)b;
    return (flags & DESC) ? a > b : a < b;
}
static bool before64(u64 a, u64 b, uint32_t flags)
{
    if (flags & SIGNED) return (flags & DESC) ? (long long)a > (long long)b : (long long)a < (long long)b;
    return (flags & DESC) ? a > b : a < b;
}

static void check_normalisation()
{
    const uint32_t e32[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const u64 e64[] = {0ull, 1ull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 0x100000000ull, 0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull,
                       0x8000000000000001ull, 0xFFFFFFFF00000000ull, 0xFFFFFFFFFFFFFFFFull};
    for (uint32_t dir : {0u, DESC})
        for (uint32_t sign : {0u, SIGNED}) {
            const uint32_t f = dir | sign;
            for (uint32_t a : e32)
                for (uint32_t b : e32) {
                    REQUIRE((norm32(a, f) < norm32(b, f)) == before32(a, b, f), "%08x %08x flags %u", a, b, f);
                    REQUIRE((norm(a, f) < norm(b, f)) == before32(a, b, f) && (norm(a, f) >> 32) == 0, "%08x %08x flags %u", a, b, f);
                    // the digits of the normalised word are what a pass reads from the column's word
                    for (uint32_t p = 0; p < 4; ++p) {
                        const uint32_t flags1[1] = {f};
                        const Pass s = pass_of(1, flags1, p);
                        REQUIRE(s.key == 0 && s.stride == 1 && s.word == 0 && pass_digit(a, s.xor_mask, s.shift) == digit(norm(a, f), p), "%08x flags %u pass %u", a, f, p);
                    }
                    ++cases;
                }
            for (u64 a : e64)
                for (u64 b : e64) {
                    REQUIRE((norm64(a, f) < norm64(b, f)) == before64(a, b, f), "%016llx %016llx flags %u", a, b, f);
                    REQUIRE((norm(a, f | WIDE) < norm(b, f | WIDE)) == before64(a, b, f), "%016llx %016llx flags %u", a, b, f);
                    for (uint32_t p = 0; p < 8; ++p) {
                        const uint32_t flags1[1] = {f | WIDE};
                        const Pass s = pass_of(1, flags1, p);
                        const uint32_t w = (uint32_t)(a >> (32 * s.word));
                        REQUIRE(s.stride == 2 && s.word == p / 4 && pass_digit(w, s.xor_mask, s.shift) == digit(norm(a, f | WIDE), p), "%016llx flags %u pass %u", a, f, p);
                    }
                    ++cases;
                }
        }
}

// ---- the pass sequence --------------------------------------------------------------------------------------------------------------------------
struct Keys {
    uint32_t nkeys;
    uint32_t flags[MAX_KEYS];
    std::vector<u64> col[MAX_KEYS];                     // a 32-bit key: the low half
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static std::vector<uint32_t> by_stable_sort(const Keys &k, const std::vector<uint32_t> &selected)
{
    std::vector<uint32_t> perm = selected;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
        for (uint32_t c = 0; c < k.nkeys; ++c) {
            const u64 x = k.col[c][a], y = k.col[c][b];
            const bool wide = (k.flags[c] & WIDE) != 0;
            if (wide ? before64(x, y, k.flags[c]) : before32((uint32_t)x, (uint32_t)y, k.flags[c])) return true;
            if (wide ? before64(y, x, k.flags[c]) : before32((uint32_t)y, (uint32_t)x, k.flags[c])) return false;
        }
        return false;
    });
    return perm;
}

// the device road: per pass a histogram per range, an exclusive scan over (digit, range), a scatter that walks every range chunk by chunk
static std::vector<uint32_t> by_device_road(const Keys &k, const std::vector<uint32_t> &selected, u64 n, uint32_t ranges)
{
    std::vector<uint32_t> perm = selected, next(selected.size());
    const u64 live = selected.size();
    const Layout l = layout(n, ranges);
    const uint32_t passes = passes_of(k.nkeys, k.flags);
    for (uint32_t p = 0; p < passes; ++p) {
        const Pass s = pass_of(k.nkeys, k.flags, p);
        auto digit_at = [&](u64 pos) {
            const u64 x = k.col[s.key][perm[pos]];
            return pass_digit((uint32_t)(x >> (32 * s.word)), s.xor_mask, s.shift);
        };
        std::vector<uint32_t> counts((size_t)DIGITS * ranges, 0), bases((size_t)DIGITS * ranges, 0);
        for (uint32_t g = 0; g < ranges; ++g)
            for (u64 pos = l.begin(g); pos < std::min<u64>(l.end(g), live); ++pos) ++counts[(size_t)digit_at(pos) * ranges + g];
        uint32_t at = 0;
        for (size_t i = 0; i < counts.size(); ++i) { bases[i] = at; at += counts[i]; }
        for (uint32_t g = 0; g < ranges; ++g) {
            uint32_t run[DIGITS];
            for (uint32_t d = 0; d < DIGITS; ++d) run[d] = bases[(size_t)d * ranges + g];
            const u64 end = std::min<u64>(l.end(g), live);
            for (u64 chunk0 = l.begin(g); chunk0 < end; chunk0 += CHUNK_ROWS)
                for (u64 pos = chunk0; pos < std::min<u64>(chunk0 + CHUNK_ROWS, end); ++pos) next[run[digit_at(pos)]++] = perm[pos];
        }
        perm.swap(next);
    }
    return perm;
}

// the LDS road: the normalised word travels with the row number; a pass whose digit is the same for every row is skipped
static std::vector<uint32_t> by_lds_road(const Keys &k, const std::vector<uint32_t> &selected, long *skipped)
{
    std::vector<uint32_t> perm = selected, next(selected.size());
    std::vector<u64> key(selected.size()), key_next(selected.size());
    for (uint32_t c = k.nkeys; c-- > 0;) {
        for (size_t i = 0; i < perm.size(); ++i) key[i] = norm(k.col[c][perm[i]], k.flags[c]);
        for (uint32_t d = 0; d < digits_of(k.flags[c]); ++d) {
            uint32_t count[DIGITS] = {}, start[DIGITS];
            for (size_t i = 0; i < perm.size(); ++i) ++count[digit(key[i], d)];
            bool same = false;
            uint32_t at = 0;
            for (uint32_t x = 0; x < DIGITS; ++x) { start[x] = at; at += count[x]; same |= count[x] == perm.size(); }
            if (same) { ++*skipped; continue; }
            for (size_t i = 0; i < perm.size(); ++i) { const uint32_t r = start[digit(key[i], d)]++; next[r] = perm[i]; key_next[r] = key[i]; }
            perm.swap(next); key.swap(key_next);
        }
    }
    return perm;
}

static void check_passes()
{
    long skipped = 0;
    const u64 sizes[] = {0, 1, 2, 63, 64, 65, 1000, CHUNK_ROWS - 1, CHUNK_ROWS, CHUNK_ROWS + 1, 3 * CHUNK_ROWS + 17, LDS_ROWS, LDS_ROWS + 1};
    for (u64 n : sizes)
        for (uint32_t nkeys = 1; nkeys <= MAX_KEYS; ++nkeys)
            for (uint32_t trial = 0; trial < 6; ++trial) {
                Keys k;
                k.nkeys = nkeys;
                for (uint32_t c = 0; c < nkeys; ++c) {
                    k.flags[c] = (uint32_t)(rnd() & 7);                             // width, direction and signedness mixed
                    k.col[c].resize(n);
                    // few distinct values (ties reach the later keys and the row number), the edges, or anything
                    const uint32_t kind = (uint32_t)(rnd() % 4);
                    for (u64 i = 0; i < n; ++i) {
                        u64 x = rnd();
                        if (kind == 0) x %= 3;
                        else if (kind == 1) x = (x % 5) << ((rnd() & 1) ? 60 : 29);
                        else if (kind == 2) x = (x & 1) ? ~(x % 7) : x % 7;
                        if (!(k.flags[c] & WIDE)) x &= 0xFFFFFFFFull;
                        k.col[c][i] = x;
                    }
                }
                std::vector<uint32_t> selected;
                const uint32_t mask_kind = (uint32_t)(rnd() % 3);                   // every row, about half of them, a few
                for (u64 i = 0; i < n; ++i)
                    if (mask_kind == 0 || (mask_kind == 1 ? (rnd() & 1) : rnd() % 16 == 0)) selected.push_back((uint32_t)i);
                const std::vector<uint32_t> want = by_stable_sort(k, selected);
                for (uint32_t ranges : {1u, 2u, 3u, 7u}) REQUIRE(by_device_road(k, selected, n, ranges) == want, "the device road: n %llu, %u keys, %u ranges", n, nkeys, ranges);
                REQUIRE(by_lds_road(k, selected, &skipped) == want, "the LDS road: n %llu, %u keys", n, nkeys);
                ++cases;
            }
    REQUIRE(skipped > 0, "no pass was ever skipped");
}

int main()
{
    static_assert(LDS_ROWS >= 4096, "the few thousand groups of a GROUP BY fit one workgroup");
    static_assert(CHUNK_ROWS % 256 == 0 && (u64)2 * 2 * CHUNK_ROWS <= ((u64)1 << 23), "two ranges of two chunks below 2^23 rows");
    for (uint32_t ranges : {1u, 2u, 3u, 64u, 1000u, MAX_RANGES}) {
        for (u64 n = 0; n <= 4 * (u64)CHUNK_ROWS + 1; n += (n < 70 || n % CHUNK_ROWS < 2 || n % CHUNK_ROWS > CHUNK_ROWS - 3) ? 1 : 97) check_ranges(n, ranges);
        for (u64 n : {(u64)LDS_ROWS - 1, (u64)LDS_ROWS, (u64)LDS_ROWS + 1, (u64)ranges * CHUNK_ROWS - 1, (u64)ranges * CHUNK_ROWS, (u64)ranges * CHUNK_ROWS + 1,
                      (u64)ranges * 2 * CHUNK_ROWS, (u64)ranges * 2 * CHUNK_ROWS + 1, (u64)0xFFFFFFFFull})
            check_ranges(n, ranges);
        // the smallest n with at least two ranges of at least two chunks
        const u64 n2 = ranges >= 3 ? (u64)ranges * CHUNK_ROWS + 1 : ranges == 2 ? 3 * (u64)CHUNK_ROWS + 1 : 0;
        if (n2) {
            const Layout l = layout(n2, ranges), below = layout(n2 - 1, ranges);
            REQUIRE(l.end(0) - l.begin(0) >= 2 * CHUNK_ROWS && l.end(1) - l.begin(1) > CHUNK_ROWS, "ranges %u", ranges);
            REQUIRE(!(below.end(0) - below.begin(0) >= 2 * CHUNK_ROWS && below.end(1) - below.begin(1) > CHUNK_ROWS), "ranges %u", ranges);
        }
    }
    REQUIRE(lds_road(LDS_ROWS) && !lds_road(LDS_ROWS + 1) && lds_road(0), "the road switch");
    REQUIRE(workspace_bytes(LDS_ROWS) == COUNT_WORD_BYTES && workspace_bytes(LDS_ROWS + 1) == WORKSPACE_HEAD + 2 * perm_bytes(LDS_ROWS + 1), "the workspace");
    REQUIRE(perm_bytes(5) == 32 && perm_bytes(8) == 32, "whole vectors");
    REQUIRE(ranges_of(256) == MAX_RANGES && ranges_of(0) == RESIDENT && ranges_of(100000) == MAX_RANGES, "ranges_of");
    check_normalisation();
    check_passes();
    printf("ok: %ld cases\n", cases);
    return 0;
}
