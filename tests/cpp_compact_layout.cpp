// CPU test of hash_join_codes_knl_amd/csrc/compact_layout.hpp (compiled and run by tests/test_compact_layout.py): the ranges that
// hjgpu_compact_selected's two launches walk, for n from 0 through the tails of the GPU tests, around multiples of a chunk and of a
// whole grid of chunks, and up to 2^40, with 1, 2, 512 and 2048 ranges.  The ranges must be disjoint, ascending and cover [0, n) exactly;
// every range but the last non-empty one is a whole number of chunks; every range starts at a multiple of 256 rows; nothing overflows 64
// bits (the sanitizer and 128-bit arithmetic beside the header's say so); the mask words a range's count pass touches lie inside the
// mask's (n + 31) / 32 words, the ranges' words together are exactly those, and a word is shared by no two ranges.
#include <stdio.h>
#include <vector>
#include "compact_layout.hpp"

using hj_compact::u64;
typedef unsigned __int128 u128;

static int fail(const char *what, u64 n, uint32_t G, uint32_t g)
{
    fprintf(stderr, "FAIL: %s (n = %llu, ranges = %u, range %u)\n", what, n, G, g);
    return 1;
}

static int check(u64 n, uint32_t G)
{
    const u64 C = hj_compact::CHUNK_ROWS;
    const hj_compact::Layout l = hj_compact::layout(n, G);
    if (l.ranges != G || l.n != n) return fail("layout fields", n, G, 0);
    if (l.range_rows % C) return fail("a range is not a whole number of chunks", n, G, 0);
    if ((u128)l.range_rows * G < (u128)n) return fail("the ranges do not hold n rows", n, G, 0);
    if (n && (u128)l.range_rows * G >= (u128)n + (u128)C * G) return fail("the ranges are a chunk too long", n, G, 0);
    const u64 words = (n + 31) / 32;
    u64 at = 0, word_at = 0;
    bool tail_seen = false;
    for (uint32_t g = 0; g < G; ++g) {
        const u64 b = l.begin(g), e = l.end(g);
        // what the header computes, in 128 bits
        const u128 wb = (u128)g * l.range_rows, we = wb + l.range_rows;
        if (b != (u64)(wb < n ? wb : (u128)n) || e != (u64)(we < n ? we : (u128)n)) return fail("begin / end differ from the 128-bit arithmetic", n, G, g);
        if (b != at) return fail("ranges are not contiguous and ascending", n, G, g);
        if (e < b || e > n) return fail("range end", n, G, g);
        if (e > b) {
            if (b % 256) return fail("a range does not start at a multiple of 256 rows", n, G, g);
            if (tail_seen) return fail("a non-empty range behind the tail", n, G, g);
            if ((e - b) % C) { if (e != n) return fail("a range that is not the last non-empty one is not whole chunks", n, G, g); }
            if (e == n) tail_seen = true;
            else if (e - b != l.range_rows) return fail("a range before the tail is short", n, G, g);
        } else if (b != n) return fail("an empty range does not lie at n", n, G, g);
        u64 w0 = 0, w1 = 0;
        hj_compact::count_words(l, g, &w0, &w1);
        if (w1 < w0 || w1 > words) return fail("the count pass reads beyond the mask's words", n, G, g);
        if (e > b) {
            if (w0 != word_at) return fail("mask words are skipped or shared between ranges", n, G, g);
            if (w0 % 4) return fail("a range's mask words do not start 16-byte aligned", n, G, g);
            if (w0 * 32 != b || w1 * 32 < e || (w1 - 1) * 32 >= e) return fail("the range's words are not the words of its rows", n, G, g);
            word_at = w1;
        } else if (w1 != w0) return fail("an empty range reads mask words", n, G, g);
        at = e;
    }
    if (at != n) return fail("the ranges do not cover [0, n)", n, G, G);
    if (word_at != words) return fail("the count passes do not read every mask word once", n, G, G);
    return 0;
}

int main()
{
    const u64 C = hj_compact::CHUNK_ROWS;
    if (C != (u64)hj_compact::BLOCK * 4 * hj_compact::VEC || C % 256) { fprintf(stderr, "FAIL: chunk rows\n"); return 1; }
    if (hj_compact::ranges_of(256) != 2048 || hj_compact::ranges_of(1) != hj_compact::RESIDENT || hj_compact::ranges_of(0) != hj_compact::RESIDENT ||
        hj_compact::ranges_of(100000) != hj_compact::MAX_RANGES) { fprintf(stderr, "FAIL: ranges_of\n"); return 1; }
    const uint32_t grids[] = {1, 2, 512, 2048};
    size_t cases = 0;
    for (uint32_t G : grids) {
        std::vector<u64> ns = {0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099};
        const u64 centres[] = {C, 2 * C, 3 * C, (u64)G * C, 2 * (u64)G * C, 5 * (u64)G * C, ((u64)G - 1) * C, ((u64)G + 1) * C, 1000000000ull,
                               1ull << 32, 1ull << 40};
        for (u64 c : centres)
            for (u64 d : {(u64)0, (u64)1, (u64)31, (u64)32, (u64)33, (u64)255, (u64)256, C - 1, C, C + 1}) {
                if (c >= d) ns.push_back(c - d);
                if (c + d <= (1ull << 40)) ns.push_back(c + d);
            }
        for (u64 n : ns) { if (check(n, G)) return 1; ++cases; }
    }
    printf("ok: %zu layouts\n", cases);
    return 0;
}
