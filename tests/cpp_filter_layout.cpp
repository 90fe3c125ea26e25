// CPU test of hash_join_codes_knl_amd/csrc/filter_layout.hpp (compiled and run by tests/test_filter_layout.py): hjgpu_filter_selected's
// predicate arithmetic - normalise() on the host, passes() on the device - against the definition written out directly: lo <= x <= hi in
// uint32 order, or in int32 order under HJGPU_PRED_SIGNED, inverted under HJGPU_PRED_NOT.  All four flag combinations and all triples
// (lo, hi, x) of a boundary set around 0, the sign change and 2^32: 4 x 9^3 cases that hold empty ranges (lo > hi), the full range, single
// values and signed ranges that straddle 0.  Exact agreement; plus the shape of the normal form and the geometry's counter.
#include <stdio.h>
#include "filter_layout.hpp"

static bool by_definition(uint32_t lo, uint32_t hi, uint32_t flags, uint32_t x)
{
    bool in;
    if (flags & hj_filter::PRED_SIGNED) in = (int32_t)lo <= (int32_t)x && (int32_t)x <= (int32_t)hi;
    else in = lo <= x && x <= hi;
    return (flags & hj_filter::PRED_NOT) ? !in : in;
}

int main()
{
    const uint32_t edge[9] = {0u, 1u, 2u, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    size_t cases = 0, passing = 0, empty = 0;
    for (uint32_t flags = 0; flags < 4; ++flags)
        for (uint32_t lo : edge)
            for (uint32_t hi : edge) {
                const hj_filter::Norm p = hj_filter::normalise(lo, hi, flags);
                if (p.invert > 1u || p.bias != ((flags & hj_filter::PRED_SIGNED) ? 0x80000000u : 0u) || (uint64_t)p.lo + p.span > 0xFFFFFFFFull) {
                    fprintf(stderr, "FAIL: normal form of lo %08x hi %08x flags %u: bias %08x lo %08x span %08x invert %u\n", lo, hi, flags, p.bias, p.lo,
                            p.span, p.invert);
                    return 1;
                }
                const bool is_empty = (flags & hj_filter::PRED_SIGNED) ? (int32_t)lo > (int32_t)hi : lo > hi;
                empty += is_empty ? 1 : 0;
                for (uint32_t x : edge) {
                    const bool want = by_definition(lo, hi, flags, x), got = hj_filter::passes(p, x);
                    if (is_empty && want != ((flags & hj_filter::PRED_NOT) != 0)) { fprintf(stderr, "FAIL: the test's own definition of the empty range\n"); return 1; }
                    if (got != want) {
                        fprintf(stderr, "FAIL: lo %08x hi %08x flags %u x %08x: passes() says %d, the definition %d\n", lo, hi, flags, x, (int)got, (int)want);
                        return 1;
                    }
                    ++cases; passing += want ? 1 : 0;
                }
            }
    if (cases != 4 * 9 * 9 * 9 || passing == 0 || passing == cases || empty != 4 * 36) { fprintf(stderr, "FAIL: the case set (%zu cases, %zu passing, %zu empty ranges)\n", cases, passing, empty); return 1; }
    if (hj_filter::step_rows(256) != 256ull * hj_filter::RESIDENT * hj_filter::BLOCK * 4 * hj_filter::BATCH || hj_filter::step_rows(0) != hj_filter::step_rows(1) ||
        hj_filter::step_rows(1) % 256) { fprintf(stderr, "FAIL: step_rows\n"); return 1; }
    printf("ok: %zu cases, %zu passing, %zu empty ranges\n", cases, passing, empty);
    return 0;
}
