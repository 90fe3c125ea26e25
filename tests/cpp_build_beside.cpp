// CPU test of hash_join_codes_knl_amd/csrc/build_beside_layout.hpp (compiled and run by tests/test_build_beside_layout.py): the CU split
// between the build side's chain and the probe side's passes, for 1 ... 304 CUs and option "build_cus" 0 ... 400 (and a negative one), with
// relations large enough for the library's own choice, too small for it, and empty.  Either there is no overlap - build 0, the probe side
// has every CU - or both sides have at least one CU and the two budgets are exactly the CUs there are; an explicit option is honoured up to
// CUs - 1; the library's own choice is the committed default, on chips of MIN_CUS CUs and more, probe sides of MIN_PROBE_ROWS and more and
// at least MIN_PROBE_PER_BUILD probe rows per build row - and the one-stream order everywhere else (64 M x 64 M, 64 M x 256 M).
#include <stdio.h>
#include "build_beside_layout.hpp"

static int fail(const char *what, int cus, int opt, uint64_t inner, uint64_t outer)
{
    fprintf(stderr, "FAIL: %s (cus %d, build_cus %d, inner %llu, outer %llu)\n", what, cus, opt, (unsigned long long)inner, (unsigned long long)outer);
    return 1;
}

int main()
{
    using namespace hj_beside;
    // what the sweep chose (profiles/r24_build_cus_sweep.txt) and what DESIGN.md and README.md quote
    static_assert(DEFAULT_BUILD_CUS == 32, "the committed default");
    static_assert(MIN_CUS == 128 && MIN_PROBE_ROWS == (1u << 20) && MIN_PROBE_PER_BUILD == 12, "the thresholds of the library's own choice");
    // a probe side that is not many times its build side: the build side's chain on 32 CUs would outlast the probe side's passes
    static_assert(!split(256, 0, 64000000, 64000000).overlap() && !split(256, 0, 64000000, 256000000).overlap() &&
                  !split(256, 0, 64000000, 12ull * 64000000 - 1).overlap() && split(256, 0, 64000000, 12ull * 64000000).overlap(), "the ratio rule");
    static_assert(split(256, 32, 64000000, 64000000).build == 32, "an explicit build_cus overlaps at any ratio");
    static_assert(split(256, 0, 64000000, 1000000000).build == 32 && split(256, 0, 64000000, 1000000000).probe == 224, "the headline's split");
    const uint64_t rows[] = {0, 1, 1000, 16384, MIN_PROBE_ROWS / 12, MIN_PROBE_ROWS / 12 + 1, MIN_PROBE_ROWS - 1, MIN_PROBE_ROWS, 3000000, 36000000 - 1, 36000000, 1ull << 33};
    auto small_ratio = [](uint64_t inner, uint64_t outer) { return outer / MIN_PROBE_PER_BUILD < inner; };
    size_t cases = 0, overlapping = 0;
    for (int cus = 1; cus <= 304; ++cus)
        for (int opt = -1; opt <= 400; ++opt)
            for (uint64_t inner : rows)
                for (uint64_t outer : rows) {
                    const Split s = split(cus, opt, inner, outer);
                    ++cases;
                    if (s.build + s.probe != cus) return fail("the budgets do not sum to the CUs", cus, opt, inner, outer);
                    if (s.overlap() != (s.build > 0)) return fail("overlap() and build disagree", cus, opt, inner, outer);
                    if (!s.overlap()) {
                        if (s.build != 0 || s.probe != cus) return fail("no overlap, but the probe side does not have every CU", cus, opt, inner, outer);
                        // when is stepping aside right?  one CU, an empty relation, a negative option, or the library's choice below its thresholds
                        const bool may = cus < 2 || !inner || !outer || opt < 0 || (opt == 0 && (DEFAULT_BUILD_CUS == 0 || cus < MIN_CUS || outer < MIN_PROBE_ROWS || small_ratio(inner, outer)));
                        if (!may) return fail("stepped aside without a reason", cus, opt, inner, outer);
                        continue;
                    }
                    ++overlapping;
                    if (s.build < 1 || s.probe < 1) return fail("a side without a CU", cus, opt, inner, outer);
                    if (!inner || !outer || cus < 2 || opt < 0) return fail("overlap where there is nothing to overlap", cus, opt, inner, outer);
                    if (opt > 0 && s.build != (opt < cus - 1 ? opt : cus - 1)) return fail("an explicit build_cus is not honoured", cus, opt, inner, outer);
                    if (opt == 0 && (s.build != DEFAULT_BUILD_CUS || cus < MIN_CUS || outer < MIN_PROBE_ROWS || small_ratio(inner, outer)))
                        return fail("the library's own choice is not the default inside its thresholds", cus, opt, inner, outer);
                }
    printf("ok: %zu splits, %zu of them overlap; the library's choice is %d CUs from %d CUs, %llu probe rows and %llu probe rows per build row on\n",
           cases, overlapping, DEFAULT_BUILD_CUS, MIN_CUS, (unsigned long long)MIN_PROBE_ROWS, (unsigned long long)MIN_PROBE_PER_BUILD);
    return 0;
}
