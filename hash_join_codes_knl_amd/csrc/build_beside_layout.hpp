// build_beside_layout.hpp - how a blocking whole join with a claimed probe side shares the chip between its two streams (hjgpu_api.hip
// PhjRun::partition_beside, DESIGN.md section 3 "Build side beside the probe side").  Plain arithmetic, no HIP: tests/cpp_build_beside.cpp
// walks every CU count and every value of option "build_cus".
//
// K6 occupies a CU completely, so a kernel of the build side's chain finds a CU only where the probe side's grids leave one free: the
// probe side's two passes get `probe` CUs, every launch of the build side's chain (K4, K6 pass 1, K6 pass 2) `build` CUs, and
// build + probe = the CUs the context lets K6 have.  build == 0 says "no overlap": the join takes the one-stream order.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hj_beside {
// The library's choice of `build` (option "build_cus" = 0), from profiles/r24_build_cus_sweep.txt (64 M x 1 G, 256 CUs): with 16 or 24 CUs the
// build side's chain is not over when the probe side's pass 2 is (the caller's stream waits 1.75 / 0.47 ms for it), with 32 it is
// (0.01 ms) and the step is the shortest of the sweep; 48 take more from the probe side's pass 1 than they give.
constexpr int DEFAULT_BUILD_CUS = 32;
// The library's choice steps aside on a chip with fewer CUs than this (a build side's share of a small chip is a large share of K6's rate) ...
constexpr int MIN_CUS = 128;
// ... and for a probe side below this many rows: its passes are over before the build side's chain of launches is, and the fork and the
// join cost three event operations ...
constexpr uint64_t MIN_PROBE_ROWS = 1u << 20;
// ... and unless the probe side has at least this many rows per build row.  The build side's launches keep their `build` CUs for their
// whole life - their grids do not widen when the probe side's passes end - so the form pays only while the build side's chain ends inside
// the probe side's two passes; where it does not, the caller's stream waits for a chain that is five times slower than on the whole chip.
// profiles/r24_build_beside_kernel_stats.txt: 64 M build rows take 3.1 - 3.3 ms on 32 of 256 CUs (0.05 ms per million rows), the two passes
// over 1 G probe rows 6.0 ms on the other 224 (0.006 ms per million): the two end together at 8.3 probe rows per build row.  12 leaves
// the chain 70 % of the passes' span.  Reasoned from that one trace, like MIN_CUS and MIN_PROBE_ROWS, not measured; that a rule
// is needed is (profiles/r24_build_beside_other_shapes.txt: forced, 64 M x 256 M takes 3.68 ms against 2.95, 64 M x 64 M 3.15 against 1.72).
// An explicit "build_cus" overlaps at any size and any ratio.
constexpr uint64_t MIN_PROBE_PER_BUILD = 12;

struct Split {
    int build, probe;           // CUs of the build side's launches / of the probe side's passes; build == 0: no overlap, probe = all
    constexpr bool overlap() const { return build > 0; }
};

// cus: the CUs K6 may occupy; build_cus: option "build_cus" (0 = the library's choice, else the build side's CUs, at most cus - 1)
constexpr Split split(int cus, int build_cus, uint64_t inner_rows, uint64_t outer_rows)
{
    const Split none = {0, cus};
    if (cus < 2 || inner_rows == 0 || outer_rows == 0 || build_cus < 0) return none;
    if (build_cus == 0) {
        if (DEFAULT_BUILD_CUS == 0 || cus < MIN_CUS || outer_rows < MIN_PROBE_ROWS || outer_rows / MIN_PROBE_PER_BUILD < inner_rows) return none;
        build_cus = DEFAULT_BUILD_CUS;
    }
    const int b = build_cus < cus - 1 ? build_cus : cus - 1;
    return Split{b, cus - b};
}
}  // namespace hj_beside
