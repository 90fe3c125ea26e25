// The constants of hash_join_codes_knl_amd/csrc/scatter_layout.hpp that tests/operator_cases.py states (compiled and run by
// tests/test_operator_cases.py, as tests/cpp_scatter_layout.cpp is by tests/test_scatter_layout.py): one "name value" line each, and the
// tile that K6 pass 1 takes at every fan-out by hj_scatter_config's rule for packed output (partition_kernels.hip): 1024 threads x the
// largest of 4, 3, 2 vectors whose carry buffers fit the LDS beside the tile, else 1024 x 4 without carry.
#include <stdio.h>
#include "scatter_layout.hpp"

int main()
{
    printf("HJ_LINE_TUPLES %u\nHJ_STREAM_UNIT %u\nHJ_MAX_HEAVY %u\n", HJ_LINE_TUPLES, HJ_STREAM_UNIT, HJ_MAX_HEAVY);
    for (uint32_t F = 1; F <= 1024; ++F) {
        int vpt = 4, carry = 0;
        for (int v = 4; v >= 2; --v)
            if (hj_scatter::carry_fits(1024, v, F)) { vpt = v; carry = 1; break; }
        printf("tile %u %d %d\n", F, 1024 * vpt * 4, carry);
    }
    return 0;
}
