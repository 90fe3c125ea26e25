// CPU test of hash_join_codes_knl_amd/csrc/gather_layout.hpp (compiled and run by tests/test_gather_layout.py): hjgpu_gather_selected's row
// classification against its definition written out directly - a row is gathered when it is selected and its index is below src_rows; a
// selected row whose index is neither below src_rows nor HJGPU_NULL_VAL is out of range; everything else is a NULL row - for selected in
// {0, 1} and all pairs (index, src_rows) of a boundary set around 0, 2^30 (where 4 * index leaves 32 bits), 2^31 and 2^32: 2 x 8^2 cases.
// A gathered row's byte offset 4 * index, formed in 64 bits as the kernel forms it, stays inside the source column.  Plus the geometry's
// counter.
#include <stdio.h>
#include "gather_layout.hpp"

int main()
{
    using namespace hj_gather;
    const uint32_t edge[8] = {0u, 1u, 2u, 0x3FFFFFFFu, 0x40000000u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    size_t cases = 0, seen[3] = {0, 0, 0};
    for (int selected = 0; selected < 2; ++selected)
        for (uint32_t idx : edge)
            for (uint32_t src_rows : edge) {
                Row want = ROW_NULL;
                if (selected && (uint64_t)idx < (uint64_t)src_rows) want = ROW_GATHERED;
                else if (selected && idx != 0xFFFFFFFFu) want = ROW_OUT_OF_RANGE;
                const Row got = classify(selected != 0, idx, src_rows);
                if (got != want) {
                    fprintf(stderr, "FAIL: selected %d idx %08x src_rows %08x: classify() says %u, the definition %u\n", selected, idx, src_rows, (unsigned)got,
                            (unsigned)want);
                    return 1;
                }
                if (got == ROW_GATHERED && ((uint64_t)idx * 4 + 4 > (uint64_t)src_rows * 4 || idx == NULL_VAL)) {
                    fprintf(stderr, "FAIL: a gathered row outside the source: idx %08x src_rows %08x\n", idx, src_rows);
                    return 1;
                }
                ++cases; ++seen[got];
            }
    if (cases != 2 * 8 * 8 || !seen[ROW_NULL] || !seen[ROW_GATHERED] || !seen[ROW_OUT_OF_RANGE] || seen[ROW_NULL] != 64 + 8) {
        fprintf(stderr, "FAIL: the case set (%zu cases: %zu null, %zu gathered, %zu out of range)\n", cases, seen[0], seen[1], seen[2]);
        return 1;
    }
    if (MAX_COLS != 4 || NULL_VAL != 0xFFFFFFFFu) { fprintf(stderr, "FAIL: constants\n"); return 1; }
    if (grid_of(256) != 256 * RESIDENT || grid_of(0) != grid_of(1) || grid_of(-3) != RESIDENT ||
        step_rows(256) != 256ull * RESIDENT * BLOCK * 4 * BATCH || step_rows(0) != step_rows(1) || step_rows(1) % 256 ||
        step_rows(1 << 20) <= 0xFFFFFFFFull) { fprintf(stderr, "FAIL: grid_of / step_rows\n"); return 1; }
    printf("ok: %zu cases, %zu null, %zu gathered, %zu out of range\n", cases, seen[0], seen[1], seen[2]);
    return 0;
}
