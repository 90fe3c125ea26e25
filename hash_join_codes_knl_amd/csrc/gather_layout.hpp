// gather_layout.hpp - the row classification and the geometry of hjgpu_gather_selected (gen_kernels.hip gather_kernel, DESIGN.md section 5
// "Gather by row number").  Plain host / device arithmetic, no HIP: the kernel classifies every row with classify() before it forms an
// address, and tests/test_gather_layout.py compiles the same function with g++ and compares it with the definition.
//
// A row is GATHERED when it is selected and its index is below src_rows: only then is a source element read.  A selected row whose index is
// HJGPU_NULL_VAL - the NULL of a look-up or of an outer join - and every unselected row, whatever its index holds, is a NULL row.  A
// selected row whose index is neither is OUT OF RANGE: it is written like a NULL row and counted.  src_rows never exceeds 0xFFFFFFFF (the
// entry points refuse more), so HJGPU_NULL_VAL is never below it and "idx < src_rows" alone keeps every read inside the source column.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HJ_GATHER_FN __host__ __device__ inline
#else
#define HJ_GATHER_FN inline
#endif

namespace hj_gather {
typedef unsigned long long u64;

constexpr uint32_t MAX_COLS = 4;                        // HJGPU_GATHER_MAX_COLS
constexpr uint32_t NULL_VAL = 0xFFFFFFFFu;              // HJGPU_NULL_VAL

constexpr uint32_t BLOCK = 256;                         // lanes per workgroup
constexpr uint32_t BATCH = 2;                           // wave trips (of hj_lookup.hpp: 256 rows) per wave and loop iteration
constexpr uint32_t RESIDENT = 5;                        // workgroups of BLOCK lanes per CU in the persistent grid: the waves per SIMD that every instance,
                                                        // the four-column one at 96 VGPRs included, holds - the whole grid is resident at once

// the persistent grid's workgroups on a device of `cus` compute units (fewer when the rows have fewer wave trips: hj_launch_gather)
inline uint32_t grid_of(int cus) { return (uint32_t)(cus < 1 ? 1 : cus) * RESIDENT; }
// hjgpu_get_counter "gather_step_rows": the rows that grid covers in one loop iteration
inline u64 step_rows(int cus) { return (u64)grid_of(cus) * BLOCK * 4 * BATCH; }

enum Row : uint32_t { ROW_NULL = 0, ROW_GATHERED = 1, ROW_OUT_OF_RANGE = 2 };

HJ_GATHER_FN Row classify(bool selected, uint32_t idx, uint32_t src_rows)
{
    if (!selected) return ROW_NULL;                     // garbage is legal in an unselected row's index and is not counted
    if (idx < src_rows) return ROW_GATHERED;
    return idx == NULL_VAL ? ROW_NULL : ROW_OUT_OF_RANGE;
}
}  // namespace hj_gather
