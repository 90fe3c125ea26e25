// compact_layout.hpp - how hjgpu_compact_selected cuts its rows (gen_kernels.hip compact_count_kernel / compact_kernel, DESIGN.md section 5
// "Compaction by bitmap").  Plain host arithmetic, no HIP: the launchers and the kernels share it with tests/test_compact_layout.py, which
// compiles it with g++ and walks the ranges on the CPU.
//
// The rows [0, n) are cut into `ranges` contiguous ranges, one per workgroup of both launches.  A range is a whole number of chunks - a
// chunk is what one workgroup compacts per loop iteration, CHUNK_ROWS = BLOCK lanes x 4 rows x VEC vectors - so every range starts at a
// multiple of 256 rows: at a 16-byte boundary of the mask and of every column.  The last non-empty range holds the tail, the ranges behind
// it are empty ([n, n)).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hj_compact {
typedef unsigned long long u64;

constexpr uint32_t BLOCK = 256;                         // lanes per workgroup
constexpr uint32_t VEC = 2;                             // 16-byte vectors per lane, column and iteration
constexpr uint32_t CHUNK_ROWS = BLOCK * 4 * VEC;        // hjgpu_get_counter "compact_chunk_rows"
constexpr uint32_t MAX_RANGES = 2048;
constexpr uint32_t RESIDENT = 8;                        // workgroups of BLOCK lanes a CU holds at once

// hjgpu_get_counter "compact_ranges": the grid of both launches
inline uint32_t ranges_of(int cus)
{
    const u64 g = (u64)(cus < 1 ? 1 : cus) * RESIDENT;
    return (uint32_t)(g < MAX_RANGES ? g : MAX_RANGES);
}

struct Layout {
    u64 n;
    u64 range_rows;         // a multiple of CHUNK_ROWS (0 when n == 0)
    uint32_t ranges;
#if defined(__HIPCC__)
    __host__ __device__
#endif
    u64 begin(uint32_t g) const
    {
        // (g * range_rows < n + ranges * CHUNK_ROWS wherever it matters: the product is only formed below n / range_rows + 1)
        if (range_rows == 0 || g > n / range_rows) return n;
        return (u64)g * range_rows;
    }
#if defined(__HIPCC__)
    __host__ __device__
#endif
    u64 end(uint32_t g) const
    {
        const u64 b = begin(g);
        return n - b < range_rows ? n : b + range_rows;
    }
};

inline Layout layout(u64 n, uint32_t ranges)
{
    Layout l;
    l.n = n; l.ranges = ranges ? ranges : 1;
    const u64 chunks = n / CHUNK_ROWS + (n % CHUNK_ROWS ? 1 : 0);
    const u64 per = chunks / l.ranges + (chunks % l.ranges ? 1 : 0);
    l.range_rows = per * CHUNK_ROWS;
    return l;
}

// the mask words [first, last) that the count pass of range g reads; last <= (n + 31) / 32
inline void count_words(const Layout &l, uint32_t g, u64 *first, u64 *last)
{
    const u64 b = l.begin(g), e = l.end(g);
    *first = b >> 5;
    *last = (e >> 5) + ((e & 31) ? 1 : 0);
    if (e <= b) *last = *first;
}
}  // namespace hj_compact
