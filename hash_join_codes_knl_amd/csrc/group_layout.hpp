// group_layout.hpp - the tables of hjgpu_group_sum (gen_kernels.hip group_sum_kernel / group_emit_kernel, DESIGN.md section 5 "Grouped
// aggregation").  Plain host / device arithmetic, no HIP: the launchers and the kernels share it with tests/test_group_layout.py, which
// compiles it with g++ and checks the size rules on the CPU.
//
// A slot is the key tuple in one 64-bit word (key 0 low, key 1 high; 0 with one key column), a count and four sums.  Both tables - a
// workgroup's in LDS, the merge table in device memory - are open-addressed arrays of such slots with linear probing, followed by ONE MORE
// slot at index `slots`: the slot of the tuple whose word is 0.  A hashed slot is occupied when its tuple word is not 0 - insert-or-find is
// one 64-bit compare-and-swap of that word, nobody ever waits for a half-written slot - and the tuple 0, which that word cannot tell from
// "empty", has its own slot, whose occupancy state is its count (a group has at least one row).  So every key value is legal.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HJ_GROUP_HD __host__ __device__
#else
#define HJ_GROUP_HD
#endif

namespace hj_group {
typedef unsigned long long u64;

constexpr uint32_t MAX_KEYS = 2;                        // HJGPU_GROUP_MAX_KEYS
constexpr uint32_t MAX_VALS = 4;                        // HJGPU_GROUP_MAX_VALS

struct Slot {
    u64 tuple;                                          // key 0 | key 1 << 32; 0: empty (hashed slots), unused in the slot of tuple 0
    u64 count;
    u64 sums[MAX_VALS];
};

constexpr uint32_t BLOCK = 1024;                        // lanes per workgroup of the aggregation
constexpr uint32_t LOG2_LDS_SLOTS = 11;
constexpr uint32_t LDS_SLOTS = 1u << LOG2_LDS_SLOTS;    // hashed slots of a workgroup's table
constexpr uint32_t LDS_GROUPS = LDS_SLOTS / 2;          // hjgpu_get_counter "group_lds_groups": it claims no more hashed slots than these
constexpr uint32_t LDS_PROBES = 256;                    // slots a row looks at before it goes to the merge table (an empty slot ends the walk: the table is at most half full)
constexpr size_t LDS_BUDGET = 160 * 1024;               // bytes of LDS of a gfx950 compute unit
constexpr size_t LDS_BYTES = ((size_t)LDS_SLOTS + 1) * sizeof(Slot) + 16;      // the table, the slot of tuple 0, the claim counter

constexpr u64 MIN_MERGE_SLOTS = 1024;
constexpr u64 MAX_CAPACITY = 1ull << 40;                // beyond it the merge table's bytes leave 64 bits' comfortable range: no such device

// the merge table's hashed slots: a power of two, at least 2 * capacity and at least MIN_MERGE_SLOTS (0: capacity > MAX_CAPACITY)
inline u64 merge_slots(u64 capacity)
{
    if (capacity > MAX_CAPACITY) return 0;
    u64 s = MIN_MERGE_SLOTS;
    while (s < 2 * capacity) s <<= 1;
    return s;
}

// The context's workspace: the blocking form's count word, the overflow word, then merge_slots + 1 slots
constexpr size_t WORKSPACE_HEAD = 16;
inline u64 workspace_bytes(u64 slots) { return WORKSPACE_HEAD + (slots + 1) * sizeof(Slot); }

HJ_GROUP_HD inline u64 tuple_of(uint32_t k0, uint32_t k1) { return (u64)k0 | ((u64)k1 << 32); }

// 64 well-mixed bits of a tuple: a workgroup's table takes the top LOG2_LDS_SLOTS, the merge table the low ones
HJ_GROUP_HD inline u64 mix(u64 x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
HJ_GROUP_HD inline uint32_t lds_home(u64 h) { return (uint32_t)(h >> (64 - LOG2_LDS_SLOTS)); }
}  // namespace hj_group
