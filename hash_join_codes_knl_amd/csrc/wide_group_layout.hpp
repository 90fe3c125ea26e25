// wide_group_layout.hpp - the tables of hjgpu_group_by with three and four key columns (gen_kernels.hip wide_group_kernel / wide_emit_kernel,
// DESIGN.md section 5 "Wide keys").  Plain host / device arithmetic, no HIP: the launchers and the kernels share it with
// tests/cpp_wide_group_protocol.cpp, which compiles it with g++ and runs the very walk of the kernels over std::atomic on the CPU.
//
// A slot is four 64-bit key words, a count and four aggregate words (agg_layout.hpp's).  Key word c of an occupied slot holds
// key_c | 1 << 32: it is never 0, whatever the key, so no tuple needs a slot of its own and zeroed memory is an empty table.  Words at index
// >= nkeys stay 0 and are never compared.
//
// INSERT-OR-FIND WITHOUT WAITING.  There is no compare-and-swap of a whole tuple, and a claim-then-publish state word would make the lanes of
// a wave wait for one another.  Instead a lane walks from its home slot, linear probing, and at a slot goes through words 0 ... nkeys - 1 in
// order: it loads the word; if that is 0 it tries a 64-bit compare-and-swap 0 -> its own word and takes what comes back; if the word is not
// its own it goes on to the next slot; if all nkeys words are its own, that is its slot.  A word only ever goes from 0 to a value, so what a
// lane has seen stays true, relaxed atomics suffice, and every lane of one tuple passes over the same slots and stops at the same one: the
// first slot on its path whose words end up all its own.  A word that a lane wrote into a slot which another tuple then won is simply a
// part of that tuple's prefix.  A lane that has written word c of a slot goes straight on to word c + 1 of the same slot, so once every
// lane is through no slot is half filled: a slot whose word 0 is not 0 holds nkeys words.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "group_layout.hpp"

namespace hj_wide {
typedef unsigned long long u64;

constexpr uint32_t MAX_KEYS = 4;                        // HJGPU_GROUP_BY_MAX_KEYS
constexpr uint32_t MIN_KEYS = 3;                        // fewer: hjgpu_group_agg's tables (group_layout.hpp)
constexpr uint32_t MAX_AGGS = 4;                        // HJGPU_AGG_MAX_AGGS

struct Slot {
    u64 key[MAX_KEYS];                                  // key c | 1 << 32; 0: empty (and every word at index >= nkeys)
    u64 count;
    u64 aggs[MAX_AGGS];
};

constexpr uint32_t BLOCK = 1024;                        // lanes per workgroup of the aggregation
constexpr uint32_t BATCH = 2;                           // wave trips (of hj_lookup.hpp: 256 rows) per wave and loop iteration
constexpr uint32_t LOG2_LDS_SLOTS = 11;
constexpr uint32_t LDS_SLOTS = 1u << LOG2_LDS_SLOTS;    // slots of a workgroup's table
constexpr uint32_t LDS_GROUPS = LDS_SLOTS / 2;          // hjgpu_get_counter "group_by_lds_groups": it claims no more slots than these
constexpr uint32_t LDS_PROBES = 256;                    // slots a row looks at before it goes to the merge table
constexpr size_t LDS_BUDGET = 160 * 1024;               // bytes of LDS of a gfx950 compute unit
constexpr size_t LDS_BYTES = (size_t)LDS_SLOTS * sizeof(Slot) + 16;     // the table, the claim counter and padding

constexpr u64 MIN_MERGE_SLOTS = 1024;
constexpr u64 MAX_CAPACITY = 1ull << 40;                // hj_group::MAX_CAPACITY
constexpr u64 NO_SLOT = 1ull << 62;                     // find_slot: the walk ended without a slot

// hjgpu_get_counter "group_by_step_rows": the rows the whole grid (one workgroup per compute unit) covers in one loop iteration
inline u64 step_rows(int cus) { return (u64)(cus < 1 ? 1 : cus) * BLOCK * 4 * BATCH; }

// the merge table's slots: a power of two, at least 2 * capacity and at least MIN_MERGE_SLOTS (0: capacity > MAX_CAPACITY)
inline u64 merge_slots(u64 capacity)
{
    if (capacity > MAX_CAPACITY) return 0;
    u64 s = MIN_MERGE_SLOTS;
    while (s < 2 * capacity) s <<= 1;
    return s;
}

// The context's workspace: the blocking form's count word, the overflow word, then merge_slots slots
constexpr size_t WORKSPACE_HEAD = 16;
inline u64 workspace_bytes(u64 slots) { return WORKSPACE_HEAD + slots * sizeof(Slot); }

HJ_GROUP_HD inline u64 key_word(uint32_t key) { return (u64)key | (1ull << 32); }
HJ_GROUP_HD inline uint32_t key_of(u64 word) { return (uint32_t)word; }

// 64 well-mixed bits of a tuple's key words (those at index >= nkeys are 0): for any three keys fixed it is a bijection of the fourth's
// pair, so two tuples that differ in one key never share all 64 bits.  A workgroup's table takes the top LOG2_LDS_SLOTS, the merge
// table the low ones
HJ_GROUP_HD inline u64 hash(const u64 (&w)[MAX_KEYS])
{
    const u64 t01 = (u64)key_of(w[0]) | ((u64)key_of(w[1]) << 32), t23 = (u64)key_of(w[2]) | ((u64)key_of(w[3]) << 32);
    return hj_group::mix(hj_group::mix(t01) + t23 * 0x9E3779B97F4A7C15ull);
}
HJ_GROUP_HD inline uint32_t lds_home(u64 h) { return (uint32_t)(h >> (64 - LOG2_LDS_SLOTS)); }

// The walk (see the head of this file).  `tab` has mask + 1 slots, a power of two; the walk starts at `home & mask` and looks at no more
// than `probes` slots; w[c] = key_word(key c) for c < NKEYS.  Returns the slot's index, or NO_SLOT.  A is the memory the table lies in:
//   u64 load(const u64 *p)         a relaxed atomic load;
//   u64 cas(u64 *p, u64 word)      a relaxed 64-bit compare-and-swap 0 -> word that returns what the word held before;
//   bool claim() / void unclaim()  asked before word 0 of an empty slot is written (false: the table takes no further tuple, the walk ends
//                                  with NO_SLOT) and taken back when that write lost - a workgroup's table counts its slots with them.
template <uint32_t NKEYS, class A>
HJ_GROUP_HD inline u64 find_slot(A &mem, Slot *tab, u64 mask, u64 home, u64 probes, const u64 (&w)[MAX_KEYS])
{
    static_assert(NKEYS >= 1 && NKEYS <= MAX_KEYS, "one to four key words");
    u64 s = home & mask;
    for (u64 p = 0; p < probes; ++p) {
        // (all the slot's words are loaded before the first is looked at: one round trip to the table where the tuple is found, which
        // is the common case.  A word loaded early is as good as one loaded late - it is 0, and the compare-and-swap then tells, or it
        // is final)
        u64 seen[NKEYS];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t c = 0; c < NKEYS; ++c) seen[c] = mem.load(&tab[s].key[c]);
        bool mine = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t c = 0; c < NKEYS; ++c) {
            u64 cur = seen[c];
            if (cur == 0) {
                if (c == 0 && !mem.claim()) return NO_SLOT;
                cur = mem.cas(&tab[s].key[c], w[c]);
                if (cur == 0) cur = w[c];
                else if (c == 0) mem.unclaim();
            }
            if (cur != w[c]) { mine = false; break; }
        }
        if (mine) return s;
        s = (s + 1) & mask;
    }
    return NO_SLOT;
}
}  // namespace hj_wide
