// wide_lookup_layout.hpp - the table of hjgpu_lookup_wide, the positional look-up on two to four key columns (gen_kernels.hip
// wide_lookup_build_kernel / wide_lookup_kernel, DESIGN.md section 5 "Wide look-up").  Plain host / device arithmetic, no HIP: the
// launchers and the kernels share it with tests/cpp_wide_lookup_protocol.cpp, which compiles it with g++ and runs the very walk of the
// kernels over atomic claim words on the CPU.
//
// A slot starts with one 64-bit claim word, payload | 1 << 32: it is 0 while the slot is empty and never 0 afterwards, whatever the payload,
// so zeroed memory is an empty table.  The key words follow as uint32: two of them fill a 16-byte slot, three and four a 32-byte slot whose
// unused words stay 0.  A slot is aligned to its size: one or two 16-byte loads from one 128-byte line.
//
// CLAIM, THEN STORE.  The build never compares a key: a lane walks from its tuple's home slot, linear probing with wrap-around, tries one
// 64-bit compare-and-swap 0 -> its claim word at each slot, stores its key words into the slot it won and is done; a loser goes on to the
// next slot.  So duplicated tuples take a slot each, no lane ever waits for another lane's store, and a slot's key words are written by one
// lane only.  Nobody reads a slot during the build: the look-up is a later launch on the same stream, and by then every claimed slot holds
// its keys.  (hjgpu_group_by's table - wide_group_layout.hpp - must FIND a tuple while others insert it, which is why its key words are
// claimed one by one; a look-up table is only ever filled and then only ever read.)
// The table has more slots than build rows, so there is always an empty slot and every walk ends.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "group_layout.hpp"

namespace hj_wlk {
typedef unsigned long long u64;

constexpr uint32_t MIN_KEYS = 2;                        // HJGPU_LOOKUP_WIDE_MIN_KEYS (one key column: hjgpu_lookup_selected)
constexpr uint32_t MAX_KEYS = 4;                        // HJGPU_LOOKUP_WIDE_MAX_KEYS
constexpr uint32_t NULL_VAL = 0xFFFFFFFFu;              // HJGPU_NULL_VAL

template <uint32_t NKEYS>
struct Slot {
    static_assert(NKEYS >= MIN_KEYS && NKEYS <= MAX_KEYS, "two to four key words");
    u64 claim;                                          // payload | 1 << 32; 0: empty
    uint32_t key[NKEYS == 2 ? 2 : 6];                   // the key words, then (three and four keys) words that stay 0
};
static_assert(sizeof(Slot<2>) == 16 && sizeof(Slot<3>) == 32 && sizeof(Slot<4>) == 32, "a slot is one or two 16-byte vectors");

constexpr size_t slot_bytes(uint32_t nkeys) { return nkeys == 2 ? 16 : 32; }

constexpr uint32_t BLOCK = 256;                         // lanes per workgroup of either kernel
constexpr uint32_t BATCH = 2;                           // wave trips (of hj_lookup.hpp: 256 rows) per wave and loop iteration of the look-up
constexpr uint32_t RESIDENT = 4;                        // workgroups of BLOCK lanes per CU in the look-up's persistent grid: the waves per SIMD that
                                                        // every instance, the four-key ones at 120 VGPRs included, holds
constexpr uint32_t BUILD_RESIDENT = 8;                  // the same for the build

constexpr double DEFAULT_LOAD = 0.5, MAX_LOAD = 0.99;
constexpr u64 MIN_SLOTS = 16;
constexpr u64 NO_SLOT = 1ull << 62;                     // insert: the walk went once round a table without an empty slot (the launcher refuses such a table)

inline uint32_t grid_of(int cus) { return (uint32_t)(cus < 1 ? 1 : cus) * RESIDENT; }
// hjgpu_get_counter "lookup_wide_step_rows": the rows the look-up's whole grid covers in one iteration of its loop
inline u64 step_rows(int cus) { return (u64)grid_of(cus) * BLOCK * 4 * BATCH; }

// the table's slots for `inner` build rows at `load` (0: DEFAULT_LOAD; the entry point refuses load > MAX_LOAD): max(16, inner + 1,
// floor(inner / load)) rounded up to a multiple of 8.  inner == 0: no table at all
inline u64 slots_of(u64 inner, double load)
{
    if (inner == 0) return 0;
    if (!(load > 0)) load = DEFAULT_LOAD;
    u64 r = (u64)((double)inner / load);
    if (r < inner + 1) r = inner + 1;
    if (r < MIN_SLOTS) r = MIN_SLOTS;
    return (r + 7) / 8 * 8;
}

// The context's workspace: the call's four aggregate words (an hjgpu_result) in a line of their own, then the table
constexpr size_t WORKSPACE_HEAD = 128;
inline u64 workspace_bytes(u64 slots, uint32_t nkeys) { return WORKSPACE_HEAD + slots * slot_bytes(nkeys); }

HJ_GROUP_HD inline u64 claim_word(uint32_t payload) { return (u64)payload | (1ull << 32); }
HJ_GROUP_HD inline uint32_t payload_of(u64 claim) { return (uint32_t)claim; }

// 64 well-mixed bits of a tuple (wide_group_layout.hpp's hash over the plain key words; a missing pair is 0): for any other keys fixed it
// is a bijection of one pair, so two tuples that differ in one key never share all 64 bits
template <uint32_t NKEYS>
HJ_GROUP_HD inline u64 hash(const uint32_t (&k)[NKEYS])
{
    const u64 t01 = (u64)k[0] | ((u64)k[1] << 32);
    u64 t23 = 0;
    if constexpr (NKEYS > 2) t23 = (u64)k[2];
    if constexpr (NKEYS > 3) t23 |= (u64)k[3] << 32;
    return hj_group::mix(hj_group::mix(t01) + t23 * 0x9E3779B97F4A7C15ull);
}

// the home slot: the high half of the 128-bit product of the hash and the slot count - below `slots` for any slot count
HJ_GROUP_HD inline u64 home(u64 h, u64 slots)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(h, slots);
#else
    return (u64)(((unsigned __int128)h * slots) >> 64);
#endif
}
HJ_GROUP_HD inline u64 next(u64 s, u64 slots) { return s + 1 == slots ? 0 : s + 1; }

// what a walk does with the slot it has loaded: the claim word 0 ends it without a match, all key words equal end it with the payload in
// the claim word's low half, anything else sends it to the next slot
enum Step : uint32_t { STEP_MISS = 0, STEP_HIT = 1, STEP_NEXT = 2 };
template <uint32_t NKEYS>
HJ_GROUP_HD inline Step judge(u64 claim, const uint32_t (&seen)[NKEYS], const uint32_t (&k)[NKEYS])
{
    if (claim == 0) return STEP_MISS;
    bool same = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t c = 0; c < NKEYS; ++c) same = same && seen[c] == k[c];
    return same ? STEP_HIT : STEP_NEXT;
}

// The two walks.  `tab` has `slots` slots; A is the memory the table lies in:
//   u64 cas(u64 *claim, u64 word)                                 a relaxed 64-bit compare-and-swap 0 -> word that returns what the word held before;
//   void store_pair(uint32_t *p, uint32_t lo, uint32_t hi)        plain stores of two neighbouring key words (p is 8-byte aligned);
//   void load(const Slot<NKEYS> *s, u64 &claim, uint32_t (&seen)[NKEYS])   plain loads of a whole slot.
// insert: returns the slot the row took (NO_SLOT: a table without an empty slot - slots_of never makes one).
template <uint32_t NKEYS, class A>
HJ_GROUP_HD inline u64 insert(A &mem, Slot<NKEYS> *tab, u64 slots, const uint32_t (&k)[NKEYS], uint32_t payload)
{
    const u64 word = claim_word(payload);
    u64 s = home(hash<NKEYS>(k), slots);
    for (u64 p = 0; p < slots; ++p) {
        if (mem.cas(&tab[s].claim, word) == 0) {
            mem.store_pair(&tab[s].key[0], k[0], k[1]);
            if constexpr (NKEYS == 3) mem.store_pair(&tab[s].key[2], k[2], 0u);
            if constexpr (NKEYS == 4) mem.store_pair(&tab[s].key[2], k[2], k[3]);
            return s;
        }
        s = next(s, slots);
    }
    return NO_SLOT;
}

// find: true and the payload of the first slot on the tuple's path that holds it, false at the first empty slot.  (wide_lookup_kernel walks
// four rows at once - home, the loads of all four, judge, next - so that four slots are in flight: the same steps, interleaved)
template <uint32_t NKEYS, class A>
HJ_GROUP_HD inline bool find(A &mem, const Slot<NKEYS> *tab, u64 slots, const uint32_t (&k)[NKEYS], uint32_t *payload)
{
    if (slots == 0) return false;
    u64 s = home(hash<NKEYS>(k), slots);
    for (u64 p = 0; p < slots; ++p) {
        u64 claim;
        uint32_t seen[NKEYS];
        mem.load(&tab[s], claim, seen);
        const Step st = judge<NKEYS>(claim, seen, k);
        if (st == STEP_HIT) { *payload = payload_of(claim); return true; }
        if (st == STEP_MISS) return false;
        s = next(s, slots);
    }
    return false;
}
}  // namespace hj_wlk
