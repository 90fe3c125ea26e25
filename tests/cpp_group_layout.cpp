// CPU test of hash_join_codes_knl_amd/csrc/group_layout.hpp (compiled and run by tests/test_group_layout.py): the size rules of
// hjgpu_group_sum's tables.  The merge table has a power of two of at least 2 * capacity and at least 1024 hashed slots, for capacities 0,
// 1, 511, 512, 513, 2^20, 2^32 and around every power of two up to the largest legal capacity; its workspace's bytes fit 64 bits (128-bit
// arithmetic beside the header's, and the sanitizer, say so).  A slot is 48 bytes with the count right behind the tuple and the sums behind
// the count (the kernels address count and sums as words 0 ... 4 behind the tuple); a workgroup's table - the hashed slots, the slot of
// tuple 0, the claim counter - fits the LDS of a compute unit, claims at most half of its hashed slots, and its home slots stay inside it.
#include <stddef.h>
#include <stdio.h>
#include "group_layout.hpp"

using hj_group::u64;
typedef unsigned __int128 u128;

static int fail(const char *what, u64 x)
{
    fprintf(stderr, "FAIL: %s (%llu)\n", what, x);
    return 1;
}

static int check_capacity(u64 capacity)
{
    const u64 s = hj_group::merge_slots(capacity);
    if (capacity > hj_group::MAX_CAPACITY) return s == 0 ? 0 : fail("a capacity beyond the limit has a table", capacity);
    if (s == 0) return fail("a legal capacity has no table", capacity);
    if (s & (s - 1)) return fail("the slot count is no power of two", capacity);
    if (s < hj_group::MIN_MERGE_SLOTS) return fail("fewer than the minimum slots", capacity);
    if ((u128)s < (u128)2 * capacity) return fail("fewer than 2 * capacity slots", capacity);
    if (s > hj_group::MIN_MERGE_SLOTS && (u128)(s / 2) >= (u128)2 * capacity) return fail("twice the slots the rule asks for", capacity);
    const u128 bytes = (u128)hj_group::WORKSPACE_HEAD + ((u128)s + 1) * sizeof(hj_group::Slot);
    if (bytes >> 63) return fail("the workspace's bytes leave 63 bits", capacity);
    if ((u128)hj_group::workspace_bytes(s) != bytes) return fail("workspace_bytes differs from the 128-bit arithmetic", capacity);
    return 0;
}

int main()
{
    using namespace hj_group;
    if (sizeof(Slot) != 48 || offsetof(Slot, tuple) != 0 || offsetof(Slot, count) != 8 || offsetof(Slot, sums) != 16 || sizeof(Slot) % 16)
        return fail("slot layout", sizeof(Slot));
    if (MAX_KEYS != 2 || MAX_VALS != 4 || sizeof(((Slot *)0)->sums) != 8 * MAX_VALS) return fail("slot columns", MAX_VALS);
    if (WORKSPACE_HEAD % 16 || WORKSPACE_HEAD < 12) return fail("workspace head", WORKSPACE_HEAD);
    if (LDS_SLOTS != (1u << LOG2_LDS_SLOTS) || LDS_GROUPS < 1 || LDS_GROUPS * 2 > LDS_SLOTS) return fail("LDS table geometry", LDS_SLOTS);
    if (LDS_BYTES != ((size_t)LDS_SLOTS + 1) * sizeof(Slot) + 16 || LDS_BYTES > LDS_BUDGET) return fail("the LDS table exceeds the budget", LDS_BYTES);
    if (LDS_PROBES < 1 || LDS_PROBES > LDS_SLOTS || BLOCK % 64 || BLOCK > 1024) return fail("probe bound / block", LDS_PROBES);
    size_t cases = 0;
    const u64 asked[] = {0, 1, 511, 512, 513, 1ull << 20, 1ull << 32};
    const u64 slots[] = {1024, 1024, 1024, 1024, 2048, 1ull << 21, 1ull << 33};
    for (int i = 0; i < 7; ++i) {
        if (check_capacity(asked[i])) return 1;
        if (merge_slots(asked[i]) != slots[i]) return fail("merge_slots", asked[i]);
        ++cases;
    }
    for (int b = 0; b <= 40; ++b)
        for (long long d = -2; d <= 2; ++d) {
            const u64 c = (1ull << b) + (u64)d;
            if ((long long)(1ull << b) + d < 0) continue;
            if (check_capacity(c)) return 1;
            ++cases;
        }
    if (check_capacity(~0ull) || check_capacity(1ull << 63) || check_capacity((1ull << 63) + 1)) return 1;
    // the hash: home slots inside the table, tuple_of is the documented packing, and the tuples of a small dense domain spread out
    if (tuple_of(0, 0) != 0 || tuple_of(0xFFFFFFFFu, 0) != 0xFFFFFFFFull || tuple_of(1, 2) != 0x200000001ull) return fail("tuple_of", 0);
    unsigned used[LDS_SLOTS] = {0};
    unsigned most = 0;
    for (uint32_t k = 0; k < LDS_GROUPS; ++k) {
        const uint32_t h = lds_home(mix(tuple_of(k, 7)));
        if (h >= LDS_SLOTS) return fail("a home slot outside the table", h);
        if (++used[h] > most) most = used[h];
    }
    if (most > 8) return fail("a dense key range piles up in one home slot", most);
    printf("ok: %zu capacities\n", cases);
    return 0;
}
