// cpp_wide_group_protocol.cpp - csrc/wide_group_layout.hpp on the CPU: the very walk of wide_group_kernel (find_slot) over atomic 64-bit
// words, raced by 16 threads, and the header's size rules.  Built once plain and once with -fsanitize=thread (tests/test_wide_group_protocol.py).
// The tuples are {0, 1, 0x80000000, 0xFFFFFFFF}^nkeys for nkeys 3 and 4: every prefix is shared by many tuples.  The table has twice as many
// slots as there are tuples and the home slot is cut to 4 bits, so the walks are long and collide all the time.  After every round: every
// tuple in exactly one slot, every occupied slot with nkeys non-zero words and zero words behind them, the counts add up to the inserts.
// Then the same under a claim limit (a workgroup's table), and a full table, which reports "no slot" and does not spin.  Prints "ok: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <thread>
#include <vector>

#include "wide_group_layout.hpp"

using namespace hj_wide;

static long cases = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// host memory: the builtins the sanitizer understands; `limit` slots may be claimed at most (the ticket rule of a workgroup's table)
struct HostMemory {
    uint32_t *used;
    uint32_t limit;
    u64 load(const u64 *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    u64 cas(u64 *p, u64 word)
    {
        u64 seen = 0;
        __atomic_compare_exchange_n(p, &seen, word, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return seen;
    }
    bool claim()
    {
        if (__atomic_load_n(used, __ATOMIC_RELAXED) >= limit) return false;
        if (__atomic_fetch_add(used, 1u, __ATOMIC_RELAXED) >= limit) { __atomic_fetch_sub(used, 1u, __ATOMIC_RELAXED); return false; }
        return true;
    }
    void unclaim() { __atomic_fetch_sub(used, 1u, __ATOMIC_RELAXED); }
};

static const uint32_t VALUES[4] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};

template <uint32_t NKEYS>
static void words_of(uint32_t id, u64 (&w)[MAX_KEYS])
{
    for (uint32_t c = 0; c < MAX_KEYS; ++c) w[c] = c < NKEYS ? key_word(VALUES[(id >> (2 * c)) & 3u]) : 0;
}

// a barrier of spinning threads, so that every round starts with all of them on an empty table
struct Gate {
    uint32_t arrived = 0, phase = 0;
    void wait(uint32_t threads)
    {
        const uint32_t my = __atomic_load_n(&phase, __ATOMIC_ACQUIRE);
        if (__atomic_add_fetch(&arrived, 1u, __ATOMIC_ACQ_REL) == threads) {
            __atomic_store_n(&arrived, 0u, __ATOMIC_RELAXED);
            __atomic_store_n(&phase, my + 1, __ATOMIC_RELEASE);
        } else {
            while (__atomic_load_n(&phase, __ATOMIC_ACQUIRE) == my) std::this_thread::yield();
        }
    }
};

template <uint32_t NKEYS>
static void race(uint32_t limit_divisor, int rounds, uint32_t inserts_per_thread)
{
    constexpr uint32_t THREADS = 16, TUPLES = 1u << (2 * NKEYS), SLOTS = 2 * TUPLES;
    const uint32_t limit = limit_divisor ? TUPLES / limit_divisor : SLOTS;
    std::vector<Slot> tab(SLOTS);
    uint32_t used = 0;
    u64 refused[THREADS];
    Gate gate;
    auto worker = [&](uint32_t t) {
        for (int r = 0; r < rounds; ++r) {
            gate.wait(THREADS + 1);                                     // the table is empty
            HostMemory mem{&used, limit};
            u64 none = 0;
            uint32_t x = 0x9E3779B1u * (t + 1) + (uint32_t)r;
            for (uint32_t i = 0; i < inserts_per_thread; ++i) {
                x = x * 1664525u + 1013904223u;
                // (the first inserts of a round: every thread the same few tuples, so that they race for the same empty slots)
                const uint32_t id = i < 8 ? (i * 85u + (uint32_t)r) % TUPLES : (x >> 8) % TUPLES;
                u64 w[MAX_KEYS];
                words_of<NKEYS>(id, w);
                const u64 h = hash(w);
                const u64 s = find_slot<NKEYS>(mem, tab.data(), SLOTS - 1, (h >> 60), SLOTS, w);        // the home slot: 4 bits
                if (s == NO_SLOT) ++none;
                else __atomic_fetch_add(&tab[s].count, 1ull, __ATOMIC_RELAXED);
            }
            refused[t] = none;
            gate.wait(THREADS + 1);                                     // every thread is through
        }
    };
    std::vector<std::thread> threads;
    for (uint32_t t = 0; t < THREADS; ++t) threads.emplace_back(worker, t);
    for (int r = 0; r < rounds; ++r) {
        memset((void *)tab.data(), 0, SLOTS * sizeof(Slot));
        used = 0;
        gate.wait(THREADS + 1);
        gate.wait(THREADS + 1);
        std::map<std::vector<u64>, uint32_t> where;
        u64 counted = 0, none = 0;
        uint32_t occupied = 0;
        for (uint32_t t = 0; t < THREADS; ++t) none += refused[t];
        for (uint32_t s = 0; s < SLOTS; ++s) {
            const Slot &e = tab[s];
            bool any = false;
            for (uint32_t c = 0; c < MAX_KEYS; ++c) any = any || e.key[c] != 0;
            if (!any) { REQUIRE(e.count == 0, "slot %u: a count without a tuple", s); continue; }
            ++occupied;
            for (uint32_t c = 0; c < MAX_KEYS; ++c) {
                if (c < NKEYS) REQUIRE((e.key[c] >> 32) == 1, "slot %u: word %u of an occupied slot is %llx", s, c, e.key[c]);
                else REQUIRE(e.key[c] == 0, "slot %u: word %u behind the tuple is %llx", s, c, e.key[c]);
            }
            std::vector<u64> t(e.key, e.key + MAX_KEYS);
            REQUIRE(!where.count(t), "a tuple in slots %u and %u", where[t], s);
            where[t] = s;
            REQUIRE(e.count > 0, "slot %u: a tuple that nobody counted", s);
            counted += e.count;
        }
        REQUIRE(counted + none == (u64)THREADS * inserts_per_thread, "round %d: %llu counted + %llu refused of %llu inserts", r, counted, none,
                (u64)THREADS * inserts_per_thread);
        REQUIRE(occupied <= limit && used == occupied, "round %d: %u slots occupied, %u claimed, limit %u", r, occupied, used, limit);
        if (!limit_divisor) REQUIRE(none == 0 && occupied == TUPLES, "round %d: %u of %u tuples, %llu refused", r, occupied, TUPLES, none);
        else REQUIRE(occupied == limit && none > 0, "round %d: the limited table holds %u of %u", r, occupied, limit);
        ++cases;
    }
    for (auto &t : threads) t.join();
}

// a table without an empty slot: a further tuple is told so after `probes` slots
template <uint32_t NKEYS>
static void full_table()
{
    constexpr uint32_t SLOTS = 8;
    Slot tab[SLOTS];
    memset((void *)tab, 0, sizeof(tab));
    uint32_t used = 0;
    HostMemory mem{&used, SLOTS};
    u64 w[MAX_KEYS];
    for (uint32_t id = 0; id < SLOTS; ++id) {
        words_of<NKEYS>(id * 5u, w);
        const u64 s = find_slot<NKEYS>(mem, tab, SLOTS - 1, hash(w), SLOTS, w);
        REQUIRE(s < SLOTS, "tuple %u of %u found no slot", id, SLOTS);
        REQUIRE(find_slot<NKEYS>(mem, tab, SLOTS - 1, hash(w), SLOTS, w) == s, "tuple %u: found again elsewhere", id);
    }
    REQUIRE(used == SLOTS, "%u slots claimed", used);
    words_of<NKEYS>(63u, w);
    REQUIRE(find_slot<NKEYS>(mem, tab, SLOTS - 1, hash(w), SLOTS, w) == NO_SLOT, "a ninth tuple in eight slots");
    REQUIRE(find_slot<NKEYS>(mem, tab, SLOTS - 1, hash(w), 3, w) == NO_SLOT, "a walk of three probes");
    for (uint32_t id = 0; id < SLOTS; ++id) {                          // and those inside are still found
        words_of<NKEYS>(id * 5u, w);
        REQUIRE(find_slot<NKEYS>(mem, tab, SLOTS - 1, hash(w), SLOTS, w) < SLOTS, "tuple %u lost", id);
    }
    ++cases;
}

static void sizes()
{
    static_assert(sizeof(Slot) == 72, "a slot is four key words, a count and four aggregate words");
    static_assert(LDS_BYTES <= LDS_BUDGET && LDS_BUDGET == 160 * 1024, "a workgroup's table fits the compute unit's LDS");
    static_assert(LDS_SLOTS == 2048 && LDS_GROUPS == 1024 && LDS_PROBES <= 256 && MAX_KEYS == 4 && MIN_KEYS == 3 && MAX_AGGS == 4, "the planned sizes");
    static_assert((LDS_SLOTS & (LDS_SLOTS - 1)) == 0 && LDS_SLOTS == 1u << LOG2_LDS_SLOTS, "a power of two");
    const u64 caps[] = {0, 1, 511, 512, 513, 1ull << 20};
    for (u64 cap : caps) {
        const u64 s = merge_slots(cap);
        REQUIRE(s >= 1024 && s >= 2 * cap && (s & (s - 1)) == 0, "merge_slots(%llu) = %llu", cap, s);
        REQUIRE(s == 1024 || s / 2 < 2 * cap, "merge_slots(%llu) = %llu is not the smallest", cap, s);
        REQUIRE(workspace_bytes(s) == 16 + s * 72, "workspace_bytes(%llu)", s);
        ++cases;
    }
    REQUIRE(merge_slots(512) == 1024 && merge_slots(513) == 2048, "the step at 512");
    REQUIRE(merge_slots(MAX_CAPACITY) == 2 * MAX_CAPACITY && merge_slots(MAX_CAPACITY + 1) == 0, "the capacity limit");
    REQUIRE(step_rows(256) == 256ull * BLOCK * 4 * BATCH && step_rows(0) == step_rows(1), "step_rows");
    // key words: never 0, the key comes back
    for (uint32_t v : VALUES) REQUIRE(key_word(v) != 0 && key_of(key_word(v)) == v && (key_word(v) >> 32) == 1, "key_word(%x)", v);
    // the hash depends on every key: a single changed key changes it, and the home slots of both tables see all four keys
    const uint32_t sample[][4] = {{0, 0, 0, 0}, {1, 2, 3, 4}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, {0x80000000u, 0, 1, 0xFFFFFFFFu}, {1997, 25, 7, 40}};
    for (const auto &t : sample) {
        u64 w[MAX_KEYS];
        for (uint32_t c = 0; c < MAX_KEYS; ++c) w[c] = key_word(t[c]);
        const u64 h = hash(w);
        for (uint32_t c = 0; c < MAX_KEYS; ++c) {
            uint32_t top = 0, low = 0;
            for (uint32_t bit = 0; bit < 32; ++bit) {
                u64 x[MAX_KEYS] = {w[0], w[1], w[2], w[3]};
                x[c] = key_word(t[c] ^ (1u << bit));
                const u64 g = hash(x);
                REQUIRE(g != h, "key %u bit %u does not reach the hash", c, bit);
                top += lds_home(g) != lds_home(h);
                low += (g & 1023) != (h & 1023);
                ++cases;
            }
            REQUIRE(top >= 28 && low >= 28, "key %u: %u / %u of 32 single-bit changes move the home slots", c, top, low);
        }
        // a three-key tuple: word 3 is 0
        u64 x[MAX_KEYS] = {w[0], w[1], w[2], 0};
        REQUIRE(hash(x) == hash(x) && lds_home(hash(x)) < LDS_SLOTS, "the hash of three keys");
    }
}

int main()
{
    sizes();
    full_table<3>();
    full_table<4>();
    race<3>(0, 30, 1000);
    race<4>(0, 30, 1500);
    race<3>(2, 10, 1000);                                               // a claim limit of half the tuples
    race<4>(2, 10, 1500);
    printf("ok: %ld cases\n", cases);
    return 0;
}
