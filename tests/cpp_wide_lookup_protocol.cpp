// cpp_wide_lookup_protocol.cpp - csrc/wide_lookup_layout.hpp on the CPU: the very insert of wide_lookup_build_kernel over atomic claim words,
// raced by 16 threads, then the very find of wide_lookup_kernel once the threads have joined, and the header's size rules.  Built once plain
// and once with -fsanitize=thread (tests/test_wide_lookup_protocol.py).  The tuples are {0, 1, 0x80000000, 0xFFFFFFFF}^nkeys for nkeys 2, 3
// and 4: every prefix is shared by many tuples.  Every other tuple is inserted, every third of those three times; the table has the default
// load's slots, or inserts + 1 slots, where the walks wrap round.  Afterwards: every inserted tuple is found with the payload of one of its
// copies, every other tuple is a miss, as many slots are occupied as rows were inserted, the unused key words are 0.  Prints "ok: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <thread>
#include <vector>

#include "wide_lookup_layout.hpp"

using namespace hj_wlk;

static long cases = 0;
#define REQUIRE(cond, ...) do { ++cases; if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// host memory: the claim through the builtin the sanitizer understands, the key words plain - a slot's keys are written by its winner alone
// and read only after the threads have joined
struct HostMemory {
    u64 cas(u64 *p, u64 word)
    {
        u64 seen = 0;
        __atomic_compare_exchange_n(p, &seen, word, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return seen;
    }
    void store_pair(uint32_t *p, uint32_t lo, uint32_t hi) { p[0] = lo; p[1] = hi; }
    template <uint32_t NKEYS>
    void load(const Slot<NKEYS> *s, u64 &claim, uint32_t (&seen)[NKEYS])
    {
        claim = s->claim;
        for (uint32_t c = 0; c < NKEYS; ++c) seen[c] = s->key[c];
    }
};

static const uint32_t VALUES[4] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};

template <uint32_t NKEYS>
static void tuple_of(uint32_t id, uint32_t (&k)[NKEYS])
{
    for (uint32_t c = 0; c < NKEYS; ++c) k[c] = VALUES[(id >> (2 * c)) & 3u];
}

struct Row { uint32_t id, payload; };

template <uint32_t NKEYS>
static void race(bool tight)
{
    constexpr uint32_t THREADS = 16, TUPLES = 1u << (2 * NKEYS);
    // every other tuple (by a bit pattern that cuts through every column), every third of those three times; the payloads include 0 and
    // 0xFFFFFFFF and tell the copies apart
    std::vector<Row> rows;
    std::vector<std::set<uint32_t>> payloads(TUPLES);
    uint32_t taken = 0;
    for (uint32_t id = 0; id < TUPLES; ++id) {
        if (__builtin_popcount(id) & 1) continue;
        const uint32_t copies = taken++ % 3 == 0 ? 3 : 1;
        for (uint32_t c = 0; c < copies; ++c) {
            const uint32_t payload = rows.empty() ? 0u : rows.size() == 1 ? 0xFFFFFFFFu : id * 16u + c;
            rows.push_back({id, payload});
            payloads[id].insert(payload);
        }
    }
    const u64 inserts = rows.size();
    const u64 slots = tight ? inserts + 1 : slots_of(inserts, 0.0);
    std::vector<Slot<NKEYS>> tab(slots);
    memset(tab.data(), 0, slots * sizeof(Slot<NKEYS>));
    std::vector<u64> took(inserts, NO_SLOT);
    auto worker = [&](uint32_t t) {
        HostMemory mem;
        for (u64 i = t; i < inserts; i += THREADS) {
            uint32_t k[NKEYS];
            tuple_of<NKEYS>(rows[i].id, k);
            took[i] = insert<NKEYS>(mem, tab.data(), slots, k, rows[i].payload);
        }
    };
    std::vector<std::thread> threads;
    for (uint32_t t = 0; t < THREADS; ++t) threads.emplace_back(worker, t);
    for (auto &th : threads) th.join();

    std::set<u64> distinct;
    for (u64 i = 0; i < inserts; ++i) {
        REQUIRE(took[i] < slots, "nkeys %u row %llu took no slot", NKEYS, i);
        distinct.insert(took[i]);
    }
    REQUIRE(distinct.size() == inserts, "nkeys %u: %zu slots for %llu rows", NKEYS, distinct.size(), inserts);
    u64 occupied = 0;
    for (u64 s = 0; s < slots; ++s) {
        const Slot<NKEYS> &x = tab[s];
        if (x.claim == 0) {
            for (uint32_t c = 0; c < sizeof(x.key) / 4; ++c) REQUIRE(x.key[c] == 0, "nkeys %u: empty slot %llu holds a key word", NKEYS, s);
            continue;
        }
        ++occupied;
        REQUIRE((x.claim >> 32) == 1, "nkeys %u: claim word %llx of slot %llu", NKEYS, x.claim, s);
        for (uint32_t c = NKEYS; c < sizeof(x.key) / 4; ++c) REQUIRE(x.key[c] == 0, "nkeys %u: unused word %u of slot %llu is not 0", NKEYS, c, s);
    }
    REQUIRE(occupied == inserts, "nkeys %u: %llu occupied slots, %llu inserts", NKEYS, occupied, inserts);
    if (tight) REQUIRE(occupied == slots - 1, "the tight table has one empty slot");
    HostMemory mem;
    for (uint32_t id = 0; id < TUPLES; ++id) {
        uint32_t k[NKEYS], payload = 0x12345678u;
        tuple_of<NKEYS>(id, k);
        const bool hit = find<NKEYS>(mem, tab.data(), slots, k, &payload);
        if (payloads[id].empty()) REQUIRE(!hit, "nkeys %u: tuple %u was never inserted and is found", NKEYS, id);
        else {
            REQUIRE(hit, "nkeys %u: tuple %u is not found", NKEYS, id);
            REQUIRE(payloads[id].count(payload) == 1, "nkeys %u: tuple %u found with payload %x of another tuple", NKEYS, id, payload);
            uint32_t again = 0;
            REQUIRE(find<NKEYS>(mem, tab.data(), slots, k, &again) && again == payload, "nkeys %u: tuple %u: a second walk ends elsewhere", NKEYS, id);
        }
    }
    // no table at all: every tuple is a miss
    uint32_t k[NKEYS], payload;
    tuple_of<NKEYS>(5, k);
    REQUIRE(!find<NKEYS>(mem, (const Slot<NKEYS> *)nullptr, 0, k, &payload), "a look-up without a table is a miss");
}

static u64 formula(u64 inner, double load)
{
    if (inner == 0) return 0;
    u64 r = (u64)((double)inner / load);
    if (r < inner + 1) r = inner + 1;
    if (r < 16) r = 16;
    return (r + 7) / 8 * 8;
}

int main()
{
    // the sizes
    REQUIRE(sizeof(Slot<2>) == 16 && alignof(Slot<2>) == 8 && slot_bytes(2) == 16, "a two-key slot is 16 bytes");
    REQUIRE(sizeof(Slot<3>) == 32 && slot_bytes(3) == 32, "a three-key slot is 32 bytes");
    REQUIRE(sizeof(Slot<4>) == 32 && slot_bytes(4) == 32, "a four-key slot is 32 bytes");
    REQUIRE(offsetof(Slot<2>, key) == 8 && offsetof(Slot<4>, key) == 8, "the key words follow the claim word");
    REQUIRE(WORKSPACE_HEAD % 128 == 0 && workspace_bytes(0, 2) == WORKSPACE_HEAD && workspace_bytes(24, 3) == WORKSPACE_HEAD + 24 * 32, "the workspace");
    for (u64 inner : {0ull, 1ull, 15ull, 16ull, 1000ull}) {
        for (double load : {0.5, 0.99}) {
            const u64 s = slots_of(inner, load);
            REQUIRE(s == formula(inner, load), "slots_of(%llu, %g) = %llu", inner, load, s);
            REQUIRE(inner == 0 ? s == 0 : (s % 8 == 0 && s >= 16 && s > inner), "slots_of(%llu, %g) = %llu", inner, load, s);
        }
        REQUIRE(slots_of(inner, 0.0) == slots_of(inner, 0.5), "load 0 is 0.5");
    }
    REQUIRE(slots_of(1, 0.5) == 16 && slots_of(15, 0.99) == 16 && slots_of(16, 0.99) == 24 && slots_of(16, 0.5) == 32, "small tables");
    REQUIRE(slots_of(1000, 0.5) == 2000 && slots_of(1000, 0.99) == 1016, "slots_of(1000)");
    // the claim word is never 0 and keeps every payload; the home slot lies inside any table
    for (uint32_t p : {0u, 1u, 0x80000000u, 0xFFFFFFFFu}) REQUIRE(claim_word(p) != 0 && payload_of(claim_word(p)) == p, "claim word of %x", p);
    for (u64 h : {0ull, 1ull, ~0ull, 0x8000000000000000ull})
        for (u64 s : {1ull, 16ull, 1016ull, (1ull << 40) + 8}) REQUIRE(home(h, s) < s, "home(%llx, %llu)", h, s);
    REQUIRE(home(~0ull, 16) == 15 && home(0, 16) == 0 && next(15, 16) == 0 && next(3, 16) == 4, "home and next");
    // (a, b) and (b, a) are different tuples to the hash
    { const uint32_t ab[2] = {1, 2}, ba[2] = {2, 1}; REQUIRE(hash<2>(ab) != hash<2>(ba), "the hash is positional"); }

    for (int round = 0; round < 20; ++round) {
        for (bool tight : {false, true}) {
            race<2>(tight);
            race<3>(tight);
            race<4>(tight);
        }
    }
    printf("ok: %ld cases\n", cases);
    return 0;
}
