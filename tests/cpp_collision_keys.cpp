// cpp_collision_keys.cpp - the hashes and homes of key tuples, computed by the grouped operators' own headers (group_layout.hpp,
// wide_group_layout.hpp), for tests/test_collision_keys.py: it pins tests/collision_keys.py - a numpy port of these functions and the
// crafted tuples of tests/test_gpu_group_collisions.py - to what the kernels compute.
//
//   cpp_collision_keys IN OUT
// IN:  uint32 nkeys (1 .. 4), uint32 count, then count tuples of four uint32 keys (those at index >= nkeys are 0).
// OUT: per tuple four uint64: hj_group::mix(tuple_of(key 0, key 1)), its hj_group::lds_home, and - nkeys 3 and 4, else 0 - hj_wide::hash
//      of the key words and its hj_wide::lds_home.
// stdout: "NAME narrow wide" per constant of the two layouts.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "group_layout.hpp"
#include "wide_group_layout.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    uint32_t head[2];
    if (fread(head, sizeof(uint32_t), 2, in) != 2 || head[0] < 1 || head[0] > hj_wide::MAX_KEYS) { fprintf(stderr, "bad header\n"); return 2; }
    const uint32_t nkeys = head[0], count = head[1];
    std::vector<uint32_t> keys((size_t)count * 4);
    if (fread(keys.data(), sizeof(uint32_t), keys.size(), in) != keys.size()) { fprintf(stderr, "short input\n"); return 2; }
    fclose(in);
    std::vector<unsigned long long> out((size_t)count * 4, 0);
    for (size_t i = 0; i < count; ++i) {
        const uint32_t *k = &keys[i * 4];
        const hj_group::u64 h = hj_group::mix(hj_group::tuple_of(k[0], k[1]));
        out[i * 4] = h;
        out[i * 4 + 1] = hj_group::lds_home(h);
        if (nkeys >= hj_wide::MIN_KEYS) {
            hj_wide::u64 w[hj_wide::MAX_KEYS] = {0, 0, 0, 0};
            for (uint32_t c = 0; c < nkeys; ++c) w[c] = hj_wide::key_word(k[c]);
            const hj_wide::u64 hw = hj_wide::hash(w);
            out[i * 4 + 2] = hw;
            out[i * 4 + 3] = hj_wide::lds_home(hw);
        }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), sizeof(unsigned long long), out.size(), o) != out.size() || fclose(o) != 0) { fprintf(stderr, "short output\n"); return 2; }
    printf("MAX_KEYS %u %u\n", hj_group::MAX_KEYS, hj_wide::MAX_KEYS);
    printf("BLOCK %u %u\n", hj_group::BLOCK, hj_wide::BLOCK);
    printf("LOG2_LDS_SLOTS %u %u\n", hj_group::LOG2_LDS_SLOTS, hj_wide::LOG2_LDS_SLOTS);
    printf("LDS_SLOTS %u %u\n", hj_group::LDS_SLOTS, hj_wide::LDS_SLOTS);
    printf("LDS_PROBES %u %u\n", hj_group::LDS_PROBES, hj_wide::LDS_PROBES);
    printf("LDS_GROUPS %u %u\n", hj_group::LDS_GROUPS, hj_wide::LDS_GROUPS);
    printf("MIN_MERGE_SLOTS %llu %llu\n", hj_group::MIN_MERGE_SLOTS, hj_wide::MIN_MERGE_SLOTS);
    printf("MERGE_SLOTS_511 %llu %llu\n", hj_group::merge_slots(511), hj_wide::merge_slots(511));
    printf("MERGE_SLOTS_3000 %llu %llu\n", hj_group::merge_slots(3000), hj_wide::merge_slots(3000));
    printf("MERGE_SLOTS_2_19 %llu %llu\n", hj_group::merge_slots(1ull << 19), hj_wide::merge_slots(1ull << 19));
    return 0;
}
