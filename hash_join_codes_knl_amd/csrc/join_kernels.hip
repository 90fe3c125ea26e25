// join_kernels.hip — K7+K8: per-partition build + probe with the hash table in LDS.
//
// Replaces build()/probe() of phj.cpp:307-397 / 399-571 (scalar definitions
// 577-647) and the join loop phj.cpp:1869-1924 / cpra2.cpp:1883-1971.
// Design (not a translation):
//   * The reference keeps a ~128 KB double-hashing table per thread in L2
//     (phj.cpp:1976-1977); here each workgroup owns an 8192-slot table of
//     {key, payload} words in LDS (64 KiB, two workgroups per CU so that one
//     workgroup's clear/build overlaps the other's probe stream).
//   * FAST PATH - 2-choice cuckoo table.  rocprof PMC showed the open-addressing
//     probe loop was instruction-bound (127 VALU + 77 SALU wave-instructions per
//     probe key: 64 lanes x 4 chains wait for the longest chain), not memory-bound.
//     In a cuckoo table a key lives in exactly one of two slots
//     a1 = top bits of key*tf0, a2 = a1 + odd offset from key*tf1, so a probe is two
//     independent ds_read_b64 and two compares: no loop, no divergence, and up
//     to two copies of a build key are reported naturally (multi-match).
//     Build = ds_wrxchg_rtn_b64 eviction walk, bounded; at load <= 0.5 it succeeds
//     with overwhelming probability for unique keys.
//   * FALLBACK - double-hashing chains (the reference's scheme over a power-of-two
//     table, odd step) when the cuckoo build does not converge: >= 3 copies of a
//     build key (config-1-like duplicate-heavy build sides) or an unlucky cycle.
//     Probe walks to the first empty slot and reports every match (no _UNIQUE,
//     phj.cpp:616-644).
//   * At most SLOTS/2 build tuples per table fill; larger partitions are processed
//     in several fills, re-streaming the probe slice (skew overflow path).
//   * The empty sentinel of partition q is the smallest value that does NOT hash to
//     q (generalises phj.cpp:1886-1897), so key 0 is legal.
//   * A work item is (partition, slice of its probe rows); CPRA's per-chunk pieces
//     (cpra2.cpp:1891-1959 memcpy gather) are walked in place: the "gather" is
//     just the loop over chunk offsets.
//   * Results: register aggregates (count + 3 sums) reduced per workgroup, or
//     materialised rows through per-wave 64-bit cursors into atomically claimed
//     blocks (the reference's block protocol, npj.cpp:244-246, 312-316).
#include "hj_device.hpp"
#include "hj_internal.hpp"
#include "hj_emit.hpp"
#include "hj_lookup.hpp"

// PACKED: the relations arrive as payload << 32 | key tuples (the library's own
// partition passes); !PACKED: separate key / payload columns (hjgpu_join_partitions).
// UNIQUE: the reference's _UNIQUE build (npj.cpp:288-290, phj.cpp:459, 635): a probe tuple reports its FIRST
// match only.  Inside one table that is "one of the key's two cuckoo slots" / "the first hit of the chain";
// a build partition that takes several table fills keeps one bit per probe row of the work item in LDS
// (`matched`), so that a row reported by an earlier fill is skipped by the later ones (such partitions
// are then planned as ONE fill group: all fills of a probe slice stay with one workgroup).
// Round 4: that bookkeeping is needed by multi-fill partitions only - skew, never the planned case - but its code cost
// every _UNIQUE join 26 VGPRs (one probe vector per lane, no build-row prefetch: join phase 1.88 instead of 1.59 ms at
// 64 M x 1 G).  A _UNIQUE join is therefore TWO launches: <UNIQUE, !DEDUP> takes the work items whose build rows fit
// one fill, with the default instance's geometry (two vectors per lane, prefetch, no `matched` words), and skips the
// others; <UNIQUE, DEDUP> takes exactly those and returns at once when the plan counted none (JoinArgs::multi_fill).
// Waves per SIMD the geometry runs at: workgroups per CU (LDS: one table + ~10 KiB each in 160 KiB; threads: 2048
// per CU) x waves per workgroup / 4 SIMDs.  It is the second argument of __launch_bounds__ (HIP: minimum waves per
// execution unit), i.e. the register budget: 512 / waves VGPRs per lane.  More bytes in flight per lane at the price
// of fewer waves does NOT pay here (round 3, profiles/r03_ab_emit.txt: 384 threads x 4 vectors at 3 waves per SIMD
// 3.15 ms, 256 x 8 at 2 waves 2.74 ms, against 1.58 ms for 512 x 2 at 4 waves): K7+K8 is bound by instruction issue
// and LDS latency, which only resident waves hide, not by the probe stream's bytes in flight.
constexpr int hj_join_wgs_per_cu(int block, int log2slots)
{
    const int by_lds = (160 * 1024) / ((1 << log2slots) * 8 + 1024 + 9 * 1024), by_threads = 2048 / block;
    const int n = by_lds < by_threads ? by_lds : by_threads;
    return n < 1 ? 1 : n;
}
constexpr int hj_join_waves_per_simd(int block, int log2slots)
{
    const int w = hj_join_wgs_per_cu(block, log2slots) * (block / 64) / 4;
    return w < 1 ? 1 : w;
}

// The two slots of a key in the cuckoo table of 2^LOG2SLOTS slots: the top bits of key * tf0, and an odd distance from key * tf1 further
template <int LOG2SLOTS>
__device__ __forceinline__ uint2 hj_cuckoo_slots(uint32_t key, uint32_t tf0, uint32_t tf1)
{
    const uint32_t a1 = (key * tf0) >> (32 - LOG2SLOTS);
    return make_uint2(a1, (a1 + (((key * tf1) >> (32 - LOG2SLOTS)) | 1u)) & ((1u << LOG2SLOTS) - 1));
}

// HJ_EMIT4 (build-time, default 1; 0 for A/B): a probe vector whose four tuples matched exactly once each leaves the lane as ONE 16-byte
// store per result column (EmitterT::emit4) instead of four 4-byte ones.  Round 6, 64 M x 1 G with 10^9 rows, default policy
// (non-temporal rows), one process, same allocations: join 4.48 -> 3.83 ms (profiles/r06_ab_emit4.txt) - the 4-byte non-temporal
// stores cost 14 % over plain ones (round 5), whole 16-byte pieces cost nothing, as in K6.
#ifndef HJ_EMIT4
#define HJ_EMIT4 1
#endif
// the probe of a left outer join's tail pass (join_body): no table, every open row is reported as a NULL row
struct hj_tail_pass {
    __device__ uint32_t operator()(const uint32_t (&)[4], const uint32_t (&)[4], const bool (&)[4]) const { return 0u; }
};
// the probe of HJ_MODE_MARK (join_body): nothing is reported, the table slots the item's probe rows hit are marked
struct hj_mark_pass {
    __device__ uint32_t operator()(const uint32_t (&)[4], const uint32_t (&)[4], const bool (&)[4]) const { return 0u; }
};

// NTROWS: result rows through non-temporal stores (EmitterT<true>; JoinArgs::nt_rows) - false only for solo joins
// MODE (HJ_MODE_*): what a probe tuple reports.  HJ_MODE_INNER: its matches (join_kernel).  HJ_MODE_SEMI / HJ_MODE_ANTI
// (exists_probe_kernel, always with UNIQUE): ONE row (key, outer_val) when it has a match / when it has none, from its match state -
// the first-match walk of _UNIQUE; rows of two columns (EmitterT<.., 2>), aggregates without sum_inner_vals.  Anti-join details:
//   * the probe rows of an item with no build rows (a partition or group without build tuples, or a whole join with inner == 0) are
//     all reported - the plan gives such partitions work items under ANTI (PlanArgs::anti);
//   * a multi-fill item (DEDUP) only sets its rows' `matched` bits during the fills and reports the rows whose bit is clear in ONE
//     more pass over its probe rows after the last fill;
//   * a broadcast join's probe key equal to the sentinel matches nothing and is reported.
// HJ_MODE_LEFT_OUTER (outer_probe_kernel): the inner join's rows plus ONE row (key, outer_val, HJGPU_NULL_VAL) per probe tuple without a
// match.  Here UNIQUE is the first-match walk only (HJGPU_FLAG_UNIQUE); the two launches - single-fill items, then multi-fill ones
// (DEDUP) - and one fill group per probe slice (PlanArgs::unique) hold either way.  A single-fill item emits a probe vector's matches and
// NULL rows together (one emit4 when each of its tuples yields exactly one row: every full vector under UNIQUE); a multi-fill item emits
// the matches of every fill and marks their rows (under UNIQUE the marks also skip the rows in later fills), then reports the unmarked
// rows in the anti-join's tail pass; an item without build rows reports all its probe rows.
// HJ_MODE_RIGHT_OUTER (right_probe_kernel) reports what the inner join reports, HJ_MODE_FULL_OUTER (full_probe_kernel) what the left outer
// join reports; both also find out which BUILD rows matched.  "Matched" is a property of a build key - if any probe tuple carries it,
// every build row with it is matched - so the table needs no row ids: a probe sets one bit per table SLOT it hits in LDS (`slot_bits`),
// and after the probe loop of each table fill the workgroup walks the fill's build rows once more (L2-hot), looks every key up and ORs
// "a slot holding this key is marked" into JoinArgs::build_bits, one bit per row of the partitioned build array.  The OR is atomic, on
// whole 32-bit words from a ballot (a wave's rows are consecutive): the slices of one partition are work items of their own, in any
// workgroups and any order, and each sees only its own probe rows.  The rows whose bit stays clear - also those of partitions without a
// single work item - are reported by build_unmatched_kernel behind the join.  Never with UNIQUE: a first-match walk would leave the other
// copies of a duplicated build key unvisited.
// The multi-fill items of a full outer join: the left outer join's multi-fill instance is at its 128 VGPRs - anything added to it, even the
// clear of `slot_bits`, spills - so it reports them as it is (outer_probe_kernel<.., DEDUP>), and a third launch, HJ_MODE_MARK
// (mark_probe_kernel), fills the tables of those items once more and only marks (hj_mark_pass): no rows, no aggregates.
// Right semi- and anti-joins (HJ_MODE_RIGHT_SEMI / _ANTI) report build rows only, so ALL their probes are HJ_MODE_MARK: the single-fill
// items by mark_single_probe_kernel (DEDUP = false), the multi-fill items by mark_probe_kernel as it is; build_rows_kernel behind them
// reports the marked / the clear rows.  hj_mark_pass stops at a key's first hit: the slot it marks is the slot mark_build_rows finds - a
// cuckoo table's row pass looks at both slots of a key, a chained table's walks from the same first slot to the same first copy.
template <bool ON, uint32_t WORDS>
struct SlotBits {
    static __device__ __forceinline__ uint32_t *get() { __shared__ uint32_t bits[WORDS]; return bits; }
};
template <uint32_t WORDS>
struct SlotBits<false, WORDS> {
    static __device__ __forceinline__ uint32_t *get() { return nullptr; }
};

template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED, bool UNIQUE, bool DEDUP, bool NTROWS, int MODE>
__device__ __forceinline__ void join_body(JoinArgs a)
{
    // LEFTISH: the modes that report like the left outer join; KEEPB: the modes that mark the build rows their probes hit
    constexpr bool LEFTISH = MODE == HJ_MODE_LEFT_OUTER || MODE == HJ_MODE_FULL_OUTER;
    constexpr bool MARKING = MODE == HJ_MODE_MARK;
    constexpr bool KEEPB = MODE == HJ_MODE_RIGHT_OUTER || MODE == HJ_MODE_FULL_OUTER || MARKING;
    static_assert(UNIQUE || !DEDUP || MODE == HJ_MODE_LEFT_OUTER || MARKING, "DEDUP is the multi-fill half of a _UNIQUE or left / full outer join");
    static_assert(MODE == HJ_MODE_INNER || ((UNIQUE || LEFTISH || KEEPB) && NTROWS),
                  "semi- and anti-joins walk to the first match; rows non-temporal");
    static_assert(!(KEEPB && UNIQUE), "right and full outer joins walk to every copy of a build key");
    static_assert(!(KEEPB && DEDUP) || MARKING, "the multi-fill items of a full outer join are marked by a launch of its own");
    // the two launches of a _UNIQUE join: single-fill items, then multi-fill ones (DEDUP); left and full outer joins always
    constexpr bool SPLIT = UNIQUE || LEFTISH || MARKING;
    // the plan found no partition that takes several fills (the planned case): nothing for this launch to do
    if (DEDUP && a.multi_fill && *a.multi_fill == 0) return;
    constexpr uint32_t SLOTS = 1u << LOG2SLOTS;
    constexpr uint32_t MASK = SLOTS - 1;
    constexpr uint32_t CAP = SLOTS / 2;
    constexpr int SHIFT = 32 - LOG2SLOTS;
    constexpr int NW = BLOCK / 64;
    constexpr int RB = 8;                        // build rows a lane loads before inserting
    constexpr int CUCKOO_MAX_EVICTIONS = 64;
    __shared__ u64 tab64[SLOTS];                 // low word = key, high word = build payload
    __shared__ u64 red[4][NW];
    __shared__ u64 wave_cursor[NW];
    __shared__ uint32_t cuckoo_failed;
    // UNIQUE: one bit per probe row of the current work item (<= HJ_JOIN_SLICE + 1 rows per chunk piece)
    constexpr uint32_t MATCHED_WORDS = (DEDUP && !MARKING) ? (HJ_JOIN_SLICE + 64) / 32 + 2 : 1;
    __shared__ uint32_t matched[MATCHED_WORDS];
    constexpr bool dedup = DEDUP;                // every item of the DEDUP launch takes more than one fill, none of the other's
    uint2 *tab = reinterpret_cast<uint2 *>(tab64);   // chained view: .x = key, .y = payload
    uint32_t *const slot_bits = SlotBits<KEEPB, SLOTS / 32>::get();   // KEEPB: one bit per table slot a probe of this fill has hit

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const uint32_t P = a.P, C = a.chunks;
    const u64 total_items = a.slice_prefix[P];
    const uint4 *__restrict__ sk4 = reinterpret_cast<const uint4 *>(PACKED ? a.sk : a.sk - a.s_align);
    const uint4 *__restrict__ sv4 = reinterpret_cast<const uint4 *>(PACKED ? a.sk : a.sv - a.s_align);
    const u64 *__restrict__ r64 = reinterpret_cast<const u64 *>(a.rk);
    const uint32_t tf0 = a.tf0, tf1 = a.tf1;

    EmitterT<NTROWS, (MODE == HJ_MODE_SEMI || MODE == HJ_MODE_ANTI) ? 2 : 3> em;
    em.init(a.ok, a.oov, a.oiv, a.block_size, a.block_limit, a.block_counter, a.overflow,
            &wave_cursor[wave]);
    // (the multi-fill half of a _UNIQUE join runs behind the single-fill half on the same stream, with the same grid: wave w of
    // workgroup b goes on in the block that wave w of workgroup b left open, and leaves its cursor in the same slot - one
    // launch's worth of worker slots for close_gaps, not two)
    // (device-planned groups - JoinArgs::resume - do the same from group to group: one block counter, one set of open blocks, one close_gaps)
    if (hj_lane() == 0) wave_cursor[wave] = ((DEDUP || a.resume) && a.ok) ? a.final_offsets[(u64)blockIdx.x * NW + wave] : HJ_NO_CURSOR;

    u64 acc_n = 0, acc_k = 0, acc_o = 0, acc_i = 0;
    uint32_t empty = 0;
    uint32_t q = 0;
    bool anti_tail = false;                          // HJ_MODE_ANTI: the pass that reports the item's rows without a match
    uint32_t lo_open = 0;                            // HJ_MODE_LEFT_OUTER, single-fill items: the current vector's tuples of the slice

    // ---- visit rows [fill_beg, fill_end) of the chunk-concatenated build partition q ----
    // rows below `from_row` were already inserted (from the prefetch registers)
    auto for_each_build_row = [&](u64 fill_beg, u64 fill_end, u64 from_row, auto insert) {
        if (C > 1) {
            // chunked relation (CPRA): the partition's rows lie in C pieces.  Walking the pieces one after
            // another costs one memory round trip per piece (C x ~2 us against ~40 us per work item); here a
            // lane's RB rows are rows of the CONCATENATION, so that all loads of a fill are in flight together.
            u64 pb[8], cum[9];                        // piece c = rows [cum[c], cum[c+1]) at pb[c]
            cum[0] = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                pb[c] = 0; cum[c + 1] = cum[c];
                if ((uint32_t)c < C) { pb[c] = a.roff[(u64)c * P + q]; cum[c + 1] = cum[c] + (a.rend[(u64)c * P + q] - pb[c]); }
            }
            for (u64 base = max(fill_beg, from_row); base < fill_end; base += (u64)BLOCK * RB) {
                uint32_t k[RB], v[RB];
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const u64 i = base + (u64)j * BLOCK + tid;
                    k[j] = 0; v[j] = 0;
                    if (i < fill_end) {
                        u64 at = pb[0] + i;
#pragma unroll
                        for (int c = 1; c < 8; ++c) if (i >= cum[c]) at = pb[c] + (i - cum[c]);   // cum is non-decreasing
                        if (PACKED) { const u64 t = r64[at]; k[j] = (uint32_t)t; v[j] = (uint32_t)(t >> 32); }
                        else { k[j] = a.rk[at]; v[j] = a.rv[at]; }
                    }
                }
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const u64 i = base + (u64)j * BLOCK + tid;
                    if (i < fill_end) insert(k[j], v[j]);
                }
            }
            return;
        }
        u64 seen = 0;
        for (uint32_t c = 0; c < C; ++c) {
            const u64 b = a.roff[(u64)c * P + q], e = a.rend[(u64)c * P + q];
            const u64 len = e - b;
            const u64 lo = max(max(seen, fill_beg), from_row), hi = min(seen + len, fill_end);
            for (u64 base = lo; base < hi; base += (u64)BLOCK * RB) {
                uint32_t k[RB], v[RB];
                // all loads of the batch are issued before the first insert
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const u64 i = base + (u64)j * BLOCK + tid;
                    k[j] = 0; v[j] = 0;
                    if (i < hi) {
                        if (PACKED) { const u64 t = r64[b + (i - seen)]; k[j] = (uint32_t)t; v[j] = (uint32_t)(t >> 32); }
                        else { k[j] = a.rk[b + (i - seen)]; v[j] = a.rv[b + (i - seen)]; }
                    }
                }
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const u64 i = base + (u64)j * BLOCK + tid;
                    if (i < hi) insert(k[j], v[j]);
                }
            }
            seen += len;
        }
    };

    // semi- / anti-join: the tuples j of a probe vector with bit j of `rep` leave as rows (key, outer_val); left outer join: as NULL rows
    // (key, outer_val, `iv` = HJGPU_NULL_VAL), which add nothing to sum_inner_vals
    auto report4 = [&](const uint32_t (&key)[4], const uint32_t (&val)[4], uint32_t rep, uint32_t iv) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool r = (rep >> j) & 1u;
            acc_n += r ? 1u : 0u; acc_k += r ? key[j] : 0u; acc_o += r ? val[j] : 0u;
        }
        if (a.ok) {
            const uint32_t none[4] = {iv, iv, iv, iv};
            if (rep == 15u && a.block_size >= 512) em.emit4(key, val, none);       // (emit4: blocks of 512 rows and more)
            else if (rep) {
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((rep >> j) & 1u) em.emit(key[j], val[j], iv);
            }
        }
    };

    // ---- stream the S rows [gb, ge): BATCH key + BATCH payload vectors in flight per lane ----
    // `row0`: index of row gb among the probe rows of this work item (UNIQUE's `matched` bits)
    auto for_each_probe_vector = [&](u64 gb, u64 ge, u64 row0, auto probe4) {
        // left outer join: the tail pass (see below) is an instance of its own, the probes' instances carry no tail path
        constexpr bool TAIL = __is_same(decltype(probe4), hj_tail_pass);
        constexpr bool MARK = __is_same(decltype(probe4), hj_mark_pass);
        for (u64 g0 = (gb & ~3ull) + (u64)tid * 4; g0 < ge; g0 += (u64)BLOCK * 4 * BATCH) {
            uint4 kk[BATCH], vv[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const u64 g = g0 + (u64)u * BLOCK * 4;
                kk[u] = make_uint4(0, 0, 0, 0); vv[u] = kk[u];
                if (g < ge) {
                    if (PACKED) { kk[u] = sk4[g >> 1]; vv[u] = sk4[(g >> 1) + 1]; }     // 4 tuples = 2 x 16 bytes
                    else { kk[u] = sk4[g >> 2]; vv[u] = sv4[g >> 2]; }
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const u64 g = g0 + (u64)u * BLOCK * 4;
                if (g >= ge) break;
                const uint32_t key[4] = {kk[u].x, PACKED ? kk[u].z : kk[u].y, PACKED ? vv[u].x : kk[u].z, PACKED ? vv[u].z : kk[u].w};
                const uint32_t val[4] = {PACKED ? kk[u].y : vv[u].x, PACKED ? kk[u].w : vv[u].y, PACKED ? vv[u].y : vv[u].z, vv[u].w};
                if constexpr (MODE == HJ_MODE_SEMI || MODE == HJ_MODE_ANTI) {
                    // inr: the rows of the slice that are still open (DEDUP: not reported by an earlier fill); valid: those that may match -
                    // a probe key equal to the broadcast sentinel matches nothing (see below), and the anti-join reports it
                    bool inr[4], valid[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t row = (uint32_t)(row0 + (g + j - gb));
                        inr[j] = (g + j >= gb) && (g + j < ge);
                        if (dedup && inr[j]) inr[j] = !((matched[row >> 5] >> (row & 31)) & 1u);
                        valid[j] = inr[j] && (PACKED || key[j] != empty);
                    }
                    const uint32_t hits = anti_tail ? 0u : probe4(key, val, valid);
                    if (dedup) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t row = (uint32_t)(row0 + (g + j - gb));
                            if ((hits >> j) & 1u) atomicOr(&matched[row >> 5], 1u << (row & 31));
                        }
                    }
                    uint32_t rep = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) rep |= (inr[j] && (((hits >> j) & 1u) != 0) == (MODE == HJ_MODE_SEMI)) ? 1u << j : 0u;
                    if (MODE == HJ_MODE_ANTI && dedup && !anti_tail) rep = 0;       // the fills only mark; the tail pass reports
                    report4(key, val, rep, 0u);
                    continue;
                }
                if constexpr (MARK) {
                    // the first slot of the key's walk that holds it: what mark_build_rows looks at (both slots of a cuckoo table)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (g + j < gb || g + j >= ge) continue;
                        if (!cuckoo_failed) {
                            const uint2 at2 = hj_cuckoo_slots<LOG2SLOTS>(key[j], tf0, tf1);
                            const uint32_t a1 = at2.x, a2 = at2.y;
                            const uint32_t k1 = (uint32_t)tab64[a1], k2 = (uint32_t)tab64[a2];
                            const uint32_t at = k1 == key[j] ? a1 : a2;
                            if (k1 == key[j] || k2 == key[j]) atomicOr(&slot_bits[at >> 5], 1u << (at & 31));
                        } else {
                            uint32_t slot = (key[j] * tf0) >> SHIFT;
                            const uint32_t step = ((key[j] * tf1) >> SHIFT) | 1u;
                            for (uint32_t n = 0; n < SLOTS; ++n) {
                                const uint32_t tk = tab[slot].x;
                                if (tk == key[j]) { atomicOr(&slot_bits[slot >> 5], 1u << (slot & 31)); break; }
                                if (tk == empty) break;
                                slot = (slot + step) & MASK;
                            }
                        }
                    }
                    continue;
                }
                if constexpr (LEFTISH) {
                    // inr: the rows of the slice still open (DEDUP: under UNIQUE, and in the tail pass, not yet matched by a fill);
                    // valid: those that may match (a probe key equal to the broadcast sentinel matches nothing: a NULL row)
                    bool inr[4], valid[4];
                    uint32_t open = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t row = (uint32_t)(row0 + (g + j - gb));
                        inr[j] = (g + j >= gb) && (g + j < ge);
                        if (dedup && (UNIQUE || TAIL) && inr[j]) inr[j] = !((matched[row >> 5] >> (row & 31)) & 1u);
                        valid[j] = inr[j] && (PACKED || key[j] != empty);
                        open |= inr[j] ? 1u << j : 0u;
                    }
                    if constexpr (TAIL) {
                        if constexpr (DEDUP) {
                            // row by row: report4's emit4 beside the fills' costs the 1024-thread DEDUP instance 3 spilled VGPRs
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                if ((open >> j) & 1u) {
                                    acc_n += 1; acc_k += key[j]; acc_o += val[j];
                                    if (a.ok) em.emit(key[j], val[j], HJGPU_NULL_VAL);
                                }
                            }
                        } else report4(key, val, open, HJGPU_NULL_VAL);
                        continue;
                    } else {
                        lo_open = open;               // the single-fill probes emit the NULL rows of `open` beside the matches
                        const uint32_t hits = probe4(key, val, valid);
                        if (dedup) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const uint32_t row = (uint32_t)(row0 + (g + j - gb));
                                if ((hits >> j) & 1u) atomicOr(&matched[row >> 5], 1u << (row & 31));
                            }
                        }
                        continue;
                    }
                }
                bool valid[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    valid[j] = (g + j >= gb) && (g + j < ge);
                    // A probe key that equals the empty sentinel must not "match" empty slots.  In partitioned
                    // joins no tuple of partition q carries that value (it hashes elsewhere); in a broadcast
                    // join the probe side is the caller's unpartitioned column and may hold it (no build key
                    // does).  Only the separate-column instance serves broadcast joins.
                    if (!PACKED) valid[j] = valid[j] && key[j] != empty;
                }
                if (UNIQUE && dedup) {
                    // rows an earlier fill of this partition has already reported are done
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t row = (uint32_t)(row0 + (g + j - gb));
                        if (valid[j]) valid[j] = !((matched[row >> 5] >> (row & 31)) & 1u);
                    }
                    const uint32_t hits = probe4(key, val, valid);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t row = (uint32_t)(row0 + (g + j - gb));
                        if ((hits >> j) & 1u) atomicOr(&matched[row >> 5], 1u << (row & 31));
                    }
                } else (void)probe4(key, val, valid);
            }
        }
    };

    // cuckoo probe: two independent slot reads per key, no loop
    auto probe4_cuckoo = [&](const uint32_t (&key)[4], const uint32_t (&val)[4], const bool (&valid)[4]) -> uint32_t {
        u64 t1[4], t2[4];
        uint32_t hits = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint2 at = hj_cuckoo_slots<LOG2SLOTS>(key[j], tf0, tf1);
            const uint32_t a1 = at.x;
#if defined(HJ_JOIN_LIMIT_STUDY) && HJ_JOIN_LIMIT_STUDY == 1
            // LIMIT STUDY, never the product (tools/build_variant.py join_one_slot -DHJ_JOIN_LIMIT_STUDY=1; results are WRONG): the second
            // slot's multiply, address and LDS read do not exist - an upper bound on what ANY scheme that fetches a key's two slots with one
            // LDS instruction and one address computation could save (round 5's review asked for ds_read2_b64; its two offsets are
            // immediates of the instruction, the same for every lane, and a fixed distance between a key's slots is no cuckoo table)
            t1[j] = tab64[a1];
            t2[j] = t1[j] ^ ((u64)1 << 63);
#else
            t1[j] = tab64[a1];
            t2[j] = tab64[at.y];
#endif
        }
        if constexpr (MODE == HJ_MODE_SEMI || MODE == HJ_MODE_ANTI) {
#pragma unroll
            for (int j = 0; j < 4; ++j) hits |= (valid[j] && ((uint32_t)t1[j] == key[j] || (uint32_t)t2[j] == key[j])) ? 1u << j : 0u;
            return hits;
        }
        if constexpr (KEEPB) {
            // one marked slot per matched key is enough: the walk over the build rows below looks at both slots of a key
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint2 a12 = hj_cuckoo_slots<LOG2SLOTS>(key[j], tf0, tf1);
                const bool h1 = valid[j] && ((uint32_t)t1[j] == key[j]), h2 = valid[j] && ((uint32_t)t2[j] == key[j]);
                const uint32_t at = h1 ? a12.x : a12.y;
                if (h1 || h2) atomicOr(&slot_bits[at >> 5], 1u << (at & 31));             // ds_or_b32
            }
        }
        if constexpr (LEFTISH) {
            // the inner join's matches; a single-fill item also the NULL row of every open tuple without one (a multi-fill item: the tail pass)
            u64 sk_ = 0, so_ = 0, si_ = 0;
            uint32_t n = 0;
            bool one = true;                  // every tuple of the vector yields exactly one row: ONE emit4
            uint32_t iv4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool h1 = valid[j] && ((uint32_t)t1[j] == key[j]);
                const bool h2 = valid[j] && ((uint32_t)t2[j] == key[j]) && !(UNIQUE && h1);
                const bool z = !DEDUP && ((lo_open >> j) & 1u) && !h1 && !h2;
                const uint32_t m = (h1 ? 1u : 0u) + (h2 ? 1u : 0u) + (z ? 1u : 0u);
                hits |= (h1 || h2) ? 1u << j : 0u;
                n += m;
                sk_ += (u64)key[j] * m;
                so_ += (u64)val[j] * m;
                si_ += (h1 ? (uint32_t)(t1[j] >> 32) : 0u);
                si_ += (h2 ? (uint32_t)(t2[j] >> 32) : 0u);
                one = one && m == 1u;
            }
            if (a.ok) {
                // (a wave's emit4 writes up to 256 rows and claims at most ONE new block: blocks of 512 rows and more)
                if (one && a.block_size >= 512) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        iv4[j] = ((uint32_t)t1[j] == key[j] && valid[j]) ? (uint32_t)(t1[j] >> 32)
                               : ((uint32_t)t2[j] == key[j] && valid[j]) ? (uint32_t)(t2[j] >> 32) : HJGPU_NULL_VAL;
                    em.emit4(key, val, iv4);
                }
                else if (n) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool h1 = valid[j] && ((uint32_t)t1[j] == key[j]);
                        const bool h2 = valid[j] && ((uint32_t)t2[j] == key[j]) && !(UNIQUE && h1);
                        if (h1 | h2) em.emit(key[j], val[j], (uint32_t)((h1 ? t1[j] : t2[j]) >> 32));
                        if (h1 & h2) em.emit(key[j], val[j], (uint32_t)(t2[j] >> 32));
                        if (!DEDUP && ((lo_open >> j) & 1u) && !h1 && !h2) em.emit(key[j], val[j], HJGPU_NULL_VAL);
                    }
                }
            }
            acc_n += n; acc_k += sk_; acc_o += so_; acc_i += si_;
            return hits;
        }
        u64 sk_ = 0, so_ = 0, si_ = 0;
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool h1 = valid[j] && ((uint32_t)t1[j] == key[j]);
            const bool h2 = valid[j] && ((uint32_t)t2[j] == key[j]) && !(UNIQUE && h1);
            const uint32_t m = (h1 ? 1u : 0u) + (h2 ? 1u : 0u);
            hits |= m ? 1u << j : 0u;
            n += m;
            sk_ += (u64)key[j] * m;
            so_ += (u64)val[j] * m;
            si_ += (h1 ? (uint32_t)(t1[j] >> 32) : 0u);
            si_ += (h2 ? (uint32_t)(t2[j] >> 32) : 0u);
#if !HJ_EMIT4
            if (a.ok) {
                // one emit for "this key matched" (with unique build keys that is every lane of the wave:
                // 64 rows, the cursor moves in whole lines), a second one only for a key found in BOTH slots
                if (h1 | h2) em.emit(key[j], val[j], (uint32_t)((h1 ? t1[j] : t2[j]) >> 32));
                if (h1 & h2) em.emit(key[j], val[j], (uint32_t)(t2[j] >> 32));
            }
#endif
        }
#if HJ_EMIT4
        if (a.ok) {
            // a vector whose four probe tuples matched exactly once each (the common case) leaves as ONE 16-byte store per column and
            // lane (EmitterT::emit4); any other vector row by row as before
            bool once[4], twice = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool h1 = valid[j] && ((uint32_t)t1[j] == key[j]);
                const bool h2 = valid[j] && ((uint32_t)t2[j] == key[j]) && !(UNIQUE && h1);
                once[j] = h1 != h2; twice = twice || (h1 && h2);
            }
            // (a wave's emit4 writes up to 256 rows and claims at most ONE new block: blocks of 512 rows and more)
            if (once[0] && once[1] && once[2] && once[3] && a.block_size >= 512) {
                uint32_t iv4[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) iv4[j] = (uint32_t)((((uint32_t)t1[j] == key[j]) ? t1[j] : t2[j]) >> 32);
                em.emit4(key, val, iv4);
            } else if (once[0] || once[1] || once[2] || once[3] || twice) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool h1 = valid[j] && ((uint32_t)t1[j] == key[j]);
                    const bool h2 = valid[j] && ((uint32_t)t2[j] == key[j]) && !(UNIQUE && h1);
                    if (h1 | h2) em.emit(key[j], val[j], (uint32_t)((h1 ? t1[j] : t2[j]) >> 32));
                    if (h1 & h2) em.emit(key[j], val[j], (uint32_t)(t2[j] >> 32));
                }
            }
        }
#endif
        acc_n += n; acc_k += sk_; acc_o += so_; acc_i += si_;
        return hits;
    };

    // chained probe: 4 chains per lane advanced in lock step to the first empty slot
    auto probe4_chained = [&](const uint32_t (&key)[4], const uint32_t (&val)[4], const bool (&valid)[4]) -> uint32_t {
        uint32_t slot[4], step[4];
        uint2 t[4];
        bool live[4];
        uint32_t hits = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            live[j] = valid[j];
            slot[j] = (key[j] * tf0) >> SHIFT;
            step[j] = ((key[j] * tf1) >> SHIFT) | 1u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { t[j] = make_uint2(empty, 0u); if (live[j]) t[j] = tab[slot[j]]; }
        for (;;) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool hit = live[j] && (t[j].x == key[j]);
                if constexpr (MODE == HJ_MODE_INNER || LEFTISH || KEEPB) {
                    acc_n += hit ? 1u : 0u;
                    acc_k += hit ? key[j] : 0u;
                    acc_o += hit ? val[j] : 0u;
                    acc_i += hit ? t[j].y : 0u;
                    if (a.ok) { if (hit) em.emit(key[j], val[j], t[j].y); }
                }
                hits |= hit ? 1u << j : 0u;
                if constexpr (KEEPB) { if (hit) atomicOr(&slot_bits[slot[j] >> 5], 1u << (slot[j] & 31)); }   // every copy: the full walk
                live[j] = live[j] && (t[j].x != empty) && !(UNIQUE && hit);
                slot[j] = (slot[j] + step[j]) & MASK;
            }
            if (!(live[0] | live[1] | live[2] | live[3])) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (live[j]) t[j] = tab[slot[j]];
        }
        // left outer join, single-fill item: the NULL rows of the open tuples without a match
        if constexpr (LEFTISH && !DEDUP) report4(key, val, lo_open & ~hits, HJGPU_NULL_VAL);
        return hits;
    };

    // nslices_word = probe slices | extra probe pieces << 24: a claimed probe side (JoinArgs::s_pieces) has two pieces of one region per
    // partition in soff / send - pass 2's front lines and back tails - where the build side has one (the count travels with the item's
    // descriptor: a kernel-argument load here costs the 1024-thread instances scratch)
    auto probe_item = [&](u64 slice, u64 nslices_word, auto probe4) {
        u64 row0 = 0;
        const u64 nslices = nslices_word & 0xFFFFFFu;
        const uint32_t pieces = C + (uint32_t)(nslices_word >> 24);
        for (uint32_t c = 0; c < pieces; ++c) {
            const u64 b = a.soff[(u64)c * P + q], e = a.send[(u64)c * P + q];
            const u64 len = e - b;
            if (len == 0) continue;
            // sub-range `slice` of `nslices` equal parts (len < 2^40, slices < 2^24)
            const u64 sb = b + (len * slice) / nslices;
            const u64 se = b + (len * (slice + 1)) / nslices;
            if (se <= sb) continue;
            for_each_probe_vector(a.s_align + sb, a.s_align + se, row0, probe4);
            row0 += se - sb;
        }
    };

    // KEEPB, after the probes of a table fill: rows [fill_beg, fill_end) of partition q once more - a row whose key sits in a marked slot
    // gets its bit in a.build_bits.  The lanes of a wave hold consecutive rows of one piece, so a ballot gives whole words: the lane on a
    // word boundary (and lane 0) ORs the word in, non-zero words only.
    auto mark_build_rows = [&](u64 fill_beg, u64 fill_end, bool chained) {
        u64 seen = 0;
        for (uint32_t c = 0; c < C; ++c) {
            const u64 b = a.roff[(u64)c * P + q], e = a.rend[(u64)c * P + q];
            const u64 len = e - b;
            const u64 lo = max(seen, fill_beg), hi = min(seen + len, fill_end);
            for (u64 base = lo; base < hi; base += BLOCK) {
                const u64 i = base + tid;
                const u64 at = b + (i - seen);                // row of the partitioned build array
                bool hit = false;
                if (i < hi) {
                    const uint32_t k = PACKED ? (uint32_t)r64[at] : a.rk[at];
                    if (!chained) {
                        const uint2 a12 = hj_cuckoo_slots<LOG2SLOTS>(k, tf0, tf1);
                        const uint32_t a1 = a12.x, a2 = a12.y;
                        const u64 t1 = tab64[a1], t2 = tab64[a2];
                        hit = ((uint32_t)t1 == k && ((slot_bits[a1 >> 5] >> (a1 & 31)) & 1u)) ||
                              ((uint32_t)t2 == k && ((slot_bits[a2 >> 5] >> (a2 & 31)) & 1u));
                    } else {
                        // the key is in the table (this fill inserted it); a probe that carried it marked every copy
                        uint32_t slot = (k * tf0) >> SHIFT;
                        const uint32_t step = ((k * tf1) >> SHIFT) | 1u;
                        for (uint32_t n = 0; n < SLOTS; ++n) {
                            const uint32_t tk = tab[slot].x;
                            if (tk == k) { hit = (slot_bits[slot >> 5] >> (slot & 31)) & 1u; break; }
                            if (tk == empty) break;
                            slot = (slot + step) & MASK;
                        }
                    }
                }
                const u64 m = __ballot(hit);
                const uint32_t lane = hj_lane(), sh = (uint32_t)at & 31u;
                if (m && (sh == 0 || lane == 0)) {
                    const uint32_t w = (uint32_t)((m >> lane) << sh);      // rows at ... at + 31 - sh = lanes lane ... lane + 31 - sh
                    if (w) atomicOr(&a.build_bits[at >> 5], w);            // global_atomic_or, no return
                }
            }
            seen += len;
        }
    };

    // work items are claimed dynamically (one atomic per item): partitions differ in size
    // and so does the memory system's service, a static round-robin leaves a tail
    // Work-item descriptors are double-buffered: while item n runs out of slot `par`, thread 0
    // claims item n+1 into the other slot at the top of the loop; the clear barrier publishes it,
    // and (single-chunk joins) every lane then loads its share of item n+1's build rows into
    // registers right after item n's build, so that they arrive during the probe of item n.
    __shared__ u64 d_item[2], d_rb[2], d_rn[2];
    __shared__ u64 d_rows_beg[2], d_rows_end[2];      // build rows (of the chunk-concatenated partition) this item inserts
    __shared__ uint32_t d_q[2], d_slice[2], d_nslices[2];
    auto claim = [&](int slot) {                          // thread 0 only
        const u64 w = atomicAdd(a.work_counter, 1ull);
        d_item[slot] = w;
        if (w < total_items) {
            const uint32_t nq = a.item_part[w];
            d_q[slot] = nq;
            // item t of partition q = (probe slice t % nslices, fill group t / nslices), see plan_items_kernel;
            // the divisions are done here, by one thread and one item ahead of use
            const u64 shape = a.slices[nq];
            const uint32_t nslices = (uint32_t)shape, groups = (uint32_t)(shape >> 32);
            const uint32_t t = (uint32_t)(w - a.slice_prefix[nq]);
            const u64 rb = a.roff[nq], rn = a.rend[nq] - rb;
            d_rb[slot] = rb;
            d_rn[slot] = rn;
            d_nslices[slot] = nslices | (a.s_pieces << 24);
            u64 rows = rn;
            for (uint32_t c = 1; c < C; ++c) rows += a.rend[(u64)c * P + nq] - a.roff[(u64)c * P + nq];
            if (groups == 1) {
                // the planned case: the partition fits one table (or its few fills stay with one workgroup)
                d_slice[slot] = t;
                d_rows_beg[slot] = 0;
                d_rows_end[slot] = rows;
            } else {
                // this item's share of the oversize partition's table fills
                const uint32_t group = t / nslices;
                d_slice[slot] = t - group * nslices;
                const uint32_t fills = (uint32_t)((rows + CAP - 1) >> (LOG2SLOTS - 1));
                const uint32_t per_group = (fills + groups - 1) / groups;
                d_rows_beg[slot] = min(rows, (u64)group * per_group * CAP);
                d_rows_end[slot] = min(rows, (u64)(group + 1) * per_group * CAP);
            }
        }
    };
    uint32_t pk[RB], pv[RB];                              // prefetched build rows j*BLOCK + tid
#pragma unroll
    for (int j = 0; j < RB; ++j) { pk[j] = 0; pv[j] = 0; }
    u64 pre_rows = 0;                                     // rows [0, pre_rows) of the coming item are in pk/pv
    int par = 0;
    if (tid == 0) claim(0);
    __syncthreads();
    for (;;) {
        const u64 w = hj_uniform(d_item[par]);
        if (w >= total_items) break;
        q = hj_uniform(d_q[par]);
        const u64 slice = hj_uniform(d_slice[par]);
        const u64 nslices = hj_uniform(d_nslices[par]);            // | extra probe pieces << 24 (probe_item)
        const u64 rows_beg = hj_uniform(d_rows_beg[par]), rows_end = hj_uniform(d_rows_end[par]);
        if (tid == 0) claim(par ^ 1);                     // published by the clear barrier below
        u64 have_rows = pre_rows;
        pre_rows = 0;

        // empty sentinel: smallest value whose partition is not q (P >= 2); broadcast join: a value that no
        // build key equals, found once by broadcast_meta_kernel
        if (a.broadcast) empty = hj_uniform(*a.sentinel);
        else {
            // (pre-partitioned relations: p1_base shifts the pass-1 partition; values of other ranks' partitions wrap to
            // numbers far above P and never equal q)
            empty = 0;
            while ((hj_hash(empty, a.f1, a.F1) - a.p1_base) * a.F2 + hj_hash(empty, a.f2, a.F2) == q) ++empty;
        }
        const u64 EMPTY64 = (u64)empty;
        if (SPLIT) {
            // single-fill items belong to the <UNIQUE, !DEDUP> launch, multi-fill items to <UNIQUE, DEDUP>
            const bool multi = rows_end - rows_beg > CAP;
            if (multi != DEDUP) {
                __syncthreads();                          // everybody has read this item's slot; publishes the next claim
                par ^= 1;
                continue;
            }
            if (DEDUP && !MARKING) for (uint32_t i = tid; i < MATCHED_WORDS; i += BLOCK) matched[i] = 0;    // published by the clear barrier
        }

        for (u64 fill_beg = rows_beg; fill_beg < rows_end; fill_beg += CAP) {
            const u64 fill_end = min(rows_end, fill_beg + CAP);
            // ---- clear + cuckoo build --------------------------------------------
            for (uint32_t i = tid; i < SLOTS; i += BLOCK) tab64[i] = EMPTY64;
            if constexpr (KEEPB) for (uint32_t i = tid; i < SLOTS / 32; i += BLOCK) slot_bits[i] = 0;
            if (tid == 0) cuckoo_failed = a.force_chained;
            __syncthreads();
            auto cuckoo_insert = [&](uint32_t k, uint32_t v) {
                u64 cur = (u64)k | ((u64)v << 32);
                uint32_t loc = (k * tf0) >> SHIFT;
                int it = 0;
                for (; it < CUCKOO_MAX_EVICTIONS; ++it) {
                    const u64 old = atomicExch(&tab64[loc], cur);            // ds_wrxchg_rtn_b64
                    if ((uint32_t)old == empty) break;                       // slot was free
                    // `old` was evicted: it moves to the other one of its two slots
                    const uint2 a12 = hj_cuckoo_slots<LOG2SLOTS>((uint32_t)old, tf0, tf1);
                    loc = (loc == a12.x) ? a12.y : a12.x;
                    cur = old;
                }
                if (it == CUCKOO_MAX_EVICTIONS) cuckoo_failed = 1;           // a tuple is left in hand
            };
            const u64 from_regs = (fill_beg == 0) ? have_rows : 0;
#pragma unroll
            for (int j = 0; j < RB; ++j)
                if ((u64)j * BLOCK + tid < from_regs) cuckoo_insert(pk[j], pv[j]);
            for_each_build_row(fill_beg, fill_end, from_regs, cuckoo_insert);
            __syncthreads();
            // build rows of the NEXT item: issue the loads now, they land during this probe
            // (not in the DEDUP instance: the 16 prefetch registers are what it would spill to scratch, and no shipped
            // kernel may use scratch - see the note at hj_launch_join)
            // (nor in the semi- / anti-join instances: their report path leaves no room for them either, 3 VGPRs spilled)
            if (MODE == HJ_MODE_INNER && !DEDUP && fill_beg == 0 && C == 1 && PACKED && d_item[par ^ 1] < total_items) {
                const u64 nb = d_rb[par ^ 1];
                pre_rows = min(min(d_rn[par ^ 1], (u64)BLOCK * RB), (u64)CAP);
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const u64 i = (u64)j * BLOCK + tid;
                    if (i < pre_rows) { const u64 t = r64[nb + i]; pk[j] = (uint32_t)t; pv[j] = (uint32_t)(t >> 32); }
                }
            }
            if (!cuckoo_failed) {
                if constexpr (MARKING) probe_item(slice, nslices, hj_mark_pass{});
                else probe_item(slice, nslices, probe4_cuckoo);
            } else {
                // ---- fallback: rebuild as double-hashing chains, multi-match probe -----
                __syncthreads();
                for (uint32_t i = tid; i < SLOTS; i += BLOCK) tab64[i] = EMPTY64;
                __syncthreads();
                for_each_build_row(fill_beg, fill_end, 0, [&](uint32_t k, uint32_t v) {
                    uint32_t slot = (k * tf0) >> SHIFT;
                    const uint32_t step = ((k * tf1) >> SHIFT) | 1u;
                    for (;;) {
                        const uint32_t old = atomicCAS(&tab[slot].x, empty, k);   // ds_cmpst_rtn_b32
                        if (old == empty) { tab[slot].y = v; break; }
                        slot = (slot + step) & MASK;
                    }
                });
                __syncthreads();
                if constexpr (MARKING) probe_item(slice, nslices, hj_mark_pass{});
                else probe_item(slice, nslices, probe4_chained);
            }
            if constexpr (KEEPB) {
                __syncthreads();   // every probe of this fill has left its marks
                mark_build_rows(fill_beg, fill_end, cuckoo_failed != 0);
            }
            __syncthreads();   // table is reused by the next fill / work item
        }
        if constexpr (MODE == HJ_MODE_ANTI) {
            // an item without build rows reports all its probe rows; a multi-fill item the rows no fill has marked
            if (DEDUP || rows_beg >= rows_end) {
                anti_tail = true;
                probe_item(slice, nslices, hj_tail_pass{});
                anti_tail = false;
                if (DEDUP) __syncthreads();          // every lane has read `matched` before the next item clears it
            }
        }
        if constexpr (LEFTISH) {
            // the anti-join's tail pass: NULL rows for all probe rows of an item without build rows / the unmarked rows of a multi-fill item
            if (DEDUP || rows_beg >= rows_end) {
                probe_item(slice, nslices, hj_tail_pass{});
                if (DEDUP) __syncthreads();          // every lane has read `matched` before the next item clears it
            }
        }
        if (rows_beg >= rows_end) __syncthreads();   // no fill (a trailing fill group of an oversize partition): publish the next claim
        par ^= 1;
    }

    // ---- per-wave cursors -> final offsets (close_gaps input) ---------------------
    if (a.ok) hj_leave_cursor(a.final_offsets, wave_cursor);

    // ---- workgroup reduction of the aggregates, 4 atomics per workgroup ---------
    hj_add_to_result(red, a.result, acc_n, acc_k, acc_o, acc_i);
}

template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED, bool UNIQUE, bool DEDUP = false, bool NTROWS = true>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void join_kernel(JoinArgs a)
{
    join_body<BLOCK, LOG2SLOTS, BATCH, PACKED, UNIQUE, DEDUP, NTROWS, HJ_MODE_INNER>(a);
}

// Semi- and anti-joins (HJGPU_FLAG_SEMI / _ANTI): the _UNIQUE join's two launches - single-fill items, then multi-fill ones (DEDUP) -
// reporting each probe tuple's match state.  A kernel of its own name: every join_kernel instance is a three-column inner join
// (tests/test_store_policy_isa.py reads them so).  Rows are always non-temporal (no solo instance).
template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED, int MODE, bool DEDUP>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void exists_probe_kernel(JoinArgs a)
{
    join_body<BLOCK, LOG2SLOTS, BATCH, PACKED, true, DEDUP, true, MODE>(a);
}

// Left outer joins (HJGPU_FLAG_LEFT_OUTER): the _UNIQUE join's two launches - single-fill items, then multi-fill ones (DEDUP) - with
// UNIQUE the first-match walk of HJGPU_FLAG_UNIQUE only.  A kernel of its own name, like exists_probe_kernel; rows always non-temporal.
template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED, bool UNIQUE, bool DEDUP>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void outer_probe_kernel(JoinArgs a)
{
    join_body<BLOCK, LOG2SLOTS, BATCH, PACKED, UNIQUE, DEDUP, true, HJ_MODE_LEFT_OUTER>(a);
}

// Right outer joins (HJGPU_FLAG_RIGHT_OUTER): the inner join's single launch (fill groups as planned for it), marking the build rows it hits;
// full outer joins (HJGPU_FLAG_FULL_OUTER): the left outer join's two launches - the first marking likewise - and mark_probe_kernel.  Kernels of their own names; packed
// inputs only (the broadcast join, the one user of column inputs, is bypassed in these modes); rows always non-temporal; no build-row prefetch.
template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void right_probe_kernel(JoinArgs a)
{
    join_body<BLOCK, LOG2SLOTS, BATCH, PACKED, false, false, true, HJ_MODE_RIGHT_OUTER>(a);
}

template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void full_probe_kernel(JoinArgs a)
{
    join_body<BLOCK, LOG2SLOTS, BATCH, PACKED, false, false, true, HJ_MODE_FULL_OUTER>(a);
}

// the marks of a full outer join's multi-fill items (their rows: outer_probe_kernel<.., DEDUP>); aggregate-only by construction
template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void mark_probe_kernel(JoinArgs a)
{
    join_body<BLOCK, LOG2SLOTS, BATCH, PACKED, false, true, true, HJ_MODE_MARK>(a);
}

// Right semi- and anti-joins (HJGPU_FLAG_RIGHT_SEMI / _RIGHT_ANTI): the marks of the single-fill items - the multi-fill items take
// mark_probe_kernel.  Launched without output columns (JoinArgs::ok == NULL): no rows, no aggregates, the waves' cursors stay as they are.
template <int BLOCK, int LOG2SLOTS, int BATCH, bool PACKED>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void mark_single_probe_kernel(JoinArgs a)
{
    join_body<BLOCK, LOG2SLOTS, BATCH, PACKED, false, false, true, HJ_MODE_MARK>(a);
}

// The tail of a right / full outer join: the rows of the partitioned (packed) build array whose bit in a.build_bits is clear leave as
// (key, HJGPU_NULL_VAL, inner_val).  It runs behind the join's launches with the join's grid and block: wave w of workgroup b resumes the
// output block that wave left open (final_offsets), so close_gaps sees one launch's worth of worker slots.  The array is walked piece by
// piece (roff / rend of every partition and chunk: line-aligned partitions have gaps), a piece cut into `split` equal parts so that few
// large pieces still occupy the grid; four tuples (2 x 16 bytes) and their four bits per lane and step.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void build_unmatched_kernel(JoinArgs a, uint32_t split)
{
    constexpr int NW = BLOCK / 64;
    __shared__ u64 red[3][NW];
    __shared__ u64 wave_cursor[NW];
    const int tid = threadIdx.x, wave = tid >> 6;
    EmitterT<true, 3> em;
    em.init(a.ok, a.oov, a.oiv, a.block_size, a.block_limit, a.block_counter, a.overflow, &wave_cursor[wave]);
    if (hj_lane() == 0) wave_cursor[wave] = a.ok ? a.final_offsets[(u64)blockIdx.x * NW + wave] : HJ_NO_CURSOR;
    const uint4 *__restrict__ r4 = reinterpret_cast<const uint4 *>(a.rk);
    const uint32_t *__restrict__ bits = a.build_bits;
    const u64 units = (u64)a.P * a.chunks * split;
    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    for (u64 u = blockIdx.x; u < units; u += gridDim.x) {
        const u64 piece = u / split, part = u - piece * split;
        const u64 b = a.roff[piece], len = a.rend[piece] - b;
        const u64 sb = b + len * part / split, se = b + len * (part + 1) / split;
        for (u64 g = (sb & ~3ull) + (u64)tid * 4; g < se; g += (u64)BLOCK * 4) {
            const uint4 x = r4[g >> 1], y = r4[(g >> 1) + 1];                 // tuples g ... g + 3 (the array ends in 4 spare tuples)
            const uint32_t seen = bits[g >> 5] >> ((uint32_t)g & 31u);          // g is a multiple of 4: the four bits lie in one word
            const uint32_t key[4] = {x.x, x.z, y.x, y.z}, val[4] = {x.y, x.w, y.y, y.w};
            uint32_t rep = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool r = g + j >= sb && g + j < se && !((seen >> j) & 1u);
                rep |= r ? 1u << j : 0u;
                acc_n += r ? 1u : 0u; acc_k += r ? key[j] : 0u; acc_i += r ? val[j] : 0u;
            }
            if (a.ok) {
                const uint32_t none[4] = {HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL};
                if (rep == 15u && a.block_size >= 512) em.emit4(key, none, val);       // (emit4: blocks of 512 rows and more)
                else if (rep) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if ((rep >> j) & 1u) em.emit(key[j], HJGPU_NULL_VAL, val[j]);
                }
            }
        }
    }
    if (a.ok) hj_leave_cursor(a.final_offsets, wave_cursor);
    // (three sums, written out: the reduction as a call changes the schedule of this kernel, see hj_add_to_result)
    acc_n = wave_reduce_sum(acc_n); acc_k = wave_reduce_sum(acc_k); acc_i = wave_reduce_sum(acc_i);
    if (hj_lane() == 0) { red[0][wave] = acc_n; red[1][wave] = acc_k; red[2][wave] = acc_i; }
    __syncthreads();
    if (tid < 3) {
        u64 s = 0;
        for (int i = 0; i < NW; ++i) s += red[tid][i];
        u64 *dst = reinterpret_cast<u64 *>(a.result) + (tid == 2 ? 3 : tid);       // count, sum_keys, sum_inner_vals
        if (s) atomicAdd(dst, s);
    }
}

// The tail of a right semi- / anti-join, build_unmatched_kernel's sibling: the same walk over the partitioned build array, the same grid
// and worker slots.  `flip` = 0: the rows whose bit is clear (right anti-join); ~0: the rows whose bit is set (right semi-join).  Rows
// of two columns, (key, inner_val): a.oiv is the emitter's second column, a.oov is not touched.  No join launch has emitted anything, so
// the cursors it resumes are "no block yet" (a device-planned group: what the groups before it left).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void build_rows_kernel(JoinArgs a, uint32_t split, uint32_t flip)
{
    constexpr int NW = BLOCK / 64;
    __shared__ u64 red[3][NW];
    __shared__ u64 wave_cursor[NW];
    const int tid = threadIdx.x, wave = tid >> 6;
    EmitterT<true, 2> em;
    em.init(a.ok, a.oiv, nullptr, a.block_size, a.block_limit, a.block_counter, a.overflow, &wave_cursor[wave]);
    if (hj_lane() == 0) wave_cursor[wave] = a.ok ? a.final_offsets[(u64)blockIdx.x * NW + wave] : HJ_NO_CURSOR;
    const uint4 *__restrict__ r4 = reinterpret_cast<const uint4 *>(a.rk);
    const uint32_t *__restrict__ bits = a.build_bits;
    const u64 units = (u64)a.P * a.chunks * split;
    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    for (u64 u = blockIdx.x; u < units; u += gridDim.x) {
        const u64 piece = u / split, part = u - piece * split;
        const u64 b = a.roff[piece], len = a.rend[piece] - b;
        const u64 sb = b + len * part / split, se = b + len * (part + 1) / split;
        for (u64 g = (sb & ~3ull) + (u64)tid * 4; g < se; g += (u64)BLOCK * 4) {
            const uint4 x = r4[g >> 1], y = r4[(g >> 1) + 1];                 // tuples g ... g + 3 (the array ends in 4 spare tuples)
            const uint32_t skip = (bits[g >> 5] ^ flip) >> ((uint32_t)g & 31u);   // g is a multiple of 4: the four bits lie in one word
            const uint32_t key[4] = {x.x, x.z, y.x, y.z}, val[4] = {x.y, x.w, y.y, y.w};
            uint32_t rep = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool r = g + j >= sb && g + j < se && !((skip >> j) & 1u);
                rep |= r ? 1u << j : 0u;
                acc_n += r ? 1u : 0u; acc_k += r ? key[j] : 0u; acc_i += r ? val[j] : 0u;
            }
            if (a.ok) {
                if (rep == 15u && a.block_size >= 512) em.emit4(key, val, val);        // (emit4: blocks of 512 rows and more)
                else if (rep) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if ((rep >> j) & 1u) em.emit(key[j], val[j], 0u);
                }
            }
        }
    }
    if (a.ok) hj_leave_cursor(a.final_offsets, wave_cursor);
    acc_n = wave_reduce_sum(acc_n); acc_k = wave_reduce_sum(acc_k); acc_i = wave_reduce_sum(acc_i);
    if (hj_lane() == 0) { red[0][wave] = acc_n; red[1][wave] = acc_k; red[2][wave] = acc_i; }
    __syncthreads();
    if (tid < 3) {
        u64 s = 0;
        for (int i = 0; i < NW; ++i) s += red[tid][i];
        u64 *dst = reinterpret_cast<u64 *>(a.result) + (tid == 2 ? 3 : tid);       // count, sum_keys, sum_inner_vals
        if (s) atomicAdd(dst, s);
    }
}

#include <stdlib.h>
#include <stdio.h>

// Broadcast join metadata (see BroadcastMeta).  One workgroup: a bitmap of the build keys' low 14 bits in LDS
// (inner < 16384 keys cannot occupy all 16384 residues), the first free residue is the sentinel.
__global__ __launch_bounds__(1024) void broadcast_meta_kernel(const uint32_t *__restrict__ keys, u64 inner, u64 outer,
                                                               uint32_t nslices, uint32_t groups, BroadcastMeta m)
{
    __shared__ uint32_t bits[512];
    __shared__ uint32_t first_free;
    for (uint32_t i = threadIdx.x; i < 512; i += 1024) bits[i] = 0;
    if (threadIdx.x == 0) first_free = 0xFFFFFFFFu;
    __syncthreads();
    for (u64 i = threadIdx.x; i < inner; i += 1024) {
        const uint32_t r = keys[i] & 16383u;
        atomicOr(&bits[r >> 5], 1u << (r & 31));
    }
    __syncthreads();
    if (threadIdx.x < 512) {
        const uint32_t free_bits = ~bits[threadIdx.x];
        if (free_bits) atomicMin(&first_free, threadIdx.x * 32 + (uint32_t)__builtin_ctz(free_bits));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        hj_store(m.sentinel, first_free);
        hj_store(&m.roff[0], (u64)0); hj_store(&m.rend[0], inner); hj_store(&m.soff[0], (u64)0); hj_store(&m.send[0], outer);
        hj_store(&m.slice_prefix[0], (u64)0); hj_store(&m.slice_prefix[1], (u64)nslices * groups);
        hj_store(&m.slices[0], (u64)nslices | ((u64)groups << 32));
    }
}

int hj_launch_broadcast_meta(const uint32_t *inner_keys, size_t inner, size_t outer, uint32_t nslices,
                             uint32_t groups, const BroadcastMeta &m, hipStream_t stream)
{
    // (inner == 0: an anti-join with no build rows - every item reports its whole probe slice)
    if (inner > 16383 || nslices == 0 || groups == 0) return HJGPU_EINVAL;
    hipLaunchKernelGGL(broadcast_meta_kernel, dim3(1), dim3(1024), 0, stream, inner_keys, (u64)inner, (u64)outer,
                       nslices, groups, m);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

const JoinConfig &hj_join_config_big()
{
    static const JoinConfig cfg = {1024, 14, 2};
    return cfg;
}

// workgroups per CU the LDS table allows (160 KiB per CU, + 9 KiB: the UNIQUE instances' `matched` bits; the same grid for both keeps
// hj_join_workers one number), capped by 2048 threads per CU
static int join_grid(int cus, const JoinConfig &c) { return cus * hj_join_wgs_per_cu(c.block, c.log2slots); }
// Worker slots (final_offsets entries, one open output block each) of a join: one per wave of ONE launch.  A _UNIQUE join is
// two launches (see join_kernel) of the same grid; the second half's waves continue in the first half's open blocks.
int hj_join_workers(const HjTuning &t, int cus, bool big_tables)
{
    const JoinConfig &c = hj_join_config_of(t, big_tables);
    return join_grid(cus, c) * (c.block / 64);
}

// The geometries that are built (option "join_cfg"): {block, log2slots, batch, a UNIQUE instance exists}.
// NO SHIPPED INSTANCE MAY USE SCRATCH (tests/test_kernel_resources.py reads the compiler's remarks): a K6 instance with a
// private segment loses stores next to other streams' kernels (DESIGN section 3 "Round 4": found by round 3's multi-GPU
// stress runs, narrowed down in round 4 - the private values themselves are never wrong; the cause is below the ISA), and
// nothing says the other kernels would be exempt.  The multi-fill half of a _UNIQUE join (<UNIQUE, DEDUP>) therefore runs
// with ONE probe vector per lane and without the build-row prefetch (what fits 128 VGPRs), and the geometries that
// spill (512,13,1 and 512,13,4 without _UNIQUE) are not built.
static const struct { int block, log2slots, batch; bool unique; } JOIN_BUILT[] = {
    {512, 13, 2, true}, {1024, 14, 2, true}, {256, 12, 2, false},
};

bool hj_join_config_built(const JoinConfig &c, bool unique)
{
    for (const auto &g : JOIN_BUILT)
        if (g.block == c.block && g.log2slots == c.log2slots && g.batch == c.batch && (!unique || g.unique)) return true;
    return false;
}

// The launches of one join at geometry (B, L), all with the same grid on the same stream.  `first`: the join's arguments as they are.
// `multi`: the multi-fill items of a join of two launches (see join_kernel) - a _UNIQUE join (join_kernel), a semi- or anti-join
// (exists_probe_kernel), a left outer join (outer_probe_kernel, with the first-match walk or without it) - at one vector per lane, with
// their own work counter.  `mark`: a full outer join's third launch, the marks of its multi-fill items (their rows: the left outer
// join's multi-fill instance as it is), with the third work counter and no rows.  A right outer join is one launch, as the inner join;
// a right semi- or anti-join is `first` = mark_single_probe_kernel and `mark`, both without rows (no `multi`: nothing is reported here).
// Right and full outer, right semi- and anti-joins take packed inputs only.  SPLIT: the geometry has the instances of the joins of several launches.
// (the plain-row instances serve solo materialising joins only; aggregate-only joins never emit: the NTROWS = true instance)
typedef void (*JoinKernel)(JoinArgs);
struct JoinLaunches { JoinKernel first, multi, mark; };

// the inner join: join_kernel, the geometry's one batch (2) or, under _UNIQUE, its two launches; `nt`: the NTROWS instances
template <int B, int L, bool SPLIT>
static JoinLaunches inner_join_kernels(bool packed, bool unique, bool nt, int batch)
{
    JoinLaunches k = {nullptr, nullptr, nullptr};
    hj_with_bool(packed, [&](auto p) {
        hj_with_bool(nt, [&](auto r) {
            constexpr bool P = decltype(p)::value, NT = decltype(r)::value;
            if (!unique) {
                if (batch == 2) k.first = join_kernel<B, L, 2, P, false, false, NT>;
            } else if constexpr (SPLIT) {
                k.first = join_kernel<B, L, 2, P, true, false, NT>;
                k.multi = join_kernel<B, L, 1, P, true, true, NT>;
            }
        });
    });
    return k;
}

// every other mode (SPLIT geometries only); rows always non-temporal
template <int B, int L>
static JoinLaunches mode_join_kernels(uint32_t mode, bool packed, bool unique)
{
    JoinLaunches k = {nullptr, nullptr, nullptr};
    if (hj_mode_marks_build(mode)) {
        if (!packed) return k;
        if (mode == HJ_MODE_RIGHT_OUTER) k.first = right_probe_kernel<B, L, 2, true>;
        else if (hj_mode_reports_build(mode)) {
            k.first = mark_single_probe_kernel<B, L, 2, true>;
            k.mark = mark_probe_kernel<B, L, 1, true>;
        } else {
            k.first = full_probe_kernel<B, L, 2, true>;
            k.multi = outer_probe_kernel<B, L, 1, true, false, true>;
            k.mark = mark_probe_kernel<B, L, 1, true>;
        }
        return k;
    }
    hj_with_bool(packed, [&](auto p) {
        constexpr bool P = decltype(p)::value;
        if (mode == HJ_MODE_SEMI) {
            k.first = exists_probe_kernel<B, L, 2, P, HJ_MODE_SEMI, false>;
            k.multi = exists_probe_kernel<B, L, 1, P, HJ_MODE_SEMI, true>;
        } else if (mode == HJ_MODE_ANTI) {
            k.first = exists_probe_kernel<B, L, 2, P, HJ_MODE_ANTI, false>;
            k.multi = exists_probe_kernel<B, L, 1, P, HJ_MODE_ANTI, true>;
        } else if (mode == HJ_MODE_LEFT_OUTER) {
            hj_with_bool(unique, [&](auto u) {
                constexpr bool U = decltype(u)::value;
                k.first = outer_probe_kernel<B, L, 2, P, U, false>;
                k.multi = outer_probe_kernel<B, L, 1, P, U, true>;
            });
        }
    });
    return k;
}

template <int B, int L, bool SPLIT>
static int launch_join_at(const JoinArgs &b, int batch, int grid, hipStream_t stream)
{
    JoinLaunches k = {nullptr, nullptr, nullptr};
    if (b.mode == HJ_MODE_INNER) k = inner_join_kernels<B, L, SPLIT>(b.packed != 0, b.unique != 0, !(b.ok && !b.nt_rows), batch);
    else if constexpr (SPLIT) k = mode_join_kernels<B, L>(b.mode, b.packed != 0, b.unique != 0);
    // a geometry without this join's instances (hj_join_config_built), column inputs to a right / full outer join, no third counter
    if (!k.first || (k.mark && !b.work_counter3)) return HJGPU_EINVAL;
    const JoinKernel kernels[3] = {k.first, k.multi, k.mark};
    u64 *const counters[3] = {b.work_counter, b.work_counter2, b.work_counter3};
    for (int i = 0; i < 3; ++i) {
        if (!kernels[i]) continue;
        JoinArgs d = b;
        d.work_counter = counters[i];
        if (i == 2 || hj_mode_reports_build(b.mode)) d.ok = nullptr;     // the marking launches report nothing
        hipLaunchKernelGGL(kernels[i], dim3(grid), dim3(B), 0, stream, d);
    }
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_build_unmatched(const JoinArgs &a, const HjTuning &t, int cus, hipStream_t stream)
{
    if (!a.packed || !a.build_bits || a.P < 1 || a.chunks == 0 || (a.ok && !a.final_offsets)) return HJGPU_EINVAL;
    const JoinConfig &c = hj_join_config_of(t, a.big_tables != 0);
    const int grid = join_grid(cus, c);
    const u64 pieces = (u64)a.P * a.chunks;
    u64 split = (u64)grid * 4 / pieces;
    split = split < 1 ? 1 : split > 4096 ? 4096 : split;
    if (c.block == 512) hipLaunchKernelGGL((build_unmatched_kernel<512>), dim3(grid), dim3(512), 0, stream, a, (uint32_t)split);
    else if (c.block == 1024) hipLaunchKernelGGL((build_unmatched_kernel<1024>), dim3(grid), dim3(1024), 0, stream, a, (uint32_t)split);
    else return HJGPU_EINVAL;
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_build_rows(const JoinArgs &a, const HjTuning &t, int cus, hipStream_t stream)
{
    if (!hj_mode_reports_build(a.mode) || !a.packed || !a.build_bits || a.P < 1 || a.chunks == 0 || (a.ok && (!a.final_offsets || !a.oiv))) return HJGPU_EINVAL;
    const JoinConfig &c = hj_join_config_of(t, a.big_tables != 0);
    const int grid = join_grid(cus, c);
    const u64 pieces = (u64)a.P * a.chunks;
    u64 split = (u64)grid * 4 / pieces;
    split = split < 1 ? 1 : split > 4096 ? 4096 : split;
    const uint32_t flip = a.mode == HJ_MODE_RIGHT_SEMI ? ~0u : 0u;
    if (c.block == 512) hipLaunchKernelGGL((build_rows_kernel<512>), dim3(grid), dim3(512), 0, stream, a, (uint32_t)split, flip);
    else if (c.block == 1024) hipLaunchKernelGGL((build_rows_kernel<1024>), dim3(grid), dim3(1024), 0, stream, a, (uint32_t)split, flip);
    else return HJGPU_EINVAL;
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_join(const JoinArgs &a, const HjTuning &t, int cus, hipStream_t stream)
{
    if ((a.P < 2 && !a.broadcast) || a.P < 1 || a.chunks == 0) return HJGPU_EINVAL;
    const JoinConfig &c = hj_join_config_of(t, a.big_tables != 0);
    JoinArgs b = a;
    b.force_chained = t.force_chained ? 1u : 0u;       // tests: exercise the fallback table everywhere
    b.unique = (a.unique || t.unique) ? 1u : 0u;
    if ((b.unique || b.mode) && !b.work_counter2) return HJGPU_EINVAL;
    if (hj_mode_keeps_build(b.mode) && (b.unique || !b.build_bits)) return HJGPU_EINVAL;
    if (hj_mode_reports_build(b.mode) && !b.build_bits) return HJGPU_EINVAL;      // (unique: ignored, the marking walk stops at the first hit anyway)
    const int grid = join_grid(cus, c);
    if (c.block == 512 && c.log2slots == 13) return launch_join_at<512, 13, true>(b, c.batch, grid, stream);
    if (c.block == 1024 && c.log2slots == 14) return launch_join_at<1024, 14, true>(b, c.batch, grid, stream);
    if (c.block == 256 && c.log2slots == 12) return launch_join_at<256, 12, false>(b, c.batch, grid, stream);
    return HJGPU_EINVAL;
}

// --------------------------------------------------------------------------
// LDS look-up (hjgpu_lookup*, DESIGN.md section 5 "LDS look-up"): the positional look-up (npj_kernels.hip "Positional look-up") for a build
// side that fits ONE LDS table.  One persistent grid; every workgroup fills its own table ONCE from the caller's build columns (L2-hot
// after the first workgroups) - join_body's fill: cuckoo insertion, double-hashing chains when that does not converge or under option
// "force_chained" - and then streams the probe column in whole-wave trips of 256 consecutive rows: lane v owns rows 4 v ... 4 v + 3 of a
// trip, BATCH trips in flight per wave.  No work items, no claims, no block protocol.  The empty sentinel is key 0: a build key 0 is
// refused anyway (the fill raises DevState::zero_key and skips the row), a probe key 0 matches nothing.  The chained fill drops a row
// whose key is already in the table (the CAS returns the key itself): any copy may answer, and a heavily duplicated key builds no chain.
// The probe's LDS reads: one ds_read_b64 per slot, key and payload together (bank = (address / 4) % 64 over each half of the wave; the
// slots are hashed, so the conflicts are those of 32 independent addresses over 32 slot-wide bank pairs, whatever the layout - a split
// key / payload layout halves the bytes per slot but pays a second, dependent read per hit and loses the 64-bit exchange of the fill).
// Selected LDS look-up (hjgpu_lookup_selected*, DESIGN.md section 5 "Selected look-up"), SEL: the same body for the rows whose bit is set
// in select_bits.  The same two geometries and the same fill, which never looks at the mask - it is what finds a build key 0.  An
// unselected row is never valid: no read of the table, HJGPU_NULL_VAL, bit 0, counted nowhere.  The head and the end of a trip are
// hj_lookup.hpp's, where the in-place rule (match_bits == select_bits) is kept.
// --------------------------------------------------------------------------
// The one fill of a workgroup's table: clear, cuckoo build, and the table again as double-hashing chains when that does not converge or
// under force_chained.  All threads of the workgroup; returns whether the table is chained.  A build key 0 raises *zero_key and is skipped.
struct LdsFill { const uint32_t *rk, *rv; uint32_t inner, tf0, tf1, force_chained; uint32_t *zero_key; };
template <int BLOCK, int LOG2SLOTS>
__device__ __forceinline__ bool lds_lookup_fill(const LdsFill &a, u64 *tab64, uint32_t &cuckoo_failed)
{
    constexpr uint32_t SLOTS = 1u << LOG2SLOTS;
    constexpr uint32_t MASK = SLOTS - 1;
    constexpr int SHIFT = 32 - LOG2SLOTS;
    constexpr int RB = 8;                        // build rows a lane loads before inserting
    constexpr int CUCKOO_MAX_EVICTIONS = 64;
    uint2 *tab = reinterpret_cast<uint2 *>(tab64);   // chained view: .x = key, .y = payload
    const uint32_t tid = threadIdx.x;
    const uint32_t tf0 = a.tf0, tf1 = a.tf1, inner = a.inner;

    // every row of the build side, a lane's RB loads issued before its first insert
    auto for_each_build_row = [&](auto insert) {
        for (uint32_t base = 0; base < inner; base += (uint32_t)BLOCK * RB) {
            uint32_t k[RB], v[RB];
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const uint32_t i = base + (uint32_t)j * BLOCK + tid;
                k[j] = 0; v[j] = 0;
                if (i < inner) { k[j] = a.rk[i]; v[j] = a.rv[i]; }
            }
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const uint32_t i = base + (uint32_t)j * BLOCK + tid;
                if (i < inner) insert(k[j], v[j]);
            }
        }
    };

    // ---- the one fill: clear + cuckoo build ----------------------------------
    for (uint32_t i = tid; i < SLOTS; i += BLOCK) tab64[i] = 0;
    if (tid == 0) cuckoo_failed = a.force_chained;
    __syncthreads();
    for_each_build_row([&](uint32_t k, uint32_t v) {
        if (k == 0) { atomicOr(a.zero_key, 1u); return; }                // 0 is "empty": refused (HJGPU_EZEROKEY), the row is skipped
        u64 cur = (u64)k | ((u64)v << 32);
        uint32_t loc = (k * tf0) >> SHIFT;
        int it = 0;
        for (; it < CUCKOO_MAX_EVICTIONS; ++it) {
            const u64 old = atomicExch(&tab64[loc], cur);                // ds_wrxchg_rtn_b64
            if ((uint32_t)old == 0u) break;                              // slot was free
            // `old` was evicted: it moves to the other one of its two slots
            const uint2 a12 = hj_cuckoo_slots<LOG2SLOTS>((uint32_t)old, tf0, tf1);
            loc = (loc == a12.x) ? a12.y : a12.x;
            cur = old;
        }
        if (it == CUCKOO_MAX_EVICTIONS) cuckoo_failed = 1;               // a tuple is left in hand
    });
    __syncthreads();
    const bool chained = hj_uniform(cuckoo_failed) != 0;
    if (chained) {
        // ---- fallback: the table again as double-hashing chains, one copy per key ----
        for (uint32_t i = tid; i < SLOTS; i += BLOCK) tab64[i] = 0;
        __syncthreads();
        for_each_build_row([&](uint32_t k, uint32_t v) {
            if (k == 0) return;
            uint32_t slot = (k * tf0) >> SHIFT;
            const uint32_t step = ((k * tf1) >> SHIFT) | 1u;
            for (;;) {
                const uint32_t old = atomicCAS(&tab[slot].x, 0u, k);     // ds_cmpst_rtn_b32
                if (old == 0u) { tab[slot].y = v; break; }
                if (old == k) break;                                     // a copy of this key is in the table already
                slot = (slot + step) & MASK;
            }
        });
        __syncthreads();
    }

    return chained;
}

template <bool SEL, int BLOCK, int LOG2SLOTS, bool VALS, bool BITS>
__device__ __forceinline__ void lds_lookup_body(const LdsLookupArgs &a, const uint32_t *select_bits)
{
    constexpr uint32_t SLOTS = 1u << LOG2SLOTS;
    constexpr uint32_t MASK = SLOTS - 1;
    constexpr int SHIFT = 32 - LOG2SLOTS;
    constexpr int NW = BLOCK / 64;
    constexpr int BATCH = 2;                     // probe vectors (wave trips) in flight per lane
    __shared__ u64 tab64[SLOTS];                 // low word = key (0: empty), high word = build payload
    __shared__ u64 red[4][NW];
    __shared__ uint32_t cuckoo_failed;
    uint2 *tab = reinterpret_cast<uint2 *>(tab64);   // chained view: .x = key, .y = payload
    const uint32_t tid = threadIdx.x;
    const uint32_t tf0 = a.tf0, tf1 = a.tf1;
    const bool chained = lds_lookup_fill<BLOCK, LOG2SLOTS>({a.rk, a.rv, a.inner, tf0, tf1, a.force_chained, a.zero_key}, tab64, cuckoo_failed);

    // ---- probe: whole waves iterate together (the bitmaps' words need all lanes); the probe column is read exactly once ----
    const uint4 *__restrict__ k4 = reinterpret_cast<const uint4 *>(a.keys);
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    for (u64 v0 = (u64)blockIdx.x * BLOCK + (tid & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t look[BATCH];
        uint4 kk[BATCH];
        lookup_fetch<SEL, BATCH>(select_bits, k4, v0, stride, n, look, kk);
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            if (v0 + (u64)u * stride >= nvec) break;                     // the wave's trip lies beyond the column (the same for all its lanes)
            const u64 v = v0 + (u64)u * stride + hj_lane();
            const uint32_t key[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
            uint32_t res[4] = {HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL};
            uint32_t nib = 0;
            bool valid[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) valid[j] = key[j] != 0u && ((look[u] >> j) & 1u);
            if (!chained) {
                // cuckoo table: a key lives in one of two slots - two independent reads per key, no loop.  The plain kernel issues them
                // for every key, the selected one for the valid keys only
                u64 t1[4], t2[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    t1[j] = 0; t2[j] = 0;
                    bool read = true;
                    if constexpr (SEL) read = valid[j];
                    if (read) {
                        const uint2 at = hj_cuckoo_slots<LOG2SLOTS>(key[j], tf0, tf1);
                        t1[j] = tab64[at.x];
                        t2[j] = tab64[at.y];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool h1 = valid[j] && (uint32_t)t1[j] == key[j], h2 = valid[j] && (uint32_t)t2[j] == key[j];
                    if (h1 || h2) { res[j] = (uint32_t)((h1 ? t1[j] : t2[j]) >> 32); nib |= 1u << j; }
                }
            } else {
                // chains: 4 walks per lane in lock step, each to the key's copy or to the first empty slot
                uint32_t slot[4], step[4];
                uint2 t[4];
                bool live[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    live[j] = valid[j];
                    slot[j] = (key[j] * tf0) >> SHIFT;
                    step[j] = ((key[j] * tf1) >> SHIFT) | 1u;
                    t[j] = make_uint2(0u, 0u);
                    if (live[j]) t[j] = tab[slot[j]];
                }
                for (;;) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool hit = live[j] && t[j].x == key[j];
                        if (hit) { res[j] = t[j].y; nib |= 1u << j; }
                        live[j] = live[j] && t[j].x != 0u && !hit;
                        slot[j] = (slot[j] + step[j]) & MASK;
                    }
                    if (!(live[0] | live[1] | live[2] | live[3])) break;
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (live[j]) t[j] = tab[slot[j]];
                }
            }
            lookup_leave<VALS, BITS>(a.vals_out, a.match_bits, n, v, key, res, nib, acc_n, acc_k, acc_i);
        }
    }
    hj_add_to_result(red, a.result, acc_n, acc_k, 0ull, acc_i);
}

template <int BLOCK, int LOG2SLOTS, bool VALS, bool BITS>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void lds_lookup_kernel(LdsLookupArgs a)
{
    lds_lookup_body<false, BLOCK, LOG2SLOTS, VALS, BITS>(a, nullptr);
}

template <int BLOCK, int LOG2SLOTS, bool VALS, bool BITS>
__global__ __launch_bounds__(BLOCK, hj_join_waves_per_simd(BLOCK, LOG2SLOTS)) void lds_lookup_sel_kernel(LdsLookupSelArgs a)
{
    lds_lookup_body<true, BLOCK, LOG2SLOTS, VALS, BITS>(a, a.select_bits);
}

// <512, 13> for build sides of up to 4096 rows (two workgroups per CU), <1024, 14> above (one): the broadcast join's pair, whatever
// option "join_cfg" says.  One persistent grid, no larger than the probe column has wave trips for; always at least one workgroup - the
// fill is what finds a build key 0, also when there is nothing to probe.  a.select_bits == NULL: the plain kernel on the base slice.
template <int B, int L>
static int launch_lds_lookup_at(const LdsLookupSelArgs &a, int cus, hipStream_t stream)
{
    const u64 nvec = ((u64)a.n + 3) >> 2, need = (nvec + B - 1) / B, full = (u64)cus * hj_join_wgs_per_cu(B, L);
    const u64 grid = need < 1 ? 1 : need < full ? need : full;
    void (*plain)(LdsLookupArgs) = nullptr;
    void (*selected)(LdsLookupSelArgs) = nullptr;
    hj_with_bool(a.vals_out != nullptr, [&](auto vals) {
        hj_with_bool(a.match_bits != nullptr, [&](auto bits) {
            constexpr bool V = decltype(vals)::value, M = decltype(bits)::value;
            plain = lds_lookup_kernel<B, L, V, M>;
            selected = lds_lookup_sel_kernel<B, L, V, M>;
        });
    });
    if (a.select_bits) hipLaunchKernelGGL(selected, dim3((uint32_t)grid), dim3(B), 0, stream, a);
    else hipLaunchKernelGGL(plain, dim3((uint32_t)grid), dim3(B), 0, stream, static_cast<const LdsLookupArgs &>(a));
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_lds_lookup(const LdsLookupSelArgs &a, int cus, hipStream_t stream)
{
    if (a.inner == 0 && a.n == 0) return HJGPU_OK;
    if (!a.result || !a.zero_key || (a.n && !a.keys) || (a.inner && (!a.rk || !a.rv)) || cus < 1) return HJGPU_EINVAL;
    if (a.inner > (uint32_t)hj_join_config_big().cap() || !(a.tf0 & 1u) || !(a.tf1 & 1u)) return HJGPU_EINVAL;
    if (((uintptr_t)a.keys | (uintptr_t)a.vals_out | (uintptr_t)a.match_bits | (uintptr_t)a.select_bits) & 15) return HJGPU_EINVAL;
    if (a.inner <= 4096) return launch_lds_lookup_at<512, 13>(a, cus, stream);
    return launch_lds_lookup_at<1024, 14>(a, cus, stream);
}
