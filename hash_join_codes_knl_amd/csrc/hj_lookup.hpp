// hj_lookup.hpp — what the six look-up kernels share (npj_lookup_line_kernel, npj_lookup_kernel, lds_lookup_kernel and their selected
// forms npj_lookup_sel_line_kernel, npj_lookup_sel_kernel, lds_lookup_sel_kernel; DESIGN.md section 5 "Positional look-up", "LDS look-up",
// "Selected look-up"): the head of a loop iteration, which loads the select words (SEL) and then the keys of all its wave trips, and the
// end of a trip.  A wave trip is 256 consecutive rows: lane L owns rows 4 L ... 4 L + 3, a group of 8 lanes owns one word of either bitmap
// and one 128-byte line of the key column.
// THE IN-PLACE RULE.  match_bits may be the very pointer select_bits, so a bitmap word is read only by the wave that stores it, and before
// it stores it: lookup_fetch loads word v / 8 in the 8 lanes whose vectors make it up, lookup_leave stores it from the first of them, and
// the store is issued behind the walk that waited for the load.  Neither pointer is __restrict__: the compiler keeps a load of select_bits
// in front of every earlier store through match_bits.
// The same rule for a COLUMN: gather_kernel (gen_kernels.hip) hands lookup_fetch its index column in the key column's place, and one of
// its output columns may be that very pointer.  Vector v of the index is loaded by one lane only, the lane that stores vector v of every
// output column, and lookup_fetch has loaded all vectors of an iteration before the iteration's first store: a lane reads its index
// vector before it stores the same vector, and no other lane, wave or iteration ever reads it.
#pragma once
#include "hj_device.hpp"

__device__ __forceinline__ uint32_t hj_load_nt(const uint32_t *p) { return __builtin_nontemporal_load(p); }

// The head of an iteration of BATCH wave trips (trip u: vectors v0 + u * stride + lane).  nib[u] = the bits of this lane's four rows that
// are to be looked up, 0 for a row at n or beyond; kk[u] is 0 where nothing was loaded.  The last, partial vector is loaded whole: up to
// 12 bytes past row n are read and masked out by nib; the column's 16-byte alignment keeps them inside its allocation.
// SEL: all select words first, then the keys, so that the dependent load is paid once per iteration.  nib[u] = the select bits of the
// rows below n (whatever the last word holds beyond); no word at index >= (n + 31) / 32 is read.  A group of 8 lanes whose word is 0
// loads no keys: its 32 rows are one 128-byte line of the column.
// Without SEL no mask is read (select_bits is not looked at) and nib[u] = the rows below n.  NT: the keys are loaded non-temporally (the
// selected kernels and the LDS look-up: the column is read exactly once) or with an ordinary load (the plain NPJ look-ups).
template <bool SEL, int BATCH, bool NT = true>
__device__ __forceinline__ void lookup_fetch(const uint32_t *select_bits, const uint4 *k4, u64 v0, u64 stride, u64 n, uint32_t (&nib)[BATCH],
                                             uint4 (&kk)[BATCH])
{
    const u64 nvec = (n + 3) >> 2;
    uint32_t w[BATCH];
    if constexpr (SEL) {
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const u64 v = v0 + (u64)u * stride + hj_lane();
            w[u] = 0;
            if (v < nvec) w[u] = hj_load_nt(select_bits + (v >> 3));    // (v < nvec: row 4 v < n, and word v / 8 starts at or before it)
        }
    }
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
        const u64 v = v0 + (u64)u * stride + hj_lane(), g = v << 2;
        kk[u] = make_uint4(0, 0, 0, 0);
        if constexpr (SEL) { if (w[u] != 0u) kk[u] = hj_load_nt(k4 + v); }  // (w != 0 only where v < nvec)
        else if (v < nvec) kk[u] = NT ? hj_load_nt(k4 + v) : k4[v];
        const uint32_t rows = g + 4 <= n ? 15u : g < n ? (1u << (uint32_t)(n - g)) - 1u : 0u;
        if constexpr (SEL) nib[u] = (w[u] >> ((threadIdx.x & 7u) * 4)) & rows;
        else nib[u] = rows;
    }
}

// The end of a wave trip, all 64 lanes (the bitmap's words are combined across lanes): v = this lane's vector, res / hit = the answers and
// match bits of its four rows.  hit is 0 for every row that was not looked up - unselected, or at n and beyond -, so the stored word is
// select AND match and the last word's high bits leave as 0.
template <bool VALS, bool BITS>
__device__ __forceinline__ void lookup_leave(uint32_t *vals_out, uint32_t *match_bits, u64 n, u64 v, const uint32_t (&kc)[4], const uint32_t (&res)[4],
                                             uint32_t hit, u64 &acc_n, u64 &acc_k, u64 &acc_i)
{
    const u64 g = v << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool h = (hit >> j) & 1u;
        acc_n += h ? 1u : 0u; acc_k += h ? kc[j] : 0u; acc_i += h ? res[j] : 0u;
    }
    if constexpr (VALS) {
        if (g + 4 <= n) hj_store(reinterpret_cast<uint4 *>(vals_out) + v, make_uint4(res[0], res[1], res[2], res[3]));
        else {                                                  // the last, partial vector: nothing at n and beyond is written
#pragma unroll
            for (int j = 0; j < 3; ++j) if (g + j < n) hj_store(vals_out + g + j, res[j]);
        }
    }
    if constexpr (BITS) {
        // 8 lanes x 4 rows = one word: OR over each group of 8 lanes, its first lane stores
        uint32_t w = hit << ((threadIdx.x & 7u) * 4);
        w |= hj_dpp<0xB1>(w);                                   // quad_perm: lanes 0<->1, 2<->3
        w |= hj_dpp<0x4E>(w);                                   // quad_perm: lanes 0<->2, 1<->3
        w |= hj_dpp<0x141>(w);                                  // row_half_mirror: lane i <-> 7 - i of the group, the other quad
        // (v is a multiple of 8 in the storing lane: word v / 8 starts at row 4 v; a word whose first row is at n or beyond is not stored)
        if ((threadIdx.x & 7u) == 0 && g < n) hj_store(match_bits + (v >> 3), w);
    }
}
