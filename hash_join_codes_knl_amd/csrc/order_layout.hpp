// order_layout.hpp - the key normalisation, the digit passes and the geometry of hjgpu_order_by (gen_kernels.hip order_*_kernel, DESIGN.md
// section 5 "Order by").  Plain host arithmetic, no HIP: the launchers and the kernels share it with tests/test_order_layout.py, which
// compiles it with g++, walks the ranges and runs the whole pass sequence on the CPU.
//
// The operator sorts a PERMUTATION - uint32 row numbers, first the selected rows ascending - by least-significant-digit radix passes of
// 8 bits: from the last key's lowest digit to the first key's highest, every pass a stable counting sort by digit(key[perm[i]]).  A key
// is normalised to an unsigned word whose plain order is the wanted one: the sign bit flipped under HJGPU_ORDER_SIGNED, every bit
// complemented under HJGPU_ORDER_DESC.  Both are one XOR, so a pass needs one 32-bit word of the key - the low or the high half of a
// 64-bit one - an XOR mask and a shift (Pass).
//
// n <= LDS_ROWS: one workgroup sorts in LDS (the LDS road).  Beyond, the current permutation [0, J) is cut as compact_layout.hpp cuts its
// rows: `ranges` contiguous ranges of whole chunks laid out from n (J is known on the device alone), the tail in the last non-empty one.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HJ_ORDER_HD __host__ __device__
#else
#define HJ_ORDER_HD
#endif

namespace hj_order {
typedef unsigned long long u64;

constexpr uint32_t MAX_KEYS = 4, MAX_COLS = 8;          // HJGPU_ORDER_MAX_KEYS, HJGPU_ORDER_MAX_COLS
constexpr uint32_t DESC = 1, SIGNED = 2, WIDE = 4;      // HJGPU_ORDER_DESC, _SIGNED, _WIDE
constexpr uint32_t DIGIT_BITS = 8, DIGITS = 1u << DIGIT_BITS;
constexpr uint32_t MAX_PASSES = MAX_KEYS * 8;           // four 64-bit keys

// the LDS road: one workgroup of LDS_BLOCK lanes, LDS_ITEMS rows per lane
constexpr uint32_t LDS_BLOCK = 1024, LDS_ITEMS = 8;
constexpr uint32_t LDS_ROWS = LDS_BLOCK * LDS_ITEMS;    // hjgpu_get_counter "order_lds_rows"
// the device road: workgroups of BLOCK lanes, ITEMS rows per lane and chunk
constexpr uint32_t BLOCK = 256, ITEMS = 8;
constexpr uint32_t CHUNK_ROWS = BLOCK * ITEMS;          // hjgpu_get_counter "order_chunk_rows"
constexpr uint32_t MAX_RANGES = 1024;
constexpr uint32_t RESIDENT = 4;                        // workgroups of BLOCK lanes per CU: the grid of the histogram and scatter launches

// hjgpu_get_counter "order_ranges"
inline uint32_t ranges_of(int cus)
{
    const u64 g = (u64)(cus < 1 ? 1 : cus) * RESIDENT;
    return (uint32_t)(g < MAX_RANGES ? g : MAX_RANGES);
}

inline bool lds_road(u64 n) { return n <= LDS_ROWS; }

// ---- normalisation and digits -----------------------------------------------------------------------------------------------------------
// the XOR that turns a key's 32-bit word into its normalised word; top: the word holds the key's sign bit (a 32-bit key's only word, a
// 64-bit key's high half)
HJ_ORDER_HD inline uint32_t xor_of(uint32_t flags, bool top)
{
    return ((flags & SIGNED) && top ? 0x80000000u : 0u) ^ ((flags & DESC) ? 0xFFFFFFFFu : 0u);
}
HJ_ORDER_HD inline uint32_t norm32(uint32_t x, uint32_t flags) { return x ^ xor_of(flags, true); }
HJ_ORDER_HD inline u64 norm64(u64 x, uint32_t flags) { return x ^ (((u64)xor_of(flags, true) << 32) | xor_of(flags, false)); }
// a key of either width as the 64-bit word the LDS road carries (a 32-bit key: its normalised word, the high half 0)
HJ_ORDER_HD inline u64 norm(u64 x, uint32_t flags) { return (flags & WIDE) ? norm64(x, flags) : (u64)norm32((uint32_t)x, flags); }
HJ_ORDER_HD inline uint32_t digits_of(uint32_t flags) { return (flags & WIDE) ? 8u : 4u; }
// digit d (0: the lowest) of a normalised word
HJ_ORDER_HD inline uint32_t digit(u64 normalised, uint32_t d) { return (uint32_t)(normalised >> (d * DIGIT_BITS)) & (DIGITS - 1u); }

// One pass of the device road: the digit is ((words[row * stride + word] ^ xor_mask) >> shift) & 255 of key column `key`
struct Pass {
    uint32_t key, stride, word, shift, xor_mask;
};
HJ_ORDER_HD inline uint32_t pass_digit(uint32_t w, uint32_t xor_mask, uint32_t shift) { return ((w ^ xor_mask) >> shift) & (DIGITS - 1u); }

inline uint32_t passes_of(uint32_t nkeys, const uint32_t *flags)
{
    uint32_t p = 0;
    for (uint32_t k = 0; k < nkeys; ++k) p += digits_of(flags[k]);
    return p;
}

// pass p of passes_of(nkeys, flags): the last key's lowest digit first
inline Pass pass_of(uint32_t nkeys, const uint32_t *flags, uint32_t p)
{
    uint32_t k = nkeys - 1;
    while (p >= digits_of(flags[k])) { p -= digits_of(flags[k]); --k; }
    const bool wide = (flags[k] & WIDE) != 0;
    Pass s;
    s.key = k; s.stride = wide ? 2u : 1u; s.word = p >> 2; s.shift = (p & 3u) * DIGIT_BITS;
    s.xor_mask = xor_of(flags[k], !wide || s.word == 1u);
    return s;
}

// ---- the device road's ranges -------------------------------------------------------------------------------------------------------------
struct Layout {
    u64 n;
    u64 range_rows;         // a multiple of CHUNK_ROWS (0 when n == 0)
    uint32_t ranges;
    HJ_ORDER_HD u64 begin(uint32_t g) const
    {
        if (range_rows == 0 || g > n / range_rows) return n;
        return (u64)g * range_rows;
    }
    HJ_ORDER_HD u64 end(uint32_t g) const
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

// ---- the workspace (the context's, sized from n alone) --------------------------------------------------------------------------------------
// the blocking form's count word first; on the device road then the compaction's range counts, the digit totals of every pass, the (digit,
// range) counts and bases of the pass under way, and the two permutation buffers: 8 bytes per row behind WORKSPACE_HEAD
constexpr u64 COUNT_WORD_BYTES = 16;
constexpr u64 COMPACT_COUNTS_AT = COUNT_WORD_BYTES;
constexpr u64 COMPACT_COUNTS_BYTES = 2048 * sizeof(u64);                                   // hj_compact::MAX_RANGES
constexpr u64 TOTALS_AT = COMPACT_COUNTS_AT + COMPACT_COUNTS_BYTES;
constexpr u64 TOTALS_BYTES = (u64)MAX_PASSES * DIGITS * sizeof(uint32_t);
constexpr u64 COUNTS_AT = TOTALS_AT + TOTALS_BYTES;
constexpr u64 COUNTS_BYTES = (u64)DIGITS * MAX_RANGES * sizeof(uint32_t);
constexpr u64 BASES_AT = COUNTS_AT + COUNTS_BYTES;
constexpr u64 WORKSPACE_HEAD = BASES_AT + COUNTS_BYTES;
static_assert(WORKSPACE_HEAD == 2146320 && WORKSPACE_HEAD % 16 == 0, "include/hjgpu.h states the size");
inline u64 perm_bytes(u64 n) { return (n + 3) / 4 * 16; }                                  // whole 16-byte vectors
inline u64 workspace_bytes(u64 n) { return lds_road(n) ? COUNT_WORD_BYTES : WORKSPACE_HEAD + 2 * perm_bytes(n); }
}  // namespace hj_order
