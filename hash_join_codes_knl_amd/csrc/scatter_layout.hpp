// scatter_layout.hpp - the LDS of one K6 workgroup (partition_kernels.hip scatter_kernel, DESIGN.md section 3 "K6: one LDS layout, one
// dispatcher").  Plain arithmetic, no HIP: the kernel carves its dynamic LDS from layout() and from nothing else, and the host takes the
// same function's byte count to choose a geometry (hj_scatter_config), to refuse a launch and to size the persistent grid.
// tests/test_scatter_layout.py compiles it with g++ and walks every geometry the dispatcher lists.
//
// Writers and readers are the blocks of scatter_kernel's tile loop, by the words of their comments: hand-over (the previous tile's tails
// join the carry), rank, plan (local bases, one output run per partition, claims issued), sort, consume (the claims), stream-out (packed,
// tails, or columns), CLAIM's final flush.  This table is the only copy.
//   array  element  length           written by                          read by
//   delta  u64      Fpad             plan / consume / final flush        every stream-out
//   stage  u64      tile             sort                                every stream-out, hand-over
//   carry  u64      Fpad * 16        hand-over                           packed stream-out (the head of a run), final flush
//   tinfo  u64      Fpad             consume (pass 2, aligned claims)    tail stream-out
//   hist   u32      Fpad             rank (counts), plan (local bases)   plan, sort, packed and tail stream-out
//   meta   u32      Fpad             plan / consume / final flush        packed and tail stream-out
//   left   u32      Fpad             plan                                hand-over
//   wsum   u32      block / 64       plan (the scan's wave totals)       plan
//   ctl    u32      CTL_WORDS        see the CTL_ constants
//   heavy  u32      HJ_MAX_HEAVY     plan / consume (add_units)          packed stream-out
// carry and left exist in whole-line (carry) mode only, tinfo at pass 2 only; the kernel has no instance with both, so tinfo starts
// where carry would.  16 bytes stay free behind the heavy list.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr uint32_t HJ_LINE_TUPLES = 16;          // packed (8-byte) tuples per 128-byte line
constexpr uint32_t HJ_STREAM_UNIT = 256;         // output slots one 16-lane group streams out at a time
// Listed units per tile.  A run of e tuples that starts at slot `off` (< 16) of its line lists (off + e - 1) / HJ_STREAM_UNIT units, so a
// tile lists at most (tile + 15 F [line offsets] + 15 F [carried tuples, carry mode]) / HJ_STREAM_UNIT: 124 at 1024 x 4 without carry at
// F = 1024, the worst geometry that fits the LDS (89 for the largest carry tile, 16384 + 30 * 216).  The kernel does not check the
// list's bound: tests/cpp_scatter_layout.cpp walks every geometry hj_scatter_config can choose.
constexpr uint32_t HJ_MAX_HEAVY = 128;

namespace hj_scatter {
constexpr size_t LDS_LIMIT = 160 * 1024;         // gfx950: 160 KiB per CU, all of it usable by one workgroup

// the control words behind the scan's wave totals
enum : uint32_t {
    CTL_TILE_COUNT = 0,     // tuples of this tile (the scan's total; valid after the barrier that follows the scan)
    CTL_EXTRA_UNITS = 1,    // units listed in `heavy`: the further units of runs longer than one unit
    CTL_HOT = 2,            // this tile's hot partition (count << 10 | bin, 0 = none), named by the previous tile
    CTL_NEXT_HOT = 3,       // the same for the next tile: the largest partition of this one, if it held > 1/16 of the tile
    CTL_TICKETS = 4,        // [2] prefetched tickets
    CTL_WORDS = 6
};

struct Layout {
    int Fpad, tile;                                                        // F rounded up to 4; tuples per tile
    int delta, stage, carry, tinfo, hist, meta, left, wsum, ctl, heavy;    // byte offsets
    int bytes;
};

constexpr Layout layout(int block, int vpt, uint32_t F, bool carry, bool pass2)
{
    Layout l = {};
    l.Fpad = (int)((F + 3) & ~3u);
    l.tile = block * vpt * 4;
    l.delta = 0;
    l.stage = l.delta + l.Fpad * 8;
    l.carry = l.stage + l.tile * 8;
    l.tinfo = l.carry + (carry ? l.Fpad * (int)HJ_LINE_TUPLES * 8 : 0);
    l.hist = l.tinfo + (pass2 ? l.Fpad * 8 : 0);
    l.meta = l.hist + l.Fpad * 4;
    l.left = l.meta + l.Fpad * 4;
    l.wsum = l.left + (carry ? l.Fpad * 4 : 0);
    l.ctl = l.wsum + block / 64 * 4;
    l.heavy = l.ctl + (int)CTL_WORDS * 4;
    l.bytes = l.heavy + (int)HJ_MAX_HEAVY * 4 + 16;
    return l;
}

// does a pass-1 workgroup of this geometry hold its tile AND the carry buffers?  (hj_scatter_config: whole-line mode where it does)
// (block and vpt may come straight from an option: a tile beyond 5120 vectors or a fan-out beyond 2048 fits no LDS, and layout() counts in int)
constexpr bool carry_fits(int block, int vpt, uint32_t F)
{
    return block > 0 && vpt > 0 && (long long)block * vpt <= 5120 && F <= 2048 && (size_t)layout(block, vpt, F, true, false).bytes <= LDS_LIMIT;
}
}  // namespace hj_scatter
