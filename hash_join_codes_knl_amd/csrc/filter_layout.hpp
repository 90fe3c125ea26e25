// filter_layout.hpp - the predicate arithmetic and the geometry of hjgpu_filter_selected (gen_kernels.hip filter_kernel, DESIGN.md section 5
// "Filter").  Plain host / device arithmetic, no HIP: the host normalises a predicate once per call, the kernel tests a value with one
// subtract and one compare, and tests/test_filter_layout.py compiles both functions with g++ and compares them with the definition.
//
// A predicate {lo, hi, flags} holds on x when lo <= x <= hi, both ends inclusive, in uint32 order or - HJGPU_PRED_SIGNED - in int32
// order; HJGPU_PRED_NOT inverts it.  lo > hi in the predicate's order is the empty range: nothing passes, or everything under NOT.
// XOR with 0x80000000 maps int32 order to uint32 order, so a signed predicate is the unsigned one on the biased values; an inclusive
// range [lo', hi'] of uint32 is (x' - lo') <= hi' - lo' in arithmetic modulo 2^32 (x' below lo' wraps to a value above every span); the
// empty range has no such form and becomes the full range [0, 0xFFFFFFFF] with the inversion flipped.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HJ_FILTER_FN __host__ __device__ inline
#else
#define HJ_FILTER_FN inline
#endif

namespace hj_filter {
typedef unsigned long long u64;

constexpr uint32_t MAX_PREDS = 4;                       // HJGPU_FILTER_MAX_PREDS
constexpr uint32_t PRED_NOT = 1u, PRED_SIGNED = 2u;     // HJGPU_PRED_NOT, HJGPU_PRED_SIGNED

constexpr uint32_t BLOCK = 256;                         // lanes per workgroup
constexpr uint32_t BATCH = 2;                           // wave trips (of hj_lookup.hpp: 256 rows) per wave and loop iteration
constexpr uint32_t RESIDENT = 8;                        // workgroups of BLOCK lanes a CU holds at once

// the persistent grid's workgroups on a device of `cus` compute units (fewer when the rows have fewer wave trips: hj_launch_filter)
inline uint32_t grid_of(int cus) { return (uint32_t)(cus < 1 ? 1 : cus) * RESIDENT; }
// hjgpu_get_counter "filter_step_rows": the rows that grid covers in one loop iteration
inline u64 step_rows(int cus) { return (u64)grid_of(cus) * BLOCK * 4 * BATCH; }

// a predicate as the kernel takes it: x passes when (((x ^ bias) - lo) <= span) != invert
struct Norm {
    uint32_t bias;          // 0x80000000 under HJGPU_PRED_SIGNED, else 0: applied to lo, hi and, on the device, to x
    uint32_t lo;            // the biased lower end
    uint32_t span;          // biased hi - biased lo
    uint32_t invert;        // 0 or 1
};

HJ_FILTER_FN Norm normalise(uint32_t lo, uint32_t hi, uint32_t flags)
{
    Norm p;
    p.bias = (flags & PRED_SIGNED) ? 0x80000000u : 0u;
    p.invert = (flags & PRED_NOT) ? 1u : 0u;
    const uint32_t l = lo ^ p.bias, h = hi ^ p.bias;
    if (l > h) { p.lo = 0u; p.span = 0xFFFFFFFFu; p.invert ^= 1u; }     // the empty range: NOT the full range
    else { p.lo = l; p.span = h - l; }
    return p;
}

HJ_FILTER_FN bool passes(const Norm &p, uint32_t x)
{
    return ((uint32_t)((x ^ p.bias) - p.lo) <= p.span) != (p.invert != 0u);
}
}  // namespace hj_filter
