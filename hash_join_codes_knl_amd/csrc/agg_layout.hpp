// agg_layout.hpp - the aggregate functions and the geometry of hjgpu_group_agg (gen_kernels.hip agg_group_kernel / agg_scalar_kernel /
// agg_emit_kernel, DESIGN.md section 5 "Aggregate functions").  Plain host / device arithmetic, no HIP: the kernels and the launchers share
// it with tests/test_group_agg_checks.py, which compiles it with g++ and compares the transform with the definition on the CPU.
//
// The tables are group_layout.hpp's, zero-initialised, and a slot's four 64-bit words hold one aggregate each.  What a row contributes to
// its word (term) and how words are combined (is_extreme: unsigned maximum, else addition modulo 2^64):
//   SUM      the value, zero-extended, or sign-extended under SIGNED;
//   SUM_MUL  the exact 64-bit product of the two values, uint32 x uint32 or - SIGNED - int32 x int32;
//   MAX      w = a (SIGNED: a ^ 0x80000000, which maps int32 order to uint32 order), zero-extended;
//   MIN      the 32-bit complement of MAX's w, zero-extended: the smallest value has the largest complement.
// 0 is the neutral word of both combines, and a group has at least one row, so a word that was never combined is never emitted: no slot
// needs an initial value other than 0.  result() undoes the transform for the emit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HJ_AGG_FN __host__ __device__ inline
#else
#define HJ_AGG_FN inline
#endif

namespace hj_agg {
typedef unsigned long long u64;

constexpr uint32_t MAX_AGGS = 4;                        // HJGPU_AGG_MAX_AGGS (a slot's four words: hj_group::MAX_VALS)
constexpr uint32_t SUM = 0, SUM_MUL = 1, MIN = 2, MAX = 3;     // HJGPU_AGG_*
constexpr uint32_t SIGNED = 1;                          // HJGPU_AGG_SIGNED

// the grouped road: group_sum_kernel's geometry - one workgroup of hj_group::BLOCK lanes per compute unit, GROUP_BATCH wave trips (of
// hj_lookup.hpp: 256 rows) per wave and loop iteration
constexpr uint32_t GROUP_BLOCK = 1024;                  // hj_group::BLOCK
constexpr uint32_t GROUP_BATCH = 2;
// hjgpu_get_counter "agg_step_rows": the rows the grouped road's whole grid covers in one loop iteration
inline u64 group_step_rows(int cus) { return (u64)(cus < 1 ? 1 : cus) * GROUP_BLOCK * 4 * GROUP_BATCH; }

// the scalar road (nkeys == 0): no table, so a compute unit holds several small workgroups - filter_layout.hpp's geometry.  The whole
// persistent grid is resident at once only while the kernel is compiled to SCALAR_RESIDENT waves per SIMD (tests/test_group_agg_isa.py)
constexpr uint32_t SCALAR_BLOCK = 256;                  // lanes per workgroup
constexpr uint32_t SCALAR_BATCH = 2;                    // wave trips per wave and loop iteration
constexpr uint32_t SCALAR_RESIDENT = 8;                 // workgroups of SCALAR_BLOCK lanes a CU holds at once
inline uint32_t scalar_grid_of(int cus) { return (uint32_t)(cus < 1 ? 1 : cus) * SCALAR_RESIDENT; }
// hjgpu_get_counter "agg_scalar_step_rows": the rows that grid covers in one loop iteration
inline u64 scalar_step_rows(int cus) { return (u64)scalar_grid_of(cus) * SCALAR_BLOCK * 4 * SCALAR_BATCH; }

HJ_AGG_FN bool is_extreme(uint32_t fn) { return fn >= MIN; }

// MIN / MAX: the word XORed onto a value on its way into the tables and, being its own inverse, on its way out
HJ_AGG_FN uint32_t extreme_xor(uint32_t fn, uint32_t flags)
{
    return ((flags & SIGNED) ? 0x80000000u : 0u) ^ (fn == MIN ? 0xFFFFFFFFu : 0u);
}

// The three bodies a kernel has for an aggregate, chosen once per aggregate and loop iteration (fn is uniform), and what is left of fn and
// flags inside them: two uniform words, so that a row's term is straight-line code without a branch.
constexpr int KIND_VALUE = 0, KIND_PRODUCT = 1, KIND_EXTREME = 2;      // SUM; SUM_MUL; MIN and MAX
HJ_AGG_FN int kind_of(uint32_t fn) { return fn == SUM ? KIND_VALUE : fn == SUM_MUL ? KIND_PRODUCT : KIND_EXTREME; }
struct Norm {
    uint32_t xorw;          // KIND_EXTREME: extreme_xor(fn, flags)
    uint32_t smask;         // 0xFFFFFFFF under SIGNED, else 0: ANDed onto a value's sign word
};
HJ_AGG_FN Norm normalise(uint32_t fn, uint32_t flags)
{
    Norm p;
    p.xorw = extreme_xor(fn, flags);
    p.smask = (flags & SIGNED) ? 0xFFFFFFFFu : 0u;
    return p;
}

// what one row contributes: x = a's value, y = b's (KIND_PRODUCT only).  KIND_VALUE: x under its sign word (0 when unsigned).
// KIND_PRODUCT: the unsigned product, and for int32 factors the correction that two's complement asks for: x_s * y_s = x * y -
// 2^32 * ((x < 0 ? y : 0) + (y < 0 ? x : 0)) modulo 2^64.
template <int KIND>
HJ_AGG_FN u64 term(const Norm &p, uint32_t x, uint32_t y)
{
    const uint32_t sx = (uint32_t)(0u - (x >> 31)) & p.smask, sy = (uint32_t)(0u - (y >> 31)) & p.smask;
    if (KIND == KIND_VALUE) return (u64)x | ((u64)sx << 32);
    if (KIND == KIND_PRODUCT) return (u64)x * (u64)y - ((u64)(uint32_t)((sx & y) + (sy & x)) << 32);
    return (u64)(x ^ p.xorw);
}

template <int KIND>
HJ_AGG_FN u64 combine(u64 acc, u64 t) { return KIND == KIND_EXTREME ? (t > acc ? t : acc) : acc + t; }

// the same by the function's number (the closing reductions; the CPU test)
HJ_AGG_FN u64 term(uint32_t fn, uint32_t flags, uint32_t x, uint32_t y)
{
    const Norm p = normalise(fn, flags);
    return fn == SUM ? term<KIND_VALUE>(p, x, y) : fn == SUM_MUL ? term<KIND_PRODUCT>(p, x, y) : term<KIND_EXTREME>(p, x, y);
}
HJ_AGG_FN u64 combine(uint32_t fn, u64 acc, u64 t) { return is_extreme(fn) ? combine<KIND_EXTREME>(acc, t) : combine<KIND_VALUE>(acc, t); }

// a table word as the caller reads it: the sums as they are; the extremes back in the column's own values, sign-extended under SIGNED
HJ_AGG_FN u64 result(uint32_t fn, uint32_t flags, u64 word)
{
    if (!is_extreme(fn)) return word;
    const uint32_t x = (uint32_t)word ^ extreme_xor(fn, flags);
    return (flags & SIGNED) ? (u64)(long long)(int32_t)x : (u64)x;
}
}  // namespace hj_agg
