// CPU test of hash_join_codes_knl_amd/csrc/scatter_layout.hpp (compiled and run by tests/test_scatter_layout.py): the LDS of a K6
// workgroup for every (block, vpt) pair hj_launch_scatter lists, F from 1 to 1024, whole-line carry on and off, pass 2 on and off.
// The total must be the byte formula the launcher used before the header existed (geometry, refusals and the grid follow from it); the
// arrays lie in the order the kernel steps through them, overlap nowhere and end inside the total; 8-byte arrays are 8-byte aligned,
// `stage` and the scan's wave totals 16-byte aligned (smem is; the scan reads the totals in 16-byte pieces); the control words follow the
// wave totals directly (the scan leaves the tile's count in scratch[NW]); tinfo shares carry's first byte only where there is no carry;
// the heavy list holds HJ_MAX_HEAVY words, which is at least what any tile of a geometry that hj_scatter_config can choose lists.
#include <stdio.h>
#include "scatter_layout.hpp"

static int fail(const char *what, int block, int vpt, uint32_t F, bool carry, bool pass2)
{
    fprintf(stderr, "FAIL: %s (block %d, vpt %d, F %u, carry %d, pass2 %d)\n", what, block, vpt, F, (int)carry, (int)pass2);
    return 1;
}

// the launcher's byte count before scatter_layout.hpp (partition_kernels.hip scatter_lds), literally
static size_t parent_scatter_lds(int block, int vpt, uint32_t F, bool carry, bool pass2)
{
    const size_t Fpad = (F + 3) & ~3u;
    return Fpad * 16 + (size_t)block * vpt * 4 * 8 + (carry ? Fpad * (HJ_LINE_TUPLES * 8 + 4) : 0) + (pass2 ? Fpad * 8 : 0) +
           (block / 64 + 6) * 4 + HJ_MAX_HEAVY * 4 + 16;
}

static int check(int block, int vpt, uint32_t F, bool carry, bool pass2)
{
    const hj_scatter::Layout l = hj_scatter::layout(block, vpt, F, carry, pass2);
    if ((size_t)l.bytes != parent_scatter_lds(block, vpt, F, carry, pass2)) return fail("total differs from the launcher's formula", block, vpt, F, carry, pass2);
    if (l.Fpad < (int)F || l.Fpad % 4 || l.Fpad >= (int)F + 4 || l.tile != block * vpt * 4) return fail("Fpad / tile", block, vpt, F, carry, pass2);
    const int NW = block / 64;
    struct Array { const char *name; int off, elem, len; };
    const Array arrays[] = {
        {"delta", l.delta, 8, l.Fpad},
        {"stage", l.stage, 8, l.tile},
        {"carry", l.carry, 8, carry ? l.Fpad * (int)HJ_LINE_TUPLES : 0},
        {"tinfo", l.tinfo, 8, pass2 ? l.Fpad : 0},
        {"hist", l.hist, 4, l.Fpad},
        {"meta", l.meta, 4, l.Fpad},
        {"left", l.left, 4, carry ? l.Fpad : 0},
        {"wsum", l.wsum, 4, NW},
        {"ctl", l.ctl, 4, (int)hj_scatter::CTL_WORDS},
        {"heavy", l.heavy, 4, (int)HJ_MAX_HEAVY},
    };
    int at = 0;
    for (const Array &x : arrays) {
        if (x.off < at) return fail("two arrays overlap (or are out of order)", block, vpt, F, carry, pass2);
        if (x.off % x.elem) return fail("an array is not aligned to its element", block, vpt, F, carry, pass2);
        at = x.off + x.elem * x.len;
    }
    if (at > l.bytes) return fail("the arrays end beyond the total", block, vpt, F, carry, pass2);
    if (l.delta != 0 || l.stage % 16 || l.wsum % 16 || NW % 4) return fail("stage / the wave totals are not 16-byte aligned", block, vpt, F, carry, pass2);
    if (l.ctl != l.wsum + NW * 4) return fail("the control words do not follow the wave totals", block, vpt, F, carry, pass2);
    // tinfo starts where carry does only when there is no carry; the kernel has no instance with both (carry needs pass 1)
    if (carry ? l.tinfo < l.carry + 8 * l.Fpad * (int)HJ_LINE_TUPLES : l.tinfo != l.carry) return fail("tinfo and carry", block, vpt, F, carry, pass2);
    if (l.heavy + 4 * (int)HJ_MAX_HEAVY > l.bytes) return fail("the heavy list ends beyond the total", block, vpt, F, carry, pass2);
    if (hj_scatter::CTL_TICKETS + 2 != hj_scatter::CTL_WORDS) return fail("the tickets are not the last control words", block, vpt, F, carry, pass2);
    return 0;
}

int main()
{
    // the pairs of hj_launch_scatter (partition_kernels.hip)
    const int pairs[][2] = {{1024, 4}, {1024, 3}, {1024, 2}, {512, 4}, {512, 3}, {512, 2}, {256, 4}, {256, 2}};
    size_t cases = 0;
    unsigned worst = 0, worst_F = 0;
    int worst_block = 0, worst_vpt = 0, worst_carry = 0;
    for (const auto &p : pairs)
        for (uint32_t F = 1; F <= 1024; ++F)
            for (int carry = 0; carry < 2; ++carry)
                for (int pass2 = 0; pass2 < 2; ++pass2) {
                    if (check(p[0], p[1], F, carry != 0, pass2 != 0)) return 1;
                    ++cases;
                    // hj_scatter_config chooses a listed pair (the planned 1024 x {4, 3, 2}, or any by option), with carry only at pass 1
                    // and only where carry_fits(); the launcher refuses what does not fit the LDS.  A run of e tuples that starts at slot
                    // off (< 16) of its line lists (off + e - 1) / UNIT further units; over a tile's runs that is at most
                    // (tile + 15 F line offsets + 15 F carried tuples) / UNIT.
                    if (carry && (pass2 || !hj_scatter::carry_fits(p[0], p[1], F))) continue;
                    if ((size_t)hj_scatter::layout(p[0], p[1], F, carry != 0, pass2 != 0).bytes > hj_scatter::LDS_LIMIT) continue;
                    const unsigned units = ((unsigned)p[0] * p[1] * 4 + (carry ? 30 : 15) * F) / HJ_STREAM_UNIT;
                    if (units > HJ_MAX_HEAVY) return fail("a tile can list more units than HJ_MAX_HEAVY", p[0], p[1], F, carry != 0, pass2 != 0);
                    if (units > worst) { worst = units; worst_F = F; worst_block = p[0]; worst_vpt = p[1]; worst_carry = carry; }
                }
    // the largest fan-out at which a 1024-thread carry tile of 4 / 3 / 2 vectors per thread fits: what hj_scatter_config's comment quotes
    unsigned fmax[5] = {0, 0, 0, 0, 0};
    for (int vpt = 2; vpt <= 4; ++vpt) {
        for (uint32_t F = 1; F <= 1024; ++F)
            if (hj_scatter::carry_fits(1024, vpt, F)) {
                if (fmax[vpt] != F - 1) return fail("carry_fits is not a prefix of the fan-outs", 1024, vpt, F, true, false);
                fmax[vpt] = F;
            }
    }
    if (fmax[4] != 216 || fmax[3] != 436 || fmax[2] != 660) {
        fprintf(stderr, "FAIL: largest carry fan-outs %u / %u / %u, the comments quote 216 / 436 / 660\n", fmax[4], fmax[3], fmax[2]);
        return 1;
    }
    // what the comments quote
    if (worst != 124 || worst_block != 1024 || worst_vpt != 4 || worst_carry != 0 || worst_F != 1024 || (16384 + 30 * 216) / HJ_STREAM_UNIT != 89) {
        fprintf(stderr, "FAIL: worst listed units %u at %d x %d carry %d F %u, the comments quote 124 at 1024 x 4 without carry at F 1024\n", worst,
                worst_block, worst_vpt, worst_carry, worst_F);
        return 1;
    }
    // options reach carry_fits with anything: no overflow, no fit
    if (hj_scatter::carry_fits(1 << 30, 1 << 30, 1) || hj_scatter::carry_fits(1024, 4, 0xFFFFFFFFu) || hj_scatter::carry_fits(0, 4, 8) ||
        hj_scatter::carry_fits(1024, -1, 8)) { fprintf(stderr, "FAIL: carry_fits on absurd geometries\n"); return 1; }
    printf("ok: %zu layouts, carry tiles up to F = %u / %u / %u, at most %u of %u listed units\n", cases, fmax[4], fmax[3], fmax[2], worst, HJ_MAX_HEAVY);
    return 0;
}
