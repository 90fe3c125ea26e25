"""CPU test (hipcc cross-compiles without a GPU): the kernels of hjgpu_group_by's wide road in gen_kernels.hip - wide_group_kernel<NKEYS, SEL>
for three and four key columns and wide_emit_kernel - exist for gfx950 in exactly the planned instances, use no scratch and spill no
register, and keep the store policy: the aggregation kernels have no global store at all (they reach memory through atomics alone), every
store of the emit is non-temporal.  The aggregation instances hold the table accesses DESIGN.md names - the 64-bit compare-and-swap in its
LDS and in its global form, the 64-bit adds and unsigned maxima of both memories - and every 16-byte global load of any instance is
non-temporal: nkeys key columns, a and b, for each of the wave trips of an iteration.  A workgroup's table fits the compute unit's LDS.  Plus
the two entry points in the library, in EXPORTS and on HjGpu, and the header's limit."""
import os
import re

import pytest

from device_compile import compile_device, split_kernels, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "gen_kernels.hip"
ENTRY_POINTS = ["hjgpu_group_by", "hjgpu_group_by_async"]
GROUPED = {"_Z17wide_group_kernelILi%dELb%dEEv8WideArgs" % (nkeys, sel): (nkeys, sel) for nkeys in (3, 4) for sel in (0, 1)}
EMIT = "_Z16wide_emit_kernel12WideEmitArgs"


def found_instances():
    """{mangled symbol: the whole body} of the wide_* kernels: up to the function's end label, not to the first s_endpgm"""
    text = compile_device(SOURCE)[0]
    out = {}
    for sym in split_kernels(text, "wide_"):
        start = text.index("\n%s:" % sym)
        out[sym] = text[start:text.index(".Lfunc_end", start)]
    return out


def instructions(body):
    return [line.split(";")[0].strip() for line in body.splitlines() if line.split(";")[0].strip()]


def count(ins, prefix):
    return sum(1 for i in ins if i.startswith(prefix))


def layout(name):
    text = open(os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc", "wide_group_layout.hpp")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


def test_every_planned_instance_exists():
    assert len(GROUPED) == 4
    assert set(found_instances()) == set(GROUPED) | {EMIT}, sorted(found_instances())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?wide_(group|emit)_kernel[<(]", k)}
    assert len(rows) == 5, sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad
    for k, v in rows.items():
        print(k, v)


def test_the_table_fits_the_lds():
    text = compile_device(SOURCE)[0]
    for name in GROUPED:
        start = text.index(".amdhsa_kernel %s" % name)
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", text[start:]).group(1))
        assert 2048 * 72 <= lds <= 160 * 1024, (name, lds)


def test_store_policy():
    found = found_instances()
    for k in GROUPED:
        assert not _stores(found[k]), (k, _stores(found[k]))                        # atomics only
    stores = _stores(found[EMIT])
    assert not {s: n for s, n in stores.items() if not s[1]}, stores
    assert stores[("dword", True)] >= 4 and stores[("dwordx2", True)] >= 5, stores     # four key columns; the count and four aggregates


@pytest.mark.parametrize("name", sorted(GROUPED))
def test_the_wide_road_reaches_its_tables_through_atomics(name):
    nkeys, sel = GROUPED[name]
    ins = instructions(found_instances()[name])
    for op in ("ds_cmpst_rtn_b64", "ds_add_u64", "ds_max_u64", "global_atomic_cmpswap_x2", "global_atomic_add_x2", "global_atomic_umax_x2", "global_atomic_or"):
        assert count(ins, op) >= 1, (name, op)
    # one compare-and-swap per key word in the walk over a workgroup's table; the walk over the merge table is there twice (the loop, the flush)
    assert count(ins, "ds_cmpst_rtn_b64") >= nkeys and count(ins, "global_atomic_cmpswap_x2") >= nkeys, name
    assert not count(ins, "flat_"), [i for i in ins if i.startswith("flat_")]
    # the columns: 16-byte non-temporal loads and no other 16-byte global load - nkeys key columns, a and b per wave trip; the mask: a
    # 4-byte non-temporal load
    wide = [i for i in ins if i.startswith("global_load_dwordx4")]
    assert len(wide) >= layout("BATCH") * (nkeys + 2) and all(" nt" in i for i in wide), wide
    words = [i for i in ins if re.match(r"global_load_dword\s", i) and " nt" in i]
    assert (len(words) >= 1) == bool(sel), words


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]
    text = open(os.path.join(ROOT, "include", "hjgpu.h")).read()
    assert int(re.search(r"#define HJGPU_GROUP_BY_MAX_KEYS\s+(\d+)u", text).group(1)) == layout("MAX_KEYS") == 4
    assert int(re.search(r"#define HJGPU_GROUP_MAX_KEYS\s+(\d+)u", text).group(1)) == 2
