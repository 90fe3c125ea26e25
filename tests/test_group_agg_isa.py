"""CPU test (hipcc cross-compiles without a GPU): the kernels of hjgpu_group_agg in gen_kernels.hip - agg_group_kernel<NKEYS, SEL>,
agg_scalar_kernel<SEL> and agg_emit_kernel - exist for gfx950 in exactly the planned instances, use no scratch and spill no register, and
keep the store policy: the aggregation kernels have no global store at all (they reach memory through atomics alone), every store of the
emit is non-temporal.  The grouped instances hold the table accesses DESIGN.md names - the 64-bit LDS compare-and-swap, add and unsigned
maximum, the 64-bit global add and unsigned maximum - and every 16-byte global load of any instance is non-temporal.  The scalar kernel is
compiled to at least the waves per SIMD that its persistent grid takes for granted.  Plus the two entry points in the library, in EXPORTS
and on HjGpu, and hjgpu_aggregate's layout under gcc against the ctypes mirror."""
import ctypes
import os
import re
import subprocess

import pytest

from device_compile import compile_device, split_kernels, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "gen_kernels.hip"
ENTRY_POINTS = ["hjgpu_group_agg", "hjgpu_group_agg_async"]
GROUPED = {"_Z16agg_group_kernelILi%dELb%dEEv7AggArgs" % (nkeys, sel): (nkeys, sel) for nkeys in (1, 2) for sel in (0, 1)}
SCALAR = {"_Z17agg_scalar_kernelILb%dEEv7AggArgs" % sel: sel for sel in (0, 1)}
EMIT = "_Z15agg_emit_kernel11AggEmitArgs"


def found_instances():
    """{mangled symbol: the whole body} of the agg_* kernels: up to the function's end label, not to the first s_endpgm - the compiler
    lays blocks out behind an early exit (the scalar kernel's closing atomics are such blocks)"""
    text = compile_device(SOURCE)[0]
    out = {}
    for sym in split_kernels(text, "agg_"):
        start = text.index("\n%s:" % sym)
        out[sym] = text[start:text.index(".Lfunc_end", start)]
    return out


def instructions(body):
    return [line.split(";")[0].strip() for line in body.splitlines() if line.split(";")[0].strip()]


def count(ins, prefix):
    return sum(1 for i in ins if i.startswith(prefix))


def test_every_planned_instance_exists():
    assert len(GROUPED) == 4 and len(SCALAR) == 2
    assert set(found_instances()) == set(GROUPED) | set(SCALAR) | {EMIT}, sorted(found_instances())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?agg_(group|scalar|emit)_kernel[<(]", k)}
    assert len(rows) == 7, sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad
    for k, v in rows.items():
        print(k, v)


def test_the_scalar_grid_is_resident_at_once():
    """agg_layout.hpp's SCALAR_RESIDENT workgroups of four waves per compute unit are that many waves per SIMD"""
    text = open(os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc", "agg_layout.hpp")).read()
    resident = int(re.search(r"SCALAR_RESIDENT = (\d+);", text).group(1))
    assert int(re.search(r"SCALAR_BLOCK = (\d+);", text).group(1)) == 256
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?agg_scalar_kernel<", k)}
    assert len(rows) == 2 and all(v["occ"] >= resident for v in rows.values()), (resident, rows)


def test_store_policy():
    found = found_instances()
    for k in list(GROUPED) + list(SCALAR):
        assert not _stores(found[k]), (k, _stores(found[k]))                        # atomics only
    stores = _stores(found[EMIT])
    assert not {s: n for s, n in stores.items() if not s[1]}, stores
    assert stores[("dword", True)] >= 2 and stores[("dwordx2", True)] >= 5, stores     # two key columns; the count and four aggregates


@pytest.mark.parametrize("name", sorted(GROUPED))
def test_the_grouped_road_reaches_its_tables_through_atomics(name):
    nkeys, sel = GROUPED[name]
    ins = instructions(found_instances()[name])
    for op in ("ds_cmpst_rtn_b64", "ds_add_u64", "ds_max_u64", "global_atomic_cmpswap_x2", "global_atomic_add_x2", "global_atomic_umax_x2", "global_atomic_or"):
        assert count(ins, op) >= 1, (name, op)
    assert not count(ins, "flat_"), [i for i in ins if i.startswith("flat_")]
    # the columns: 16-byte non-temporal loads and no other 16-byte global load (the keys, a and b); the mask: a 4-byte non-temporal load
    wide = [i for i in ins if i.startswith("global_load_dwordx4")]
    assert len(wide) >= 2 * (nkeys + 2) and all(" nt" in i for i in wide), wide
    words = [i for i in ins if re.match(r"global_load_dword\s", i) and " nt" in i]
    assert (len(words) >= 1) == bool(sel), words


@pytest.mark.parametrize("name", sorted(SCALAR))
def test_the_scalar_road_loads_non_temporally_and_ends_in_atomics(name):
    sel = SCALAR[name]
    ins = instructions(found_instances()[name])
    assert count(ins, "global_atomic_add_x2") >= 1 and count(ins, "global_atomic_umax_x2") >= 1, name
    assert not count(ins, "global_atomic_cmpswap") and not count(ins, "flat_"), name
    wide = [i for i in ins if i.startswith("global_load_dwordx4")]
    assert len(wide) >= 2 and all(" nt" in i for i in wide), wide
    words = [i for i in ins if re.match(r"global_load_dword\s", i)]
    assert all(" nt" in i for i in words) and (len(words) >= 1) == bool(sel), words


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]
    for name, value in (("AGG_SUM", 0), ("AGG_SUM_MUL", 1), ("AGG_MIN", 2), ("AGG_MAX", 3), ("AGG_SIGNED", 1)):
        assert getattr(H, name) == value, name


def test_the_aggregate_struct_agrees_with_gcc(tmp_path):
    from hash_join_codes_knl_amd.api import Aggregate
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hjgpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(hjgpu_aggregate), offsetof(hjgpu_aggregate, fn), '
                   'offsetof(hjgpu_aggregate, flags), offsetof(hjgpu_aggregate, d_a), offsetof(hjgpu_aggregate, d_b)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(Aggregate), Aggregate.fn.offset, Aggregate.flags.offset, Aggregate.d_a.offset, Aggregate.d_b.offset], got
    # the constants of the header
    text = open(os.path.join(ROOT, "include", "hjgpu.h")).read()
    import hash_join_codes_knl_amd as H
    for name in ("AGG_SUM", "AGG_SUM_MUL", "AGG_MIN", "AGG_MAX", "AGG_SIGNED"):
        assert int(re.search(r"#define HJGPU_%s\s+(\d+)u" % name, text).group(1)) == getattr(H, name), name
