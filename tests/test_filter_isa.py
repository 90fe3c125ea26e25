"""CPU test (hipcc cross-compiles without a GPU): the kernel of hjgpu_filter_selected in gen_kernels.hip - filter_kernel<NPREDS, SEL> - exists
for gfx950 in exactly the eight planned instances (1 to 4 predicates, each with and without a mask), uses no scratch and no spills, stores
every global word non-temporally and through global_ instructions alone, loads its columns in 16-byte non-temporal loads - one load site
per trip and column - and its mask, where it has one, in 4-byte non-temporal loads, and reaches the count word through one 64-bit global
atomic add.  Plus the two entry points in the library, in EXPORTS and on HjGpu, and hjgpu_predicate's layout against api.Predicate."""
import ctypes as C
import os
import re
import subprocess

import pytest

from device_compile import compile_device, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "gen_kernels.hip"
ENTRY_POINTS = ["hjgpu_filter_selected", "hjgpu_filter_selected_async"]
INSTANCES = {"_Z13filter_kernelILi%dELb%dEEv10FilterArgs" % (npreds, sel): (npreds, sel) for npreds in (1, 2, 3, 4) for sel in (0, 1)}
BATCH = 2                               # filter_layout.hpp: wave trips per loop iteration


def found_instances():
    text, _ = compile_device(SOURCE)
    out = {}
    for m in re.finditer(r"^(_Z\d+filter_\w+):\s*; @", text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


def instructions(body):
    return [line.split(";")[0].strip() for line in body.splitlines() if line.split(";")[0].strip()]


def test_every_planned_instance_exists():
    assert len(INSTANCES) == 8
    assert set(found_instances()) == set(INSTANCES), sorted(found_instances())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?filter_kernel<", k)}
    assert len(rows) == 8, sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_loads_stores_and_the_atomic(name):
    npreds, sel = INSTANCES[name]
    body = found_instances()[name]
    ins = instructions(body)
    # the bitmap word: a 4-byte non-temporal store per trip, and no other store
    stores = _stores(body)
    assert not {s: n for s, n in stores.items() if not s[1]}, stores
    assert set(stores) == {("dword", True)} and stores[("dword", True)] >= 1, stores
    assert not [i for i in ins if i.startswith("flat_")], [i for i in ins if i.startswith("flat_")]
    # the columns: 16-byte non-temporal loads - every trip of every column has a load site of its own - and no other 16-byte global load
    wide = [i for i in ins if i.startswith("global_load_dwordx4")]
    assert len(wide) >= BATCH * npreds and all(" nt" in i for i in wide), wide
    # the mask: 4-byte non-temporal loads exactly where there is one; without it no global load but the columns'
    words = [i for i in ins if re.match(r"global_load_dword\s", i) and " nt" in i]
    assert (len(words) >= 1) == bool(sel), words
    other = [i for i in ins if i.startswith("global_load_") and i not in wide and i not in words]
    assert not other, other
    # the count: one 64-bit atomic add, nothing else atomic
    atomics = [i for i in ins if i.startswith("global_atomic_")]
    assert len(atomics) == 1 and atomics[0].startswith("global_atomic_add_x2"), atomics


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]
    assert H.PRED_NOT == H.api.PRED_NOT == 1 and H.PRED_SIGNED == H.api.PRED_SIGNED == 2 and H.Predicate is H.api.Predicate


def test_predicate_layout_matches_the_header(tmp_path):
    """api.Predicate has the size and field offsets gcc gives include/hjgpu.h's hjgpu_predicate, and the constants are the header's"""
    from hash_join_codes_knl_amd import api
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hjgpu.h"', 'int main(void){',
             'printf("%zu", sizeof(hjgpu_predicate));']
    for fname, _ in api.Predicate._fields_:
        lines.append('printf(" %%zu", offsetof(hjgpu_predicate, %s));' % fname)
    lines.append('printf("\\n%u %u %u\\n", HJGPU_FILTER_MAX_PREDS, HJGPU_PRED_NOT, HJGPU_PRED_SIGNED);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    got = [int(x) for x in out[0].split()]
    want = [C.sizeof(api.Predicate)] + [getattr(api.Predicate, f).offset for f, _ in api.Predicate._fields_]
    assert got == want == [16, 0, 4, 8, 12], (got, want)
    assert [int(x) for x in out[1].split()] == [api.FILTER_MAX_PREDS, api.PRED_NOT, api.PRED_SIGNED]
    p = api.Predicate.of((-5, 7, api.PRED_SIGNED))
    assert (p.lo, p.hi, p.flags, p.reserved) == (0xFFFFFFFB, 7, 2, 0) and api.Predicate.of(p) is p
    q = api.Predicate.of((1, 3))
    assert (q.lo, q.hi, q.flags, q.reserved) == (1, 3, 0, 0)
