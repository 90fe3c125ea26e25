"""CPU test (hipcc cross-compiles without a GPU): the kernel of hjgpu_gather_selected in gen_kernels.hip - gather_kernel<NCOLS, SEL> - exists
for gfx950 in exactly the eight planned instances (1 to 4 columns, each with and without a mask), uses no scratch and no spills, stores
every global word non-temporally and through global_ instructions alone - 16-byte stores for the columns, 4-byte stores for the last,
partial vector and the bitmap word -, reads its index in 16-byte non-temporal loads and nothing else in 16-byte loads, its mask, where it
has one, in 4-byte non-temporal loads, the source elements in ordinary 4-byte loads - one load site per row, trip and column -, and reaches
the count words through 64-bit global atomic adds alone.  Plus the two entry points in the library, in EXPORTS and on HjGpu, and the
header's two new constants against api's."""
import os
import re
import subprocess

import pytest

from device_compile import compile_device, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "gen_kernels.hip"
ENTRY_POINTS = ["hjgpu_gather_selected", "hjgpu_gather_selected_async"]
INSTANCES = {"_Z13gather_kernelILi%dELb%dEEv10GatherArgs" % (ncols, sel): (ncols, sel) for ncols in (1, 2, 3, 4) for sel in (0, 1)}
BATCH = 2                               # gather_layout.hpp: wave trips per loop iteration


def found_instances():
    text, _ = compile_device(SOURCE)
    out = {}
    for m in re.finditer(r"^(_Z\d+gather_\w+):\s*; @", text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


def instructions(body):
    return [line.split(";")[0].strip() for line in body.splitlines() if line.split(";")[0].strip()]


def test_every_planned_instance_exists():
    assert len(INSTANCES) == 8
    assert set(found_instances()) == set(INSTANCES), sorted(found_instances())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?gather_kernel<", k)}
    assert len(rows) == 8, sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad


def test_the_whole_grid_is_resident():
    """gather_layout.hpp's RESIDENT workgroups of 4 waves per CU are RESIDENT waves per SIMD: every instance reaches that occupancy, so no
    workgroup of the persistent grid queues behind another"""
    header = open(os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc", "gather_layout.hpp")).read()
    resident = int(re.search(r"constexpr uint32_t RESIDENT = (\d+);", header).group(1))
    assert int(re.search(r"constexpr uint32_t BATCH = (\d+);", header).group(1)) == BATCH
    _, res = compile_device(SOURCE)
    low = {k: v["occ"] for k, v in res.items() if re.match(r"(void )?gather_kernel<", k) and v["occ"] < resident}
    assert 1 <= resident <= 8 and not low, (resident, low)


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_loads_stores_and_the_atomics(name):
    ncols, sel = INSTANCES[name]
    body = found_instances()[name]
    ins = instructions(body)
    # stores: every one non-temporal and global_; 16 bytes per trip and column, 4 bytes for the partial vector and the bitmap word
    stores = _stores(body)
    assert not {s: n for s, n in stores.items() if not s[1]}, stores
    assert set(stores) == {("dword", True), ("dwordx4", True)}, stores
    assert stores[("dwordx4", True)] >= BATCH * ncols and stores[("dword", True)] >= 1, stores
    assert not [i for i in ins if i.startswith("flat_")], [i for i in ins if i.startswith("flat_")]
    # the index: 16-byte non-temporal loads, one site per trip at least, and no other 16-byte global load
    wide = [i for i in ins if i.startswith("global_load_dwordx4")]
    assert len(wide) >= BATCH and all(" nt" in i for i in wide), wide
    # the mask: 4-byte non-temporal loads exactly where there is one
    words = [i for i in ins if re.match(r"global_load_dword\s", i) and " nt" in i]
    assert (len(words) >= 1) == bool(sel), words
    # the source elements: ordinary (cached) 4-byte loads, a site per row, trip and column; and no global load of any other kind
    elems = [i for i in ins if re.match(r"global_load_dword\s", i) and " nt" not in i]
    assert len(elems) >= 4 * BATCH * ncols and not [i for i in elems if " sc0" in i or " sc1" in i], elems
    other = [i for i in ins if i.startswith("global_load_") and i not in wide and i not in words and i not in elems]
    assert not other, other
    # the counts: 64-bit atomic adds, nothing else atomic
    atomics = [i for i in ins if "atomic" in i]
    assert 1 <= len(atomics) <= 2 and all(i.startswith("global_atomic_add_x2") for i in atomics), atomics


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]
    assert lib.hjgpu_status_string(H.api.ERANGE) not in (b"", b"unknown status")


def test_constants_match_the_header(tmp_path):
    """HJGPU_GATHER_MAX_COLS and HJGPU_ERANGE as gcc reads them from include/hjgpu.h equal api's"""
    from hash_join_codes_knl_amd import api
    src = tmp_path / "constants.c"
    src.write_text('#include <stdio.h>\n#include "hjgpu.h"\nint main(void){printf("%u %d\\n", HJGPU_GATHER_MAX_COLS, HJGPU_ERANGE);return 0;}\n')
    exe = tmp_path / "constants"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [api.GATHER_MAX_COLS, api.ERANGE] == [4, 9], got
