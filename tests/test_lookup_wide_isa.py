"""CPU test (hipcc cross-compiles without a GPU): the two kernels of hjgpu_lookup_wide in gen_kernels.hip - hj_wlk::wide_lookup_build_kernel<NKEYS>
and hj_wlk::wide_lookup_kernel<NKEYS, SEL, VALS, BITS> - exist for gfx950 in exactly the planned instances (3 builds, 3 x 2 x 2 x 2 = 24
look-ups), use no scratch and no spills and store every global word non-temporally; a look-up instance that writes values holds a 16-byte
store, one that writes bits a 4-byte store, the aggregate-only instances hold no global store at all; the build claims its slots by 64-bit
compare-and-swap and stores nothing but key words, 8 bytes at a time.  Plus the two entry points in the library, in EXPORTS and on HjGpu,
and the header's two constants against api's.  Stores and resources only."""
import os
import re
import subprocess

import pytest

from device_compile import compile_device, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "gen_kernels.hip"
ENTRY_POINTS = ["hjgpu_lookup_wide", "hjgpu_lookup_wide_async"]
BUILD = {"_ZN6hj_wlk24wide_lookup_build_kernelILi%dEEEv19WideLookupBuildArgs" % nkeys: nkeys for nkeys in (2, 3, 4)}
LOOKUP = {"_ZN6hj_wlk18wide_lookup_kernelILi%dELb%dELb%dELb%dEEEv14WideLookupArgs" % (nkeys, sel, vals, bits): (nkeys, sel, vals, bits)
          for nkeys in (2, 3, 4) for sel in (0, 1) for vals in (0, 1) for bits in (0, 1)}


def found_instances():
    """{mangled symbol: the whole body} of the hj_wlk:: kernels: up to the function's end label, not to the first s_endpgm"""
    text, _ = compile_device(SOURCE)
    out = {}
    for m in re.finditer(r"^(_ZN6hj_wlk\w+):\s*; @", text, re.M):
        out[m.group(1)] = text[m.end():text.index(".Lfunc_end", m.end())]
    return out


def instructions(body):
    return [line.split(";")[0].strip() for line in body.splitlines() if line.split(";")[0].strip()]


def test_every_planned_instance_exists():
    assert len(BUILD) == 3 and len(LOOKUP) == 24
    assert set(found_instances()) == set(BUILD) | set(LOOKUP), sorted(found_instances())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?hj_wlk::wide_lookup_(build_)?kernel<", k)}
    assert len(rows) == 27, sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad


def test_the_whole_grid_is_resident():
    """wide_lookup_layout.hpp's RESIDENT workgroups of 4 waves per CU are RESIDENT waves per SIMD: every look-up instance reaches that
    occupancy, so no workgroup of the persistent grid queues behind another"""
    header = open(os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc", "wide_lookup_layout.hpp")).read()
    resident = int(re.search(r"constexpr uint32_t RESIDENT = (\d+);", header).group(1))
    assert int(re.search(r"constexpr uint32_t BLOCK = (\d+);", header).group(1)) == 256
    _, res = compile_device(SOURCE)
    low = {k: v["occ"] for k, v in res.items() if re.match(r"(void )?hj_wlk::wide_lookup_kernel<", k) and v["occ"] < resident}
    assert 1 <= resident <= 8 and not low, (resident, low)


def test_every_store_non_temporal():
    found = found_instances()
    assert len(found) == 27
    for k, body in found.items():
        plain = {s: n for s, n in _stores(body).items() if not s[1]}
        assert not plain, (k, plain)
        assert not [i for i in instructions(body) if i.startswith("flat_")], k


@pytest.mark.parametrize("name", sorted(LOOKUP))
def test_look_up_stores_follow_the_template_arguments(name):
    _, _, vals, bits = LOOKUP[name]
    stores = _stores(found_instances()[name])
    if vals:
        assert stores[("dwordx4", True)] >= 1, stores                   # a lane's four answers in one store
    if bits:
        assert stores[("dword", True)] >= 1, stores                     # a word of the bitmap
    if not vals:
        assert not [s for s in stores if s[0] == "dwordx4"], stores
    if not vals and not bits:
        assert not stores, stores


@pytest.mark.parametrize("name", sorted(BUILD))
def test_the_build_claims_by_compare_and_swap_and_stores_key_words_only(name):
    ins = instructions(found_instances()[name])
    atomics = [i for i in ins if "atomic" in i]
    assert atomics and all(i.startswith("global_atomic_cmpswap_x2") for i in atomics), atomics
    stores = _stores(found_instances()[name])
    # two key words at a time; the compiler may merge a slot's two neighbouring pairs into one 16-byte store
    assert stores and set(stores) <= {("dwordx2", True), ("dwordx4", True)}, stores
    wide = [i for i in ins if i.startswith("global_load_dwordx4")]
    assert len(wide) >= BUILD[name] + 1 and all(" nt" in i for i in wide), wide       # the key vectors and the payload vector


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]


def test_constants_match_the_header(tmp_path):
    """HJGPU_LOOKUP_WIDE_MIN_KEYS / _MAX_KEYS as gcc reads them from include/hjgpu.h equal api's"""
    from hash_join_codes_knl_amd import api
    src = tmp_path / "constants.c"
    src.write_text('#include <stdio.h>\n#include "hjgpu.h"\nint main(void){printf("%u %u\\n", HJGPU_LOOKUP_WIDE_MIN_KEYS, HJGPU_LOOKUP_WIDE_MAX_KEYS);return 0;}\n')
    exe = tmp_path / "constants"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [api.LOOKUP_WIDE_MIN_KEYS, api.LOOKUP_WIDE_MAX_KEYS] == [2, 4], got
