"""CPU test (hipcc cross-compiles without a GPU): the kernel of the LDS look-up (hjgpu_lookup*: lds_lookup_kernel<BLOCK, LOG2SLOTS, VALS,
BITS>, join_kernels.hip) exists for gfx950 in exactly the eight planned instances - <512, 13> and <1024, 14>, each with every pair of
outputs -, uses no scratch and no spills and stores every global word non-temporally; an instance that writes values holds a 16-byte
store, the aggregate-only instances hold no 4- or 16-byte global store at all.  Plus the two entry points in the library and in the
Python binding."""
import re

from device_compile import compile_device, _stores

SOURCE = "join_kernels.hip"
NAME = "lds_lookup_kernel"
ENTRY_POINTS = ["hjgpu_lookup", "hjgpu_lookup_async"]
# {mangled name: (VALS, BITS)} of the instances hj_launch_lds_lookup launches
PLANNED = {"_Z%d%sILi%dELi%dELb%dELb%dEEv13LdsLookupArgs" % (len(NAME), NAME, block, log2slots, v, b): (v, b)
           for block, log2slots in ((512, 13), (1024, 14)) for v in (0, 1) for b in (0, 1)}


def found_instances():
    text, _ = compile_device(SOURCE)
    out = {}
    for m in re.finditer(r"^(_Z%d%sI\w+13LdsLookupArgs):\s*; @" % (len(NAME), NAME), text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


def test_every_planned_instance_exists():
    assert len(PLANNED) == 8
    assert set(found_instances()) == set(PLANNED), sorted(found_instances())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?%s[<(]" % NAME, k)}
    assert len(rows) == len(PLANNED), sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"]}
    assert not bad, bad


def test_every_store_non_temporal():
    found = found_instances()
    assert found
    for k, body in found.items():
        plain = {s: n for s, n in _stores(body).items() if not s[1]}
        assert not plain, (k, plain)


def test_stores_follow_the_template_arguments():
    found = found_instances()
    for k, (vals, bits) in PLANNED.items():
        stores = _stores(found[k])
        if vals:
            assert stores[("dwordx4", True)] >= 1, (k, stores)             # a lane's four answers in one store
        if not vals and not bits:
            assert not [s for s in stores if s[0] in ("dword", "dwordx4")], (k, stores)


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]
