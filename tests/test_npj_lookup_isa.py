"""CPU test (hipcc cross-compiles without a GPU): the kernels of the positional NPJ look-up (hjgpu_npj_lookup*) exist for gfx950 in exactly
the planned instances, use no scratch and no spills and store every global word non-temporally; an instance that writes values holds a
16-byte store, the aggregate-only instances hold no 4- or 16-byte global store at all.  Plus the three entry points in the library and
in the Python binding."""
import re

import pytest

from device_compile import compile_device, _stores

SOURCE = "npj_kernels.hip"
KERNELS = ["npj_lookup_line_kernel", "npj_lookup_kernel"]
ENTRY_POINTS = ["hjgpu_npj_lookup", "hjgpu_npj_lookup_async", "hjgpu_npj_lookup_table"]


def planned(name):
    """{mangled name: (VALS, BITS)} of the instances hj_launch_npj_lookup launches"""
    n = len(name)
    if name == "npj_lookup_line_kernel":                                      # <VALS, BITS>
        return {"_Z%d%sILb%dELb%dEEv13NpjLookupArgs" % (n, name, v, b): (v, b) for v in (0, 1) for b in (0, 1)}
    return {"_Z%d%sILb%dELb%dELb%dEEv13NpjLookupArgs" % (n, name, g, v, b): (v, b) for g in (0, 1) for v in (0, 1) for b in (0, 1)}      # <GROUPED, VALS, BITS>


def found_instances(name):
    text, _ = compile_device(SOURCE)
    out = {}
    for m in re.finditer(r"^(_Z%d%sI\w+13NpjLookupArgs):\s*; @" % (len(name), name), text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


@pytest.mark.parametrize("name", KERNELS)
def test_every_planned_instance_exists(name):
    assert set(found_instances(name)) == set(planned(name)), sorted(found_instances(name))


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_spills(name):
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?%s[<(]" % name, k)}
    assert len(rows) == len(planned(name)), sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"]}
    assert not bad, bad


@pytest.mark.parametrize("name", KERNELS)
def test_every_store_non_temporal(name):
    found = found_instances(name)
    assert found, name
    for k, body in found.items():
        plain = {s: n for s, n in _stores(body).items() if not s[1]}
        assert not plain, (k, plain)


@pytest.mark.parametrize("name", KERNELS)
def test_stores_follow_the_template_arguments(name):
    found = found_instances(name)
    for k, (vals, bits) in planned(name).items():
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
