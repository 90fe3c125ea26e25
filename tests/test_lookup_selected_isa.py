"""CPU test (hipcc cross-compiles without a GPU): the three kernels of the selected look-ups (hjgpu_lookup_selected*,
hjgpu_npj_lookup_table_selected) - npj_lookup_sel_line_kernel<VALS, BITS> and npj_lookup_sel_kernel<GROUPED, VALS, BITS> in npj_kernels.hip,
lds_lookup_sel_kernel<BLOCK, LOG2SLOTS, VALS, BITS> in join_kernels.hip - exist for gfx950 in exactly the planned instances, use no
scratch and no spills and store every global word non-temporally; an instance that writes values holds a 16-byte store, the
aggregate-only instances hold no 4- or 16-byte global store at all.  Plus the three entry points in the library and in the Python
binding.  Stores and resources only."""
import re

import pytest

from device_compile import compile_device, _stores

ENTRY_POINTS = ["hjgpu_lookup_selected", "hjgpu_lookup_selected_async", "hjgpu_npj_lookup_table_selected"]
PAIRS = [(v, b) for v in (0, 1) for b in (0, 1)]


def _mangled(name, args, struct):
    return "_Z%d%sI%sEv%d%s" % (len(name), name, "".join(args), len(struct), struct)


def _b(x):
    return "Lb%dE" % x


# kernel: (source, argument struct, {mangled name: (VALS, BITS)} of the instances its launcher launches)
KERNELS = {
    "npj_lookup_sel_line_kernel": ("npj_kernels.hip", "NpjLookupSelArgs",
                                   {_mangled("npj_lookup_sel_line_kernel", [_b(v), _b(b)], "NpjLookupSelArgs"): (v, b) for v, b in PAIRS}),
    "npj_lookup_sel_kernel": ("npj_kernels.hip", "NpjLookupSelArgs",
                              {_mangled("npj_lookup_sel_kernel", [_b(g), _b(v), _b(b)], "NpjLookupSelArgs"): (v, b)
                               for g in (0, 1) for v, b in PAIRS}),
    "lds_lookup_sel_kernel": ("join_kernels.hip", "LdsLookupSelArgs",
                              {_mangled("lds_lookup_sel_kernel", ["Li%dE" % block, "Li%dE" % log2slots, _b(v), _b(b)], "LdsLookupSelArgs"): (v, b)
                               for block, log2slots in ((512, 13), (1024, 14)) for v, b in PAIRS}),
}


def found_instances(name):
    source, struct, _ = KERNELS[name]
    text, _ = compile_device(source)
    out = {}
    for m in re.finditer(r"^(_Z%d%sI\w+%d%s):\s*; @" % (len(name), name, len(struct), struct), text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_every_planned_instance_exists(name):
    planned = KERNELS[name][2]
    assert len(planned) == (4 if name == "npj_lookup_sel_line_kernel" else 8)
    assert set(found_instances(name)) == set(planned), sorted(found_instances(name))


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_scratch_no_spills(name):
    source, _, planned = KERNELS[name]
    _, res = compile_device(source)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?%s[<(]" % name, k)}
    assert len(rows) == len(planned), sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_every_store_non_temporal(name):
    found = found_instances(name)
    assert found, name
    for k, body in found.items():
        plain = {s: n for s, n in _stores(body).items() if not s[1]}
        assert not plain, (k, plain)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_stores_follow_the_template_arguments(name):
    found = found_instances(name)
    for k, (vals, bits) in KERNELS[name][2].items():
        stores = _stores(found[k])
        if vals:
            assert stores[("dwordx4", True)] >= 1, (k, stores)             # a lane's four answers in one store
        if bits:
            assert stores[("dword", True)] >= 1, (k, stores)               # a word of the bitmap
        if not vals and not bits:
            assert not [s for s in stores if s[0] in ("dword", "dwordx4")], (k, stores)


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]
