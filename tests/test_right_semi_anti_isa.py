"""CPU test (hipcc cross-compiles without a GPU): the kernels of the right semi- and right anti-joins (HJGPU_FLAG_RIGHT_SEMI / _RIGHT_ANTI)
exist for gfx950 in exactly the planned instances, use no scratch and no spills and store every global word non-temporally; the probes
mark with an LDS OR plus a global atomic OR (PHJ / CPRA) or a global atomic OR (NPJ) and hold no store to a result column; the tails
write whole 16-byte pieces into two columns, d_keys and d_inner_vals.  Plus the flags' values in the Python package."""
import os
import re

import pytest

from device_compile import compile_device, instances, kernarg_bytes, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the probes that only mark (PHJ / CPRA: table slots in LDS, then build rows in memory; NPJ: buckets in memory), and the tails that report
PROBES = {"join_kernels.hip": ["mark_single_probe_kernel", "mark_probe_kernel"], "npj_kernels.hip": ["npj_mark_kernel", "npj_mark_line_kernel"]}
TAILS = {"join_kernels.hip": ["build_rows_kernel"], "npj_kernels.hip": ["npj_rows_kernel"]}
ALL = [(s, n) for group in (PROBES, TAILS) for s, ns in group.items() for n in ns]
OK = {"join_kernels.hip": 152, "npj_kernels.hip": 64}        # offsetof(JoinArgs, ok), offsetof(NpjProbeArgs, ok)
OOV = {"join_kernels.hip": 160, "npj_kernels.hip": 72}       # ... oov
OIV = {"join_kernels.hip": 168, "npj_kernels.hip": 80}       # ... oiv
GEOMETRIES = ((512, 13), (1024, 14))                          # the two geometries with mode instances


def planned(name):
    """mangled names of the instances hj_launch_join / hj_launch_build_rows / hj_launch_npj_probe / hj_launch_npj_rows launch"""
    n = len(name)
    if name == "mark_single_probe_kernel":
        # <BLOCK, LOG2SLOTS, BATCH = 2, PACKED = true>: the single-fill items, two probe vectors per lane; packed inputs only - the
        # broadcast join, the one user of column inputs, is bypassed in these modes
        return {"_Z%d%sILi%dELi%dELi2ELb1EEv8JoinArgs" % (n, name, b, l) for b, l in GEOMETRIES}
    if name == "mark_probe_kernel":
        return {"_Z%d%sILi%dELi%dELi1ELb1EEv8JoinArgs" % (n, name, b, l) for b, l in GEOMETRIES}       # the multi-fill items: as the full outer join's
    if name == "build_rows_kernel":
        return {"_Z%d%sILi%dEEv8JoinArgsjj" % (n, name, b) for b, _ in GEOMETRIES}                      # <BLOCK>(args, split, flip)
    if name == "npj_rows_kernel":
        return {"_Z%d%s12NpjProbeArgsj" % (n, name)}                                                     # (args, flip)
    if name == "npj_mark_line_kernel":
        return {"_Z%d%s12NpjProbeArgs" % (n, name)}                                                      # never materialises: one instance
    return {"_Z%d%sILb%dEEv12NpjProbeArgs" % (n, name, x) for x in (0, 1)}                              # npj_mark_kernel<GROUPED>


def found_instances(source, name):
    text, _ = compile_device(source)
    # (exact kernel names: a non-template kernel's symbol has no template arguments behind its name)
    out = {}
    for m in re.finditer(r"^(_Z%d%s(?:I\w+)?(?:8JoinArgs|12NpjProbeArgs)\w*):\s*; @" % (len(name), name), text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


@pytest.mark.parametrize("source,name", ALL)
def test_every_planned_instance_exists(source, name):
    assert set(found_instances(source, name)) == planned(name), sorted(found_instances(source, name))


@pytest.mark.parametrize("source,name", ALL)
def test_no_scratch_no_spills(source, name):
    _, res = compile_device(source)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?%s[<(]" % name, k)}
    assert len(rows) == len(planned(name)), sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"]}
    assert not bad, bad


@pytest.mark.parametrize("source,name", ALL)
def test_every_store_non_temporal(source, name):
    found = found_instances(source, name)
    assert found, name
    for k, body in found.items():
        plain = {s: n for s, n in _stores(body).items() if not s[1]}
        assert not plain, (k, plain)


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in PROBES.items() for n in ns])
def test_marking_probes_hold_no_store_to_a_result_column(source, name):
    """no row: the payload columns' pointers are not even loaded, nothing is stored through a 4- or 16-byte store (what EmitterT writes
    rows with), and the only global store left is the 8-byte cursor of a wave (hj_leave_cursor, never reached: the launches pass no
    output columns).  The sums every lane carries are constant zeros, so the epilogue's atomics never run"""
    for k, body in found_instances(source, name).items():
        args = kernarg_bytes(body)
        assert OOV[source] not in args and OIV[source] not in args, k
        stores = _stores(body)
        assert not [s for s in stores if s[0] != "dwordx2"], (k, stores)
        assert sum(stores.values()) <= 1, (k, stores)


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in PROBES.items() for n in ns])
def test_marking_instances_mark_atomically(source, name):
    for k, body in found_instances(source, name).items():
        assert "global_atomic_or" in body, k
        if source == "join_kernels.hip":
            assert "ds_or_b32" in body, k              # one bit per table slot in LDS, combined per build row in memory


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in TAILS.items() for n in ns])
def test_tail_kernels_store_two_columns_in_whole_vectors_non_temporally(source, name):
    for k, body in found_instances(source, name).items():
        args = kernarg_bytes(body)
        assert OK[source] in args and OIV[source] in args and OOV[source] not in args, k      # d_keys and d_inner_vals; d_outer_vals not even loaded
        assert re.search(r"global_store_dwordx4 .* nt", body), k
        assert _stores(body)[("dwordx4", True)] >= 2, k
        assert _stores(body)[("dword", True)] >= 2, k
        assert "global_load_dwordx4" in body, k        # the build array / the table in 16-byte pieces


@pytest.mark.parametrize("name", PROBES["join_kernels.hip"])
def test_two_workgroups_per_cu_still_fit_the_lds(name):
    """the slot bitmap (1 KiB at 8192 slots) beside the table: two 512-thread workgroups per CU in 160 KiB"""
    text, _ = compile_device("join_kernels.hip")
    sym = [k for k in found_instances("join_kernels.hip", name) if "ILi512E" in k][0]
    lds = int(re.search(r"\.amdhsa_kernel %s\s.*?\.amdhsa_group_segment_fixed_size (\d+)" % re.escape(sym), text, re.S).group(1))
    assert 0 < 2 * lds <= 160 * 1024, (name, lds)


def test_modes_keep_their_values():
    hdr = open(os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc", "hj_internal.hpp")).read()
    for name, value in (("HJ_MODE_MARK", 6), ("HJ_MODE_RIGHT_SEMI", 7), ("HJ_MODE_RIGHT_ANTI", 8)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr), name


def test_flags_are_exported():
    import hash_join_codes_knl_amd as H
    assert H.FLAG_RIGHT_SEMI == 32 and H.FLAG_RIGHT_ANTI == 64
    assert "FLAG_RIGHT_SEMI" in H.__all__ and "FLAG_RIGHT_ANTI" in H.__all__
    hdr = open(os.path.join(ROOT, "include", "hjgpu.h")).read()
    assert re.search(r"#define HJGPU_FLAG_RIGHT_SEMI 32u", hdr)
    assert re.search(r"#define HJGPU_FLAG_RIGHT_ANTI 64u", hdr)
