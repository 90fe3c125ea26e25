"""CPU test (hipcc cross-compiles without a GPU): the kernels of the right and full outer joins (HJGPU_FLAG_RIGHT_OUTER / _FULL_OUTER)
exist for gfx950 in exactly the planned instances, use no scratch and no spills, store every global word non-temporally, load both
payload columns' pointers (JoinArgs / NpjProbeArgs::oov and ::oiv) where they materialise, mark with an LDS OR and a global atomic OR,
and the tail kernels write whole 16-byte pieces.  Plus the flags' values in the Python package."""
import os
import re

import pytest

from device_compile import compile_device, instances, kernarg_bytes, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the probes that mark (PHJ / CPRA: table slots in LDS, then build rows in memory; NPJ: buckets in memory), and the tails that report
PROBES = {"join_kernels.hip": ["right_probe_kernel", "full_probe_kernel", "mark_probe_kernel"],
          "npj_kernels.hip": ["npj_right_kernel", "npj_full_kernel", "npj_right_line_kernel", "npj_full_line_kernel"]}
TAILS = {"join_kernels.hip": ["build_unmatched_kernel"], "npj_kernels.hip": ["npj_unmatched_kernel"]}
ALL = [(s, n) for group in (PROBES, TAILS) for s, ns in group.items() for n in ns]
OOV = {"join_kernels.hip": 160, "npj_kernels.hip": 72}       # offsetof(JoinArgs, oov), offsetof(NpjProbeArgs, oov)
OIV = {"join_kernels.hip": 168, "npj_kernels.hip": 80}       # offsetof(JoinArgs, oiv), offsetof(NpjProbeArgs, oiv)
GEOMETRIES = ((512, 13), (1024, 14))                          # the two geometries with a _UNIQUE instance


def planned(name):
    """mangled names of the instances hj_launch_join / hj_launch_build_unmatched / hj_launch_npj_probe / hj_launch_npj_unmatched launch"""
    n = len(name)
    if name in ("right_probe_kernel", "full_probe_kernel"):
        # <BLOCK, LOG2SLOTS, BATCH = 2, PACKED = true>: both geometries; packed inputs only - the broadcast join, the one user of column
        # inputs, is bypassed in these modes.  One launch each: a right outer join is planned like the inner join (fill groups); the
        # multi-fill items of a full outer join are reported by the left outer join's multi-fill instance and marked by mark_probe_kernel
        return {"_Z%d%sILi%dELi%dELi2ELb1EEv8JoinArgs" % (n, name, b, l) for b, l in GEOMETRIES}
    if name == "mark_probe_kernel":
        return {"_Z%d%sILi%dELi%dELi1ELb1EEv8JoinArgs" % (n, name, b, l) for b, l in GEOMETRIES}       # one vector per lane, as every multi-fill launch
    if name == "build_unmatched_kernel":
        return {"_Z%d%sILi%dEEv8JoinArgsj" % (n, name, b) for b, _ in GEOMETRIES}                       # <BLOCK>: the join's block, its worker slots
    if name == "npj_unmatched_kernel":
        return {"_Z%d%s12NpjProbeArgsj" % (n, name)}
    return {"_Z%d%sILb%dEEv12NpjProbeArgs" % (n, name, x) for x in (0, 1)}                              # <GROUPED> / <MATERIALIZE>


def found_instances(source, name):
    return instances(source, name)[0]


@pytest.mark.parametrize("source,name", ALL)
def test_every_planned_instance_exists(source, name):
    assert set(found_instances(source, name)) == planned(name), sorted(found_instances(source, name))


def test_the_left_outer_multi_fill_instance_a_full_outer_join_launches_exists():
    found = found_instances("join_kernels.hip", "outer_probe_kernel")
    for b, l in GEOMETRIES:
        assert "_Z18outer_probe_kernelILi%dELi%dELi1ELb1ELb0ELb1EEv8JoinArgs" % (b, l) in found


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


def _materialises(name, k):
    if name == "mark_probe_kernel":
        return False                                   # marks only: no rows
    if name.endswith("_line_kernel"):
        return "ILb1E" in k                            # MATERIALIZE
    return True


@pytest.mark.parametrize("source,name", ALL)
def test_materialising_instances_load_both_payload_columns(source, name):
    for k, body in found_instances(source, name).items():
        if not _materialises(name, k):
            continue
        args = kernarg_bytes(body)
        assert OOV[source] in args and OIV[source] in args, k
        assert _stores(body)[("dword", True)] >= 3, k


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in TAILS.items() for n in ns])
def test_tail_kernels_store_whole_vectors_non_temporally(source, name):
    for k, body in found_instances(source, name).items():
        assert re.search(r"global_store_dwordx4 .* nt", body), k
        assert _stores(body)[("dwordx4", True)] >= 3, k
        assert "global_load_dwordx4" in body, k        # the build array / the table in 16-byte pieces


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in PROBES.items() for n in ns])
def test_marking_instances_mark_atomically(source, name):
    for k, body in found_instances(source, name).items():
        assert "global_atomic_or" in body, k
        if source == "join_kernels.hip":
            assert "ds_or_b32" in body, k              # one bit per table slot in LDS, combined per build row in memory


@pytest.mark.parametrize("name", PROBES["join_kernels.hip"])
def test_two_workgroups_per_cu_still_fit_the_lds(name):
    """the slot bitmap (1 KiB at 8192 slots) beside the table: two 512-thread workgroups per CU in 160 KiB"""
    text, _ = compile_device("join_kernels.hip")
    sym = [k for k in found_instances("join_kernels.hip", name) if "ILi512E" in k][0]
    lds = int(re.search(r"\.amdhsa_kernel %s\s.*?\.amdhsa_group_segment_fixed_size (\d+)" % re.escape(sym), text, re.S).group(1))
    assert 0 < 2 * lds <= 160 * 1024, (name, lds)


def test_modes_keep_their_values():
    hdr = open(os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc", "hj_internal.hpp")).read()
    for name, value in (("HJ_MODE_SEMI", 1), ("HJ_MODE_ANTI", 2), ("HJ_MODE_RIGHT_OUTER", 4), ("HJ_MODE_FULL_OUTER", 5)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr), name


def test_flags_are_exported():
    import hash_join_codes_knl_amd as H
    assert H.FLAG_RIGHT_OUTER == 16 and H.FLAG_FULL_OUTER == 24 == (H.FLAG_LEFT_OUTER | H.FLAG_RIGHT_OUTER)
    assert "FLAG_RIGHT_OUTER" in H.__all__ and "FLAG_FULL_OUTER" in H.__all__
    hdr = open(os.path.join(ROOT, "include", "hjgpu.h")).read()
    assert re.search(r"#define HJGPU_FLAG_RIGHT_OUTER 16u", hdr)
    assert re.search(r"#define HJGPU_FLAG_FULL_OUTER \(HJGPU_FLAG_LEFT_OUTER \| HJGPU_FLAG_RIGHT_OUTER\)", hdr)
