"""CPU test (hipcc cross-compiles without a GPU): the left outer join kernels (HJGPU_FLAG_LEFT_OUTER) exist for gfx950 in every planned
instance, use no scratch and no spills, store every global word non-temporally, and - materialising - write the third result column
(its pointer, JoinArgs / NpjProbeArgs::oiv, is loaded from the kernel arguments)."""
import collections
import itertools
import re

import pytest

from device_compile import compile_device, instances, kernarg_bytes, _stores

KERNELS = {"join_kernels.hip": ["outer_probe_kernel"], "npj_kernels.hip": ["npj_outer_kernel", "npj_outer_line_kernel"]}
OIV = {"join_kernels.hip": 168, "npj_kernels.hip": 80}       # offsetof(JoinArgs, oiv), offsetof(NpjProbeArgs, oiv)


def _b(x):
    return "1" if x else "0"


def planned(name):
    """mangled-name prefixes of the instances hj_launch_join / hj_launch_npj_probe launch"""
    if name == "outer_probe_kernel":
        # <BLOCK, LOG2SLOTS, BATCH, PACKED, UNIQUE, DEDUP>: both _UNIQUE geometries, packed and column inputs, the full and the
        # first-match walk, the single-fill launch (two vectors per lane) and the multi-fill one (one vector)
        return {"_Z18outer_probe_kernelILi%dELi%dELi%dELb%sELb%sELb%sEEv8JoinArgs" % (b, l, 1 if dd else 2, _b(p), _b(u), _b(dd))
                for (b, l), p, u, dd in itertools.product(((512, 13), (1024, 14)), (True, False), (True, False), (True, False))}
    n = len(name)
    return {"_Z%d%sILb%sELb%sEEv12NpjProbeArgs" % (n, name, _b(x), _b(u)) for x, u in itertools.product((True, False), (True, False))}


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in KERNELS.items() for n in ns])
def test_every_planned_instance_exists(source, name):
    found, _ = instances(source, name)
    assert set(found) == planned(name), sorted(found)


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in KERNELS.items() for n in ns])
def test_no_scratch_no_spills(source, name):
    _, res = compile_device(source)
    rows = {k: v for k, v in res.items() if k.startswith("void %s<" % name)}
    assert len(rows) == len(planned(name)), sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"]}
    assert not bad, bad


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in KERNELS.items() for n in ns])
def test_every_store_non_temporal(source, name):
    found, _ = instances(source, name)
    assert found, name
    for k, body in found.items():
        stores = _stores(body)
        plain = {s: n for s, n in stores.items() if not s[1]}
        assert not plain, (k, plain)


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in KERNELS.items() for n in ns])
def test_materialising_instances_write_three_columns(source, name):
    """every instance that can materialise loads the third result column's pointer from its arguments and stores 4-byte rows; the
    outer_probe_kernel single-fill instances also store whole 16-byte pieces (emit4)"""
    found, _ = instances(source, name)
    for k, body in found.items():
        if name == "npj_outer_line_kernel" and k.startswith("_Z21npj_outer_line_kernelILb0"):
            continue                                   # MATERIALIZE = false: no rows
        assert OIV[source] in kernarg_bytes(body), k
        stores = _stores(body)
        assert stores[("dword", True)] >= 3, (k, stores)
        if name == "outer_probe_kernel" and k.endswith("ELb0EEv8JoinArgs"):
            assert stores[("dwordx4", True)] >= 3, (k, stores)
