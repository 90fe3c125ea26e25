"""CPU test (hipcc cross-compiles without a GPU): the semi- and anti-join kernels (HJGPU_FLAG_SEMI / _ANTI) exist for gfx950 in both
modes, use no scratch and no spills, store every global word non-temporally, and write two result columns - never a third."""
import collections
import re

import pytest

from device_compile import compile_device, instances, kernarg_bytes, _stores

MODES = {"1": "semi", "2": "anti"}
KERNELS = {"join_kernels.hip": ["exists_probe_kernel"], "npj_kernels.hip": ["npj_exists_kernel", "npj_exists_line_kernel"]}


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in KERNELS.items() for n in ns])
def test_instances_exist_in_both_modes(source, name):
    found, _ = instances(source, name)
    # MODE: the int template argument after the PACKED / MATERIALIZE / GROUPED bool (exists_probe_kernel<B, L, BATCH, PACKED, MODE, DEDUP>,
    # npj_exists_*_kernel<bool, MODE>)
    modes = collections.Counter(re.search(r"Lb[01]ELi([12])E", k).group(1) for k in found)
    assert set(modes) == {"1", "2"}, (name, sorted(found))
    assert not any("join_kernel" in k for k in found)


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in KERNELS.items() for n in ns])
def test_no_scratch_no_spills(source, name):
    _, res = compile_device(source)
    rows = {k: v for k, v in res.items() if k.startswith("void %s<" % name)}
    assert rows, name
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"]}
    assert not bad, bad


@pytest.mark.parametrize("source,name", [(s, n) for s, ns in KERNELS.items() for n in ns])
def test_every_store_non_temporal(source, name):
    found, _ = instances(source, name)
    assert found, name
    for k, body in found.items():
        plain = {s: n for s, n in _stores(body).items() if not s[1]}
        assert not plain, (k, plain)


@pytest.mark.parametrize("source,inner_name,names,oiv", [
    ("join_kernels.hip", "join_kernel", ["exists_probe_kernel"], 168),                      # offsetof(JoinArgs, oiv)
    ("npj_kernels.hip", "npj_probe_line_kernel", ["npj_exists_kernel", "npj_exists_line_kernel"], 80)])   # offsetof(NpjProbeArgs, oiv)
def test_no_third_row_column(source, inner_name, names, oiv):
    """the inner-join instances that materialise load the third result column's pointer (JoinArgs / NpjProbeArgs::oiv) from their
    arguments; no semi- / anti-join instance ever does, so none can store to it"""
    inner, _ = instances(source, inner_name)
    assert any(oiv in kernarg_bytes(b) for b in inner.values()), "the scan no longer finds the inner join's load of oiv"
    for name in names:
        found, _ = instances(source, name)
        assert found, name
        for k, body in found.items():
            assert oiv not in kernarg_bytes(body), k
