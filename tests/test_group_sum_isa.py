"""CPU test (hipcc cross-compiles without a GPU): the kernels of hjgpu_group_sum in gen_kernels.hip - group_sum_kernel<NKEYS, SEL> and
group_emit_kernel - exist for gfx950 in exactly the planned instances (NKEYS 1 and 2, each with and without a mask, plus the emit), use no
scratch and no spills, and store every global word non-temporally: the aggregation has no global store at all (it reaches memory through
atomics alone), the emit holds the 4-byte key stores and the 8-byte count and sum stores.  The aggregation's table accesses are the ones
DESIGN.md names: a 64-bit LDS compare-and-swap, 64-bit LDS adds, a 64-bit global compare-and-swap and adds; its column loads are
non-temporal.  Plus the two entry points in the library, in EXPORTS and on HjGpu."""
import re

import pytest

from device_compile import compile_device, _stores

SOURCE = "gen_kernels.hip"
ENTRY_POINTS = ["hjgpu_group_sum", "hjgpu_group_sum_async"]
AGGREGATE = {"_Z16group_sum_kernelILi%dELb%dEEv9GroupArgs" % (nkeys, sel): (nkeys, sel) for nkeys in (1, 2) for sel in (0, 1)}
EMIT = "_Z17group_emit_kernel13GroupEmitArgs"


def found_instances():
    text, _ = compile_device(SOURCE)
    out = {}
    for m in re.finditer(r"^(_Z\d+group_\w+):\s*; @", text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


def instructions(body):
    return [line.split(";")[0].strip() for line in body.splitlines() if line.split(";")[0].strip()]


def test_every_planned_instance_exists():
    assert len(AGGREGATE) == 4
    assert set(found_instances()) == set(AGGREGATE) | {EMIT}, sorted(found_instances())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?group_(sum|emit)_kernel[<(]", k)}
    assert len(rows) == 5, sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad


def test_every_store_non_temporal():
    found = found_instances()
    assert found
    for k, body in found.items():
        plain = {s: n for s, n in _stores(body).items() if not s[1]}
        assert not plain, (k, plain)
    for k in AGGREGATE:
        assert not _stores(found[k]), (k, _stores(found[k]))                        # atomics only
    stores = _stores(found[EMIT])
    assert stores[("dword", True)] >= 2 and stores[("dwordx2", True)] >= 5, stores     # two key columns; the count and four sums


@pytest.mark.parametrize("name", sorted(AGGREGATE))
def test_the_aggregation_reaches_its_tables_through_atomics(name):
    nkeys, sel = AGGREGATE[name]
    ins = instructions(found_instances()[name])

    def count(prefix):
        return sum(1 for i in ins if i.startswith(prefix))
    assert count("ds_cmpst_rtn_b64") >= 1 and count("ds_add_u64") >= 1, name
    assert count("global_atomic_cmpswap_x2") >= 1 and count("global_atomic_add_x2") >= 1 and count("global_atomic_or") >= 1, name
    assert not count("flat_"), [i for i in ins if i.startswith("flat_")]
    # the columns: 16-byte non-temporal loads and no other 16-byte global load; the mask: a 4-byte non-temporal load where there is one
    wide = [i for i in ins if i.startswith("global_load_dwordx4")]
    assert len(wide) >= 2 * (nkeys + 1) and all(" nt" in i for i in wide), wide
    words = [i for i in ins if re.match(r"global_load_dword\s", i) and " nt" in i]
    assert (len(words) >= 1) == bool(sel), words


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]
