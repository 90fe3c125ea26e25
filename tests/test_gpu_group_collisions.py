"""GPU tests of hjgpu_group_sum, hjgpu_group_agg and hjgpu_group_by with key tuples crafted to collide in their tables.

The operators keep their groups in two open-addressed tables with linear probing - a workgroup's in LDS, the merge table in device
memory (csrc/gen_kernels.hip: group_lds_slot, group_merge_slot, hj_wide::find_slot, the flushes) - whose load the code fixes at no
more than a half, so with well-mixed keys no walk is longer than a handful of slots.  Here the keys are computed from the hash
(tests/collision_keys.py; tests/test_collision_keys.py pins every set to the headers on the CPU), so that the walks are hundreds of slots
long, pass the last slot of either table, end at the LDS table's probe bound, meet in one chain of the merge table from several
workgroups at once, fill it, and - wide keys - pass slots whose leading key words are their own:

  a  200 tuples with one LDS home in mid-table: all of them live in LDS, after walks of up to 200 slots
  b  the same at home LDS_SLOTS - 3: the walk goes on at slot 0 and keeps out of what lies behind the last slot (narrow layout: the
     slot of tuple 0)
  c  LDS_PROBES + 44 tuples with one LDS home, all of them in every workgroup: at least 44 leave each table by the probe bound (the
     table holds fewer than LDS_GROUPS tuples, so not because it is full); also at home LDS_SLOTS - 3
  d  300 tuples with one merge home (the hash's low 20 bits are 5), eight workgroups flushing the one chain at once; the smallest
     table and one of 2^20 slots
  e  the same at home slots - 3 (low 20 bits 0xFFFFD), tables of 1024 and 8192 slots: the chain wraps to slot 0, not into merge[slots]
  f  LDS_PROBES + 44 tuples that share both homes: rows leave LDS by the probe bound straight into a long wrapping merge chain that the
     other workgroups flush into.  Two keys and more: one key has 32 bits to choose and pins one home
  g  1100 tuples with merge home slots - 3 at capacity 511, 1024 slots: HJGPU_EOVERFLOW, capacity < count <= J, nothing written behind
     capacity
  h  wide keys whose colliding tuples share key words: all columns but the last fixed, all but the first fixed, and - four keys -
     keys 0 and 1 fixed with both homes pinned

One key column pins a merge home of 10 bits by scanning, which is the home in the smallest table only: its d, e and g run there alone.

Every case runs without a mask and under a half mask that leaves every workgroup a row of every crafted tuple.  Beside the crafted
tuples there are the all-zero tuple, with a row count no other group has, and 50 random ones.  The calls are the existing helpers'
(test_gpu_group_sum.group, test_gpu_group_agg.agg, test_gpu_group_by.by): exact equality with numpy in every output, canaries behind
capacity, mask and inputs read back unchanged.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import functools

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
import collision_keys as C
from test_gpu_lookup_selected import hj        # noqa: F401 (the fixture)
from test_gpu_group_sum import group, measures, expected
from test_gpu_group_agg import agg, values, all_four, want_agg
from test_gpu_group_by import by

pytestmark = pytest.mark.gpu

FAMILIES = {"group_sum": (1, 2), "group_agg": (1, 2), "group_by": (3, 4)}
CASES = [(name, family, nkeys) for name, nkeys in C.CASES for family, served in FAMILIES.items() if nkeys in served]


@functools.lru_cache(maxsize=None)
def inputs(name, nkeys):
    """the key columns of the scenario's rows and its two masks (shared by the families, never written)"""
    tuples, _ = C.scenario(name, nkeys)
    ids, sels = C.masked_rows(name, nkeys)
    keys = tuple(np.ascontiguousarray(tuples[ids, c]) for c in range(nkeys))
    for k in keys:
        k.setflags(write=False)
    return keys, sels, len(tuples)


@pytest.mark.parametrize("name,family,nkeys", CASES)
def test_crafted_collisions(hj, name, family, nkeys):
    assert hj.counter("group_lds_groups") == C.NARROW.LDS_GROUPS and hj.counter("group_by_lds_groups") == C.WIDE.LDS_GROUPS
    keys, sels, S = inputs(name, nkeys)
    keys = list(keys)
    n = len(keys[0])
    assert hj.device_info()["compute_units"] >= -(-n // C.BLOCK_ROWS), "a workgroup would own more than one run of BLOCK_ROWS rows"
    overflow = C.SCENARIOS[name].get("overflow", False)
    for kind in ("null", "half"):
        sel = sels[kind]
        if family == "group_sum":
            vals = measures(n, 2, seed=nkeys)
            want = expected(keys, vals, sel)
        else:
            aggs = all_four(values(n, nkeys), values(n, nkeys + 10), flip=H.AGG_SIGNED if kind == "half" else 0)
            want = want_agg(keys, aggs, sel)
        uniq, counts = want[0], want[1]
        assert len(uniq) == S and not uniq[0].any() and int((counts == counts[0]).sum()) == 1      # every tuple; tuple 0's count is its own
        for capacity in C.capacities(name, nkeys):
            if family == "group_sum":
                got = group(hj, keys, vals, sel, kind, capacity=capacity, overflow=overflow, want=want)
            elif family == "group_agg":
                got = agg(hj, keys, aggs, sel, kind, capacity=capacity, overflow=overflow, want=want)
            else:
                got = by(hj, keys, aggs, sel, kind, capacity=capacity, overflow=overflow, want=want)
            assert overflow or got == S
