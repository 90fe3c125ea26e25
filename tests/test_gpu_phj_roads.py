"""Every road of the PHJ enqueue path ("Roads of the PHJ enqueue path") on ONE pair of relations: 5 003 build rows with
duplicated keys, 40 009 probe rows of which about half find a partner, PhjParams(fanout1=8, fanout2=4) - two passes with ragged last
tiles.  The roads are those of tools/launch_sequence.py (which lists their launches); here their results are checked: aggregates
against helpers.numpy_join, materialised rows against helpers.materialised_rows, and the plan that hjgpu_get_stats reports.
The batched road takes test_gpu_shapes.py's probe size and batch_tuples, the grouped roads test_gpu_grouped.py's group_from / group_inner:
the smallest at which they engage (and a grouped plan is never an explicit one: it reports the fan-out chosen for a group, 64 x 1).
The three roads with a join mode report build rows that the inner join does not have: numpy_join gives their inner part, the rest
follows from the mode's definition."""
import importlib.util
import os

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from helpers import numpy_join, materialised_rows, sort_rows

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("launch_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               "tools", "launch_sequence.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)
NULL = np.uint32(H.NULL_VAL)


@pytest.fixture(scope="module")
def table(hj):
    """the roads (after the session's context: torch, where it is installed, has initialised the GPU first - conftest.py)"""
    return {name: (options, rel, fn) for name, options, rel, fn in L.roads()}


@pytest.fixture(scope="module")
def wanted():
    """numpy_join of every pair of relations the roads use, computed once"""
    cache = {}

    def want(rel):
        key = (len(rel[0]), len(rel[2]))
        if key not in cache:
            cache[key] = numpy_join(*rel)
        return cache[key]
    return want


def _sum(a):
    return int(a.astype(np.uint64).sum(dtype=np.uint64)) & L.M64


# what hjgpu_get_stats reports after the road: (fanout1, fanout2, batches, groups); batches None: two or more (the bar of
# test_gpu_shapes.py for the same sizes).  A host pipeline's stats count its upload batches: 40 009 probe rows are far below two
# batches, so the columns go up whole and it reports none
PLAN = {name: (8, 4, 0, 0) for name in L.NAMES}
PLAN.update({"09 one pass": (32, 1, 0, 0), "11 batch_tuples": (8, 4, None, 0), "12 grouped device-planned": (64, 1, 0, 2),
             "13 grouped host-planned": (64, 1, 0, 2), "18 npj + npj_lookup": (0, 0, 0, 0), "19a join_host phj": (8, 4, 0, 0),
             "19b join_host npj": (0, 0, 0, 0)})


@pytest.mark.parametrize("name", L.NAMES)
def test_road(table, wanted, name):
    options, rel, fn = table[name]
    ik, iv, ok, ov = rel
    got = L.run_road(options, rel, fn)
    inner = wanted(rel)
    unmatched = ~np.isin(ik, ok)
    rows = None
    if name == "15 right outer rows":
        # S RIGHT JOIN R: the inner join, and every build row without a partner with a NULL outer_val
        want = (inner[0] + int(unmatched.sum()), (inner[1] + _sum(ik[unmatched])) & L.M64, inner[2], (inner[3] + _sum(iv[unmatched])) & L.M64)
        wk, wo, wi = materialised_rows(ik, iv, ok, ov)
        rows = sort_rows(np.concatenate([wk, ik[unmatched]]), np.concatenate([wo, np.full(int(unmatched.sum()), NULL)]), np.concatenate([wi, iv[unmatched]]))
    elif name == "16 right semi rows":
        # the build rows with a partner, (key, inner_val) each
        k, i = ik[~unmatched], iv[~unmatched]
        want = (len(k), _sum(k), 0, _sum(i))
        idx = np.lexsort((i, k))
        rows = (k[idx], i[idx])
    elif name == "17 full outer empty probe":
        assert inner == (0, 0, 0, 0)
        want = (len(ik), _sum(ik), 0, _sum(iv))
        rows = sort_rows(ik, np.full(len(ik), NULL), iv)
    else:
        want = inner
    print(name, "got", got["agg"], "want", want, {k: got["stats"][k] for k in ("fanout1", "fanout2", "batches", "groups")})
    assert tuple(got["agg"]) == want
    if rows is not None:
        mine = got["rows"]
        idx = np.lexsort(tuple(reversed(mine)))
        assert len(mine) == len(rows) and all(np.array_equal(m[idx], w) for m, w in zip(mine, rows))
    f1, f2, batches, groups = PLAN[name]
    st = got["stats"]
    assert (st["fanout1"], st["fanout2"], st["groups"]) == (f1, f2, groups)
    assert st["batches"] >= 2 if batches is None else st["batches"] == batches
    if "lookup" in got:
        # the look-up's aggregates count every probe key with a partner once; bit i answers probe key i, and where the build key is
        # unique the payload is its partner's
        hit = np.isin(ok, ik)
        assert got["lookup"][0] == int(hit.sum()) and got["lookup"][1] == _sum(ok[hit])
        bits = np.unpackbits(got["lookup_bits"].view(np.uint8), bitorder="little")[:len(ok)].astype(bool)
        assert np.array_equal(bits, hit)
        keys, counts = np.unique(ik, return_counts=True)
        once = np.isin(ok, keys[counts == 1])
        order = np.argsort(ik, kind="stable")
        assert np.array_equal(got["lookup_vals"][once], iv[order][np.searchsorted(ik[order], ok[once])])
