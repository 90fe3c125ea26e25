"""Every road of a multi-GPU step ("Roads of a CPRA step") on ONE device and ONE pair of relations: the roads of
tools/launch_sequence.py --multi (which lists their launches) - 5 003 build rows with duplicated keys, 40 009 probe rows of which about
half find a partner, cut evenly into the ranks' chunks; the loopback transport puts a world of 2 or 3 on device 0, RCCL runs at world 1.
Here their results are checked: the four aggregates against helpers.numpy_join, materialised rows against helpers.materialised_rows,
`self_copies` of the in-place and the copying exchange, and what option "debug_forensics" leaves behind."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from helpers import numpy_join, materialised_rows, sort_rows

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("launch_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               "tools", "launch_sequence.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)


@pytest.fixture(scope="module")
def table(hj):
    """the roads (after the session's context: torch, where it is installed, has initialised the GPU first - conftest.py)"""
    return {t[0]: t[1:] for t in L.multi_roads()}


@pytest.fixture(scope="module")
def rel():
    return L.relations()


@pytest.fixture(scope="module")
def want(rel):
    """the definition of the join, computed once: (aggregates, sorted rows)"""
    return numpy_join(*rel), sort_rows(*materialised_rows(*rel))


@pytest.mark.parametrize("name", L.MULTI_NAMES)
def test_road(table, rel, want, name):
    got = L.run_multi_road(*table[name], rel=rel)
    st = got["stats"]
    print(name, "got", got["agg"], "want", want[0], {k: st[k] for k in ("joins", "self_copies", "bytes_sent")}, "groups", st["join"]["groups"])
    assert tuple(got["agg"]) == want[0]
    if "rows" in got:
        assert len(got["rows"][0]) == want[0][0]
        assert all(np.array_equal(m, w) for m, w in zip(sort_rows(*got["rows"]), want[1]))
    # a rank's message to itself: never copied where it stays behind the rank's own partitions; copied by the build side's
    # exchange at the least where the exchange is not in place
    if name == "20a cpra loopback 2 in place":
        assert st["self_copies"] == 0
    if name == "20b cpra loopback 2 exchange_in_place 0":
        assert st["self_copies"] >= 1
    # the grouped road is taken: a rank's local join reports its groups (2 501 build rows in groups of 1 250)
    if name == "20e cpra loopback 2 grouped":
        assert st["join"]["groups"] >= 2


def _unique_relations():
    """unique build keys, every probe key with exactly one partner: the workload whose stages option "debug_forensics" = 2 can judge
    (a probe's result has the batch's count and sums)"""
    rng = np.random.default_rng(28)
    ik = np.unique(rng.integers(1, 2**32 - 1, size=2 * L.INNER, dtype=np.uint64).astype(np.uint32))[:L.INNER]
    rng.shuffle(ik)
    iv = rng.integers(0, 2**32 - 1, size=L.INNER, dtype=np.uint64).astype(np.uint32)
    ok = ik[rng.integers(0, L.INNER, size=L.OUTER)]
    ov = rng.integers(0, 2**32 - 1, size=L.OUTER, dtype=np.uint64).astype(np.uint32)
    return ik, iv, ok, ov


def _forensics_words(comm, fn):
    n = C.c_size_t(0)
    assert fn(comm.handle, None, 0, C.byref(n)) == 0
    buf = (C.c_uint64 * max(1, n.value))()
    assert fn(comm.handle, buf, n.value, C.byref(n)) == 0
    return [int(x) for x in buf[:n.value]]


@pytest.mark.parametrize("level", [1, 2])
def test_forensics_of_a_step(hj, level):
    """world 2 in place, 3 slices.  Option "debug_forensics" = 1: hjgpu_comm_get_forensics holds, per rank, {global rank, np, nj} and
    then 32 words for each of its np partitioning and nj join records - a rank partitions its build chunk and 3 probe slices (4 calls,
    kind 3) and joins by one build (kind 1) and 3 probes (kind 2; every slice fits one batch).  = 2 on correct data: nothing is frozen."""
    rel = _unique_relations()
    m = L.MultiRun(2, "loopback", rel, (("debug_forensics", level),))
    try:
        got = L.mroad_cpra(m)
        assert tuple(got["agg"]) == numpy_join(*rel)
        words = _forensics_words(m.comm, m.comm.lib.hjgpu_comm_get_forensics)
        at, ranks = 0, []
        while at < len(words):
            rank, npart, njoin = words[at:at + 3]
            recs = [words[at + 3 + 32 * i:at + 3 + 32 * (i + 1)] for i in range(npart + njoin)]
            print("rank", rank, "np", npart, "nj", njoin, "kinds", [r[4 * 7 + 1] for r in recs])
            assert (npart, njoin) == (4, 4) and all(len(r) == 32 for r in recs)
            assert [r[4 * 7 + 1] for r in recs] == [3, 3, 3, 3, 1, 2, 2, 2]
            ranks.append(rank)
            at += 3 + 32 * (npart + njoin)
        assert at == len(words) and ranks == [0, 1]
        frozen = _forensics_words(m.comm, m.comm.lib.hjgpu_comm_get_frozen)
        print("frozen words", len(frozen))
        assert frozen == [] and m.comm.frozen() == []
    finally:
        m.close()
