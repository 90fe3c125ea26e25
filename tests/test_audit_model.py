"""The host model of option "audit" (tests/audit_model.py) checked on its own, without a GPU: tests/test_gpu_audit.py holds the
device's records against it, so a mistake here would clear a broken kernel or convict a sound one."""
import numpy as np
import pytest

import audit_model as M
from helpers import mulhi_hash

FA, FB = 0x9E3779B1, 0x85EBCA6B


def _partitioned(n, hash, parts, seed):
    """a relation partitioned with numpy: its rows, the packed tuples sorted by partition, and the partitions' bounds.  With a first
    partition (hash[2]) the relation is what a receiver owns: the rows whose first hash falls into its `parts / F2` partitions."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    keys[:2] = (0, 0xFFFFFFFF)
    vals = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    p1 = mulhi_hash(keys, hash[0], hash[1])
    own = (p1 >= hash[2]) & (p1 < hash[2] + parts // hash[4])
    keys, vals = keys[own], vals[own]
    p = M.partition_of(keys, *hash)
    assert p.min() >= 0 and p.max() < parts
    order = np.argsort(p, kind="stable")
    tuples = (vals[order].astype(np.uint64) << np.uint64(32)) | keys[order].astype(np.uint64)
    beg = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=parts))]).astype(np.int64)
    return keys, vals, tuples, beg[:-1].copy(), beg[1:].copy()


@pytest.mark.parametrize("hash,parts", [((FA, 8, 0, 1, 1), 8),             # one pass
                                        ((FA, 8, 0, FB, 4), 32),           # two passes
                                        ((FA, 12, 4, FB, 5), 20)])         # pieces: partitions [4, 8) of 12, five ways each
def test_misplaced_counts_exactly_the_rows_that_were_moved(hash, parts):
    keys, vals, tuples, beg, end = _partitioned(20_011, hash, parts, seed=parts)
    assert len(keys) > 5_000
    assert M.misplaced(tuples, beg, end, hash, parts) == 0
    assert M.stage_of(tuples, beg, end, hash, parts) == M.sums(keys, vals)
    # chunked layouts list every partition once per chunk: part q holds partition q % modulo
    half = (beg + end) // 2
    beg2, end2 = np.concatenate([beg, half]), np.concatenate([half, end])
    assert M.misplaced(tuples, beg2, end2, hash, parts) == 0
    assert M.stage_of(tuples, beg2, end2, hash, parts) == M.sums(keys, vals)
    for k in (1, 3, 17):
        q = int(np.argmax(end[:-1] - beg[:-1]))           # (a partition with a right neighbour)
        assert end[q] - beg[q] >= k
        moved_end, moved_beg = end.copy(), beg.copy()
        moved_end[q] -= k; moved_beg[q + 1] -= k            # the last k rows of q now lie in its neighbour
        assert M.misplaced(tuples, moved_beg, moved_end, hash, parts) == k
        assert M.stage_of(tuples, moved_beg, moved_end, hash, parts) == (k,) + M.sums(keys, vals)[1:]
    # a partition that lost a row changes the sums and not the first word
    lost = end.copy(); lost[parts - 1] -= 1
    k_lost, v_lost = M.unpack(tuples[-1:])
    got = M.stage_of(tuples, beg, lost, hash, parts)
    assert got[0] == 0 and got[3] == len(keys) - 1
    assert got[1] == (M.sums(keys, vals)[1] - int(k_lost[0])) & M.MASK and got[2] == (M.sums(keys, vals)[2] - int(v_lost[0])) & M.MASK


@pytest.mark.parametrize("n", [0, 1, 37, 70_001])
@pytest.mark.parametrize("fanout,own_first,own_count", [(192, 48, 24), (192, 0, 96), (192, 168, 24), (8, 3, 1), (6, 0, 6), (64, 10, 0)])
def test_own_last_bounds_is_the_layout_with_the_own_partitions_at_the_end(n, fanout, own_first, own_count):
    """The layout tests/test_gpu_prepartitioned.py::test_own_partitions_last asserts of the device, built here row by row: the other
    partitions in their order, then the own ones."""
    rng = np.random.default_rng(n + fanout)
    part = np.sort(rng.integers(0, fanout, size=n))
    prefix = np.concatenate([[0], np.cumsum(np.bincount(part, minlength=fanout))]).astype(np.int64)
    own = [p for p in range(fanout) if own_first <= p < own_first + own_count]
    layout = np.concatenate([np.full(prefix[p + 1] - prefix[p], p) for p in [p for p in range(fanout) if p not in own] + own]
                            + [np.zeros(0, np.int64)]).astype(np.int64)
    first, last = M.own_last_bounds(prefix, own_first, own_count, n)
    assert len(layout) == n
    for p in range(fanout):
        assert last[p] - first[p] == prefix[p + 1] - prefix[p]
        assert 0 <= first[p] <= last[p] <= n
        assert np.all(layout[first[p]:last[p]] == p)
    # that test's own formula
    own_rows = prefix[own_first + own_count] - prefix[own_first]
    want = [prefix[p] if p < own_first else (n - own_rows + prefix[p] - prefix[own_first] if p < own_first + own_count else prefix[p] - own_rows)
            for p in range(fanout)]
    assert list(first) == [int(x) for x in want]


def test_sums_wrap_at_two_to_the_64():
    n = 1 << 20
    ones = np.full(n, 0xFFFFFFFF, np.uint32)
    plain = M.sums(ones, ones)
    assert plain == (0, n * 0xFFFFFFFF, n * 0xFFFFFFFF, n)
    # a stage that already holds almost 2^64: the sums go round, the first word and the rows add up
    start = (5, M.MASK, M.MASK - n * 0xFFFFFFFF + 1, 7)
    assert M.sums(ones, ones, start) == (5, n * 0xFFFFFFFF - 1, 0, n + 7)
    assert M.sums(ones, ones, M.sums(ones, ones)) == (0, 2 * n * 0xFFFFFFFF, 2 * n * 0xFFFFFFFF, 2 * n)
    assert M.add_words((1, M.MASK, 2, 3), (1, 1, M.MASK, 4)) == [2, 0, 1, 7]
    assert M.sums(np.zeros(0, np.uint32), np.zeros(0, np.uint32)) == (0, 0, 0, 0)


def test_partition_of_and_record():
    keys = np.array([0, 1, 0xFFFFFFFF, 12345], np.uint32)
    assert list(M.partition_of(keys, FA, 8, 0, 1, 1)) == list(mulhi_hash(keys, FA, 8))
    assert list(M.partition_of(keys, FA, 8, 0, FB, 4)) == list(mulhi_hash(keys, FA, 8) * 4 + mulhi_hash(keys, FB, 4))
    p1 = mulhi_hash(keys, FA, 12)
    assert list(M.partition_of(keys, FA, 12, 2, FB, 4)) == [int(((a - 2) * 4 + b) & 0xFFFFFFFF) for a, b in zip(p1, mulhi_hash(keys, FB, 4))]
    rec = M.record(9, 3, 37, 0, {0: (0, 1, 2, 37), 1: (0, 1, 2, 37)})
    assert rec[0] == rec[1] == [0, 1, 2, 37] and rec[2:7] == [[0, 0, 0, 0]] * 5 and rec[7] == [9, 3, 37, 0]
