"""Host model of option "audit" (test infrastructure, numpy only): what a stage record of include/hjgpu.h's hjgpu_audit_read must
hold for given relations.  Written from the header and the comments of csrc/audit_kernels.hip: a stage is
{tuples lying in a partition their key does not hash to, sum of keys, sum of payloads, tuples}, every word a uint64 that wraps."""
import numpy as np

from helpers import mulhi_hash

MASK = (1 << 64) - 1
STAGES = 8
ZERO = [0, 0, 0, 0]


def sums(keys, vals, start=None):
    """(0, sum of keys, sum of payloads, rows) mod 2^64, added to the stage `start` when one is given.  Partitioning permutes the rows
    of a relation, so this is what every filled stage of it holds."""
    keys, vals = np.asarray(keys), np.asarray(vals)
    assert keys.shape == vals.shape
    got = [0, int(keys.astype(np.uint64).sum(dtype=np.uint64)), int(vals.astype(np.uint64).sum(dtype=np.uint64)), int(keys.size)]
    if start is not None:
        got = [(a + int(b)) & MASK for a, b in zip(got, start)]
    return tuple(got)


def unpack(tuples):
    """(keys, payloads) of packed tuples (payload << 32 | key)"""
    tuples = np.asarray(tuples, dtype=np.uint64)
    return (tuples & np.uint64(0xFFFFFFFF)).astype(np.uint32), (tuples >> np.uint64(32)).astype(np.uint32)


def partition_of(keys, f1, F1, p1_base, f2, F2):
    """the final partition of a key under a plan of two hashes: (H(k, f1, F1) - p1_base) * F2 + H(k, f2, F2), in 32-bit unsigned arithmetic"""
    keys = np.asarray(keys, dtype=np.uint32)
    p = (mulhi_hash(keys, f1, F1) - int(p1_base)) * int(F2) + mulhi_hash(keys, f2, F2)
    return p & 0xFFFFFFFF


def misplaced(tuples, beg, end, hash, modulo):
    """rows of the partitions q = [beg[q], end[q]) of `tuples` whose key does not hash to q % modulo; hash = (f1, F1, p1_base, f2, F2)"""
    keys, _ = unpack(tuples)
    bad = 0
    for q, (b, e) in enumerate(zip(beg, end)):
        b, e = int(b), int(e)
        if e > b:
            bad += int(np.count_nonzero(partition_of(keys[b:e], *hash) != q % modulo))
    return bad


def stage_of(tuples, beg, end, hash, modulo):
    """the whole stage of a partitioned array: misplaced rows, then the sums over the rows the partitions span"""
    keys, vals = unpack(tuples)
    rows = np.concatenate([np.arange(int(b), int(e)) for b, e in zip(beg, end)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return (misplaced(tuples, beg, end, hash, modulo),) + sums(keys[rows], vals[rows])[1:]


def own_last_bounds(prefix, own_first, own_count, n):
    """first and last (exclusive) row of every partition in the layout of hjgpu_partition_packed_own_last_async, from the plain prefix
    of the counts (the header's three lines): partitions [own_first, own_first + own_count) end the n rows, the others close up"""
    prefix = np.asarray(prefix, dtype=np.int64)
    fanout = len(prefix) - 1
    own_rows = prefix[own_first + own_count] - prefix[own_first]
    first = np.empty(fanout, np.int64)
    for p in range(fanout):
        if p < own_first:
            first[p] = prefix[p]
        elif p < own_first + own_count:
            first[p] = n - own_rows + prefix[p] - prefix[own_first]
        else:
            first[p] = prefix[p] - own_rows
    return first, first + np.diff(prefix)


def record(seq, kind, build_rows, probe_rows, stages=None):
    """a whole record: `stages` maps a stage number to its four words, every other stage of 0-6 is zero, stage 7 is the call's"""
    rec = [list(ZERO) for _ in range(STAGES)]
    for s, words in (stages or {}).items():
        assert 0 <= s < STAGES - 1
        rec[s] = [int(w) & MASK for w in words]
    rec[STAGES - 1] = [int(seq), int(kind), int(build_rows), int(probe_rows)]
    return rec


def add_words(*stages):
    """the word-wise sum of stages, mod 2^64"""
    return [sum(int(s[w]) for s in stages) & MASK for w in range(4)]
