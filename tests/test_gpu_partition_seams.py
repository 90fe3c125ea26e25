"""GPU tests of the partition operators on both sides of every change of K6's geometry (hj_scatter_config, partition_kernels.hip): packed
output takes 16 384-tuple tiles with carry up to fan-out 216, 12 288 up to 436, 8 192 up to 660 and 16 384 without carry beyond; column
output never carries.  Row counts sit on the tile's seams (T - 1, T, T + 1, 2 T + 17), and the key distributions are the ones a tile's
bookkeeping can get wrong: a hot partition on either side of CTL_NEXT_HOT's threshold, one that changes from tile to tile, runs longer
than HJ_STREAM_UNIT (the `heavy` list), sorted input, everything in the first or the last partition.  Inputs and references:
tests/operator_cases.py.  Every comparison is exact equality against numpy."""
import numpy as np
import pytest

from helpers import mulhi_hash
import operator_cases as oc

pytestmark = pytest.mark.gpu

TAIL = 64                                           # rows behind row n, which no operator may write
PATTERN64 = np.uint64(0xA5C3F00DDEADBEEF)
PATTERN32 = np.uint32(0xA5C3F00D)


def _free(*cols):
    for c in cols:
        c.free()


def check_packed(t, tail, keys, vals, off_got, fanout, own_first=0, own_count=0):
    n = len(keys)
    off, first = oc.partition_reference(keys, fanout, own_first=own_first, own_count=own_count)
    assert np.array_equal(off_got.astype(np.int64), off)                                    # d_offsets = the prefix of np.bincount
    got = mulhi_hash((t & np.uint64(oc.M32)).astype(np.uint32), oc.F_PART, fanout)
    assert np.array_equal(got, oc.expected_partition_of_rows(off, first))                   # every row where the header's rule puts its partition
    assert np.array_equal(np.sort(t), np.sort((vals.astype(np.uint64) << np.uint64(32)) | keys.astype(np.uint64)))    # the input, as a multiset
    assert (tail == PATTERN64).all()                                                        # nothing behind row n


def run_packed(hj, keys, vals, fanout, own=None, counted=None):
    """one call of a packed form; returns (tuples[:n], the TAIL rows behind them, offsets, counts2 or None)"""
    n = len(keys)
    dk, dv = hj.column(keys), hj.column(vals)
    dt = hj.column(np.full(n + TAIL, PATTERN64, np.uint64), np.uint64)
    do = hj.column(np.full(fanout + 1, PATTERN64, np.uint64), np.uint64)
    dc = None
    if counted is not None:
        fanout2 = counted
        dc = hj.column(np.full(fanout * fanout2, PATTERN64, np.uint64), np.uint64)
        hj.partition_packed_counted_async(dk, dv, n, oc.F_PART, fanout, own[0], own[1], oc.F_PART2, fanout2, dt, do, dc)
    elif own is not None:
        hj.partition_packed_own_last_async(dk, dv, n, oc.F_PART, fanout, own[0], own[1], dt, do)
    else:
        hj.partition_packed_async(dk, dv, n, oc.F_PART, fanout, dt, do)
    hj.synchronize()
    all_rows = dt.download()
    res = (all_rows[:n], all_rows[n:], do.download(), dc.download() if dc is not None else None)
    _free(dk, dv, dt, do, *([dc] if dc is not None else []))
    return res


@pytest.mark.parametrize("dist", oc.DISTRIBUTIONS)
@pytest.mark.parametrize("fanout", oc.PACKED_FANOUTS)
def test_partition_packed(hj, fanout, dist):
    tile = oc.packed_tile(fanout)
    for n in oc.seam_rows(tile):
        keys, vals = oc.partition_input(dist, n, fanout, tile)
        t, tail, off, _ = run_packed(hj, keys, vals, fanout)
        check_packed(t, tail, keys, vals, off, fanout)


@pytest.mark.parametrize("dist", oc.DISTRIBUTIONS)
@pytest.mark.parametrize("fanout", oc.PACKED_FANOUTS)
def test_partition_packed_own_last(hj, fanout, dist):
    """own ranges: first, middle, last, all, empty"""
    tile = oc.packed_tile(fanout)
    for n in oc.seam_rows(tile):
        keys, vals = oc.partition_input(dist, n, fanout, tile)
        for own in oc.own_ranges(fanout):
            t, tail, off, _ = run_packed(hj, keys, vals, fanout, own=own)
            check_packed(t, tail, keys, vals, off, fanout, *own)


@pytest.mark.parametrize("dist", oc.DISTRIBUTIONS)
@pytest.mark.parametrize("fanout,fanout2", oc.COUNTED_FANOUTS)
def test_partition_packed_counted(hj, fanout, fanout2, dist):
    """the fused second-level counts, with an own range in the middle and without one"""
    tile = oc.packed_tile(fanout)
    for n in oc.seam_rows(tile):
        keys, vals = oc.partition_input(dist, n, fanout, tile)
        want2 = oc.counts2_reference(keys, fanout, fanout2)
        for own in (oc.own_ranges(fanout)[1], (0, 0)):
            t, tail, off, counts2 = run_packed(hj, keys, vals, fanout, own=own, counted=fanout2)
            check_packed(t, tail, keys, vals, off, fanout, *own)
            assert np.array_equal(counts2, want2)                                           # d_counts2 = the two-level np.bincount


@pytest.mark.parametrize("dist", oc.DISTRIBUTIONS)
@pytest.mark.parametrize("fanout", oc.COLUMN_FANOUTS)
def test_partition_columns(hj, fanout, dist):
    tile = oc.PLAIN_TILE
    for n in oc.seam_rows(tile):
        keys, vals = oc.partition_input(dist, n, fanout, tile)
        dk, dv = hj.column(keys), hj.column(vals)
        dko, dvo = hj.column(np.full(n + TAIL, PATTERN32, np.uint32)), hj.column(np.full(n + TAIL, PATTERN32, np.uint32))
        do = hj.column(np.full(fanout + 1, PATTERN64, np.uint64), np.uint64)
        hj.partition(dk, dv, n, oc.F_PART, fanout, dko, dvo, do)
        ko, vo, off_got = dko.download(), dvo.download(), do.download()
        _free(dk, dv, dko, dvo, do)
        off, first = oc.partition_reference(keys, fanout)
        assert np.array_equal(off_got.astype(np.int64), off)
        assert np.array_equal(mulhi_hash(ko[:n], oc.F_PART, fanout), oc.expected_partition_of_rows(off, first))
        assert np.array_equal(np.sort(oc.pairs(ko[:n], vo[:n])), np.sort(oc.pairs(keys, vals)))
        assert (ko[n:] == PATTERN32).all() and (vo[n:] == PATTERN32).all()
