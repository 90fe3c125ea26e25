"""GPU tests of hjgpu_group_agg / hjgpu_group_agg_async: GROUP BY nothing, one or two uint32 columns; COUNT(*) and up to four of SUM(a),
SUM(a * b), MIN(a) and MAX(a), unsigned or - AGG_SIGNED - on int32, over the rows a bitmap in d_match_bits' layout selects (NULL: every row).

Expected values come from numpy: np.unique(keys, axis=0, return_inverse=True), np.bincount for the counts, np.add.at on uint64 / int64 for
the sums and the exact 64-bit products, np.minimum.at / np.maximum.at on uint32 / int32 for the extremes.  Everything is an exact integer:
every comparison is for equality.  The helpers are test_gpu_group_sum's: outputs longer than `capacity` behind a canary, masks followed by
all-ones words that nothing may read, mask and inputs read back unchanged, both sides sorted by tuple.  On top of them every input column
is allocated longer than n and holds 0xFFFFFFFF behind row n: a last vector that is not masked shows in a product or in a MAX.  Group
counts and row counts come from the context's counters ("group_lds_groups", "agg_step_rows", "agg_scalar_step_rows"), never hard-coded.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import HjGpuError
from test_gpu_npj_lookup import relations, outputs
from test_gpu_lookup_selected import hj, mask_words, selection, col        # noqa: F401 (hj: the fixture)
from test_gpu_group_sum import (MASKS, TAILS, MANY, CANARY32, CANARY64, ONES, lds_groups, sel_of, tuples, measures, expected, canary, by_tuple,
                                check_outputs, random_ids)

pytestmark = pytest.mark.gpu

SUM, MUL, MIN, MAX, SIGNED = H.AGG_SUM, H.AGG_SUM_MUL, H.AGG_MIN, H.AGG_MAX, H.AGG_SIGNED
I32_MIN, I32_MAX = 0x80000000, 0x7FFFFFFF          # the bit patterns
PAD = 64                                           # rows of 0xFFFFFFFF behind row n of every input column


def padded(hj, a):
    host = np.concatenate([np.asarray(a, np.uint32), np.full(PAD, ONES, np.uint32)])
    return hj.column(host), host


def want_agg(keys, aggs, sel):
    """(sorted distinct tuples [J, nkeys], counts [J], words [naggs][J] as uint64) of the selected rows; aggs: (fn, a, b or None, flags)"""
    nsel = int(sel.sum())
    if keys:
        K = np.stack([k[sel] for k in keys], axis=1)
        uniq, inv = np.unique(K, axis=0, return_inverse=True) if nsel else (K, np.zeros(0, np.int64))
        inv = inv.reshape(-1)
    else:
        uniq, inv = np.zeros((1 if nsel else 0, 0), np.uint32), np.zeros(nsel, np.int64)
    J = len(uniq)
    counts = np.bincount(inv, minlength=J).astype(np.uint64)
    words = []
    for fn, a, b, flags in aggs:
        x = a[sel].view(np.int32).astype(np.int64) if flags & SIGNED else a[sel].astype(np.uint64)
        if fn == MUL:
            x = x * (b[sel].view(np.int32).astype(np.int64) if flags & SIGNED else b[sel].astype(np.uint64))        # exact: 32 x 32 bits
        if fn in (SUM, MUL):
            w = np.zeros(J, x.dtype)
            np.add.at(w, inv, x)                                                                                       # wraps modulo 2^64
        elif fn == MIN:
            w = np.full(J, x.max() if nsel else 0, x.dtype)
            np.minimum.at(w, inv, x)
        else:
            w = np.full(J, x.min() if nsel else 0, x.dtype)
            np.maximum.at(w, inv, x)
        words.append(w.view(np.uint64) if w.dtype == np.int64 else w)
    return uniq, counts, words


def check_agg(want, J_got, capacity, kout, cout, aout, overflow, what):
    if kout:
        return check_outputs(want, J_got, capacity, kout, cout, aout, overflow, what)
    # no key column: one row at index 0, or none
    uniq, counts, words = want
    J = len(uniq)
    m = min(J_got, capacity)
    raws = ([cout.download()] if cout is not None else []) + [d.download() for d in aout]
    for c, raw in enumerate(raws):
        assert np.all(raw[m:] == CANARY64), (what, "uint64 output", c, "written at index >= min(J, capacity)")
    if overflow:
        assert capacity < J_got <= J, (what, capacity, J_got, J)
        return
    assert J_got == J and J <= 1, (what, J_got, J)
    for c, (raw, w) in enumerate(zip(raws, ([counts] if cout is not None else []) + words)):
        assert np.array_equal(raw[:J], w), (what, "scalar output", c, raw[:J], w)


def agg(hj, keys, aggs, sel, kind="null", capacity=None, counts=True, overflow=False, want=None):
    """one blocking call checked against numpy in every respect; returns the count.  aggs: (fn, a, b or None, flags), host arrays - the same
    array object in several places is one device column"""
    n = len(sel)
    want = want_agg(keys, aggs, sel) if want is None else want
    J = len(want[0])
    capacity = J if capacity is None else capacity
    words = mask_words(sel, kind) if kind != "null" else None
    dsel = hj.column(words) if words is not None else None
    made = {}

    def dev(a):
        if id(a) not in made:
            made[id(a)] = padded(hj, a)
        return made[id(a)][0]
    dk = [dev(k) for k in keys]
    dag = [(fn, dev(a), dev(b) if b is not None else None, flags) for fn, a, b, flags in aggs]
    kout = [canary(hj, capacity, np.uint32) for _ in keys]
    cout = canary(hj, capacity, np.uint64) if counts else None
    aout = [canary(hj, capacity, np.uint64) for _ in aggs]
    try:
        got = hj.group_agg(dsel, n, dk, dag, kout, aout, cout, capacity=capacity)
        assert not overflow, "HJGPU_EOVERFLOW expected"
    except HjGpuError as e:
        assert overflow and e.status == api.EOVERFLOW, str(e)
        got = e.count
    print(kind, "n", n, "nkeys", len(keys), "aggs", [(a[0], a[3]) for a in aggs], "capacity", capacity, "count", got, "want", J)
    check_agg(want, got, capacity, kout, cout, aout, overflow, (kind, n, len(keys)))
    if words is not None:
        assert np.array_equal(dsel.download(), words), "the mask was written"
    for d, host in made.values():
        assert np.array_equal(d.download(), host), "an input column was written"
        d.free()
    for d in ([dsel] if dsel is not None else []) + kout + aout + ([cout] if counts else []):
        d.free()
    return got


def values(n, seed):
    return np.random.default_rng(seed + 2000).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def all_four(a, b, flip=0):
    """SUM, SUM(a * b), MIN and MAX in one call, two of them signed"""
    return [(SUM, a, None, flip), (MUL, a, b, flip ^ SIGNED), (MIN, a, None, flip ^ SIGNED), (MAX, b, None, flip)]


@pytest.mark.parametrize("nkeys", [0, 1, 2])
@pytest.mark.parametrize("kind", MASKS)
def test_tails(hj, kind, nkeys):
    """the partial vector, the partial word, garbage bits at >= n, no row at all - with 0xFFFFFFFF behind row n of every column"""
    for n in TAILS:
        keys = tuples(random_ids(n, 7, seed=n), nkeys) if nkeys else []
        agg(hj, keys, all_four(values(n, n), values(n, n + 1), flip=n & 1), sel_of(kind, n, seed=n + 3), kind)


@pytest.mark.parametrize("nkeys", [1, 2])
def test_extremes_against_zero_initialisation(hj, nkeys):
    """the tables start as 0: a MAX whose only value is 0, a MIN whose only value is 0xFFFFFFFF, and the signed edges - each as a group
    of one row and all of them in one group; the tuple-0 group with every function"""
    edge = np.array([I32_MIN, 0xFFFFFFFF, 0, I32_MAX], np.uint32)              # INT32_MIN, -1, 0, INT32_MAX
    # ids 0 ... 3: one row each, the edge values in turn (id 0 is the tuple 0); id 4: all four mixed; ids 5, 6: only 0s, only 0xFFFFFFFFs
    ids = np.array([0, 1, 2, 3, 4, 4, 4, 4, 5, 5, 5, 6, 6, 6])
    a = np.concatenate([edge, edge, np.zeros(3, np.uint32), np.full(3, ONES, np.uint32)])
    for rot in range(4):                                                        # every edge value in the tuple-0 group in turn
        ar = a.copy()
        ar[:4] = np.roll(edge, rot)
        ar[4:8] = np.roll(edge, rot)
        for flags in (0, SIGNED):
            aggs = [(MIN, ar, None, flags), (MAX, ar, None, flags), (SUM, ar, None, flags), (MUL, ar, ar, flags)]
            sel = np.ones(len(ids), bool)
            assert agg(hj, tuples(ids, nkeys), aggs, sel) == 7
            assert agg(hj, tuples(ids, nkeys), aggs, sel, "ones") == 7
    # the tuple 0 alone, many rows
    n = 10_001
    x, y = values(n, 5), values(n, 6)
    zero = [np.zeros(n, np.uint32)] * nkeys
    for flip in (0, SIGNED):
        assert agg(hj, zero, all_four(x, y, flip), sel_of("half", n, 3), "half") == 1


def test_scalar_extremes(hj):
    edge = np.array([I32_MIN, 0xFFFFFFFF, 0, I32_MAX], np.uint32)
    for flags in (0, SIGNED):
        for v in edge:
            one = np.full(5, v, np.uint32)
            assert agg(hj, [], [(MIN, one, None, flags), (MAX, one, None, flags), (SUM, one, None, flags), (MUL, one, one, flags)], np.ones(5, bool)) == 1
        assert agg(hj, [], [(MIN, edge, None, flags), (MAX, edge, None, flags)], np.ones(4, bool)) == 1
    assert agg(hj, [], [(MIN, edge, None, 0)], np.zeros(4, bool), "zeros") == 0
    assert agg(hj, [], [], np.ones(4, bool)) == 1                                # the count alone
    assert agg(hj, [], [], np.ones(4099, bool), "ones", counts=False) == 1       # nothing but J


@pytest.mark.parametrize("shape", ["constant_over_the_lane", "rows_0_2_and_1_3"])
def test_the_fold(hj, shape):
    """a lane's four rows share a tuple, the group's extremes at each of the four positions in turn; rows 0 and 2 share one tuple and
    rows 1 and 3 another"""
    n = 4099
    i = np.arange(n, dtype=np.uint64)
    ids = i // 4 if shape == "constant_over_the_lane" else (i // 4) * 2 + (i & 1)
    for pos in range(4):
        for flags in (0, SIGNED):
            a = (values(n, pos) >> 2) + 0x20000000                              # unsigned and signed: strictly inside the range
            hi, lo = (0xFFFFFFF0, 3) if not flags else (0x7FFFFFF0, 0x80000003)
            a[(i & 3) == pos] = hi
            a[(i & 3) == ((pos + 1) & 3)] = lo
            if shape == "rows_0_2_and_1_3":                                     # each pair has its own extremes
                a[(i & 3) == ((pos + 2) & 3)] = hi - 1
                a[(i & 3) == ((pos + 3) & 3)] = lo + 1
            b = values(n, pos + 9)
            aggs = [(MIN, a, None, flags), (MAX, a, None, flags), (MUL, a, b, flags), (SUM, b, None, flags)]
            for kind in ("null", "half"):
                for nkeys in (1, 2):
                    keys = [ids.astype(np.uint32)] + ([np.full(n, 7, np.uint32)] if nkeys == 2 else [])
                    agg(hj, keys, aggs, sel_of(kind, n, seed=6), kind)


def test_products(hj):
    # 0xFFFFFFFF squared over three rows of one group passes 2^64
    big = np.full(3, ONES, np.uint32)
    for keys in ([], [np.zeros(3, np.uint32)], [np.full(3, 9, np.uint32), np.full(3, 9, np.uint32)]):
        want = want_agg(keys, [(MUL, big, big, 0)], np.ones(3, bool))
        assert int(want[2][0][0]) == (3 * 0xFFFFFFFF * 0xFFFFFFFF) % (1 << 64) < 0xFFFFFFFF * 0xFFFFFFFF
        agg(hj, keys, [(MUL, big, big.copy(), 0)], np.ones(3, bool), want=want)
        agg(hj, keys, [(MUL, big, big, 0)], np.ones(3, bool), want=want)        # d_a == d_b
    # signed: INT32_MIN squared, products of mixed sign
    a = np.array([I32_MIN, I32_MIN, I32_MAX, 0xFFFFFFFF, 5, 0xFFFFFFFB, 0, I32_MIN], np.uint32)
    b = np.array([I32_MIN, I32_MAX, I32_MIN, I32_MIN, 0xFFFFFFF9, 0xFFFFFFFD, I32_MIN, 1], np.uint32)
    ids = np.array([0, 1, 1, 2, 2, 3, 3, 0])
    want = want_agg([], [(MUL, a[:1], b[:1], SIGNED)], np.ones(1, bool))
    assert int(want[2][0][0]) == 1 << 62
    for nkeys in (0, 1, 2):
        keys = tuples(ids, nkeys) if nkeys else []
        for flags in (SIGNED, 0):
            agg(hj, keys, [(MUL, a, b, flags), (MUL, b, a, flags), (MUL, a, a, flags)], np.ones(len(a), bool))
    # one column in two aggregates and as a key; a sum of squares over many rows
    n = 20_011
    k = tuples(random_ids(n, 33, seed=31), 1)[0]
    v = values(n, 32)
    sel = selection("half", n, seed=33)
    assert agg(hj, [k, k], [(MUL, k, k, 0), (MAX, k, None, SIGNED), (MUL, v, k, SIGNED), (MIN, v, None, 0)], sel, "half") == 33
    assert agg(hj, [k], [(SUM, k, None, SIGNED), (SUM, k, None, 0), (MUL, v, v, 0), (MUL, v, v, SIGNED)], sel, "half") == 33
    agg(hj, [], [(MUL, v, v, 0), (MUL, v, v, SIGNED), (SUM, v, None, 0), (SUM, v, None, SIGNED)], sel, "half")


@pytest.mark.parametrize("nkeys", [1, 2])
def test_table_roads(hj, nkeys):
    """G - 1, G + 1 and 2 G + 3 groups: a tuple lives in several workgroups' LDS tables and in the merge table, and rows go to either
    directly - the combine is right on every path"""
    G = lds_groups(hj)
    a, b = values(MANY, 1), values(MANY, 2)
    for groups in (G - 1, G + 1, 2 * G + 3):
        for cyclic in (False, True):
            ids = np.arange(MANY) % groups if cyclic else random_ids(MANY, groups, seed=groups)
            kind = "null" if cyclic else "half"
            aggs = [(MIN, a, None, SIGNED if cyclic else 0), (MAX, a, None, 0 if cyclic else SIGNED), (MUL, a, b, SIGNED if cyclic else 0), (MAX, b, None, 0)]
            assert agg(hj, tuples(ids, nkeys), aggs, sel_of(kind, MANY, seed=5), kind) == groups


def test_the_loops_iterate(hj):
    """one step of the whole grid plus 37 rows, on each road"""
    for counter, nkeys in (("agg_step_rows", 1), ("agg_scalar_step_rows", 0)):
        n = hj.counter(counter) + 37
        assert 37 < n <= 1 << 23, (counter, n)
        a, b = values(n, 7), values(n, 8)
        keys = tuples(random_ids(n, 1000, seed=11), 1) if nkeys else []
        for kind in ("half", "null"):
            agg(hj, keys, all_four(a, b, flip=SIGNED), sel_of(kind, n, seed=13), kind)


@pytest.mark.parametrize("nkeys", [1, 2])
@pytest.mark.parametrize("nvals", [0, 1, 2, 3, 4])
def test_unsigned_sums_agree_with_group_sum(hj, nkeys, nvals):
    n = 50_021
    keys, vals = tuples(random_ids(n, 300, seed=nvals), nkeys), measures(n, nvals, seed=nvals + 1)
    dk, dv = [hj.column(k) for k in keys], [hj.column(v) for v in vals]
    for kind in ("null", "half", "eighth"):
        sel = sel_of(kind, n, seed=7)
        dsel = hj.column(mask_words(sel, kind)) if kind != "null" else None
        rows = []
        for call in ("group_sum", "group_agg"):
            kout = [canary(hj, 300, np.uint32) for _ in keys]
            sout, cout = [canary(hj, 300, np.uint64) for _ in vals], canary(hj, 300, np.uint64)
            if call == "group_sum":
                J = hj.group_sum(dsel, n, dk, dv, kout, sout, cout, capacity=300)
            else:
                J = hj.group_agg(dsel, n, dk, [(SUM, d) for d in dv], kout, sout, cout, capacity=300)
            got = [d.download() for d in kout + [cout] + sout]
            order = by_tuple([g[:J] for g in got[:nkeys]])
            rows.append((J, [g[:J][order] for g in got], [g[J:] for g in got]))
        assert rows[0][0] == rows[1][0] == len(expected(keys, vals, sel)[0])
        for x, y in zip(rows[0][1] + rows[0][2], rows[1][1] + rows[1][2]):
            assert np.array_equal(x, y), (kind, nkeys, nvals)


def test_overflow(hj):
    G = lds_groups(hj)
    n = 50_003
    groups = 2 * G + 5
    keys, a, b = tuples(random_ids(n, groups, seed=41), 2), values(n, 42), values(n, 43)
    aggs = all_four(a, b)
    sel = np.ones(n, bool)
    want = want_agg(keys, aggs, sel)
    J = len(want[0])
    assert J == groups
    agg(hj, keys, aggs, sel, capacity=J, want=want)
    agg(hj, keys, aggs, sel, capacity=J - 1, overflow=True, want=want)
    agg(hj, keys, aggs, sel, capacity=0, overflow=True, want=want)
    agg(hj, keys, aggs, sel, capacity=1 << 20, want=want)
    assert agg(hj, keys, aggs, np.zeros(n, bool), "zeros", capacity=0) == 0
    # no key column: capacity 0 is an overflow as soon as one row is selected
    agg(hj, [], aggs, sel, capacity=0, overflow=True)
    agg(hj, [], aggs, selection("last_row", n, 0), "last_row", capacity=0, overflow=True)
    assert agg(hj, [], aggs, np.zeros(n, bool), "zeros", capacity=0) == 0
    assert agg(hj, [], aggs, sel, capacity=5) == 1


def test_refusals_name_the_aggregate(hj):
    """each returns before anything is enqueued: the canaries are untouched afterwards (the whole table of refusals: test_group_agg_checks)"""
    import torch
    n = 1000
    da, _ = padded(hj, values(n, 1))
    db, _ = padded(hj, values(n, 2))
    kout, aout, cout = [canary(hj, n, np.uint32)], [canary(hj, n, np.uint64), canary(hj, n, np.uint64)], canary(hj, n, np.uint64)
    d_count = hj.column(np.full(2, 77, np.uint64), np.uint64)
    good = [(SUM, da), (MUL, da, db, SIGNED)]

    def blocking(aggs=good, ki=[da], ko=kout, ao=aout, stream=None, capacity=n):
        return hj.group_agg(None, n, ki, aggs, ko, ao, cout, capacity=capacity, stream=stream)

    def enqueue(aggs=good, ki=[da], ko=kout, ao=aout, stream=None, capacity=n, count=d_count):
        return hj.group_agg_async(None, n, ki, aggs, ko, ao, cout, capacity, count, stream=stream)

    for call in (blocking, enqueue):
        cases = [("fn 4", dict(aggs=[good[0], (4, da)]), api.EINVAL, "aggregate 1"),
                 ("an unknown flag", dict(aggs=[(SUM, da, None, 2), good[1]]), api.EINVAL, "aggregate 0"),
                 ("null d_a", dict(aggs=[good[0], (MUL, None, db)]), api.EINVAL, "aggregate 1"),
                 ("null d_b under SUM_MUL", dict(aggs=[(MUL, da), good[1]]), api.EINVAL, "aggregate 0"),
                 ("d_b under MAX", dict(aggs=[good[0], (MAX, da, db)]), api.EINVAL, "aggregate 1"),
                 ("five aggregates", dict(aggs=[good[0]] * 5, ao=aout * 2 + aout[:1]), api.EINVAL, "naggs"),
                 ("three keys", dict(ki=[da] * 3, ko=kout * 3), api.EINVAL, "nkeys"),
                 ("misaligned d_b", dict(aggs=[good[0], (MUL, da, db.ptr + 4)]), api.EALIGN, "aligned"),
                 ("an output over d_b", dict(ao=[aout[0], db.ptr + 16]), api.EINVAL, "overlaps"),
                 ("capacity beyond 2^40", dict(capacity=(1 << 40) + 1), api.EINVAL, "capacity")]
        if call is enqueue:
            cases += [("misaligned d_ngroups", dict(count=d_count.ptr + 4), api.EALIGN, "d_ngroups"),
                      ("d_ngroups inside an output", dict(count=cout.ptr + 8), api.EINVAL, "overlaps")]
        for name, kw, status, text in cases:
            with pytest.raises(HjGpuError) as e:
                call(**kw)
            assert e.value.status == status and text in str(e.value), (name, str(e.value))
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(HjGpuError) as e:
                    call(stream=s.cuda_stream)
                assert e.value.status == api.EINVAL and "capturing" in str(e.value)
            finally:
                g.capture_end()
        s.synchronize()
    hj.synchronize()
    assert np.all(kout[0].download() == CANARY32) and all(np.all(d.download() == CANARY64) for d in aout + [cout]), "a refused call wrote an output"
    assert [int(x) for x in d_count.download()] == [77, 77]
    # n == 0 accepts NULL everywhere else
    assert hj.group_agg(None, 0, [], [], [], [], None, capacity=0) == 0
    hj.group_agg_async(None, 0, [None, None], [], [None, None], [], None, 5, d_count)
    hj.synchronize()
    assert int(d_count.download()[0]) == 0
    assert blocking() == len(np.unique(values(n, 1)))


def test_enqueue_only(hj):
    """two calls with different functions and capacities back to back on one stream, then a hjgpu_group_sum_async, no host wait in
    between; the status of the join before them stays what it was"""
    ik, iv, ok = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0                                                      # the preceding join's status: HJGPU_EZEROKEY
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    dv, db = outputs(hj, len(ok), "both")
    d_res = hj.column(4, np.uint64)
    hj.reserve(len(ik), len(ok))
    hj.npj_lookup_async(rk, rv, len(ik), sk, len(ok), None, dv, db, d_res)
    runs = []
    for n, kind, nkeys, groups, capacity, which in ((70_013, "half", 2, 300, 300, "agg"), (20_001, "eighth", 0, 1, 6000, "agg"), (4099, "null", 1, 9, 5, "sum")):
        sel = sel_of(kind, n, seed=n)
        keys = tuples(random_ids(n, groups, seed=n + 1), nkeys) if nkeys else []
        a, b = values(n, n + 2), values(n, n + 3)
        aggs = [(MIN, a, None, SIGNED), (MUL, a, b, 0), (MAX, b, None, 0)] if nkeys == 2 else [(MUL, a, b, SIGNED), (SUM, a, None, SIGNED), (MIN, b, None, 0), (MAX, a, None, SIGNED)]
        if which == "sum":
            aggs = [(SUM, a, None, 0)]
        dcol = {id(x): padded(hj, x)[0] for x in keys + [a, b]}
        runs.append(dict(n=n, sel=sel, keys=keys, aggs=aggs, capacity=capacity, which=which,
                         dsel=hj.column(mask_words(sel, kind)) if kind != "null" else None, dk=[dcol[id(k)] for k in keys],
                         dag=[(fn, dcol[id(x)], dcol[id(y)] if y is not None else None, fl) for fn, x, y, fl in aggs],
                         kout=[canary(hj, capacity, np.uint32) for _ in keys], aout=[canary(hj, capacity, np.uint64) for _ in aggs],
                         cout=canary(hj, capacity, np.uint64), d_count=hj.column(np.full(1, 77, np.uint64), np.uint64)))
    # (the workspace for the largest capacity first: growing it between the enqueues would wait for the device)
    hj.group_agg(None, 0, [], [], [], [], None, capacity=6000)
    for r in runs:
        if r["which"] == "agg":
            hj.group_agg_async(r["dsel"], r["n"], r["dk"], r["dag"], r["kout"], r["aout"], r["cout"], r["capacity"], r["d_count"])
        else:
            hj.group_sum_async(r["dsel"], r["n"], r["dk"], [x[1] for x in r["dag"]], r["kout"], r["aout"], r["cout"], r["capacity"], r["d_count"])
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()                                        # waits for the stream
    assert e.value.status == api.EZEROKEY
    for r in runs:
        want = want_agg(r["keys"], r["aggs"], r["sel"])
        got = int(r["d_count"].download()[0])
        check_agg(want, got, r["capacity"], r["kout"], r["cout"], r["aout"], got > r["capacity"], (r["n"], r["which"]))
    assert [int(r["d_count"].download()[0]) for r in runs] == [300, 1, 9]      # the last: the caller's comparison with capacity (5), an overflow


def test_stats(hj):
    for nkeys in (2, 0):
        n = hj.counter("agg_step_rows") + 37
        keys = tuples(random_ids(n, 100, seed=3), 2) if nkeys else []
        agg(hj, keys, all_four(values(n, 4), values(n, 5)), selection("half", n, seed=5), "half")
        s = hj.stats()
        print(s)
        assert s["ms_total"] > 0 and s["ms_histogram"] > 0 and s["ms_join"] > 0 and s["ms_close_gaps"] > 0, s
        assert s["ms_total"] >= (s["ms_histogram"] + s["ms_join"] + s["ms_close_gaps"]) * (1 - 1e-5), s
        for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_build", "ms_inner_wait"):
            assert s[k] == 0, (k, s)
        assert s["fanout1"] == 0 and s["fanout2"] == 0 and s["buckets"] == 0 and s["groups"] == 0, s
