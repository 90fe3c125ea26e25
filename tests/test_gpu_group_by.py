"""GPU tests of hjgpu_group_by / hjgpu_group_by_async: hjgpu_group_agg with up to four key columns.  No, one and two key columns are
hjgpu_group_agg itself; three and four take the wide tables (csrc/wide_group_layout.hpp), in which a slot has a 64-bit word per key and
insert-or-find goes through the words one compare-and-swap at a time.

Expected values come from numpy (test_gpu_group_agg.want_agg: np.unique over the key tuples, np.bincount, np.add.at, np.minimum.at /
np.maximum.at); every comparison is for equality.  The helpers are those of test_gpu_group_sum and test_gpu_group_agg.  Every call is
checked in every respect by one helper (by): canaries behind min(J, capacity) in every output, the mask - with the all-ones words behind
its last word - and every input column - with 0xFFFFFFFF behind row n - read back unchanged.  Group counts and row counts come from the
context's counters ("group_by_lds_groups", "group_by_step_rows"), never hard-coded.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import itertools

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import HjGpuError
from test_gpu_npj_lookup import relations, outputs
from test_gpu_lookup_selected import hj, mask_words, selection, col        # noqa: F401 (hj: the fixture)
from test_gpu_group_sum import TAILS, MANY, MASKS, CANARY32, CANARY64, ONES, sel_of, random_ids, canary, check_outputs, by_tuple
from test_gpu_group_agg import padded, want_agg, values, all_four, check_agg

pytestmark = pytest.mark.gpu

SUM, MUL, MIN, MAX, SIGNED = H.AGG_SUM, H.AGG_SUM_MUL, H.AGG_MIN, H.AGG_MAX, H.AGG_SIGNED
EDGE = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)
WIDE = [3, 4]


def spread(ids, nkeys):
    """nkeys key columns whose tuples are distinct exactly where the ids are: the id's digits to the bases 7, 5 (and 11), the rest in the
    last column, so that with 35 (385) groups and more every column takes more than one value.  Digit 0 is key 0 and digit 1 is key
    0xFFFFFFFF = HJGPU_NULL_VAL in every column; id 0 is the all-zero tuple"""
    ids = np.asarray(ids).astype(np.uint64)
    digits = [ids % 7, (ids // 7) % 5] + ([ids // 35] if nkeys == 3 else [(ids // 35) % 11, ids // 385])
    cols = []
    for d in digits:
        k = (d * 0x9E3779B1) & 0xFFFFFFFF
        k[d == 1] = 0xFFFFFFFF
        assert not ((k == 0xFFFFFFFF) & (d != 1)).any()
        cols.append(k.astype(np.uint32))
    return cols


def by(hj, keys, aggs, sel, kind="null", capacity=None, counts=True, overflow=False, want=None, call="group_by"):
    """one blocking call checked against numpy in every respect; returns the count.  aggs: (fn, a, b or None, flags), host arrays - the
    same array object in several places is one device column"""
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
        got = getattr(hj, call)(dsel, n, dk, dag, kout, aout, cout, capacity=capacity)
        assert not overflow, "HJGPU_EOVERFLOW expected"
    except HjGpuError as e:
        assert overflow and e.status == api.EOVERFLOW, str(e)
        got = e.count
    print(kind, "n", n, "nkeys", len(keys), "aggs", [(a[0], a[3]) for a in aggs], "capacity", capacity, "count", got, "want", J)
    check_agg(want, got, capacity, kout, cout, aout, overflow, (kind, n, len(keys)))     # (check_outputs, or its form without key columns)
    if words is not None:
        assert np.array_equal(dsel.download(), words), "the mask, or a word behind it, was written"
    for d, host in made.values():
        assert np.array_equal(d.download(), host), "an input column, or the 0xFFFFFFFF behind its row n, was written"
        d.free()
    for d in ([dsel] if dsel is not None else []) + kout + aout + ([cout] if counts else []):
        d.free()
    return got


@pytest.mark.parametrize("nkeys", WIDE)
@pytest.mark.parametrize("kind", MASKS)
def test_tails(hj, kind, nkeys):
    """the partial vector, the partial word, garbage bits at >= n, no row at all - with 0xFFFFFFFF behind row n of every column"""
    for n in TAILS:
        by(hj, spread(random_ids(n, 7, seed=n), nkeys), all_four(values(n, n), values(n, n + 1), flip=n & 1), sel_of(kind, n, seed=n + 3), kind)


@pytest.mark.parametrize("nkeys", WIDE)
def test_prefixes(hj, nkeys):
    """tuples that share every prefix: the 4^nkeys tuples of {0, 1, 0x80000000, 0xFFFFFFFF}, rows in random order and sorted by tuple;
    groups that differ in the first key only and in the last key only; the all-zero and the all-ones tuple come out as one group each"""
    n = 20_011
    combos = np.array(list(itertools.product(range(4), repeat=nkeys)))
    a, b = values(n, 1), values(n, 2)
    for order in ("random", "sorted"):
        ids = random_ids(n, len(combos), seed=nkeys)
        if order == "sorted":
            ids = np.sort(ids)
        keys = [EDGE[combos[ids, c]] for c in range(nkeys)]
        for kind in ("null", "half"):
            sel = sel_of(kind, n, seed=5)
            want = want_agg(keys, all_four(a, b), sel)
            assert len(want[0]) == 4 ** nkeys
            for edge in (0, ONES):                                  # one group each, the keys intact
                assert int((want[0] == edge).all(axis=1).sum()) == 1
            assert by(hj, keys, all_four(a, b), sel, kind, want=want) == 4 ** nkeys
    ids = random_ids(n, 300, seed=9)
    for c in (0, nkeys - 1):
        keys = [np.full(n, v, np.uint32) for v in (0, ONES, 0x80000000, 1)[:nkeys]]
        keys[c] = ((ids.astype(np.uint64) * 0x9E3779B1) & 0xFFFFFFFF).astype(np.uint32)
        assert by(hj, keys, all_four(a, b, flip=SIGNED), sel_of("half", n, seed=6), "half") == 300
    # one tuple alone, many rows: all keys 0, all keys 0xFFFFFFFF
    for v in (0, ONES):
        assert by(hj, [np.full(n, v, np.uint32)] * nkeys, all_four(a, b), sel_of("eighth", n, seed=7), "eighth") == 1


@pytest.mark.parametrize("nkeys", WIDE)
def test_table_roads(hj, nkeys):
    """G - 1, G + 1 and 2 G + 3 groups: a tuple lives in several workgroups' LDS tables and in the merge table, and rows go to either
    directly - the combine is right on every path"""
    G = hj.counter("group_by_lds_groups")
    assert 64 <= G <= 4096, G
    a, b = values(MANY, 1), values(MANY, 2)
    for groups in (G - 1, G + 1, 2 * G + 3):
        for cyclic in (False, True):
            ids = np.arange(MANY) % groups if cyclic else random_ids(MANY, groups, seed=groups)
            keys = spread(ids, nkeys)
            assert all(len(np.unique(k)) > 1 for k in keys)
            kind = "null" if cyclic else "half"
            aggs = [(MIN, a, None, SIGNED if cyclic else 0), (MAX, a, None, 0 if cyclic else SIGNED), (MUL, a, b, SIGNED if cyclic else 0), (MAX, b, None, 0)]
            assert by(hj, keys, aggs, sel_of(kind, MANY, seed=5), kind) == groups


def test_the_loop_iterates(hj):
    """one step of the whole grid plus 37 rows"""
    n = hj.counter("group_by_step_rows") + 37
    assert 37 < n <= 1 << 23, n
    a, b = values(n, 7), values(n, 8)
    ids = random_ids(n, 1000, seed=11)
    for kind, nkeys in (("half", 3), ("null", 4)):
        assert by(hj, spread(ids, nkeys), all_four(a, b, flip=SIGNED), sel_of(kind, n, seed=13), kind) == 1000


def sorted_rows(hj, call, dsel, n, dk, dag, nkeys, naggs, capacity):
    kout = [canary(hj, capacity, np.uint32) for _ in range(nkeys)]
    aout, cout = [canary(hj, capacity, np.uint64) for _ in range(naggs)], canary(hj, capacity, np.uint64)
    J = getattr(hj, call)(dsel, n, dk, dag, kout, aout, cout, capacity=capacity)
    got = [d.download() for d in kout + [cout] + aout]
    order = by_tuple([g[:J] for g in got[:nkeys]]) if nkeys else np.arange(J)
    return J, [g[:J][order] for g in got], [g[J:] for g in got]


@pytest.mark.parametrize("nkeys", WIDE)
def test_the_same_as_two_keys(hj, nkeys):
    """the further key columns constant: the sorted (keys 0 - 1, count, aggregates) are hjgpu_group_agg's over the same inputs"""
    n = 50_021
    ids = random_ids(n, 300, seed=nkeys)
    k01 = [(ids % 20).astype(np.uint32), ((ids // 20) * 0x10001).astype(np.uint32)]
    const = [np.full(n, v, np.uint32) for v in (ONES, 0)][:nkeys - 2]
    a, b = values(n, 3), values(n, 4)
    dk = [hj.column(k) for k in k01 + const]
    da, db = hj.column(a), hj.column(b)
    dag = [(SUM, da, None, SIGNED), (MUL, da, db, 0), (MIN, db, None, SIGNED), (MAX, da, None, 0)]
    for kind in ("null", "half", "eighth"):
        sel = sel_of(kind, n, seed=7)
        dsel = hj.column(mask_words(sel, kind)) if kind != "null" else None
        J2, rows2, tail2 = sorted_rows(hj, "group_agg", dsel, n, dk[:2], dag, 2, 4, 300)
        Jw, rowsw, tailw = sorted_rows(hj, "group_by", dsel, n, dk, dag, nkeys, 4, 300)
        assert J2 == Jw == len(np.unique(np.stack([k[sel] for k in k01], axis=1), axis=0))
        for c, v in enumerate(const):
            assert np.all(rowsw[2 + c] == v[0]), "a constant key column came back changed"
        for x, y in zip(rows2, rowsw[:2] + rowsw[nkeys:]):
            assert np.array_equal(x, y), (kind, nkeys)
        assert all(np.all(t == CANARY32) for t in tailw[:nkeys]) and all(np.all(t == CANARY64) for t in tailw[nkeys:])


@pytest.mark.parametrize("nkeys", [0, 1, 2])
def test_up_to_two_keys_are_group_agg(hj, nkeys):
    """the same results, the same stats mapping (and, without keys, the scalar road's J of 0 or 1)"""
    n = 50_021
    ids = random_ids(n, 300, seed=nkeys)
    keys = [(ids % 20).astype(np.uint32), (ids // 20).astype(np.uint32)][:nkeys]
    a, b = values(n, 3), values(n, 4)
    dk, da, db = [hj.column(k) for k in keys], hj.column(a), hj.column(b)
    dag = [(SUM, da, None, SIGNED), (MUL, da, db, 0), (MIN, db, None, SIGNED), (MAX, da, None, 0)]
    sel = sel_of("half", n, seed=7)
    dsel = hj.column(mask_words(sel, "half"))
    one = sorted_rows(hj, "group_agg", dsel, n, dk, dag, nkeys, 4, 300)
    s1 = hj.stats()
    two = sorted_rows(hj, "group_by", dsel, n, dk, dag, nkeys, 4, 300)
    s2 = hj.stats()
    assert one[0] == two[0] == (len(np.unique(ids[sel])) if nkeys == 2 else 20 if nkeys == 1 else 1)
    for x, y in zip(one[1] + one[2], two[1] + two[2]):
        assert np.array_equal(x, y), nkeys
    for s in (s1, s2):
        assert s["ms_total"] >= s["ms_join"] > 0 and s["ms_histogram"] > 0 and s["ms_close_gaps"] > 0, s
        assert all(s[k] == 0 for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_build", "ms_inner_wait", "fanout1", "fanout2", "buckets", "groups")), s
    by(hj, keys, all_four(a, b), sel, "half")
    # more than two keys stay refused where they were
    with pytest.raises(HjGpuError) as e:
        hj.group_agg(None, n, [da] * 3, [], [canary(hj, 8, np.uint32) for _ in range(3)], [], None, capacity=8)
    assert e.value.status == api.EINVAL and "nkeys" in str(e.value)


def test_overflow(hj):
    G = hj.counter("group_by_lds_groups")
    n = 50_003
    groups = 2 * G + 5
    a, b = values(n, 42), values(n, 43)
    aggs = all_four(a, b)
    sel = np.ones(n, bool)
    for nkeys in WIDE:
        keys = spread(random_ids(n, groups, seed=41), nkeys)
        want = want_agg(keys, aggs, sel)
        J = len(want[0])
        assert J == groups
        by(hj, keys, aggs, sel, capacity=J, want=want)
        by(hj, keys, aggs, sel, capacity=J - 1, overflow=True, want=want)
        by(hj, keys, aggs, sel, capacity=0, overflow=True, want=want)      # the merge table's minimum size is below J here
        assert by(hj, keys, aggs, np.zeros(n, bool), "zeros", capacity=0) == 0


def test_enqueue_only(hj):
    """the _async form leaves J in device memory; two calls with different nkeys (4, then 3) back to back on one stream, no host wait in
    between: the clears of the one workspace are ordered by the stream"""
    ik, iv, ok = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0                                                      # the preceding join's status: HJGPU_EZEROKEY
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    dv, db = outputs(hj, len(ok), "both")
    d_res = hj.column(4, np.uint64)
    hj.reserve(len(ik), len(ok))
    hj.npj_lookup_async(rk, rv, len(ik), sk, len(ok), None, dv, db, d_res)
    runs = []
    for n, kind, nkeys, groups, capacity in ((70_013, "half", 4, 900, 900), (20_001, "eighth", 3, 400, 900), (4099, "null", 3, 9, 5)):
        sel = sel_of(kind, n, seed=n)
        keys = spread(random_ids(n, groups, seed=n + 1), nkeys)
        a, b = values(n, n + 2), values(n, n + 3)
        aggs = [(MIN, a, None, SIGNED), (MUL, a, b, 0), (MAX, b, None, 0)] if nkeys == 4 else all_four(a, b, flip=SIGNED)
        dcol = {id(x): padded(hj, x)[0] for x in keys + [a, b]}
        runs.append(dict(n=n, sel=sel, keys=keys, aggs=aggs, capacity=capacity,
                         dsel=hj.column(mask_words(sel, kind)) if kind != "null" else None, dk=[dcol[id(k)] for k in keys],
                         dag=[(fn, dcol[id(x)], dcol[id(y)] if y is not None else None, fl) for fn, x, y, fl in aggs],
                         kout=[canary(hj, capacity, np.uint32) for _ in keys], aout=[canary(hj, capacity, np.uint64) for _ in aggs],
                         cout=canary(hj, capacity, np.uint64), d_count=hj.column(np.full(1, 77, np.uint64), np.uint64)))
    # (the workspace for the largest capacity first: growing it between the enqueues would wait for the device)
    assert hj.group_by(None, 0, [None] * 4, [], [None] * 4, [], None, capacity=900) == 0
    for r in runs:
        hj.group_by_async(r["dsel"], r["n"], r["dk"], r["dag"], r["kout"], r["aout"], r["cout"], r["capacity"], r["d_count"])
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()                                        # waits for the stream
    assert e.value.status == api.EZEROKEY
    counts = []
    for r in runs:
        want = want_agg(r["keys"], r["aggs"], r["sel"])
        got = int(r["d_count"].download()[0])
        check_outputs(want, got, r["capacity"], r["kout"], r["cout"], r["aout"], got > r["capacity"], r["n"])
        counts.append((got, len(want[0])))
    assert counts[0] == (900, 900) and counts[1][0] == counts[1][1] > 300 and counts[2] == (9, 9), counts   # the last: an overflow (capacity 5)


def test_refusals(hj):
    """each returns before anything is enqueued: the canaries are untouched afterwards, and the stats stay those of the call before"""
    import torch
    n = 1000
    words = np.concatenate([mask_words(selection("half", 16384, seed=6)), np.full(4, ONES, np.uint32)])      # room for overlapping pointers
    dsel = hj.column(words)
    h = [(np.arange(n, dtype=np.uint32) % m).astype(np.uint32) for m in (3, 5, 7, 2)]
    din = [padded(hj, x)[0] for x in h]
    da, db = padded(hj, values(n, 1))[0], padded(hj, values(n, 2))[0]
    kout, aout, cout = [canary(hj, n, np.uint32) for _ in range(5)], [canary(hj, n, np.uint64), canary(hj, n, np.uint64)], canary(hj, n, np.uint64)
    d_count = hj.column(np.full(2, 77, np.uint64), np.uint64)
    good = [(SUM, da), (MUL, da, db, SIGNED)]
    ki, ko = [d.ptr for d in din], [d.ptr for d in kout[:4]]
    sel = np.unpackbits(words[:(n + 31) // 32].view(np.uint8), bitorder="little")[:n].astype(bool)
    want = want_agg(h, [(SUM, values(n, 1), None, 0), (MUL, values(n, 1), values(n, 2), SIGNED)], sel)
    J = len(want[0])
    assert 100 < J <= 210

    def reset():
        for d in kout:
            d.upload(np.full(d.n, CANARY32, np.uint32))
        for d in aout + [cout]:
            d.upload(np.full(d.n, CANARY64, np.uint64))

    def blocking(bits=dsel.ptr, aggs=good, ki=ki, ko=ko, ao=aout, stream=None, capacity=n):
        return hj.group_by(bits, n, ki, aggs, ko, [getattr(d, "ptr", d) for d in ao], cout.ptr, capacity=capacity, stream=stream)

    def enqueue(bits=dsel.ptr, aggs=good, ki=ki, ko=ko, ao=aout, stream=None, capacity=n, count=d_count):
        return hj.group_by_async(bits, n, ki, aggs, ko, [getattr(d, "ptr", d) for d in ao], cout.ptr, capacity, count, stream=stream)

    for call in (blocking, enqueue):
        # a valid call first: the stats that every refusal must leave alone
        call()
        hj.synchronize()
        before = hj.stats()
        assert before["ms_join"] > 0
        reset()
        cases = [("five keys", dict(ki=ki + ki[:1], ko=ko + [kout[4].ptr]), api.EINVAL, "nkeys"),
                 ("a null third key", dict(ki=[ki[0], ki[1], None, ki[3]]), api.EINVAL, "null"),
                 ("a null fourth key output", dict(ko=ko[:3] + [None]), api.EINVAL, "null"),
                 ("a misaligned fourth key output", dict(ko=ko[:3] + [ko[3] + 8]), api.EALIGN, "aligned"),
                 ("a misaligned third key", dict(ki=ki[:2] + [ki[2] + 4, ki[3]]), api.EALIGN, "aligned"),
                 ("key output 2 over the mask", dict(ko=ko[:2] + [dsel.ptr + 16, ko[3]]), api.EINVAL, "overlaps"),
                 ("key output 3 over key input 2", dict(ko=ko[:3] + [ki[2] + 16]), api.EINVAL, "overlaps"),
                 ("key output 3 over key output 2", dict(ko=ko[:3] + [ko[2] + 16]), api.EINVAL, "overlaps"),
                 ("an output over d_b", dict(ao=[aout[0], db.ptr + 16]), api.EINVAL, "overlaps"),
                 ("fn 4", dict(aggs=[good[0], (4, da)]), api.EINVAL, "aggregate 1"),
                 ("d_b under MAX", dict(aggs=[(MAX, da, db), good[1]]), api.EINVAL, "aggregate 0"),
                 ("five aggregates", dict(aggs=[good[0]] * 5, ao=aout * 2 + aout[:1]), api.EINVAL, "naggs"),
                 ("capacity beyond 2^40", dict(capacity=(1 << 40) + 1), api.EINVAL, "capacity")]
        if call is enqueue:
            cases += [("misaligned d_ngroups", dict(count=d_count.ptr + 4), api.EALIGN, "d_ngroups"),
                      ("d_ngroups inside key output 3", dict(count=kout[3].ptr + 8), api.EINVAL, "overlaps")]
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
        assert hj.stats() == before, "a refused call enqueued something"
        assert all(np.all(d.download() == CANARY32) for d in kout) and all(np.all(d.download() == CANARY64) for d in aout + [cout]), "a refused call wrote an output"
        assert np.array_equal(dsel.download(), words)
    # n == 0 accepts NULL everywhere else, five keys are refused there too
    assert hj.group_by(None, 0, [None] * 4, [], [None] * 4, [], None, capacity=0) == 0
    with pytest.raises(HjGpuError) as e:
        hj.group_by(None, 0, [None] * 5, [], [None] * 5, [], None, capacity=0)
    assert e.value.status == api.EINVAL and "nkeys" in str(e.value)
    hj.group_by_async(None, 0, [None] * 3, [], [None] * 3, [], None, 5, d_count)
    hj.synchronize()
    assert int(d_count.download()[0]) == 0
    # the same pointers, accepted, and the stats are this call's
    assert blocking() == J
    check_outputs(want, J, n, kout[:4], cout, aout, False, "accepted")
    assert hj.stats()["ms_join"] > 0


def test_stats_and_counters(hj):
    G, step = hj.counter("group_by_lds_groups"), hj.counter("group_by_step_rows")
    assert G > 0 and step > 0 and step % 1024 == 0
    n = MANY
    for nkeys in WIDE:
        by(hj, spread(random_ids(n, 100, seed=3), nkeys), all_four(values(n, 4), values(n, 5)), selection("half", n, seed=5), "half")
        s = hj.stats()
        print(s)
        assert s["ms_total"] >= s["ms_join"] > 0 and s["ms_histogram"] > 0 and s["ms_close_gaps"] > 0, s
        assert s["ms_total"] >= (s["ms_histogram"] + s["ms_join"] + s["ms_close_gaps"]) * (1 - 1e-5), s
        for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_build", "ms_inner_wait"):
            assert s[k] == 0, (k, s)
        assert s["fanout1"] == 0 and s["fanout2"] == 0 and s["buckets"] == 0 and s["groups"] == 0, s


def test_the_same_column_in_every_place(hj):
    n = 4099
    k = ((random_ids(n, 33, seed=31).astype(np.uint64) * 0x9E3779B1) & 0xFFFFFFFF).astype(np.uint32)
    v = values(n, 32)
    sel = selection("half", n, seed=33)
    assert by(hj, [k, k, k, k], [(MUL, k, k, 0), (MAX, k, None, SIGNED), (MUL, v, k, SIGNED), (MIN, v, None, 0)], sel, "half") == 33
    assert by(hj, [k, v, k], [(SUM, k, None, SIGNED)], sel, "half", counts=False) == int(sel.sum())


def test_a_star_query_end_to_end(hj):
    """a filter on a fact column, three selected look-ups that narrow the one bitmap in place and whose value columns are the group keys,
    then SUM(revenue) GROUP BY (c_nation, s_nation, d_year): the same query in numpy"""
    n = 20_003
    rng = np.random.default_rng(61)
    dims = []
    for rows, attrs in ((25, 5), (25, 5), (7, 7)):
        dk = (rng.permutation(rows * 2)[:rows] + 1).astype(np.uint32)          # keys 1 ... 2 rows: half of the fact's foreign keys match
        dims.append((dk, rng.integers(0, attrs, rows).astype(np.uint32), rng.integers(1, rows * 2 + 1, n).astype(np.uint32)))
    quantity = rng.integers(0, 50, n).astype(np.uint32)
    revenue = values(n, 62)
    bits = hj.column(np.zeros((n + 31) // 32 + 4, np.uint32))
    dq = padded(hj, quantity)[0]
    passed = hj.filter_selected(None, n, [dq], [(10, 40)], bits)
    live = (quantity >= 10) & (quantity <= 40)
    assert passed == int(live.sum())
    attr_cols, want_keys = [], []
    for dk, dv, fk in dims:
        out = hj.column(np.full(n + 64, ONES, np.uint32))
        hj.lookup_selected(hj.column(dk), hj.column(dv), len(dk), padded(hj, fk)[0], n, select_bits=bits, vals_out=out, match_bits=bits)
        pos = {int(k): int(v) for k, v in zip(dk, dv)}
        hit = np.array([int(k) in pos for k in fk])
        live = live & hit
        want_keys.append(np.array([pos.get(int(k), 0xFFFFFFFF) for k in fk], np.uint32))
        attr_cols.append(out)
    want = want_agg(want_keys, [(SUM, revenue, None, 0)], live)
    J = len(want[0])
    assert 50 < J <= 175 and int(live.sum()) > 500
    kout, aout, cout = [canary(hj, J, np.uint32) for _ in range(3)], [canary(hj, J, np.uint64)], canary(hj, J, np.uint64)
    got = hj.group_by(bits, n, attr_cols, [(SUM, padded(hj, revenue)[0])], kout, aout, cout, capacity=J)
    check_outputs(want, got, J, kout, cout, aout, False, "star query")
    assert int(cout.download()[:J].sum()) == int(live.sum())
