"""GPU tests of the wide look-up (hjgpu_lookup_wide, hjgpu_lookup_wide_async): the positional look-up on two to four key columns.

Expected values come from a numpy model.  The tuples of a test are rows of a UNIVERSE of distinct tuples whose columns are drawn from a
small pool of values - 0, 1, 0x80000000 and 0xFFFFFFFF among them, so that many tuples share every one of their columns with others -; a
build side is a subset of the universe with a payload per tuple, a probe side an index column into the universe.  So hit = in_build[idx] &
selected, vals = where(hit, payload[idx], NULL), and the aggregates follow.  Every comparison is exact equality.  Both outputs are longer
than asked for and pre-filled with a canary; a mask is followed by all-ones words that nothing may read, and (where it is not the output)
comes back unchanged.

Every test takes a context of its own."""
import itertools

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import NpjParams, HjGpuError
from test_gpu_npj_lookup import outputs, read_outputs
from test_gpu_lookup_selected import (selection, pack, mask_words, MASKS, MODES, TAILS, MODE_FLAGS, EXTRA_WORDS, ONES, CANARY, NULL)

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NKEYS = [2, 3, 4]
CORNERS = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)


@pytest.fixture
def hj():
    """a context of this test's own; its device columns are all freed when the test ends (a DeviceColumn is freed only by free())"""
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    with H.HjGpu(0) as h:
        made, column = [], h.column

        def tracked(*a, **k):
            c = column(*a, **k)
            made.append(c)
            return c
        h.column = tracked
        try:
            yield h
        finally:
            for c in made:
                c.free()


def _sum(a):
    return int(a.astype(np.uint64).sum(dtype=np.uint64)) & M64


def col(hj, a):
    return hj.column(a) if len(a) else hj.column(np.zeros(4, np.uint32))


def universe(nkeys, size, seed):
    """`size` distinct tuples (size x nkeys, uint32) in random order, their columns drawn from a pool of 128 values with the corners in it"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([CORNERS, rng.integers(0, 1 << 32, 124, dtype=np.uint64).astype(np.uint32)])
    rows = np.unique(pool[rng.integers(0, len(pool), (4 * size, nkeys))], axis=0)
    assert len(rows) >= size, (len(rows), size)
    return rows[rng.permutation(len(rows))[:size]].copy()


class Sides:
    """a build side of `inner` tuples of a universe of 2 * inner (at least 16) with one payload each, uploaded once, and probe sides drawn
    from the whole universe: half of the probe tuples are present"""

    def __init__(self, hj, nkeys, inner, seed, payload=None):
        self.hj, self.nkeys, self.inner = hj, nkeys, inner
        self.rng = np.random.default_rng(seed + 1000)
        self.uni = universe(nkeys, max(2 * inner, 16), seed)
        self.in_build = np.arange(len(self.uni)) < inner
        self.pay = self.rng.integers(0, 1 << 32, len(self.uni), dtype=np.uint64).astype(np.uint32) if payload is None else payload
        order = self.rng.permutation(inner)                               # the build rows in an order of their own
        self.rk = [col(hj, self.uni[order, c]) for c in range(nkeys)]
        self.rv = col(hj, self.pay[order])

    def probe(self, outer):
        idx = self.rng.integers(0, len(self.uni), outer)
        return idx, [col(self.hj, self.uni[idx, c]) for c in range(self.nkeys)]

    def want(self, idx, sel):
        hit = self.in_build[idx] & sel
        vals = np.where(hit, self.pay[idx], NULL).astype(np.uint32)
        return hit, vals, (int(hit.sum()), _sum(self.uni[idx, 0][hit]), 0, _sum(vals[hit]))

    def call(self, sk, outer, dsel=None, dv=None, db=None, params=None):
        return tuple(self.hj.lookup_wide(self.rk, self.rv, self.inner, sk, outer, params=params, select_bits=dsel, vals_out=dv, match_bits=db))


def check(sides, outer, kind=None, mode="both", in_place=False, params=None, seed=5):
    """one blocking call against the model: the aggregates, the values, the bits, the canaries, the last word's high bits, the mask"""
    hj = sides.hj
    idx, sk = sides.probe(outer)
    sel = selection(kind, outer, seed) if kind else np.ones(outer, bool)
    words = mask_words(sel, kind) if kind else None
    dsel = hj.column(words) if kind else None
    dv, db = outputs(hj, outer, mode)
    if in_place:
        assert kind and mode in ("both", "bits")
        db = dsel
    hit, vals, agg = sides.want(idx, sel)
    got = sides.call(sk, outer, dsel, dv, db, params)
    assert got == agg, (got, agg)
    gv, gb = read_outputs(outer, dv, None if in_place else db)
    if gv is not None:
        assert np.array_equal(gv, vals)
    if in_place:
        raw = dsel.download()
        assert np.array_equal(raw[:-EXTRA_WORDS], pack(hit)) and np.all(raw[-EXTRA_WORDS:] == ONES)
    else:
        if gb is not None:
            assert np.array_equal(gb, hit)
        if kind:
            assert np.array_equal(dsel.download(), words), "the mask came back changed"
    for c in [dsel, dv, db] + sk:
        if c is not None:
            c.free()
    return hit, vals, agg


# ---- tails ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nkeys", NKEYS)
def test_tails(hj, nkeys, mode):
    sides = Sides(hj, nkeys, 1000, seed=nkeys)
    for outer in TAILS:
        hit, _, _ = check(sides, outer, mode=mode, seed=outer)
        if outer >= 255:
            assert 0 < hit.sum() < outer


# ---- masks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("nkeys", NKEYS)
def test_masks(hj, nkeys, kind):
    sides = Sides(hj, nkeys, 1000, seed=10 + nkeys)
    for outer in (1025, 4099):
        check(sides, outer, kind, seed=outer)                       # out of place: the mask comes back unchanged
        check(sides, outer, kind, in_place=True, seed=outer + 1)    # match_bits is select_bits
        check(sides, outer, kind, mode="vals", seed=outer + 2)
        check(sides, outer, kind, mode="none", seed=outer + 3)


# ---- every column counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", NKEYS)
def test_every_column_counts(hj, nkeys):
    """the tuple set {0, 1, 0x80000000, 0xFFFFFFFF}^nkeys, every other tuple in the build side (by the parity of its digits' sum, which cuts
    through every column), payloads with 0 and 0xFFFFFFFF among them, every tuple probed several times: fails when any one column is not
    compared, when 0 or HJGPU_NULL_VAL is special in any column or as a payload, or when the bit and the value disagree"""
    digits = np.array(list(itertools.product(range(4), repeat=nkeys)))
    uni = CORNERS[digits]
    inb = digits.sum(axis=1) % 2 == 0
    pay = (np.arange(len(uni), dtype=np.uint32) * np.uint32(0x9E3779B1)).astype(np.uint32)
    build = np.flatnonzero(inb)
    pay[build[0]], pay[build[1]], pay[build[2]] = 0, 0xFFFFFFFF, 1
    rng = np.random.default_rng(nkeys)
    build = build[rng.permutation(len(build))]
    rk, rv = [col(hj, uni[build, c]) for c in range(nkeys)], col(hj, pay[build])
    idx = rng.permutation(np.repeat(np.arange(len(uni)), 5))
    outer = len(idx)
    sk = [col(hj, uni[idx, c]) for c in range(nkeys)]
    dv, db = outputs(hj, outer, "both")
    got = tuple(hj.lookup_wide(rk, rv, len(build), sk, outer, vals_out=dv, match_bits=db))
    hit = inb[idx]
    vals = np.where(hit, pay[idx], NULL).astype(np.uint32)
    gv, gb = read_outputs(outer, dv, db)
    assert np.array_equal(gb, hit) and np.array_equal(gv, vals)
    assert got == (int(hit.sum()), _sum(uni[idx, 0][hit]), 0, _sum(vals[hit]))
    assert (gv[gb] == NULL).sum() == 5 and (gv[gb] == 0).sum() == 5           # a matched 0xFFFFFFFF and a matched 0, told from NULL by the bit


@pytest.mark.parametrize("nkeys", NKEYS)
def test_the_columns_are_positional(hj, nkeys):
    """(a, b, ...) against (b, a, ...): nothing matches; the same column given twice on both sides matches on its own"""
    rng = np.random.default_rng(40 + nkeys)
    a = rng.permutation(3000).astype(np.uint32)[:1500]                     # distinct values below 3000 ...
    b = a + np.uint32(100_000)                                             # ... and a second column that shares none with the first
    cols = [a, b, a ^ np.uint32(0x55), b ^ np.uint32(0xAA)][:nkeys]
    rk, rv = [col(hj, c) for c in cols], col(hj, np.arange(1500, dtype=np.uint32))
    swapped = [rk[1], rk[0]] + rk[2:]
    dv, db = outputs(hj, 1500, "both")
    assert tuple(hj.lookup_wide(rk, rv, 1500, swapped, 1500, vals_out=dv, match_bits=db)) == (0, 0, 0, 0)
    gv, gb = read_outputs(1500, dv, db)
    assert not gb.any() and np.all(gv == NULL)
    # in order, every row finds itself
    assert tuple(hj.lookup_wide(rk, rv, 1500, rk, 1500, vals_out=dv, match_bits=db)) == (1500, _sum(a), 0, _sum(np.arange(1500)))
    gv, gb = read_outputs(1500, dv, db)
    assert gb.all() and np.array_equal(gv, np.arange(1500, dtype=np.uint32))
    # the same column in every place
    same = [rk[0]] * nkeys
    assert tuple(hj.lookup_wide(same, rv, 1500, same, 1500, vals_out=dv, match_bits=db)) == (1500, _sum(a), 0, _sum(np.arange(1500)))
    assert np.array_equal(read_outputs(1500, dv, db)[0], np.arange(1500, dtype=np.uint32))


# ---- duplicates ------------------------------------------------------------------------------------------------------------------------------
def check_dups(hj, nkeys, uni, build_ids, idx, sel_kind=None):
    """build row r carries tuple build_ids[r] and payload r: the answer of a probe tuple is the number of one of its build rows, the same
    one at every position of that tuple"""
    rk, rv = [col(hj, uni[build_ids, c]) for c in range(nkeys)], col(hj, np.arange(len(build_ids), dtype=np.uint32))
    outer = len(idx)
    sk = [col(hj, uni[idx, c]) for c in range(nkeys)]
    sel = selection(sel_kind, outer, 3) if sel_kind else np.ones(outer, bool)
    dsel = hj.column(mask_words(sel, sel_kind)) if sel_kind else None
    dv, db = outputs(hj, outer, "both")
    got = tuple(hj.lookup_wide(rk, rv, len(build_ids), sk, outer, select_bits=dsel, vals_out=dv, match_bits=db))
    gv, gb = read_outputs(outer, dv, db)
    hit = np.isin(idx, build_ids) & sel
    assert np.array_equal(gb, hit) and np.all(gv[~hit] == NULL)
    assert np.all(gv[hit] < len(build_ids)) and np.array_equal(build_ids[gv[hit]], idx[hit]), "an answer is not a row of the probe tuple"
    pairs = np.unique(np.stack([idx[hit], gv[hit].astype(np.int64)], axis=1), axis=0)
    assert len(pairs) == len(np.unique(idx[hit])), "two positions of one tuple received different copies"
    assert got == (int(hit.sum()), _sum(uni[idx, 0][hit]), 0, _sum(gv[hit]))


@pytest.mark.parametrize("nkeys", NKEYS)
def test_every_build_tuple_three_times(hj, nkeys):
    uni = universe(nkeys, 2000, seed=50 + nkeys)
    rng = np.random.default_rng(60 + nkeys)
    build_ids = rng.permutation(np.repeat(np.arange(1000), 3))
    check_dups(hj, nkeys, uni, build_ids, rng.integers(0, 2000, 4099))
    check_dups(hj, nkeys, uni, build_ids, rng.integers(0, 2000, 4099), "half")


@pytest.mark.parametrize("nkeys", NKEYS)
def test_one_tuple_2000_times_among_1000_others(hj, nkeys):
    uni = universe(nkeys, 2002, seed=70 + nkeys)
    rng = np.random.default_rng(80 + nkeys)
    build_ids = rng.permutation(np.concatenate([np.arange(1000), np.full(2000, 1000)]))
    idx = rng.integers(0, 2002, 4099)
    idx[::3] = 1000                                                        # the heavy tuple at a third of the positions
    check_dups(hj, nkeys, uni, build_ids, idx)


# ---- load ------------------------------------------------------------------------------------------------------------------------------------
def slots_formula(inner, load):
    if inner == 0:
        return 0
    r = max(16, inner + 1, int(inner / (load or 0.5)))
    return (r + 7) // 8 * 8


@pytest.mark.parametrize("load", [0, 0.05, 0.99])
@pytest.mark.parametrize("nkeys", NKEYS)
def test_load(hj, nkeys, load):
    """0.99 at inner 3000: 3032 slots for 3000 rows - long walks, and wrap-around for the tuples at home near the table's end"""
    sides = Sides(hj, nkeys, 3000, seed=90 + nkeys)
    p = NpjParams(); p.load = load
    check(sides, 4099, params=p)
    assert hj.stats()["buckets"] == slots_formula(3000, load)
    check(sides, 4099, "half", in_place=True, params=p)
    s = hj.stats()
    assert s["buckets"] == slots_formula(3000, load) and s["fanout1"] == s["fanout2"] == s["groups"] == 0 and s["ms_close_gaps"] == 0
    assert s["ms_total"] > 0 and s["ms_join"] > 0 and s["ms_histogram"] > 0


def test_load_beyond_099_is_refused(hj):
    sides = Sides(hj, 2, 100, seed=99)
    _, sk = sides.probe(300)
    dv, db = outputs(hj, 300, "both")
    for load in (1.0, 0.995, 2.5):
        p = NpjParams(); p.load = load
        with pytest.raises(HjGpuError) as e:
            sides.call(sk, 300, None, dv, db, p)
        assert e.value.status == api.EINVAL and "load" in str(e.value), str(e.value)
    assert np.all(dv.download() == CANARY) and np.all(db.download() == CANARY)


# ---- more than one loop iteration ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, "half"])
@pytest.mark.parametrize("nkeys", [2, 4])
def test_more_than_one_loop_iteration(hj, nkeys, kind):
    step = hj.counter("lookup_wide_step_rows")
    assert step > 0 and step % 2048 == 0
    sides = Sides(hj, nkeys, 1000, seed=110 + nkeys)
    check(sides, 2 * step + 257, kind)


# ---- empty sides -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", NKEYS)
def test_no_build_rows(hj, nkeys):
    """inner == 0: all NULL, all bits 0, count 0 - with a mask, in place, and with NULL where nothing is read"""
    sides = Sides(hj, nkeys, 0, seed=120 + nkeys)
    for outer in (1, 777, 4099):
        hit, vals, agg = check(sides, outer, "half")
        assert agg == (0, 0, 0, 0) and np.all(vals == NULL) and not hit.any()
        check(sides, outer, "half", in_place=True)
        check(sides, outer)
    assert hj.stats()["buckets"] == 0
    dv, db = outputs(hj, 777, "both")
    assert tuple(hj.lookup_wide([None] * nkeys, None, 0, [None] * nkeys, 777, vals_out=dv, match_bits=db)) == (0, 0, 0, 0)
    gv, gb = read_outputs(777, dv, db)
    assert np.all(gv == NULL) and not gb.any()


@pytest.mark.parametrize("inner", [0, 1000])
def test_no_probe_rows(hj, inner):
    """outer == 0: nothing is written, nothing is read - not of the mask (the buffer holds no mask word at all), not of any column"""
    sides = Sides(hj, 3, inner, seed=130)
    dsel = hj.column(np.full(EXTRA_WORDS, ONES, np.uint32))
    dv, db = outputs(hj, 0, "both")
    _, sk = sides.probe(0)
    assert sides.call(sk, 0, dsel, dv, db) == (0, 0, 0, 0)
    read_outputs(0, dv, db)
    assert sides.call(sk, 0, dsel, dv, dsel) == (0, 0, 0, 0)
    assert np.all(dsel.download() == ONES)
    assert tuple(hj.lookup_wide([None] * 3, None, inner, [None] * 3, 0)) == (0, 0, 0, 0)
    d_res = hj.column(np.full(4, 7, np.uint64), np.uint64)
    hj.lookup_wide_async([None] * 3, None, inner, [None] * 3, 0, None, None, None, None, d_res)
    hj.synchronize()
    assert [int(x) for x in d_res.download()] == [0, 0, 0, 0]


# ---- refusals that need a context ----------------------------------------------------------------------------------------------------------------
def test_refusals(hj):
    sides = Sides(hj, 3, 100, seed=140)
    idx, sk = sides.probe(300)
    sel = selection("half", 300, 1)
    words = mask_words(sel)
    dsel = hj.column(words)
    dv, db = outputs(hj, 300, "both")
    d_res = hj.column(4, np.uint64)
    reserved = hj.stats()["ms_reserve"]
    # every join-mode flag, by name, in both forms
    for name, flag in MODE_FLAGS:
        p = NpjParams(); p.flags = flag
        with pytest.raises(HjGpuError) as e:
            sides.call(sk, 300, dsel, dv, db, p)
        assert e.value.status == api.EINVAL and name in str(e.value) and "hjgpu_lookup_wide" in str(e.value), (name, str(e.value))
        with pytest.raises(HjGpuError) as e:
            hj.lookup_wide_async(sides.rk, sides.rv, 100, sk, 300, p, dsel, dv, db, d_res)
        assert e.value.status == api.EINVAL and name in str(e.value) and "hjgpu_lookup_wide_async" in str(e.value), (name, str(e.value))
    # nkeys 1 and 5 through the binding
    with pytest.raises(HjGpuError) as e:
        hj.lookup_wide(sides.rk[:1], sides.rv, 100, sk[:1], 300, vals_out=dv)
    assert e.value.status == api.EINVAL and "nkeys" in str(e.value) and "hjgpu_lookup_selected" in str(e.value), str(e.value)
    with pytest.raises(HjGpuError) as e:
        hj.lookup_wide(sides.rk + sides.rk[:2], sides.rv, 100, sk + sk[:2], 300, vals_out=dv)
    assert e.value.status == api.EINVAL and "nkeys" in str(e.value), str(e.value)
    # an overlap and an alignment
    with pytest.raises(HjGpuError) as e:
        sides.call(sk, 300, dsel, dv, dsel.ptr + 16)
    assert e.value.status == api.EINVAL and "overlap" in str(e.value), str(e.value)
    with pytest.raises(HjGpuError) as e:
        sides.call(sk, 300, dsel, dv.ptr + 4, db)
    assert e.value.status == api.EALIGN
    # a refused call writes nothing and leaves no workspace behind
    assert np.all(dv.download() == CANARY) and np.all(db.download() == CANARY) and np.array_equal(dsel.download(), words)
    assert hj.stats()["ms_reserve"] == reserved
    # HJGPU_FLAG_UNIQUE and a factor are accepted and change nothing
    p = NpjParams(); p.flags = api.FLAG_UNIQUE; p.factor = 12345
    assert sides.call(sk, 300, dsel, dv, db, p) == sides.want(idx, sel)[2] == sides.call(sk, 300, dsel, dv, db)
    assert hj.stats()["ms_reserve"] > reserved                            # the workspace of its own, counted


def test_unknown_counter_names_the_new_one(hj):
    with pytest.raises(HjGpuError) as e:
        hj.counter("no_such_counter")
    assert "lookup_wide_step_rows" in str(e.value)


# ---- async -----------------------------------------------------------------------------------------------------------------------------------
def test_async_form(hj):
    """d_result in device memory equals the blocking result; two calls of different sizes (and key counts) back to back on one stream
    without a host synchronisation in between, the second one in place and with a larger table than the context has seen; what
    hjgpu_get_async_status reports - here the HJGPU_EZEROKEY of an earlier selected look-up - is what it reported before"""
    a, b = Sides(hj, 2, 1500, seed=150), Sides(hj, 4, 6000, seed=151)
    ia, ska = a.probe(9001)
    ib, skb = b.probe(7003)
    sela, selb = selection("half", 9001, 1), selection("eighth", 7003, 2)
    dsa, dsb = hj.column(mask_words(sela)), hj.column(mask_words(selb))
    (dva, dba), (dvb, _) = outputs(hj, 9001, "both"), outputs(hj, 7003, "vals")
    # an earlier enqueue-only look-up whose build side holds key 0
    zk = np.arange(500, dtype=np.uint32)
    zrk, zsk, zres = col(hj, zk), col(hj, zk), hj.column(4, np.uint64)
    hj.lookup_selected_async(zrk, zrk, 500, zsk, 500, None, None, None, None, zres)
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()
    assert e.value.status == api.EZEROKEY
    blocking = a.call(ska, 9001, dsa)
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()
    assert e.value.status == api.EZEROKEY
    ra, rb = hj.column(np.full(4, 9, np.uint64), np.uint64), hj.column(np.full(4, 9, np.uint64), np.uint64)
    hj.lookup_wide_async(a.rk, a.rv, a.inner, ska, 9001, None, dsa, dva, dba, ra)
    hj.lookup_wide_async(b.rk, b.rv, b.inner, skb, 7003, None, dsb, dvb, dsb, rb)
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()
    assert e.value.status == api.EZEROKEY
    hj.synchronize()
    hit_a, vals_a, agg_a = a.want(ia, sela)
    hit_b, vals_b, agg_b = b.want(ib, selb)
    gva, gba = read_outputs(9001, dva, dba)
    gvb, _ = read_outputs(7003, dvb, None)
    assert tuple(int(x) for x in ra.download()) == agg_a == blocking
    assert tuple(int(x) for x in rb.download()) == agg_b
    assert np.array_equal(gva, vals_a) and np.array_equal(gba, hit_a) and np.array_equal(gvb, vals_b)
    got = dsb.download()
    assert np.array_equal(got[:-EXTRA_WORDS], pack(hit_b)) and np.all(got[-EXTRA_WORDS:] == ONES)
    # d_result NULL: the call only writes its outputs
    hj.lookup_wide_async(a.rk, a.rv, a.inner, ska, 9001, None, dsa, dva, dba, None)
    hj.synchronize()
    assert np.array_equal(read_outputs(9001, dva, dba)[0], vals_a)


# ---- neighbours ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [1000, 20000])
def test_a_constant_second_column_is_the_one_column_look_up(hj, inner):
    """non-zero unique keys in column 0, one constant in column 1 of both sides: values, bits and aggregates equal hjgpu_lookup_selected's"""
    rng = np.random.default_rng(160)
    keys = (rng.permutation(4 * inner)[:2 * inner] + 1).astype(np.uint32)
    ik, iv = keys[:inner], rng.integers(0, 1 << 32, inner, dtype=np.uint64).astype(np.uint32)
    ok = keys[rng.integers(0, 2 * inner, 4099)]
    sel = selection("half", 4099, 1)
    rk, rv, sk, dsel = col(hj, ik), col(hj, iv), col(hj, ok), hj.column(mask_words(sel))
    rc, sc = col(hj, np.full(inner, 77, np.uint32)), col(hj, np.full(4099, 77, np.uint32))
    dv, db = outputs(hj, 4099, "both")
    dv1, db1 = outputs(hj, 4099, "both")
    wide = tuple(hj.lookup_wide([rk, rc], rv, inner, [sk, sc], 4099, select_bits=dsel, vals_out=dv, match_bits=db))
    one = tuple(hj.lookup_selected(rk, rv, inner, sk, 4099, select_bits=dsel, vals_out=dv1, match_bits=db1))
    assert wide == one and wide[0] > 0
    assert np.array_equal(dv.download(), dv1.download()) and np.array_equal(db.download(), db1.download())
    # a different constant on the probe side: nothing matches
    sc2 = col(hj, np.full(4099, 78, np.uint32))
    assert tuple(hj.lookup_wide([rk, rc], rv, inner, [sk, sc2], 4099, select_bits=dsel)) == (0, 0, 0, 0)


def test_a_prepared_build_side_survives(hj):
    """hjgpu_phj_build, then hjgpu_phj_probe with a lookup_wide call in between: the same result as without one"""
    rng = np.random.default_rng(170)
    inner, outer = 50_000, 120_000
    ik = (rng.permutation(4 * inner)[:inner] + 1).astype(np.uint32)
    iv = rng.integers(0, 1 << 32, inner, dtype=np.uint64).astype(np.uint32)
    ok = ik[rng.integers(0, inner, outer)]
    ov = rng.integers(0, 1 << 32, outer, dtype=np.uint64).astype(np.uint32)
    rk, rv, sk, sv = col(hj, ik), col(hj, iv), col(hj, ok), col(hj, ov)
    hj.phj_build(rk, rv, inner, outer)
    before = tuple(hj.phj_probe(sk, sv, outer))
    sides = Sides(hj, 3, 3000, seed=171)
    check(sides, 4099, "half")
    after = tuple(hj.phj_probe(sk, sv, outer))
    assert before == after and before[0] == outer


# ---- the join it enables ---------------------------------------------------------------------------------------------------------------------
def test_a_composite_key_join_by_look_up_and_gather(hj):
    """lineitem JOIN partsupp ON (partkey, suppkey): lookup_wide with the dimension's row numbers as the build payload, then
    gather_selected of two dimension columns - equal to numpy's merge on the two columns"""
    rng = np.random.default_rng(180)
    parts, supps, dim_rows, fact_rows = 400, 50, 5000, 20011
    pairs = rng.permutation(parts * supps)[:dim_rows]
    d_part, d_supp = (pairs // supps).astype(np.uint32), (pairs % supps).astype(np.uint32)      # part 0 and supplier 0 are ordinary values
    d_cost, d_qty = rng.integers(0, 1 << 32, dim_rows, dtype=np.uint64).astype(np.uint32), rng.integers(0, 10_000, dim_rows).astype(np.uint32)
    f_part, f_supp = rng.integers(0, parts, fact_rows).astype(np.uint32), rng.integers(0, supps, fact_rows).astype(np.uint32)
    # numpy's merge: the dimension row of every fact row, -1 without one
    order = np.argsort(pairs)
    fkey = f_part.astype(np.int64) * supps + f_supp
    pos = np.searchsorted(pairs[order], fkey)
    found = (pos < dim_rows) & (pairs[order][np.minimum(pos, dim_rows - 1)] == fkey)
    row = np.where(found, order[np.minimum(pos, dim_rows - 1)], -1)
    assert 0 < found.sum() < fact_rows
    want_cost = np.where(found, d_cost[row], NULL).astype(np.uint32)
    want_qty = np.where(found, d_qty[row], NULL).astype(np.uint32)

    rk = [col(hj, d_part), col(hj, d_supp)]
    rows = col(hj, np.arange(dim_rows, dtype=np.uint32))
    sk = [col(hj, f_part), col(hj, f_supp)]
    d_idx, d_bits = outputs(hj, fact_rows, "both")
    res = tuple(hj.lookup_wide(rk, rows, dim_rows, sk, fact_rows, vals_out=d_idx, match_bits=d_bits))
    assert res == (int(found.sum()), _sum(f_part[found]), 0, _sum(row[found]))
    (o_cost, _), (o_qty, _) = outputs(hj, fact_rows, "vals"), outputs(hj, fact_rows, "vals")
    gathered, out_of_range = hj.gather_selected(d_bits, d_idx, fact_rows, [col(hj, d_cost), col(hj, d_qty)], dim_rows, [o_cost, o_qty])
    assert (gathered, out_of_range) == (int(found.sum()), 0)
    assert np.array_equal(read_outputs(fact_rows, o_cost, None)[0], want_cost)
    assert np.array_equal(read_outputs(fact_rows, o_qty, None)[0], want_qty)
    assert np.array_equal(read_outputs(fact_rows, None, d_bits)[1], found)
