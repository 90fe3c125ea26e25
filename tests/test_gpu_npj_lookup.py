"""GPU tests of the positional NPJ look-up (hjgpu_npj_lookup, hjgpu_npj_lookup_async, hjgpu_npj_lookup_table): for every probe key, IN THE
PROBE COLUMN'S ORDER, the payload of the first build tuple its walk meets (HJGPU_NULL_VAL: none) and one bit "there is a match".  Expected
values come from numpy, exact equality.  The output buffers are longer than asked for and pre-filled with a pattern: nothing at index
>= outer / >= (outer + 31) // 32 may change, and the high bits of the last word are 0.

Every test takes a context of its own: options set here must not reach the session's other tests."""
import os

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import NpjParams, HjGpuError

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NULL = 0xFFFFFFFF
CANARY = 0xA5A5A5A5
EXTRA_VALS, EXTRA_WORDS = 64, 4
MODES = ["both", "vals", "bits", "none"]
TAILS = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]
NPJ_FACTOR = 0x9E3779B1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODE_FLAGS = [("HJGPU_FLAG_SEMI", api.FLAG_SEMI), ("HJGPU_FLAG_ANTI", api.FLAG_ANTI), ("HJGPU_FLAG_LEFT_OUTER", api.FLAG_LEFT_OUTER),
              ("HJGPU_FLAG_RIGHT_OUTER", api.FLAG_RIGHT_OUTER), ("HJGPU_FLAG_FULL_OUTER", api.FLAG_FULL_OUTER),
              ("HJGPU_FLAG_RIGHT_SEMI", api.FLAG_RIGHT_SEMI), ("HJGPU_FLAG_RIGHT_ANTI", api.FLAG_RIGHT_ANTI)]


@pytest.fixture
def ctx():
    """a context whose device columns are all freed when the test ends (a DeviceColumn is freed only by free())"""
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    with H.HjGpu(0) as hj:
        made, column = [], hj.column

        def tracked(*a, **k):
            c = column(*a, **k)
            made.append(c)
            return c
        hj.column = tracked
        try:
            yield hj
        finally:
            for c in made:
                c.free()


def _sum(a):
    return int(a.astype(np.uint64).sum(dtype=np.uint64)) & M64


def relations(inner, outer, sel=0.5, seed=1, copies=1):
    """`inner` distinct build keys (each `copies` times, shuffled), payloads of every value; a `sel` share of the probe keys is present"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, 2**32 - 1, size=2 * inner + 64, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    keys, miss = pool[:inner], pool[inner:]
    ik = np.repeat(keys, copies)
    rng.shuffle(ik)
    iv = rng.integers(0, 2**32, size=len(ik), dtype=np.uint64).astype(np.uint32)
    hit = (rng.random(outer) < sel) & (inner > 0)
    ok = np.where(hit, keys[rng.integers(0, max(inner, 1), size=outer)] if inner else 0, miss[rng.integers(0, len(miss), size=outer)]).astype(np.uint32)
    return ik, iv, ok


def want_unique(ik, iv, ok):
    """(hit, vals, aggregates) of the look-up in unique build keys: the definition"""
    if len(ik) == 0:
        hit = np.zeros(len(ok), bool)
        vals = np.full(len(ok), NULL, np.uint32)
    else:
        o = np.argsort(ik)
        p = np.searchsorted(ik[o], ok).clip(0, len(ik) - 1)
        hit = ik[o][p] == ok
        vals = np.where(hit, iv[o][p], NULL).astype(np.uint32)
    return hit, vals, (int(hit.sum()), _sum(ok[hit]), 0, _sum(vals[hit]))


def col(hj, a):
    return hj.column(a) if len(a) else hj.column(np.zeros(4, np.uint32))


def outputs(hj, outer, mode):
    dv = hj.column(np.full(outer + EXTRA_VALS, CANARY, np.uint32)) if mode in ("both", "vals") else None
    db = hj.column(np.full((outer + 31) // 32 + EXTRA_WORDS, CANARY, np.uint32)) if mode in ("both", "bits") else None
    return dv, db


def read_outputs(outer, dv, db):
    """the outputs' first `outer` values / bits, after the canaries and the last word's high bits have been checked"""
    vals = bits = None
    if dv is not None:
        raw = dv.download()
        assert np.all(raw[outer:] == CANARY), "d_vals_out was written at index >= outer"
        vals = raw[:outer]
    if db is not None:
        raw = db.download()
        words = (outer + 31) // 32
        assert np.all(raw[words:] == CANARY), "d_match_bits was written at index >= (outer + 31) / 32"
        unpacked = np.unpackbits(raw[:words].view(np.uint8), bitorder="little")
        assert not unpacked[outer:].any(), "bits of the last word at positions >= outer are not 0"
        bits = unpacked[:outer].astype(bool)
    return vals, bits


def lookup(hj, ik, iv, ok, mode="both", prm=None, columns=None):
    """(aggregates, vals or None, bits or None) of one blocking look-up"""
    rk, rv, sk = columns or (col(hj, ik), col(hj, iv), col(hj, ok))
    dv, db = outputs(hj, len(ok), mode)
    try:
        res = hj.npj_lookup(rk, rv, len(ik), sk, len(ok), params=prm, vals_out=dv, match_bits=db)
        vals, bits = read_outputs(len(ok), dv, db)
    finally:
        for c in (dv, db) + (() if columns else (rk, rv, sk)):
            if c is not None:
                c.free()
    return tuple(res), vals, bits


def check_unique(hj, ik, iv, ok, modes=MODES, prm_fn=lambda: None):
    hit, vals, agg = want_unique(ik, iv, ok)
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    for mode in modes:
        res, gv, gb = lookup(hj, ik, iv, ok, mode, prm_fn(), columns=(rk, rv, sk))
        print("outer", len(ok), mode, res, "want", agg)
        assert res == agg, (mode, res, agg)
        if gv is not None:
            assert np.array_equal(gv, vals), (mode, np.flatnonzero(gv != vals)[:8])
        if gb is not None:
            assert np.array_equal(gb, hit), (mode, np.flatnonzero(gb != hit)[:8])
    for c in (rk, rv, sk):
        c.free()


def check_dups(ik, iv, ok, res, vals, bits):
    """duplicated build keys: EVERY position - the bit, a payload of that key where it is set, NULL where it is clear - and the count"""
    hit = np.isin(ok, ik)
    assert np.array_equal(bits, hit)
    assert np.all(vals[~hit] == NULL)
    pairs = np.unique((ik.astype(np.uint64) << np.uint64(32)) | iv.astype(np.uint64))
    got = (ok.astype(np.uint64) << np.uint64(32)) | vals.astype(np.uint64)
    assert np.all(np.isin(got[hit], pairs)), "a value that is no payload of its key"
    assert res == (int(hit.sum()), _sum(ok[hit]), 0, _sum(vals[hit])), res


def dup_relations(seed=7):
    """512 distinct keys x 16 copies, plus one key with 300 copies (its walk goes over many lines); probe keys half present"""
    ik, iv, ok = relations(512, 6001, 0.5, seed, copies=16)
    rng = np.random.default_rng(seed + 1)
    heavy = np.uint32(0x12345677)
    assert heavy not in ik and heavy not in ok
    ik = np.concatenate([ik, np.full(300, heavy, np.uint32)])
    iv = np.concatenate([iv, rng.integers(0, 2**32, size=300, dtype=np.uint64).astype(np.uint32)])
    perm = rng.permutation(len(ik))
    ok[rng.integers(0, len(ok), size=200)] = heavy
    return ik[perm], iv[perm], ok


@pytest.mark.parametrize("outer", TAILS)
def test_tails(ctx, outer):
    """vector, word, wave and workgroup edges; both outputs, values only, bits only, neither"""
    ik, iv, ok = relations(1000, outer, 0.5, seed=outer + 1)
    check_unique(ctx, ik, iv, ok)


def test_more_than_one_trip_of_the_grid_stride_loop(ctx):
    cus = ctx.device_info()["compute_units"]
    outer = cus * 8 * 1024 * 2 + cus * 1024 + 5
    ik, iv, ok = relations(100_000, outer, 0.5, seed=3)
    check_unique(ctx, ik, iv, ok, modes=["both", "none"])


@pytest.mark.parametrize("inner,load", [(4096, 0.95), (7, 0.99)])
def test_long_walks_and_the_wrap(ctx, inner, load):
    """inner = 7 at load 0.99: 16 buckets, two lines - walks cross the table's end"""
    ik, iv, ok = relations(inner, 5003, 0.5, seed=inner)

    def prm():
        p = NpjParams(); p.load = load; return p
    check_unique(ctx, ik, iv, ok, modes=["both", "bits"], prm_fn=prm)
    assert ctx.stats()["buckets"] == (16 if inner == 7 else (int(inner / load) + 7) & ~7)


def test_duplicated_build_keys(ctx):
    ik, iv, ok = dup_relations()
    res, vals, bits = lookup(ctx, ik, iv, ok)
    check_dups(ik, iv, ok, res, vals, bits)
    hit = np.isin(ok, ik)
    assert lookup(ctx, ik, iv, ok, "none")[0][:2] == (int(hit.sum()), _sum(ok[hit]))


def test_duplicated_probe_keys(ctx):
    """every position gets its own answer"""
    ik, iv, _ = relations(300, 0, seed=5)
    rng = np.random.default_rng(6)
    few = np.concatenate([ik[:5], np.array([0xDEAD0001, 0xDEAD0003], np.uint32)])
    assert not np.isin(few[5:], ik).any()
    ok = few[rng.integers(0, len(few), size=3001)]
    check_unique(ctx, ik, iv, ok, modes=["both"])


def test_a_genuine_payload_of_all_ones(ctx):
    """value 0xFFFFFFFF with the bit SET beside absent keys with the bit clear: what the bitmap exists for"""
    ik, iv, ok = relations(200, 777, 0.5, seed=8)
    iv[::2] = NULL
    hit, vals, agg = want_unique(ik, iv, ok)
    assert (vals[hit] == NULL).any() and (~hit).any()
    res, gv, gb = lookup(ctx, ik, iv, ok)
    assert res == agg and np.array_equal(gv, vals) and np.array_equal(gb, hit)
    assert np.all(gv[~gb] == NULL) and (gv[gb] == NULL).sum() == (vals[hit] == NULL).sum()


def test_probe_key_zero_matches_nothing(ctx):
    ik, iv, ok = relations(500, 1000, 0.5, seed=9)
    ok[[0, 3, 64, 999]] = 0
    hit, vals, agg = want_unique(ik, iv, ok)
    assert not hit[[0, 3, 64, 999]].any()
    res, gv, gb = lookup(ctx, ik, iv, ok)
    assert res == agg and np.array_equal(gv, vals) and np.array_equal(gb, hit)


def test_build_key_zero(ctx):
    ik, iv, ok = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0
    rk, rv, sk = col(ctx, ik), col(ctx, iv), col(ctx, ok)
    dv, db = outputs(ctx, len(ok), "both")
    with pytest.raises(HjGpuError) as e:
        ctx.npj_lookup(rk, rv, len(ik), sk, len(ok), vals_out=dv, match_bits=db)
    assert e.value.status == api.EZEROKEY
    d_res = ctx.column(4, np.uint64)
    d_flags = ctx.column(np.zeros(2, np.uint64), np.uint64)
    ctx.npj_lookup_async(rk, rv, len(ik), sk, len(ok), None, dv, db, d_res)
    ctx.accumulate_async_status(d_flags)
    with pytest.raises(HjGpuError) as e:
        ctx.get_async_status()
    assert e.value.status == api.EZEROKEY
    assert [int(x) for x in d_flags.download()] == [1, 0]


def test_no_build_rows(ctx):
    ik, iv, ok = relations(0, 777, seed=11)
    res, gv, gb = lookup(ctx, ik, iv, ok)
    assert res == (0, 0, 0, 0) and np.all(gv == NULL) and not gb.any()


@pytest.mark.parametrize("outer", TAILS)
def test_reference_hash_tails(ctx, outer):
    ctx.set_option("npj_refhash", 1)
    ik, iv, ok = relations(1000, outer, 0.5, seed=outer + 100)
    check_unique(ctx, ik, iv, ok)


def test_reference_hash_duplicates(ctx):
    ctx.set_option("npj_refhash", 1)
    ik, iv, ok = dup_relations(seed=17)
    res, vals, bits = lookup(ctx, ik, iv, ok)
    check_dups(ik, iv, ok, res, vals, bits)


@pytest.mark.parametrize("buckets", [4000, 4001])
def test_lookup_in_a_built_table(ctx, buckets):
    """buckets % 4 == 0: the grouped walk; % 4 == 1: bucket at a time.  Two batches against one table; results equal npj_lookup's"""
    ik, iv, ok = relations(1500, 5003, 0.5, seed=buckets)
    hit, vals, _ = want_unique(ik, iv, ok)
    rk, rv = col(ctx, ik), col(ctx, iv)
    dt = ctx.column(buckets, np.uint64)
    ctx.npj_build(rk, rv, len(ik), dt, buckets, NPJ_FACTOR)
    for lo, hi in ((0, 2048), (2048, len(ok))):
        part = ok[lo:hi]
        sk = col(ctx, part)
        for mode in MODES:
            dv, db = outputs(ctx, len(part), mode)
            res = ctx.npj_lookup_table(sk, len(part), dt, buckets, NPJ_FACTOR, vals_out=dv, match_bits=db)
            gv, gb = read_outputs(len(part), dv, db)
            whole = lookup(ctx, ik, iv, part, mode)
            assert tuple(res) == whole[0] == (int(hit[lo:hi].sum()), _sum(part[hit[lo:hi]]), 0, _sum(vals[lo:hi][hit[lo:hi]])), (mode, res)
            if gv is not None:
                assert np.array_equal(gv, vals[lo:hi]) and np.array_equal(gv, whole[1])
            if gb is not None:
                assert np.array_equal(gb, hit[lo:hi]) and np.array_equal(gb, whole[2])
            for c in (dv, db):
                if c is not None:
                    c.free()


def test_async_form(ctx):
    """d_result equals the blocking result; two look-ups in flight on one stream with different output buffers both come out right"""
    ik, iv, ok = relations(3000, 9001, 0.5, seed=21)
    ik2, iv2, ok2 = relations(2000, 7003, 0.3, seed=22)
    ctx.reserve(len(ik), len(ok))
    blocking = lookup(ctx, ik, iv, ok)[0]
    a = [col(ctx, x) for x in (ik, iv, ok)]
    b = [col(ctx, x) for x in (ik2, iv2, ok2)]
    (dva, dba), (dvb, dbb) = outputs(ctx, len(ok), "both"), outputs(ctx, len(ok2), "both")
    ra, rb = ctx.column(4, np.uint64), ctx.column(4, np.uint64)
    ctx.npj_lookup_async(a[0], a[1], len(ik), a[2], len(ok), None, dva, dba, ra)
    ctx.npj_lookup_async(b[0], b[1], len(ik2), b[2], len(ok2), None, dvb, dbb, rb)
    ctx.get_async_status()
    for (k, v, o), dv, db, dr in ((ik, iv, ok), dva, dba, ra), ((ik2, iv2, ok2), dvb, dbb, rb):
        hit, vals, agg = want_unique(k, v, o)
        gv, gb = read_outputs(len(o), dv, db)
        assert tuple(int(x) for x in dr.download()) == agg
        assert np.array_equal(gv, vals) and np.array_equal(gb, hit)
    assert tuple(int(x) for x in ra.download()) == blocking


def test_consistent_with_the_joins(ctx):
    ik, iv, ok = relations(5000, 20011, 0.5, seed=31)
    ov = np.arange(len(ok), dtype=np.uint32)
    res = lookup(ctx, ik, iv, ok, "none")[0]
    rk, rv, sk, sv = (ctx.column(x) for x in (ik, iv, ok, ov))
    p = NpjParams(); p.flags = api.FLAG_SEMI
    semi = ctx.npj(rk, rv, len(ik), sk, sv, len(ok), params=p)
    assert res[:2] == tuple(semi)[:2]
    p = NpjParams(); p.flags = api.FLAG_UNIQUE
    uniq = ctx.npj(rk, rv, len(ik), sk, sv, len(ok), params=p)
    assert res[3] == tuple(uniq)[3] and res[0] == tuple(uniq)[0]


def test_stats(ctx):
    ik, iv, ok = relations(5000, 20011, 0.5, seed=32)
    lookup(ctx, ik, iv, ok)
    s = ctx.stats()
    assert s["buckets"] == (int(5000 / 0.25) + 7) & ~7
    assert s["ms_close_gaps"] == 0 and s["ms_build"] > 0 and s["ms_join"] > 0 and s["ms_total"] >= s["ms_join"]


def test_refusals(ctx):
    ik, iv, ok = relations(100, 300, 0.5, seed=41)
    rk, rv, sk = col(ctx, ik), col(ctx, iv), col(ctx, ok)
    dv, db = outputs(ctx, len(ok), "both")
    want = lookup(ctx, ik, iv, ok, "none")[0]
    # each output, and the probe keys, misaligned by 4 bytes
    for kw in (dict(vals_out=dv.ptr + 4), dict(match_bits=db.ptr + 4)):
        with pytest.raises(HjGpuError) as e:
            ctx.npj_lookup(rk, rv, len(ik), sk, len(ok), **kw)
        assert e.value.status == api.EALIGN, kw
    with pytest.raises(HjGpuError) as e:
        ctx.npj_lookup(rk, rv, len(ik), sk.ptr + 4, len(ok) - 1)
    assert e.value.status == api.EALIGN
    dt = ctx.column(1024, np.uint64)
    ctx.npj_build(rk, rv, len(ik), dt, 1024, NPJ_FACTOR)
    for kw in (dict(vals_out=dv.ptr + 4), dict(match_bits=db.ptr + 4)):
        with pytest.raises(HjGpuError) as e:
            ctx.npj_lookup_table(sk, len(ok), dt, 1024, NPJ_FACTOR, **kw)
        assert e.value.status == api.EALIGN, kw
    # every join-mode flag, by name
    d_res = ctx.column(4, np.uint64)
    for name, flag in MODE_FLAGS:
        p = NpjParams(); p.flags = flag
        with pytest.raises(HjGpuError) as e:
            ctx.npj_lookup(rk, rv, len(ik), sk, len(ok), params=p, vals_out=dv, match_bits=db)
        assert e.value.status == api.EINVAL and name in str(e.value), (name, str(e.value))
        with pytest.raises(HjGpuError) as e:
            ctx.npj_lookup_async(rk, rv, len(ik), sk, len(ok), p, dv, db, d_res)
        assert e.value.status == api.EINVAL and name in str(e.value), (name, str(e.value))
    assert np.all(dv.download() == CANARY) and np.all(db.download() == CANARY)      # a refused call writes nothing
    # HJGPU_FLAG_UNIQUE is accepted and changes nothing
    p = NpjParams(); p.flags = api.FLAG_UNIQUE
    assert tuple(ctx.npj_lookup(rk, rv, len(ik), sk, len(ok), params=p)) == want
    p = NpjParams(); p.load = 1.0
    with pytest.raises(HjGpuError) as e:
        ctx.npj_lookup(rk, rv, len(ik), sk, len(ok), params=p)
    assert e.value.status == api.EINVAL


@pytest.mark.parametrize("name", ["unique_2k_16k", "dups16_8k_512", "key_zero_and_extremes"])
def test_golden_fixtures(ctx, name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    ik, iv, ok = g["inner_keys"], g["inner_vals"], g["outer_keys"]
    if (ik == 0).any():
        with pytest.raises(HjGpuError) as e:
            lookup(ctx, ik, iv, ok)
        assert e.value.status == api.EZEROKEY
    elif len(np.unique(ik)) == len(ik):
        check_unique(ctx, ik, iv, ok)
    else:
        res, vals, bits = lookup(ctx, ik, iv, ok)
        check_dups(ik, iv, ok, res, vals, bits)
