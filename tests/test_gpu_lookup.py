"""GPU tests of hjgpu_lookup / hjgpu_lookup_async: the positional look-up that answers build sides of up to L rows
(hjgpu_get_counter "lookup_lds_rows") from hash tables in LDS - one persistent grid, every workgroup fills a table of its own once and
streams the probe column - and hands every larger build side to hjgpu_npj_lookup.  The contract is hjgpu_npj_lookup's: expected values
come from numpy, exact equality; the output buffers are longer than asked for and pre-filled with a pattern (nothing at index >= outer /
>= (outer + 31) // 32 may change, the high bits of the last word are 0).  hjgpu_get_stats tells the roads apart: fanout1 = fanout2 = 1
and buckets = 0 after the LDS road, buckets > 0 after the NPJ road.

Every test takes a context of its own: options set here must not reach the session's other tests."""
import os

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import NpjParams, HjGpuError
from test_gpu_npj_lookup import relations, want_unique, check_dups, outputs, read_outputs

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NULL = 0xFFFFFFFF
CANARY = 0xA5A5A5A5
MODES = ["both", "vals", "bits", "none"]
TAILS = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODE_FLAGS = [("HJGPU_FLAG_SEMI", api.FLAG_SEMI), ("HJGPU_FLAG_ANTI", api.FLAG_ANTI), ("HJGPU_FLAG_LEFT_OUTER", api.FLAG_LEFT_OUTER),
              ("HJGPU_FLAG_RIGHT_OUTER", api.FLAG_RIGHT_OUTER), ("HJGPU_FLAG_FULL_OUTER", api.FLAG_FULL_OUTER),
              ("HJGPU_FLAG_RIGHT_SEMI", api.FLAG_RIGHT_SEMI), ("HJGPU_FLAG_RIGHT_ANTI", api.FLAG_RIGHT_ANTI)]


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


def took_lds(hj):
    s = hj.stats()
    return s["fanout1"] == 1 and s["fanout2"] == 1 and s["buckets"] == 0


def took_npj(hj):
    s = hj.stats()
    return s["buckets"] > 0 and s["fanout1"] == 0 and s["fanout2"] == 0


def lookup(hj, ik, iv, ok, mode="both", prm=None, columns=None, fn=None):
    """(aggregates, vals or None, bits or None) of one blocking look-up (fn: hj.lookup, or hj.npj_lookup for comparison)"""
    rk, rv, sk = columns or (col(hj, ik), col(hj, iv), col(hj, ok))
    dv, db = outputs(hj, len(ok), mode)
    res = (fn or hj.lookup)(rk, rv, len(ik), sk, len(ok), params=prm, vals_out=dv, match_bits=db)
    vals, bits = read_outputs(len(ok), dv, db)
    return tuple(res), vals, bits


def check_unique(hj, ik, iv, ok, modes=MODES, road=took_lds):
    hit, vals, agg = want_unique(ik, iv, ok)
    columns = col(hj, ik), col(hj, iv), col(hj, ok)
    for mode in modes:
        res, gv, gb = lookup(hj, ik, iv, ok, mode, columns=columns)
        print("inner", len(ik), "outer", len(ok), mode, res, "want", agg)
        assert road(hj), hj.stats()
        assert res == agg, (mode, res, agg)
        if gv is not None:
            assert np.array_equal(gv, vals), (mode, np.flatnonzero(gv != vals)[:8])
        if gb is not None:
            assert np.array_equal(gb, hit), (mode, np.flatnonzero(gb != hit)[:8])


@pytest.mark.parametrize("outer", TAILS)
def test_tails(hj, outer):
    """vector, word, wave and workgroup edges; both outputs, values only, bits only, neither"""
    ik, iv, ok = relations(1000, outer, 0.5, seed=outer + 1)
    check_unique(hj, ik, iv, ok)


@pytest.mark.parametrize("inner", [0, 1, 7, 4096, 4097, "L"])
def test_geometry_edges(hj, inner):
    """no build rows, the 8 K-slot table up to its 4096 rows, the 16 K-slot table from 4097 to L"""
    L = hj.counter("lookup_lds_rows")
    assert 4097 < L <= 8192
    inner = L if inner == "L" else inner
    ik, iv, ok = relations(inner, 5003, 0.5, seed=inner + 2)
    check_unique(hj, ik, iv, ok, modes=["both", "none"])
    s = hj.stats()
    assert s["ms_build"] == 0 and s["ms_close_gaps"] == 0 and s["ms_join"] > 0 and s["ms_total"] >= s["ms_join"], s


def test_one_row_beyond_L_takes_the_npj_road(hj):
    L = hj.counter("lookup_lds_rows")
    ik, iv, ok = relations(L + 1, 5003, 0.5, seed=77)
    check_unique(hj, ik, iv, ok, modes=["both", "none"], road=took_npj)
    check_unique(hj, ik[:L], iv[:L], ok, modes=["both"], road=took_lds)


@pytest.mark.parametrize("inner", [1000, "L"])
def test_chained_path(hj, inner):
    """option force_chained: the double-hashing chains, unique keys"""
    hj.set_option("force_chained", 1)
    inner = hj.counter("lookup_lds_rows") if inner == "L" else inner
    ik, iv, ok = relations(inner, 5003, 0.5, seed=inner + 3)
    check_unique(hj, ik, iv, ok)


def test_more_than_one_trip_of_the_grid_stride_loop(hj):
    cus = hj.device_info()["compute_units"]
    outer = 2 * cus * 4096 + cus * 1024 + 5
    ik, iv, ok = relations(3000, outer, 0.5, seed=3)
    check_unique(hj, ik, iv, ok, modes=["both", "none"])


def dup_relations(distinct, heavy_copies, seed):
    """`distinct` keys x 16 copies plus one key with `heavy_copies` copies: the cuckoo fill cannot converge; probe keys half present"""
    ik, iv, ok = relations(distinct, 6001, 0.5, seed, copies=16)
    rng = np.random.default_rng(seed + 1)
    heavy = np.uint32(0x12345677)
    assert heavy not in ik and heavy not in ok
    ik = np.concatenate([ik, np.full(heavy_copies, heavy, np.uint32)])
    iv = np.concatenate([iv, rng.integers(0, 2**32, size=heavy_copies, dtype=np.uint64).astype(np.uint32)])
    perm = rng.permutation(len(ik))
    ok[rng.integers(0, len(ok), size=200)] = heavy
    return ik[perm], iv[perm], ok


@pytest.mark.parametrize("distinct,heavy_copies", [(128, 100), (256, 300)])
def test_duplicated_build_keys(hj, distinct, heavy_copies):
    """128 x 16 + 100 = 2148 rows: the 8 K-slot table; 256 x 16 + 300 = 4396 rows: the 16 K-slot table"""
    ik, iv, ok = dup_relations(distinct, heavy_copies, seed=7 + distinct)
    assert len(ik) <= hj.counter("lookup_lds_rows") and (len(ik) <= 4096) == (distinct == 128)
    res, vals, bits = lookup(hj, ik, iv, ok)
    assert took_lds(hj)
    check_dups(ik, iv, ok, res, vals, bits)
    hit = np.isin(ok, ik)
    assert lookup(hj, ik, iv, ok, "none")[0][:2] == (int(hit.sum()), _sum(ok[hit]))


def test_duplicated_probe_keys(hj):
    """every position gets its own answer; a genuine payload 0xFFFFFFFF has its bit set beside NULLs with the bit clear; key 0 matches nothing"""
    ik, iv, _ = relations(300, 0, seed=5)
    iv[::2] = NULL
    rng = np.random.default_rng(6)
    few = np.concatenate([ik[:6], np.array([0xDEAD0001, 0xDEAD0003, 0], np.uint32)])
    assert not np.isin(few[6:], ik).any()
    ok = few[rng.integers(0, len(few), size=3001)]
    ok[[0, 3, 64, 3000]] = 0
    hit, vals, agg = want_unique(ik, iv, ok)
    assert (vals[hit] == NULL).any() and (~hit).any() and not hit[ok == 0].any()
    res, gv, gb = lookup(hj, ik, iv, ok)
    assert took_lds(hj)
    assert res == agg and np.array_equal(gv, vals) and np.array_equal(gb, hit)
    assert np.all(gv[~gb] == NULL) and (gv[gb] == NULL).sum() == (vals[hit] == NULL).sum()


def test_build_key_zero(hj):
    ik, iv, ok = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    dv, db = outputs(hj, len(ok), "both")
    with pytest.raises(HjGpuError) as e:
        hj.lookup(rk, rv, len(ik), sk, len(ok), vals_out=dv, match_bits=db)
    assert e.value.status == api.EZEROKEY
    assert took_lds(hj)
    d_res = hj.column(4, np.uint64)
    d_flags = hj.column(np.zeros(2, np.uint64), np.uint64)
    hj.lookup_async(rk, rv, len(ik), sk, len(ok), None, dv, db, d_res)
    hj.accumulate_async_status(d_flags)
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()
    assert e.value.status == api.EZEROKEY
    assert [int(x) for x in d_flags.download()] == [1, 0]


def test_async_form(hj):
    """d_result equals the blocking result; two look-ups in flight on one stream with different output buffers both come out right"""
    ik, iv, ok = relations(3000, 9001, 0.5, seed=21)
    ik2, iv2, ok2 = relations(5000, 7003, 0.3, seed=22)
    hj.reserve(len(ik2), len(ok))
    blocking = lookup(hj, ik, iv, ok)[0]
    a = [col(hj, x) for x in (ik, iv, ok)]
    b = [col(hj, x) for x in (ik2, iv2, ok2)]
    (dva, dba), (dvb, dbb) = outputs(hj, len(ok), "both"), outputs(hj, len(ok2), "both")
    ra, rb = hj.column(4, np.uint64), hj.column(4, np.uint64)
    hj.lookup_async(a[0], a[1], len(ik), a[2], len(ok), None, dva, dba, ra)
    hj.lookup_async(b[0], b[1], len(ik2), b[2], len(ok2), None, dvb, dbb, rb)
    hj.get_async_status()
    assert took_lds(hj)
    for (k, v, o), dv, db, dr in ((ik, iv, ok), dva, dba, ra), ((ik2, iv2, ok2), dvb, dbb, rb):
        hit, vals, agg = want_unique(k, v, o)
        gv, gb = read_outputs(len(o), dv, db)
        assert tuple(int(x) for x in dr.download()) == agg
        assert np.array_equal(gv, vals) and np.array_equal(gb, hit)
    assert tuple(int(x) for x in ra.download()) == blocking


@pytest.mark.parametrize("inner", [2500, 6000])
def test_agrees_with_npj_lookup(hj, inner):
    """unique build keys: values, bits and aggregates identical to hjgpu_npj_lookup's on the same columns; under no_broadcast the NPJ road"""
    ik, iv, ok = relations(inner, 20011, 0.5, seed=31 + inner)
    columns = col(hj, ik), col(hj, iv), col(hj, ok)
    for mode in MODES:
        mine = lookup(hj, ik, iv, ok, mode, columns=columns)
        assert took_lds(hj)
        npj = lookup(hj, ik, iv, ok, mode, columns=columns, fn=hj.npj_lookup)
        assert took_npj(hj)
        assert mine[0] == npj[0], (mode, mine[0], npj[0])
        for x, y in zip(mine[1:], npj[1:]):
            assert (x is None and y is None) or np.array_equal(x, y), mode
    hj.set_option("no_broadcast", 1)
    assert hj.counter("lookup_lds_rows") == 0
    again = lookup(hj, ik, iv, ok, "both", columns=columns)
    assert took_npj(hj)
    hit, vals, agg = want_unique(ik, iv, ok)
    assert again[0] == agg and np.array_equal(again[1], vals) and np.array_equal(again[2], hit)


def test_refusals(hj):
    ik, iv, ok = relations(100, 300, 0.5, seed=41)
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    dv, db = outputs(hj, len(ok), "both")
    want = lookup(hj, ik, iv, ok, "none")[0]
    # each output, and the probe keys, misaligned by 4 bytes
    for kw in (dict(vals_out=dv.ptr + 4), dict(match_bits=db.ptr + 4)):
        with pytest.raises(HjGpuError) as e:
            hj.lookup(rk, rv, len(ik), sk, len(ok), **kw)
        assert e.value.status == api.EALIGN, kw
    with pytest.raises(HjGpuError) as e:
        hj.lookup(rk, rv, len(ik), sk.ptr + 4, len(ok) - 1)
    assert e.value.status == api.EALIGN
    # every join-mode flag, by name, in both forms
    d_res = hj.column(4, np.uint64)
    for name, flag in MODE_FLAGS:
        p = NpjParams(); p.flags = flag
        with pytest.raises(HjGpuError) as e:
            hj.lookup(rk, rv, len(ik), sk, len(ok), params=p, vals_out=dv, match_bits=db)
        assert e.value.status == api.EINVAL and name in str(e.value), (name, str(e.value))
        with pytest.raises(HjGpuError) as e:
            hj.lookup_async(rk, rv, len(ik), sk, len(ok), p, dv, db, d_res)
        assert e.value.status == api.EINVAL and name in str(e.value), (name, str(e.value))
    assert np.all(dv.download() == CANARY) and np.all(db.download() == CANARY)      # a refused call writes nothing
    # HJGPU_FLAG_UNIQUE is accepted and changes nothing
    p = NpjParams(); p.flags = api.FLAG_UNIQUE
    assert tuple(hj.lookup(rk, rv, len(ik), sk, len(ok), params=p)) == want
    assert took_lds(hj)


@pytest.mark.parametrize("name", ["unique_2k_16k", "dups16_8k_512", "key_zero_and_extremes"])
def test_golden_fixtures(hj, name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    ik, iv, ok = g["inner_keys"], g["inner_vals"], g["outer_keys"]
    if (ik == 0).any():
        with pytest.raises(HjGpuError) as e:
            lookup(hj, ik, iv, ok)
        assert e.value.status == api.EZEROKEY
    elif len(np.unique(ik)) == len(ik):
        check_unique(hj, ik, iv, ok, road=took_lds if len(ik) <= hj.counter("lookup_lds_rows") else took_npj)
    else:
        res, vals, bits = lookup(hj, ik, iv, ok)
        check_dups(ik, iv, ok, res, vals, bits)
        assert (took_lds if len(ik) <= hj.counter("lookup_lds_rows") else took_npj)(hj)      # dups16_8k_512: beyond L, the NPJ hand-over
