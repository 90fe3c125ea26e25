"""GPU tests of the selected look-ups (hjgpu_lookup_selected, hjgpu_lookup_selected_async, hjgpu_npj_lookup_table_selected): the positional
look-ups with an input bitmap in d_match_bits' layout.  Only the rows whose bit is set are looked up; an unselected row gets NULL and bit
0 and is counted in no aggregate; d_match_bits may be d_select_bits itself, and is then select AND match afterwards.

Expected values come from numpy: hit_sel = hit & sel, vals = where(hit_sel, vals, NULL), the aggregates over hit_sel.  Exact equality.
Both outputs are longer than asked for and pre-filled with a pattern; the mask is followed by all-ones words that must not influence
anything, and (where it is not the output) comes back unchanged.  Every road is asserted with hjgpu_get_stats.

Every test takes a context of its own: options set here must not reach the session's other tests."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import NpjParams, HjGpuError
from test_gpu_npj_lookup import relations, want_unique, check_dups, outputs, read_outputs
from test_gpu_npj_lookup import dup_relations as npj_dup_relations
from test_gpu_lookup import dup_relations as lds_dup_relations

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NULL = 0xFFFFFFFF
CANARY = 0xA5A5A5A5
ONES = 0xFFFFFFFF
EXTRA_WORDS = 4
MODES = ["both", "vals", "bits", "none"]
TAILS = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]
NPJ_FACTOR = 0x9E3779B1
MODE_FLAGS = [("HJGPU_FLAG_SEMI", api.FLAG_SEMI), ("HJGPU_FLAG_ANTI", api.FLAG_ANTI), ("HJGPU_FLAG_LEFT_OUTER", api.FLAG_LEFT_OUTER),
              ("HJGPU_FLAG_RIGHT_OUTER", api.FLAG_RIGHT_OUTER), ("HJGPU_FLAG_FULL_OUTER", api.FLAG_FULL_OUTER),
              ("HJGPU_FLAG_RIGHT_SEMI", api.FLAG_RIGHT_SEMI), ("HJGPU_FLAG_RIGHT_ANTI", api.FLAG_RIGHT_ANTI)]
ROADS = ["lds512", "lds1024", "chained", "npj_line", "npj_line_beyond_L", "npj_refhash", "table_ungrouped", "table_grouped"]
MASKS = ["ones", "zeros", "half", "eighth", "alternating_words", "first_row", "last_row", "garbage_tail"]


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


def selection(kind, outer, seed):
    """the rows a mask of this kind selects"""
    rng = np.random.default_rng(seed)
    sel = np.zeros(outer, bool)
    if kind == "ones":
        sel[:] = True
    elif kind in ("half", "garbage_tail"):
        sel = rng.random(outer) < 0.5
    elif kind == "eighth":
        sel = rng.random(outer) < 0.125
    elif kind == "alternating_words":
        sel = (np.arange(outer) >> 5) % 2 == 1               # words 0x00000000 / 0xFFFFFFFF: key-load skip and trip skip beside live words
    elif kind == "first_row":
        sel[:1] = True
    elif kind == "last_row":
        sel[outer - 1:] = True
    else:
        assert kind == "zeros", kind
    return sel


def pack(bits):
    """the bitmap words of a bool array, the last word's high bits 0"""
    padded = np.zeros((len(bits) + 31) // 32 * 32, np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint32).copy()


def mask_words(sel, kind="half"):
    """the mask buffer: the bitmap (kinds ones / alternating_words / garbage_tail: the last word's bits at positions >= outer SET), then
    EXTRA_WORDS all-ones words that nothing may read"""
    w = pack(sel)
    if kind in ("ones", "alternating_words", "garbage_tail") and len(sel) % 32:
        w[-1] = np.uint32(int(w[-1]) | (ONES << (len(sel) % 32)) & ONES)
    return np.concatenate([w, np.full(EXTRA_WORDS, ONES, np.uint32)])


def want_selected(ik, iv, ok, sel):
    hit, vals, _ = want_unique(ik, iv, ok)
    hit_sel = hit & sel
    vals = np.where(hit_sel, vals, NULL).astype(np.uint32)
    return hit_sel, vals, (int(hit_sel.sum()), _sum(ok[hit_sel]), 0, _sum(vals[hit_sel]))


class Road:
    """one of the roads a selected look-up takes: its options, its build side (uploaded once), its call, and how the stats show it"""

    def __init__(self, hj, name, seed=1, build=None):
        self.hj, self.name, self.seed = hj, name, seed
        L = hj.counter("lookup_lds_rows")
        assert 4097 < L <= 8192
        self.inner = {"lds1024": L, "npj_line_beyond_L": L + 1, "table_ungrouped": 1500, "table_grouped": 1500}.get(name, 1000)
        if name == "chained":
            hj.set_option("force_chained", 1)
        if name in ("npj_line", "npj_refhash"):
            hj.set_option("no_broadcast", 1)
        if name == "npj_refhash":
            hj.set_option("npj_refhash", 1)
        self.ik, self.iv = build if build is not None else relations(self.inner, 0, seed=seed)[:2]
        self.rk, self.rv = col(hj, self.ik), col(hj, self.iv)
        self.table = name.startswith("table")
        if self.table:
            self.buckets = 4001 if name == "table_ungrouped" else 4000          # % 4 != 0: bucket at a time; % 4 == 0 and 32-byte aligned: grouped
            self.dt = hj.column(self.buckets, np.uint64)
            assert self.dt.ptr % 32 == 0
            hj.npj_build(self.rk, self.rv, len(self.ik), self.dt, self.buckets, NPJ_FACTOR)

    def probe_keys(self, outer):
        """probe keys, half of them present (relations() draws the build side first: the same for every outer)"""
        if len(self.ik) != self.inner:
            raise AssertionError("a road with a build side of its own has no generated probe keys")
        ik, _, ok = relations(self.inner, outer, 0.5, seed=self.seed)
        assert np.array_equal(ik, self.ik)
        return ok

    def call(self, sk, outer, select_bits, dv, db, prm=None):
        if self.table:
            return tuple(self.hj.npj_lookup_table_selected(sk, outer, self.dt, self.buckets, NPJ_FACTOR, select_bits=select_bits,
                                                           vals_out=dv, match_bits=db))
        return tuple(self.hj.lookup_selected(self.rk, self.rv, len(self.ik), sk, outer, params=prm, select_bits=select_bits,
                                             vals_out=dv, match_bits=db))

    def plain(self, sk, outer, dv, db):
        if self.table:
            return tuple(self.hj.npj_lookup_table(sk, outer, self.dt, self.buckets, NPJ_FACTOR, vals_out=dv, match_bits=db))
        return tuple(self.hj.lookup(self.rk, self.rv, len(self.ik), sk, outer, vals_out=dv, match_bits=db))

    def assert_taken(self):
        s = self.hj.stats()
        assert s["ms_close_gaps"] == 0, s
        if self.name in ("lds512", "lds1024", "chained"):
            assert s["fanout1"] == 1 and s["fanout2"] == 1 and s["buckets"] == 0 and s["ms_build"] == 0, s
        elif self.table:
            assert s["buckets"] == self.buckets, s
        else:
            assert s["buckets"] > 0 and s["fanout1"] == 0 and s["fanout2"] == 0, s


def check(road, ok, sel, kind="half", modes=("both",)):
    """one selected look-up per output mode against numpy; the mask comes back unchanged"""
    hj, outer = road.hj, len(ok)
    hit_sel, vals, agg = want_selected(road.ik, road.iv, ok, sel)
    words = mask_words(sel, kind)
    sk, dsel = col(hj, ok), hj.column(words)
    for mode in modes:
        dv, db = outputs(hj, outer, mode)
        res = road.call(sk, outer, dsel, dv, db)
        gv, gb = read_outputs(outer, dv, db)
        print(road.name, kind, "outer", outer, mode, res, "want", agg)
        road.assert_taken()
        assert res == agg, (road.name, kind, outer, mode, res, agg)
        if gv is not None:
            assert np.array_equal(gv, vals), (road.name, kind, outer, mode, np.flatnonzero(gv != vals)[:8])
        if gb is not None:
            assert np.array_equal(gb, hit_sel), (road.name, kind, outer, mode, np.flatnonzero(gb != hit_sel)[:8])
        assert np.array_equal(dsel.download(), words), "the mask was written"
        for c in (dv, db):
            if c is not None:
                c.free()
    return sk, (hit_sel, vals, agg)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", ROADS)
def test_masks(hj, name, kind):
    """every kind of mask over the vector, word, wave and workgroup edges of outer; an all-ones mask gives the plain look-up's outputs"""
    road = Road(hj, name)
    for outer in TAILS:
        ok = road.probe_keys(outer)
        sel = selection(kind, outer, seed=outer + 11)
        sk, (hit_sel, vals, agg) = check(road, ok, sel, kind)
        if kind == "ones":
            dv, db = outputs(hj, outer, "both")
            res = road.plain(sk, outer, dv, db)
            gv, gb = read_outputs(outer, dv, db)
            assert res == agg and np.array_equal(gv, vals) and np.array_equal(gb, hit_sel), (name, outer)
        if kind == "zeros":
            assert agg == (0, 0, 0, 0) and np.all(vals == NULL) and not hit_sel.any()


@pytest.mark.parametrize("name", ROADS)
def test_output_modes(hj, name):
    """both / values only / bits only / neither"""
    road = Road(hj, name, seed=2)
    ok = road.probe_keys(4099)
    check(road, ok, selection("half", 4099, seed=5), modes=MODES)


@pytest.mark.parametrize("name", ROADS)
def test_in_place(hj, name):
    """match_bits IS select_bits: afterwards the bitmap is sel & hit, the words behind it are untouched; also over more than one trip of
    the grid-stride loop"""
    road = Road(hj, name, seed=3)
    cus = hj.device_info()["compute_units"]
    for outer in (33, 257, 4099, 2 * cus * 4096 + cus * 1024 + 5):
        ok = road.probe_keys(outer)
        sel = selection("garbage_tail", outer, seed=outer + 7)
        hit_sel, vals, agg = want_selected(road.ik, road.iv, ok, sel)
        words = mask_words(sel, "garbage_tail")
        sk, dbits = col(hj, ok), hj.column(words)
        dv, _ = outputs(hj, outer, "vals")
        res = road.call(sk, outer, dbits, dv, dbits)
        road.assert_taken()
        gv, _ = read_outputs(outer, dv, None)
        got = dbits.download()
        n = (outer + 31) // 32
        assert res == agg, (name, outer, res, agg)
        assert np.array_equal(got[:n], pack(hit_sel)), (name, outer, np.flatnonzero(got[:n] != pack(hit_sel))[:8])
        assert np.all(got[n:] == ONES), "words behind the bitmap were written"
        assert np.array_equal(gv, vals), (name, outer, np.flatnonzero(gv != vals)[:8])
        for c in (sk, dbits, dv):
            c.free()


def test_a_chain_of_two_dimensions(hj):
    """bits = lookup(d1); lookup_selected(d2, select = bits, match_bits = bits): ONE bitmap narrowed in place, over both roads"""
    L = hj.counter("lookup_lds_rows")
    outer = 100_003
    d1k, d1v, k1 = relations(5000, outer, 0.5, seed=51)
    d2k, d2v, k2 = relations(L + 1, outer, 0.5, seed=52)
    cols = [col(hj, x) for x in (d1k, d1v, k1, d2k, d2v, k2)]
    dv1, bits = outputs(hj, outer, "both")
    dv2, _ = outputs(hj, outer, "vals")
    r1 = tuple(hj.lookup(cols[0], cols[1], len(d1k), cols[2], outer, vals_out=dv1, match_bits=bits))
    s = hj.stats()
    assert s["fanout1"] == 1 and s["buckets"] == 0, s                    # d1: the LDS road
    in1 = np.isin(k1, d1k)
    assert r1[0] == int(in1.sum())
    r2 = tuple(hj.lookup_selected(cols[3], cols[4], len(d2k), cols[5], outer, select_bits=bits, vals_out=dv2, match_bits=bits))
    s = hj.stats()
    assert s["buckets"] > 0 and s["fanout1"] == 0, s                     # d2: the NPJ road
    hit2, vals2, agg2 = want_selected(d2k, d2v, k2, in1)
    gv2, gb = read_outputs(outer, dv2, bits)
    assert np.array_equal(gb, in1 & np.isin(k2, d2k)) and np.array_equal(gb, hit2)
    assert r2 == agg2
    assert np.array_equal(gv2, vals2) and np.all(gv2[~gb] == NULL)


@pytest.mark.parametrize("name", ["lds", "npj_line"])
def test_duplicated_build_keys(hj, name):
    """any copy may answer a selected row; check_dups restricted to the selected rows, the others NULL with bit 0"""
    if name == "lds":
        ik, iv, ok = lds_dup_relations(128, 100, seed=135)
        road = Road(hj, "lds512", build=(ik, iv))
    else:
        ik, iv, ok = npj_dup_relations()
        road = Road(hj, "npj_line", build=(ik, iv))
    outer = len(ok)
    sel = selection("half", outer, seed=9)
    sk, dsel = col(hj, ok), hj.column(mask_words(sel))
    dv, db = outputs(hj, outer, "both")
    res = road.call(sk, outer, dsel, dv, db)
    road.assert_taken()
    gv, gb = read_outputs(outer, dv, db)
    assert np.all(gv[~sel] == NULL) and not gb[~sel].any()
    check_dups(ik, iv, ok[sel], res, gv[sel], gb[sel])


@pytest.mark.parametrize("name", ["lds512", "npj_line"])
def test_a_selected_probe_key_zero_matches_nothing(hj, name):
    road = Road(hj, name, seed=4)
    ok = road.probe_keys(1000)
    ok[[0, 3, 64, 999]] = 0
    sel = selection("half", 1000, seed=4)
    sel[[0, 3, 64, 999]] = True
    _, (hit_sel, _, _) = check(road, ok, sel)
    assert not hit_sel[[0, 3, 64, 999]].any()


@pytest.mark.parametrize("name", ["lds512", "npj_line"])
def test_build_key_zero_under_an_all_zero_mask(hj, name):
    """the fill finds it whatever the mask says: the blocking form raises, the async form reports through the status calls"""
    ik, iv, ok = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0
    road = Road(hj, name, build=(ik, iv))
    sk, dsel = col(hj, ok), hj.column(mask_words(np.zeros(len(ok), bool)))
    dv, db = outputs(hj, len(ok), "both")
    with pytest.raises(HjGpuError) as e:
        road.call(sk, len(ok), dsel, dv, db)
    assert e.value.status == api.EZEROKEY
    road.assert_taken()
    d_res = hj.column(4, np.uint64)
    d_flags = hj.column(np.zeros(2, np.uint64), np.uint64)
    hj.lookup_selected_async(road.rk, road.rv, len(ik), sk, len(ok), None, dsel, dv, db, d_res)
    hj.accumulate_async_status(d_flags)
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()
    assert e.value.status == api.EZEROKEY
    assert [int(x) for x in d_flags.download()] == [1, 0]


@pytest.mark.parametrize("no_broadcast", [0, 1])
def test_no_build_rows(hj, no_broadcast):
    """inner == 0 is never beyond lookup_lds_rows, 0 under no_broadcast included: the LDS road, as for hjgpu_lookup"""
    road = Road(hj, "lds512", build=(np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
    hj.set_option("no_broadcast", no_broadcast)
    _, _, ok = relations(0, 777, seed=11)
    _, (hit_sel, vals, agg) = check(road, ok, selection("half", 777, seed=12))
    assert agg == (0, 0, 0, 0) and np.all(vals == NULL)


@pytest.mark.parametrize("name", ["lds512", "npj_line", "table_grouped"])
def test_no_probe_rows_with_a_mask_pointer(hj, name):
    """outer == 0: nothing is written, nothing is read of the mask (the buffer holds no mask word at all)"""
    road = Road(hj, name)
    sk, dsel = col(hj, np.zeros(0, np.uint32)), hj.column(np.full(EXTRA_WORDS, ONES, np.uint32))
    dv, db = outputs(hj, 0, "both")
    assert road.call(sk, 0, dsel, dv, db) == (0, 0, 0, 0)
    read_outputs(0, dv, db)
    assert road.call(sk, 0, dsel, dv, dsel) == (0, 0, 0, 0)
    assert np.all(dsel.download() == ONES)


@pytest.mark.parametrize("name", ROADS)
def test_without_a_mask_it_is_the_plain_look_up(hj, name):
    """select_bits = None: bit for bit what hj.lookup / hj.npj_lookup_table give"""
    road = Road(hj, name, seed=6)
    ok = road.probe_keys(4099)
    sk = col(hj, ok)
    dv, db = outputs(hj, 4099, "both")
    dv2, db2 = outputs(hj, 4099, "both")
    mine = road.call(sk, 4099, None, dv, db)
    road.assert_taken()
    plain = road.plain(sk, 4099, dv2, db2)
    assert mine == plain == want_unique(road.ik, road.iv, ok)[2]
    assert np.array_equal(dv.download(), dv2.download()) and np.array_equal(db.download(), db2.download())


@pytest.mark.parametrize("inner", [3000, "beyond_L"])
def test_async_form(hj, inner):
    """d_result in device memory equals the blocking aggregates; two calls back to back on one stream, the second one in place"""
    inner = hj.counter("lookup_lds_rows") + 1 if inner == "beyond_L" else inner
    ik, iv, ok = relations(inner, 9001, 0.5, seed=21)
    ik2, iv2, ok2 = relations(inner, 7003, 0.3, seed=22)
    hj.reserve(inner, len(ok))
    sel, sel2 = selection("half", len(ok), seed=23), selection("eighth", len(ok2), seed=24)
    a = [col(hj, x) for x in (ik, iv, ok)] + [hj.column(mask_words(sel))]
    b = [col(hj, x) for x in (ik2, iv2, ok2)] + [hj.column(mask_words(sel2))]
    (dva, dba), (dvb, _) = outputs(hj, len(ok), "both"), outputs(hj, len(ok2), "vals")
    blocking = tuple(hj.lookup_selected(a[0], a[1], inner, a[2], len(ok), select_bits=a[3]))
    ra, rb = hj.column(4, np.uint64), hj.column(4, np.uint64)
    hj.lookup_selected_async(a[0], a[1], inner, a[2], len(ok), None, a[3], dva, dba, ra)
    hj.lookup_selected_async(b[0], b[1], inner, b[2], len(ok2), None, b[3], dvb, b[3], rb)
    hj.get_async_status()
    hit_a, vals_a, agg_a = want_selected(ik, iv, ok, sel)
    hit_b, vals_b, agg_b = want_selected(ik2, iv2, ok2, sel2)
    gva, gba = read_outputs(len(ok), dva, dba)
    gvb, _ = read_outputs(len(ok2), dvb, None)
    assert tuple(int(x) for x in ra.download()) == agg_a == blocking
    assert tuple(int(x) for x in rb.download()) == agg_b
    assert np.array_equal(gva, vals_a) and np.array_equal(gba, hit_a) and np.array_equal(gvb, vals_b)
    got = b[3].download()
    assert np.array_equal(got[:-EXTRA_WORDS], pack(hit_b)) and np.all(got[-EXTRA_WORDS:] == ONES)


def test_refusals(hj):
    ik, iv, ok = relations(100, 300, 0.5, seed=41)
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    words = np.concatenate([pack(selection("half", 4096, seed=42)), np.full(EXTRA_WORDS, ONES, np.uint32)])      # room for the shifted pointers
    dsel = hj.column(words)
    dv, db = outputs(hj, len(ok), "both")
    dt = hj.column(1024, np.uint64)
    hj.npj_build(rk, rv, len(ik), dt, 1024, NPJ_FACTOR)
    d_res = hj.column(4, np.uint64)
    calls = [lambda **kw: hj.lookup_selected(rk, rv, len(ik), sk, len(ok), vals_out=dv, **kw),
             lambda **kw: hj.lookup_selected_async(rk, rv, len(ik), sk, len(ok), None, kw["select_bits"], dv, kw["match_bits"], d_res),
             lambda **kw: hj.npj_lookup_table_selected(sk, len(ok), dt, 1024, NPJ_FACTOR, vals_out=dv, **kw)]
    for call in calls:
        # a mask 4 bytes off alignment
        with pytest.raises(HjGpuError) as e:
            call(select_bits=dsel.ptr + 4, match_bits=db)
        assert e.value.status == api.EALIGN
        # match_bits inside the mask's range, 16 bytes on: neither disjoint nor the mask itself
        with pytest.raises(HjGpuError) as e:
            call(select_bits=dsel, match_bits=dsel.ptr + 16)
        assert e.value.status == api.EINVAL and "overlap" in str(e.value), str(e.value)
    # every join-mode flag, by name, in both forms
    for name, flag in MODE_FLAGS:
        p = NpjParams(); p.flags = flag
        with pytest.raises(HjGpuError) as e:
            hj.lookup_selected(rk, rv, len(ik), sk, len(ok), params=p, select_bits=dsel, vals_out=dv, match_bits=db)
        assert e.value.status == api.EINVAL and name in str(e.value) and "hjgpu_lookup_selected" in str(e.value), (name, str(e.value))
        with pytest.raises(HjGpuError) as e:
            hj.lookup_selected_async(rk, rv, len(ik), sk, len(ok), p, dsel, dv, db, d_res)
        assert e.value.status == api.EINVAL and name in str(e.value) and "hjgpu_lookup_selected_async" in str(e.value), (name, str(e.value))
    # a refused call writes nothing
    assert np.all(dv.download() == CANARY) and np.all(db.download() == CANARY) and np.array_equal(dsel.download(), words)
    # HJGPU_FLAG_UNIQUE is accepted and changes nothing
    sel = np.unpackbits(words[:10].view(np.uint8), bitorder="little")[:len(ok)].astype(bool)
    p = NpjParams(); p.flags = api.FLAG_UNIQUE
    assert tuple(hj.lookup_selected(rk, rv, len(ik), sk, len(ok), params=p, select_bits=dsel)) == want_selected(ik, iv, ok, sel)[2]


@pytest.mark.parametrize("name", ROADS)
def test_stats(hj, name):
    """as after the plain look-ups: no close_gaps; LDS road fanout 1 x 1, no buckets, ms_build 0; NPJ road the table's buckets and a build"""
    road = Road(hj, name, seed=8)
    ok = road.probe_keys(20011)
    check(road, ok, selection("eighth", 20011, seed=8), "eighth")
    s = hj.stats()
    assert s["ms_close_gaps"] == 0 and s["ms_join"] > 0 and s["ms_total"] >= s["ms_join"], s
    if name in ("lds512", "lds1024", "chained"):
        assert s["ms_build"] == 0 and s["fanout1"] == 1 and s["fanout2"] == 1 and s["buckets"] == 0, s
    elif not road.table:
        assert s["ms_build"] > 0 and s["buckets"] > 0, s
        if name != "npj_refhash":
            assert s["buckets"] == (int(road.inner / 0.25) + 7) & ~7, s
