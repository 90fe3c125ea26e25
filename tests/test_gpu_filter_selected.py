"""GPU tests of hjgpu_filter_selected / hjgpu_filter_selected_async: range predicates over up to four uint32 columns into a bitmap in
d_match_bits' layout, under an optional selection mask, in place or not, with the exact count of the passing rows.

Expected values come from numpy: row i passes when it is selected and lo <= x <= hi holds on every column (uint32 order, int32 order under
PRED_SIGNED, inverted under PRED_NOT); the bitmap is np.packbits of that, the count its popcount.  Exact equality.  Every output bitmap is
followed by canary words that must not change, the mask by all-ones words that nothing may read; mask (where it is not the output) and
columns come back unchanged; the last word's high bits are 0.  A column's values are drawn from around its predicate's bounds - lo - 1, lo,
hi, hi + 1 and a few more - independently per column, so every bound is hit from both sides and later columns pass where earlier ones fail
and the reverse.  The grid-seam sizes are derived from the context's counter "filter_step_rows", never hard-coded.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import HjGpuError, PRED_NOT, PRED_SIGNED
from test_gpu_npj_lookup import relations, outputs
from test_gpu_lookup_selected import hj, pack, mask_words, selection, col, want_selected        # noqa: F401 (hj: the fixture)

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF                       # HJGPU_NULL_VAL
CANARY = 0xA5A5A5A5
ONES = 0xFFFFFFFF
EXTRA = 4                               # canary words behind an output bitmap (the mask's all-ones words when in place)
M32 = (1 << 32) - 1
MASKS = ["null", "ones", "zeros", "half", "eighth", "alternating_words", "first_row", "last_row", "garbage_tail"]
TAILS = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]
FORMS_N = 5 * 2048 + 77

# the predicate forms: (lo, hi, flags)
PLAIN = (100, 200, 0)
EQUAL = (7, 7, 0)
NOT_EQUAL = (7, 7, PRED_NOT)
SIGNED_ACROSS_0 = (-5 & M32, 5, PRED_SIGNED)
NOT_SIGNED = (-5 & M32, 5, PRED_SIGNED | PRED_NOT)
EMPTY = (200, 100, 0)
EMPTY_NOT = (200, 100, PRED_NOT)
FULL = (0, M32, 0)
SIGNED_EMPTY = (5, -5 & M32, PRED_SIGNED)               # 5 > -5 in int32 order (in uint32 order it would be a huge range)
SIGNED_FULL = (0x80000000, 0x7FFFFFFF, PRED_SIGNED)
UP_TO_MAX = (0xFFFFFF00, M32, 0)
FORMS = {"plain": PLAIN, "equal": EQUAL, "not_equal": NOT_EQUAL, "signed_across_0": SIGNED_ACROSS_0, "not_signed": NOT_SIGNED, "empty": EMPTY,
         "empty_not": EMPTY_NOT, "full": FULL, "signed_empty": SIGNED_EMPTY, "signed_full": SIGNED_FULL, "up_to_max": UP_TO_MAX}


def holds(x, pred):
    """the definition, in Python integers' order"""
    lo, hi, flags = pred
    xi = x.astype(np.int64)
    if flags & PRED_SIGNED:
        xi = x.view(np.int32).astype(np.int64)
        lo, hi = (lo ^ 0x80000000) - 0x80000000, (hi ^ 0x80000000) - 0x80000000
    inside = (xi >= lo) & (xi <= hi)
    return ~inside if flags & PRED_NOT else inside


def column_for(pred, n, seed):
    """n values from around the predicate's bounds: lo - 1, lo, hi, hi + 1 (modulo 2^32) twice as often as the rest"""
    lo, hi, _ = pred
    near = [(lo - 1) & M32, lo, hi, (hi + 1) & M32]
    pool = np.array(near + near + [(lo + 1) & M32, (hi - 1) & M32, ((lo + hi) // 2) & M32, 0, M32, 0x7FFFFFFF, 0x80000000], np.uint32)
    return pool[np.random.default_rng(seed).integers(0, len(pool), n)]


def columns_for(preds, n, seed):
    return [column_for(p, n, seed + 17 * i) for i, p in enumerate(preds)]


def sel_of(kind, n, seed):
    return np.ones(n, bool) if kind == "null" else selection(kind, n, seed)


def passing(cols, preds, sel):
    ok = sel.copy()
    for x, p in zip(cols, preds):
        ok &= holds(x, p)
    return ok


def check_bitmap(raw, ok, tail, what):
    """raw: the downloaded output buffer; ok: the rows that pass; tail: what the words behind the bitmap must still hold"""
    n, words = len(ok), (len(ok) + 31) // 32
    want = pack(ok)
    assert np.all(raw[words:] == tail), (what, "a word at index >= (n + 31) / 32 was written")
    bad = np.flatnonzero(raw[:words] != want)
    assert len(bad) == 0, (what, "bitmap words", bad[:8], [hex(int(x)) for x in raw[:words][bad[:4]]], [hex(int(x)) for x in want[bad[:4]]])
    if n % 32:
        assert int(raw[words - 1]) >> (n % 32) == 0, (what, "the last word's high bits")


def run(hj, cols, preds, sel, kind="null", in_place=False, dcols=None):
    """one blocking call with a bitmap and a count, checked against numpy in every respect; returns (count, the bitmap's words)"""
    n = len(sel)
    ok = passing([c[:n] for c in cols], preds, sel)
    words = mask_words(sel, kind) if kind != "null" else None
    assert not (in_place and words is None)
    dsel = hj.column(words) if words is not None else None
    own = dcols is None
    dcols = [col(hj, c) for c in cols] if own else dcols
    nwords = (n + 31) // 32
    dout = dsel if in_place else hj.column(np.full(nwords + EXTRA, CANARY, np.uint32))
    got = hj.filter_selected(dsel, n, dcols, preds, dout)
    what = (kind, "n", n, "in place" if in_place else "out of place", preds)
    print(*what, "count", got, "want", int(ok.sum()))
    raw = dout.download()
    check_bitmap(raw, ok, ONES if in_place else CANARY, what)
    assert got == int(ok.sum()), (what, got, int(ok.sum()))
    if dsel is not None and not in_place:
        assert np.array_equal(dsel.download(), words), (what, "the mask was written")
    if own:
        for h, d in zip(cols, dcols):
            if len(h):
                assert np.array_equal(d.download(), h), (what, "a column was written")
    for d in ([dsel] if dsel is not None else []) + ([dout] if not in_place else []) + (dcols if own else []):
        d.free()
    return got, raw[:nwords]


@pytest.mark.parametrize("kind", MASKS)
def test_tails(hj, kind):
    """the partial vector, the partial word, garbage bits at >= n, no row at all; two predicates"""
    preds = [PLAIN, SIGNED_ACROSS_0]
    for n in TAILS:
        run(hj, columns_for(preds, n, seed=n), preds, sel_of(kind, n, seed=n + 3), kind)
        if kind != "null":
            run(hj, columns_for(preds, n, seed=n), preds, sel_of(kind, n, seed=n + 3), kind, in_place=True)


@pytest.mark.parametrize("kind", ["half", "alternating_words"])
def test_grid_seams(hj, kind):
    """n = 2 S + t, S the rows the whole grid covers per iteration: every workgroup has two iterations, the first ones a tail; three predicates"""
    S = hj.counter("filter_step_rows")
    assert S % 2048 == 0 and 2048 <= S <= 1 << 24, S
    preds = [PLAIN, NOT_SIGNED, (6, 8, 0)]
    nmax = 2 * S + 255
    cols = columns_for(preds, nmax, seed=5)
    dcols = [hj.column(c) for c in cols]
    allsel = selection(kind, nmax, seed=6)                          # (both kinds: a prefix of the selection is the selection of the prefix)
    for t in (0, 1, 33, 255):
        n = 2 * S + t
        sel = allsel[:n].copy()
        got, _ = run(hj, cols, preds, sel, kind, dcols=dcols)
        assert 0 < got < int(sel.sum())
    for h, d in zip(cols, dcols):
        assert np.array_equal(d.download(), h), "a column was written"


@pytest.mark.parametrize("npreds", [1, 2, 3, 4])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_predicate_forms(hj, npreds, form):
    """every form in every position that npreds has, beside plain ranges; a mask and none"""
    n = FORMS_N
    for at in range(npreds):
        preds = [PLAIN] * npreds
        preds[at] = FORMS[form]
        cols = columns_for(preds, n, seed=at)
        for kind in ("null", "half"):
            got, _ = run(hj, cols, preds, sel_of(kind, n, seed=9), kind)
            if form in ("empty", "signed_empty"):
                assert got == 0
        if form in ("empty_not", "full", "signed_full") and npreds == 1:
            assert run(hj, cols, preds, sel_of("null", n, 0))[0] == n


def test_predicate_tuples_and_structs(hj):
    """(lo, hi), (lo, hi, flags) with negative bounds, and api.Predicate give the same call"""
    n = 4099
    x = column_for(SIGNED_ACROSS_0, n, seed=1)
    d = hj.column(x)
    want = int(holds(x, SIGNED_ACROSS_0).sum())
    assert hj.filter_selected(None, n, [d], [(-5, 5, PRED_SIGNED)]) == want
    assert hj.filter_selected(None, n, [d], [api.Predicate(-5 & M32, 5, PRED_SIGNED, 0)]) == want
    assert hj.filter_selected(None, n, [d], [(0, 5)]) == int(holds(x, (0, 5, 0)).sum())
    with pytest.raises(ValueError):
        hj.filter_selected(None, n, [d, d], [(0, 5)])
    with pytest.raises(ValueError):
        hj.filter_selected_async(None, n, [d], [(0, 5), (1, 2)], None, None)


def test_the_same_column_twice(hj):
    """two NOT ranges on one column: x not in [100, 120] and x not in [180, 200], under a third range on it"""
    n = FORMS_N
    preds = [(90, 210, 0), (100, 120, PRED_NOT), (180, 200, PRED_NOT)]
    x = (np.random.default_rng(3).integers(80, 220, n)).astype(np.uint32)
    run(hj, [x, x, x], preds, sel_of("half", n, 4), "half")
    d = hj.column(x)                                                # the very same device column three times
    sel = sel_of("eighth", n, 5)
    got, _ = run(hj, [x, x, x], preds, sel, "eighth", dcols=[d, d, d])
    assert got == int((sel & (x >= 90) & (x <= 210) & ~((x >= 100) & (x <= 120)) & ~((x >= 180) & (x <= 200))).sum())
    assert np.array_equal(d.download(), x)


def test_null_vals_in_a_looked_up_column(hj):
    """HJGPU_NULL_VAL is the ordinary value 0xFFFFFFFF: an unsigned range below it drops the unmatched rows, [NULL, NULL] keeps them alone,
    a signed range sees them as -1"""
    n = FORMS_N
    rng = np.random.default_rng(7)
    x = rng.integers(0, 50, n).astype(np.uint32)
    x[rng.random(n) < 0.3] = NULL
    sel = sel_of("half", n, 8)
    for pred, want in [((0, 49, 0), sel & (x != NULL)), ((NULL, NULL, 0), sel & (x == NULL)), ((0, NULL - 1, 0), sel & (x != NULL)),
                       ((-1 & M32, 10, PRED_SIGNED), sel & ((x == NULL) | (x <= 10))), ((NULL, NULL, PRED_NOT), sel & (x != NULL))]:
        got, _ = run(hj, [x], [pred], sel, "half")
        assert got == int(want.sum()), pred


def test_in_place_count_only_and_bits_only(hj):
    n = FORMS_N
    preds = [PLAIN, EQUAL, NOT_SIGNED]
    cols = columns_for(preds, n, seed=21)
    for kind in ("half", "eighth", "garbage_tail", "ones"):
        sel = sel_of(kind, n, seed=22)
        a, wa = run(hj, cols, preds, sel, kind)
        b, wb = run(hj, cols, preds, sel, kind, in_place=True)
        assert a == b and np.array_equal(wa, wb)
        # the count alone; the bitmap alone (the C entry point: the binding always passes the blocking form a count)
        words = mask_words(sel, kind)
        dsel, dcols = hj.column(words), [hj.column(c) for c in cols]
        assert hj.filter_selected(dsel, n, dcols, preds, None) == a
        dout = hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32))
        arr = (api.C.c_void_p * 3)(*[d.ptr for d in dcols])
        prs = (api.Predicate * 3)(*[api.Predicate.of(p) for p in preds])
        assert hj.lib.hjgpu_filter_selected(hj.handle, dsel.ptr, n, 3, arr, prs, dout.ptr, None, None) == api.OK
        check_bitmap(dout.download(), passing(cols, preds, sel), CANARY, (kind, "bits only"))
        # the _async form with either output NULL
        d_count = hj.column(np.full(2, 77, np.uint64), np.uint64)
        hj.filter_selected_async(dsel, n, dcols, preds, None, d_count)
        dout2 = hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32))
        hj.filter_selected_async(dsel, n, dcols, preds, dout2, None)
        hj.synchronize()
        assert [int(v) for v in d_count.download()] == [a, 77]
        check_bitmap(dout2.download(), passing(cols, preds, sel), CANARY, (kind, "async bits only"))
        assert np.array_equal(dsel.download(), words)


def test_n_zero_accepts_null(hj):
    assert hj.filter_selected(None, 0, [None], [(1, 2)], None) == 0
    d_count = hj.column(np.full(1, 77, np.uint64), np.uint64)
    hj.filter_selected_async(None, 0, [None, None], [(1, 2), (3, 4)], None, d_count)
    hj.synchronize()
    assert int(d_count.download()[0]) == 0
    assert hj.lib.hjgpu_filter_selected(hj.handle, None, 0, 1, None, None, None, None, None) == api.OK


def test_enqueue_only(hj):
    """two filters of different sizes and predicates back to back on one stream, no host wait in between, into two device count words; the
    status of the join before them stays what it was"""
    ik, iv, ok_ = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0                                                      # the preceding join's status: HJGPU_EZEROKEY
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok_)
    dv, db = outputs(hj, len(ok_), "both")
    d_res = hj.column(4, np.uint64)
    hj.reserve(len(ik), len(ok_))
    hj.npj_lookup_async(rk, rv, len(ik), sk, len(ok_), None, dv, db, d_res)
    shapes = [(70_013, "half", [PLAIN, SIGNED_ACROSS_0, NOT_EQUAL]), (20_001, "null", [EQUAL])]
    runs = []
    for n, kind, preds in shapes:
        sel = sel_of(kind, n, seed=n)
        cols = columns_for(preds, n, seed=n + 1)
        runs.append(dict(n=n, preds=preds, ok=passing(cols, preds, sel), dsel=hj.column(mask_words(sel, kind)) if kind != "null" else None,
                         dcols=[hj.column(c) for c in cols], dout=hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32)),
                         d_count=hj.column(np.full(2, 77, np.uint64), np.uint64)))
    hj.filter_selected(None, 0, [None], [(0, 0)])                    # (the context's count word first: making it would wait for the device)
    for r in runs:
        hj.filter_selected_async(r["dsel"], r["n"], r["dcols"], r["preds"], r["dout"], r["d_count"])
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()                                        # waits for the stream
    assert e.value.status == api.EZEROKEY
    for r in runs:
        assert [int(v) for v in r["d_count"].download()] == [int(r["ok"].sum()), 77]
        check_bitmap(r["dout"].download(), r["ok"], CANARY, ("async", r["n"]))


def test_refusals(hj):
    """each returns before anything is enqueued: the canaries, the mask and the columns are untouched afterwards"""
    import torch
    n = 1000
    words = np.concatenate([pack(selection("half", 16384, seed=6)), np.full(4, ONES, np.uint32)])      # room for shifted and overlapping pointers
    dsel = hj.column(words)
    h = [np.arange(n + 64, dtype=np.uint32) % 13, np.arange(n + 64, dtype=np.uint32) % 5]
    din = [hj.column(x) for x in h]
    dout = hj.column(np.full(1024, CANARY, np.uint32))
    d_count = hj.column(np.full(4, 77, np.uint64), np.uint64)
    cols, preds = [d.ptr for d in din], [(1, 7), (0, 2)]

    def blocking(bits=dsel.ptr, n=n, cols=cols, preds=preds, out=dout.ptr, stream=None, **_):
        return hj.filter_selected(bits, n, cols, preds, out, stream=stream)

    def enqueue(bits=dsel.ptr, n=n, cols=cols, preds=preds, out=dout.ptr, count=d_count.ptr, stream=None):
        return hj.filter_selected_async(bits, n, cols, preds, out, count, stream=stream)

    for call in (blocking, enqueue):
        cases = [("misaligned mask", dict(bits=dsel.ptr + 4), api.EALIGN, "d_select_bits"),
                 ("misaligned column", dict(cols=[cols[0], cols[1] + 4]), api.EALIGN, "aligned"),
                 ("misaligned output", dict(out=dout.ptr + 8), api.EALIGN, "d_bits_out"),
                 ("no predicate", dict(cols=[], preds=[]), api.EINVAL, "npreds"),
                 ("five predicates", dict(cols=cols * 2 + cols[:1], preds=preds * 2 + preds[:1]), api.EINVAL, "npreds"),
                 ("null column", dict(cols=[cols[0], None]), api.EINVAL, "null"),
                 ("unknown flag", dict(preds=[(1, 7), (0, 2, 4)]), api.EINVAL, "flag"),
                 ("unknown flag beside known ones", dict(preds=[(1, 7, 3 | 0x80000000), (0, 2)]), api.EINVAL, "flag"),
                 ("reserved not 0", dict(preds=[api.Predicate(1, 7, 0, 1), (0, 2)]), api.EINVAL, "reserved"),
                 ("bitmaps overlapping by one word", dict(out=dsel.ptr + 4 * ((n + 31) // 32 - 1) // 16 * 16), api.EINVAL, "overlaps"),
                 ("output inside a column", dict(out=cols[1] + 16), api.EINVAL, "overlaps"),
                 ("output over a column's last row", dict(out=cols[0] + 4 * (n - 1) // 16 * 16), api.EINVAL, "overlaps")]
        if call is enqueue:
            cases += [("misaligned d_count", dict(count=d_count.ptr + 4), api.EALIGN, "d_count"),
                      ("both outputs null", dict(out=None, count=None), api.EINVAL, "both null"),
                      ("d_count inside the output", dict(count=dout.ptr + 8), api.EINVAL, "overlaps"),
                      ("d_count inside a column", dict(count=cols[0] + 8), api.EINVAL, "overlaps"),
                      ("d_count inside the mask", dict(count=dsel.ptr + 8), api.EINVAL, "overlaps")]
        for name, kw, status, text in cases:
            with pytest.raises(HjGpuError) as e:
                call(**kw)
            assert e.value.status == status, (name, str(e.value))
            assert text in str(e.value), (name, str(e.value))
        # a capturing stream
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
    # (the binding always passes the blocking form a count: the C entry point itself refuses both outputs NULL)
    arr = (api.C.c_void_p * 2)(*cols)
    prs = (api.Predicate * 2)(*[api.Predicate.of(p) for p in preds])
    assert hj.lib.hjgpu_filter_selected(hj.handle, dsel.ptr, n, 2, arr, prs, None, None, None) == api.EINVAL
    assert b"both null" in hj.lib.hjgpu_last_error(hj.handle)
    assert hj.lib.hjgpu_filter_selected(hj.handle, dsel.ptr, n, 2, None, prs, dout.ptr, None, None) == api.EINVAL
    hj.synchronize()
    assert np.all(dout.download() == CANARY), "a refused call wrote the output"
    assert np.array_equal(dsel.download(), words) and all(np.array_equal(d.download(), x) for d, x in zip(din, h))
    assert [int(x) for x in d_count.download()] == [77] * 4
    # the same pointers, accepted: plain integers as well as DeviceColumns; the bitmaps side by side without a shared word
    sel = np.unpackbits(words[:(n + 31) // 32].view(np.uint8), bitorder="little")[:n].astype(bool)
    ok = passing([x[:n] for x in h], [(1, 7, 0), (0, 2, 0)], sel)
    assert blocking() == int(ok.sum()) > 0
    check_bitmap(dout.download(), ok, CANARY, "accepted")
    assert blocking(out=dsel.ptr + 4 * ((n + 31) // 32 + 3) // 16 * 16) == int(ok.sum())


def test_stats(hj):
    S = hj.counter("filter_step_rows")
    n = S + 4099
    preds = [PLAIN, EQUAL]
    run(hj, columns_for(preds, n, seed=3), preds, sel_of("half", n, seed=5), "half")
    s = hj.stats()
    print(s)
    assert s["ms_total"] >= s["ms_join"] > 0, s
    assert s["ms_histogram"] > 0 and s["ms_total"] >= (s["ms_histogram"] + s["ms_join"]) * (1 - 1e-5), s
    for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_build", "ms_close_gaps", "ms_inner_wait"):
        assert s[k] == 0, (k, s)
    assert s["fanout1"] == 0 and s["fanout2"] == 0 and s["buckets"] == 0 and s["groups"] == 0, s


def test_a_small_star_query(hj):
    """WHERE discount BETWEEN 1 AND 3 AND quantity < 25 AND d.attr BETWEEN 5 AND 30 GROUP BY d.attr, SUM(measure): a filter on two fact
    columns makes the bitmap, a selected look-up against an LDS-road dimension narrows it in place, a filter on the looked-up value column
    narrows it again, group_sum ends the query; the same in numpy, as the sorted set of (key, count, sum)"""
    n = 300_007
    rng = np.random.default_rng(61)
    dk, dv, fk = relations(1000, n, 0.5, seed=62)
    dv = (dv % 40).astype(np.uint32)
    discount, quantity = rng.integers(0, 11, n).astype(np.uint32), rng.integers(1, 51, n).astype(np.uint32)
    measure = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    assert len(dk) <= hj.counter("lookup_lds_rows")
    ddisc, dquant, dmeas, dfk, ddk, ddv = [hj.column(x) for x in (discount, quantity, measure, fk, dk, dv)]
    bits = hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32))
    vals, _ = outputs(hj, n, "vals")
    fact = (discount >= 1) & (discount <= 3) & (quantity < 25)
    assert hj.filter_selected(None, n, [ddisc, dquant], [(1, 3), (0, 24)], bits) == int(fact.sum())
    hj.lookup_selected(ddk, ddv, len(dk), dfk, n, select_bits=bits, vals_out=vals, match_bits=bits)
    s = hj.stats()
    assert s["fanout1"] == 1 and s["fanout2"] == 1 and s["buckets"] == 0, s       # the LDS road
    hit, looked, _ = want_selected(dk, dv, fk, fact)
    final = hit & (looked >= 5) & (looked <= 30)
    assert hj.filter_selected(bits, n, [vals], [(5, 30)], bits) == int(final.sum())
    check_bitmap(bits.download(), final, CANARY, "chain")
    # the unmatched rows carry HJGPU_NULL_VAL: the same range over the first bitmap drops them by itself
    bits1 = hj.column(mask_words(fact))
    assert (looked[fact] == NULL).any()
    assert hj.filter_selected(bits1, n, [vals], [(5, 30)], None) == int(final.sum())
    keys, inv = np.unique(looked[final], return_inverse=True)
    counts = np.bincount(inv.reshape(-1), minlength=len(keys)).astype(np.uint64)
    sums = np.zeros(len(keys), np.uint64)
    np.add.at(sums, inv.reshape(-1), measure[final].astype(np.uint64))
    J = len(keys)
    assert J == 26
    kout, cout, sout = hj.column(J, np.uint32), hj.column(J, np.uint64), hj.column(J, np.uint64)
    assert hj.group_sum(bits, n, [vals], [dmeas], [kout], [sout], cout, capacity=J) == J
    gk, gc, gs = kout.download(), cout.download(), sout.download()
    order = np.argsort(gk)
    assert np.array_equal(gk[order], keys) and np.array_equal(gc[order], counts) and np.array_equal(gs[order], sums)
