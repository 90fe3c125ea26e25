"""GPU tests of hjgpu_compact_selected / hjgpu_compact_selected_async: the ordered compaction of up to 8 uint32 columns, and optionally the
row numbers, by a bitmap in d_match_bits' layout.

Expected values come from numpy (col[sel], np.flatnonzero(sel)), exact equality.  Every output is longer than `capacity` and pre-filled with a
canary: nothing at index >= min(J, capacity) may change.  The mask is followed by all-ones words that nothing may read; mask and inputs come
back unchanged.  The shapes are derived from the context's counters "compact_ranges" (G) and "compact_chunk_rows" (C), never hard-coded.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import HjGpuError
from helpers import numpy_join
from test_gpu_npj_lookup import relations, outputs, read_outputs
from test_gpu_lookup_selected import hj, pack, mask_words, selection, col, want_selected        # noqa: F401 (hj: the fixture)

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF
CANARY = 0xA5A5A5A5
ONES = 0xFFFFFFFF
EXTRA = 64
MULT = [0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F, 0x165667B1, 0x7FEB352D, 0x846CA68B, 0x2545F491]
MASKS = ["ones", "zeros", "half", "eighth", "alternating_words", "first_row", "last_row", "garbage_tail"]
SEAM_MASKS = ["half", "sixtyfourth", "first_row_of_every_range", "last_row_of_every_range", "first_range", "last_range", "alternating_words"]


def geometry(hj):
    G, C = hj.counter("compact_ranges"), hj.counter("compact_chunk_rows")
    assert 1 <= G <= 2048 and C >= 256 and C % 256 == 0, (G, C)
    return G, C


def tails(hj):
    _, C = geometry(hj)
    return [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, C - 1, C, C + 1]


def data(c, n):
    """input column c: every row a different value, different in every column"""
    return (np.arange(n, dtype=np.uint64) * MULT[c % 8] + 7 * c + 1).astype(np.uint32)


def canary(hj, rows):
    return hj.column(np.full(rows + EXTRA, CANARY, np.uint32))


def compact(hj, sel, kind="half", ncols=3, rows=True, capacity=None, cols=None, overflow=False):
    """one blocking compaction checked against numpy in every respect; returns the count"""
    n = len(sel)
    want_rows = np.flatnonzero(sel).astype(np.uint32)
    J = len(want_rows)
    capacity = J if capacity is None else capacity
    host = [data(c, n) for c in range(ncols)] if cols is None else cols
    words = mask_words(sel, kind)
    dsel = hj.column(words)
    din = [col(hj, h) for h in host]
    dout = [canary(hj, capacity) for _ in host]
    drows = canary(hj, capacity) if rows else None
    try:
        got = hj.compact_selected(dsel, n, din, dout, drows, capacity=capacity)
        assert not overflow, "HJGPU_EOVERFLOW expected"
    except HjGpuError as e:
        assert overflow and e.status == api.EOVERFLOW, str(e)
        got = e.count
    print(kind, "n", n, "ncols", ncols, "rows", rows, "capacity", capacity, "count", got, "want", J)
    assert got == J, (kind, n, got, J)
    m = min(J, capacity)
    for c, (h, d) in enumerate(zip(host, dout)):
        raw = d.download()
        assert np.array_equal(raw[:m], h[sel][:m]), (kind, n, c, np.flatnonzero(raw[:m] != h[sel][:m])[:8])
        assert np.all(raw[m:] == CANARY), (kind, n, c, "written at index >= min(J, capacity)")
    if rows:
        raw = drows.download()
        assert np.array_equal(raw[:m], want_rows[:m]), (kind, n, np.flatnonzero(raw[:m] != want_rows[:m])[:8])
        assert np.all(raw[m:] == CANARY), (kind, n, "d_rows_out written at index >= min(J, capacity)")
    assert np.array_equal(dsel.download(), words), "the mask was written"
    for h, d in zip(host, din):
        if len(h):
            assert np.array_equal(d.download(), h), "an input column was written"
    for d in [dsel] + din + dout + ([drows] if rows else []):
        d.free()
    return got


@pytest.mark.parametrize("kind", MASKS)
def test_tails(hj, kind):
    """the partial vector, the partial word, garbage bits at >= n, one busy workgroup beside G - 1 empty ones"""
    for n in tails(hj):
        compact(hj, selection(kind, n, seed=n + 3), kind)


def seam_selection(kind, n, G, C, seed):
    chunks = (n + C - 1) // C
    rr = (chunks + G - 1) // G * C                      # rows per range (csrc/compact_layout.hpp)
    sel = np.zeros(n, bool)
    if kind == "sixtyfourth":
        sel = np.random.default_rng(seed).random(n) < 1 / 64
    elif kind == "first_row_of_every_range":
        sel[::rr] = True
    elif kind == "last_row_of_every_range":
        sel[rr - 1::rr] = True
        sel[n - 1] = True
    elif kind == "first_range":
        sel[:rr] = True
    elif kind == "last_range":
        sel[(n - 1) // rr * rr:] = True
    else:
        sel = selection(kind, n, seed)
    return sel


@pytest.mark.parametrize("kind", SEAM_MASKS)
def test_range_seams(hj, kind):
    """every workgroup has at least two iterations and a predecessor"""
    G, C = geometry(hj)
    for t in [0, 1, 33, C - 1]:
        n = 2 * G * C + t
        compact(hj, seam_selection(kind, n, G, C, seed=t + 5), kind if kind == "alternating_words" else "half", ncols=2)


@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("ncols", [0, 1, 3, 4, 5, 8])
def test_shapes_of_the_call(hj, ncols, rows):
    """5 and 8 columns take the second launch; no columns and no row numbers is the count alone"""
    _, C = geometry(hj)
    n = 5 * C + 77
    compact(hj, selection("half", n, seed=ncols), ncols=ncols, rows=rows)


def test_count_only_with_null_arrays(hj):
    _, C = geometry(hj)
    n = 3 * C + 5
    sel = selection("eighth", n, seed=1)
    dsel = hj.column(mask_words(sel))
    assert hj.compact_selected(dsel, n, None, None, None, capacity=0) == int(sel.sum())
    assert hj.compact_selected(dsel, n, [], [], capacity=0) == int(sel.sum())
    # n == 0: the count, and NULL everywhere else
    assert hj.compact_selected(None, 0, None, None, None, capacity=0) == 0
    d_count = hj.column(np.full(1, 77, np.uint64), np.uint64)
    hj.compact_selected_async(None, 0, None, None, None, 0, d_count)
    hj.synchronize()
    assert int(d_count.download()[0]) == 0


def test_the_same_input_column_twice(hj):
    n = 4099
    h = data(0, n)
    compact(hj, selection("half", n, seed=2), cols=[h, h], ncols=2)
    sel = selection("half", n, seed=2)
    dsel, din = hj.column(mask_words(sel)), hj.column(h)
    a, b = canary(hj, n), canary(hj, n)
    J = hj.compact_selected(dsel, n, [din, din], [a, b], capacity=n)
    assert J == int(sel.sum())
    assert np.array_equal(a.download()[:J], h[sel]) and np.array_equal(b.download(), a.download())


def test_capacity(hj):
    _, C = geometry(hj)
    n = 3 * C + 19
    sel = selection("half", n, seed=4)
    J = int(sel.sum())
    assert J > 1
    compact(hj, sel, capacity=J)
    compact(hj, sel, capacity=J - 1, overflow=True)
    compact(hj, sel, capacity=0, overflow=True)
    compact(hj, sel, capacity=J + 100)
    compact(hj, sel, capacity=J - 1, ncols=5, overflow=True)        # the second launch keeps to capacity too
    # the default capacity is the shortest output
    dsel, din = hj.column(mask_words(sel)), hj.column(data(0, n))
    out, rows = hj.column(np.full(J + 8, CANARY, np.uint32)), hj.column(np.full(J - 8, CANARY, np.uint32))
    with pytest.raises(HjGpuError) as e:
        hj.compact_selected(dsel, n, [din], [out], rows)
    assert e.value.status == api.EOVERFLOW and e.value.count == J
    assert np.array_equal(rows.download(), np.flatnonzero(sel)[:J - 8])
    raw = out.download()
    assert np.array_equal(raw[:J - 8], data(0, n)[sel][:J - 8]) and np.all(raw[J - 8:] == CANARY)


def test_refusals(hj):
    """each returns before anything is enqueued: the canaries, the mask and the inputs are untouched afterwards"""
    n = 1000
    words = np.concatenate([pack(selection("half", 8192, seed=6)), np.full(4, ONES, np.uint32)])       # room for shifted and overlapping pointers
    dsel = hj.column(words)
    h = [data(0, n + 64), data(1, n + 64)]
    din = [hj.column(x) for x in h]
    dout = [canary(hj, n), canary(hj, n)]
    drows = canary(hj, n)
    d_count = hj.column(np.full(2, 77, np.uint64), np.uint64)
    ins, outs = [d.ptr for d in din], [d.ptr for d in dout]

    def blocking(bits=dsel.ptr, n=n, ci=ins, co=outs, rows=drows.ptr, capacity=n, count=None):
        return hj.compact_selected(bits, n, ci, co, rows, capacity=capacity)

    def enqueue(bits=dsel.ptr, n=n, ci=ins, co=outs, rows=drows.ptr, capacity=n, count=d_count.ptr):
        return hj.compact_selected_async(bits, n, ci, co, rows, capacity, count)

    for call in (blocking, enqueue):
        cases = [("misaligned mask", dict(bits=dsel.ptr + 4), api.EALIGN, None),
                 ("misaligned input", dict(ci=[ins[0], ins[1] + 4]), api.EALIGN, None),
                 ("misaligned output", dict(co=[outs[0] + 8, outs[1]]), api.EALIGN, None),
                 ("misaligned rows", dict(rows=drows.ptr + 4), api.EALIGN, None),
                 ("null mask", dict(bits=None), api.EINVAL, None),
                 ("nine columns", dict(ci=ins * 4 + ins[:1], co=outs * 4 + outs[:1]), api.EINVAL, None),
                 ("null input entry", dict(ci=[ins[0], None]), api.EINVAL, None),
                 ("null output entry", dict(co=[None, outs[1]]), api.EINVAL, None),
                 ("output over the mask", dict(co=[outs[0], dsel.ptr + 16]), api.EINVAL, "overlaps"),
                 ("rows over the mask", dict(rows=dsel.ptr), api.EINVAL, "overlaps"),
                 ("output over an input", dict(co=[ins[1] + 16, outs[1]]), api.EINVAL, "overlaps"),
                 ("output over an output", dict(co=[outs[0], outs[0] + 16]), api.EINVAL, "overlaps"),
                 ("rows over an output", dict(rows=outs[1] + 4 * (n - 4)), api.EINVAL, "overlaps"),
                 ("2^32 rows with row numbers", dict(n=2**32), api.EINVAL, None)]
        if call is enqueue:
            cases += [("null d_count", dict(count=None), api.EINVAL, None), ("misaligned d_count", dict(count=d_count.ptr + 4), api.EALIGN, None)]
        for name, kw, status, text in cases:
            with pytest.raises(HjGpuError) as e:
                call(**kw)
            assert e.value.status == status, (name, str(e.value))
            assert text is None or text in str(e.value), (name, str(e.value))
    hj.synchronize()
    for d in dout + [drows]:
        assert np.all(d.download() == CANARY), "a refused call wrote an output"
    assert np.array_equal(dsel.download(), words) and all(np.array_equal(d.download(), x) for d, x in zip(din, h))
    assert [int(x) for x in d_count.download()] == [77, 77]
    # the same pointers, accepted: plain integers as well as DeviceColumns
    sel = np.unpackbits(words[:(n + 31) // 32].view(np.uint8), bitorder="little")[:n].astype(bool)
    assert blocking() == int(sel.sum())
    assert np.array_equal(dout[1].download()[:int(sel.sum())], h[1][:n][sel])


def test_enqueue_only(hj):
    """two compactions of different masks and sizes back to back on one stream, no host wait in between; the status of the join before
    them stays what it was"""
    _, C = geometry(hj)
    ik, iv, ok = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0                                                      # the preceding join's status: HJGPU_EZEROKEY
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    dv, db = outputs(hj, len(ok), "both")
    d_res = hj.column(4, np.uint64)
    hj.reserve(len(ik), len(ok))
    hj.npj_lookup_async(rk, rv, len(ik), sk, len(ok), None, dv, db, d_res)
    shapes = [(7 * C + 13, "half", 3, True), (2 * C + 1, "eighth", 5, False)]
    runs = []
    for n, kind, ncols, rows in shapes:
        sel = selection(kind, n, seed=n)
        host = [data(c, n) for c in range(ncols)]
        runs.append(dict(n=n, sel=sel, host=host, dsel=hj.column(mask_words(sel, kind)), din=[hj.column(x) for x in host],
                         dout=[canary(hj, n) for _ in host], drows=canary(hj, n) if rows else None,
                         d_count=hj.column(np.full(1, 77, np.uint64), np.uint64)))
    for r in runs:
        hj.compact_selected_async(r["dsel"], r["n"], r["din"], r["dout"], r["drows"], r["n"], r["d_count"])
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()                                        # waits for the stream
    assert e.value.status == api.EZEROKEY
    for r in runs:
        sel, J = r["sel"], int(r["sel"].sum())
        assert int(r["d_count"].download()[0]) == J
        for x, d in zip(r["host"], r["dout"]):
            raw = d.download()
            assert np.array_equal(raw[:J], x[sel]) and np.all(raw[J:] == CANARY)
        if r["drows"] is not None:
            raw = r["drows"].download()
            assert np.array_equal(raw[:J], np.flatnonzero(sel)) and np.all(raw[J:] == CANARY)


def test_stats(hj):
    G, C = geometry(hj)
    n = 2 * G * C + 33
    compact(hj, selection("half", n, seed=3), ncols=3)
    s = hj.stats()
    print(s)
    assert s["ms_total"] > 0 and s["ms_histogram"] > 0 and s["ms_join"] > 0, s
    assert s["ms_total"] >= (s["ms_histogram"] + s["ms_join"]) * (1 - 1e-5), s
    for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_close_gaps", "ms_build", "ms_inner_wait"):
        assert s[k] == 0, (k, s)
    assert s["fanout1"] == 0 and s["fanout2"] == 0 and s["buckets"] == 0 and s["groups"] == 0, s


def test_the_end_of_a_look_up_chain(hj):
    """two selected look-ups narrow one bitmap in place - the LDS road, then the NPJ road under no_broadcast in a second context - and one
    compaction turns the bitmap, the fact key column and the two value columns into the dense result rows"""
    outer = 100_003
    d1k, d1v, k1 = relations(1000, outer, 0.5, seed=51)
    d2k, d2v, k2 = relations(2000, outer, 0.5, seed=52)
    filt = selection("half", outer, seed=53)
    assert (d1v != NULL).all() and (d2v != NULL).all()
    cols = [col(hj, x) for x in (d1k, d1v, k1, d2k, d2v, k2)]
    bits = hj.column(mask_words(filt))
    dv1, _ = outputs(hj, outer, "vals")
    dv2, _ = outputs(hj, outer, "vals")
    hj.lookup_selected(cols[0], cols[1], len(d1k), cols[2], outer, select_bits=bits, vals_out=dv1, match_bits=bits)
    s = hj.stats()
    assert s["fanout1"] == 1 and s["buckets"] == 0, s                    # d1: the LDS road
    with H.HjGpu(0) as second:
        second.set_option("no_broadcast", 1)
        r2 = tuple(second.lookup_selected(cols[3], cols[4], len(d2k), cols[5], outer, select_bits=bits, vals_out=dv2, match_bits=bits))
        s = second.stats()
        assert s["buckets"] > 0 and s["fanout1"] == 0, s                 # d2: the NPJ road
    hit1, vals1, _ = want_selected(d1k, d1v, k1, filt)
    hit2, vals2, agg2 = want_selected(d2k, d2v, k2, hit1)
    assert r2 == agg2
    J = int(hit2.sum())
    out = [canary(hj, J) for _ in range(3)]
    rows = canary(hj, J)
    count = hj.compact_selected(bits, outer, [cols[2], dv1, dv2], out, rows, capacity=J)
    assert count == r2[0] == J
    got = [d.download() for d in out]
    for g, want in zip(got, (k1[hit2], vals1[hit2], vals2[hit2])):
        assert np.array_equal(g[:J], want) and np.all(g[J:] == CANARY)
    assert not (got[1][:J] == NULL).any() and not (got[2][:J] == NULL).any()
    assert np.array_equal(rows.download()[:J], np.flatnonzero(hit2))


def test_in_front_of_a_join(hj):
    """probe keys and payloads compacted by a filter bitmap, then hjgpu_phj on the dense columns: the join of the numpy-filtered columns"""
    inner, outer = 5000, 200_003
    ik, iv, ok = relations(inner, outer, 0.5, seed=61)
    ov = data(3, outer)
    sel = selection("half", outer, seed=62)
    J = int(sel.sum())
    rk, rv, sk, sv = (col(hj, x) for x in (ik, iv, ok, ov))
    dsel = hj.column(mask_words(sel))
    ck, cv = canary(hj, J), canary(hj, J)
    assert hj.compact_selected(dsel, outer, [sk, sv], [ck, cv], capacity=J) == J
    got = tuple(hj.phj(rk, rv, inner, ck, cv, J))
    assert got == numpy_join(ik, iv, ok[sel], ov[sel]), got
