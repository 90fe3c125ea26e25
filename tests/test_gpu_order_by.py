"""GPU tests of hjgpu_order_by / hjgpu_order_by_async: ORDER BY up to four keys - uint32 or uint64, each ascending or descending, unsigned
or two's complement - with LIMIT over the rows a bitmap in d_match_bits' layout selects (NULL: every row), ties broken by ascending row
number.

The model is np.lexsort over the selected rows with the row number as the last tie-break; a key enters it as its dense rank in the order
of its own numpy dtype (int32 / int64 under ORDER_SIGNED), negated under ORDER_DESC.  The result is fully determined, so every
comparison is for equality.  One helper, order(), checks every call in every respect: the count; every output - longer than
min(limit, n) and pre-filled with a canary - equal to the model below min(J, limit) and untouched behind it; the mask, followed by
all-ones words that nothing may read, and every input, followed by a sentinel behind row n, read back unchanged.  The shapes come from the
context's counters "order_lds_rows" (L), "order_ranges" and "order_chunk_rows", never hard-coded.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import itertools

import numpy as np
import pytest

from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import ORDER_DESC as DESC, ORDER_SIGNED as SIGNED, ORDER_WIDE as WIDE
from test_gpu_lookup_selected import hj, mask_words, selection        # noqa: F401 (hj: the fixture)
from test_gpu_group_sum import MASKS, sel_of

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF                       # HJGPU_NULL_VAL
CANARY32 = 0xA5A5A5A5
CANARY64 = 0xA5A5A5A5A5A5A5A5
SENTINEL32 = 0x5EEDBEEF
SENTINEL64 = 0x5EEDBEEF5EEDBEEF
EXTRA = 64
EDGES = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]


def geometry(hj):
    """(L, ranges, chunk rows, the smallest n with at least two ranges of at least two chunks)"""
    L, ranges, chunk = hj.counter("order_lds_rows"), hj.counter("order_ranges"), hj.counter("order_chunk_rows")
    assert L >= 4096 and ranges >= 2 and chunk >= 256, (L, ranges, chunk)
    two_by_two = ranges * chunk + 1 if ranges >= 3 else 3 * chunk + 1
    assert L < two_by_two <= 1 << 23, (L, two_by_two)
    return L, ranges, chunk, two_by_two


def dtype_of(flags):
    return np.uint64 if flags & WIDE else np.uint32


def model(keys, sel):
    """the selected row numbers in the wanted order: np.lexsort, the row number the last tie-break"""
    rows = np.flatnonzero(sel)
    ranks = []
    for a, flags in keys:
        x = np.asarray(a, dtype_of(flags))[rows]
        if flags & SIGNED:
            x = x.view(np.int64 if flags & WIDE else np.int32)
        r = np.unique(x, return_inverse=True)[1].reshape(-1).astype(np.int64)
        ranks.append(-r if flags & DESC else r)
    return rows[np.lexsort((rows,) + tuple(reversed(ranks)))].astype(np.uint32)


def with_sentinel(a):
    a = np.ascontiguousarray(a)
    return np.concatenate([a, np.full(EXTRA, SENTINEL64 if a.dtype.itemsize == 8 else SENTINEL32, a.dtype)])


def canary(hj, rows, dtype):
    return hj.column(np.full(rows + EXTRA, CANARY64 if np.dtype(dtype).itemsize == 8 else CANARY32, dtype), dtype)


def check_column(raw, want, m, what):
    assert np.array_equal(raw[:m], want[:m]), (what, "differs first at", int(np.flatnonzero(raw[:m] != want[:m])[0]), raw[:m][:8], want[:m][:8])
    assert np.all(raw[m:] == (CANARY64 if raw.dtype.itemsize == 8 else CANARY32)), (what, "written at index >= min(J, limit)")


class Call:
    """the device side of one call: the inputs uploaded (a column that appears several times, once), the outputs pre-filled"""

    def __init__(self, hj, n, keys, sel, kind, cols, rows, limit, want=None):
        self.hj, self.n, self.keys, self.sel, self.kind, self.cols, self.limit = hj, n, keys, sel, kind, cols, limit
        self.words = mask_words(sel, kind) if kind != "null" else None
        self.dsel = hj.column(self.words) if self.words is not None else None
        self.host, self.dev = {}, {}
        for a in [k for k, _ in keys] + list(cols):
            if id(a) not in self.dev:
                self.host[id(a)] = with_sentinel(a)
                self.dev[id(a)] = hj.column(self.host[id(a)], a.dtype)
        m_alloc = min(n if limit is None else limit, n)
        self.outs = [canary(hj, m_alloc, c.dtype) for c in cols]
        self.rows_out = canary(hj, m_alloc, np.uint32) if rows else None
        self.want = model(keys, sel) if want is None else want

    def args(self):
        return (self.dsel, self.n, [(self.dev[id(k)], f) for k, f in self.keys], [self.dev[id(c)] for c in self.cols], self.outs, self.rows_out, self.limit)

    def check(self, got):
        J = len(self.want)
        assert got == J == int(self.sel.sum()), (self.kind, self.n, "count", got, "want", J)
        m = min(J, self.n if self.limit is None else self.limit)
        if self.rows_out is not None:
            check_column(self.rows_out.download(), self.want, m, (self.kind, self.n, "rows_out"))
        for c, (d, h) in enumerate(zip(self.outs, self.cols)):
            check_column(d.download(), h[self.want[:m]], m, (self.kind, self.n, "column", c))
        if self.words is not None:
            assert np.array_equal(self.dsel.download(), self.words), "the mask was written"
        for key, d in self.dev.items():
            assert np.array_equal(d.download(), self.host[key]), "an input column was written"

    def free(self):
        for d in ([self.dsel] if self.dsel is not None else []) + list(self.dev.values()) + self.outs + ([self.rows_out] if self.rows_out is not None else []):
            d.free()


def order(hj, keys, sel, kind="null", cols=(), rows=True, limit=None, want=None):
    """one blocking call checked against the model in every respect; keys: [(host column, flags)], cols: host columns.  Returns J"""
    call = Call(hj, len(sel), keys, sel, kind, list(cols), rows, limit, want)
    got = hj.order_by(*call.args())
    call.check(got)
    call.free()
    return got


def random_keys(n, flags, seed, distinct=None):
    """a key column per entry of flags; distinct: that many values at most, so that ties reach the later keys and the row number"""
    rng = np.random.default_rng(seed)
    out = []
    for f in flags:
        x = rng.integers(0, 1 << 64, n, dtype=np.uint64) if distinct is None else rng.integers(0, distinct, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        out.append((x.astype(dtype_of(f)) if f & WIDE else (x >> np.uint64(32)).astype(np.uint32), f))
    return out


def payload(n, seed, dtype=np.uint32):
    return np.random.default_rng(seed + 500).integers(0, 1 << 32, n, dtype=np.uint64).astype(dtype) * (dtype(0x100000001) if dtype == np.uint64 else dtype(1))


@pytest.mark.parametrize("kind", MASKS)
def test_tails_on_both_roads(hj, kind):
    """n around words, vectors, one chunk, the road switch, one chunk beyond it and the first shape with two ranges of two chunks; two keys, the second one wide
    and descending, few distinct values; the row numbers and one carried column"""
    L, ranges, chunk, big = geometry(hj)
    sizes = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, L - 1, L, L + 1, L + chunk - 1, L + chunk, L + chunk + 1, big - 1, big, big + 1]
    for n in sizes:
        small = n <= L + chunk + 1
        flags = [0, DESC | WIDE] if small else [0]                 # (the large shapes: one key, four passes)
        keys = random_keys(n, flags, seed=n, distinct=50 if small else 1 << 20)
        order(hj, keys, sel_of(kind, n, seed=n + 7), kind, cols=[payload(n, n)])


@pytest.mark.parametrize("road", ["lds", "device"])
def test_stability(hj, road):
    L, ranges, chunk, big = geometry(hj)
    n = L - 5 if road == "lds" else L + 3 * chunk + 5
    sel = selection("half", n, seed=1)
    rows = np.flatnonzero(sel).astype(np.uint32)
    same32, same64 = np.full(n, 0x80000001, np.uint32), np.full(n, 1 << 63, np.uint64)
    # all keys equal: the selected row numbers ascending, under ASC and under DESC, signed and unsigned, narrow and wide
    for flags in (0, DESC, SIGNED, DESC | SIGNED):
        assert order(hj, [(same32, flags), (same64, flags | WIDE)], sel, "half", want=rows) == len(rows)
    # two distinct values only, in either direction
    two = (np.random.default_rng(2).random(n) < 0.3).astype(np.uint32) * np.uint32(0xFFFFFFFF)
    for flags in (0, DESC, SIGNED, DESC | SIGNED):
        order(hj, [(two, flags)], sel, "half", cols=[two])
    # already sorted, reverse sorted, with runs of equal keys
    up = (np.arange(n, dtype=np.uint32) // 3) * np.uint32(0x10001)
    for flags in (0, DESC):
        order(hj, [(up, flags)], sel, "half")
        order(hj, [(up[::-1].copy(), flags)], sel, "half")


@pytest.mark.parametrize("road", ["lds", "device"])
@pytest.mark.parametrize("nkeys", [1, 2, 3, 4])
def test_edge_values_under_every_direction_and_signedness(hj, nkeys, road):
    """the cartesian product of the edge values over the keys, every combination of DESC / SIGNED per key; on the device road the
    product is repeated until it is longer than L, so every tuple ties with its copies"""
    L, ranges, chunk, big = geometry(hj)
    product = np.array(list(itertools.product(EDGES, repeat=nkeys)), np.uint32)
    reps = 1 if road == "lds" else L // len(product) + 2
    product = np.tile(product, (reps, 1))
    n = len(product)
    assert (n <= L) == (road == "lds")
    columns = [np.ascontiguousarray(product[:, c]) for c in range(nkeys)]
    sel = np.ones(n, bool)
    carried = np.arange(n, dtype=np.uint32) ^ np.uint32(0x55AA55AA)
    for combo in itertools.product((0, DESC, SIGNED, DESC | SIGNED), repeat=nkeys):
        order(hj, list(zip(columns, combo)), sel, "null", cols=[carried])


@pytest.mark.parametrize("road", ["lds", "device"])
def test_wide_keys(hj, road):
    """64-bit keys that vary in the high half only, in the low half only and in one byte only, and the 64-bit edge values"""
    L, ranges, chunk, big = geometry(hj)
    n = 3001 if road == "lds" else L + chunk + 77
    rng = np.random.default_rng(3)
    r = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    edges = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, 0xFFFFFFFF00000000, (1 << 64) - 1], np.uint64)
    shapes = {"high half": (r << np.uint64(32)) | np.uint64(0x1234), "low half": r | np.uint64(0xABCD << 32),
              "byte 5": ((r & np.uint64(0xFF)) << np.uint64(40)) | np.uint64(0x0102030000040506), "byte 0": (r & np.uint64(0xFF)) | np.uint64(0xFFFFFFFFFFFFFF00),
              "edges": edges[rng.integers(0, len(edges), n)]}
    sel = selection("half", n, seed=4)
    for name, key in shapes.items():
        for flags in (WIDE, WIDE | DESC, WIDE | SIGNED, WIDE | SIGNED | DESC):
            print(name, flags)
            order(hj, [(key, flags)], sel, "half", cols=[key])
    # a narrow key in front of a wide one and behind it
    narrow = (r & np.uint64(3)).astype(np.uint32)
    order(hj, [(narrow, DESC), (shapes["edges"], WIDE | SIGNED)], sel, "half")
    order(hj, [(shapes["byte 5"], WIDE), (narrow, SIGNED), (shapes["edges"], WIDE | DESC)], sel, "half")


def test_skew(hj):
    L, ranges, chunk, big = geometry(hj)
    # a key whose digit is constant in some passes and takes all 256 values in others, on both roads
    for n in (L - 1, L + 2 * chunk + 9):
        i = np.arange(n, dtype=np.uint64)
        key32 = (((i * 7) % 256) << np.uint64(8)).astype(np.uint32) | np.uint32(0x11000022)
        key64 = (((i * 11) % 256) << np.uint64(48)) | (((i * 3) % 256) << np.uint64(16))
        sel = selection("half", n, seed=5)
        order(hj, [(key32, 0)], sel, "half")
        order(hj, [(key64, WIDE | DESC), (key32, DESC)], sel, "half", cols=[key64])
    # one digit value holds all rows but one: a bin larger than a chunk that spans ranges
    n = big
    key = np.full(n, 0x05050505, np.uint32)
    key[n // 2 + 3] = 0x05030505
    for flags in (0, DESC):
        order(hj, [(key, flags)], np.ones(n, bool), "null", cols=[payload(n, 6)])


@pytest.mark.parametrize("road", ["lds", "device"])
def test_carried_columns(hj, road):
    L, ranges, chunk, big = geometry(hj)
    n = 2999 if road == "lds" else L + chunk + 31
    sel = selection("half", n, seed=8)
    keys = random_keys(n, [DESC, WIDE], seed=9, distinct=40)
    c32 = [payload(n, 10 + c) for c in range(4)]
    c64 = [payload(n, 20 + c, np.uint64) for c in range(4)]
    order(hj, keys, sel, "half", cols=[])                                            # the row numbers alone
    order(hj, keys, sel, "half", cols=[c64[0]])
    order(hj, keys, sel, "half", cols=[c32[0]], rows=False)
    order(hj, keys, sel, "half", cols=[c32[0], c64[0], c32[1], c64[1], c64[2], c32[2], c32[3], c64[3]])      # eight, 4- and 8-byte mixed
    order(hj, keys, sel, "half", cols=[keys[0][0], keys[1][0], c32[0]])               # the key columns carried
    order(hj, keys, sel, "half", cols=[c32[0], c64[0], c32[0], c64[0]], rows=False)   # the same column twice
    order(hj, [keys[0], keys[0], keys[1]], sel, "half", cols=[c32[1]])                # the same key twice
    assert order(hj, keys, sel, "half", cols=[], rows=False) == int(sel.sum())       # the count alone
    assert order(hj, keys, np.ones(n, bool), "null", cols=[], rows=False) == n


@pytest.mark.parametrize("road", ["lds", "device"])
def test_limit(hj, road):
    L, ranges, chunk, big = geometry(hj)
    n = 1000 if road == "lds" else L + chunk + 1
    sel = selection("half", n, seed=11)
    J = int(sel.sum())
    keys = random_keys(n, [SIGNED, DESC], seed=12, distinct=30)
    cols = [payload(n, 13), payload(n, 14, np.uint64)]
    want = model(keys, sel)
    for limit in (0, 1, J - 1, J, J + 1, n, n + 5, 1 << 40):
        assert order(hj, keys, sel, "half", cols=cols, limit=limit, want=want) == J  # (no exception below J: LIMIT is not an overflow)


def test_enqueue_only(hj):
    """three calls of different n and roads back to back on one stream before one synchronise, the counts in device memory"""
    L, ranges, chunk, big = geometry(hj)
    shapes = [(L + 2 * chunk + 3, "half", [0, WIDE | DESC], 300), (777, "eighth", [SIGNED | DESC], None), (L + 5, "null", [WIDE], 10)]
    calls = []
    for n, kind, flags, limit in shapes:
        sel = sel_of(kind, n, seed=n)
        calls.append((Call(hj, n, random_keys(n, flags, seed=n + 1, distinct=100), sel, kind, [payload(n, n + 2), payload(n, n + 3, np.uint64)], True, limit),
                      hj.column(np.full(2, 77, np.uint64), np.uint64)))
    # (the workspace for the largest n first: growing it between the enqueues would wait for the device)
    hj.order_by(None, shapes[0][0], [(calls[0][0].dev[id(calls[0][0].keys[0][0])], 0)], [], [], None, limit=0)
    for call, d_count in calls:
        hj.order_by_async(*call.args(), d_count)
    hj.synchronize()
    for call, d_count in calls:
        got = d_count.download()
        assert int(got[1]) == 77, "the word behind the count was written"
        call.check(int(got[0]))
    hj.get_async_status()                                                             # nothing to report: no join ran


def test_n_zero_accepts_null(hj):
    assert hj.order_by(None, 0, [(None, 0)], [], [], None) == 0
    d_count = hj.column(np.full(1, 77, np.uint64), np.uint64)
    hj.order_by_async(None, 0, [(None, 0xFF), (None, 0)], [(None, 0xFF)], [None], None, 5, d_count)
    hj.synchronize()
    assert int(d_count.download()[0]) == 0


def test_refusals_reach_the_caller(hj):
    """the checks themselves are tests/test_order_by_checks.py's: here, that a refused call raises with the status and the text, writes
    nothing, and that a capturing stream is refused"""
    import torch
    n = 1000
    key, out, rows = hj.column(with_sentinel(np.arange(n, dtype=np.uint32))), canary(hj, n, np.uint32), canary(hj, n, np.uint32)
    d_count = hj.column(np.full(2, 77, np.uint64), np.uint64)

    def blocking(keys=((key, 0),), cols_in=(key,), cols_out=(out,), rows_out=rows, n=n, stream=None):
        return hj.order_by(None, n, list(keys), list(cols_in), list(cols_out), rows_out, stream=stream)

    def enqueue(keys=((key, 0),), cols_in=(key,), cols_out=(out,), rows_out=rows, n=n, count=d_count, stream=None):
        return hj.order_by_async(None, n, list(keys), list(cols_in), list(cols_out), rows_out, None, count, stream=stream)

    for call in (blocking, enqueue):
        cases = [("no key", dict(keys=()), api.EINVAL, "nkeys"), ("five keys", dict(keys=((key, 0),) * 5), api.EINVAL, "nkeys"),
                 ("nine columns", dict(cols_in=(key,) * 9, cols_out=(out,) * 9), api.EINVAL, "ncols"),
                 ("an undefined flag", dict(keys=((key, 0), (key, 8))), api.EINVAL, "key 1"),
                 ("a NULL key column", dict(keys=((None, 0),)), api.EINVAL, "key 0"),
                 ("a misaligned output", dict(cols_out=(out.ptr + 4,)), api.EALIGN, "aligned"),
                 ("in place", dict(cols_out=(key,)), api.EINVAL, "overlaps"),
                 ("the row numbers over an output", dict(rows_out=out.ptr + 16), api.EINVAL, "overlaps"),
                 ("n beyond 32 bits", dict(n=1 << 32), api.EINVAL, "0xFFFFFFFF")]
        if call is enqueue:
            cases += [("null d_count", dict(count=None), api.EINVAL, "null"), ("misaligned d_count", dict(count=d_count.ptr + 4), api.EALIGN, "d_count"),
                      ("d_count inside an output", dict(count=out.ptr + 8), api.EINVAL, "overlaps")]
        for name, kw, status, text in cases:
            with pytest.raises(api.HjGpuError) as e:
                call(**kw)
            assert e.value.status == status and text in str(e.value), (name, str(e.value))
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(api.HjGpuError) as e:
                    call(stream=s.cuda_stream)
                assert e.value.status == api.EINVAL and "capturing" in str(e.value)
            finally:
                g.capture_end()
        s.synchronize()
    hj.synchronize()
    assert np.all(out.download() == CANARY32) and np.all(rows.download() == CANARY32), "a refused call wrote an output"
    assert [int(x) for x in d_count.download()] == [77, 77]
    assert blocking() == n and np.array_equal(rows.download()[:n], np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("road", ["lds", "device"])
def test_stats(hj, road):
    L, ranges, chunk, big = geometry(hj)
    n = L if road == "lds" else big
    hj.order_by(None, 16, [(hj.column(np.zeros(16, np.uint32)), 0)], [], [], hj.column(16))     # (the context's first launch is not the timed one)
    before = hj.stats()["ms_reserve"]
    order(hj, random_keys(n, [0], seed=15), selection("half", n, seed=16), "half", cols=[payload(n, 17)])
    s = hj.stats()
    print(s)
    assert s["ms_total"] > 0 and s["ms_join"] > 0, s
    if road == "device":
        assert s["ms_histogram"] > 0 and s["ms_close_gaps"] > 0 and s["ms_reserve"] > before, s
    assert s["ms_total"] >= (s["ms_histogram"] + s["ms_join"] + s["ms_close_gaps"]) * (1 - 1e-5), s
    for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_build", "ms_inner_wait"):
        assert s[k] == 0, (k, s)
    assert s["fanout1"] == 0 and s["fanout2"] == 0 and s["buckets"] == 0 and s["groups"] == 0, s


def test_the_end_of_a_real_chain(hj):
    """GROUP BY three keys with a SUM, then ORDER BY key 0 ASC, the uint64 sum DESC carrying all columns: the numpy-sorted groups"""
    n, groups = 200_003, 3000
    rng = np.random.default_rng(21)
    ids = rng.integers(0, groups, n)
    keys = [(ids % 7).astype(np.uint32), ((ids // 7) % 20).astype(np.uint32) * np.uint32(0x01000193), (ids // 140).astype(np.uint32) | np.uint32(0x80000000)]
    measure = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    sel = selection("half", n, seed=22)
    bits = hj.column(mask_words(sel))
    dk, dm = [hj.column(k) for k in keys], hj.column(measure)
    cap = 4096
    kout, sout, cout = [hj.column(cap) for _ in keys], hj.column(cap, np.uint64), hj.column(cap, np.uint64)
    J = hj.group_by(bits, n, dk, [(api.AGG_SUM, dm)], kout, [sout], cout, capacity=cap)
    # the same query in numpy
    K = np.stack([k[sel] for k in keys], axis=1)
    uniq, inv = np.unique(K, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    sums = np.zeros(len(uniq), np.uint64)
    np.add.at(sums, inv, measure[sel].astype(np.uint64))
    counts = np.bincount(inv, minlength=len(uniq)).astype(np.uint64)
    assert J == len(uniq) and 100 < J <= min(cap, hj.counter("order_lds_rows"))
    # key 0 ascending, then the sum descending; what still ties (no two groups' sums do here, the model says so) keeps the group order,
    # which is unspecified - so the comparison is of the sorted tuples, and the order itself is checked on the keys it is made of
    okeys, osum, ocnt, orows = [canary(hj, J, np.uint32) for _ in keys], canary(hj, J, np.uint64), canary(hj, J, np.uint64), canary(hj, J, np.uint32)
    got = hj.order_by(None, J, [(kout[0], 0), (sout, WIDE | DESC)], kout + [sout, cout], okeys + [osum, ocnt], orows)
    assert got == J
    sum_rank = np.unique(sums, return_inverse=True)[1].reshape(-1).astype(np.int64)
    order_np = np.lexsort((-sum_rank, uniq[:, 0]))
    pairs = np.stack([uniq[:, 0].astype(np.uint64), sums], axis=1)
    assert len(np.unique(pairs, axis=0)) == J, "two groups tie in (key 0, sum): the comparison below would depend on the groups' order"
    for c in range(3):
        check_column(okeys[c].download(), uniq[order_np, c], J, ("chain", "key", c))
    check_column(osum.download(), sums[order_np], J, ("chain", "sum"))
    check_column(ocnt.download(), counts[order_np], J, ("chain", "count"))
    # the row numbers are positions in the grouped output: they gather the groups' own columns into the same order
    rows = orows.download()[:J]
    assert np.array_equal(kout[1].download()[:J][rows], uniq[order_np, 1]) and np.array_equal(sout.download()[:J][rows], sums[order_np])
