"""GPU tests of hjgpu_group_sum / hjgpu_group_sum_async: GROUP BY one or two uint32 columns, COUNT(*) and up to four SUMs over the rows a
bitmap in d_match_bits' layout selects (NULL: every row).

Expected values come from numpy: np.unique(keys, axis=0, return_inverse=True), np.bincount for the counts and np.add.at on uint64 for the
sums.  The order of the groups is unspecified, so both sides are sorted by key tuple before they are compared; equality is exact.  Every
output is longer than `capacity` and pre-filled with a canary: nothing at index >= min(J, capacity) may change.  The mask is followed by
all-ones words that nothing may read; mask and inputs come back unchanged.  The group counts are derived from the context's counter
"group_lds_groups" (G), never hard-coded.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import HjGpuError
from test_gpu_npj_lookup import relations, outputs
from test_gpu_lookup_selected import hj, pack, mask_words, selection, col, want_selected        # noqa: F401 (hj: the fixture)

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF                       # HJGPU_NULL_VAL
CANARY32 = 0xA5A5A5A5
CANARY64 = 0xA5A5A5A5A5A5A5A5
ONES = 0xFFFFFFFF
EXTRA = 64
MASKS = ["null", "ones", "zeros", "half", "eighth", "alternating_words", "first_row", "last_row", "garbage_tail"]
TAILS = [0, 1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 1023, 1025, 4099]
MANY = 300_007                          # several workgroups
LOOPS = 2_400_011                       # more wave trips than one grid of workgroups has: the grid-stride loop iterates


def lds_groups(hj):
    G = hj.counter("group_lds_groups")
    assert 64 <= G <= 4096, G
    return G


def sel_of(kind, n, seed):
    return np.ones(n, bool) if kind == "null" else selection(kind, n, seed)


def tuples(ids, nkeys):
    """key columns whose tuples are distinct exactly where the ids are.  One column: an odd multiple of the id (id 0 is key 0).  Two columns:
    ids 2 a and 2 a + 1 differ in the second column alone, which is 0 or 0xFFFFFFFF; id 0 is the tuple (0, 0)."""
    ids = ids.astype(np.uint64)
    if nkeys == 1:
        return [((ids * 0x9E3779B1) & 0xFFFFFFFF).astype(np.uint32)]
    return [(ids >> 1).astype(np.uint32), ((ids & 1) * 0xFFFFFFFF).astype(np.uint32)]


def measures(n, nvals, seed):
    rng = np.random.default_rng(seed + 1000)
    return [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(nvals)]


def expected(keys, vals, sel):
    """(sorted distinct tuples [J, nkeys], counts [J], sums [nvals][J]) of the selected rows"""
    K = np.stack([k[sel] for k in keys], axis=1)
    if len(K) == 0:
        return K, np.zeros(0, np.uint64), [np.zeros(0, np.uint64) for _ in vals]
    uniq, inv = np.unique(K, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    counts = np.bincount(inv, minlength=len(uniq)).astype(np.uint64)
    sums = []
    for v in vals:
        s = np.zeros(len(uniq), np.uint64)
        np.add.at(s, inv, v[sel].astype(np.uint64))
        sums.append(s)
    return uniq, counts, sums


def canary(hj, rows, dtype):
    return hj.column(np.full(rows + EXTRA, CANARY32 if dtype == np.uint32 else CANARY64, dtype), dtype)


def by_tuple(cols):
    """the order that sorts the rows by (cols[0], cols[1] ...), as np.unique(axis=0) does"""
    return np.lexsort(tuple(reversed(cols)))


def check_outputs(want, J_got, capacity, kout, cout, sout, overflow, what):
    uniq, counts, sums = want
    J = len(uniq)
    gk = [d.download() for d in kout]
    gc = cout.download() if cout is not None else None
    gs = [d.download() for d in sout]
    m = min(J_got, capacity)
    for c, raw in enumerate(gk):
        assert np.all(raw[m:] == CANARY32), (what, "key column", c, "written at index >= min(J, capacity)")
    for c, raw in enumerate(([gc] if gc is not None else []) + gs):
        assert np.all(raw[m:] == CANARY64), (what, "uint64 output", c, "written at index >= min(J, capacity)")
    if overflow:
        assert capacity < J_got <= J, (what, capacity, J_got, J)
        return
    assert J_got == J, (what, J_got, J)
    order = by_tuple([g[:J] for g in gk])
    for c, raw in enumerate(gk):
        assert np.array_equal(raw[:J][order], uniq[:, c]), (what, "key column", c)
    if gc is not None:
        assert np.array_equal(gc[:J][order], counts), (what, "counts", np.flatnonzero(gc[:J][order] != counts)[:8])
    for c, raw in enumerate(gs):
        assert np.array_equal(raw[:J][order], sums[c]), (what, "sums", c, np.flatnonzero(raw[:J][order] != sums[c])[:8])


def group(hj, keys, vals, sel, kind="null", capacity=None, counts=True, overflow=False, want=None):
    """one blocking call checked against numpy in every respect; returns the count"""
    n = len(sel)
    want = expected(keys, vals, sel) if want is None else want
    J = len(want[0])
    capacity = J if capacity is None else capacity
    words = mask_words(sel, kind) if kind != "null" else None
    dsel = hj.column(words) if words is not None else None
    dk, dv = [col(hj, k) for k in keys], [col(hj, v) for v in vals]
    kout = [canary(hj, capacity, np.uint32) for _ in keys]
    cout = canary(hj, capacity, np.uint64) if counts else None
    sout = [canary(hj, capacity, np.uint64) for _ in vals]
    try:
        got = hj.group_sum(dsel, n, dk, dv, kout, sout, cout, capacity=capacity)
        assert not overflow, "HJGPU_EOVERFLOW expected"
    except HjGpuError as e:
        assert overflow and e.status == api.EOVERFLOW, str(e)
        got = e.count
    print(kind, "n", n, "nkeys", len(keys), "nvals", len(vals), "capacity", capacity, "count", got, "want", J)
    check_outputs(want, got, capacity, kout, cout, sout, overflow, (kind, n))
    if words is not None:
        assert np.array_equal(dsel.download(), words), "the mask was written"
    for h, d in zip(list(keys) + list(vals), dk + dv):
        if len(h):
            assert np.array_equal(d.download(), h), "an input column was written"
    for d in ([dsel] if dsel is not None else []) + dk + dv + kout + sout + ([cout] if counts else []):
        d.free()
    return got


def random_ids(n, groups, seed):
    """ids of [0, groups), every one of them present when n >= groups"""
    ids = np.random.default_rng(seed).integers(0, groups, n)
    ids[:min(n, groups)] = np.arange(min(n, groups))
    return ids


@pytest.mark.parametrize("kind", MASKS)
def test_row_counts(hj, kind):
    """the partial vector, the partial word, garbage bits at >= n, no row at all; then several workgroups"""
    for n in TAILS + [MANY]:
        keys = tuples(random_ids(n, 7, seed=n), 2)
        group(hj, keys, measures(n, 1, seed=n), sel_of(kind, n, seed=n + 3), kind)


def test_basic_parity(hj):
    n = 4099
    sel = selection("half", n, seed=1)
    for nkeys in (1, 2):
        assert group(hj, tuples(random_ids(n, 50, seed=2), nkeys), measures(n, 2, seed=3), sel, "half") == 50


def test_grid_stride_iterations(hj):
    keys = tuples(random_ids(LOOPS, 1000, seed=11), 2)
    group(hj, keys, measures(LOOPS, 1, seed=12), selection("half", LOOPS, seed=13), "half")


@pytest.mark.parametrize("nkeys", [1, 2])
@pytest.mark.parametrize("fill", ["random", "cyclic"])
def test_group_counts(hj, nkeys, fill):
    """G - 1, G and G + 1 groups around the point where a workgroup's table stops claiming slots; 3 G: most rows go straight to the merge
    table and the flush adds the rest.  cyclic: the rows of every wave trip run through all the groups"""
    G = lds_groups(hj)
    for groups in [1, 2, 7, G - 1, G, G + 1, 3 * G]:
        ids = random_ids(MANY, groups, seed=groups) if fill == "random" else np.arange(MANY) % groups
        got = group(hj, tuples(ids, nkeys), measures(MANY, 1, seed=groups), sel_of("null", MANY, 0) if fill == "cyclic" else selection("half", MANY, seed=5),
                    "null" if fill == "cyclic" else "half")
        assert got == groups


@pytest.mark.parametrize("shape", ["all_equal", "runs_of_4", "runs_of_4_shifted", "runs_of_3"])
def test_clustered_keys(hj, shape):
    """the fold of a lane's four rows: all of them equal, runs that are a lane's rows, runs that straddle two lanes"""
    n = 40_003
    i = np.arange(n, dtype=np.uint64)
    k = {"all_equal": np.full(n, 12345, np.uint64), "runs_of_4": i // 4, "runs_of_4_shifted": (i + 2) // 4, "runs_of_3": i // 3}[shape]
    keys = [k.astype(np.uint32), np.full(n, 7, np.uint32)]
    for kind in ("null", "half"):
        group(hj, keys, measures(n, 2, seed=4), sel_of(kind, n, seed=6), kind)
        group(hj, keys[:1], measures(n, 1, seed=4), sel_of(kind, n, seed=6), kind)


def test_key_values(hj):
    """0, 0xFFFFFFFF = HJGPU_NULL_VAL and their tuples are ordinary groups; tuples that differ in the second column alone"""
    n = 10_001
    special = np.array([0, NULL, 1, 0x80000000, 0xFFFFFFFE], np.uint32)
    rng = np.random.default_rng(8)
    k0, k1 = special[rng.integers(0, len(special), n)], special[rng.integers(0, len(special), n)]
    k0[:2], k1[:2] = [0, 0], [0, NULL]                     # (0, 0) and (0, NULL)
    vals = measures(n, 1, seed=9)
    for kind in ("null", "eighth"):
        sel = sel_of(kind, n, seed=10)
        sel[:2] = True
        assert group(hj, [k0, k1], vals, sel, kind) == 25
        assert group(hj, [k0], vals, sel, kind) == 5
        assert group(hj, [k1, k1], vals, sel, kind) == 5
    # the tuple 0 alone, and absent
    group(hj, [np.zeros(n, np.uint32), np.zeros(n, np.uint32)], vals, sel_of("half", n, 3), "half")
    group(hj, [np.zeros(n, np.uint32)], vals, sel_of("half", n, 3), "half")
    group(hj, [np.full(n, NULL, np.uint32), np.full(n, NULL, np.uint32)], vals, sel_of("half", n, 3), "half")


@pytest.mark.parametrize("nvals", [0, 1, 4])
def test_measures(hj, nvals):
    n = MANY
    keys = tuples(random_ids(n, 7, seed=21), 2)
    sel = selection("half", n, seed=22)
    group(hj, keys, measures(n, nvals, seed=23), sel, "half")
    group(hj, keys, measures(n, nvals, seed=23), sel, "half", counts=False)          # d_counts_out NULL
    # every measure 0xFFFFFFFF: the sums pass 2^32
    big = [np.full(n, ONES, np.uint32) for _ in range(nvals)]
    want = expected(keys[:1], big, sel)
    if nvals:
        assert int(want[2][0].max()) > 1 << 32
    group(hj, keys[:1], big, sel, "half", want=want)


def test_the_same_column_twice(hj):
    n = 4099
    k = tuples(random_ids(n, 33, seed=31), 1)[0]
    v = measures(n, 1, seed=32)[0]
    sel = selection("half", n, seed=33)
    group(hj, [k, k], [v, v, k], sel, "half")
    # the very same device column in several places
    dsel, dk, dv = hj.column(mask_words(sel)), hj.column(k), hj.column(v)
    kout = [canary(hj, 33, np.uint32) for _ in range(2)]
    sout = [canary(hj, 33, np.uint64) for _ in range(3)]
    cout = canary(hj, 33, np.uint64)
    assert hj.group_sum(dsel, n, [dk, dk], [dv, dv, dk], kout, sout, cout, capacity=33) == 33
    check_outputs(expected([k, k], [v, v, k], sel), 33, 33, kout, cout, sout, False, "one column")


def test_capacity(hj):
    G = lds_groups(hj)
    n = 50_003
    groups = 2 * G + 5
    keys, vals = tuples(random_ids(n, groups, seed=41), 2), measures(n, 1, seed=42)
    sel = np.ones(n, bool)
    want = expected(keys, vals, sel)
    J = len(want[0])
    assert J == groups
    group(hj, keys, vals, sel, capacity=J, want=want)
    group(hj, keys, vals, sel, capacity=J - 1, overflow=True, want=want)
    group(hj, keys, vals, sel, capacity=0, overflow=True, want=want)                # the merge table's minimum size is below J here
    group(hj, keys, vals, sel, capacity=1 << 20, want=want)
    group(hj, keys, vals, sel, capacity=7, overflow=True, want=want)
    # capacity 0 with no group at all is no overflow
    assert group(hj, keys, vals, np.zeros(n, bool), "zeros", capacity=0) == 0
    # the default capacity is the shortest output
    dk, dv = [hj.column(k) for k in keys], [hj.column(v) for v in vals]
    kout = [hj.column(np.full(J + 8, CANARY32, np.uint32)), hj.column(np.full(J - 8, CANARY32, np.uint32))]
    sout = [hj.column(np.full(J + 8, CANARY64, np.uint64), np.uint64)]
    with pytest.raises(HjGpuError) as e:
        hj.group_sum(None, n, dk, dv, kout, sout)
    assert e.value.status == api.EOVERFLOW and e.value.count == J
    assert np.all(kout[0].download()[J - 8:] == CANARY32) and np.all(sout[0].download()[J - 8:] == CANARY64)


def test_refusals(hj):
    """each returns before anything is enqueued: the canaries, the mask and the inputs are untouched afterwards"""
    import torch
    n = 1000
    words = np.concatenate([pack(selection("half", 16384, seed=6)), np.full(4, ONES, np.uint32)])      # room for shifted and overlapping pointers
    dsel = hj.column(words)
    h = [np.arange(n + 64, dtype=np.uint32) % 13, np.arange(n + 64, dtype=np.uint32) % 5, np.arange(n + 64, dtype=np.uint32)]
    din = [hj.column(x) for x in h]
    kout = [canary(hj, n, np.uint32), canary(hj, n, np.uint32)]
    sout = [canary(hj, n, np.uint64)]
    cout = canary(hj, n, np.uint64)
    d_count = hj.column(np.full(2, 77, np.uint64), np.uint64)
    ki, vi, ko, so = [din[0].ptr, din[1].ptr], [din[2].ptr], [d.ptr for d in kout], [d.ptr for d in sout]

    def blocking(bits=dsel.ptr, n=n, ki=ki, vi=vi, ko=ko, so=so, counts=cout.ptr, capacity=n, stream=None):
        return hj.group_sum(bits, n, ki, vi, ko, so, counts, capacity=capacity, stream=stream)

    def enqueue(bits=dsel.ptr, n=n, ki=ki, vi=vi, ko=ko, so=so, counts=cout.ptr, capacity=n, count=d_count.ptr, stream=None):
        return hj.group_sum_async(bits, n, ki, vi, ko, so, counts, capacity, count, stream=stream)

    for call in (blocking, enqueue):
        cases = [("misaligned mask", dict(bits=dsel.ptr + 4), api.EALIGN, "d_select_bits"),
                 ("misaligned key column", dict(ki=[ki[0], ki[1] + 4]), api.EALIGN, "aligned"),
                 ("misaligned measure column", dict(vi=[vi[0] + 8]), api.EALIGN, "aligned"),
                 ("misaligned key output", dict(ko=[ko[0] + 8, ko[1]]), api.EALIGN, "aligned"),
                 ("misaligned sum output", dict(so=[so[0] + 8]), api.EALIGN, "aligned"),
                 ("misaligned counts", dict(counts=cout.ptr + 8), api.EALIGN, "d_counts_out"),
                 ("no key column", dict(ki=[], ko=[]), api.EINVAL, "nkeys"),
                 ("three key columns", dict(ki=ki + ki[:1], ko=ko + ko[:1]), api.EINVAL, "nkeys"),
                 ("five measures", dict(vi=vi * 5, so=so * 5), api.EINVAL, "nvals"),
                 ("null key entry", dict(ki=[ki[0], None]), api.EINVAL, "null"),
                 ("null key output entry", dict(ko=[None, ko[1]]), api.EINVAL, "null"),
                 ("null measure entry", dict(vi=[None]), api.EINVAL, "null"),
                 ("null sum entry", dict(so=[None]), api.EINVAL, "null"),
                 ("capacity beyond 2^40", dict(capacity=(1 << 40) + 1), api.EINVAL, "capacity"),
                 ("key output over the mask", dict(ko=[ko[0], dsel.ptr + 16]), api.EINVAL, "overlaps"),
                 ("counts over the mask", dict(counts=dsel.ptr), api.EINVAL, "overlaps"),
                 ("sums over a key column", dict(so=[ki[1] + 16]), api.EINVAL, "overlaps"),
                 ("key output over a measure column", dict(ko=[vi[0] + 16, ko[1]]), api.EINVAL, "overlaps"),
                 ("key output over a key output", dict(ko=[ko[0], ko[0] + 16]), api.EINVAL, "overlaps"),
                 ("counts over the sums", dict(counts=so[0] + 8 * (n - 2)), api.EINVAL, "overlaps")]
        if call is enqueue:
            cases += [("null d_ngroups", dict(count=None), api.EINVAL, "null"), ("misaligned d_ngroups", dict(count=d_count.ptr + 4), api.EALIGN, "d_ngroups"),
                      ("d_ngroups inside an output", dict(count=cout.ptr + 8), api.EINVAL, "overlaps")]
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
    # (the binding always passes the blocking form a count: the C entry point itself refuses NULL)
    assert hj.lib.hjgpu_group_sum(hj.handle, dsel.ptr, n, 2, None, 0, None, None, None, None, n, None, None) == api.EINVAL
    assert b"null group count" in hj.lib.hjgpu_last_error(hj.handle)
    hj.synchronize()
    for d in kout:
        assert np.all(d.download() == CANARY32), "a refused call wrote an output"
    for d in sout + [cout]:
        assert np.all(d.download() == CANARY64), "a refused call wrote an output"
    assert np.array_equal(dsel.download(), words) and all(np.array_equal(d.download(), x) for d, x in zip(din, h))
    assert [int(x) for x in d_count.download()] == [77, 77]
    # the same pointers, accepted: plain integers as well as DeviceColumns
    sel = np.unpackbits(words[:(n + 31) // 32].view(np.uint8), bitorder="little")[:n].astype(bool)
    want = expected([x[:n] for x in h[:2]], [h[2][:n]], sel)
    assert blocking() == len(want[0]) == 65
    check_outputs(want, 65, n, kout, cout, sout, False, "accepted")


def test_n_zero_accepts_null(hj):
    assert hj.group_sum(None, 0, [None], [], [None], [], None, capacity=0) == 0
    d_count = hj.column(np.full(1, 77, np.uint64), np.uint64)
    hj.group_sum_async(None, 0, [None, None], [None], [None, None], [None], None, 5, d_count)
    hj.synchronize()
    assert int(d_count.download()[0]) == 0


def test_enqueue_only(hj):
    """two aggregations of different shapes back to back on one stream, no host wait in between - the second one's merge table is larger
    than the first one's, and a third call goes back to the small one; the status of the join before them stays what it was"""
    ik, iv, ok = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0                                                      # the preceding join's status: HJGPU_EZEROKEY
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok)
    dv, db = outputs(hj, len(ok), "both")
    d_res = hj.column(4, np.uint64)
    hj.reserve(len(ik), len(ok))
    hj.npj_lookup_async(rk, rv, len(ik), sk, len(ok), None, dv, db, d_res)
    shapes = [(70_013, "half", 2, 1, 300, 300), (20_001, "eighth", 1, 3, 5000, 6000), (4099, "null", 2, 0, 9, 5)]
    runs = []
    for n, kind, nkeys, nvals, groups, capacity in shapes:
        sel = sel_of(kind, n, seed=n)
        keys, vals = tuples(random_ids(n, groups, seed=n + 1), nkeys), measures(n, nvals, seed=n + 2)
        runs.append(dict(n=n, sel=sel, keys=keys, vals=vals, capacity=capacity, dsel=hj.column(mask_words(sel, kind)) if kind != "null" else None,
                         dk=[hj.column(x) for x in keys], dv=[hj.column(x) for x in vals],
                         kout=[canary(hj, capacity, np.uint32) for _ in keys], sout=[canary(hj, capacity, np.uint64) for _ in vals],
                         cout=canary(hj, capacity, np.uint64), d_count=hj.column(np.full(1, 77, np.uint64), np.uint64)))
    # (the workspace for the largest capacity first: growing it between the enqueues would wait for the device)
    hj.group_sum(None, 0, [None], [], [None], [], None, capacity=6000)
    for r in runs:
        hj.group_sum_async(r["dsel"], r["n"], r["dk"], r["dv"], r["kout"], r["sout"], r["cout"], r["capacity"], r["d_count"])
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()                                        # waits for the stream
    assert e.value.status == api.EZEROKEY
    for r in runs:
        want = expected(r["keys"], r["vals"], r["sel"])
        got = int(r["d_count"].download()[0])
        check_outputs(want, got, r["capacity"], r["kout"], r["cout"], r["sout"], got > r["capacity"], r["n"])
    assert int(runs[2]["d_count"].download()[0]) == 9                # the caller's comparison with capacity (5): an overflow


def test_stats(hj):
    n = LOOPS
    group(hj, tuples(random_ids(n, 100, seed=3), 2), measures(n, 1, seed=4), selection("half", n, seed=5), "half")
    s = hj.stats()
    print(s)
    assert s["ms_total"] > 0 and s["ms_histogram"] > 0 and s["ms_join"] > 0 and s["ms_close_gaps"] > 0, s
    assert s["ms_total"] >= (s["ms_histogram"] + s["ms_join"] + s["ms_close_gaps"]) * (1 - 1e-5), s
    for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_build", "ms_inner_wait"):
        assert s[k] == 0, (k, s)
    assert s["fanout1"] == 0 and s["fanout2"] == 0 and s["buckets"] == 0 and s["groups"] == 0, s


def test_the_end_of_a_look_up_chain(hj):
    """a filter bitmap, two selected look-ups that narrow it in place and whose value columns are the group keys, then the aggregation of
    a measure column over (vals1, vals2): the same query in numpy"""
    outer = 100_003
    d1k, d1v, k1 = relations(1000, outer, 0.5, seed=51)
    d2k, d2v, k2 = relations(2000, outer, 0.5, seed=52)
    d1v, d2v = (d1v % 40).astype(np.uint32), (d2v % 25).astype(np.uint32)          # the dimensions' attributes: 40 x 25 groups at most
    measure = measures(outer, 1, seed=54)[0]
    filt = selection("half", outer, seed=53)
    cols = [col(hj, x) for x in (d1k, d1v, k1, d2k, d2v, k2)]
    dm = hj.column(measure)
    bits = hj.column(mask_words(filt))
    dv1, _ = outputs(hj, outer, "vals")
    dv2, _ = outputs(hj, outer, "vals")
    hj.lookup_selected(cols[0], cols[1], len(d1k), cols[2], outer, select_bits=bits, vals_out=dv1, match_bits=bits)
    hj.lookup_selected(cols[3], cols[4], len(d2k), cols[5], outer, select_bits=bits, vals_out=dv2, match_bits=bits)
    hit1, vals1, _ = want_selected(d1k, d1v, k1, filt)
    hit2, vals2, _ = want_selected(d2k, d2v, k2, hit1)
    want = expected([vals1, vals2], [measure], hit2)
    J = len(want[0])
    assert 100 < J <= 1000
    kout = [canary(hj, J, np.uint32) for _ in range(2)]
    sout, cout = [canary(hj, J, np.uint64)], canary(hj, J, np.uint64)
    got = hj.group_sum(bits, outer, [dv1, dv2], [dm], kout, sout, cout, capacity=J)
    check_outputs(want, got, J, kout, cout, sout, False, "chain")
    assert int(cout.download()[:J].sum()) == int(hit2.sum())
    # the rows that the first dimension did not match, selected all the same: HJGPU_NULL_VAL is an ordinary group
    bits1 = hj.column(mask_words(filt))
    want = expected([vals1], [measure], filt)
    assert (want[0][:, 0] == NULL).any()
    kout, sout, cout = [canary(hj, 41, np.uint32)], [canary(hj, 41, np.uint64)], canary(hj, 41, np.uint64)
    check_outputs(want, hj.group_sum(bits1, outer, [dv1], [dm], kout, sout, cout, capacity=41), 41, kout, cout, sout, False, "null group")
