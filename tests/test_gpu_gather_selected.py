"""GPU tests of hjgpu_gather_selected / hjgpu_gather_selected_async: up to four uint32 columns fetched by an index column of row numbers,
in position, under an optional selection mask, with the gathered rows' bitmap and the exact counts of gathered and out-of-range rows.

Expected values come from numpy: row i is gathered when it is selected and idx[i] < src_rows, then out[c][i] = src[c][idx[i]] and bit i is
1; every other row holds HJGPU_NULL_VAL and bit 0; a selected row whose index is neither below src_rows nor HJGPU_NULL_VAL is counted as
out of range.  Exact equality.  Every output column and bitmap is followed by canary words that must not change, the mask by all-ones words
that nothing may read; mask, index (where it is not an output) and sources come back unchanged; the last bitmap word's high bits are 0.
The sources hold genuine 0xFFFFFFFF values, so only the bitmap tells those from NULLs.  The grid-seam sizes are derived from the context's
counter "gather_step_rows", never hard-coded.

Every test takes a context of its own (the fixture of test_gpu_lookup_selected)."""
import os
import re

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd import api
from hash_join_codes_knl_amd.api import HjGpuError, PhjParams
from test_gpu_npj_lookup import relations, outputs
from test_gpu_lookup_selected import hj, pack, mask_words, selection, col, want_selected        # noqa: F401 (hj: the fixture)
from test_gpu_left_outer import relations as join_relations

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF                       # HJGPU_NULL_VAL
CANARY = 0xA5A5A5A5
ONES = 0xFFFFFFFF
EXTRA = 8                               # canary words behind an output column or bitmap (the mask's all-ones words when in place: 4)
MASKS = ["null", "ones", "zeros", "half", "eighth", "alternating_words", "first_row", "last_row", "garbage_tail"]
TAILS = [0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]
SRC_ROWS = 1000


def sources(ncols, src_rows, seed):
    """ncols columns of src_rows values, one in eight of them a genuine 0xFFFFFFFF"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(ncols):
        s = rng.integers(0, 1 << 32, src_rows, dtype=np.uint64).astype(np.uint32)
        s[rng.random(src_rows) < 0.125] = NULL
        out.append(s)
    return out


def indices(n, src_rows, seed, bad=()):
    """n row numbers drawn from {0, src_rows - 1, uniform, HJGPU_NULL_VAL} and, one row in eight, from `bad`"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, n)
    top = max(src_rows, 1)
    idx = np.select([kind == 0, kind == 1, kind == 2], [0, top - 1, rng.integers(0, top, n)], NULL).astype(np.uint32)
    if len(bad):
        at = rng.random(n) < 0.125
        idx[at] = np.asarray(bad, np.uint32)[rng.integers(0, len(bad), int(at.sum()))]
    return idx


def sel_of(kind, n, seed):
    return np.ones(n, bool) if kind == "null" else selection(kind, n, seed)


def expected(sel, idx, srcs, src_rows):
    """(the output columns, the gathered rows, the out-of-range rows) by the definition"""
    good = sel & (idx.astype(np.int64) < src_rows)
    beyond = sel & ~good & (idx != NULL)
    safe = np.where(good, idx, 0).astype(np.int64)
    cols = [np.where(good, s[safe] if src_rows else NULL, NULL).astype(np.uint32) for s in srcs]
    return cols, good, beyond


def check_bitmap(raw, ok, tail, what):
    """raw: the downloaded bitmap buffer; ok: the gathered rows; tail: what the words behind the bitmap must still hold"""
    n, words = len(ok), (len(ok) + 31) // 32
    want = pack(ok)
    assert np.all(raw[words:] == tail), (what, "a word at index >= (n + 31) / 32 was written")
    bad = np.flatnonzero(raw[:words] != want)
    assert len(bad) == 0, (what, "bitmap words", bad[:8], [hex(int(x)) for x in raw[:words][bad[:4]]], [hex(int(x)) for x in want[bad[:4]]])
    if n % 32:
        assert int(raw[words - 1]) >> (n % 32) == 0, (what, "the last word's high bits")


def check_column(raw, want, what):
    n = len(want)
    assert np.all(raw[n:] == CANARY), (what, "an element at n or beyond was written")
    bad = np.flatnonzero(raw[:n] != want)
    assert len(bad) == 0, (what, "rows", bad[:8], [hex(int(x)) for x in raw[:n][bad[:4]]], [hex(int(x)) for x in want[bad[:4]]])


def run(hj, idx, sel, srcs, src_rows, kind="null", bits_in_place=False, col_in_place=None, dsrcs=None, bitmap=True, async_=False):
    """one call with every output, checked against numpy in every respect; returns (gathered, out of range).  A blocking call with
    out-of-range rows must raise HJGPU_ERANGE carrying both counts; the _async form returns and leaves them in d_counts."""
    n = len(sel)
    want, good, beyond = expected(sel, idx, srcs, src_rows)
    words = mask_words(sel, kind) if kind != "null" else None
    assert not (bits_in_place and words is None)
    dsel = hj.column(words) if words is not None else None
    didx = hj.column(np.concatenate([idx, np.full(EXTRA, CANARY, np.uint32)]))
    own = dsrcs is None
    dsrcs = [col(hj, s) for s in srcs] if own else dsrcs
    douts = [didx if c == col_in_place else hj.column(np.full(n + EXTRA, CANARY, np.uint32)) for c in range(len(srcs))]
    dbits = None if not bitmap else dsel if bits_in_place else hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32))
    what = (kind, "n", n, "ncols", len(srcs), "src_rows", src_rows, "bits in place" if bits_in_place else "", "column in place", col_in_place)
    if async_:
        d_counts = hj.column(np.full(4, 77, np.uint64), np.uint64)
        hj.gather_selected_async(dsel, didx, n, dsrcs, src_rows, douts, dbits, d_counts)
        hj.synchronize()
        raw = [int(v) for v in d_counts.download()]
        assert raw[2:] == [77, 77], (what, raw)
        got = tuple(raw[:2])
    elif beyond.any():
        with pytest.raises(HjGpuError) as e:
            hj.gather_selected(dsel, didx, n, dsrcs, src_rows, douts, dbits)
        assert e.value.status == api.ERANGE and "src_rows" in str(e.value), str(e.value)
        got = e.value.counts
    else:
        got = hj.gather_selected(dsel, didx, n, dsrcs, src_rows, douts, dbits)
    print(*what, "counts", got, "want", (int(good.sum()), int(beyond.sum())))
    for c, d in enumerate(douts):
        check_column(d.download(), want[c], what + ("column", c))
    if dbits is not None:
        check_bitmap(dbits.download(), good, ONES if bits_in_place else CANARY, what)
    assert got == (int(good.sum()), int(beyond.sum())), (what, got)
    if dsel is not None and not bits_in_place:
        assert np.array_equal(dsel.download(), words), (what, "the mask was written")
    if col_in_place is None:
        assert np.array_equal(didx.download(), np.concatenate([idx, np.full(EXTRA, CANARY, np.uint32)])), (what, "the index was written")
    if own:
        for h, d in zip(srcs, dsrcs):
            if len(h):
                assert np.array_equal(d.download(), h), (what, "a source column was written")
    for d in [didx] + ([dsel] if dsel is not None else []) + [o for o in douts if o is not didx] + (dsrcs if own else []) + \
            ([dbits] if dbits is not None and not bits_in_place else []):
        d.free()
    return got


@pytest.mark.parametrize("ncols", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", MASKS)
def test_tails_and_masks(hj, kind, ncols):
    """the partial vector, the partial word, garbage bits at >= n, no row at all; indices from {0, src_rows - 1, uniform, NULL}"""
    srcs = sources(ncols, SRC_ROWS, seed=ncols)
    dsrcs = [hj.column(s) for s in srcs]
    for n in TAILS:
        gathered, beyond = run(hj, indices(n, SRC_ROWS, seed=n), sel_of(kind, n, seed=n + 3), srcs, SRC_ROWS, kind, dsrcs=dsrcs)
        assert beyond == 0
        if kind == "zeros":
            assert gathered == 0
    for h, d in zip(srcs, dsrcs):
        assert np.array_equal(d.download(), h), "a source column was written"


@pytest.mark.parametrize("kind", ["null", "half"])
def test_grid_seams(hj, kind):
    """n around S and beyond 2 S, S the rows the whole grid covers per iteration: the last workgroups' first iteration, the first ones'
    second; the counter is gather_layout.hpp's step_rows of the device's compute units"""
    S = hj.counter("gather_step_rows")
    cus = hj.device_info()["compute_units"]
    assert S % 2048 == 0 and S % cus == 0 and 2048 <= S // cus <= 1 << 16, (S, cus)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hash_join_codes_knl_amd", "csrc", "gather_layout.hpp")).read()
    resident, block, batch = (int(re.search(r"constexpr uint32_t %s = (\d+);" % k, header).group(1)) for k in ("RESIDENT", "BLOCK", "BATCH"))
    assert S == cus * resident * block * 4 * batch, (S, cus, resident, block, batch)
    srcs = sources(2, SRC_ROWS, seed=8)
    dsrcs = [hj.column(s) for s in srcs]
    nmax = 2 * S + 77
    allidx, allsel = indices(nmax, SRC_ROWS, seed=5), sel_of(kind, nmax, seed=6)
    for n in (S - 1, S, S + 1, 2 * S + 77):
        gathered, beyond = run(hj, allidx[:n].copy(), allsel[:n].copy(), srcs, SRC_ROWS, kind, dsrcs=dsrcs)
        assert 0 < gathered < n and beyond == 0


@pytest.mark.parametrize("src_rows", [SRC_ROWS, 1, 0])
def test_out_of_range(hj, src_rows):
    """indices src_rows, src_rows + 1 and 0xFFFFFFFE among good ones: HJGPU_ERANGE with both counts exact, NULL and bit 0 at those rows,
    every other row right; unselected rows holding the same bad indices are not counted; the _async form returns OK with d_counts[1] set"""
    n = 4099
    bad = [src_rows, src_rows + 1, 0xFFFFFFFE]
    srcs = sources(2, src_rows, seed=4)
    idx = indices(n, src_rows, seed=7, bad=bad)
    for kind in ("null", "half"):
        gathered, beyond = run(hj, idx, sel_of(kind, n, seed=9), srcs, src_rows, kind)
        assert beyond > 0 and (gathered > 0) == (src_rows > 0)
        assert run(hj, idx, sel_of(kind, n, seed=9), srcs, src_rows, kind, async_=True) == (gathered, beyond)
    # the bad indices in unselected rows alone: nothing is counted, the call succeeds
    sel = sel_of("half", n, seed=9)
    clean = indices(n, src_rows, seed=7) if src_rows else np.full(n, NULL, np.uint32)        # (no row of an empty source is in range)
    idx2 = np.where(sel, clean, idx).astype(np.uint32)
    assert ((idx2 >= src_rows) & (idx2 != NULL) & ~sel).any()
    assert run(hj, idx2, sel, srcs, src_rows, "half")[1] == 0


def test_wide_addresses(hj):
    """a source of 2^30 + 64 rows (4 GiB: its upload takes a few seconds; the only large allocation of this module): 4 * idx leaves 32 bits
    from row 2^30 on.  Rows 0, 2^30 - 1, 2^30, 2^30 + 63 and a few hundred uniform ones, the same source twice; exact values"""
    src_rows = (1 << 30) + 64
    mult = np.uint32(0x9E3779B1)
    host = np.arange(src_rows, dtype=np.uint32)
    host *= mult                                                     # value = row * an odd constant mod 2^32
    dsrc = hj.column(host)
    del host
    n = 515
    idx = np.random.default_rng(3).integers(0, src_rows, n).astype(np.uint32)
    idx[:4] = [0, (1 << 30) - 1, 1 << 30, (1 << 30) + 63]
    idx[4:20] = (1 << 30) + np.arange(16) * 4 + 1                    # (uniform rows almost never fall into the last 64)
    want = (idx.astype(np.uint64) * np.uint64(mult) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert (idx >= 1 << 30).sum() >= 18 and want[2] == (int(mult) << 30) & 0xFFFFFFFF
    didx = hj.column(idx)
    douts = [hj.column(np.full(n + EXTRA, CANARY, np.uint32)) for _ in range(2)]
    dbits = hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32))
    assert hj.gather_selected(None, didx, n, [dsrc, dsrc], src_rows, douts, dbits) == (n, 0)
    for d in douts:
        check_column(d.download(), want, "wide")
    check_bitmap(dbits.download(), np.ones(n, bool), CANARY, "wide")
    # one row beyond the source's end is out of range, not read
    idx[7] = src_rows
    didx.upload(idx)
    with pytest.raises(HjGpuError) as e:
        hj.gather_selected(None, didx, n, [dsrc, dsrc], src_rows, douts, dbits)
    assert e.value.status == api.ERANGE and e.value.counts == (n - 1, 1)
    want[7] = NULL
    check_column(douts[1].download(), want, "wide, one row beyond")
    dsrc.free()


@pytest.mark.parametrize("ncols", [1, 3])
def test_in_place(hj, ncols):
    """d_bits_out == d_select_bits; one output column == d_idx (the first, the last); both at once - over more than one loop iteration"""
    S = hj.counter("gather_step_rows")
    srcs = sources(ncols, SRC_ROWS, seed=12)
    dsrcs = [hj.column(s) for s in srcs]
    for n in (4099, S + 4099):
        idx, sel = indices(n, SRC_ROWS, seed=n), sel_of("half", n, seed=n + 1)
        plain = run(hj, idx, sel, srcs, SRC_ROWS, "half", dsrcs=dsrcs)
        assert run(hj, idx, sel, srcs, SRC_ROWS, "half", bits_in_place=True, dsrcs=dsrcs) == plain
        for c in {0, ncols - 1} if n < S else ():
            assert run(hj, idx, sel, srcs, SRC_ROWS, "half", col_in_place=c, dsrcs=dsrcs) == plain
            assert run(hj, idx, sel_of("null", n, 0), srcs, SRC_ROWS, "null", col_in_place=c, dsrcs=dsrcs)[0] >= plain[0]
        assert run(hj, idx, sel, srcs, SRC_ROWS, "half", bits_in_place=True, col_in_place=ncols - 1, dsrcs=dsrcs) == plain


def test_either_output_optional(hj):
    """the bitmap NULL; the counts NULL - with bad indices the blocking form still returns HJGPU_ERANGE then"""
    n = 4099
    srcs = sources(2, SRC_ROWS, seed=31)
    idx, sel = indices(n, SRC_ROWS, seed=32), sel_of("half", n, seed=33)
    full = run(hj, idx, sel, srcs, SRC_ROWS, "half")
    assert run(hj, idx, sel, srcs, SRC_ROWS, "half", bitmap=False) == full
    assert run(hj, idx, sel, srcs, SRC_ROWS, "half", bitmap=False, async_=True) == full
    # the C entry points with counts NULL (the binding always passes the blocking form its count words)
    want, good, _ = expected(sel, idx, srcs, SRC_ROWS)
    dsel, didx, dsrcs = hj.column(mask_words(sel, "half")), hj.column(idx), [hj.column(s) for s in srcs]
    arr = api.C.c_void_p * 2
    for form in (hj.lib.hjgpu_gather_selected, hj.lib.hjgpu_gather_selected_async):
        douts = [hj.column(np.full(n + EXTRA, CANARY, np.uint32)) for _ in srcs]
        dbits = hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32))
        assert form(hj.handle, dsel.ptr, didx.ptr, n, 2, arr(*[d.ptr for d in dsrcs]), SRC_ROWS, arr(*[d.ptr for d in douts]), dbits.ptr, None, None) == api.OK
        hj.synchronize()
        for c, d in enumerate(douts):
            check_column(d.download(), want[c], ("counts NULL", form.__name__, c))
        check_bitmap(dbits.download(), good, CANARY, ("counts NULL", form.__name__))
    bad_idx = indices(n, SRC_ROWS, seed=32, bad=[SRC_ROWS, 0xFFFFFFFE])
    want, good, beyond = expected(sel, bad_idx, srcs, SRC_ROWS)
    assert beyond.any()
    didx.upload(bad_idx)
    douts = [hj.column(np.full(n + EXTRA, CANARY, np.uint32)) for _ in srcs]
    st = hj.lib.hjgpu_gather_selected(hj.handle, dsel.ptr, didx.ptr, n, 2, arr(*[d.ptr for d in dsrcs]), SRC_ROWS, arr(*[d.ptr for d in douts]), None, None, None)
    assert st == api.ERANGE and b"src_rows" in hj.lib.hjgpu_last_error(hj.handle)
    for c, d in enumerate(douts):
        check_column(d.download(), want[c], ("counts NULL, bad indices", c))


def test_n_zero_accepts_null(hj):
    assert hj.gather_selected(None, None, 0, [None], 0, [None]) == (0, 0)
    d_counts = hj.column(np.full(2, 77, np.uint64), np.uint64)
    hj.gather_selected_async(None, None, 0, [None, None], 5, [None, None], None, d_counts)
    hj.synchronize()
    assert [int(v) for v in d_counts.download()] == [0, 0]
    assert hj.lib.hjgpu_gather_selected(hj.handle, None, None, 0, 1, None, 0, None, None, None, None) == api.OK


def test_refusals(hj):
    """each returns before anything is enqueued: the canaries, the mask, the index and the sources are untouched afterwards"""
    import torch
    n, src_rows = 1000, 2000
    words = np.concatenate([pack(selection("half", 16384, seed=6)), np.full(4, ONES, np.uint32)])      # room for shifted and overlapping pointers
    dsel = hj.column(words)
    hidx = np.concatenate([indices(n, src_rows, seed=2), np.full(64, CANARY, np.uint32)])
    didx = hj.column(hidx)
    hsrc = sources(2, src_rows + 64, seed=3)
    dsrc = [hj.column(s) for s in hsrc]
    dout = [hj.column(np.full(2048, CANARY, np.uint32)) for _ in range(2)]
    dbits = hj.column(np.full(1024, CANARY, np.uint32))
    d_counts = hj.column(np.full(4, 77, np.uint64), np.uint64)
    srcs, outs = [d.ptr for d in dsrc], [d.ptr for d in dout]
    last_word = 4 * ((n + 31) // 32 - 1) // 16 * 16                  # the 16-byte vector that holds a bitmap's last word
    last_row = 4 * (n - 1) // 16 * 16                                # ... a column's last row

    def blocking(bits=dsel.ptr, idx=didx.ptr, n=n, srcs=srcs, src_rows=src_rows, outs=outs, bits_out=dbits.ptr, stream=None, **_):
        return hj.gather_selected(bits, idx, n, srcs, src_rows, outs, bits_out, stream=stream)

    def enqueue(bits=dsel.ptr, idx=didx.ptr, n=n, srcs=srcs, src_rows=src_rows, outs=outs, bits_out=dbits.ptr, counts=d_counts.ptr, stream=None):
        return hj.gather_selected_async(bits, idx, n, srcs, src_rows, outs, bits_out, counts, stream=stream)

    for call in (blocking, enqueue):
        cases = [("no column", dict(srcs=[], outs=[]), api.EINVAL, "ncols"),
                 ("five columns", dict(srcs=srcs * 2 + srcs[:1], outs=outs * 2 + outs[:1]), api.EINVAL, "ncols"),
                 ("null source", dict(srcs=[srcs[0], None]), api.EINVAL, "null"),
                 ("null output", dict(outs=[None, outs[1]]), api.EINVAL, "null"),
                 ("null index", dict(idx=None), api.EINVAL, "null"),
                 ("src_rows 2^32", dict(src_rows=1 << 32), api.EINVAL, "src_rows"),
                 ("misaligned mask", dict(bits=dsel.ptr + 4), api.EALIGN, "d_select_bits"),
                 ("misaligned index", dict(idx=didx.ptr + 4), api.EALIGN, "d_idx"),
                 ("misaligned source", dict(srcs=[srcs[0], srcs[1] + 8]), api.EALIGN, "source"),
                 ("misaligned output", dict(outs=[outs[0] + 4, outs[1]]), api.EALIGN, "output"),
                 ("misaligned bitmap", dict(bits_out=dbits.ptr + 8), api.EALIGN, "d_bits_out"),
                 ("output over the index's last row", dict(outs=[outs[0], didx.ptr + last_row]), api.EINVAL, "overlaps"),
                 ("both outputs the index", dict(outs=[didx.ptr, didx.ptr]), api.EINVAL, "overlaps"),
                 ("outputs overlapping by one vector", dict(outs=[outs[0], outs[0] + last_row]), api.EINVAL, "overlaps"),
                 ("output is a source", dict(outs=[srcs[1], outs[1]]), api.EINVAL, "overlaps"),
                 ("output over a source's last row", dict(outs=[outs[0], srcs[0] + 4 * (src_rows - 1) // 16 * 16]), api.EINVAL, "overlaps"),
                 ("output inside the mask", dict(outs=[dsel.ptr + last_word, outs[1]]), api.EINVAL, "overlaps"),
                 ("bitmaps overlapping by one word", dict(bits_out=dsel.ptr + last_word), api.EINVAL, "overlaps"),
                 ("bitmap inside the index", dict(bits_out=didx.ptr + last_row), api.EINVAL, "overlaps"),
                 ("bitmap inside an output", dict(bits_out=outs[1] + 16), api.EINVAL, "overlaps"),
                 ("bitmap inside a source", dict(bits_out=srcs[0] + 16), api.EINVAL, "overlaps")]
        if call is enqueue:
            cases += [("misaligned d_counts", dict(counts=d_counts.ptr + 8), api.EALIGN, "d_counts"),
                      ("d_counts inside the mask", dict(counts=dsel.ptr + 16), api.EINVAL, "overlaps"),
                      ("d_counts inside the index", dict(counts=didx.ptr + 16), api.EINVAL, "overlaps"),
                      ("d_counts inside an output", dict(counts=outs[1] + 16), api.EINVAL, "overlaps"),
                      ("d_counts inside a source", dict(counts=srcs[1] + 16), api.EINVAL, "overlaps"),
                      ("d_counts inside the bitmap", dict(counts=dbits.ptr + 16), api.EINVAL, "overlaps")]
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
    arr = api.C.c_void_p * 2
    assert hj.lib.hjgpu_gather_selected(hj.handle, dsel.ptr, didx.ptr, n, 2, None, src_rows, arr(*outs), dbits.ptr, None, None) == api.EINVAL
    hj.synchronize()
    assert all(np.all(d.download() == CANARY) for d in dout + [dbits]), "a refused call wrote an output"
    assert np.array_equal(dsel.download(), words) and np.array_equal(didx.download(), hidx)
    assert all(np.array_equal(d.download(), x) for d, x in zip(dsrc, hsrc))
    assert [int(x) for x in d_counts.download()] == [77] * 4
    # the same pointers, accepted: plain integers as well as DeviceColumns; the same source twice; outputs side by side without a shared byte
    sel = np.unpackbits(words[:(n + 31) // 32].view(np.uint8), bitorder="little")[:n].astype(bool)
    want, good, beyond = expected(sel, hidx[:n], [hsrc[0], hsrc[0]], src_rows)
    assert not beyond.any()
    assert blocking(srcs=[srcs[0], srcs[0]], outs=[outs[0], outs[0] + 4 * ((n + 3) // 4 * 4)]) == (int(good.sum()), 0)
    raw = dout[0].download()
    assert np.array_equal(raw[:n], want[0]) and np.array_equal(raw[(n + 3) // 4 * 4:][:n], want[1])
    check_bitmap(dbits.download(), good, CANARY, "accepted")


def test_enqueue_only(hj):
    """two gathers of different shapes and a filter back to back on one stream, no host wait in between; the status of the join before
    them stays what it was"""
    ik, iv, ok_ = relations(500, 1000, 0.5, seed=10)
    ik[123] = 0                                                      # the preceding join's status: HJGPU_EZEROKEY
    rk, rv, sk = col(hj, ik), col(hj, iv), col(hj, ok_)
    dv, db = outputs(hj, len(ok_), "both")
    d_res = hj.column(4, np.uint64)
    hj.reserve(len(ik), len(ok_))
    hj.npj_lookup_async(rk, rv, len(ik), sk, len(ok_), None, dv, db, d_res)
    runs = []
    for n, kind, ncols, bad in [(70_013, "half", 3, ()), (20_001, "null", 1, (SRC_ROWS + 5,))]:
        sel, idx, srcs = sel_of(kind, n, seed=n), indices(n, SRC_ROWS, seed=n + 1, bad=bad), sources(ncols, SRC_ROWS, seed=n + 2)
        want, good, beyond = expected(sel, idx, srcs, SRC_ROWS)
        runs.append(dict(n=n, want=want, good=good, beyond=beyond, dsel=hj.column(mask_words(sel, kind)) if kind != "null" else None,
                         didx=hj.column(idx), dsrcs=[hj.column(s) for s in srcs],
                         douts=[hj.column(np.full(n + EXTRA, CANARY, np.uint32)) for _ in srcs],
                         dbits=hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32)),
                         d_counts=hj.column(np.full(4, 77, np.uint64), np.uint64)))
    hj.gather_selected(None, None, 0, [None], 0, [None])             # (the contexts' count words first: making them would wait for the device)
    hj.filter_selected(None, 0, [None], [(0, 0)])
    d_pass = hj.column(np.full(2, 77, np.uint64), np.uint64)
    r0 = runs[0]
    hj.gather_selected_async(r0["dsel"], r0["didx"], r0["n"], r0["dsrcs"], SRC_ROWS, r0["douts"], r0["dbits"], r0["d_counts"])
    # the filter reads the first gather's output column 0 under its bitmap: a range that keeps everything but the genuine 0xFFFFFFFF values
    hj.filter_selected_async(r0["dbits"], r0["n"], [r0["douts"][0]], [(0, NULL - 1)], None, d_pass)
    r1 = runs[1]
    hj.gather_selected_async(r1["dsel"], r1["didx"], r1["n"], r1["dsrcs"], SRC_ROWS, r1["douts"], r1["dbits"], r1["d_counts"])
    with pytest.raises(HjGpuError) as e:
        hj.get_async_status()                                        # waits for the stream
    assert e.value.status == api.EZEROKEY
    for r in runs:
        assert [int(v) for v in r["d_counts"].download()] == [int(r["good"].sum()), int(r["beyond"].sum()), 77, 77]
        for c, d in enumerate(r["douts"]):
            check_column(d.download(), r["want"][c], ("async", r["n"], c))
        check_bitmap(r["dbits"].download(), r["good"], CANARY, ("async", r["n"]))
    assert runs[1]["beyond"].any()
    assert [int(v) for v in d_pass.download()] == [int((r0["good"] & (r0["want"][0] != NULL)).sum()), 77]


def test_stats(hj):
    S = hj.counter("gather_step_rows")
    n = S + 4099
    run(hj, indices(n, SRC_ROWS, seed=3), sel_of("half", n, seed=5), sources(2, SRC_ROWS, seed=4), SRC_ROWS, "half")
    s = hj.stats()
    print(s)
    assert s["ms_total"] >= s["ms_join"] > 0, s
    assert s["ms_histogram"] > 0 and s["ms_total"] >= (s["ms_histogram"] + s["ms_join"]) * (1 - 1e-5), s
    for k in ("ms_plan", "ms_scatter0", "ms_scatter1", "ms_scatter2", "ms_build", "ms_close_gaps", "ms_inner_wait"):
        assert s[k] == 0, (k, s)
    assert s["fanout1"] == 0 and s["fanout2"] == 0 and s["buckets"] == 0 and s["groups"] == 0, s
    with pytest.raises(HjGpuError) as e:
        hj.counter("no_such_counter")
    assert "gather_step_rows" in str(e.value)


def _sorted_rows(*cols):
    order = np.lexsort(tuple(reversed(cols)))
    return [np.asarray(c)[order] for c in cols]


def test_left_outer_join_rows_with_further_columns(hj):
    """hjgpu_phj under HJGPU_FLAG_LEFT_OUTER whose two payload columns are the relations' row numbers; two further columns of each relation
    gathered by the result's d_outer_vals / d_inner_vals.  The multiset of five-column rows (key, s_a, s_b, r_a, r_b) equals numpy's left
    outer join, the NULL rows' (NULL, NULL) on the build side included; duplicated build keys, probe keys without a match"""
    inner, outer = 3000, 5000
    ik, _, ok, _ = join_relations(inner, outer, 0.6, seed=41, distinct=700)
    rng = np.random.default_rng(42)
    r_a, r_b, s_a, s_b = (rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32) for m in (inner, inner, outer, outer))
    # numpy: every (probe row, build row) pair of equal keys, then one NULL row per probe row without a match
    order = np.argsort(ik, kind="stable")
    lo, hi = np.searchsorted(ik[order], ok, "left"), np.searchsorted(ik[order], ok, "right")
    cnt = (hi - lo).astype(np.int64)
    probe = np.repeat(np.arange(outer), cnt)
    build = order[np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
    lone = np.flatnonzero(cnt == 0)
    assert len(lone) > 100 and cnt.max() > 1
    nulls = np.full(len(lone), NULL, np.uint32)
    want = _sorted_rows(np.concatenate([ok[probe], ok[lone]]), np.concatenate([s_a[probe], s_a[lone]]), np.concatenate([s_b[probe], s_b[lone]]),
                        np.concatenate([r_a[build], nulls]), np.concatenate([r_b[build], nulls]))
    J = len(want[0])
    rk, rv, sk, sv = hj.column(ik), hj.column(np.arange(inner, dtype=np.uint32)), hj.column(ok), hj.column(np.arange(outer, dtype=np.uint32))
    cap = hj.output_capacity(1, outer, J + outer, 0)
    dk, do, di = (hj.column(np.zeros(cap, np.uint32)) for _ in range(3))
    prm = PhjParams(); prm.flags = H.FLAG_LEFT_OUTER
    res = hj.phj(rk, rv, inner, sk, sv, outer, params=prm, out=(dk, do, di, cap, 0))
    assert res[0] == J
    outs = [hj.column(np.full(J + EXTRA, CANARY, np.uint32)) for _ in range(4)]
    bits = hj.column(np.full((J + 31) // 32 + EXTRA, CANARY, np.uint32))
    assert hj.gather_selected(None, do, J, [hj.column(s_a), hj.column(s_b)], outer, outs[:2]) == (J, 0)
    assert hj.gather_selected(None, di, J, [hj.column(r_a), hj.column(r_b)], inner, outs[2:], bits) == (J - len(lone), 0)
    got = _sorted_rows(dk.download(J), *[d.download(J) for d in outs])
    for c, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), ("column", c, np.flatnonzero(g != w)[:8])
    assert int(np.unpackbits(bits.download()[:(J + 31) // 32].view(np.uint8)).sum()) == J - len(lone)
    assert all(np.all(d.download()[J:] == CANARY) for d in outs)


def test_a_star_query_with_two_attributes(hj):
    """WHERE discount BETWEEN 1 AND 3 AND d.region = 2 GROUP BY d.nation, d.city SUM(measure): a filter makes the bitmap, a selected
    look-up whose build payload is the dimension's ROW NUMBER narrows it in place, the gather fetches region, nation and city of that row
    under the narrowed bitmap, a filter on region narrows it again, group_sum by (nation, city) ends the query; the same in numpy"""
    n, drows = 200_003, 1000
    rng = np.random.default_rng(61)
    dk, _, fk = relations(drows, n, 0.5, seed=62)
    rownum = np.arange(drows, dtype=np.uint32)
    region, nation, city = (rng.integers(0, m, drows).astype(np.uint32) for m in (5, 7, 3))
    discount = rng.integers(0, 11, n).astype(np.uint32)
    measure = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ddisc, dmeas, dfk, ddk, drow = [hj.column(x) for x in (discount, measure, fk, dk, rownum)]
    bits = hj.column(np.full((n + 31) // 32 + EXTRA, CANARY, np.uint32))
    rows, _ = outputs(hj, n, "vals")
    fact = (discount >= 1) & (discount <= 3)
    assert hj.filter_selected(None, n, [ddisc], [(1, 3)], bits) == int(fact.sum())
    hj.lookup_selected(ddk, drow, drows, dfk, n, select_bits=bits, vals_out=rows, match_bits=bits)
    hit, looked, _ = want_selected(dk, rownum, fk, fact)
    attrs = [hj.column(np.full(n + EXTRA, CANARY, np.uint32)) for _ in range(3)]
    # an unmatched but selected row would hold HJGPU_NULL_VAL as its row number and pass through as NULL: here the bitmap is already narrowed
    assert hj.gather_selected(bits, rows, n, [hj.column(region), hj.column(nation), hj.column(city)], drows, attrs, bits) == (int(hit.sum()), 0)
    safe = np.where(hit, looked, 0)
    for d, a in zip(attrs, (region, nation, city)):
        check_column(d.download(), np.where(hit, a[safe], NULL).astype(np.uint32), "attribute")
    final = hit & (region[safe] == 2)
    assert hj.filter_selected(bits, n, [attrs[0]], [(2, 2)], bits) == int(final.sum())
    check_bitmap(bits.download(), final, CANARY, "chain")
    pair = nation[safe][final].astype(np.uint64) << np.uint64(32) | city[safe][final].astype(np.uint64)
    keys, inv = np.unique(pair, return_inverse=True)
    counts = np.bincount(inv.reshape(-1), minlength=len(keys)).astype(np.uint64)
    sums = np.zeros(len(keys), np.uint64)
    np.add.at(sums, inv.reshape(-1), measure[final].astype(np.uint64))
    J = len(keys)
    assert 10 < J <= 21
    k0, k1, cout, sout = hj.column(J, np.uint32), hj.column(J, np.uint32), hj.column(J, np.uint64), hj.column(J, np.uint64)
    assert hj.group_sum(bits, n, [attrs[1], attrs[2]], [dmeas], [k0, k1], [sout], cout, capacity=J) == J
    gk = k0.download().astype(np.uint64) << np.uint64(32) | k1.download().astype(np.uint64)
    order = np.argsort(gk)
    assert np.array_equal(gk[order], keys) and np.array_equal(cout.download()[order], counts) and np.array_equal(sout.download()[order], sums)
