"""GPU tests of the build side partitioned beside the probe side: a blocking two-pass PHJ with a claimed probe side runs the build side's
whole chain (K4, K5, K5b, K6 x 2) on the context's side stream while the probe side goes through its two passes on the caller's
(options "build_beside", default 1, and "build_cus").  The form (build_beside=1), the one-stream order (build_beside=0) and the exact path
(exact_probe_counts=1) are compared with each other and with the oracle, aggregates and rows.

Two passes are forced at small sizes with explicit fan-outs.  The library's own choice of CUs steps aside below 2^20 probe rows, so the
tests name their "build_cus" unless they are about that choice (which also wants 12 probe rows per build row).  Every test takes a
context of its own: a fallback makes the context's later joins exact, and the session context must not inherit options."""
import functools
import math
import threading

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from helpers import materialised_rows, sort_rows

pytestmark = pytest.mark.gpu

F1, F2 = 16, 8              # explicit fan-outs: a two-pass plan (the only one with a claimed probe side) at any size
TILE = 16384                # tuples of one K6 tile at these fan-outs
NULL = 0xFFFFFFFF
M64 = (1 << 64) - 1
# (inner, outer): one tile of R and the smallest build side that is no broadcast join; fewer tiles of R than its workgroups; a build
# side whose last tile is ragged; the probe side over long before the build side
SHAPES = {"one_tile": (TILE, 3_000_017), "few_tiles": (20 * TILE, 3_000_000), "mid": (200_000, 2_999_999), "short_probe": (200_000, 1000)}


@pytest.fixture
def ctx():
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


@functools.lru_cache(maxsize=None)
def _case(inner, outer, seed=0):
    """Relations (unique build keys; a third of the probe rows carries one, the others none), made once per shape and never written to,
    with their sorted result rows."""
    rng = np.random.default_rng(1000 * inner + outer + seed)
    pool = np.unique(rng.integers(1, 2**32 - 1, size=2 * inner + 4096, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    ik, miss = pool[:inner].copy(), pool[inner:]
    iv = rng.integers(0, 2**32 - 1, size=inner, dtype=np.uint64).astype(np.uint32)
    hit = rng.random(outer) < 1 / 3
    ok = np.where(hit, ik[rng.integers(0, inner, size=outer)], miss[rng.integers(0, len(miss), size=outer)]).astype(np.uint32)
    ov = rng.integers(0, 2**32 - 1, size=outer, dtype=np.uint64).astype(np.uint32)
    for a in (ik, iv, ok, ov):
        a.setflags(write=False)
    return ik, iv, ok, ov, materialised_rows(ik, iv, ok, ov)


@functools.lru_cache(maxsize=None)
def _want(oracle, inner, outer):
    """the oracle's aggregates, once per shape"""
    ik, iv, ok, ov, _ = _case(inner, outer)
    return tuple(oracle.join_definition(ik, iv, ok, ov))


def _params(flags=0):
    return H.PhjParams(fanout1=F1, fanout2=F2, flags=flags)


def _upload(hj, ik, iv, ok, ov):
    return [hj.column(a) if len(a) else hj.column(np.zeros(4, np.uint32)) for a in (ik, iv, ok, ov)]


def _rows(hj, cols, inner, outer, prm, count, stream=None):
    """the join with materialised rows: (aggregates, sorted rows)"""
    block = 4096
    cap = hj.output_capacity(1, outer, count, block)
    out = [hj.column(max(cap, 4)) for _ in range(3)]
    res = hj.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, prm, out=(out[0], out[1], out[2], cap, block), stream=stream)
    got = sort_rows(*(c.download()[:res[0]] for c in out))
    for c in out:
        c.free()
    return tuple(res), got


def _same_rows(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_stats(hj, beside):
    s = hj.stats()
    times = {k: v for k, v in s.items() if k.startswith("ms_")}
    assert times and all(math.isfinite(v) and v >= 0 for v in times.values()), times
    if beside:
        # the phases on the caller's stream lie inside the call's span (the build side's spans belong to the side stream).  Every span is
        # its own hipEventElapsedTime of its own pair of events, rounded to a float on its own: 1 us of room for that rounding
        for k in ("ms_scatter1", "ms_scatter2", "ms_inner_wait", "ms_join", "ms_close_gaps"):
            assert s[k] <= s["ms_total"] + 1e-3, (k, times)
    assert s["fanout1"] == F1 and s["fanout2"] == F2


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_form_the_one_stream_order_and_the_exact_path_agree_with_the_oracle(ctx, oracle, shape):
    inner, outer = SHAPES[shape]
    ik, iv, ok, ov, rows = _case(inner, outer)
    want = _want(oracle, inner, outer)
    assert want[0] == len(rows[0])
    cols = _upload(ctx, ik, iv, ok, ov)
    ctx.set_option("build_cus", 24)
    # aggregates only, then rows: the form
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == want
    assert ctx.counter("build_beside") == 1
    _check_stats(ctx, beside=True)
    got = _rows(ctx, cols, inner, outer, _params(), want[0])
    assert got[0] == want and _same_rows(got[1], rows)
    assert ctx.counter("build_beside") == 2 and ctx.counter("probe_fallbacks") == 0
    # the one-stream order
    ctx.set_option("build_beside", 0)
    got = _rows(ctx, cols, inner, outer, _params(), want[0])
    assert got[0] == want and _same_rows(got[1], rows)
    assert ctx.counter("build_beside") == 2 and ctx.counter("probe_exact") == 0
    _check_stats(ctx, beside=False)
    # the exact path never takes the form
    ctx.set_option("build_beside", 1)
    ctx.set_option("exact_probe_counts", 1)
    got = _rows(ctx, cols, inner, outer, _params(), want[0])
    assert got[0] == want and _same_rows(got[1], rows)
    assert ctx.counter("build_beside") == 2


@pytest.mark.parametrize("inner,outer", [(200_000, 0), (0, 1000), (0, 0)])
def test_the_form_steps_aside_without_rows(ctx, inner, outer):
    ik, iv, ok, ov, _ = _case(200_000, 1000)
    cols = _upload(ctx, ik[:inner], iv[:inner], ok[:outer], ov[:outer])
    ctx.set_option("build_cus", 24)
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == (0, 0, 0, 0)
    assert ctx.counter("build_beside") == 0
    _check_stats(ctx, beside=False)


def test_the_librarys_own_choice_overlaps_large_probe_sides_only(ctx, oracle):
    """option build_cus = 0: the committed default from 2^20 probe rows (and 128 CUs) on when the probe side has 12 rows and more per build
    row (mid: 15); the one-stream order for a short probe side and for one that is only 9 times its build side (few_tiles)"""
    assert ctx.device_info()["compute_units"] >= 128
    for shape, moved in (("mid", 1), ("short_probe", 0), ("few_tiles", 0)):
        inner, outer = SHAPES[shape]
        ik, iv, ok, ov, _ = _case(inner, outer)
        cols = _upload(ctx, ik, iv, ok, ov)
        before = ctx.counter("build_beside")
        assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == _want(oracle, inner, outer)
        assert ctx.counter("build_beside") == before + moved
        _check_stats(ctx, beside=bool(moved))


def test_a_solo_join_stays_on_one_stream(ctx, oracle):
    """option solo: the caller's promise of one stream, on which K6's partial-line stores are plain - such a join never forks, whatever
    build_beside and build_cus say"""
    inner, outer = SHAPES["mid"]
    ik, iv, ok, ov, _ = _case(inner, outer)
    want = _want(oracle, inner, outer)
    cols = _upload(ctx, ik, iv, ok, ov)
    ctx.set_option("solo", 1)
    for cus in (0, 24):
        ctx.set_option("build_cus", cus)
        assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == want
        assert ctx.counter("build_beside") == 0
        _check_stats(ctx, beside=False)
    ctx.set_option("solo", 0)
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == want
    assert ctx.counter("build_beside") == 1 and ctx.counter("probe_fallbacks") == 0


@pytest.mark.parametrize("where", ["default_stream", "non_blocking_stream"])
def test_callers_stream(ctx, oracle, where):
    import torch
    inner, outer = SHAPES["mid"]
    ik, iv, ok, ov, rows = _case(inner, outer)
    want = _want(oracle, inner, outer)
    cols = _upload(ctx, ik, iv, ok, ov)
    ctx.set_option("build_cus", 24)
    ts = torch.cuda.Stream() if where == "non_blocking_stream" else None      # (torch's streams are hipStreamNonBlocking)
    stream = ts.cuda_stream if ts is not None else None
    for _ in range(3):
        assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params(), stream=stream) == want
    got = _rows(ctx, cols, inner, outer, _params(), want[0], stream=stream)
    assert got[0] == want and _same_rows(got[1], rows)
    assert ctx.counter("build_beside") == 4
    _check_stats(ctx, beside=True)


def test_unique(ctx, oracle):
    """_UNIQUE (first match only) over unique build keys: the plain join's result, on all three roads"""
    inner, outer = SHAPES["mid"]
    ik, iv, ok, ov, _ = _case(inner, outer)
    want = _want(oracle, inner, outer)
    cols = _upload(ctx, ik, iv, ok, ov)
    ctx.set_option("build_cus", 24)
    prm = _params(H.api.FLAG_UNIQUE)
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, prm) == want
    assert ctx.counter("build_beside") == 1
    _check_stats(ctx, beside=True)
    ctx.set_option("build_beside", 0)
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, prm) == want
    ctx.set_option("exact_probe_counts", 1)
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, prm) == want
    assert ctx.counter("build_beside") == 1


def test_right_outer_marks_build_rows(ctx):
    """a mode that marks build rows: the bitmap's clear and the tail kernel follow the join of the two streams"""
    inner, outer = SHAPES["mid"]
    ik, iv, ok, ov, rows = _case(inner, outer)
    rnull = ~np.isin(ik, ok)
    nr = int(rnull.sum())
    assert 0 < nr < inner
    k = np.concatenate([rows[0], ik[rnull]])
    o = np.concatenate([rows[1], np.full(nr, NULL, np.uint32)])
    i = np.concatenate([rows[2], iv[rnull]])
    want_rows = sort_rows(k, o, i)
    want = (len(k), _sum(k), _sum(rows[1]), _sum(i))
    cols = _upload(ctx, ik, iv, ok, ov)
    ctx.set_option("build_cus", 24)
    prm = _params(H.FLAG_RIGHT_OUTER)
    got = _rows(ctx, cols, inner, outer, prm, want[0])
    assert got[0] == want and _same_rows(got[1], want_rows)
    assert ctx.counter("build_beside") == 1
    _check_stats(ctx, beside=True)
    ctx.set_option("build_beside", 0)
    got0 = _rows(ctx, cols, inner, outer, prm, want[0])
    assert got0[0] == want and _same_rows(got0[1], want_rows)
    assert ctx.counter("build_beside") == 1


@pytest.mark.parametrize("which", ["least", "largest"])
def test_build_cus_at_its_bounds(ctx, oracle, which):
    cus = ctx.device_info()["compute_units"]
    inner, outer = SHAPES["few_tiles"]
    ik, iv, ok, ov, rows = _case(inner, outer)
    want = _want(oracle, inner, outer)
    cols = _upload(ctx, ik, iv, ok, ov)
    for bad in (cus, cus + 7, -1):
        with pytest.raises(H.HjGpuError):
            ctx.set_option("build_cus", bad)
    ctx.set_option("build_cus", 1 if which == "least" else cus - 1)
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == want
    got = _rows(ctx, cols, inner, outer, _params(), want[0])
    assert got[0] == want and _same_rows(got[1], rows)
    assert ctx.counter("build_beside") == 2
    _check_stats(ctx, beside=True)


def test_fifty_joins_back_to_back_alternating_two_shapes(ctx, oracle):
    """meta, tickets, cursors and both streams are reused across the join of the two streams: every result is checked"""
    shapes = [SHAPES["mid"], SHAPES["few_tiles"]]
    cols = [_upload(ctx, *_case(*s)[:4]) for s in shapes]
    want = [_want(oracle, *s) for s in shapes]
    ctx.set_option("build_cus", 24)
    for n in range(50):
        (inner, outer), c = shapes[n & 1], cols[n & 1]
        assert ctx.phj(c[0], c[1], inner, c[2], c[3], outer, _params()) == want[n & 1], n
    assert ctx.counter("build_beside") == 50 and ctx.counter("probe_fallbacks") == 0
    _check_stats(ctx, beside=True)


def test_a_full_region_falls_back_with_the_form_on(ctx, oracle):
    """regions without any slack (option probe_slack=0): the join is done again exactly on one stream, the fallback is counted, and the
    next call is right too"""
    inner, outer = SHAPES["mid"]
    ik, iv, ok, ov, _ = _case(inner, outer)
    want = _want(oracle, inner, outer)
    cols = _upload(ctx, ik, iv, ok, ov)
    ctx.set_option("build_cus", 24)
    ctx.set_option("probe_slack", 0)
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == want
    assert ctx.counter("build_beside") == 1                      # the optimistic attempt took the form
    assert ctx.counter("probe_fallbacks") == 1 and ctx.counter("probe_exact") == 1
    _check_stats(ctx, beside=False)                              # the statistics are the second, exact join's
    assert ctx.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params()) == want
    assert ctx.counter("probe_fallbacks") == 1 and ctx.counter("build_beside") == 1      # exact at once: never the form


def test_two_contexts_on_two_host_threads(oracle):
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    shapes = [SHAPES["mid"], SHAPES["few_tiles"]]
    want = [_want(oracle, *s) for s in shapes]
    for s in shapes:
        _case(*s)
    failures = []

    def work(t):
        try:
            inner, outer = shapes[t]
            ik, iv, ok, ov, _ = _case(inner, outer)
            with H.HjGpu(0) as hj:
                cols = [hj.column(a) for a in (ik, iv, ok, ov)]
                try:
                    hj.set_option("build_cus", 24)
                    for n in range(8):
                        got = hj.phj(cols[0], cols[1], inner, cols[2], cols[3], outer, _params())
                        if got != want[t]:
                            failures.append((t, n, got, want[t]))
                    if hj.counter("build_beside") != 8:
                        failures.append((t, "counter", hj.counter("build_beside")))
                finally:
                    for c in cols:
                        c.free()
        except Exception as e:      # noqa: BLE001 - reported by the asserting thread
            failures.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failures, failures
