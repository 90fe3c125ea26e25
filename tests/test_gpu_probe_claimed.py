"""GPU tests of the claimed probe side: a blocking two-pass PHJ partitions its probe side without the histogram pass, into
optimistic regions, and joins again on the exact path when a region is full.  Results are bit-exact against the independent
definition of the join (helpers.numpy_join / materialised_rows) and against the exact path (option "exact_probe_counts").

Every test takes a context of its own: a fallback makes the context's later joins exact, and the session context must not
inherit that."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from helpers import numpy_join, materialised_rows, sort_rows

pytestmark = pytest.mark.gpu

INNER = 3_000_000          # > 640 partitions: a two-pass plan, the only one with a claimed probe side


@pytest.fixture
def ctx():
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    with H.HjGpu(0) as hj:
        yield hj


def _relations(inner, outer, seed, hot_share=0.0):
    rng = np.random.default_rng(seed)
    ik = np.unique(rng.integers(1, 2**32, size=inner + inner // 8, dtype=np.uint64).astype(np.uint32))[:inner]
    rng.shuffle(ik)
    iv = rng.integers(0, 2**32, size=inner, dtype=np.uint64).astype(np.uint32)
    ok = ik[rng.integers(0, inner, size=outer)]
    if hot_share:
        ok[rng.random(outer) < hot_share] = ik[17]
    ov = rng.integers(0, 2**32, size=outer, dtype=np.uint64).astype(np.uint32)
    return ik, iv, ok, ov


def _upload(hj, ik, iv, ok, ov, pad=0):
    """Columns on the device; the probe side starts `pad` words (a multiple of 4: 16-byte aligned) into its allocation."""
    z = np.zeros(pad, np.uint32)
    cols = [hj.column(ik), hj.column(iv), hj.column(np.concatenate([z, ok])), hj.column(np.concatenate([z, ov]))]
    return cols, (cols[0], cols[1], cols[2].ptr + 4 * pad, cols[3].ptr + 4 * pad)


@pytest.mark.parametrize("outer,pad", [(6_000_000, 0), (5_000_003, 4), (12_345_679, 12)])
def test_claimed_probe_side_is_exact(ctx, outer, pad):
    ik, iv, ok, ov = _relations(INNER, outer, seed=outer + pad)
    want = numpy_join(ik, iv, ok, ov)
    cols, (rk, rv, sk, sv) = _upload(ctx, ik, iv, ok, ov, pad)
    assert ctx.phj(rk, rv, INNER, sk, sv, outer) == want
    assert ctx.stats()["fanout2"] > 1
    assert ctx.counter("probe_fallbacks") == 0 and ctx.counter("probe_exact") == 0
    assert ctx.phj(rk, rv, INNER, sk, sv, outer) == want          # the cursors and regions of the first join are reset
    ctx.set_option("exact_probe_counts", 1)
    assert ctx.counter("probe_exact") == 1
    assert ctx.phj(rk, rv, INNER, sk, sv, outer) == want
    assert ctx.counter("probe_fallbacks") == 0
    for c in cols:
        c.free()


def test_claimed_probe_side_materialised_rows(ctx):
    outer = 4_000_037
    ik, iv, ok, ov = _relations(INNER, outer, seed=11)
    want = numpy_join(ik, iv, ok, ov)
    cols, (rk, rv, sk, sv) = _upload(ctx, ik, iv, ok, ov, pad=8)
    block = 4096
    cap = (want[0] // block + ctx.device_info()["compute_units"] * 16 + 8) * block
    jk, jo, ji = ctx.column(cap), ctx.column(cap), ctx.column(cap)
    assert ctx.phj(rk, rv, INNER, sk, sv, outer, out=(jk, jo, ji, cap, block)) == want
    assert ctx.counter("probe_fallbacks") == 0
    rows = sort_rows(jk.download()[:want[0]], jo.download()[:want[0]], ji.download()[:want[0]])
    for a, b in zip(rows, materialised_rows(ik, iv, ok, ov)):
        assert np.array_equal(a, b)
    for c in cols + [jk, jo, ji]:
        c.free()


def test_claimed_probe_side_unique(ctx):
    """_UNIQUE (first match only): claimed and exact probe sides give the same aggregates; with unique build keys both equal
    the plain join's."""
    outer = 7_000_001
    ik, iv, ok, ov = _relations(INNER, outer, seed=5)
    cols, (rk, rv, sk, sv) = _upload(ctx, ik, iv, ok, ov)
    prm = H.PhjParams(flags=H.api.FLAG_UNIQUE)
    got = ctx.phj(rk, rv, INNER, sk, sv, outer, prm)
    assert ctx.counter("probe_fallbacks") == 0
    assert got == numpy_join(ik, iv, ok, ov)
    ctx.set_option("exact_probe_counts", 1)
    assert ctx.phj(rk, rv, INNER, sk, sv, outer, prm) == got
    for c in cols:
        c.free()


def test_claimed_probe_side_unique_multi_fill_near_a_slice(ctx):
    """_UNIQUE with a build partition larger than one table fill (the <UNIQUE, DEDUP> join keeps one bit per probe row of a work
    item) and ~65 000 probe rows per partition, so that many regions hold more than one slice of HJ_JOIN_SLICE = 65 536 rows.
    The work items are planned for whole regions: no item gets more probe rows than the bitmap holds.  20 000 copies of one
    build tuple (same key, same payload): the first match of every probe row is determined, i.e. the join of the build side
    without the copies."""
    F1, F2 = 32, 27
    outer = F1 * F2 * 65_000
    ik, iv, ok, ov = _relations(INNER, outer, seed=65)
    ok[:50] = ik[17]                                              # the hot build key is probed, too
    ik_dup = np.concatenate([ik, np.full(20_000, ik[17], np.uint32)])
    iv_dup = np.concatenate([iv, np.full(20_000, iv[17], np.uint32)])
    want = numpy_join(ik, iv, ok, ov)
    cols, (rk, rv, sk, sv) = _upload(ctx, ik_dup, iv_dup, ok, ov)
    prm = H.PhjParams(fanout1=F1, fanout2=F2, flags=H.api.FLAG_UNIQUE)
    assert ctx.phj(rk, rv, len(ik_dup), sk, sv, outer, prm) == want
    assert ctx.counter("probe_fallbacks") == 0 and ctx.counter("probe_exact") == 0
    ctx.set_option("exact_probe_counts", 1)
    assert ctx.phj(rk, rv, len(ik_dup), sk, sv, outer, prm) == want
    for c in cols:
        c.free()


@pytest.mark.parametrize("kind", ["heavy_hitter", "zipf", "no_slack"])
def test_a_full_region_falls_back_to_the_exact_path(ctx, kind):
    """A probe side that does not fit the optimistic regions - one key in 30 % of the rows, a Zipf(1.2) probe side, or regions
    without any slack (option probe_slack=0) - is joined again exactly: right result, the fallback counted, and the context's
    later joins exact at once."""
    outer = 6_000_000
    if kind == "zipf":
        rng = np.random.default_rng(9)
        ik, iv, _, ov = _relations(INNER, outer, seed=9)
        ranks = np.minimum(rng.zipf(1.2, size=outer), INNER) - 1
        ok = ik[ranks.astype(np.int64)]
    else:
        ik, iv, ok, ov = _relations(INNER, outer, seed=21, hot_share=0.3 if kind == "heavy_hitter" else 0.0)
    if kind == "no_slack":
        ctx.set_option("probe_slack", 0)
    want = numpy_join(ik, iv, ok, ov)
    cols, (rk, rv, sk, sv) = _upload(ctx, ik, iv, ok, ov, pad=4)
    assert ctx.phj(rk, rv, INNER, sk, sv, outer) == want
    assert ctx.counter("probe_fallbacks") == 1
    assert ctx.counter("probe_exact") == 1
    assert ctx.phj(rk, rv, INNER, sk, sv, outer) == want
    assert ctx.counter("probe_fallbacks") == 1                   # the second join took the exact path at once
    for c in cols:
        c.free()
