"""GPU tests of right semi- and right anti-joins (HJGPU_FLAG_RIGHT_SEMI / _RIGHT_ANTI) through hjgpu_phj, hjgpu_cpra and hjgpu_npj, against
their definition on the host: RIGHT_SEMI is ik[np.isin(ik, ok)] with its iv, RIGHT_ANTI is ik[~np.isin(ik, ok)] with its iv - one row
(key, inner_val) per BUILD tuple, build-side duplicates one by one, probe-side duplicates never multiplying a row.  Exact equality:
aggregates (count, sum_keys, 0, sum_inner_vals), and rows after a lexsort.  The rows land in d_keys and d_inner_vals; d_outer_vals is
neither read nor written.  Out-of-scope entry points and flag combinations must refuse the flags instead of returning an inner join
(bits 32 and 64 used to be ignored).

Every test takes a context of its own: options set here must not reach the session's other tests."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd.api import PhjParams, NpjParams, HjGpuError

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
RSEMI, RANTI = H.FLAG_RIGHT_SEMI, H.FLAG_RIGHT_ANTI
NAMES = {RSEMI: "HJGPU_FLAG_RIGHT_SEMI", RANTI: "HJGPU_FLAG_RIGHT_ANTI"}
BOTH = [RSEMI, RANTI]
UNTOUCHED = 0xA5A5A5A5            # what the outer column is filled with before a join that must not write it


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


def want(ik, iv, ok, flags):
    """(aggregates, sorted rows) of the right semi- / anti-join: the build tuples whose key is / is not among the probe keys"""
    m = np.isin(ik, ok)
    sel = m if flags == RSEMI else ~m
    k, i = ik[sel], iv[sel]
    idx = np.lexsort((i, k))
    return (len(k), _sum(k), 0, _sum(i)), (k[idx], i[idx])


def relations(inner, outer, sel, seed, present=0.5, distinct=None, payload_max=2**32):
    """`distinct` (default: inner, unique) build keys; a `sel` share of the probe tuples carries a build key, and those are drawn from the
    first `present` share of the distinct build keys only: the others have no match.  Payloads take every value, 0xFFFFFFFF included."""
    rng = np.random.default_rng(seed)
    d = distinct or inner
    pool = np.unique(rng.integers(1, 2**32 - 1, size=2 * d + 64, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    build_keys, miss = pool[:d], pool[d:]
    ik = build_keys[rng.integers(0, d, size=inner)] if distinct else build_keys[:inner].copy()
    iv = rng.integers(0, payload_max, size=inner, dtype=np.uint64).astype(np.uint32)
    dp = int(d * present)
    hit = (rng.random(outer) < sel) & (dp > 0)
    ok = np.where(hit, build_keys[rng.integers(0, max(dp, 1), size=outer)], miss[rng.integers(0, len(miss), size=outer)]).astype(np.uint32)
    ov = rng.integers(0, 2**32, size=outer, dtype=np.uint64).astype(np.uint32)
    return ik, iv, ok, ov


def cols(hj, *arrays):
    return [hj.column(a) if len(a) else hj.column(np.zeros(4, np.uint32)) for a in arrays]


def _params(algo, prm, flags):
    if prm is None:
        prm = NpjParams() if algo == "npj" else PhjParams()
    prm.flags = flags
    return prm


ALGO_ID = {"npj": 0, "phj": 1, "cpra": 2}


def run(hj, algo, ik, iv, ok, ov, flags, prm=None, rows=True, capacity=None, block=0, outer_column=True):
    """the join's aggregates and its sorted rows.  The capacity is exactly hjgpu_output_capacity(true row count) unless given; the outer
    column, where one is passed, must come back as it went in"""
    rk, rv, sk, sv = cols(hj, ik, iv, ok, ov)
    prm = _params(algo, prm, flags)
    fn = {"phj": hj.phj, "cpra": hj.cpra, "npj": hj.npj}[algo]
    out, made = None, []
    if rows:
        cap = capacity if capacity is not None else hj.output_capacity(ALGO_ID[algo], len(ok), want(ik, iv, ok, flags)[0][0], block)
        dk, di = (hj.column(np.zeros(max(cap, 4), np.uint32)) for _ in range(2))
        do = hj.column(np.full(max(cap, 4), UNTOUCHED, np.uint32)) if outer_column else None
        made = [c for c in (dk, do, di) if c is not None]
        out = (dk, do, di, cap, block)
    try:
        res = fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=out)
        got = None
        if rows:
            n = res[0]
            k, i = dk.download(n), di.download(n)
            idx = np.lexsort((i, k))
            got = (k[idx], i[idx])
            if do is not None:
                assert np.all(do.download() == UNTOUCHED), "d_outer_vals was written"
    finally:
        for c in made + [rk, rv, sk, sv]:
            c.free()
    return tuple(res), got


def check(hj, algo, ik, iv, ok, ov, flags=BOTH, prm_fn=lambda: None, rows=True, block=0):
    """aggregates and rows against the oracle; the aggregate-only call gives the same aggregates"""
    for f in flags:
        agg, wanted = want(ik, iv, ok, f)
        res, _ = run(hj, algo, ik, iv, ok, ov, f, prm=prm_fn(), rows=False)
        print(algo, NAMES[f], "aggregate-only", res, "want", agg)
        assert res == agg, (algo, NAMES[f], "aggregate-only", res, agg)
        if rows:
            res, got = run(hj, algo, ik, iv, ok, ov, f, prm=prm_fn(), block=block)
            assert res == agg, (algo, NAMES[f], res, agg)
            assert all(np.array_equal(g, w) for g, w in zip(got, wanted)), (algo, NAMES[f])


ALGOS = [("phj", {}), ("cpra1", {}), ("cpra8", {}), ("cpra16", {}), ("npj", {}), ("npj", {"npj_refhash": 1})]
SOME = ["phj", "cpra8", "npj"]


def _prm(algo):
    if algo.startswith("cpra"):
        p = PhjParams(); p.chunks = int(algo[4:]); return p
    return None


def _algo(algo):
    return "cpra" if algo.startswith("cpra") else algo


@pytest.mark.parametrize("algo,opts", ALGOS)
@pytest.mark.parametrize("present", [0.0, 0.5, 1.0])
def test_aggregates_and_rows(ctx, algo, opts, present):
    """the first case fails without the feature: the flags used to be ignored, and the call returned the inner join"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(300_000, 1_000_003, 0.5, seed=int(present * 100) + 3, present=present)
    iv[5] = 0xFFFFFFFF                                  # an ordinary payload here: no NULL appears in these rows
    if algo != "npj":
        # every key value is legal on both sides of PHJ / CPRA: 0 on both sides (a match), 0xFFFFFFFF in the build side only and a
        # further extreme key in the probe side only
        ik[:2] = [0, 0xFFFFFFFF]
        ok[7919] = 0
        ok[2 * 7919] = 0xFFFFFFFE
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("algo", ["phj", "cpra8"])
def test_both_extreme_keys_on_both_sides(ctx, algo):
    ik, iv, ok, ov = relations(200_000, 600_001, 0.5, seed=5)
    ik[:2] = [0, 0xFFFFFFFF]
    iv[:2] = 0xFFFFFFFF
    ok[:4] = [0, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))
    ok[:4] = 1                                          # ... and on the build side only: both reported by RIGHT_ANTI
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("opts", [{}, {"npj_refhash": 1}])
def test_npj_probe_key_zero_matches_nothing(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(100_000, 400_003, 0.5, seed=12)
    ok[:5] = 0
    check(ctx, "npj", ik, iv, ok, ov)


@pytest.mark.parametrize("flags", BOTH)
def test_npj_build_key_zero_is_refused(ctx, flags):
    ik, iv, ok, ov = relations(10_000, 40_003, 0.5, seed=13)
    ik[17] = 0
    with pytest.raises(HjGpuError) as e:
        run(ctx, "npj", ik, iv, ok, ov, flags, rows=False)
    assert e.value.status == 5                          # HJGPU_EZEROKEY


@pytest.mark.parametrize("algo,opts", ALGOS)
def test_duplicated_build_keys(ctx, algo, opts):
    """16 copies of every build key: each copy of a present key is a row of RIGHT_SEMI, each copy of an absent one a row of RIGHT_ANTI"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(320_000, 500_001, 0.7, seed=14, distinct=20_000)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("algo,opts", ALGOS)
def test_duplicated_probe_keys(ctx, algo, opts):
    """2 000 distinct probe keys in 800 000 probe tuples: a build tuple is reported once however many probe tuples carry its key"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(200_000, 16, 0.5, seed=18)
    rng = np.random.default_rng(19)
    some = np.concatenate([ik[rng.choice(len(ik), size=1000, replace=False)], rng.integers(1, 2**32 - 1, size=1000, dtype=np.uint64).astype(np.uint32)])
    ok = some[rng.integers(0, len(some), size=800_003)]
    ov = rng.integers(0, 2**32, size=len(ok), dtype=np.uint64).astype(np.uint32)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("algo,opts", ALGOS)
def test_zipf_probe_keys(ctx, algo, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(250_000, 16, 0.5, seed=20)
    rng = np.random.default_rng(21)
    universe = np.concatenate([ik, np.setdiff1d(rng.integers(1, 2**32 - 1, size=250_000, dtype=np.uint64).astype(np.uint32), ik)])
    rng.shuffle(universe)
    ok = universe[(rng.zipf(1.2, size=1_200_007) - 1) % len(universe)]
    ov = rng.integers(0, 2**32, size=len(ok), dtype=np.uint64).astype(np.uint32)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("opts", [{}, {"join_cfg": "1024,14,2"}])
def test_several_probe_slices_per_partition(ctx, opts):
    """about 6 partitions of about 10 slices: each of 1000 build keys occurs exactly once in the probe side, anywhere in the column - a
    bitmap that is not combined across the work items of a partition misses some of them"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(20_000, 4_000_003, 0.0, seed=15)
    rng = np.random.default_rng(16)
    at = rng.choice(len(ok), size=1000, replace=False)
    ok[at] = ik[rng.choice(len(ik), size=1000, replace=False)]
    check(ctx, "phj", ik, iv, ok, ov, prm_fn=lambda: PhjParams(fanout1=3, fanout2=2))
    st = ctx.stats()
    parts = st["fanout1"] * st["fanout2"]
    assert parts == 6 and len(ok) / (parts * 65536) > 1, st


@pytest.mark.parametrize("algo,opts", ALGOS)
@pytest.mark.parametrize("in_probe", [True, False])
def test_heavy_build_key_multi_fill(ctx, algo, opts, in_probe):
    """20 000 copies of one build key: its partition takes several table fills (PHJ / CPRA: the mark_probe_kernel launch)"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(150_000, 600_001, 0.5, seed=51)
    ik[:20_000] = ik[0]
    if in_probe:
        ok[::3000] = ik[0]
    else:
        ok[ok == ik[0]] = 1
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("algo", ["phj", "cpra8"])
def test_chained_fallback(ctx, algo):
    ik, iv, ok, ov = relations(300_000, 1_000_003, 0.5, seed=52)
    ctx.set_option("force_chained", 1)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))
    ik[:20_000] = ik[0]                                  # ... and in the multi-fill launch
    ok[::3000] = ik[0]
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))
    ctx.set_option("force_chained", 0)
    # 3-5 copies of every build key: the cuckoo build gives up on its own
    rng = np.random.default_rng(53)
    keys = np.unique(rng.integers(1, 2**32 - 1, size=60_000, dtype=np.uint64).astype(np.uint32))
    ik = np.repeat(keys, rng.integers(3, 6, size=len(keys)))
    rng.shuffle(ik)
    iv = rng.integers(0, 2**32, size=len(ik), dtype=np.uint64).astype(np.uint32)
    ok = np.where(rng.random(400_001) < 0.5, keys[rng.integers(0, len(keys) // 2, size=400_001)],
                  rng.integers(1, 2**32 - 1, size=400_001, dtype=np.uint64).astype(np.uint32)).astype(np.uint32)
    ov = rng.integers(0, 2**32, size=len(ok), dtype=np.uint64).astype(np.uint32)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("no_broadcast", [0, 1])
@pytest.mark.parametrize("inner", [1, 1000, 6962])
def test_broadcast_sized_build_sides_take_the_partitioned_plan(ctx, inner, no_broadcast):
    ctx.set_option("no_broadcast", no_broadcast)
    ik, iv, ok, ov = relations(inner, 500_001, 0.5, seed=inner)
    ok[:16384] = np.arange(16384, dtype=np.uint32)
    check(ctx, "phj", ik, iv, ok, ov)
    st = ctx.stats()
    assert st["fanout1"] * st["fanout2"] >= 2, st        # partitioned: a broadcast join has no fan-out


@pytest.mark.parametrize("opts", [{}, {"exact_probe_counts": 1}, {"dense2": 1}, {"batch_tuples": 1 << 20}, {"solo": 1}])
def test_two_pass_plans(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(4_200_000, 6_000_001, 0.5, seed=21)
    check(ctx, "phj", ik, iv, ok, ov)
    assert ctx.stats()["fanout2"] > 1, ctx.stats()


@pytest.mark.parametrize("algo", ["cpra8", "cpra16"])
def test_two_pass_plan_with_chunks(ctx, algo):
    ik, iv, ok, ov = relations(4_200_000, 6_000_001, 0.5, seed=26)
    check(ctx, "cpra", ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


def test_one_pass_plan(ctx):
    ik, iv, ok, ov = relations(200_000, 2_000_001, 0.5, seed=22)
    check(ctx, "phj", ik, iv, ok, ov, prm_fn=lambda: PhjParams(fanout1=64, fanout2=1))
    check(ctx, "cpra", ik, iv, ok, ov, prm_fn=lambda: PhjParams(fanout1=64, fanout2=1, chunks=8))


@pytest.mark.parametrize("algo", SOME)
def test_mid_size(ctx, algo):
    """8 M x 64 M"""
    ik, iv, ok, ov = relations(8_000_000, 64_000_000, 0.5, seed=27)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


def test_partitions_with_build_rows_and_no_probe_rows(ctx):
    ik, iv, ok, ov = relations(3_000_000, 1000, 1.0, seed=17, present=1.0)
    check(ctx, "phj", ik, iv, ok, ov)
    check(ctx, "cpra", ik, iv, ok, ov, prm_fn=lambda: _prm("cpra8"))


@pytest.mark.parametrize("flags", BOTH)
def test_claimed_probe_side_falls_back_to_the_exact_path(ctx, flags):
    """a claimed probe side without slack overflows its regions: the join is done again exactly - the bitmap zeroed again, right rows"""
    ctx.set_option("probe_slack", 0)
    ik, iv, ok, ov = relations(3_000_000, 6_000_001, 0.5, seed=23)
    agg, wanted = want(ik, iv, ok, flags)
    res, got = run(ctx, "phj", ik, iv, ok, ov, flags)
    assert res == agg
    assert all(np.array_equal(g, w) for g, w in zip(got, wanted))
    assert ctx.counter("probe_fallbacks") > 0


@pytest.mark.parametrize("algo", ["phj", "cpra8"])
@pytest.mark.parametrize("group_device", [1, 0])
def test_grouped_plans(ctx, algo, group_device):
    for k, v in (("group_always", 1), ("group_from", 1000), ("group_inner", 100_000), ("group_device", group_device)):
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(800_000, 2_000_001, 0.5, seed=32)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))
    assert ctx.stats()["groups"] > 1


@pytest.mark.parametrize("group_device", [1, 0])
def test_grouped_plans_with_groups_without_probe_rows_and_without_build_rows(ctx, group_device):
    """many groups, few keys: 40 distinct build keys and 40 distinct probe keys of which 20 are build keys - most groups hold rows of one
    side only.  RIGHT_ANTI reports the build rows of a group without probe rows, RIGHT_SEMI skips such a group"""
    for k, v in (("group_always", 1), ("group_from", 2), ("group_inner", 1000), ("group_device", group_device)):
        ctx.set_option(k, v)
    rng = np.random.default_rng(101)
    keys = np.unique(rng.integers(1, 2**32 - 1, size=100, dtype=np.uint64).astype(np.uint32))[:60]
    ik = keys[rng.integers(0, 40, size=40_000)]
    iv = rng.integers(0, 2**32, size=len(ik), dtype=np.uint64).astype(np.uint32)
    ok = keys[rng.integers(20, 60, size=3001)]
    ov = rng.integers(0, 2**32, size=len(ok), dtype=np.uint64).astype(np.uint32)
    check(ctx, "phj", ik, iv, ok, ov)
    assert ctx.stats()["groups"] > 1


@pytest.mark.parametrize("flags", BOTH)
def test_a_group_beyond_group_slack_is_joined_again_host_planned(ctx, flags):
    """24 distinct build keys in 12 groups: the largest group is beyond the device plan's workspace.  The enqueue-only join marks its result
    (all ones), hjgpu_get_async_status joins again host-planned; the blocking form does the same inside the call"""
    rng = np.random.default_rng(11)
    distinct = rng.choice(np.arange(1, 1 << 31, dtype=np.uint32), size=24, replace=False)
    ik = np.repeat(distinct, 400_000)
    iv = rng.integers(0, 2**32, size=len(ik), dtype=np.uint64).astype(np.uint32)
    ok = np.concatenate([rng.choice(distinct[:12], size=3000), rng.integers(1 << 31, 2**32 - 1, size=3000, dtype=np.uint64).astype(np.uint32)])
    ov = rng.integers(0, 2**32, size=len(ok), dtype=np.uint64).astype(np.uint32)
    for n, v in (("group_from", 1000), ("group_always", 1), ("group_inner", len(ik) // 12), ("group_slack", 10)):
        ctx.set_option(n, v)
    agg, wanted = want(ik, iv, ok, flags)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d = ctx.column(4, np.uint64)
    ctx.phj_async(rk, rv, len(ik), sk, sv, len(ok), _params("phj", None, flags), d)
    ctx.synchronize()
    assert tuple(int(x) for x in d.download()) == (M64,) * 4          # a group was skipped: the result is MARKED, not partial
    ctx.get_async_status()                                             # ... and joined again, host-planned
    assert tuple(int(x) for x in d.download()) == agg
    for c in (rk, rv, sk, sv):
        c.free()
    res, got = run(ctx, "phj", ik, iv, ok, ov, flags)                  # the blocking form, with rows
    assert res == agg
    assert all(np.array_equal(g, w) for g, w in zip(got, wanted))


@pytest.mark.parametrize("algo,opts", ALGOS)
def test_empty_sides(ctx, algo, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(1000, 300_001, 0.5, seed=61)
    e = np.zeros(0, np.uint32)
    check(ctx, _algo(algo), e, e, ok, ov, prm_fn=lambda: _prm(algo))          # inner == 0: no rows, status OK
    check(ctx, _algo(algo), ik, iv, e, e, prm_fn=lambda: _prm(algo))          # outer == 0: RIGHT_SEMI is empty, RIGHT_ANTI every build tuple
    check(ctx, _algo(algo), e, e, e, e, prm_fn=lambda: _prm(algo))
    ik, iv, _, _ = relations(3_000_000, 10, 0.5, seed=62)
    check(ctx, _algo(algo), ik, iv, e, e, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("algo", SOME)
@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("bs", [0, 512, 256])
def test_exact_capacity_and_one_block_too_few(ctx, algo, flags, bs):
    """hjgpu_output_capacity(true row count) is enough (run's default capacity); one block less is HJGPU_EOVERFLOW with the exact count.
    Blocks below 512 rows take the row-by-row stores instead of emit4; 256 is the smallest block the library accepts"""
    ik, iv, ok, ov = relations(300_000, 1_000_003, 0.5, seed=71)
    agg, wanted = want(ik, iv, ok, flags)
    n, block = agg[0], bs or 65536
    res, got = run(ctx, _algo(algo), ik, iv, ok, ov, flags, prm=_prm(algo), block=bs)
    assert res == agg
    assert all(np.array_equal(g, w) for g, w in zip(got, wanted))
    # d_outer_vals = NULL is accepted
    res, got = run(ctx, _algo(algo), ik, iv, ok, ov, flags, prm=_prm(algo), block=bs, outer_column=False)
    assert res == agg
    assert all(np.array_equal(g, w) for g, w in zip(got, wanted))
    # one block too few for the rows: whole blocks only, and the last row no longer has a slot
    short = (n // block) * block if n % block else n - block
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    dk, di = ctx.column(np.zeros(max(short, 4), np.uint32)), ctx.column(np.zeros(max(short, 4), np.uint32))
    r = H.Result()
    fn = {"phj": ctx.lib.hjgpu_phj, "cpra": ctx.lib.hjgpu_cpra, "npj": ctx.lib.hjgpu_npj}[_algo(algo)]
    import ctypes as C
    prm = _params(_algo(algo), _prm(algo), flags)
    st = fn(ctx.handle, rk.ptr, rv.ptr, len(ik), sk.ptr, sv.ptr, len(ok), C.byref(prm), C.byref(r), ctx._out((dk, None, di, short, bs)), None)
    print(algo, NAMES[flags], "block", bs, "capacity", short, "status", st, "count", r.count, "want", n)
    assert st == 6                                                              # HJGPU_EOVERFLOW
    assert r.count == n                                                         # ... with result->count exact


@pytest.mark.parametrize("algo", ["phj", "npj"])
def test_block_size_64_is_below_the_smallest_block(ctx, algo):
    """a block of 64 rows is no block of this library (a wave's run of up to 256 rows must end inside the one block it claims; the smallest is
    256 rows): hjgpu_output_capacity and the join refuse it with HJGPU_EINVAL in these modes as in every other"""
    ik, iv, ok, ov = relations(10_000, 40_003, 0.5, seed=72)
    with pytest.raises(HjGpuError) as e:
        ctx.output_capacity(ALGO_ID[algo], len(ok), len(ik), 64)
    assert e.value.status == 1
    for flags in BOTH:
        with pytest.raises(HjGpuError) as e:
            run(ctx, algo, ik, iv, ok, ov, flags, capacity=1 << 20, block=64)
        assert e.value.status == 1 and "block_size" in str(e.value)


@pytest.mark.parametrize("algo", ["phj", "cpra", "npj"])
@pytest.mark.parametrize("flags", BOTH)
def test_async_forms_with_async_output_back_to_back(ctx, algo, flags):
    """two joins back to back on the stream without a host sync in between: the second join's bitmap clear is ordered behind the first
    join's tail; both results are right, and neither wrote the outer column"""
    ik, iv, ok, ov = relations(2_000_000, 4_000_001, 0.5, seed=81)
    ik2, iv2, ok2, ov2 = relations(1_500_000, 3_000_001, 0.5, seed=82, present=0.25)
    aggs = [want(ik, iv, ok, flags), want(ik2, iv2, ok2, flags)]
    sets = [cols(ctx, ik, iv, ok, ov), cols(ctx, ik2, iv2, ok2, ov2)]
    sizes = [(len(ik), len(ok)), (len(ik2), len(ok2))]
    outs, d_res = [], []
    for (agg, _), (ni, no) in zip(aggs, sizes):
        cap = ctx.output_capacity(ALGO_ID[algo], no, agg[0], 4096)
        outs.append((ctx.column(np.zeros(cap, np.uint32)), ctx.column(np.full(cap, UNTOUCHED, np.uint32)), ctx.column(np.zeros(cap, np.uint32)), cap, 4096))
        d_res.append(ctx.column(4, np.uint64))
    for j in range(2):
        rk, rv, sk, sv = sets[j]
        ctx.set_async_output(outs[j])
        getattr(ctx, algo + "_async")(rk, rv, sizes[j][0], sk, sv, sizes[j][1], _params(algo, None, flags), d_res[j])
    ctx.get_async_status()
    for j in range(2):
        agg, wanted = aggs[j]
        assert tuple(int(x) for x in d_res[j].download()) == agg, j
        k, i = outs[j][0].download(agg[0]), outs[j][2].download(agg[0])
        idx = np.lexsort((i, k))
        assert all(np.array_equal(g, w) for g, w in zip((k[idx], i[idx]), wanted)), j
        assert np.all(outs[j][1].download() == UNTOUCHED), j


@pytest.mark.parametrize("flags", BOTH)
def test_overlapped_async(ctx, flags):
    ik, iv, ok, ov = relations(1_000_000, 3_000_001, 0.5, seed=83)
    agg, wanted = want(ik, iv, ok, flags)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d_res = ctx.column(4, np.uint64)
    cap = ctx.output_capacity(1, len(ok), agg[0], 4096)
    dk, do, di = ctx.column(np.zeros(cap, np.uint32)), ctx.column(np.full(cap, UNTOUCHED, np.uint32)), ctx.column(np.zeros(cap, np.uint32))
    prm = PhjParams(); prm.flags = flags
    ctx.set_async_output((dk, do, di, cap, 4096))
    ctx.phj_overlapped_async(rk, rv, len(ik), sk, sv, len(ok), prm, d_res, None, None)
    ctx.get_async_status()
    assert tuple(int(x) for x in d_res.download()) == agg
    k, i = dk.download(agg[0]), di.download(agg[0])
    idx = np.lexsort((i, k))
    assert all(np.array_equal(g, w) for g, w in zip((k[idx], i[idx]), wanted))
    assert np.all(do.download() == UNTOUCHED)


@pytest.mark.parametrize("algo", SOME)
@pytest.mark.parametrize("flags", BOTH)
def test_unique_beside_the_flags_changes_nothing(ctx, algo, flags):
    """HJGPU_FLAG_UNIQUE and option "unique" are ignored: no row depends on which copy of a build key a walk finds"""
    ik, iv, ok, ov = relations(300_000, 700_001, 0.6, seed=85, distinct=40_000)
    ik[:20_000] = ik[0]                                  # a multi-fill partition among them
    ok[::5000] = ik[0]
    agg, wanted = want(ik, iv, ok, flags)
    res, got = run(ctx, _algo(algo), ik, iv, ok, ov, flags | H.FLAG_UNIQUE, prm=_prm(algo))
    assert res == agg and all(np.array_equal(g, w) for g, w in zip(got, wanted))
    ctx.set_option("unique", 1)
    res, got = run(ctx, _algo(algo), ik, iv, ok, ov, flags, prm=_prm(algo))
    assert res == agg and all(np.array_equal(g, w) for g, w in zip(got, wanted))


@pytest.mark.parametrize("algo", ["phj", "npj"])
def test_right_anti_is_the_null_rows_of_the_right_outer_join(ctx, algo):
    """identity against shipped code: the rows of RIGHT_ANTI are the NULL rows of HJGPU_FLAG_RIGHT_OUTER, RIGHT_SEMI the build tuples beside them"""
    ik, iv, ok, ov = relations(400_000, 900_001, 0.5, seed=84, distinct=250_000, payload_max=2**32 - 1)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    n = len(ok) * 4 + len(ik)
    cap = ctx.output_capacity(ALGO_ID[algo], len(ok), n, 0)
    dk, do, di = (ctx.column(np.zeros(cap, np.uint32)) for _ in range(3))
    fn = {"phj": ctx.phj, "npj": ctx.npj}[algo]
    res = fn(rk, rv, len(ik), sk, sv, len(ok), params=_params(algo, None, H.FLAG_RIGHT_OUTER), out=(dk, do, di, cap, 0))
    k, o, i = dk.download(res[0]), do.download(res[0]), di.download(res[0])
    null = o == np.uint32(H.NULL_VAL)
    b = np.sort((k[null].astype(np.uint64) << np.uint64(32)) | i[null].astype(np.uint64))
    _, (ak, ai) = run(ctx, algo, ik, iv, ok, ov, RANTI)
    assert np.array_equal(np.sort((ak.astype(np.uint64) << np.uint64(32)) | ai.astype(np.uint64)), b)
    res_s, _ = run(ctx, algo, ik, iv, ok, ov, RSEMI, rows=False)
    assert res_s[0] == len(ik) - int(null.sum())


def _einval_naming(fn, *names):
    with pytest.raises(HjGpuError) as e:
        fn()
    assert e.value.status == 1 and all(n in str(e.value) for n in names), str(e.value)


@pytest.mark.parametrize("flags", BOTH)
def test_out_of_scope_entry_points_refuse(ctx, flags):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=91)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    name = NAMES[flags]
    prm = PhjParams(); prm.flags = flags
    _einval_naming(lambda: ctx.phj_build(rk, rv, len(ik), len(ok), params=prm), name)
    roff = ctx.column(np.zeros(64, np.uint64), np.uint64)
    _einval_naming(lambda: ctx.join_partitions(rk, rv, roff, sk, sv, roff, prm), name)
    for algo in (0, 1, 2):
        np_prm = NpjParams(); np_prm.flags = flags
        _einval_naming(lambda: ctx.join_host(algo, ik, iv, ok, ov, phj_params=prm, npj_params=np_prm), name)
    _einval_naming(lambda: ctx.prepartitioned_plan(1_000_000, 16, prm), name)
    d_tuples = ctx.column(16, np.uint64)
    _einval_naming(lambda: ctx.phj_build_prepartitioned(d_tuples, H.api.PrePartitioned(), 1000, params=prm), name)
    comm = H.HjComm.local(2, [0, 0], H.TRANSPORT_LOOPBACK)
    try:
        shards = [(rk, rv, 500, sk, sv, 5000), (rk.ptr + 2000, rv.ptr + 2000, 500, sk.ptr + 20000, sv.ptr + 20000, 5000)]
        nprm = NpjParams(); nprm.flags = flags
        _einval_naming(lambda: comm.phj_multi(shards, params=prm), name)
        _einval_naming(lambda: comm.cpra_multi(shards, params=prm), name)
        _einval_naming(lambda: comm.npj_multi(shards, params=nprm), name)
    finally:
        comm.close()


OTHERS = [(H.FLAG_SEMI, "HJGPU_FLAG_SEMI"), (H.FLAG_ANTI, "HJGPU_FLAG_ANTI"), (H.FLAG_LEFT_OUTER, "HJGPU_FLAG_LEFT_OUTER"),
          (H.FLAG_RIGHT_OUTER, "HJGPU_FLAG_RIGHT_OUTER")]


@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("other,name", OTHERS)
def test_refused_combinations(ctx, flags, other, name):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=92)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.cpra, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = flags | other
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm), NAMES[flags], name)


def test_right_semi_with_right_anti_is_refused(ctx):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=92)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.cpra, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = RSEMI | RANTI
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm), NAMES[RSEMI], NAMES[RANTI])
    d = ctx.column(4, np.uint64)
    prm = PhjParams(); prm.flags = RSEMI | RANTI
    _einval_naming(lambda: ctx.phj_async(rk, rv, len(ik), sk, sv, len(ok), prm, d), NAMES[RSEMI], NAMES[RANTI])


@pytest.mark.parametrize("flags", BOTH)
def test_geometry_without_instances_refuses(ctx, flags):
    ctx.set_option("join_cfg", "256,12,2")
    for inner in (3_000_000, 1000):
        ik, iv, ok, ov = relations(inner, 100_000, 0.5, seed=94)
        rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
        prm = PhjParams(); prm.flags = flags
        _einval_naming(lambda: ctx.phj(rk, rv, len(ik), sk, sv, len(ok), params=prm), NAMES[flags])


@pytest.mark.parametrize("flags", BOTH)
def test_null_inner_payload_column_is_refused(ctx, flags):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=95)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    cap = ctx.output_capacity(1, len(ok), len(ik), 0)
    dk, dx = ctx.column(np.zeros(cap, np.uint32)), ctx.column(np.zeros(cap, np.uint32))
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.cpra, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = flags
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=(dk, dx, None, cap, 0)), NAMES[flags], "d_inner_vals")
