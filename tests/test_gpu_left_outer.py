"""GPU tests of left outer joins (HJGPU_FLAG_LEFT_OUTER) through hjgpu_phj, hjgpu_cpra and hjgpu_npj, against their definition on the
host: every inner-join row (the build side sorted by key, each probe key's match range from np.searchsorted, the rows from np.repeat),
plus one row (key, outer_val, NULL_VAL) for every probe tuple whose key is not among the build keys (~np.isin).  Aggregates exactly,
rows after a lexsort.  With HJGPU_FLAG_UNIQUE a probe tuple has exactly one row: its first match or its NULL row.  Out-of-scope entry
points and flag combinations must refuse the flag instead of returning an inner join.

Every test takes a context of its own: options set here must not reach the session's other tests."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd.api import PhjParams, NpjParams, HjGpuError

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NULL = np.uint32(H.NULL_VAL)


@pytest.fixture
def ctx():
    """a context whose device columns are all freed when the test ends (a DeviceColumn is freed only by free(), and the result
    columns here are gigabytes: kept, they would exhaust the device over the module)"""
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


def want(ik, iv, ok, ov):
    """(aggregates, sorted rows) of S LEFT JOIN R: every match, then one NULL row per probe tuple without one"""
    order = np.argsort(ik, kind="stable")
    bk, bv = ik[order], iv[order]
    lo, hi = np.searchsorted(bk, ok, "left"), np.searchsorted(bk, ok, "right")
    cnt = (hi - lo).astype(np.int64)
    probe = np.repeat(np.arange(len(ok)), cnt)
    first = np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    null = ~np.isin(ok, ik)
    k = np.concatenate([ok[probe], ok[null]])
    o = np.concatenate([ov[probe], ov[null]])
    i = np.concatenate([bv[first], np.full(int(null.sum()), NULL, np.uint32)])
    agg = (len(k), _sum(k), _sum(o), _sum(bv[first]))
    idx = np.lexsort((i, o, k))
    return agg, (k[idx], o[idx], i[idx])


def relations(inner, outer, sel, seed, distinct=None, extra_keys=()):
    """unique (or `distinct` repeated) build keys, a `sel` share of probe tuples with a match; payloads never equal NULL_VAL, so that a
    row's NULL is unambiguous"""
    rng = np.random.default_rng(seed)
    d = distinct or inner
    pool = np.unique(rng.integers(1, 2**32 - 1, size=2 * d + 64, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    build_keys, miss = pool[:d], pool[d:]
    ik = build_keys[rng.integers(0, d, size=inner)] if distinct else build_keys[:inner].copy()
    iv = rng.integers(0, 2**32 - 1, size=inner, dtype=np.uint64).astype(np.uint32)
    hit = rng.random(outer) < sel
    ok = np.where(hit, build_keys[rng.integers(0, max(d, 1), size=outer) % max(d, 1)] if d else 0,
                  miss[rng.integers(0, len(miss), size=outer)]).astype(np.uint32)
    for i, k in enumerate(extra_keys):
        if outer > i:
            ok[(i * 7919) % outer] = k
    ov = rng.integers(0, 2**32, size=outer, dtype=np.uint64).astype(np.uint32)
    return ik, iv, ok, ov


def cols(hj, *arrays):
    return [hj.column(a) if len(a) else hj.column(np.zeros(4, np.uint32)) for a in arrays]


def _params(algo, prm, flags):
    if prm is None:
        prm = NpjParams() if algo == "npj" else PhjParams()
    prm.flags = flags
    return prm


def run(hj, algo, ik, iv, ok, ov, unique=False, prm=None, rows=True, capacity_rows=None):
    rk, rv, sk, sv = cols(hj, ik, iv, ok, ov)
    prm = _params(algo, prm, H.FLAG_LEFT_OUTER | (H.FLAG_UNIQUE if unique else 0))
    fn = {"phj": hj.phj, "cpra": hj.cpra, "npj": hj.npj}[algo]
    out = None
    if rows:
        n = capacity_rows if capacity_rows is not None else len(ok) + len(ok)
        cap = hj.output_capacity({"npj": 0, "phj": 1, "cpra": 2}[algo], len(ok), n, 0)
        dk, do, di = (hj.column(np.zeros(cap, np.uint32)) for _ in range(3))
        out = (dk, do, di, cap, 0)
    res = fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=out)
    got = None
    if rows:
        n = res[0]
        k, o, i = dk.download(n), do.download(n), di.download(n)
        idx = np.lexsort((i, o, k))
        got = (k[idx], o[idx], i[idx])
        for c in (dk, do, di):
            c.free()
    for c in (rk, rv, sk, sv):
        c.free()
    return tuple(res), got


def check_rows(got, wanted, what):
    assert all(np.array_equal(g, w) for g, w in zip(got, wanted)), what


def check_unique(ik, iv, ok, ov, res, got, what):
    """HJGPU_FLAG_UNIQUE: one row per probe tuple; the NULL rows are exactly the probe tuples without a match; a matched row's inner
    value is one of its key's build payloads"""
    assert res[:3] == (len(ok), _sum(ok), _sum(ov)), (what, res)
    k, o, i = got
    assert len(k) == len(ok)
    idx = np.lexsort((ov, ok))
    assert np.array_equal(k, ok[idx]) and np.array_equal(o, ov[idx]), what
    null = i == NULL
    assert np.array_equal(np.sort(k[null]), np.sort(ok[~np.isin(ok, ik)])), what
    pairs = (ik.astype(np.uint64) << np.uint64(32)) | iv.astype(np.uint64)
    got_pairs = (k[~null].astype(np.uint64) << np.uint64(32)) | i[~null].astype(np.uint64)
    assert np.isin(got_pairs, pairs).all(), what
    assert res[3] == _sum(i[~null]), (what, res)


def check(hj, algo, ik, iv, ok, ov, prm_fn=lambda: None, rows=True, unique_build=True, capacity_rows=None):
    """the left outer join, without and with HJGPU_FLAG_UNIQUE (with unique build keys both are the oracle's join)"""
    agg, wanted = want(ik, iv, ok, ov)
    res, got = run(hj, algo, ik, iv, ok, ov, prm=prm_fn(), rows=rows, capacity_rows=capacity_rows)
    assert res == agg, (algo, res, agg)
    if rows:
        check_rows(got, wanted, algo)
    res, got = run(hj, algo, ik, iv, ok, ov, unique=True, prm=prm_fn(), rows=rows)
    if unique_build:
        assert res == agg, (algo, "unique", res, agg)
        if rows:
            check_rows(got, wanted, (algo, "unique"))
    else:
        check_unique(ik, iv, ok, ov, res, got, (algo, "unique"))


ALGOS = [("phj", {}), ("cpra8", {}), ("cpra64", {}), ("npj", {}), ("npj", {"npj_refhash": 1})]


def _prm(algo):
    if algo.startswith("cpra"):
        p = PhjParams(); p.chunks = int(algo[4:]); return p
    return None


def _algo(algo):
    return "cpra" if algo.startswith("cpra") else algo


@pytest.mark.parametrize("algo,opts", ALGOS)
@pytest.mark.parametrize("sel", [0.0, 0.5, 1.0])
def test_aggregates_and_rows(ctx, algo, opts, sel):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(300_000, 1_000_003, sel, seed=int(sel * 10) + 3, extra_keys=(0, 0xFFFFFFFF))
    if algo != "npj":
        ik[:2] = [0, 0xFFFFFFFF]                      # every key value is legal on both sides of PHJ / CPRA
    check(ctx, _algo(algo), ik, iv, ok, ov, lambda: _prm(algo))


def test_npj_probe_key_zero_gets_a_null_row(ctx):
    ik, iv, ok, ov = relations(100_000, 400_003, 0.5, seed=12)
    ok[:5] = 0
    check(ctx, "npj", ik, iv, ok, ov)


@pytest.mark.parametrize("inner", [1, 1000, 6963, 12000])
def test_broadcast_with_the_sentinel_in_the_probe_side(ctx, inner):
    ik, iv, ok, ov = relations(inner, 500_001, 0.5, seed=inner)
    # the sentinel is the first low-14-bit residue no build key has: put every small value in the probe side
    ok[:16384] = np.arange(16384, dtype=np.uint32)
    check(ctx, "phj", ik, iv, ok, ov)


@pytest.mark.parametrize("opts", [{"no_broadcast": 1}, {"exact_probe_counts": 1}, {"force_chained": 1}, {"dense2": 1},
                                  {"batch_tuples": 1 << 20}, {"join_cfg": "1024,14,2"}, {"unique": 1}, {"solo": 1}])
def test_plans(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(3_000_000, 6_000_001, 0.5, seed=21)
    check(ctx, "phj", ik, iv, ok, ov)


def test_one_pass_plan(ctx):
    ik, iv, ok, ov = relations(200_000, 2_000_001, 0.5, seed=22)
    check(ctx, "phj", ik, iv, ok, ov, lambda: PhjParams(fanout1=64, fanout2=1))


def test_claimed_probe_side_falls_back_to_the_exact_path(ctx):
    """a claimed probe side without slack (option probe_slack=0) overflows its regions: the join is done again exactly - right rows,
    the fallback counted"""
    ctx.set_option("probe_slack", 0)
    ik, iv, ok, ov = relations(3_000_000, 6_000_001, 0.5, seed=23)
    agg, wanted = want(ik, iv, ok, ov)
    res, got = run(ctx, "phj", ik, iv, ok, ov)
    assert res == agg
    check_rows(got, wanted, "fallback")
    assert ctx.counter("probe_fallbacks") == 1


def test_solo_does_not_change_the_result(ctx):
    ik, iv, ok, ov = relations(400_000, 2_000_001, 0.5, seed=24)
    agg, wanted = want(ik, iv, ok, ov)
    plain = run(ctx, "phj", ik, iv, ok, ov)
    ctx.set_option("solo", 1)
    solo = run(ctx, "phj", ik, iv, ok, ov)
    assert plain[0] == agg and solo[0] == agg
    check_rows(plain[1], wanted, "not solo")
    check_rows(solo[1], wanted, "solo")


@pytest.mark.parametrize("group_device", [1, 0])
def test_grouped_plans_with_empty_groups(ctx, group_device):
    ctx.set_option("group_always", 1)
    ctx.set_option("group_from", 1000)
    ctx.set_option("group_inner", 100_000)
    ctx.set_option("group_device", group_device)
    # 3 distinct build keys of ~133 000 copies each: 21 probe tuples match (2.8 M rows), the others get NULL rows
    ik, iv, ok, ov = relations(400_000, 2_000_001, 0.0, seed=31, distinct=3)
    ok[::100_000] = ik[0]
    check(ctx, "phj", ik, iv, ok, ov, unique_build=False, capacity_rows=len(ok) + 21 * 140_000)
    ik, iv, ok, ov = relations(800_000, 2_000_001, 0.5, seed=32)
    check(ctx, "phj", ik, iv, ok, ov)


def test_few_distinct_build_keys_two_passes(ctx):
    ik, iv, ok, ov = relations(50_000, 2_001, 0.5, seed=41, distinct=5)
    cap = len(ok) + len(ok) * 12_000
    check(ctx, "phj", ik, iv, ok, ov, lambda: PhjParams(fanout1=32, fanout2=16), unique_build=False, capacity_rows=cap)
    check(ctx, "cpra", ik, iv, ok, ov, lambda: PhjParams(fanout1=32, fanout2=16, chunks=8), unique_build=False, capacity_rows=cap)


@pytest.mark.parametrize("algo", ["phj", "cpra8", "npj"])
def test_heavy_build_key_multi_fill(ctx, algo):
    """20 000 copies of one build key: its partition takes several table fills (the multi-fill launch, its marks and its tail pass)"""
    ik, iv, ok, ov = relations(150_000, 600_001, 0.5, seed=51)
    ik[:20_000] = ik[0]
    ok[::3000] = ik[0]
    check(ctx, _algo(algo), ik, iv, ok, ov, lambda: _prm(algo), unique_build=False, capacity_rows=len(ok) + 201 * 20_000)


@pytest.mark.parametrize("algo", ["phj", "cpra8", "npj"])
def test_empty_sides(ctx, algo):
    ik, iv, ok, ov = relations(1000, 300_001, 0.5, seed=61)
    e = np.zeros(0, np.uint32)
    check(ctx, _algo(algo), e, e, ok, ov, lambda: _prm(algo))
    check(ctx, _algo(algo), ik, iv, e, e, lambda: _prm(algo), rows=False)
    check(ctx, _algo(algo), e, e, ok, ov, lambda: PhjParams(fanout1=32, fanout2=16, chunks=8 if algo == "cpra8" else 0)
          if algo != "npj" else None)


def test_null_inner_column_is_refused(ctx):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=72)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    cap = ctx.output_capacity(1, len(ok), 2 * len(ok), 0)
    dk, do = ctx.column(np.zeros(cap, np.uint32)), ctx.column(np.zeros(cap, np.uint32))
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = H.FLAG_LEFT_OUTER
        with pytest.raises(HjGpuError) as e:
            fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=(dk, do, None, cap, 0))
        assert e.value.status == 1


@pytest.mark.parametrize("algo", ["phj", "cpra", "npj"])
@pytest.mark.parametrize("unique", [False, True])
def test_async_forms_with_async_output(ctx, algo, unique):
    ik, iv, ok, ov = relations(2_000_000, 4_000_001, 0.5, seed=81)
    agg, wanted = want(ik, iv, ok, ov)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d_res = ctx.column(4, np.uint64)
    # (blocks of 4096 rows: NPJ's thousands of worker slots would hold 65536 each)
    cap = ctx.output_capacity({"npj": 0, "phj": 1, "cpra": 2}[algo], len(ok), 2 * len(ok), 4096)
    dk, do, di = (ctx.column(np.zeros(cap, np.uint32)) for _ in range(3))
    prm = _params(algo, None, H.FLAG_LEFT_OUTER | (H.FLAG_UNIQUE if unique else 0))
    ctx.set_async_output((dk, do, di, cap, 4096))
    getattr(ctx, algo + "_async")(rk, rv, len(ik), sk, sv, len(ok), prm, d_res)
    ctx.get_async_status()
    assert tuple(int(x) for x in d_res.download()) == agg
    n = agg[0]
    k, o, i = dk.download(n), do.download(n), di.download(n)
    idx = np.lexsort((i, o, k))
    check_rows((k[idx], o[idx], i[idx]), wanted, (algo, unique))


def test_overlapped_async(ctx):
    """hjgpu_phj_overlapped_async (a multi-GPU call's local join, always device-planned when grouped), with rows"""
    ik, iv, ok, ov = relations(1_000_000, 3_000_001, 0.5, seed=82)
    agg, wanted = want(ik, iv, ok, ov)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d_res = ctx.column(4, np.uint64)
    cap = ctx.output_capacity(1, len(ok), 2 * len(ok), 4096)
    dk, do, di = (ctx.column(np.zeros(cap, np.uint32)) for _ in range(3))
    prm = PhjParams(); prm.flags = H.FLAG_LEFT_OUTER
    ctx.set_async_output((dk, do, di, cap, 4096))
    ctx.phj_overlapped_async(rk, rv, len(ik), sk, sv, len(ok), prm, d_res, None, None)
    ctx.get_async_status()
    assert tuple(int(x) for x in d_res.download()) == agg
    n = agg[0]
    k, o, i = dk.download(n), do.download(n), di.download(n)
    idx = np.lexsort((i, o, k))
    check_rows((k[idx], o[idx], i[idx]), wanted, "overlapped")


@pytest.mark.parametrize("blocking", [True, False])
def test_device_planned_groups_without_build_rows(ctx, blocking):
    """40 copies of ONE build key: a device-planned grouped plan of 40 groups in which 39 have probe rows and no build rows"""
    for k, v in (("group_always", 1), ("group_from", 2), ("group_inner", 1), ("group_device", 1)):
        ctx.set_option(k, v)
    rng = np.random.default_rng(101)
    ik = np.full(40, 0x12345677, np.uint32)
    iv = np.arange(40, dtype=np.uint32)
    outer = 3_000_001
    ok = rng.integers(1, 2**32 - 1, size=outer, dtype=np.uint64).astype(np.uint32)
    ok[::200] = ik[0]
    ov = rng.integers(0, 2**32, size=outer, dtype=np.uint64).astype(np.uint32)
    agg, _ = want(ik, iv, ok, ov)
    if blocking:
        check(ctx, "phj", ik, iv, ok, ov, unique_build=False, capacity_rows=outer + 40 * 15_001)
        assert ctx.stats()["groups"] > 1
        return
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d_res = ctx.column(4, np.uint64)
    prm = PhjParams(); prm.flags = H.FLAG_LEFT_OUTER
    ctx.phj_async(rk, rv, len(ik), sk, sv, outer, prm, d_res)
    ctx.get_async_status()
    assert tuple(int(x) for x in d_res.download()) == agg


def _einval_naming(fn, flagname):
    with pytest.raises(HjGpuError) as e:
        fn()
    assert e.value.status == 1 and flagname in str(e.value), str(e.value)


def test_out_of_scope_entry_points_refuse(ctx):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=91)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    name = "HJGPU_FLAG_LEFT_OUTER"
    prm = PhjParams(); prm.flags = H.FLAG_LEFT_OUTER
    _einval_naming(lambda: ctx.phj_build(rk, rv, len(ik), len(ok), params=prm), name)
    roff = ctx.column(np.zeros(64, np.uint64), np.uint64)
    _einval_naming(lambda: ctx.join_partitions(rk, rv, roff, sk, sv, roff, prm), name)
    for algo in (0, 1, 2):
        np_prm = NpjParams(); np_prm.flags = H.FLAG_LEFT_OUTER
        _einval_naming(lambda: ctx.join_host(algo, ik, iv, ok, ov, phj_params=prm, npj_params=np_prm), name)
    _einval_naming(lambda: ctx.prepartitioned_plan(1_000_000, 16, prm), name)
    d_tuples = ctx.column(16, np.uint64)
    _einval_naming(lambda: ctx.phj_build_prepartitioned(d_tuples, H.api.PrePartitioned(), 1000, params=prm), name)
    comm = H.HjComm.local(2, [0, 0], H.TRANSPORT_LOOPBACK)
    try:
        shards = [(rk, rv, 500, sk, sv, 5000), (rk.ptr + 2000, rv.ptr + 2000, 500, sk.ptr + 20000, sv.ptr + 20000, 5000)]
        nprm = NpjParams(); nprm.flags = H.FLAG_LEFT_OUTER
        _einval_naming(lambda: comm.phj_multi(shards, params=prm), name)
        _einval_naming(lambda: comm.cpra_multi(shards, params=prm), name)
        _einval_naming(lambda: comm.npj_multi(shards, params=nprm), name)
    finally:
        comm.close()


@pytest.mark.parametrize("other,name", [(H.FLAG_SEMI, "HJGPU_FLAG_SEMI"), (H.FLAG_ANTI, "HJGPU_FLAG_ANTI")])
def test_left_outer_with_semi_or_anti_is_refused(ctx, other, name):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=92)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.cpra, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = H.FLAG_LEFT_OUTER | other
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm), name)


def test_geometry_without_unique_instance_refuses(ctx):
    ctx.set_option("join_cfg", "256,12,2")
    for inner in (3_000_000, 1000):                   # the partitioned plan and the broadcast join
        ik, iv, ok, ov = relations(inner, 100_000, 0.5, seed=93)
        rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
        prm = PhjParams(); prm.flags = H.FLAG_LEFT_OUTER
        _einval_naming(lambda: ctx.phj(rk, rv, len(ik), sk, sv, len(ok), params=prm), "HJGPU_FLAG_LEFT_OUTER")


def test_full_size_against_the_generator(ctx):
    """64 M x 1 G at selectivity 0.5 from hjgpu_generate_select (unique build keys): one row per probe tuple - count |S|, the probe
    columns' sums - and sum_inner_vals the inner join's, with and without HJGPU_FLAG_UNIQUE"""
    inner, outer = 64_000_000, 1_000_000_000
    fi, fo = 0x2545F491, 0x9E3779B1
    ik, iv, ok, ov = ctx.column(inner), ctx.column(inner), ctx.column(outer), ctx.column(outer)
    exp = ctx.generate_select(1, inner, outer, 0, inner, 0, outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov)
    # the probe columns' sums: keys, and payloads (key * fo mod 2^32)
    sums = ctx.column_sums(ok, outer, fo, fi)
    for flags in (H.FLAG_LEFT_OUTER, H.FLAG_LEFT_OUTER | H.FLAG_UNIQUE):
        prm = PhjParams(); prm.flags = flags
        r = ctx.phj(ik, iv, inner, ok, ov, outer, params=prm)
        assert tuple(r) == (outer, sums[0], sums[1], exp[3]), (flags, r, exp, sums)
