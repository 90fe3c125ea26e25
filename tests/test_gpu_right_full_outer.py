"""GPU tests of right and full outer joins (HJGPU_FLAG_RIGHT_OUTER / _FULL_OUTER) through hjgpu_phj, hjgpu_cpra and hjgpu_npj, against
their definition on the host: every inner-join row (as in test_gpu_left_outer.want), plus one row (key, NULL_VAL, inner_val) for every
build tuple whose key is not among the probe keys (ik[~np.isin(ik, ok)]: duplicates one by one), plus - full outer - one row
(key, outer_val, NULL_VAL) for every probe tuple whose key is not among the build keys.  Exact equality: aggregates, and rows after a
lexsort.  Payloads are drawn below 0xFFFFFFFF on both sides, so a NULL is unambiguous.  Out-of-scope entry points and flag combinations
must refuse the flags instead of returning an inner join (bit 16 used to be ignored).

Every test takes a context of its own: options set here must not reach the session's other tests."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd.api import PhjParams, NpjParams, HjGpuError

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NULL = np.uint32(H.NULL_VAL)
RIGHT, FULL = H.FLAG_RIGHT_OUTER, H.FLAG_FULL_OUTER
NAMES = {RIGHT: "HJGPU_FLAG_RIGHT_OUTER", FULL: "HJGPU_FLAG_FULL_OUTER"}
BOTH = [RIGHT, FULL]


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


def want(ik, iv, ok, ov, flags):
    """(aggregates, sorted rows) of S RIGHT / FULL JOIN R"""
    order = np.argsort(ik, kind="stable")
    bk, bv = ik[order], iv[order]
    lo, hi = np.searchsorted(bk, ok, "left"), np.searchsorted(bk, ok, "right")
    cnt = (hi - lo).astype(np.int64)
    probe = np.repeat(np.arange(len(ok)), cnt)
    first = np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    rnull = ~np.isin(ik, ok)
    lnull = ~np.isin(ok, ik) if flags == FULL else np.zeros(len(ok), bool)
    nr, nl = int(rnull.sum()), int(lnull.sum())
    k = np.concatenate([ok[probe], ik[rnull], ok[lnull]])
    o = np.concatenate([ov[probe], np.full(nr, NULL, np.uint32), ov[lnull]])
    i = np.concatenate([bv[first], iv[rnull], np.full(nl, NULL, np.uint32)])
    agg = (len(k), _sum(k), (_sum(ov[probe]) + _sum(ov[lnull])) & M64, (_sum(bv[first]) + _sum(iv[rnull])) & M64)
    idx = np.lexsort((i, o, k))
    return agg, (k[idx], o[idx], i[idx])


def relations(inner, outer, sel, seed, present=0.5, distinct=None):
    """`distinct` (default: inner, unique) build keys; a `sel` share of the probe tuples carries a build key, and those are drawn from the
    first `present` share of the distinct build keys only: the others have no match.  Payloads never equal NULL_VAL."""
    rng = np.random.default_rng(seed)
    d = distinct or inner
    pool = np.unique(rng.integers(1, 2**32 - 1, size=2 * d + 64, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    build_keys, miss = pool[:d], pool[d:]
    ik = build_keys[rng.integers(0, d, size=inner)] if distinct else build_keys[:inner].copy()
    iv = rng.integers(0, 2**32 - 1, size=inner, dtype=np.uint64).astype(np.uint32)
    dp = int(d * present)
    hit = (rng.random(outer) < sel) & (dp > 0)
    ok = np.where(hit, build_keys[rng.integers(0, max(dp, 1), size=outer)], miss[rng.integers(0, len(miss), size=outer)]).astype(np.uint32)
    ov = rng.integers(0, 2**32 - 1, size=outer, dtype=np.uint64).astype(np.uint32)
    return ik, iv, ok, ov


def cols(hj, *arrays):
    return [hj.column(a) if len(a) else hj.column(np.zeros(4, np.uint32)) for a in arrays]


def _params(algo, prm, flags):
    if prm is None:
        prm = NpjParams() if algo == "npj" else PhjParams()
    prm.flags = flags
    return prm


ALGO_ID = {"npj": 0, "phj": 1, "cpra": 2}


def run(hj, algo, ik, iv, ok, ov, flags, prm=None, rows=True, capacity=None, block=0):
    rk, rv, sk, sv = cols(hj, ik, iv, ok, ov)
    prm = _params(algo, prm, flags)
    fn = {"phj": hj.phj, "cpra": hj.cpra, "npj": hj.npj}[algo]
    out = None
    if rows:
        cap = capacity if capacity is not None else hj.output_capacity(ALGO_ID[algo], len(ok), want(ik, iv, ok, ov, flags)[0][0], block)
        dk, do, di = (hj.column(np.zeros(max(cap, 4), np.uint32)) for _ in range(3))
        out = (dk, do, di, cap, block)
    try:
        res = fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=out)
        got = None
        if rows:
            n = res[0]
            k, o, i = dk.download(n), do.download(n), di.download(n)
            idx = np.lexsort((i, o, k))
            got = (k[idx], o[idx], i[idx])
    finally:
        if rows:
            for c in (dk, do, di):
                c.free()
        for c in (rk, rv, sk, sv):
            c.free()
    return tuple(res), got


def check(hj, algo, ik, iv, ok, ov, flags=BOTH, prm_fn=lambda: None, rows=True):
    """aggregates and rows against the oracle; the aggregate-only call gives the same aggregates; the capacity is exactly
    hjgpu_output_capacity(true row count)"""
    for f in flags:
        agg, wanted = want(ik, iv, ok, ov, f)
        res, _ = run(hj, algo, ik, iv, ok, ov, f, prm=prm_fn(), rows=False)
        print(algo, NAMES[f], "aggregate-only", res, "want", agg)
        assert res == agg, (algo, NAMES[f], "aggregate-only", res, agg)
        if rows:
            res, got = run(hj, algo, ik, iv, ok, ov, f, prm=prm_fn())
            assert res == agg, (algo, NAMES[f], res, agg)
            assert all(np.array_equal(g, w) for g, w in zip(got, wanted)), (algo, NAMES[f])


ALGOS = [("phj", {}), ("cpra1", {}), ("cpra8", {}), ("cpra16", {}), ("npj", {}), ("npj", {"npj_refhash": 1})]


def _prm(algo):
    if algo.startswith("cpra"):
        p = PhjParams(); p.chunks = int(algo[4:]); return p
    return None


def _algo(algo):
    return "cpra" if algo.startswith("cpra") else algo


@pytest.mark.parametrize("algo,opts", ALGOS)
@pytest.mark.parametrize("sel,present", [(0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (0.5, 1.0), (1.0, 0.5), (1.0, 1.0)])
def test_aggregates_and_rows(ctx, algo, opts, sel, present):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(300_000, 1_000_003, sel, seed=int(sel * 10 + present * 100) + 3, present=present)
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
    ok[:4] = [0, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


def test_npj_probe_key_zero_matches_nothing(ctx):
    ik, iv, ok, ov = relations(100_000, 400_003, 0.5, seed=12)
    ok[:5] = 0
    check(ctx, "npj", ik, iv, ok, ov)


@pytest.mark.parametrize("algo", ["phj", "cpra8", "npj"])
def test_duplicated_build_keys_absent_from_the_probe_side(ctx, algo):
    """every copy of a build key without a probe tuple gets a NULL row of its own; the copies of a present key are all matched"""
    ik, iv, ok, ov = relations(200_000, 500_001, 0.7, seed=14, distinct=80_000)
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("opts", [{}, {"join_cfg": "1024,14,2"}])
def test_several_probe_slices_per_partition(ctx, opts):
    """about 6 partitions of about 10 slices: each of 1000 build keys occurs exactly once in the probe side, anywhere in the column - a
    bitmap that is not combined across the work items of a partition reports some of them as NULL"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(20_000, 4_000_003, 0.0, seed=15)
    rng = np.random.default_rng(16)
    at = rng.choice(len(ok), size=1000, replace=False)
    ok[at] = ik[rng.choice(len(ik), size=1000, replace=False)]
    check(ctx, "phj", ik, iv, ok, ov, prm_fn=lambda: PhjParams(fanout1=3, fanout2=2))
    # the plan that ran: few enough partitions that each one's probe rows are cut into several slices (work items) of 65 536 rows
    st = ctx.stats()
    parts = st["fanout1"] * st["fanout2"]
    assert parts == 6 and len(ok) / (parts * 65536) > 1, st


def test_partitions_with_build_rows_and_no_probe_rows(ctx):
    ik, iv, ok, ov = relations(3_000_000, 1000, 1.0, seed=17, present=1.0)
    check(ctx, "phj", ik, iv, ok, ov)
    check(ctx, "cpra", ik, iv, ok, ov, prm_fn=lambda: _prm("cpra8"))


@pytest.mark.parametrize("algo", ["phj", "cpra8", "npj"])
@pytest.mark.parametrize("in_probe", [True, False])
def test_heavy_build_key_multi_fill(ctx, algo, in_probe):
    """20 000 copies of one build key: its partition takes several table fills"""
    ik, iv, ok, ov = relations(150_000, 600_001, 0.5, seed=51)
    ik[:20_000] = ik[0]
    if in_probe:
        ok[::3000] = ik[0]
    else:
        ok[ok == ik[0]] = 1
    check(ctx, _algo(algo), ik, iv, ok, ov, prm_fn=lambda: _prm(algo))


def test_chained_fallback(ctx):
    ik, iv, ok, ov = relations(300_000, 1_000_003, 0.5, seed=52)
    ctx.set_option("force_chained", 1)
    check(ctx, "phj", ik, iv, ok, ov)
    ctx.set_option("force_chained", 0)
    # 3-5 copies of every build key: the cuckoo build gives up on its own
    rng = np.random.default_rng(53)
    keys = np.unique(rng.integers(1, 2**32 - 1, size=60_000, dtype=np.uint64).astype(np.uint32))
    ik = np.repeat(keys, rng.integers(3, 6, size=len(keys)))
    rng.shuffle(ik)
    iv = rng.integers(0, 2**32 - 1, size=len(ik), dtype=np.uint64).astype(np.uint32)
    ok = np.where(rng.random(400_001) < 0.5, keys[rng.integers(0, len(keys) // 2, size=400_001)],
                  rng.integers(1, 2**32 - 1, size=400_001, dtype=np.uint64).astype(np.uint32)).astype(np.uint32)
    ov = rng.integers(0, 2**32 - 1, size=len(ok), dtype=np.uint64).astype(np.uint32)
    check(ctx, "phj", ik, iv, ok, ov)
    check(ctx, "cpra", ik, iv, ok, ov, prm_fn=lambda: _prm("cpra8"))


@pytest.mark.parametrize("opts", [{"no_broadcast": 1}, {"exact_probe_counts": 1}, {"dense2": 1}, {"batch_tuples": 1 << 20}, {"solo": 1}])
def test_plans(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(3_000_000, 6_000_001, 0.5, seed=21)
    check(ctx, "phj", ik, iv, ok, ov)


def test_dense2_with_chunks(ctx):
    ctx.set_option("dense2", 1)
    ik, iv, ok, ov = relations(1_000_000, 3_000_001, 0.5, seed=25)
    check(ctx, "cpra", ik, iv, ok, ov, prm_fn=lambda: _prm("cpra8"))


def test_one_pass_plan(ctx):
    ik, iv, ok, ov = relations(200_000, 2_000_001, 0.5, seed=22)
    check(ctx, "phj", ik, iv, ok, ov, prm_fn=lambda: PhjParams(fanout1=64, fanout2=1))
    check(ctx, "cpra", ik, iv, ok, ov, prm_fn=lambda: PhjParams(fanout1=64, fanout2=1, chunks=8))


@pytest.mark.parametrize("inner", [1, 1000, 6963, 12000])
def test_broadcast_sized_build_sides(ctx, inner):
    ik, iv, ok, ov = relations(inner, 500_001, 0.5, seed=inner)
    ok[:16384] = np.arange(16384, dtype=np.uint32)
    check(ctx, "phj", ik, iv, ok, ov)


@pytest.mark.parametrize("flags", BOTH)
def test_claimed_probe_side_falls_back_to_the_exact_path(ctx, flags):
    """a claimed probe side without slack overflows its regions: the join is done again exactly - the bitmap zeroed again, right rows"""
    ctx.set_option("probe_slack", 0)
    ik, iv, ok, ov = relations(3_000_000, 6_000_001, 0.5, seed=23)
    agg, wanted = want(ik, iv, ok, ov, flags)
    res, got = run(ctx, "phj", ik, iv, ok, ov, flags)
    assert res == agg
    assert all(np.array_equal(g, w) for g, w in zip(got, wanted))
    assert ctx.counter("probe_fallbacks") == 1


@pytest.mark.parametrize("group_device", [1, 0])
def test_grouped_plans(ctx, group_device):
    for k, v in (("group_always", 1), ("group_from", 1000), ("group_inner", 100_000), ("group_device", group_device)):
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(800_000, 2_000_001, 0.5, seed=32)
    check(ctx, "phj", ik, iv, ok, ov)
    assert ctx.stats()["groups"] > 1


@pytest.mark.parametrize("group_device", [1, 0])
def test_grouped_plans_with_groups_without_probe_rows_and_without_build_rows(ctx, group_device):
    """many groups, few keys: 40 distinct build keys and 40 distinct probe keys of which 20 are build keys - most groups hold rows of one
    side only"""
    for k, v in (("group_always", 1), ("group_from", 2), ("group_inner", 1000), ("group_device", group_device)):
        ctx.set_option(k, v)
    rng = np.random.default_rng(101)
    keys = np.unique(rng.integers(1, 2**32 - 1, size=100, dtype=np.uint64).astype(np.uint32))[:60]
    ik = keys[rng.integers(0, 40, size=40_000)]
    iv = rng.integers(0, 2**32 - 1, size=len(ik), dtype=np.uint64).astype(np.uint32)
    ok = keys[rng.integers(20, 60, size=3001)]
    ov = rng.integers(0, 2**32 - 1, size=len(ok), dtype=np.uint64).astype(np.uint32)
    check(ctx, "phj", ik, iv, ok, ov)
    assert ctx.stats()["groups"] > 1


@pytest.mark.parametrize("algo", ["phj", "cpra8", "npj"])
def test_empty_sides(ctx, algo):
    ik, iv, ok, ov = relations(1000, 300_001, 0.5, seed=61)
    e = np.zeros(0, np.uint32)
    check(ctx, _algo(algo), e, e, ok, ov, prm_fn=lambda: _prm(algo))          # inner == 0: FULL is LEFT_OUTER, RIGHT has no rows
    check(ctx, _algo(algo), ik, iv, e, e, prm_fn=lambda: _prm(algo))          # outer == 0: every build tuple
    check(ctx, _algo(algo), e, e, e, e, prm_fn=lambda: _prm(algo), rows=False)
    ik, iv, _, _ = relations(3_000_000, 10, 0.5, seed=62)
    check(ctx, _algo(algo), ik, iv, e, e, prm_fn=lambda: _prm(algo))


@pytest.mark.parametrize("algo", ["phj", "npj"])
@pytest.mark.parametrize("flags", BOTH)
def test_one_block_too_few_overflows(ctx, algo, flags):
    ik, iv, ok, ov = relations(300_000, 1_000_003, 0.5, seed=71)
    n = want(ik, iv, ok, ov, flags)[0][0]
    bs = 4096
    cap = ctx.output_capacity(ALGO_ID[algo], len(ok), n, bs)
    res, got = run(ctx, algo, ik, iv, ok, ov, flags, capacity=cap, block=bs)
    assert res[0] == n
    # one block too few for the rows: whole blocks only, and the last row no longer has a slot
    short = (n // bs) * bs if n % bs else n - bs
    with pytest.raises(HjGpuError) as e:
        run(ctx, algo, ik, iv, ok, ov, flags, capacity=short, block=bs)
    assert e.value.status == 6                                                              # HJGPU_EOVERFLOW


@pytest.mark.parametrize("algo", ["phj", "cpra", "npj"])
@pytest.mark.parametrize("flags", BOTH)
def test_async_forms_with_async_output_back_to_back(ctx, algo, flags):
    """two joins back to back on the stream without a host sync in between: the second join's bitmap clear is ordered behind the first
    join's tail; both results are right"""
    ik, iv, ok, ov = relations(2_000_000, 4_000_001, 0.5, seed=81)
    ik2, iv2, ok2, ov2 = relations(1_500_000, 3_000_001, 0.5, seed=82, present=0.25)
    aggs = [want(ik, iv, ok, ov, flags), want(ik2, iv2, ok2, ov2, flags)]
    sets = [cols(ctx, ik, iv, ok, ov), cols(ctx, ik2, iv2, ok2, ov2)]
    sizes = [(len(ik), len(ok)), (len(ik2), len(ok2))]
    outs, d_res = [], []
    for (agg, _), (ni, no) in zip(aggs, sizes):
        cap = ctx.output_capacity(ALGO_ID[algo], no, agg[0], 4096)
        outs.append(tuple(ctx.column(np.zeros(cap, np.uint32)) for _ in range(3)) + (cap, 4096))
        d_res.append(ctx.column(4, np.uint64))
    for j in range(2):
        rk, rv, sk, sv = sets[j]
        ctx.set_async_output(outs[j])
        getattr(ctx, algo + "_async")(rk, rv, sizes[j][0], sk, sv, sizes[j][1], _params(algo, None, flags), d_res[j])
    ctx.get_async_status()
    for j in range(2):
        agg, wanted = aggs[j]
        assert tuple(int(x) for x in d_res[j].download()) == agg, j
        k, o, i = (outs[j][c].download(agg[0]) for c in range(3))
        idx = np.lexsort((i, o, k))
        assert all(np.array_equal(g, w) for g, w in zip((k[idx], o[idx], i[idx]), wanted)), j


@pytest.mark.parametrize("flags", BOTH)
def test_overlapped_async(ctx, flags):
    ik, iv, ok, ov = relations(1_000_000, 3_000_001, 0.5, seed=83)
    agg, wanted = want(ik, iv, ok, ov, flags)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d_res = ctx.column(4, np.uint64)
    cap = ctx.output_capacity(1, len(ok), agg[0], 4096)
    dk, do, di = (ctx.column(np.zeros(cap, np.uint32)) for _ in range(3))
    prm = PhjParams(); prm.flags = flags
    ctx.set_async_output((dk, do, di, cap, 4096))
    ctx.phj_overlapped_async(rk, rv, len(ik), sk, sv, len(ok), prm, d_res, None, None)
    ctx.get_async_status()
    assert tuple(int(x) for x in d_res.download()) == agg
    k, o, i = dk.download(agg[0]), do.download(agg[0]), di.download(agg[0])
    idx = np.lexsort((i, o, k))
    assert all(np.array_equal(g, w) for g, w in zip((k[idx], o[idx], i[idx]), wanted))


@pytest.mark.parametrize("algo", ["phj", "npj"])
def test_null_rows_are_the_anti_join_with_the_roles_swapped(ctx, algo):
    """identity against shipped code: the NULL rows of RIGHT_OUTER(R, S), as a multiset of (key, inner_val), are the rows of
    HJGPU_FLAG_ANTI with R as the probe side and S as the build side"""
    ik, iv, ok, ov = relations(400_000, 900_001, 0.5, seed=84, distinct=250_000)
    _, (k, o, i) = run(ctx, algo, ik, iv, ok, ov, RIGHT)
    null = o == NULL
    rk, rv, sk, sv = cols(ctx, ok, ov, ik, iv)                                 # build = S, probe = R
    prm = _params(algo, None, H.FLAG_ANTI)
    cap = ctx.output_capacity(ALGO_ID[algo], len(ik), len(ik), 0)
    dk, do = ctx.column(np.zeros(cap, np.uint32)), ctx.column(np.zeros(cap, np.uint32))
    res = {"phj": ctx.phj, "npj": ctx.npj}[algo](rk, rv, len(ok), sk, sv, len(ik), params=prm, out=(dk, do, None, cap, 0))
    ak, av = dk.download(res[0]), do.download(res[0])
    assert res[0] == int(null.sum())
    a = np.sort((ak.astype(np.uint64) << np.uint64(32)) | av.astype(np.uint64))
    b = np.sort((k[null].astype(np.uint64) << np.uint64(32)) | i[null].astype(np.uint64))
    assert np.array_equal(a, b)


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


@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("other,name", [(H.FLAG_SEMI, "HJGPU_FLAG_SEMI"), (H.FLAG_ANTI, "HJGPU_FLAG_ANTI"), (H.FLAG_UNIQUE, "HJGPU_FLAG_UNIQUE")])
def test_refused_combinations(ctx, flags, other, name):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=92)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.cpra, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = flags | other
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm), NAMES[flags], name)


@pytest.mark.parametrize("flags", BOTH)
def test_option_unique_is_refused(ctx, flags):
    ctx.set_option("unique", 1)
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=93)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.cpra, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = flags
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm), NAMES[flags], "unique")


@pytest.mark.parametrize("flags", BOTH)
def test_geometry_without_instances_refuses(ctx, flags):
    ctx.set_option("join_cfg", "256,12,2")
    for inner in (3_000_000, 1000):
        ik, iv, ok, ov = relations(inner, 100_000, 0.5, seed=94)
        rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
        prm = PhjParams(); prm.flags = flags
        _einval_naming(lambda: ctx.phj(rk, rv, len(ik), sk, sv, len(ok), params=prm), NAMES[flags])


@pytest.mark.parametrize("flags", BOTH)
def test_null_payload_columns_are_refused(ctx, flags):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=95)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    cap = ctx.output_capacity(1, len(ok), 2 * len(ok), 0)
    dk, dx = ctx.column(np.zeros(cap, np.uint32)), ctx.column(np.zeros(cap, np.uint32))
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = flags
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=(dk, dx, None, cap, 0)), NAMES[flags])
        _einval_naming(lambda: fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=(dk, None, dx, cap, 0)), NAMES[flags])


def test_full_size_against_the_generator(ctx):
    """64 M x 1 G at selectivity 0.5 from hjgpu_generate_select (unique build keys, every one of them in the probe side's matching half
    many times over): RIGHT_OUTER is the inner join plus the build tuples no probe tuple carries, FULL_OUTER has one row per probe tuple
    beside them.  The number of unmatched build tuples follows from two shipped joins: |R| minus the semi-join of R against S."""
    inner, outer = 64_000_000, 1_000_000_000
    fi, fo = 0x2545F491, 0x9E3779B1
    ik, iv, ok, ov = ctx.column(inner), ctx.column(inner), ctx.column(outer), ctx.column(outer)
    exp = ctx.generate_select(1, inner, outer, 0, inner, 0, outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov)
    prm = PhjParams(); prm.flags = H.FLAG_SEMI
    semi = ctx.phj(ok, ov, outer, ik, iv, inner, params=prm)             # build tuples (probe side here) with a match in S
    s_in = ctx.column_sums(ik, inner, fi, fo)                            # the build columns' sums: keys, payloads
    prm = PhjParams(); prm.flags = RIGHT
    r = ctx.phj(ik, iv, inner, ok, ov, outer, params=prm)
    un_n, un_k, un_v = inner - semi[0], (s_in[0] - semi[1]) & M64, (s_in[1] - semi[2]) & M64
    # (the generator at selectivity 0.5: the probe side draws from the build keys of ranks [inner / 2, inner) and beyond - half the build keys)
    assert un_n == inner - inner // 2, un_n
    want_r = (exp[0] + un_n, (exp[1] + un_k) & M64, exp[2], (exp[3] + un_v) & M64)
    print("RIGHT", tuple(r), "want", want_r)
    assert tuple(r) == want_r
    s_out = ctx.column_sums(ok, outer, fo, fi)
    prm = PhjParams(); prm.flags = FULL
    f = ctx.phj(ik, iv, inner, ok, ov, outer, params=prm)
    prm = PhjParams(); prm.flags = H.FLAG_LEFT_OUTER
    left = ctx.phj(ik, iv, inner, ok, ov, outer, params=prm)
    want_f = (left[0] + un_n, (left[1] + un_k) & M64, left[2], (left[3] + un_v) & M64)
    print("FULL", tuple(f), "want", want_f)
    assert tuple(left)[:3] == (outer, s_out[0], s_out[1])
    assert tuple(f) == want_f
