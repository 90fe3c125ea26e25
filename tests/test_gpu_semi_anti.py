"""GPU tests of semi- and anti-joins (HJGPU_FLAG_SEMI / HJGPU_FLAG_ANTI) through hjgpu_phj, hjgpu_cpra and hjgpu_npj, against their
definition on the host: a probe tuple is reported by SEMI when np.isin(key, build keys), by ANTI when not - aggregates and sorted
(key, outer_val) rows.  Out-of-scope entry points must refuse the flags instead of returning an inner join.

Every test takes a context of its own: options set here must not reach the session's other tests."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd.api import PhjParams, NpjParams, HjGpuError

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture
def ctx():
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    with H.HjGpu(0) as hj:
        yield hj


def want(ik, ok, ov, flag):
    hit = np.isin(ok, ik)
    sel = hit if flag == H.FLAG_SEMI else ~hit
    k, o = ok[sel], ov[sel]
    agg = (int(sel.sum()), int(k.astype(np.uint64).sum(dtype=np.uint64)) & M64, int(o.astype(np.uint64).sum(dtype=np.uint64)) & M64, 0)
    idx = np.lexsort((o, k))
    return agg, k[idx], o[idx]


def relations(inner, outer, sel, seed, distinct=None, extra_keys=()):
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, 2**32 - 1, size=2 * (distinct or inner) + 64, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    d = distinct or inner
    build_keys, miss = pool[:d], pool[d:]
    ik = build_keys[rng.integers(0, d, size=inner)] if distinct else build_keys[:inner].copy()
    iv = rng.integers(0, 2**32, size=inner, dtype=np.uint64).astype(np.uint32)
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


def run(hj, algo, ik, iv, ok, ov, flag, prm=None, rows=False, inner_pattern=False):
    rk, rv, sk, sv = cols(hj, ik, iv, ok, ov)
    if prm is None:
        prm = NpjParams() if algo == "npj" else PhjParams()
    prm.flags = flag | (prm.flags & H.FLAG_UNIQUE)
    fn = {"phj": hj.phj, "cpra": hj.cpra, "npj": hj.npj}[algo]
    out = None
    if rows:
        cap = hj.output_capacity({"npj": 0, "phj": 1, "cpra": 2}[algo], len(ok), len(ok), 0)
        dk, do = hj.column(np.zeros(cap, np.uint32)), hj.column(np.zeros(cap, np.uint32))
        di = None
        if inner_pattern:
            pat = (np.arange(cap, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
            di = hj.column(pat)
        out = (dk, do, di.ptr if di is not None else None, cap, 0)
    res = fn(rk, rv, len(ik), sk, sv, len(ok), params=prm, out=out)
    got_rows = None
    if rows:
        n = res[0]
        k, o = dk.download(n), do.download(n)
        idx = np.lexsort((o, k))
        got_rows = (k[idx], o[idx])
        if inner_pattern:
            assert np.array_equal(di.download(), pat), "the inner_val column was written"
    return res, got_rows


def check(hj, algo, ik, iv, ok, ov, prm_fn=lambda: None, rows=True):
    for flag in (H.FLAG_SEMI, H.FLAG_ANTI):
        agg, wk, wo = want(ik, ok, ov, flag)
        res, got = run(hj, algo, ik, iv, ok, ov, flag, prm_fn(), rows=rows)
        assert tuple(res) == agg, (algo, flag, res, agg)
        if rows:
            assert np.array_equal(got[0], wk) and np.array_equal(got[1], wo), (algo, flag)


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
    check(ctx, _algo(algo), ik, iv, ok, ov, lambda: _prm(algo))


@pytest.mark.parametrize("algo", ["phj", "cpra8"])
def test_key_zero_and_all_ones_on_both_sides(ctx, algo):
    ik, iv, ok, ov = relations(200_000, 700_001, 0.5, seed=11)
    ik[:2] = [0, 0xFFFFFFFF]
    ok[:6] = [0, 0xFFFFFFFF, 0, 1, 2, 0xFFFFFFFE]
    check(ctx, _algo(algo), ik, iv, ok, ov, lambda: _prm(algo))


def test_npj_probe_key_zero_is_reported_by_anti(ctx):
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
                                  {"batch_tuples": 1 << 20}, {"join_cfg": "1024,14,2"}, {"probe_slack": 0}, {"unique": 1}])
def test_plans(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ik, iv, ok, ov = relations(3_000_000, 6_000_001, 0.5, seed=21)
    check(ctx, "phj", ik, iv, ok, ov)


def test_one_pass_plan(ctx):
    ik, iv, ok, ov = relations(200_000, 2_000_001, 0.5, seed=22)
    check(ctx, "phj", ik, iv, ok, ov, lambda: PhjParams(fanout1=64, fanout2=1))


@pytest.mark.parametrize("group_device", [1, 0])
def test_grouped_plans_with_empty_groups(ctx, group_device):
    ctx.set_option("group_always", 1)
    ctx.set_option("group_from", 1000)
    ctx.set_option("group_inner", 100_000)
    ctx.set_option("group_device", group_device)
    ik, iv, ok, ov = relations(400_000, 2_000_001, 0.5, seed=31, distinct=3)
    check(ctx, "phj", ik, iv, ok, ov)
    ik, iv, ok, ov = relations(800_000, 2_000_001, 0.5, seed=32)
    check(ctx, "phj", ik, iv, ok, ov)


def test_few_distinct_build_keys_two_passes(ctx):
    ik, iv, ok, ov = relations(50_000, 1_000_001, 0.5, seed=41, distinct=5)
    check(ctx, "phj", ik, iv, ok, ov, lambda: PhjParams(fanout1=32, fanout2=16))
    check(ctx, "cpra", ik, iv, ok, ov, lambda: PhjParams(fanout1=32, fanout2=16, chunks=8))


@pytest.mark.parametrize("algo", ["phj", "cpra8", "npj"])
def test_heavy_build_key_multi_fill(ctx, algo):
    ik, iv, ok, ov = relations(150_000, 1_500_001, 0.5, seed=51)
    ik[:100_000] = ik[0]
    ok[::3] = ik[0]
    check(ctx, _algo(algo), ik, iv, ok, ov, lambda: _prm(algo))


@pytest.mark.parametrize("algo", ["phj", "cpra8", "npj"])
def test_empty_sides(ctx, algo):
    ik, iv, ok, ov = relations(1000, 300_001, 0.5, seed=61)
    e = np.zeros(0, np.uint32)
    check(ctx, _algo(algo), e, e, ok, ov, lambda: _prm(algo))
    check(ctx, _algo(algo), ik, iv, e, e, lambda: _prm(algo), rows=False)
    check(ctx, _algo(algo), e, e, ok, ov, lambda: PhjParams(fanout1=32, fanout2=16, chunks=8 if algo == "cpra8" else 0)
          if algo != "npj" else None)


@pytest.mark.parametrize("algo", ["phj", "npj"])
def test_inner_column_is_left_alone(ctx, algo):
    ik, iv, ok, ov = relations(300_000, 900_001, 0.5, seed=71)
    for flag in (H.FLAG_SEMI, H.FLAG_ANTI):
        agg, wk, wo = want(ik, ok, ov, flag)
        res, got = run(ctx, algo, ik, iv, ok, ov, flag, rows=True, inner_pattern=True)
        assert tuple(res) == agg
        assert np.array_equal(got[0], wk) and np.array_equal(got[1], wo)


def test_null_inner_column_is_refused_for_an_inner_join(ctx):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=72)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    cap = ctx.output_capacity(1, len(ok), len(ok), 0)
    dk, do = ctx.column(np.zeros(cap, np.uint32)), ctx.column(np.zeros(cap, np.uint32))
    with pytest.raises(HjGpuError) as e:
        ctx.phj(rk, rv, len(ik), sk, sv, len(ok), out=(dk, do, None, cap, 0))
    assert e.value.status == 1


@pytest.mark.parametrize("algo", ["phj", "cpra"])
def test_async_forms(ctx, algo):
    ik, iv, ok, ov = relations(2_000_000, 4_000_001, 0.5, seed=81)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d_res = ctx.column(4, np.uint64)
    for flag in (H.FLAG_SEMI, H.FLAG_ANTI):
        prm = PhjParams(); prm.flags = flag
        getattr(ctx, algo + "_async")(rk, rv, len(ik), sk, sv, len(ok), prm, d_res)
        ctx.get_async_status()
        agg, _, _ = want(ik, ok, ov, flag)
        assert tuple(int(x) for x in d_res.download()) == agg


def _einval_naming(fn, flagname):
    with pytest.raises(HjGpuError) as e:
        fn()
    assert e.value.status == 1 and flagname in str(e.value), str(e.value)


@pytest.mark.parametrize("flag,name", [(2, "HJGPU_FLAG_SEMI"), (4, "HJGPU_FLAG_ANTI")])
def test_out_of_scope_entry_points_refuse(ctx, flag, name):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=91)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    prm = PhjParams(); prm.flags = flag
    _einval_naming(lambda: ctx.phj_build(rk, rv, len(ik), len(ok), params=prm), name)
    roff = ctx.column(np.zeros(64, np.uint64), np.uint64)
    _einval_naming(lambda: ctx.join_partitions(rk, rv, roff, sk, sv, roff, prm), name)
    for algo in (0, 1, 2):
        np_prm = NpjParams(); np_prm.flags = flag
        _einval_naming(lambda: ctx.join_host(algo, ik, iv, ok, ov, phj_params=prm, npj_params=np_prm), name)


def test_semi_and_anti_together_is_refused(ctx):
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=92)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    for fn, prm in ((ctx.phj, PhjParams()), (ctx.cpra, PhjParams()), (ctx.npj, NpjParams())):
        prm.flags = H.FLAG_SEMI | H.FLAG_ANTI
        with pytest.raises(HjGpuError) as e:
            fn(rk, rv, len(ik), sk, sv, len(ok), params=prm)
        assert e.value.status == 1


def test_geometry_without_unique_instance_refuses(ctx):
    ctx.set_option("join_cfg", "256,12,2")
    ik, iv, ok, ov = relations(3_000_000, 100_000, 0.5, seed=93)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    for flag, name in ((H.FLAG_SEMI, "HJGPU_FLAG_SEMI"), (H.FLAG_ANTI, "HJGPU_FLAG_ANTI")):
        prm = PhjParams(); prm.flags = flag
        _einval_naming(lambda: ctx.phj(rk, rv, len(ik), sk, sv, len(ok), params=prm), name)


@pytest.mark.parametrize("blocking", [True, False])
def test_device_planned_groups_without_build_rows(ctx, blocking):
    """40 copies of ONE build key: a device-planned grouped plan of 40 groups in which 39 have probe rows and no build rows, and none
    exceeds its workspace (no skew: the device path itself answers, not the host-planned replay)"""
    for k, v in (("group_always", 1), ("group_from", 2), ("group_inner", 1), ("group_device", 1)):
        ctx.set_option(k, v)
    rng = np.random.default_rng(101)
    ik = np.full(40, 0x12345677, np.uint32)
    iv = np.arange(40, dtype=np.uint32)
    outer = 3_000_001
    ok = rng.integers(1, 2**32 - 1, size=outer, dtype=np.uint64).astype(np.uint32)
    ok[::200] = ik[0]
    ov = rng.integers(0, 2**32, size=outer, dtype=np.uint64).astype(np.uint32)
    if blocking:
        check(ctx, "phj", ik, iv, ok, ov)
        assert ctx.stats()["groups"] > 1
        return
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    d_res = ctx.column(4, np.uint64)
    for flag in (H.FLAG_SEMI, H.FLAG_ANTI):
        prm = PhjParams(); prm.flags = flag
        ctx.phj_async(rk, rv, len(ik), sk, sv, outer, prm, d_res)
        ctx.get_async_status()
        assert tuple(int(x) for x in d_res.download()) == want(ik, ok, ov, flag)[0]


def test_full_size_against_the_generator(ctx):
    """64 M x 1 G at selectivity 0.5 from hjgpu_generate_select: SEMI is the generator's expected aggregates (unique build keys: the inner
    join's count, sum_keys and sum_outer_vals), and SEMI + ANTI is all of S"""
    inner, outer = 64_000_000, 1_000_000_000
    fi, fo = 0x2545F491, 0x9E3779B1
    ik, iv, ok, ov = ctx.column(inner), ctx.column(inner), ctx.column(outer), ctx.column(outer)
    exp = ctx.generate_select(1, inner, outer, 0, inner, 0, outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov)
    sums = [0, 0, 0]
    for flag in (H.FLAG_SEMI, H.FLAG_ANTI):
        prm = PhjParams(); prm.flags = flag
        r = ctx.phj(ik, iv, inner, ok, ov, outer, params=prm)
        assert r[3] == 0
        if flag == H.FLAG_SEMI:
            assert r[:3] == exp[:3], (r, exp)
        sums = [(s + x) & M64 for s, x in zip(sums, r[:3])]
    # all of S: count, and the key / payload sums of the whole probe side (payload = key * fo mod 2^32)
    keys = ok.download()
    want_k = int(keys.astype(np.uint64).sum(dtype=np.uint64)) & M64
    want_o = int((keys * np.uint32(fo)).astype(np.uint64).sum(dtype=np.uint64)) & M64
    assert sums == [outer, want_k, want_o]


@pytest.mark.parametrize("flag,name", [(2, "HJGPU_FLAG_SEMI"), (4, "HJGPU_FLAG_ANTI")])
def test_prepartitioned_and_multi_entry_points_refuse(ctx, flag, name):
    prm = PhjParams(); prm.flags = flag
    _einval_naming(lambda: ctx.prepartitioned_plan(1_000_000, 16, prm), name)
    d_tuples = ctx.column(16, np.uint64)
    _einval_naming(lambda: ctx.phj_build_prepartitioned(d_tuples, H.api.PrePartitioned(), 1000, params=prm), name)
    ik, iv, ok, ov = relations(1000, 10_000, 0.5, seed=94)
    rk, rv, sk, sv = cols(ctx, ik, iv, ok, ov)
    comm = H.HjComm.local(2, [0, 0], H.TRANSPORT_LOOPBACK)
    try:
        shards = [(rk, rv, 500, sk, sv, 5000), (rk.ptr + 2000, rv.ptr + 2000, 500, sk.ptr + 20000, sv.ptr + 20000, 5000)]
        nprm = NpjParams(); nprm.flags = flag
        _einval_naming(lambda: comm.phj_multi(shards, params=prm), name)
        _einval_naming(lambda: comm.cpra_multi(shards, params=prm), name)
        _einval_naming(lambda: comm.npj_multi(shards, params=nprm), name)
    finally:
        comm.close()
