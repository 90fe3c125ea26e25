"""GPU tests of option "audit" (hjgpu_audit_read, hjgpu_audit_recheck) against the host model tests/audit_model.py, and - with the
audit tested - of every partitioning road of the PHJ enqueue path stage by stage: a record says what a call read and what its
pass 1 and pass 2 wrote, so two errors that cancel in a join's aggregates do not cancel here.  Everything is an exact integer.

Every test takes contexts of its own (one with the option, one without): an option never leaks into the session's context."""
import ctypes as C

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
import audit_model as M
from helpers import mulhi_hash, numpy_join
from test_gpu_prepartitioned import FACTOR1, received, send, send_counted

pytestmark = pytest.mark.gpu

FA, FB = 0x9E3779B1, 0x85EBCA6B
BUILD, PROBE = 5_003, 70_001            # one ragged K6 tile and four full ones with a tail (tiles of 16384 rows); 3 and 35 of 2048
SMALL_TILES = "256,2,0"                 # option scatter_cfg: K6 pass 1 in tiles of 2048 rows
OWN_LAST = [(192, 48, 24), (192, 0, 96), (192, 168, 24), (8, 3, 1), (6, 0, 6), (64, 10, 0)]      # test_own_partitions_last's


def plan(fanout2=4, **more):
    return H.PhjParams(fanout1=8, fanout2=fanout2, factor1=FA, factor2=FB, **more)


class Contexts:
    """a context with option "audit", one without, and the device columns of a test"""

    def __init__(self):
        self.audited, self.plain = H.HjGpu(), H.HjGpu()
        self.audited.set_option("audit", 1)
        self.columns = []

    def both(self):
        return (self.audited, self.plain)

    def set_option(self, name, value):
        for c in self.both():
            c.set_option(name, value)

    def col(self, host_or_n, dtype=np.uint32):
        if not isinstance(host_or_n, (int, np.integer)) and len(host_or_n) == 0:
            host_or_n = np.zeros(1, dtype)
        self.columns.append(self.plain.column(host_or_n, dtype))
        return self.columns[-1]

    def cols(self, *arrays):
        return [self.col(a) for a in arrays]

    def close(self):
        for c in self.columns:
            c.free()
        for c in self.both():
            c.close()


@pytest.fixture
def ctxs(hj):
    """(the session's context first: it initialises torch's HIP runtime before the library's)"""
    c = Contexts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def rel(oracle):
    """the relations of this module and their join by the independent definition, each made once: (ik, iv, ok, ov, want)"""
    made = {}

    def extremes():
        rng = np.random.default_rng(24)
        u = np.unique(rng.integers(1, 2**32 - 1, size=BUILD + 64, dtype=np.uint64).astype(np.uint32))
        rng.shuffle(u)
        ik = np.concatenate([np.array([0, 0xFFFFFFFF], np.uint32), u[:BUILD - 2]])
        rng.shuffle(ik)
        ok = ik[rng.integers(0, BUILD, size=PROBE)]
        ok[:300] = 0
        ok[300:600] = 0xFFFFFFFF
        return ik, np.full(BUILD, 0xFFFFFFFF, np.uint32), ok, np.full(PROBE, 0xFFFFFFFF, np.uint32)

    def get(name):
        if name not in made:
            if name == "unique":
                r = oracle.generate(PROBE, BUILD, seed=21)
            elif name == "dups":                                  # probe smaller than build, 14 copies per build key
                r = oracle.generate(BUILD, PROBE, seed=22)
            elif name == "half":
                r = oracle.generate(PROBE, BUILD, selectivity=0.5, seed=23)
            elif name == "extremes":
                r = extremes()
            elif name == "other":                                 # other data and other sizes than "unique"
                r = oracle.generate(60_013, 4_001, seed=25)
            else:                                                 # "build1", "build37": a build side of 1 / 37 rows
                ik, iv, ok, ov, _ = get("unique")
                n = int(name[len("build"):])
                r = (ik[:n].copy(), iv[:n].copy(), ok, ov)
            made[name] = tuple(r) + (numpy_join(*r),)
        return made[name]
    return get


def join_record(seq, kind, ik, iv, ok, ov, result, probe=(0, 1, 2), build=(3, 4, 5)):
    """the record of a join: the probe side's sums in the stages `probe`, the build side's in `build`, the result in 6"""
    stages = {6: result}
    if len(ok):
        stages.update({s: M.sums(ok, ov) for s in probe})
    if len(ik):
        stages.update({s: M.sums(ik, iv) for s in build})
    return M.record(seq, kind, len(ik), len(ok), stages)


def check_recheck(ctx, rec, stages):
    """hjgpu_audit_recheck after the call that left `rec`: one check per partition stage the call filled, the fresh kernel and the host
    both count what the record holds"""
    assert [s for s in (1, 2, 4, 5) if rec[s] != M.ZERO] == sorted(stages)
    checks = ctx.audit_recheck()
    assert sorted(s for s, _, _ in checks) == sorted(stages)
    for s, fresh, host in checks:
        assert fresh == host == rec[s], (s, fresh, host, rec[s])


def audited_join(ctxs, fn, r, prm, probe=(0, 1, 2), build=(3, 4, 5), fanouts=(8, 4)):
    """one blocking whole join on both contexts: the results, the whole record and the second look"""
    ik, iv, ok, ov, want = r
    rk, rv, sk, sv = ctxs.cols(ik, iv, ok, ov)
    a, p = ctxs.both()
    seq = a.audit_next_seq()
    got = getattr(a, fn)(rk, rv, len(ik), sk, sv, len(ok), prm)
    st = a.stats()
    assert a.audit_next_seq() == seq + 1
    rec = a.audit_read(seq)[0]
    assert (st["fanout1"], st["fanout2"]) == fanouts
    assert rec == join_record(seq, 0, ik, iv, ok, ov, want, probe, build)
    assert got == want
    assert getattr(p, fn)(rk, rv, len(ik), sk, sv, len(ok), prm) == want
    assert p.audit_next_seq() == 0
    check_recheck(a, rec, [s for s in probe if s and len(ok)] + [s for s in build if s != 3 and len(ik)])
    return st, p.stats()


# ---- 1. whole hjgpu_phj: both relations side by side (partition_merged) and one after the other (partition_in_turn / partition_plain) ----
@pytest.mark.parametrize("merged", [1, 0])
@pytest.mark.parametrize("name", ["unique", "dups", "half", "extremes", "build1", "build37"])
def test_whole_phj(ctxs, rel, name, merged):
    ctxs.set_option("merged_plan", merged)
    st, st_plain = audited_join(ctxs, "phj", rel(name), plan())
    assert st["batches"] == 0 and (st_plain["fanout1"], st_plain["fanout2"]) == (8, 4)


def test_overlapped_phj_with_an_event_that_has_fired(ctxs, rel):
    import torch
    ik, iv, ok, ov, want = rel("unique")
    rk, rv, sk, sv = ctxs.cols(ik, iv, ok, ov)
    d_res = ctxs.col(4, np.uint64)
    ready = torch.cuda.Event()
    ready.record()
    ready.synchronize()
    for c in ctxs.both():
        seq = c.audit_next_seq()
        c.phj_overlapped_async(rk, rv, len(ik), sk, sv, len(ok), plan(), d_res, None, ready.cuda_event)
        c.get_async_status()
        assert tuple(int(x) for x in d_res.download()) == want
        if c is ctxs.audited:
            rec = c.audit_read(seq)[0]
            assert rec == join_record(seq, 0, ik, iv, ok, ov, want)
            check_recheck(c, rec, [1, 2, 4, 5])
    assert ctxs.plain.audit_next_seq() == 0


# ---- 2. a single pass: no pass-1 stage, the final partitions are pass 1's ----
@pytest.mark.parametrize("name", ["unique", "dups", "extremes"])
def test_single_pass(ctxs, rel, name):
    audited_join(ctxs, "phj", rel(name), plan(fanout2=1), probe=(0, 2), build=(3, 5), fanouts=(8, 1))


# ---- 3. hjgpu_cpra: chunks side by side (p-major) in line-aligned partitions, or C * P dense parts ----
@pytest.mark.parametrize("dense2", [0, 1])
@pytest.mark.parametrize("chunks", [3, 8])
def test_cpra(ctxs, rel, chunks, dense2):
    ctxs.set_option("dense2", dense2)
    for name in ("unique", "dups"):
        audited_join(ctxs, "cpra", rel(name), plan(chunks=chunks), probe=(0, 2), build=(3, 5))


# ---- 4. the probe side in batches: pass 1 of a batch into a small buffer, pass 2 straight from it ----
def test_batched_probe_side(ctxs, rel):
    ctxs.set_option("batch_tuples", 20_000)                 # (a third of the probe side at the most: hjgpu_api.hip, phj_prepare)
    st, st_plain = audited_join(ctxs, "phj", rel("unique"), plan(), probe=(0, 2))
    assert st["batches"] >= 2 and st_plain["batches"] >= 2


# ---- 5. option "range_tiles": the tiles of a pass-1 range ----
@pytest.mark.parametrize("range_tiles", [1, 2, 7, 1 << 20])
def test_range_tiles(ctxs, rel, range_tiles):
    a, p = ctxs.both()
    ctxs.set_option("range_tiles", range_tiles)
    a.set_option("scatter_cfg", SMALL_TILES)                # 3 and 35 tiles: 35 / 18 / 5 / 1 ranges on the probe side
    unique = rel("unique")
    ik, iv, ok, ov, want = unique
    rk, rv, sk, sv = ctxs.cols(ik, iv, ok, ov)
    # the audited exact road: stages 1 and 4 are pass 1 under this range plan
    audited_join(ctxs, "phj", unique, plan())
    audited_join(ctxs, "cpra", unique, plan(chunks=3), probe=(0, 2), build=(3, 5))
    # the claimed road of a context without the option (whole tiles of 16384 rows: 5 ranges at the most, on either side)
    for name in ("unique", "dups"):
        jk, jv, ck, cv, w = rel(name)
        c = ctxs.cols(jk, jv, ck, cv)
        assert p.phj(c[0], c[1], len(jk), c[2], c[3], len(ck), plan()) == w
        assert (p.stats()["fanout1"], p.stats()["fanout2"]) == (8, 4)
        assert p.counter("probe_exact") == 0 and p.counter("probe_fallbacks") == 0
    # a prepared build side whose option was set before hjgpu_phj_build
    for c in ctxs.both():
        seq = c.audit_next_seq()
        c.phj_build(rk, rv, len(ik), len(ok), plan())
        assert c.phj_probe(sk, sv, len(ok)) == want
        if c is a:
            build, probe = a.audit_read(seq, 2)
            assert build == join_record(seq, 1, ik, iv, ok[:0], ov[:0], M.ZERO)
            assert probe == join_record(seq + 1, 2, ik, iv, ok, ov, want, build=(5,))


# ---- 6. a build side prepared once and probed by batches ----
def test_prepared_build_side_and_its_probes(ctxs, rel):
    ik, iv, ok, ov, want = rel("unique")
    cut = 30_001                                            # (an odd row: the second batch is a column of its own, 16-byte aligned)
    rk, rv, sk, sv, sk2, sv2 = ctxs.cols(ik, iv, ok, ov, ok[cut:], ov[cut:])
    d_res = ctxs.col(4, np.uint64)
    results = {}
    for c in ctxs.both():
        seq = c.audit_next_seq()
        c.phj_build(rk, rv, len(ik), len(ok), plan())
        r1 = c.phj_probe(sk, sv, cut)
        r2 = c.phj_probe(sk2, sv2, len(ok) - cut)
        c.phj_probe_async(sk, sv, len(ok), d_res)
        c.get_async_status()
        r3 = tuple(int(x) for x in d_res.download())
        results[c] = (r1, r2, r3)
        assert r1 == numpy_join(ik, iv, ok[:cut], ov[:cut]) and r2 == numpy_join(ik, iv, ok[cut:], ov[cut:]) and r3 == want
        assert tuple(M.add_words(r1, r2)) == want
        if c is ctxs.audited:
            assert c.audit_next_seq() == seq + 4
            recs = c.audit_read(seq, 4)
            assert recs[0] == join_record(seq, 1, ik, iv, ok[:0], ov[:0], M.ZERO)
            assert recs[1] == join_record(seq + 1, 2, ik, iv, ok[:cut], ov[:cut], r1, build=(5,))
            assert recs[2] == join_record(seq + 2, 2, ik, iv, ok[cut:], ov[cut:], r2, build=(5,))
            assert recs[3] == join_record(seq + 3, 2, ik, iv, ok, ov, r3, build=(5,))
            assert recs[1][5] == recs[2][5] == recs[3][5] == recs[0][5]
            check_recheck(c, recs[3], [1, 2, 5])
    assert results[ctxs.audited] == results[ctxs.plain] and ctxs.plain.audit_next_seq() == 0


# ---- 7. hjgpu_partition_packed_async, _own_last_async, _counted_async ----
@pytest.mark.parametrize("n", [0, 1, 37, 70_001])
def test_packed_partitioning(ctxs, rel, n):
    a = ctxs.audited
    keys, vals = rel("unique")[2][:n], rel("unique")[3][:n]
    dk, dv = ctxs.col(np.concatenate([keys, np.zeros(1, np.uint32)])), ctxs.col(np.concatenate([vals, np.zeros(1, np.uint32)]))
    dt = ctxs.col(n + 16, np.uint64)
    want = M.sums(keys, vals)

    def look(seq, fanout, own_first, own_count, do):
        """the record, and the output itself under the model"""
        assert a.audit_next_seq() == seq + 1
        rec = a.audit_read(seq)[0]
        assert rec == M.record(seq, 3, n, 0, {0: want, 1: want} if n else {})
        t, o = dt.download(n), do.download().astype(np.int64)
        assert o[0] == 0 and o[-1] == n
        first, last = M.own_last_bounds(o, own_first, own_count, n)
        assert M.stage_of(t, first, last, (FACTOR1, fanout, 0, 1, 1), fanout) == want
        check_recheck(a, rec, [1] if n else [])
        return rec

    do = ctxs.col(193, np.uint64)
    seq = a.audit_next_seq()
    a.partition_packed_async(dk, dv, n, FACTOR1, 192, dt, do)
    look(seq, 192, 0, 0, do)
    for fanout, own_first, own_count in OWN_LAST:
        do = ctxs.col(fanout + 1, np.uint64)
        seq = a.audit_next_seq()
        a.partition_packed_own_last_async(dk, dv, n, FACTOR1, fanout, own_first, own_count, dt, do)
        look(seq, fanout, own_first, own_count, do)
    # the fused histogram beside the partitions, with the LDS a histogram workgroup asks for by default and with a CU to itself
    fanout, fanout2 = 12, 4
    do, dc = ctxs.col(fanout + 1, np.uint64), ctxs.col(fanout * fanout2, np.uint64)
    counts = np.bincount(mulhi_hash(keys, FACTOR1, fanout) * fanout2 + mulhi_hash(keys, FB, fanout2), minlength=fanout * fanout2)
    recs = []
    for lds in (0, 65536):
        a.set_option("hist_min_lds", lds)
        for own_first, own_count in ((0, 0), (4, 4)):
            seq = a.audit_next_seq()
            a.partition_packed_counted_async(dk, dv, n, FACTOR1, fanout, own_first, own_count, FB, fanout2, dt, do, dc)
            recs.append(look(seq, fanout, own_first, own_count, do)[:7])
            assert np.array_equal(dc.download().astype(np.int64), counts)
    assert all(r == recs[0] for r in recs)


# ---- 8. relations that arrive pass-1-partitioned ----
@pytest.mark.parametrize("interleave", [1, 0])
def test_prepartitioned_pieces(ctxs, rel, interleave):
    a, p = ctxs.both()
    ctxs.set_option("piece_interleave", interleave)
    ik, iv, ok, ov, want = rel("unique")
    ranks, k = 3, 4
    fanout = ranks * k
    sent_r, sent_s = send(p, ik, iv, ranks, fanout), send(p, ok, ov, ranks, fanout)
    most = max(sum(int(o[(g + 1) * k] - o[g * k]) for _, o in sent_r) for g in range(ranks))
    fanout2, factor2 = a.prepartitioned_plan(most, k)
    assert p.prepartitioned_plan(most, k) == (fanout2, factor2)
    sent_c = send_counted(p, ok, ov, ranks, fanout, factor2, fanout2)
    prm = H.PhjParams(fanout2=fanout2)
    d_res = ctxs.col(4, np.uint64)
    totals = {"cut": [M.ZERO], "counted": [M.ZERO], "plain": [M.ZERO]}
    wrong = []                                               # (receiver, call, record): every receiver is looked at before the test fails

    def held(what, rec, model, stages):
        if rec == model:
            check_recheck(a, rec, stages)
        else:
            wrong.append((g, what, rec))

    def probe(c, what, call, rows):
        seq = c.audit_next_seq()
        call(c)
        c.get_async_status()
        got = tuple(int(x) for x in d_res.download())
        assert got == numpy_join(rk_g, rv_g, *M.unpack(rows))
        if c is a:
            rec = a.audit_read(seq)[0]
            s = M.sums(*M.unpack(rows))
            held(what, rec, M.record(seq, 2, len(tr), len(rows), {0: s, 2: s, 5: M.sums(rk_g, rv_g), 6: got}), [2, 5])
            return rec[6]
        return list(got)

    for g in range(ranks):                                   # (g > 0: the receiver's first partition is not 0)
        tr, offr = received(sent_r, g, k)
        ts, offs = received(sent_s, g, k)
        tc, offc = received([(t, o) for t, o, _ in sent_c], g, k)
        counts = np.concatenate([c[g * k:(g + 1) * k].ravel() for _, _, c in sent_c]).astype(np.uint64)
        rk_g, rv_g = M.unpack(tr)
        assert len(tr) and len(ts) > 7
        dr, ds, dsc = (ctxs.col(np.concatenate([x, np.zeros(2, np.uint64)]), np.uint64) for x in (tr, ts, tc))
        dc = ctxs.col(counts, np.uint64)
        cut = (len(ts) * 3) // 7
        for c in ctxs.both():
            seq = c.audit_next_seq()
            c.phj_build_prepartitioned(dr, c.prepartitioned(FACTOR1, fanout, g * k, k, offr), max(len(ts), 1 << 16), prm)
            if c is a:
                built = a.audit_read(seq)[0]
                held("build", built, M.record(seq, 1, len(tr), 0, {3: M.sums(rk_g, rv_g), 5: M.sums(rk_g, rv_g)}), [5])
            for lo, hi in ((0, cut), (cut, len(ts))):
                lay = c.prepartitioned(FACTOR1, fanout, g * k, k, np.clip(offs, lo, hi))
                got = probe(c, "probe [%d, %d)" % (lo, hi), lambda c: c.phj_probe_prepartitioned_async(ds, lay, d_res), ts[lo:hi])
                totals["cut" if c is a else "plain"].append(got)
            lay = c.prepartitioned(FACTOR1, fanout, g * k, k, offc)
            got = probe(c, "counted probe", lambda c: c.phj_probe_prepartitioned_counted_async(dsc, lay, dc, d_res), tc)
            if c is a:
                totals["counted"].append(got)
    assert not wrong, wrong
    for which, words in totals.items():
        assert tuple(M.add_words(*words)) == want, which
    assert p.audit_next_seq() == 0


# ---- 9. join modes and empty sides ----
def mode_result(ik, iv, ok, ov, flags):
    """the aggregates of a semi-, left, right or full outer join by their definition in include/hjgpu.h"""
    has_partner, is_partner = np.isin(ok, ik), np.isin(ik, ok)
    if flags == H.FLAG_SEMI:
        return M.sums(ok[has_partner], ov[has_partner])[3:] + M.sums(ok[has_partner], ov[has_partner])[1:3] + (0,)
    count, keys, outer, inner = numpy_join(ik, iv, ok, ov)
    if flags & H.FLAG_LEFT_OUTER:
        _, k, v, n = M.sums(ok[~has_partner], ov[~has_partner])
        count, keys, outer = count + n, keys + k, outer + v
    if flags & H.FLAG_RIGHT_OUTER:
        _, k, v, n = M.sums(ik[~is_partner], iv[~is_partner])
        count, keys, inner = count + n, keys + k, inner + v
    return (count, keys & M.MASK, outer & M.MASK, inner & M.MASK)


@pytest.mark.parametrize("case", ["right_outer_no_probe", "semi", "full_outer"])
def test_modes_and_empty_sides(ctxs, rel, case):
    flags = {"right_outer_no_probe": H.FLAG_RIGHT_OUTER, "semi": H.FLAG_SEMI}.get(case, H.FLAG_FULL_OUTER)
    ik, iv, ok, ov, _ = rel("half")
    if case == "right_outer_no_probe":
        ok, ov = ok[:0], ov[:0]
    want = mode_result(ik, iv, ok, ov, flags)
    assert want[0] > 0 and want != numpy_join(ik, iv, ok, ov)
    audited_join(ctxs, "phj", (ik, iv, ok, ov, want), plan(flags=flags))


def test_a_left_outer_join_without_build_rows_is_a_broadcast_join(ctxs, rel):
    """inner == 0 under HJGPU_FLAG_LEFT_OUTER: every probe row with a NULL, by the broadcast road whatever the plan - not audited"""
    _, _, ok, ov, _ = rel("unique")
    e = np.zeros(0, np.uint32)
    rk, rv, sk, sv = ctxs.cols(e, e, ok, ov)
    want = M.sums(ok, ov)[3:] + M.sums(ok, ov)[1:3] + (0,)
    for c in ctxs.both():
        seq = c.audit_next_seq()
        assert c.phj(rk, rv, 0, sk, sv, len(ok), plan(flags=H.FLAG_LEFT_OUTER)) == want
        assert (c.stats()["fanout1"], c.stats()["fanout2"]) == (1, 1) and c.audit_next_seq() == seq


# ---- 10. a grouped plan: option "audit" selects the host-planned form, one record per group ----
def test_host_planned_grouped_plan(ctxs, rel):
    a, p = ctxs.both()
    ik, iv, ok, ov, want = rel("unique")
    groups = 5
    for name, value in (("group_from", 1000), ("group_always", 1), ("group_inner", BUILD // 4)):
        ctxs.set_option(name, value)
    rk, rv, sk, sv = ctxs.cols(ik, iv, ok, ov)
    seq = a.audit_next_seq()
    got = a.phj(rk, rv, len(ik), sk, sv, len(ok))
    assert a.stats()["groups"] == groups and a.audit_next_seq() == seq + groups
    recs = a.audit_read(seq, groups)
    for i, rec in enumerate(recs):
        # a whole join of the group's rows: every stage of a relation holds the same sums, nothing is misplaced
        assert rec[7][:2] == [seq + i, 0] and rec[7][2] == rec[3][3] > 0 and rec[7][3] == rec[0][3] > 0
        assert all(rec[s][0] == 0 for s in range(6))
        assert rec[2] == rec[0] and rec[1] in (M.ZERO, rec[0]) and rec[5] == rec[3] and rec[4] in (M.ZERO, rec[3])
    assert M.add_words(*[r[0] for r in recs]) == list(M.sums(ok, ov))
    assert M.add_words(*[r[3] for r in recs]) == list(M.sums(ik, iv))
    assert tuple(M.add_words(*[r[6] for r in recs])) == got == want
    assert p.phj(rk, rv, len(ik), sk, sv, len(ok)) == want and p.stats()["groups"] == groups and p.audit_next_seq() == 0


# ---- 11. records are zeroed and written on the call's stream ----
def test_two_joins_queued_back_to_back(ctxs, rel):
    first, second = rel("unique"), rel("other")
    c1, c2 = ctxs.cols(*first[:4]), ctxs.cols(*second[:4])
    d1, d2 = ctxs.col(4, np.uint64), ctxs.col(4, np.uint64)
    for c in ctxs.both():
        # (the workspace of both shapes first: nothing grows, and so nothing waits, between the two joins below)
        for cols, r in ((c2, second), (c1, first)):
            assert c.phj(cols[0], cols[1], len(r[0]), cols[2], cols[3], len(r[2]), plan()) == r[4]
        seq = c.audit_next_seq()
        c.phj_async(c1[0], c1[1], len(first[0]), c1[2], c1[3], len(first[2]), plan(), d1)
        c.phj_async(c2[0], c2[1], len(second[0]), c2[2], c2[3], len(second[2]), plan(), d2)
        c.get_async_status()
        assert tuple(int(x) for x in d1.download()) == first[4] and tuple(int(x) for x in d2.download()) == second[4]
        if c is ctxs.audited:
            recs = c.audit_read(seq, 2)
            assert recs[0] == join_record(seq, 0, *first)
            assert recs[1] == join_record(seq + 1, 0, *second)
            check_recheck(c, recs[1], [1, 2, 4, 5])
    assert ctxs.plain.audit_next_seq() == 0


# ---- 12. what is not audited ----
def test_calls_that_leave_no_record(ctxs, rel):
    a, p = ctxs.both()
    ik, iv, ok, ov, want = rel("unique")
    rk, rv, sk, sv = ctxs.cols(ik, iv, ok, ov)
    with pytest.raises(H.HjGpuError) as e:                  # a context that never audited has no records
        p.audit_read(0, 1)
    assert e.value.status == H.api.EINVAL
    with pytest.raises(H.HjGpuError) as e:                  # nor has one that has the option and made no call yet
        a.audit_read(0, 1)
    assert e.value.status == H.api.EINVAL
    assert a.audit_read(0, 0) == [] and a.audit_next_seq() == 0
    assert a.npj(rk, rv, len(ik), sk, sv, len(ok)) == want
    ko, vo, off = ctxs.col(len(ok)), ctxs.col(len(ok)), ctxs.col(9, np.uint64)
    a.partition(sk, sv, len(ok), FA, 8, ko, vo, off)
    assert int(off.download()[-1]) == len(ok)
    assert a.phj(rk, rv, 37, sk, sv, len(ok)) == numpy_join(ik[:37], iv[:37], ok, ov)         # a tiny build side: the broadcast join
    assert (a.stats()["fanout1"], a.stats()["fanout2"]) == (1, 1)
    assert a.filter_selected(None, len(ok), [sk], [(0, 0x7FFFFFFF)]) == int(np.count_nonzero(ok <= 0x7FFFFFFF))
    assert a.audit_next_seq() == 0
    a.set_option("audit", 0)
    assert a.phj(rk, rv, len(ik), sk, sv, len(ok), plan()) == want
    assert a.audit_next_seq() == 0
    a.set_option("audit", 1)
    assert a.phj(rk, rv, len(ik), sk, sv, len(ok), plan()) == want
    assert a.audit_next_seq() == 1 and a.audit_read(0)[0] == join_record(0, 0, ik, iv, ok, ov, want)


# ---- 13. the ring of the last 256 records ----
def test_the_ring_keeps_the_last_256_records(ctxs, rel):
    a = ctxs.audited
    calls, ring = 260, 256
    keys, vals = rel("unique")[2][:37 + calls], rel("unique")[3][:37 + calls]
    dk, dv, dt, do = ctxs.col(keys), ctxs.col(vals), ctxs.col(37 + calls + 16, np.uint64), ctxs.col(9, np.uint64)
    for i in range(calls):
        a.partition_packed_async(dk, dv, 37 + i, FACTOR1, 8, dt, do)
    nxt = a.audit_next_seq()
    assert nxt == calls
    recs = a.audit_read(nxt - ring, ring)
    for j, rec in enumerate(recs):
        i = nxt - ring + j
        s = M.sums(keys[:37 + i], vals[:37 + i])
        assert rec == M.record(i, 3, 37 + i, 0, {0: s, 1: s}), i
    assert a.audit_read(nxt - 1)[0] == recs[-1] and a.audit_read(nxt - ring)[0] == recs[0]
    for first_seq, count in ((nxt - ring - 1, 1), (nxt - ring - 1, ring), (nxt, 1), (nxt - 1, 2), (nxt - ring, ring + 1)):
        with pytest.raises(H.HjGpuError) as e:
            a.audit_read(first_seq, count)
        assert e.value.status == H.api.EINVAL, (first_seq, count)
    nothing = C.c_uint64(77)
    assert a.lib.hjgpu_audit_read(a.handle, C.byref(nothing), nxt - ring - 1, 0, None, None) == H.api.OK and nothing.value == nxt
    assert a.lib.hjgpu_audit_read(a.handle, None, 0, 1, None, None) == H.api.EINVAL             # records asked for, no array


# ---- 14. hjgpu_audit_recheck's two-call protocol ----
def test_recheck_without_room_only_counts(ctxs, rel):
    a, p = ctxs.both()
    ik, iv, ok, ov, want = rel("unique")
    rk, rv, sk, sv = ctxs.cols(ik, iv, ok, ov)
    n = C.c_size_t(99)
    assert a.lib.hjgpu_audit_recheck(a.handle, None, 0, C.byref(n)) == H.api.OK and n.value == 0           # before any audited call
    assert a.audit_recheck() == [] and p.audit_recheck() == []
    assert a.phj(rk, rv, len(ik), sk, sv, len(ok), plan()) == want
    rec = a.audit_read(0)[0]
    sentinel = 0xA5A5A5A5A5A5A5A5
    buf = (C.c_uint64 * (9 * 4))(*([sentinel] * 36))
    for words, capacity in ((None, 4), (buf, 3), (buf, 0)):
        n = C.c_size_t(99)
        assert a.lib.hjgpu_audit_recheck(a.handle, words, capacity, C.byref(n)) == H.api.OK
        assert n.value == 4 and all(x == sentinel for x in buf)
    n = C.c_size_t(99)
    assert a.lib.hjgpu_audit_recheck(a.handle, buf, 4, C.byref(n)) == H.api.OK and n.value == 4
    assert sorted(int(buf[9 * i]) for i in range(4)) == [1, 2, 4, 5]
    for i in range(4):
        assert [int(x) for x in buf[9 * i + 1:9 * i + 5]] == [int(x) for x in buf[9 * i + 5:9 * i + 9]] == rec[int(buf[9 * i])]
    assert a.lib.hjgpu_audit_recheck(a.handle, buf, 4, None) == H.api.EINVAL
    assert a.audit_next_seq() == 1                            # a second look is no call
