"""CPU test of tests/operator_cases.py: every named case of the operator-level GPU tests has the property it is named for (an edit of a
size moves no case off its kernel's edge unnoticed), the constants it states are the kernels', and its references agree with a
brute-force double loop."""
import os
import re
import subprocess

import numpy as np
import pytest

import operator_cases as oc
from helpers import mulhi_hash, numpy_join, materialised_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc")


# ---- the constants ---------------------------------------------------------------------------------------------------
def test_join_constants_are_hj_internals():
    text = open(os.path.join(CSRC, "hj_internal.hpp")).read()
    assert int(re.search(r"constexpr int HJ_JOIN_SLICE\s*=\s*1 << (\d+);", text).group(1)) == oc.JOIN_SLICE.bit_length() - 1
    assert int(re.search(r"constexpr int HJ_JOIN_FILL_GROUPS\s*=\s*(\d+);", text).group(1)) == oc.FILL_GROUPS
    # JoinConfig::cap() = slots() / 2 = 2^log2slots / 2 of the default join_cfg
    assert re.search(r"int cap\(\) const \{ return slots\(\) / 2; \}", text) and re.search(r"int slots\(\) const \{ return 1 << log2slots; \}", text)
    block, log2slots, batch = map(int, re.search(r"JoinConfig join = \{(\d+), (\d+), (\d+)\};", text).groups())
    assert (1 << log2slots) // 2 == oc.FILL_ROWS


def test_scatter_constants_are_the_layout_headers(tmp_path):
    exe = tmp_path / "operator_constants"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp_operator_constants.cpp"),
                           "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    named = {l.split()[0]: int(l.split()[1]) for l in lines if l and not l.startswith("tile")}
    assert named["HJ_STREAM_UNIT"] == oc.STREAM_UNIT and named["HJ_MAX_HEAVY"] == oc.MAX_HEAVY
    tiles = {int(f): (int(t), int(c)) for _, f, t, c in (l.split() for l in lines if l.startswith("tile"))}
    assert len(tiles) == 1024
    for F, (tile, carry) in tiles.items():
        assert oc.packed_tile(F) == tile, F
        assert carry == (F <= oc.CARRY_TILES[-1][0]), F
    # the fan-outs the seam tests use sit on both sides of every change of geometry
    for fmax, tile in oc.CARRY_TILES:
        assert fmax in oc.PACKED_FANOUTS and fmax + 1 in oc.PACKED_FANOUTS
        assert tiles[fmax][0] == tile and tiles[fmax + 1][0] != tile
    assert oc.PLAIN_TILE == tiles[1024][0] and 1024 in oc.PACKED_FANOUTS
    for F, _ in oc.COUNTED_FANOUTS:
        assert F in (217, 661, 1024)
    assert {oc.packed_tile(F) for F, _ in oc.COUNTED_FANOUTS} == {12288, 16384}
    # CTL_NEXT_HOT: "if it held > 1/16 of the tile"
    text = open(os.path.join(CSRC, "scatter_layout.hpp")).read()
    assert "if it held > 1/%d of the tile" % oc.HOT_SHARE in text


# ---- keys_in_partition, co_partitioned -------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(0, 50, 0x9E3779B1, 1), (3, 100, 0x9E3779B1, 7), (34, 64, oc.F_ONE, 5, oc.F_TWO, 7),
                                  (32767, 5, oc.F_ONE, 1024, oc.F_TWO, 32), (1023, 300, oc.F_PART, 1024)])
def test_keys_in_partition_hash_to_it(args):
    q, n = args[0], args[1]
    lay = oc.Layout(*args[2:])
    keys = oc.keys_in_partition(*args, rng=np.random.default_rng(1))
    assert keys.dtype == np.uint32 and len(keys) == n and len(np.unique(keys)) == n
    assert (lay.pid(keys) == q).all()
    p1 = mulhi_hash(keys, lay.f1, lay.F1)
    want = p1 * lay.F2 + (mulhi_hash(keys, lay.f2, lay.F2) if lay.F2 > 1 else 0)
    assert (want == q).all()
    again = oc.keys_in_partition(*args, rng=np.random.default_rng(1))
    assert np.array_equal(keys, again)
    dup = oc.keys_in_partition(*args, rng=np.random.default_rng(1), distinct=False)
    assert len(dup) == n and (lay.pid(dup) == q).all()


def test_co_partitioned_offsets_and_poison():
    lay = oc.Layout(oc.F_ONE, 4)
    rng = np.random.default_rng(2)
    bp = [(oc.keys_in_partition(q, q + 1, *lay.args(), rng=rng), np.full(q + 1, q, np.uint32)) for q in range(4)]
    pp = [(np.concatenate([b[0], b[0]]), np.full(2 * len(b[0]), 100 + q, np.uint32)) for q, b in enumerate(bp)]
    rk, rv, sk, sv, roff, soff = oc.co_partitioned(bp, pp)
    assert roff.dtype == np.uint64 and soff.dtype == np.uint64
    assert roff.tolist() == [0, 1, 3, 6, 10] and soff.tolist() == [0, 2, 6, 12, 20] and len(rk) == 10 and len(sk) == 20
    rk2, rv2, sk2, sv2, roff2, soff2 = oc.co_partitioned(bp, pp, lead_r=5, lead_s=3)
    assert roff2.tolist() == [5, 6, 8, 11, 15] and soff2.tolist() == [3, 5, 9, 15, 23] and len(rk2) == 20 and len(sk2) == 26
    assert np.array_equal(rk2[5:15], rk) and np.array_equal(rv2[5:15], rv) and np.array_equal(sk2[3:23], sk) and np.array_equal(sv2[3:23], sv)
    # the front poison carries keys of the other side's first partition, the back poison of its last
    assert np.isin(rk2[:5], pp[0][0]).all() and np.isin(rk2[15:], pp[3][0]).all()
    assert np.isin(sk2[:3], bp[0][0]).all() and np.isin(sk2[23:], bp[3][0]).all()
    assert (rv2[:5] >= oc.POISON_FRONT).all() and (sv2[23:] >= oc.POISON_BACK).all()


# ---- the references against a double loop ---------------------------------------------------------------------------
def _small_relations(seed, inner, outer, distinct):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 1 << 32, size=distinct, dtype=np.uint64).astype(np.uint32)
    ik = d[rng.integers(0, distinct, size=inner)] if inner else np.zeros(0, np.uint32)
    ok = np.concatenate([d[rng.integers(0, distinct, size=outer - outer // 3)], rng.integers(0, 1 << 32, size=outer // 3, dtype=np.uint64).astype(np.uint32)])
    vals = lambda n: rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    return ik, vals(inner), ok, vals(len(ok))


@pytest.mark.parametrize("seed,inner,outer,distinct", [(1, 0, 10, 4), (2, 1, 1, 1), (3, 60, 140, 20), (4, 100, 100, 100), (5, 90, 110, 3)])
def test_references_agree_with_a_double_loop(seed, inner, outer, distinct):
    ik, iv, ok, ov = _small_relations(seed, inner, outer, distinct)
    assert len(ik) + len(ok) <= 200
    agg, rows = oc.brute_force(ik, iv, ok, ov)
    assert numpy_join(ik, iv, ok, ov) == agg
    k, o, i = materialised_rows(ik, iv, ok, ov)
    assert list(zip(k.tolist(), o.tolist(), i.tolist())) == rows
    # first match
    (count, sum_keys, sum_outer), hits = oc.brute_force_unique(ik, iv, ok, ov)
    got = oc.unique_reference(ik, iv, ok, ov)
    assert got[:3] == (count, sum_keys, sum_outer)
    all_shared = all(len(set(h[2])) == 1 for h in hits)
    if oc.shared_payloads(ik, iv):
        assert all_shared and got[3] == sum(h[2][0] for h in hits) & oc.M64
    else:
        assert got[3] is None
    # rows that report any one copy pass, a row with a foreign payload or a lost row does not
    for pick in (0, -1):
        gk = np.array([h[0] for h in hits], np.uint32); go = np.array([h[1] for h in hits], np.uint32)
        gi = np.array([h[2][pick] for h in hits], np.uint32)
        assert oc.unique_rows_match(ik, iv, ok, ov, gk, go, gi)
        if len(hits):
            assert not oc.unique_rows_match(ik, iv, ok, ov, gk[1:], go[1:], gi[1:])
            bad = gi.copy(); bad[0] ^= np.uint32(0x5A5A5A5A)
            if not np.isin(oc.pairs(gk[:1], bad[:1]), oc.pairs(ik, iv)).any():
                assert not oc.unique_rows_match(ik, iv, ok, ov, gk, go, bad)


def test_case_references_on_a_small_case_agree_with_a_double_loop():
    for name in ("p2_minimum", "sizes_0_to_5_at_5x7"):
        case = oc.join_case(name)
        ik, iv, ok, ov = case.real()
        assert len(ik) + len(ok) <= 200
        agg, rows = oc.brute_force(ik, iv, ok, ov)
        want_agg, (k, o, i) = case.reference()
        assert want_agg == agg and list(zip(k.tolist(), o.tolist(), i.tolist())) == rows
        assert agg[0] > 0


# ---- hjgpu_join_partitions: every named case ------------------------------------------------------------------------
def _fill_of_rows(n):
    return np.arange(n) // oc.FILL_ROWS


@pytest.mark.parametrize("name", list(oc.JOIN_BUILDERS))
def test_join_case_has_the_property_it_is_named_for(name):
    case = oc.join_case(name)
    lay, props = case.lay, case.props
    P = lay.P
    assert 2 <= P <= 32768 and len(case.roff) == P + 1 and len(case.soff) == P + 1
    assert case.roff.dtype == np.uint64 and case.soff.dtype == np.uint64
    roff, soff = case.roff.astype(np.int64), case.soff.astype(np.int64)
    assert (np.diff(roff) >= 0).all() and (np.diff(soff) >= 0).all()
    assert roff[0] == case.lead and soff[0] == case.lead and len(case.rk) == roff[-1] + case.lead and len(case.sk) == soff[-1] + case.lead
    # every row of every partition hashes to it
    ik, iv, ok, ov = case.real()
    assert np.array_equal(lay.pid(ik), np.repeat(np.arange(P), np.diff(roff)))
    assert np.array_equal(lay.pid(ok), np.repeat(np.arange(P), np.diff(soff)))
    assert case.reference()[0][0] > 0, "a join without a single row checks little"
    assert not np.isin(ok, ik).all(), "misses belong to every case"
    rn, sn = np.diff(roff), np.diff(soff)

    if "partitions" in props:
        assert P == props["partitions"]
    if "fills" in props:
        q, k = props["fills"]
        assert (k - 1) * oc.FILL_ROWS < rn[q] <= k * oc.FILL_ROWS and sn[q] > 0
        assert (np.delete(rn, q) <= oc.FILL_ROWS).all()
    else:
        assert (rn <= oc.FILL_ROWS).all()
    if "slices" in props:
        q, s = props["slices"]
        assert (s - 1) * oc.JOIN_SLICE < sn[q] <= s * oc.JOIN_SLICE and rn[q] > 0
        assert (np.delete(sn, q) <= oc.JOIN_SLICE).all()
    else:
        assert (sn <= oc.JOIN_SLICE).all()
    if "build_rows" in props:
        assert rn[props["build_rows"][0]] == props["build_rows"][1]
    if "probe_rows" in props:
        assert sn[props["probe_rows"][0]] == props["probe_rows"][1]
    if props.get("unique_build_keys"):
        assert len(np.unique(ik)) == len(ik)
    if props.get("residues"):
        # among the partitions that have work (both sides non-empty)
        work = (rn > 0) & (sn > 0)
        assert set((soff[:-1][work] % 4).tolist()) == {0, 1, 2, 3} and set((roff[:-1][work] % 4).tolist()) == {0, 1, 2, 3}
    if props.get("small_sizes"):
        assert set(rn.tolist()) == set(range(6)) and set(sn.tolist()) == set(range(6))
        assert {(bool(r), bool(s)) for r, s in zip(rn, sn)} == {(False, False), (False, True), (True, False), (True, True)}
        assert rn[0] == 0 and sn[0] == 0 and rn[-1] == 0 and sn[-1] == 0
        assert len(case.sk) % 4 != 0
    if props.get("poison"):
        assert case.lead > 0
        r0, r1, s0, s1 = roff[0], roff[-1], soff[0], soff[-1]
        for pk, pv in ((case.rk[:r0], case.rv[:r0]), (case.rk[r1:], case.rv[r1:])):
            assert len(pk) == case.lead and numpy_join(pk, pv, ok, ov)[0] > 0           # a poison build row read as real adds rows
        for pk, pv in ((case.sk[:s0], case.sv[:s0]), (case.sk[s1:], case.sv[s1:])):
            assert len(pk) == case.lead and numpy_join(ik, iv, pk, pv)[0] > 0           # and so does a poison probe row
        # the poison next to the first / last partition matches THAT partition: a vector's head or tail mask that is off by one counts it
        assert np.isin(case.sk[s0 - 1], ik[:rn[0]]) and np.isin(case.sk[s1], ik[len(ik) - rn[-1]:])
        assert np.isin(case.rk[r0 - 1], ok[:sn[0]]) and np.isin(case.rk[r1], ok[len(ok) - sn[-1]:])
        assert rn[0] > 0 and sn[0] > 0 and rn[-1] > 0 and sn[-1] > 0
    if "chained" in props:
        q, copies = props["chained"]
        k = ik[roff[q] - roff[0]:roff[q + 1] - roff[0]]
        fills = _fill_of_rows(len(k))
        per_fill = {}
        for key, f in zip(k.tolist(), fills.tolist()):
            per_fill[(key, f)] = per_fill.get((key, f), 0) + 1
        assert max(per_fill.values()) >= copies and min(c for c in per_fill.values() if c > 1) >= copies
        counts = np.unique(k, return_counts=True)[1]
        assert set(counts.tolist()) == set(props["copies"])
        heavy = np.unique(k)[np.argmax(counts)]
        assert len(set(fills[k == heavy].tolist())) >= 2, "the key with the most copies spans fills"
        pk = ok[soff[q] - soff[0]:soff[q + 1] - soff[0]]
        assert np.isin(np.unique(k), pk).all(), "every key of the chained partition is probed"
    if "single_fill" in props:
        for q, copies in zip(props["single_fill"], props["copies"]):
            k = ik[roff[q] - roff[0]:roff[q + 1] - roff[0]]
            assert len(k) <= oc.FILL_ROWS and set(np.unique(k, return_counts=True)[1].tolist()) == {copies}
        assert oc.shared_payloads(ik, iv) == props["shared"]
        assert (case.unique_reference()[3] is not None) == props["shared"]
    if "one_copy_per_fill" in props:
        q = props["one_copy_per_fill"]
        k = ik[roff[q] - roff[0]:roff[q + 1] - roff[0]]
        fills = _fill_of_rows(len(k))
        pairs_kf = np.unique(np.stack([k.astype(np.int64), fills]), axis=1)
        assert pairs_kf.shape[1] == len(k), "at most one copy of a key per fill"
        assert (np.unique(k, return_counts=True)[1] >= 2).all(), "every key in at least two fills"
        assert not oc.shared_payloads(ik, iv)
        assert case.unique_reference()[0] < case.reference()[0][0]
    if props.get("edge_keys"):
        for side in (ik, ok):
            assert np.isin(oc.EDGE_KEYS, side).all()
        assert set(iv.tolist()) == {0, oc.M32} and set(ov.tolist()) == {0, oc.M32}
        # every partition's empty sentinel - the smallest value that does not hash to it - is a probe key of ANOTHER partition, and the
        # values below it are keys of this one
        for q in range(P):
            e = 0
            while lay.pid(np.array([e], np.uint32))[0] == q:
                e += 1
            assert e < 64 and e in ok
    if case.unique:
        want = case.unique_reference()
        assert 0 < want[0] <= len(ok)


def test_case_lists_cover_the_builders():
    assert set(oc.INNER_CASES) | set(oc.FIRST_MATCH_CASES) == set(oc.JOIN_BUILDERS)
    assert all(oc.join_case(n).unique for n in oc.FIRST_MATCH_CASES) and not any(oc.join_case(n).unique for n in oc.INNER_CASES)
    for n in oc.FORCE_CHAINED_CASES:
        ik = oc.join_case(n).real()[0]
        assert n in oc.INNER_CASES and (np.unique(ik, return_counts=True)[1] <= 2).all()
    assert {oc.join_case("lead_%d" % l).lead for l in (1, 37, 4099)} == {1, 37, 4099}
    big = oc.join_case("build_rows_262145")
    assert big.props["fills"] == (1, oc.FILL_GROUPS + 1) and big.props["slices"] == (1, 2)
    assert max(len(oc.join_case(n).rk) for n in oc.JOIN_BUILDERS) == len(big.rk)


def test_three_ways_relations_have_duplicates_and_misses():
    ik, iv, ok, ov = oc.three_ways_relations()
    counts = np.unique(ik, return_counts=True)[1]
    assert set(counts.tolist()) == {1, 2, 3}
    assert 0 < np.isin(ok, ik).sum() < len(ok) and len(np.unique(ok)) < len(ok)
    assert len(ok) % 4 != 0


# ---- the partition operators -------------------------------------------------------------------------------------------
def test_seam_rows_and_own_ranges():
    for tile in (8192, 12288, 16384):
        assert oc.seam_rows(tile) == (tile - 1, tile, tile + 1, 2 * tile + 17)
    for F in oc.PACKED_FANOUTS:
        ranges = oc.own_ranges(F)
        assert all(a + b <= F for a, b in ranges)
        first, middle, last, whole, empty = ranges
        assert first[0] == 0 and 0 < first[1] < F and 0 < middle[0] and middle[0] + middle[1] < F and middle[1] > 0
        assert last[0] + last[1] == F and last[0] > 0 and whole == (0, F) and empty[1] == 0


@pytest.mark.parametrize("fanout", [1, 2, 216, 437, 661, 1024])
@pytest.mark.parametrize("dist", oc.DISTRIBUTIONS)
def test_partition_inputs_have_the_distribution_they_are_named_for(dist, fanout):
    tile = oc.PLAIN_TILE if fanout < 216 else oc.packed_tile(fanout)
    n = 2 * tile + 17
    keys, vals = oc.partition_input(dist, n, fanout, tile)
    assert keys.dtype == np.uint32 and vals.dtype == np.uint32 and len(keys) == n and len(vals) == n
    assert len(np.unique(vals)) == n, "distinct payloads: a row written twice, or lost, shows in the multiset"
    pid = mulhi_hash(keys, oc.F_PART, fanout)
    per_tile = [np.bincount(pid[b:b + tile], minlength=fanout) for b in range(0, n, tile)]
    full = per_tile[:2]
    if dist == "all_in_first":
        assert (pid == 0).all()
    elif dist == "all_in_last":
        assert (pid == fanout - 1).all()
    elif dist == "sorted":
        assert (np.diff(pid) >= 0).all()
    elif fanout >= 3 and dist.startswith("hot"):
        hot = (fanout // 3, (2 * fanout) // 3)
        for t, c in enumerate(full):
            p = hot[t & 1] if dist == "hot_alternating" else hot[0]
            want = tile // oc.HOT_SHARE + (0 if dist == "hot_at_threshold" else 1)
            assert c[p] == want and c.argmax() == p and c[hot[1] if p == hot[0] else hot[0]] == 0
            # on the side of CTL_NEXT_HOT it is named for: hot means MORE than 1 / 16 of the tile
            assert (c[p] * oc.HOT_SHARE > tile) == (dist != "hot_at_threshold")
    elif dist == "heavy_runs":
        parts = oc.heavy_partitions(tile, fanout)
        for c in full:
            assert (c > 0).sum() == parts and (c[c > 0] > oc.STREAM_UNIT).all()
            assert (c[c > 0] // oc.STREAM_UNIT).sum() <= oc.MAX_HEAVY
        if tile == 16384 and fanout >= 60:
            assert parts == 60 and 265 <= full[0].max() <= 275
    # the reference's offsets and the three-case rule
    for own_first, own_count in oc.own_ranges(fanout) if fanout >= 8 else ((0, 0),):
        off, first = oc.partition_reference(keys, fanout, own_first=own_first, own_count=own_count)
        assert off[0] == 0 and off[-1] == n and np.array_equal(np.diff(off), np.bincount(pid, minlength=fanout))
        want = oc.expected_partition_of_rows(off, first)
        assert (want >= 0).all() and np.array_equal(np.bincount(want, minlength=fanout), np.diff(off))
        own = (want >= own_first) & (want < own_first + own_count)
        own_rows = int(own.sum())
        assert own[n - own_rows:].all() and not own[:n - own_rows].any()
        assert (np.diff(want[:n - own_rows]) >= 0).all() and (np.diff(want[n - own_rows:]) >= 0).all()
    c2 = oc.counts2_reference(keys, fanout, 3)
    assert np.array_equal(c2.reshape(fanout, 3).sum(axis=1), np.bincount(pid, minlength=fanout))


# ---- NPJ ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", oc.NPJ_ROWS)
def test_npj_cases(n):
    ik, iv, ok, ov = oc.npj_case(n)
    assert len(ik) == n and (ik != 0).all()
    assert set(np.unique(ik, return_counts=True)[1].tolist()) == set(oc.NPJ_COPIES[n])
    assert np.isin(np.unique(ik), ok).all() and (ok == 0).sum() == 1 and not np.isin(ok, ik).all()
    assert numpy_join(ik, iv, ok, ov)[0] > len(np.unique(ik))
    if len(ik) + len(ok) <= 200:
        agg, rows = oc.brute_force(ik, iv, ok, ov)
        assert numpy_join(ik, iv, ok, ov) == agg
