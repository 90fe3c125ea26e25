"""Inputs and references of the operator-level tests (numpy only, so that tests/test_operator_cases.py can check every case on a machine
without a GPU): hjgpu_join_partitions (tests/test_gpu_join_partitions.py), the partition operators at their geometry seams
(tests/test_gpu_partition_seams.py) and hjgpu_npj_build / hjgpu_npj_probe (tests/test_gpu_npj_operators.py).

A case is NAMED for the edge of a kernel it sits on - "the partition that takes 65 fills", "the probe partition of 65 537 rows" - and
tests/test_operator_cases.py asserts that property for every case: a later edit of a size moves no case off its edge unnoticed.

The reference of every join is helpers.numpy_join / helpers.materialised_rows over the concatenated REAL rows of the partitions (a case
may put poison rows in front of the first partition and behind the last one: they match the other side, so a read outside
[offsets[0], offsets[P]) changes the result)."""
import functools

import numpy as np

from helpers import mulhi_hash, numpy_join, materialised_rows, pairs

# ---- constants of the kernels ----------------------------------------------------------------------------------
# hash_join_codes_knl_amd/csrc/hj_internal.hpp needs the HIP headers; tests/test_operator_cases.py reads these three out of its text.
FILL_ROWS = 4096        # JoinConfig::cap() of the default "join_cfg" (512 threads, 2^13 slots): build rows per LDS table fill
JOIN_SLICE = 1 << 16    # HJ_JOIN_SLICE: probe rows per work item
FILL_GROUPS = 64        # HJ_JOIN_FILL_GROUPS: work items the fills of one partition are dealt to
# hash_join_codes_knl_amd/csrc/scatter_layout.hpp compiles without HIP: tests/cpp_operator_constants.cpp prints these from it, and
# tests/test_operator_cases.py compares.  K6 pass 1 with packed output (hj_scatter_config, partition_kernels.hip): the largest tile of
# 1024 threads x {4, 3, 2} vectors whose carry buffers fit the LDS beside it; beyond the last fan-out, and for column output, 1024 x 4
# without carry.
CARRY_TILES = ((216, 16384), (436, 12288), (660, 8192))     # (largest fan-out, tuples per tile)
PLAIN_TILE = 16384
STREAM_UNIT = 256       # HJ_STREAM_UNIT: a run longer than this lists its further units in `heavy`
MAX_HEAVY = 128         # HJ_MAX_HEAVY
HOT_SHARE = 16          # CTL_NEXT_HOT: a partition is hot when it holds MORE than 1 / 16 of a tile

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def packed_tile(fanout):
    """tuples per tile of K6 pass 1 with packed output at this fan-out"""
    for fmax, tile in CARRY_TILES:
        if fanout <= fmax:
            return tile
    return PLAIN_TILE


# ---- keys of one partition -------------------------------------------------------------------------------------
class Layout:
    """the passes that made the partitions: p = H(k, f1, F1) * F2 + H(k, f2, F2)"""

    def __init__(self, f1, F1, f2=None, F2=1):
        assert f1 & 1 and (F2 == 1 or (f2 is not None and f2 & 1))
        self.f1, self.F1, self.f2, self.F2 = f1, F1, f2, F2
        self.P = F1 * F2

    def pid(self, keys):
        p = mulhi_hash(keys, self.f1, self.F1)
        if self.F2 > 1:
            p = p * self.F2 + mulhi_hash(keys, self.f2, self.F2)
        return p

    def args(self):
        return (self.f1, self.F1, self.f2, self.F2)


def keys_in_partition(q, n, f1, F1, f2=None, F2=1, rng=None, distinct=True):
    """n random uint32 keys with mulhi_hash(k, f1, F1) * F2 + mulhi_hash(k, f2, F2) == q.  The candidates are drawn where the first level
    can accept them (k * f1 mod 2^32 uniform in partition q // F2's window, k = that times f1's inverse): the draw is uniform over the
    partition's keys and costs F2 candidates per key instead of F1 * F2; every candidate still passes through mulhi_hash."""
    rng = rng if rng is not None else np.random.default_rng(q)
    lay = Layout(f1, F1, f2, F2)
    assert 0 <= q < lay.P
    p1 = q // F2
    lo, hi = -((-p1 << 32) // F1), -((-(p1 + 1) << 32) // F1)      # ceil(p1 2^32 / F1), ceil((p1 + 1) 2^32 / F1)
    assert not distinct or 2 * n * F2 <= hi - lo, "partition too small for that many distinct keys"
    inv = np.uint64(pow(f1, -1, 1 << 32))
    out = np.zeros(0, np.uint32)
    while len(out) < n:
        x = rng.integers(lo, hi, size=int((n - len(out)) * F2 * 1.25) + 64, dtype=np.uint64)
        k = ((x * inv) & np.uint64(M32)).astype(np.uint32)
        out = np.concatenate([out, k[lay.pid(k) == q]])
        if distinct:
            _, first = np.unique(out, return_index=True)
            out = out[np.sort(first)]
    return out[:n]


def partition_on_host(keys, vals, lay):
    """(keys, vals) sorted by partition (stable), and the P + 1 offsets"""
    pid = lay.pid(keys)
    order = np.argsort(pid, kind="stable")
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.bincount(pid, minlength=lay.P), dtype=np.uint64)])
    return keys[order], vals[order], off


def split_parts(keys, vals, lay):
    k, v, off = partition_on_host(keys, vals, lay)
    o = off.astype(np.int64)
    return [(k[o[p]:o[p + 1]], v[o[p]:o[p + 1]]) for p in range(lay.P)]


# ---- co-partitioned columns ---------------------------------------------------------------------------------
POISON_FRONT, POISON_BACK = 0xBAD00000, 0xBAD80000


def co_partitioned(build_parts, probe_parts, lead_r=0, lead_s=0):
    """(rk, rv, sk, sv, roff, soff): the partitions back to back, offsets of P + 1 uint64.  lead_r / lead_s > 0: that many poison rows in
    front of row roff[0] / soff[0] and as many behind the last partition.  A poison row's key is a key of the OTHER side's first (last)
    non-empty partition, its payload POISON_FRONT (POISON_BACK) + i: read as a row of the neighbouring partition, it matches."""
    assert len(build_parts) == len(probe_parts)

    def poison(n, donors, tag):
        assert len(donors), "poison rows need keys of the other side"
        return np.resize(donors, n).astype(np.uint32), (tag + np.arange(n)).astype(np.uint32)

    def side(parts, lead, other):
        sizes = np.array([len(k) for k, _ in parts], dtype=np.uint64)
        off = np.uint64(lead) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)])
        keys = [np.asarray(k, np.uint32) for k, _ in parts]
        vals = [np.asarray(v, np.uint32) for _, v in parts]
        if lead:
            donors = [np.asarray(k, np.uint32) for k, _ in other if len(k)]
            assert donors, "poison rows need keys of the other side"
            fk, fv = poison(lead, donors[0], POISON_FRONT)
            bk, bv = poison(lead, donors[-1], POISON_BACK)
            keys, vals = [fk] + keys + [bk], [fv] + vals + [bv]
        return np.concatenate(keys + [np.zeros(0, np.uint32)]), np.concatenate(vals + [np.zeros(0, np.uint32)]), off

    rk, rv, roff = side(build_parts, lead_r, probe_parts)
    sk, sv, soff = side(probe_parts, lead_s, build_parts)
    return rk, rv, sk, sv, roff, soff


# ---- references ---------------------------------------------------------------------------------------------------
def _sum(a):
    return int(np.asarray(a).astype(np.uint64).sum(dtype=np.uint64)) & M64


def shared_payloads(ik, iv):
    """do all copies of every build key carry one payload?"""
    order = np.lexsort((iv, ik))
    k, v = ik[order], iv[order]
    same = k[1:] == k[:-1]
    return bool(np.all(v[1:][same] == v[:-1][same]))


def unique_reference(ik, iv, ok, ov):
    """first-match join (HJGPU_FLAG_UNIQUE): count, sum_keys and sum_outer_vals over the probe rows with at least one partner;
    sum_inner_vals when all copies of a key share one payload, else None (then the rows are checked: unique_rows_match)"""
    has = np.isin(ok, ik)
    inner = None
    if shared_payloads(ik, iv):
        order = np.argsort(ik, kind="stable")
        inner = _sum(iv[order][np.searchsorted(ik[order], ok[has], side="left")])
    return (int(has.sum()), _sum(ok[has]), _sum(ov[has]), inner)


def unique_rows_match(ik, iv, ok, ov, gk, go, gi):
    """rows of a first-match join: (key, outer_val) is exactly the probe rows with a partner (as a multiset), and every row's
    inner_val is the payload of one of its key's copies"""
    has = np.isin(ok, ik)
    if len(gk) != int(has.sum()):
        return False
    if not np.array_equal(np.sort(pairs(gk, go)), np.sort(pairs(ok[has], ov[has]))):
        return False
    return bool(np.isin(pairs(gk, gi), pairs(ik, iv)).all())


def brute_force(ik, iv, ok, ov):
    """the join by a double loop: (aggregates, sorted rows); for inputs of a few hundred rows"""
    rows = [(int(k), int(o), int(i)) for k, o in zip(ok, ov) for kk, i in zip(ik, iv) if int(kk) == int(k)]
    rows.sort()
    agg = (len(rows), sum(r[0] for r in rows) & M64, sum(r[1] for r in rows) & M64, sum(r[2] for r in rows) & M64)
    return agg, rows


def brute_force_unique(ik, iv, ok, ov):
    """(count, sum_keys, sum_outer_vals) of the first-match join and, per probe row with a partner, the payloads it may report"""
    hits = [(int(k), int(o), sorted(int(i) for kk, i in zip(ik, iv) if int(kk) == int(k))) for k, o in zip(ok, ov)]
    hits = [h for h in hits if h[2]]
    return (len(hits), sum(h[0] for h in hits) & M64, sum(h[1] for h in hits) & M64), hits


# ---- hjgpu_join_partitions: the named cases -------------------------------------------------------------------------
F_ONE, F_TWO = 0x2545F491, 0x27D4EB2F          # odd, and not the library's defaults


class JoinCase:
    """co-partitioned columns, their layout, and what the case is named for (`props`, asserted by tests/test_operator_cases.py)"""

    def __init__(self, name, lay, build_parts, probe_parts, lead=0, unique=False, **props):
        self.name, self.lay, self.lead, self.unique, self.props = name, lay, lead, unique, props
        self.build_parts, self.probe_parts = build_parts, probe_parts
        self.rk, self.rv, self.sk, self.sv, self.roff, self.soff = co_partitioned(build_parts, probe_parts, lead, lead)

    def real(self):
        """the real rows: (ik, iv, ok, ov)"""
        r, s = self.roff.astype(np.int64), self.soff.astype(np.int64)
        return self.rk[r[0]:r[-1]], self.rv[r[0]:r[-1]], self.sk[s[0]:s[-1]], self.sv[s[0]:s[-1]]

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """(aggregates, sorted rows) of the inner join of the real rows"""
        ik, iv, ok, ov = self.real()
        return numpy_join(ik, iv, ok, ov), materialised_rows(ik, iv, ok, ov)

    @functools.lru_cache(maxsize=None)
    def unique_reference(self):
        return unique_reference(*self.real())


def _vals(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def _build_unique(q, n, lay, rng):
    return keys_in_partition(q, n, *lay.args(), rng=rng), _vals(rng, n)


def _probe_of(build_keys, q, hits, misses, lay, rng):
    """`hits` probe rows drawn from build_keys (with repeats) and `misses` rows of partition q that carry no build key, shuffled"""
    k = np.zeros(0, np.uint32)
    if hits and len(build_keys):
        k = build_keys[rng.integers(0, len(build_keys), size=hits)]
    if misses:
        m = keys_in_partition(q, misses + 8, *lay.args(), rng=rng)
        m = m[~np.isin(m, build_keys)][:misses]
        assert len(m) == misses
        k = np.concatenate([k, m])
    k = k[rng.permutation(len(k))]
    return k.astype(np.uint32), _vals(rng, len(k))


def _handful(lay, rng, skip=(), build=(3, 9), probe=(5, 40)):
    """small partitions everywhere but at `skip`: a few build rows, a few probe rows, hits and misses"""
    bp, pp = [None] * lay.P, [None] * lay.P
    for q in range(lay.P):
        if q in skip:
            continue
        nb = int(rng.integers(*build))
        bp[q] = _build_unique(q, nb, lay, rng)
        ns = int(rng.integers(*probe))
        pp[q] = _probe_of(bp[q][0], q, ns - ns // 4, ns // 4, lay, rng)
    return bp, pp


def _case_p2():
    rng = np.random.default_rng(201)
    lay = Layout(F_ONE, 2)
    bp, pp = _handful(lay, rng)
    return JoinCase("p2_minimum", lay, bp, pp, partitions=2)


SMALL_SIZES_R = [0] + [(3 * p + p // 6) % 6 for p in range(1, 34)] + [0]
SMALL_SIZES_S = [0] + [(5 * p + 1) % 6 for p in range(1, 33)] + [5, 0]        # 85 probe rows: no multiple of 4


def _case_small_5x7():
    """partitions of 0 ... 5 rows on either side, the first and the last empty, every start residue modulo 4"""
    rng = np.random.default_rng(202)
    lay = Layout(F_ONE, 5, F_TWO, 7)
    bp, pp = [], []
    for q in range(lay.P):
        b = _build_unique(q, SMALL_SIZES_R[q], lay, rng)
        ns = SMALL_SIZES_S[q]
        hits = (ns + 1) // 2 if len(b[0]) else 0
        bp.append(b)
        pp.append(_probe_of(b[0], q, hits, ns - hits, lay, rng))
    return JoinCase("sizes_0_to_5_at_5x7", lay, bp, pp, small_sizes=True, residues=True)


def _case_p32768():
    rng = np.random.default_rng(203)
    lay = Layout(F_ONE, 1024, F_TWO, 32)
    n = 3 * lay.P
    ik = np.unique(rng.integers(0, 1 << 32, size=n + n // 8, dtype=np.uint64).astype(np.uint32))
    ik = ik[rng.permutation(len(ik))][:n]
    ok = np.concatenate([ik[rng.integers(0, n, size=n)], rng.integers(0, 1 << 32, size=n // 2 + 3, dtype=np.uint64).astype(np.uint32)])
    return JoinCase("p32768_three_rows_each", lay, split_parts(ik, _vals(rng, len(ik)), lay), split_parts(ok, _vals(rng, len(ok)), lay),
                    partitions=32768, residues=True)


def _case_lead(lead):
    """offsets that start at `lead` and end `lead` rows before the columns do; poison rows on both ends of both sides"""
    rng = np.random.default_rng(210 + lead)
    lay = Layout(F_ONE, 5, F_TWO, 7)
    bp, pp = [], []
    for q in range(lay.P):
        k, v = _build_unique(q, int(rng.integers(20, 60)), lay, rng)
        k, v = np.concatenate([k, k[:7]]), np.concatenate([v, _vals(rng, 7)])        # seven keys twice
        bp.append((k, v))
        pp.append(_probe_of(k, q, int(rng.integers(60, 150)), int(rng.integers(5, 40)), lay, rng))
    return JoinCase("lead_%d" % lead, lay, bp, pp, lead=lead, poison=True)


def _case_slices(rows):
    """one probe partition of `rows` rows beside partitions with a handful"""
    rng = np.random.default_rng(220 + rows % 1000)
    lay = Layout(F_ONE, 3)
    bp, pp = _handful(lay, rng, skip=(1,))
    bp[1] = _build_unique(1, 600, lay, rng)
    pp[1] = _probe_of(bp[1][0], 1, rows - rows // 8, rows // 8, lay, rng)
    return JoinCase("probe_rows_%d" % rows, lay, bp, pp, slices=(1, (rows + JOIN_SLICE - 1) // JOIN_SLICE), probe_rows=(1, rows))


def _case_fills(rows, probe_rows=3000):
    """one build partition of `rows` unique keys beside partitions with a handful"""
    rng = np.random.default_rng(230 + rows % 1000)
    lay = Layout(F_ONE, 3)
    bp, pp = _handful(lay, rng, skip=(1,))
    bp[1] = _build_unique(1, rows, lay, rng)
    pp[1] = _probe_of(bp[1][0], 1, probe_rows - probe_rows // 8, probe_rows // 8, lay, rng)
    props = dict(fills=(1, (rows + FILL_ROWS - 1) // FILL_ROWS), build_rows=(1, rows), unique_build_keys=True)
    if probe_rows > JOIN_SLICE:
        props["slices"] = (1, (probe_rows + JOIN_SLICE - 1) // JOIN_SLICE)
    return JoinCase("build_rows_%d" % rows, lay, bp, pp, **props)


def _case_chained():
    """a partition whose keys come in 3, 16 and 5000 copies: the cuckoo build fails (a key has two slots) and the fill falls back to its
    chained table; the key of 5000 copies spans two fills"""
    rng = np.random.default_rng(240)
    lay = Layout(F_ONE, 3)
    bp, pp = _handful(lay, rng, skip=(2,))
    keys = keys_in_partition(2, 40 + 10 + 1, *lay.args(), rng=rng)
    k = np.concatenate([np.repeat(keys[:40], 3), np.repeat(keys[40:50], 16), np.repeat(keys[50:], 5000)])
    bp[2] = (k, _vals(rng, len(k)))
    pk, pv = _probe_of(keys[:50], 2, 150, 30, lay, rng)
    pp[2] = (np.concatenate([pk, keys, keys[50:]]), np.concatenate([pv, _vals(rng, len(keys) + 1)]))      # every key; the heavy one twice
    return JoinCase("chained_3_16_5000_copies", lay, bp, pp, chained=(2, 3), fills=(2, 2), copies=(3, 16, 5000))


def _case_first_match(shared):
    """first match, single-fill partitions: 2 copies per key in partition 0, 16 in partition 1"""
    rng = np.random.default_rng(250 + shared)
    lay = Layout(F_ONE, 3)
    bp, pp = _handful(lay, rng, skip=(0, 1))
    for q, keys, copies in ((0, 500, 2), (1, 100, 16)):
        d = keys_in_partition(q, keys, *lay.args(), rng=rng)
        k = np.tile(d, copies)
        v = np.tile(_vals(rng, keys), copies) if shared else _vals(rng, len(k))
        bp[q] = (k, v)
        pp[q] = _probe_of(d, q, 3000, 400, lay, rng)
    return JoinCase("first_match_2_and_16_copies_%s" % ("one_payload" if shared else "own_payloads"), lay, bp, pp, unique=True,
                    copies=(2, 16), single_fill=(0, 1), shared=shared)


def _case_first_match_two_fills(probe_rows):
    """first match, a partition of 8193 build rows in which every key has one copy in each of two fills (one key: in each of all three):
    a row reported by the first fill must be skipped by the later ones"""
    rng = np.random.default_rng(260 + probe_rows % 1000)
    lay = Layout(F_ONE, 3)
    bp, pp = _handful(lay, rng, skip=(1,))
    d = keys_in_partition(1, FILL_ROWS, *lay.args(), rng=rng)
    k = np.concatenate([d, d[rng.permutation(FILL_ROWS)], d[:1]])
    bp[1] = (k, _vals(rng, len(k)))
    pp[1] = _probe_of(d, 1, probe_rows - probe_rows // 8, probe_rows // 8, lay, rng)
    return JoinCase("first_match_two_fills_probe_%d" % probe_rows, lay, bp, pp, unique=True, fills=(1, 3), build_rows=(1, 2 * FILL_ROWS + 1),
                    one_copy_per_fill=1, probe_rows=(1, probe_rows), slices=(1, (probe_rows + JOIN_SLICE - 1) // JOIN_SLICE))


EDGE_KEYS = np.concatenate([np.arange(64, dtype=np.uint32), np.array([0xFFFFFFFE, 0xFFFFFFFF], np.uint32)])


def _case_key_values(two_level):
    """the keys next to every partition's empty sentinel (the smallest value that does not hash to it): 0, 1 ... 63, 0xFFFFFFFE,
    0xFFFFFFFF on both sides, payloads 0 and 0xFFFFFFFF"""
    lay = Layout(0x01000193, 7, 0x7FFFFFFF, 9) if two_level else Layout(0xDEADBEEF, 11)
    ik = EDGE_KEYS.copy()
    iv = np.where(np.arange(len(ik)) % 2 == 0, 0, M32).astype(np.uint32)
    ok = np.concatenate([EDGE_KEYS, EDGE_KEYS[::-1], np.arange(64, 128, dtype=np.uint32), np.array([0xFFFFFFFD], np.uint32)])
    ov = np.where(np.arange(len(ok)) % 3 == 0, M32, 0).astype(np.uint32)
    return JoinCase("key_values_%s" % ("two_level" if two_level else "one_level"), lay, split_parts(ik, iv, lay), split_parts(ok, ov, lay),
                    edge_keys=True)


JOIN_BUILDERS = {
    "p2_minimum": _case_p2,
    "sizes_0_to_5_at_5x7": _case_small_5x7,
    "p32768_three_rows_each": _case_p32768,
    "lead_1": lambda: _case_lead(1),
    "lead_37": lambda: _case_lead(37),
    "lead_4099": lambda: _case_lead(4099),
    "probe_rows_65535": lambda: _case_slices(65535),
    "probe_rows_65536": lambda: _case_slices(65536),
    "probe_rows_65537": lambda: _case_slices(65537),
    "probe_rows_131073": lambda: _case_slices(131073),
    "build_rows_4096": lambda: _case_fills(4096),
    "build_rows_4097": lambda: _case_fills(4097),
    "build_rows_8193": lambda: _case_fills(8193),
    "build_rows_262145": lambda: _case_fills(FILL_GROUPS * FILL_ROWS + 1, 70_000),
    "chained_3_16_5000_copies": _case_chained,
    "key_values_one_level": lambda: _case_key_values(False),
    "key_values_two_level": lambda: _case_key_values(True),
    "first_match_2_and_16_copies_one_payload": lambda: _case_first_match(True),
    "first_match_2_and_16_copies_own_payloads": lambda: _case_first_match(False),
    "first_match_two_fills_probe_65536": lambda: _case_first_match_two_fills(65536),
    "first_match_two_fills_probe_65537": lambda: _case_first_match_two_fills(65537),
}
INNER_CASES = [n for n in JOIN_BUILDERS if not n.startswith("first_match")]
FIRST_MATCH_CASES = [n for n in JOIN_BUILDERS if n.startswith("first_match")]
# the unique-key partitions that run again under option "force_chained"
FORCE_CHAINED_CASES = ["sizes_0_to_5_at_5x7", "lead_37", "build_rows_4097", "key_values_two_level"]


@functools.lru_cache(maxsize=None)
def join_case(name):
    case = JOIN_BUILDERS[name]()
    assert case.name == name
    return case


@functools.lru_cache(maxsize=None)
def three_ways_relations():
    """unpartitioned relations with duplicates on both sides and misses: partitioned three ways by the GPU test"""
    rng = np.random.default_rng(270)
    d = np.unique(rng.integers(0, 1 << 32, size=21_000, dtype=np.uint64).astype(np.uint32))[:20_000]
    d = d[rng.permutation(len(d))]
    ik = np.concatenate([d, d[:3000], d[:500]])                        # 500 keys three times, 2500 twice
    ik = ik[rng.permutation(len(ik))]
    ok = np.concatenate([d[rng.integers(0, len(d), size=90_000)], rng.integers(0, 1 << 32, size=10_001, dtype=np.uint64).astype(np.uint32)])
    ok = ok[rng.permutation(len(ok))]
    return ik, _vals(rng, len(ik)), ok, _vals(rng, len(ok))


# ---- the partition operators at their seams -------------------------------------------------------------------------
COLUMN_FANOUTS = (1, 2, 1023, 1024)
PACKED_FANOUTS = (216, 217, 436, 437, 660, 661, 1024)
COUNTED_FANOUTS = ((217, 151), (661, 49), (1024, 32))
DISTRIBUTIONS = ("uniform", "hot_at_threshold", "hot_over_threshold", "hot_alternating", "heavy_runs", "sorted", "all_in_first", "all_in_last")
F_PART, F_PART2 = 0x2C1B3C6D, 0x297A2D39


def seam_rows(tile):
    return (tile - 1, tile, tile + 1, 2 * tile + 17)


def own_ranges(fanout):
    """(own_first, own_count): first, middle, last, all, empty"""
    k = max(1, fanout // 8)
    return ((0, k), (fanout // 2, min(k, fanout - fanout // 2)), (fanout - k, k), (0, fanout), (fanout // 3, 0))


def heavy_partitions(tile, fanout):
    """partitions of the "heavy_runs" distribution: 60 of about 270 rows per tile at the largest tile, fewer at the smaller tiles so that
    every run stays longer than STREAM_UNIT"""
    return max(1, min(60, tile // 270, fanout))


def _tile_keys(counts, factor, fanout, rng):
    """counts: {partition: rows}; the keys, shuffled"""
    k = [keys_in_partition(p, c, factor, fanout, rng=rng, distinct=False) for p, c in counts.items() if c]
    k = np.concatenate(k + [np.zeros(0, np.uint32)])
    return k[rng.permutation(len(k))]


def _uniform_except(n, factor, fanout, banned, rng):
    """n uniform keys that avoid the partitions in `banned` (all of them, when the fan-out has no other partition)"""
    if n <= 0:
        return np.zeros(0, np.uint32)
    if fanout <= len(banned):
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    out = np.zeros(0, np.uint32)
    while len(out) < n:
        k = rng.integers(0, 1 << 32, size=2 * (n - len(out)) + 16, dtype=np.uint64).astype(np.uint32)
        out = np.concatenate([out, k[~np.isin(mulhi_hash(k, factor, fanout), list(banned))]])
    return out[:n]


@functools.lru_cache(maxsize=None)
def partition_input(dist, n, fanout, tile, factor=F_PART):
    """(keys, payloads) of n rows; the distributions are laid out tile by tile (rows [t * tile, (t + 1) * tile))"""
    rng = np.random.default_rng([DISTRIBUTIONS.index(dist), n, fanout, tile])
    hot = (fanout // 3, (2 * fanout) // 3 if fanout > 1 else 0)
    chunks = []
    for t, beg in enumerate(range(0, n, tile)):
        rows = min(tile, n - beg)
        if dist in ("uniform", "sorted"):
            k = rng.integers(0, 1 << 32, size=rows, dtype=np.uint64).astype(np.uint32)
        elif dist in ("hot_at_threshold", "hot_over_threshold", "hot_alternating"):
            h = min(rows, tile // HOT_SHARE + (0 if dist == "hot_at_threshold" else 1))
            p = hot[t & 1] if dist == "hot_alternating" else hot[0]
            k = np.concatenate([keys_in_partition(p, h, factor, fanout, rng=rng, distinct=False),
                                _uniform_except(rows - h, factor, fanout, set(hot), rng)])
            k = k[rng.permutation(rows)]
        elif dist == "heavy_runs":
            parts = heavy_partitions(tile, fanout)
            which = (np.arange(parts) * max(1, fanout // parts)) % fanout
            per = np.full(parts, rows // parts)
            per[:rows - per.sum()] += 1
            k = _tile_keys(dict(zip(which.tolist(), per.tolist())), factor, fanout, rng)
        elif dist == "all_in_first":
            k = keys_in_partition(0, rows, factor, fanout, rng=rng, distinct=False)
        elif dist == "all_in_last":
            k = keys_in_partition(fanout - 1, rows, factor, fanout, rng=rng, distinct=False)
        else:
            raise KeyError(dist)
        chunks.append(k.astype(np.uint32))
    keys = np.concatenate(chunks)
    if dist == "sorted":
        keys = keys[np.argsort(mulhi_hash(keys, factor, fanout), kind="stable")]
    assert len(keys) == n
    return keys, np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(7)


def partition_reference(keys, fanout, factor=F_PART, own_first=0, own_count=0):
    """(offsets, first): offsets = the prefix of the counts (fanout + 1), first[p] = where partition p begins when the partitions
    [own_first, own_first + own_count) are laid out last (include/hjgpu.h, hjgpu_partition_packed_own_last_async)"""
    n = len(keys)
    off = np.concatenate([[0], np.cumsum(np.bincount(mulhi_hash(keys, factor, fanout), minlength=fanout))]).astype(np.int64)
    own_rows = off[own_first + own_count] - off[own_first]
    p = np.arange(fanout)
    first = np.where(p < own_first, off[:-1], np.where(p < own_first + own_count, n - own_rows + off[:-1] - off[own_first], off[:-1] - own_rows))
    return off, first.astype(np.int64)


def expected_partition_of_rows(off, first):
    """for every output row, the partition whose rows it belongs to"""
    want = np.full(int(off[-1]), -1, np.int64)
    for p in np.nonzero(np.diff(off))[0]:
        want[first[p]:first[p] + off[p + 1] - off[p]] = p
    return want


def counts2_reference(keys, fanout, fanout2, factor=F_PART, factor2=F_PART2):
    bins = mulhi_hash(keys, factor, fanout) * fanout2 + mulhi_hash(keys, factor2, fanout2)
    return np.bincount(bins, minlength=fanout * fanout2).astype(np.uint64)


# ---- hjgpu_npj_build / hjgpu_npj_probe ------------------------------------------------------------------------------
NPJ_ROWS = (1, 7, 4096)
NPJ_COPIES = {1: (1,), 7: (1, 2), 4096: (1, 2, 40)}
F_NPJ = 0x9E3779B1


@functools.lru_cache(maxsize=None)
def npj_case(n):
    """(ik, iv, ok, ov) for a table of n + 1 buckets: n build rows (no key 0) whose keys come in NPJ_COPIES[n] copies; the probe side hits
    every build key, misses, and carries a key 0"""
    rng = np.random.default_rng(300 + n)
    pool = np.unique(rng.integers(1, 1 << 32, size=2 * n + 64, dtype=np.uint64).astype(np.uint32))
    pool = pool[rng.permutation(len(pool))]
    if n == 1:
        ik = pool[:1]
    elif n == 7:
        ik = np.concatenate([np.repeat(pool[:2], 2), pool[2:5]])
    else:
        ik = np.concatenate([np.repeat(pool[:10], 40), np.repeat(pool[10:110], 2)])
        ik = np.concatenate([ik, pool[110:110 + n - len(ik)]])
    assert len(ik) == n
    ik = ik[rng.permutation(n)]
    d = np.unique(ik)
    miss = pool[len(pool) - (n // 2 + 3):]
    assert not np.isin(miss, ik).any()
    ok = np.concatenate([d, d[rng.integers(0, len(d), size=n + 2)], miss, np.zeros(1, np.uint32)])
    ok = ok[rng.permutation(len(ok))]
    return ik, _vals(rng, n), ok, _vals(rng, len(ok))
