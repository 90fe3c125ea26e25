"""Host model of the claimed probe side of a blocking two-pass hjgpu_phj (test infrastructure, numpy only, so that
tests/test_claimed_model.py can check it on a machine without a GPU): what every join mode of include/hjgpu.h must return, which
optimistic region every probe row goes to, and whether a probe side fits its regions.  tests/test_gpu_claimed_modes.py runs the inputs
at the end of this file on the claimed road, on the build-beside form and on the exact path.

The join modes are written from the header's text (HJGPU_FLAG_*), not from the kernels.  The regions are the header's option
"probe_slack" and DESIGN.md section 3 "Claimed probe side": pass 1 gives partition p of fanout1 a region of cap1 tuples, pass 2 gives
final partition q of fanout1 * fanout2 a region of cap2 tuples; a region holds its rows and nothing else (whole 16-tuple lines from the
front, tails from the back), so a probe side stays on the road exactly when no region gets more rows than its cap."""
import functools
import math

import numpy as np

from helpers import mulhi_hash, pairs
from operator_cases import Layout, keys_in_partition

# include/hjgpu.h (tests/test_claimed_model.py compares these with the header's text)
UNIQUE, SEMI, ANTI, LEFT_OUTER, RIGHT_OUTER, RIGHT_SEMI, RIGHT_ANTI = 1, 2, 4, 8, 16, 32, 64
INNER, FULL_OUTER = 0, LEFT_OUTER | RIGHT_OUTER
NULL_VAL = 0xFFFFFFFF
MODES = (INNER, SEMI, ANTI, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER, RIGHT_SEMI, RIGHT_ANTI)
MODE_NAMES = {INNER: "inner", SEMI: "semi", ANTI: "anti", LEFT_OUTER: "left_outer", RIGHT_OUTER: "right_outer", FULL_OUTER: "full_outer",
              RIGHT_SEMI: "right_semi", RIGHT_ANTI: "right_anti", UNIQUE: "unique", LEFT_OUTER | UNIQUE: "left_outer_unique"}
# the ten flag sets of a whole join: the eight modes, and the two first-match forms that are not refused
FLAG_SETS = MODES + (UNIQUE, LEFT_OUTER | UNIQUE)
# the library's default pass factors (hjgpu_phj_params::factor1 / factor2 = 0; csrc/hjgpu_ctx.hpp, compared by tests/test_claimed_model.py)
FACTOR1, FACTOR2 = 0x9E3779B1, 0x85EBCA6B
LINE = 16               # tuples of a 128-byte line
DEFAULT_SLACK = 12      # option "probe_slack"
M64 = (1 << 64) - 1


def _sum(a):
    return int(np.asarray(a).astype(np.uint64).sum(dtype=np.uint64)) & M64


def _u32(a):
    return np.asarray(a, dtype=np.uint32)


def sorted_rows(*cols):
    """rows sorted lexicographically, the first column the most significant"""
    idx = np.lexsort(tuple(reversed(cols)))
    return tuple(c[idx] for c in cols)


# ---- the join modes -------------------------------------------------------------------------------------------------
def _matches(ik, iv, ok, ov):
    """every pair (probe tuple, build tuple) of equal keys, unsorted: (key, outer_val, inner_val)"""
    order = np.argsort(ik, kind="stable")
    sk, sv = ik[order], iv[order]
    lo, hi = np.searchsorted(sk, ok, side="left"), np.searchsorted(sk, ok, side="right")
    mult = hi - lo
    probe = np.repeat(np.arange(len(ok)), mult)
    within = np.arange(len(probe)) - np.repeat(np.cumsum(mult) - mult, mult)
    return ok[probe], ov[probe], sv[np.repeat(lo, mult) + within]


def join_reference(mode, ik, iv, ok, ov):
    """((count, sum_keys, sum_outer_vals, sum_inner_vals), sorted rows) of a join mode of include/hjgpu.h (no HJGPU_FLAG_UNIQUE).
    Rows: (keys, outer_vals, inner_vals); semi- and anti-joins (keys, outer_vals); right semi- and anti-joins (keys, inner_vals).
    A NULL row carries HJGPU_NULL_VAL on the side without a match, and that side's sum skips it."""
    ik, iv, ok, ov = _u32(ik), _u32(iv), _u32(ok), _u32(ov)
    assert mode in MODES, mode
    has_build = np.isin(ok, ik)          # probe tuples whose key equals at least one build key
    has_probe = np.isin(ik, ok)          # build tuples whose key equals at least one probe key
    if mode in (SEMI, ANTI):
        sel = has_build if mode == SEMI else ~has_build
        k, o = ok[sel], ov[sel]
        return (len(k), _sum(k), _sum(o), 0), sorted_rows(k, o)
    if mode in (RIGHT_SEMI, RIGHT_ANTI):
        sel = has_probe if mode == RIGHT_SEMI else ~has_probe
        k, i = ik[sel], iv[sel]
        return (len(k), _sum(k), 0, _sum(i)), sorted_rows(k, i)
    k, o, i = _matches(ik, iv, ok, ov)
    sum_outer, sum_inner = _sum(o), _sum(i)              # the matched rows' payloads: a NULL adds 0 to its side's sum
    if mode & LEFT_OUTER:
        n = int((~has_build).sum())
        k = np.concatenate([k, ok[~has_build]])
        o = np.concatenate([o, ov[~has_build]])
        i = np.concatenate([i, np.full(n, NULL_VAL, np.uint32)])
        sum_outer = (sum_outer + _sum(ov[~has_build])) & M64
    if mode & RIGHT_OUTER:
        n = int((~has_probe).sum())
        k = np.concatenate([k, ik[~has_probe]])
        o = np.concatenate([o, np.full(n, NULL_VAL, np.uint32)])
        i = np.concatenate([i, iv[~has_probe]])
        sum_inner = (sum_inner + _sum(iv[~has_probe])) & M64
    return (len(k), _sum(k), sum_outer, sum_inner), sorted_rows(k, o, i)


def first_match_errors(mode, ik, iv, ok, ov, res, rows=None):
    """HJGPU_FLAG_UNIQUE (mode INNER) and HJGPU_FLAG_LEFT_OUTER | HJGPU_FLAG_UNIQUE (mode LEFT_OUTER) over duplicated build keys: which copy
    of a key answers is unspecified, everything else is not.  Returns what is wrong with the aggregates `res` and the rows (keys,
    outer_vals, inner_vals, any order; None: aggregates only) - an empty list when nothing is:
      one row per probe tuple with a match (left outer: per probe tuple, its NULL row when it has none);
      a matched row's inner value is one of its key's build payloads;
      count, sum_keys and sum_outer_vals are those rows', sum_inner_vals the sum of the matched rows' inner values - without rows, a sum
      between what the smallest and the largest payload of every matched key would give.
    Build payloads must not be HJGPU_NULL_VAL under LEFT_OUTER: a row could not tell it from a NULL."""
    ik, iv, ok, ov = _u32(ik), _u32(iv), _u32(ok), _u32(ov)
    assert mode in (INNER, LEFT_OUTER), mode
    left = mode == LEFT_OUTER
    assert not left or not np.any(iv == NULL_VAL)
    has = np.isin(ok, ik)
    rep = np.ones(len(ok), bool) if left else has                # the reported probe tuples
    bad = []
    if tuple(res[:3]) != (int(rep.sum()), _sum(ok[rep]), _sum(ov[rep])):
        bad.append("count / sum_keys / sum_outer_vals %r, wanted %r" % (tuple(res[:3]), (int(rep.sum()), _sum(ok[rep]), _sum(ov[rep]))))
    if rows is None:
        order = np.lexsort((iv, ik))
        sk, sv = ik[order], iv[order]
        lo, hi = np.searchsorted(sk, ok[has], side="left"), np.searchsorted(sk, ok[has], side="right") - 1
        least, most = int(sv[lo].astype(np.uint64).sum()), int(sv[hi].astype(np.uint64).sum())      # (far below 2^64 at a test's sizes)
        assert most < 1 << 64
        if not least <= res[3] <= most:
            bad.append("sum_inner_vals %d outside [%d, %d]" % (res[3], least, most))
        return bad
    k, o, i = (_u32(c) for c in rows)
    if not (len(k) == len(o) == len(i) == int(rep.sum())):
        return bad + ["%d rows, wanted %d" % (len(k), int(rep.sum()))]
    if not np.array_equal(np.sort(pairs(k, o)), np.sort(pairs(ok[rep], ov[rep]))):
        bad.append("(key, outer_val) is not the reported probe tuples")
    null = ~np.isin(k, ik)                                        # rows of probe tuples without a match: none unless left outer
    if np.any(i[null] != NULL_VAL):
        bad.append("a row without a match carries an inner value")
    if not np.isin(pairs(k[~null], i[~null]), pairs(ik, iv)).all():
        bad.append("an inner value is no payload of its key")
    if res[3] != _sum(i[~null]):
        bad.append("sum_inner_vals %d, the rows give %d" % (res[3], _sum(i[~null])))
    return bad


# ---- the optimistic regions -----------------------------------------------------------------------------------------
def claimed_cap(mean, slack):
    """the tuples of a region for `mean` rows: the mean, with slack > 0 plus slack per cent of it, 8 sigma (sigma = the square root of
    the mean) and 64 rows, in whole 16-tuple lines; slack 0: the mean alone, in whole lines"""
    c = int(mean)
    if slack > 0:
        c += int(mean) * int(slack) // 100 + int(8.0 * math.sqrt(float(mean))) + 64
    return (c + LINE - 1) // LINE * LINE


def region_caps(outer, F1, F2, slack=DEFAULT_SLACK):
    """(cap1, cap2): the tuples of a pass-1 region and of a final region"""
    return claimed_cap(outer // F1, slack), claimed_cap(outer // (F1 * F2), slack)


def region_rows(ok, F1, F2, f1=FACTOR1, f2=FACTOR2):
    """(rows of every pass-1 region, rows of every final region) of the probe keys `ok`"""
    ok = _u32(ok)
    lay = Layout(f1, F1, f2, F2)
    return (np.bincount(mulhi_hash(ok, f1, F1), minlength=F1).astype(np.int64), np.bincount(lay.pid(ok), minlength=lay.P).astype(np.int64))


def fits(ok, F1, F2, slack=DEFAULT_SLACK, f1=FACTOR1, f2=FACTOR2):
    """does every region hold its rows?  (then the join stays on the claimed road; else a region is full and the join falls back)"""
    cap1, cap2 = region_caps(len(ok), F1, F2, slack)
    rows1, rows2 = region_rows(ok, F1, F2, f1, f2)
    return bool(rows1.max(initial=0) <= cap1 and rows2.max(initial=0) <= cap2)


# ---- inputs of tests/test_gpu_claimed_modes.py ----------------------------------------------------------------------
# Built once and never written to.  Probe-side duplicates stay at about 40 copies per key and below: one key in a thousand probe rows
# would overflow a region, which is a legitimate fallback and not what these inputs are for.
F1, F2 = 16, 8                          # the default fan-outs: P = 128, 16 384-tuple tiles in both passes
OUTER = 200_003
FILL_ROWS = 4096                        # build rows of one LDS table fill (operator_cases.FILL_ROWS)
BUILD_SHAPES = ("unique", "triple", "hot_20000", "sparse_50", "long_build")


def _vals(rng, n, top=NULL_VAL):
    """payloads below `top`"""
    return rng.integers(0, top, size=n, dtype=np.uint64).astype(np.uint32)


def _pool(rng, n):
    """n distinct keys in random order, none of them 0 or 0xFFFFFFFF"""
    p = np.unique(rng.integers(1, NULL_VAL, size=n + n // 4 + 64, dtype=np.uint64).astype(np.uint32))
    assert len(p) >= n
    return p[rng.permutation(len(p))][:n]


def _probe(rng, outer, hit_keys, hits, miss_keys, even=True):
    """`hits` rows of hit_keys - dealt evenly (every key hits / len(hit_keys) times, give or take one) or drawn at random -, the others
    drawn from miss_keys, shuffled"""
    hit = np.resize(hit_keys, hits) if even else hit_keys[rng.integers(0, len(hit_keys), size=hits)]
    k = np.concatenate([hit, miss_keys[rng.integers(0, len(miss_keys), size=outer - hits)]])
    return k[rng.permutation(outer)].astype(np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def uniform_probe(outer=OUTER, pool=60_000, seed=7):
    """`outer` probe keys drawn uniformly from a pool of distinct keys (3.3 copies of a key on average at the default sizes), and the pool"""
    rng = np.random.default_rng([seed, outer, pool])
    keys = _pool(rng, pool)
    return _frozen(keys[rng.integers(0, pool, size=outer)].astype(np.uint32), keys)


@functools.lru_cache(maxsize=None)
def mode_case(shape):
    """(ik, iv, ok, ov) of a build shape at fan-outs 16 x 8; about half of the probe rows match unless the shape says otherwise.  No
    payload is 0xFFFFFFFF (mode_relations puts some where the header allows them).
      unique      5 003 unique build keys, 4 002 of them probed by 25 rows each; keys 0 and 0xFFFFFFFF on both sides; 200 003 probe rows
      triple      the same keys three times each, every copy with a payload of its own: the cuckoo build fails, the tables are chained
      hot_20000   unique's build side, 200 further keys of one final partition and 20 000 copies of one more key of it: 5 fills of 4 096
                  rows there.  The hot key is probed by 7 rows; the partition's other probe rows find their partner in
                  whatever fill it lies in, and 100 added ones (beside the partition's own misses) have none
      sparse_50   50 build rows over 128 partitions: most have none.  40 of the keys are probed by 30 rows each, no other probe row matches
      long_build  300 000 unique build keys against 20 011 probe rows: the probe side's passes end long before the build side's"""
    assert shape in BUILD_SHAPES, shape
    # (25 copies of a matched key make the final regions uneven: the seed is one whose worst final region, counted by region_rows, stays
    # 200 rows below its cap of 2 144; tests/test_claimed_model.py asserts the room)
    rng = np.random.default_rng([19, BUILD_SHAPES.index(shape)])
    if shape == "long_build":
        keys = _pool(rng, 330_000)
        ik, miss = keys[:300_000], keys[300_000:]
        ok = _probe(rng, 20_011, ik, 10_000, miss, even=False)
        return _frozen(ik.copy(), _vals(rng, len(ik)), ok, _vals(rng, len(ok)))
    if shape == "sparse_50":
        keys = _pool(rng, 60_050)
        ik, miss = keys[:50], keys[50:]
        ok = _probe(rng, OUTER, ik[:40], 1200, miss)
        return _frozen(ik.copy(), _vals(rng, 50), ok, _vals(rng, OUTER))
    keys = _pool(rng, 60_000)
    ik, miss = keys[:5003].copy(), keys[5003:].copy()
    ik[:2] = [0, NULL_VAL]                                  # every key value is legal on both sides
    ok = _probe(rng, OUTER, ik[:4002], OUTER // 2, miss)     # a fifth of the build keys has no probe row
    ok[[3, 70_001]] = [0, NULL_VAL]
    if shape == "triple":
        ik = np.repeat(ik, 3)
        ik = ik[rng.permutation(len(ik))]
    if shape == "hot_20000":
        lay = Layout(FACTOR1, F1, FACTOR2, F2)
        q = int(np.argmin(region_rows(ok, F1, F2)[1]))      # the final partition with the fewest probe rows has room for 307 more
        more = keys_in_partition(q, 400, *lay.args(), rng=rng)
        more = more[~np.isin(more, keys)]
        hot, partners, alone = more[0], more[1:201], more[201:301]
        assert len(alone) == 100
        ik = np.concatenate([ik, partners, np.full(20_000, hot, np.uint32)])
        ik = ik[rng.permutation(len(ik))]
        # 7 rows of the hot key, 1 of every partner, 1 of every key without one - in place of probe rows that had no match
        put = np.concatenate([np.full(7, hot, np.uint32), partners, alone])
        at = np.flatnonzero(~np.isin(ok, ik))[:len(put)]
        ok[at] = put
    return _frozen(ik.astype(np.uint32), _vals(rng, len(ik)), ok, _vals(rng, OUTER))


# the flag sets in which the header calls 0xFFFFFFFF an ordinary build payload (no row of theirs has a NULL to mistake it for)
ALL_ONES_PAYLOAD_OK = (RIGHT_SEMI, RIGHT_ANTI)


@functools.lru_cache(maxsize=None)
def mode_relations(shape, flags):
    """mode_case(shape) for a flag set: right semi- and anti-joins get the payload 0xFFFFFFFF on a matched and on an unmatched build row"""
    ik, iv, ok, ov = mode_case(shape)
    if flags in ALL_ONES_PAYLOAD_OK:
        m = np.isin(ik, ok)
        iv = iv.copy()
        iv[[np.flatnonzero(m)[0], np.flatnonzero(~m)[0]]] = NULL_VAL
        iv.setflags(write=False)
    return ik, iv, ok, ov


@functools.lru_cache(maxsize=None)
def dealt_probe(kind):
    """probe keys dealt to the regions row by row with operator_cases.keys_in_partition, for option "probe_slack" = 0 at 16 x 8:
      full_both    320 rows in every final partition (40 960 rows): cap2 = 320 and cap1 = 2 560 = 8 x 320 - every region of both passes
                   exactly full
      over_pass2   one of those rows moved to the neighbouring final partition of the same pass-1 partition: 321 > 320 there, every
                   pass-1 region still exactly full
      full_pass1   322 rows in every final partition (41 216 rows): cap1 = 2 576 = 8 x 322 exactly full, cap2 = 336 with room
      over_pass1   one of those rows moved to another pass-1 partition: 2 577 > 2 576 there, no final partition above 323"""
    per = {"full_both": 320, "over_pass2": 320, "full_pass1": 322, "over_pass1": 322}[kind]
    lay = Layout(FACTOR1, F1, FACTOR2, F2)
    parts = [keys_in_partition(q, per + 1, *lay.args(), rng=np.random.default_rng([13, q]), distinct=False) for q in range(lay.P)]
    spare = {q: p[per] for q, p in enumerate(parts)}           # one more key of every partition
    ok = np.concatenate([p[:per] for p in parts])
    if kind.startswith("over"):
        src, dst = (5 * F2 + 2, 5 * F2 + 3) if kind == "over_pass2" else (5 * F2 + 2, 9 * F2 + 6)
        ok[src * per] = spare[dst]
    ok = ok[np.random.default_rng(17).permutation(len(ok))].astype(np.uint32)
    return _frozen(ok)[0]


DEALT = ("full_both", "over_pass2", "full_pass1", "over_pass1")


def build_side(ok, inner=3001, seed=19):
    """(ik, iv): `inner` unique build keys - two thirds of them keys of the probe side `ok` (all of its keys when it has fewer), the others
    foreign to it"""
    rng = np.random.default_rng([seed, inner, len(ok)])
    d = np.unique(ok)
    own = d[rng.permutation(len(d))][:min(len(d), 2 * inner // 3)]
    foreign = _pool(rng, inner)
    foreign = foreign[~np.isin(foreign, d)][:inner - len(own)]
    ik = np.concatenate([own, foreign])
    ik = ik[rng.permutation(len(ik))].astype(np.uint32)
    assert len(ik) == inner
    return _frozen(ik, _vals(rng, inner))
