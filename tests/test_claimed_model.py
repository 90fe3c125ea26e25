"""The host model of the claimed probe side (tests/claimed_model.py) against brute force, without a GPU: every join mode against a double
loop written from include/hjgpu.h, the regions against a per-key loop, the constants against the sources they restate, and every input
of tests/test_gpu_claimed_modes.py for the property it is named for."""
import math
import os
import re

import numpy as np
import pytest

import claimed_model as cm
from operator_cases import FILL_ROWS, Layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = 0xFFFFFFFF
M64 = (1 << 64) - 1


def _text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


# ---- the constants ----------------------------------------------------------------------------------------------------
def test_flags_are_the_headers():
    h = _text("include", "hjgpu.h")
    for name, value in (("UNIQUE", cm.UNIQUE), ("SEMI", cm.SEMI), ("ANTI", cm.ANTI), ("LEFT_OUTER", cm.LEFT_OUTER), ("RIGHT_OUTER", cm.RIGHT_OUTER),
                        ("RIGHT_SEMI", cm.RIGHT_SEMI), ("RIGHT_ANTI", cm.RIGHT_ANTI)):
        assert int(re.search(r"#define\s+HJGPU_FLAG_%s\s+(\d+)u" % name, h).group(1)) == value, name
    assert re.search(r"#define\s+HJGPU_FLAG_FULL_OUTER\s+\(HJGPU_FLAG_LEFT_OUTER \| HJGPU_FLAG_RIGHT_OUTER\)", h)
    assert int(re.search(r"#define\s+HJGPU_NULL_VAL\s+0x([0-9A-Fa-f]+)u", h).group(1), 16) == cm.NULL_VAL
    assert len(set(cm.FLAG_SETS)) == 10 and set(cm.FLAG_SETS) == set(cm.MODE_NAMES)


def test_default_factors_slack_and_fill_are_the_librarys():
    c = _text("hash_join_codes_knl_amd", "csrc", "hjgpu_ctx.hpp")
    m = re.search(r"DEFAULT_F1\s*=\s*0x([0-9A-Fa-f]+)u\s*,\s*DEFAULT_F2\s*=\s*0x([0-9A-Fa-f]+)u", c)
    assert (int(m.group(1), 16), int(m.group(2), 16)) == (cm.FACTOR1, cm.FACTOR2)
    t = _text("hash_join_codes_knl_amd", "csrc", "hj_internal.hpp")
    assert int(re.search(r"int\s+probe_slack\s*=\s*(\d+)\s*;", t).group(1)) == cm.DEFAULT_SLACK
    assert cm.FILL_ROWS == FILL_ROWS


# ---- the join modes against a double loop -----------------------------------------------------------------------------
def brute_force(mode, ik, iv, ok, ov):
    """the header's text, row by row: (aggregates, sorted rows as tuples)"""
    R = [(int(k), int(v)) for k, v in zip(ik, iv)]
    S = [(int(k), int(v)) for k, v in zip(ok, ov)]
    rows, so, si = [], 0, 0
    if mode in (cm.SEMI, cm.ANTI):
        for k, o in S:
            if any(k == rk for rk, _ in R) == (mode == cm.SEMI):
                rows.append((k, o)); so += o
    elif mode in (cm.RIGHT_SEMI, cm.RIGHT_ANTI):
        for k, i in R:
            if any(k == sk for sk, _ in S) == (mode == cm.RIGHT_SEMI):
                rows.append((k, i)); si += i
    else:
        for k, o in S:
            partners = [i for rk, i in R if rk == k]
            for i in partners:
                rows.append((k, o, i)); so += o; si += i
            if not partners and mode & cm.LEFT_OUTER:
                rows.append((k, o, NULL)); so += o
        if mode & cm.RIGHT_OUTER:
            for k, i in R:
                if not any(k == sk for sk, _ in S):
                    rows.append((k, NULL, i)); si += i
    rows.sort()
    return (len(rows), sum(r[0] for r in rows) & M64, so & M64, si & M64), rows


def _u32(*values):
    return np.array(values, dtype=np.uint32)


def _small_inputs():
    """at most 40 rows a side: duplicates on both sides, keys 0 and 0xFFFFFFFF, payloads 0 and 0xFFFFFFFF, and either side empty"""
    rng = np.random.default_rng(5)
    keys = _u32(0, NULL, 1, 7, 7, 0x80000000, 12345, 12345, 12345, 99)
    ik = np.concatenate([keys, keys[:4], _u32(555, 556)])
    ok = np.concatenate([keys[rng.integers(0, len(keys), size=30)], _u32(0, NULL, 31337, 31337, 4), _u32(0, NULL)])
    iv = rng.integers(0, 1 << 32, size=len(ik), dtype=np.uint64).astype(np.uint32)
    ov = rng.integers(0, 1 << 32, size=len(ok), dtype=np.uint64).astype(np.uint32)
    iv[:2], ov[:2] = [0, NULL], [NULL, 0]
    e = np.zeros(0, np.uint32)
    assert len(ik) <= 40 and len(ok) <= 40
    return {"duplicates_both_sides": (ik, iv, ok, ov), "no_match": (_u32(1, 2, 2), _u32(5, 6, 7), _u32(3, 3, 0), _u32(8, 9, 10)),
            "empty_build": (e, e, ok, ov), "empty_probe": (ik, iv, e, e), "both_empty": (e, e, e, e),
            "one_row_each": (_u32(NULL), _u32(NULL), _u32(NULL), _u32(0))}


SMALL = _small_inputs()


@pytest.mark.parametrize("name", list(SMALL))
@pytest.mark.parametrize("mode", cm.MODES, ids=[cm.MODE_NAMES[m] for m in cm.MODES])
def test_join_reference_against_brute_force(mode, name):
    ik, iv, ok, ov = SMALL[name]
    agg, rows = cm.join_reference(mode, ik, iv, ok, ov)
    want_agg, want_rows = brute_force(mode, ik, iv, ok, ov)
    assert agg == want_agg
    assert len(rows) == (2 if mode in (cm.SEMI, cm.ANTI, cm.RIGHT_SEMI, cm.RIGHT_ANTI) else 3)
    assert [tuple(int(x) for x in r) for r in zip(*rows)] == want_rows
    assert all(c.dtype == np.uint32 for c in rows)


def test_the_modes_differ_on_the_small_input():
    """no two modes share a result there: a reference that mixed two of them up would not pass the test above"""
    ik, iv, ok, ov = SMALL["duplicates_both_sides"]
    assert len({cm.join_reference(m, ik, iv, ok, ov)[0] for m in cm.MODES}) == len(cm.MODES)


def _first_match_rows(mode, ik, iv, ok, ov, pick):
    """a legal first-match result: every probe tuple gets the copy `pick` chooses among its key's payloads"""
    rows = []
    for k, o in zip(ok, ov):
        partners = sorted(int(i) for rk, i in zip(ik, iv) if rk == k)
        if partners:
            rows.append((int(k), int(o), pick(partners)))
        elif mode == cm.LEFT_OUTER:
            rows.append((int(k), int(o), NULL))
    agg = (len(rows), sum(r[0] for r in rows) & M64, sum(r[1] for r in rows) & M64, sum(r[2] for r in rows if r[2] != NULL) & M64)
    cols = tuple(np.array([r[c] for r in rows], dtype=np.uint32) for c in range(3))
    return agg, cols


@pytest.mark.parametrize("mode", [cm.INNER, cm.LEFT_OUTER])
def test_first_match_checker(mode):
    ik, iv, ok, ov = (a.copy() for a in SMALL["duplicates_both_sides"])
    iv[iv == NULL] = 77
    for pick in (min, max, lambda p: p[len(p) // 2]):
        agg, rows = _first_match_rows(mode, ik, iv, ok, ov, pick)
        assert cm.first_match_errors(mode, ik, iv, ok, ov, agg, rows) == []
        assert cm.first_match_errors(mode, ik, iv, ok, ov, agg) == []
    agg, rows = _first_match_rows(mode, ik, iv, ok, ov, min)
    k, o, i = rows
    # a row too many, a row's payload from another key, a NULL where there is a match, aggregates that are not the rows'
    assert cm.first_match_errors(mode, ik, iv, ok, ov, agg, tuple(np.append(c, c[:1]) for c in rows))
    matched = np.flatnonzero(np.isin(k, ik))
    wrong = i.copy(); wrong[matched[0]] ^= 1
    assert cm.first_match_errors(mode, ik, iv, ok, ov, agg, (k, o, wrong))
    wrong = i.copy(); wrong[matched[0]] = NULL
    assert cm.first_match_errors(mode, ik, iv, ok, ov, agg, (k, o, wrong))
    j = int(np.flatnonzero((k != k[0]) & (o != o[0]))[0])
    swapped = o.copy(); swapped[[0, j]] = swapped[[j, 0]]
    assert cm.first_match_errors(mode, ik, iv, ok, ov, agg, (k, swapped, i))
    for w in range(4):
        off = list(agg); off[w] += 1
        assert cm.first_match_errors(mode, ik, iv, ok, ov, tuple(off), rows), w
    low = list(agg); low[3] = 0
    assert cm.first_match_errors(mode, ik, iv, ok, ov, tuple(low))


# ---- the regions --------------------------------------------------------------------------------------------------------
def test_caps_are_the_written_formula():
    """|S| / F + 12 % + 8 sigma + 64 rows in whole lines; slack 0: the mean in whole lines"""
    assert cm.region_caps(200_003, 16, 8) == (14_960, 2_144)
    assert cm.region_caps(200_003, 436, 2) == (752, 448)
    assert cm.region_caps(40_960, 16, 8, 0) == (2_560, 320)
    assert cm.region_caps(41_216, 16, 8, 0) == (2_576, 336)
    assert cm.region_caps(127, 16, 8, 0) == (16, 0) and cm.region_caps(15, 16, 8, 0) == (0, 0) and cm.region_caps(1, 16, 8) == (64, 64)
    for mean in (0, 1, 15, 16, 17, 1562, 12_500, 54_253):
        assert cm.claimed_cap(mean, 0) == -(-mean // 16) * 16
        c = cm.claimed_cap(mean, 12)
        assert c % 16 == 0 and 0 <= c - (mean + mean * 12 // 100 + math.floor(8 * math.sqrt(mean)) + 64) < 16
    assert cm.claimed_cap(54_253, 12) == 62_704          # the headline's final region


@pytest.mark.parametrize("fan", [(16, 8), (217, 2), (436, 2), (5, 7)])
def test_region_rows_against_a_per_key_loop(fan):
    F1, F2 = fan
    ok = np.concatenate([cm.uniform_probe()[0][:3000], _u32(0, NULL, 1, 0x80000000)])
    rows1, rows2 = cm.region_rows(ok, F1, F2)
    want1, want2 = [0] * F1, [0] * (F1 * F2)
    for k in ok.tolist():
        p1 = (((k * cm.FACTOR1) & 0xFFFFFFFF) * F1) >> 32
        p2 = (((k * cm.FACTOR2) & 0xFFFFFFFF) * F2) >> 32
        want1[p1] += 1
        want2[p1 * F2 + p2] += 1
    assert rows1.tolist() == want1 and rows2.tolist() == want2 and rows1.sum() == rows2.sum() == len(ok)
    cap1, cap2 = cm.region_caps(len(ok), F1, F2)
    assert cm.fits(ok, F1, F2) == (max(want1) <= cap1 and max(want2) <= cap2)
    cap1, cap2 = cm.region_caps(len(ok), F1, F2, 0)
    assert cm.fits(ok, F1, F2, slack=0) == (max(want1) <= cap1 and max(want2) <= cap2)
    assert cm.fits(np.zeros(0, np.uint32), F1, F2, slack=0)


# ---- the GPU tests' inputs ----------------------------------------------------------------------------------------------
def test_uniform_probe_stays_inside_its_regions_at_every_fan_out():
    """the worst region of each shape, as counted on the host when the cases were laid out"""
    ok, pool = cm.uniform_probe()
    assert len(ok) == 200_003 and len(pool) == 60_000 and np.bincount(np.unique(ok, return_inverse=True)[1]).max() <= 40
    for F1, F2 in ((16, 8), (216, 2), (217, 2), (300, 2), (436, 2), (437, 2)):
        assert cm.fits(ok, F1, F2), (F1, F2)
        assert not cm.fits(ok, F1, F2, slack=0)


@pytest.mark.parametrize("shape", cm.BUILD_SHAPES)
def test_mode_cases_are_what_they_are_named_for(shape):
    ik, iv, ok, ov = cm.mode_case(shape)
    assert cm.fits(ok, cm.F1, cm.F2)
    cap1, cap2 = cm.region_caps(len(ok), cm.F1, cm.F2)
    rows1, rows2 = cm.region_rows(ok, cm.F1, cm.F2)
    assert rows1.max() <= cap1 - cap1 // 12 and rows2.max() <= cap2 - cap2 // 12         # well inside: no fallback by a hair
    assert not np.any(iv == NULL) and not any(a.flags.writeable for a in (ik, iv, ok, ov))
    copies = np.bincount(np.unique(ok, return_inverse=True)[1])
    assert copies.max() <= 45, copies.max()
    matched = float(np.isin(ok, ik).mean())
    lay = Layout(cm.FACTOR1, cm.F1, cm.FACTOR2, cm.F2)
    build_rows = np.bincount(lay.pid(ik), minlength=lay.P)
    distinct, per_key = np.unique(ik, return_counts=True)
    if shape == "sparse_50":
        assert len(ik) == 50 and int((build_rows == 0).sum()) > lay.P // 2 and 0 < matched < 0.01
    elif shape == "long_build":
        assert (len(ik), len(ok)) == (300_000, 20_011) and 0.45 < matched < 0.55 and build_rows.max() <= FILL_ROWS
    else:
        assert len(ok) == 200_003 and 0.45 < matched < 0.55
        assert {0, NULL} <= set(ik.tolist()) and {0, NULL} <= set(ok.tolist())
    if shape == "unique":
        assert len(ik) == 5003 and per_key.max() == 1
    if shape == "triple":
        assert len(ik) == 3 * 5003 and per_key.min() == per_key.max() == 3 and build_rows.max() <= FILL_ROWS
        order = np.lexsort((iv, ik))
        assert np.all(np.diff(iv[order].astype(np.int64))[np.diff(ik[order].astype(np.int64)) == 0] != 0)       # a payload of its own
    if shape == "hot_20000":
        hot = distinct[per_key == 20_000]
        assert len(hot) == 1 and per_key[per_key != 20_000].max() == 1
        q = int(lay.pid(hot)[0])
        assert -(-int(build_rows[q]) // FILL_ROWS) == 5 and int((build_rows > FILL_ROWS).sum()) == 1       # five table fills there alone
        assert int((ok == hot[0]).sum()) == 7
        in_q = ok[lay.pid(ok) == q]
        has = np.isin(in_q, ik)
        assert int((has & (in_q != hot[0])).sum()) >= 200 and int((~has).sum()) >= 100
    for flags in cm.FLAG_SETS:
        rk, rv, sk, sv = cm.mode_relations(shape, flags)
        assert rk is ik and sk is ok and sv is ov
        if flags in (cm.RIGHT_SEMI, cm.RIGHT_ANTI):
            m = np.isin(rk, sk)
            assert np.any(rv[m] == NULL) and np.any(rv[~m] == NULL) and int((rv != iv).sum()) <= 2
        else:
            assert rv is iv


@pytest.mark.parametrize("kind", cm.DEALT)
def test_dealt_probe_sides_fill_their_regions_to_the_row(kind):
    ok = cm.dealt_probe(kind)
    cap1, cap2 = cm.region_caps(len(ok), cm.F1, cm.F2, 0)
    rows1, rows2 = cm.region_rows(ok, cm.F1, cm.F2)
    if kind == "full_both":
        assert len(ok) == 40_960 and np.all(rows1 == cap1) and np.all(rows2 == cap2) and cm.fits(ok, cm.F1, cm.F2, 0)
    if kind == "over_pass2":
        assert len(ok) == 40_960 and np.all(rows1 == cap1) and sorted(rows2.tolist())[-2:] == [320, 321] == [cap2, cap2 + 1]
        assert not cm.fits(ok, cm.F1, cm.F2, 0)
    if kind == "full_pass1":
        assert len(ok) == 41_216 and np.all(rows1 == cap1) and rows2.max() == 322 < cap2 == 336 and cm.fits(ok, cm.F1, cm.F2, 0)
    if kind == "over_pass1":
        assert len(ok) == 41_216 and sorted(rows1.tolist())[-2:] == [2576, 2577] == [cap1, cap1 + 1] and rows2.max() == 323 < cap2 == 336
        assert not cm.fits(ok, cm.F1, cm.F2, 0)
    base = cm.dealt_probe("full_both" if kind.endswith("both") or kind.endswith("pass2") else "full_pass1")
    assert int((np.sort(ok) != np.sort(base)).sum()) <= len(ok) and len(np.setdiff1d(ok, base)) <= 1       # one row moved, at the most


def test_build_side_matches_two_thirds():
    ok = cm.uniform_probe()[0]
    ik, iv = cm.build_side(ok)
    assert len(ik) == len(np.unique(ik)) == 3001 and int(np.isin(ik, ok).sum()) == 2000 and not np.any(iv == NULL)
    ik, _ = cm.build_side(ok[:1], inner=50)
    assert len(np.unique(ik)) == 50 and ok[0] in ik
