"""GPU tests of every join mode on the claimed probe side of a blocking two-pass hjgpu_phj, on its build-beside form and on the exact
path, against the host model tests/claimed_model.py (join_reference: every mode of include/hjgpu.h, written from the header; fits: does
every optimistic region hold its rows).  Aggregates are compared exactly, materialised rows after a lexsort; over duplicated build keys
the first-match forms are checked by first_match_errors.

Three roads:
  claimed   option build_beside = 0: pass 1 of the probe side without its histogram, two pieces per final partition in the join
  beside    option build_cus = 24: the same, with the build side's chain on the context's side stream
  exact     option exact_probe_counts = 1
Every case asserts the road it took (counters "probe_fallbacks", "probe_exact", "build_beside"), and a case that is meant to stay on the
road asserts fits() first: a failed road assertion then points at the library, not at the input.  Two passes are forced at small sizes
with explicit fan-outs, 16 x 8 unless the case is about the fan-out.

Every test takes a context of its own: a fallback makes a context's later joins exact, and the session context must not inherit options.
A case that is meant to fall back takes ONE road per test for the same reason."""
import functools

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
import claimed_model as cm

pytestmark = pytest.mark.gpu

ROADS = ("claimed", "beside", "exact")
BUILD_CUS = 24
TWO_COLUMNS = {cm.SEMI: (0, 1), cm.ANTI: (0, 1), cm.RIGHT_SEMI: (0, 2), cm.RIGHT_ANTI: (0, 2)}      # (keys, outer_vals) / (keys, inner_vals)
COUNTERS = ("probe_fallbacks", "probe_exact", "build_beside")


@pytest.fixture
def ctx():
    """a context whose device columns are all freed when the test ends"""
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


def test_the_models_flags_are_the_packages():
    assert (cm.UNIQUE, cm.SEMI, cm.ANTI, cm.LEFT_OUTER, cm.RIGHT_OUTER, cm.FULL_OUTER, cm.RIGHT_SEMI, cm.RIGHT_ANTI) == \
        (H.api.FLAG_UNIQUE, H.FLAG_SEMI, H.FLAG_ANTI, H.FLAG_LEFT_OUTER, H.FLAG_RIGHT_OUTER, H.FLAG_FULL_OUTER, H.FLAG_RIGHT_SEMI, H.FLAG_RIGHT_ANTI)


# ---- inputs and references, made once and never written to ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rel(name):
    """(ik, iv, ok, ov) of a named input:
      ("mode", shape, flags)   claimed_model.mode_relations
      ("uniform", n)           the first n rows of the uniform probe side, a build side of 3 001 unique keys, 2 000 of them the probe side's
                               (all of the probe side's keys when it has fewer)
      ("dealt", kind)          claimed_model.dealt_probe and such a build side"""
    if name[0] == "mode":
        return cm.mode_relations(name[1], name[2])
    ok = cm.uniform_probe()[0][:name[1]] if name[0] == "uniform" else cm.dealt_probe(name[1])
    ik, iv = cm.build_side(ok)
    ov = np.random.default_rng(23 + len(ok)).integers(0, 1 << 32, size=len(ok), dtype=np.uint64).astype(np.uint32)
    ov.setflags(write=False)
    return ik, iv, ok, ov


@functools.lru_cache(maxsize=None)
def _want(name, mode):
    return cm.join_reference(mode, *_rel(name))


@functools.lru_cache(maxsize=None)
def _duplicated(name):
    ik = _rel(name)[0]
    return len(np.unique(ik)) != len(ik)


@functools.lru_cache(maxsize=None)
def _fits(name, fan, slack):
    return cm.fits(_rel(name)[2], fan[0], fan[1], slack)


# ---- one join, checked --------------------------------------------------------------------------------------------------
def _upload(hj, name):
    return [hj.column(a) if len(a) else hj.column(np.zeros(4, np.uint32)) for a in _rel(name)]


def _join(hj, cols, name, flags, fan, block):
    """the join of the named input: (aggregates, rows as downloaded or None); block None: aggregates only.  The capacity is
    hjgpu_output_capacity of the true row count."""
    ik, _, ok, _ = _rel(name)
    prm = H.PhjParams(fanout1=fan[0], fanout2=fan[1], flags=flags)
    if block is None:
        return tuple(hj.phj(cols[0], cols[1], len(ik), cols[2], cols[3], len(ok), prm)), None
    mode = flags & ~cm.UNIQUE
    rows = len(ok) if flags == cm.LEFT_OUTER | cm.UNIQUE else int(np.isin(ok, ik).sum()) if flags == cm.UNIQUE else _want(name, mode)[0][0]
    cap = hj.output_capacity(1, len(ok), rows, block)
    assert cap % block == 0
    out = [hj.column(max(cap, 4)) for _ in range(3)]
    try:
        res = tuple(hj.phj(cols[0], cols[1], len(ik), cols[2], cols[3], len(ok), prm, out=(out[0], out[1], out[2], cap, block)))
        assert res[0] <= cap
        got = tuple(out[c].download(res[0]) for c in TWO_COLUMNS.get(mode, (0, 1, 2)))
    finally:
        for c in out:
            c.free()
    return res, got


def _check(name, flags, res, got, what):
    """aggregates and (where there are any) rows against the model"""
    mode = flags & ~cm.UNIQUE
    if flags & cm.UNIQUE and _duplicated(name):
        assert cm.first_match_errors(mode, *_rel(name), res, got) == [], what
        return
    # (HJGPU_FLAG_UNIQUE over unique build keys: the result is the same as without the flag)
    agg, rows = _want(name, mode)
    assert res == agg, (what, res, agg)
    if got is not None:
        got = cm.sorted_rows(*got)
        assert len(got) == len(rows) and all(np.array_equal(g, w) for g, w in zip(got, rows)), what


def _counters(hj):
    return {n: hj.counter(n) for n in COUNTERS}


def _take(hj, road):
    if road == "claimed":
        hj.set_option("build_beside", 0)
    if road == "beside":
        hj.set_option("build_beside", 1)
        hj.set_option("build_cus", BUILD_CUS)
    if road == "exact":
        hj.set_option("exact_probe_counts", 1)


def run_roads(hj, name, flag_sets, roads=ROADS, fan=(cm.F1, cm.F2), slack=cm.DEFAULT_SLACK, expect="stays", blocks=(None, 512, 4096)):
    """Every flag set on every road of `roads` (in ROADS' order on this one context), every join checked against the model, and the road
    asserted from the context's counters.  expect:
      "stays"        the probe side fits its regions (asserted here, on the host): no fallback, and the beside form every time
      "falls_back"   it does not (asserted here): the first join of a claimed or beside road falls back once, its result is the exact
                     path's, and the context is exact from then on
      "not_claimed"  the plan has no claimed probe side: no fallback, no beside form, and the context does not turn exact"""
    assert expect in ("stays", "falls_back", "not_claimed")
    ok = _rel(name)[2]
    if expect == "stays":
        assert _fits(name, fan, slack), "the input is meant to fit its regions"
    if expect == "falls_back":
        assert not _fits(name, fan, slack), "the input is meant to overflow a region"
    cols = _upload(hj, name)
    if slack != cm.DEFAULT_SLACK:
        hj.set_option("probe_slack", slack)
    for road in roads:
        _take(hj, road)
        before = _counters(hj)
        joins = 0
        for flags in flag_sets:
            for block in blocks:
                res, got = _join(hj, cols, name, flags, fan, block)
                joins += 1
                _check(name, flags, res, got, (name, cm.MODE_NAMES[flags], road, block))
                s = hj.stats()
                assert (s["fanout1"], s["fanout2"]) == fan
                if road != "exact" and expect == "falls_back" and len(ok):
                    # the first join fell back, every later one is exact at once
                    after = _counters(hj)
                    assert after["probe_fallbacks"] == before["probe_fallbacks"] + 1 and after["probe_exact"] == 1, (road, joins, after)
                    # (the optimistic attempt took the beside form - unless pass 1's regions hold no tuple: then no attempt is made)
                    attempted = cm.region_caps(len(ok), fan[0], fan[1], slack)[0] > 0
                    assert after["build_beside"] == before["build_beside"] + (1 if road == "beside" and attempted else 0), (road, joins, after)
        after = _counters(hj)
        if road == "exact":
            assert after["probe_exact"] == 1 and after["build_beside"] == before["build_beside"], after
            assert after["probe_fallbacks"] == before["probe_fallbacks"], after
        elif expect != "falls_back":
            assert after["probe_fallbacks"] == 0 and after["probe_exact"] == 0, (road, after)
            moved = joins if road == "beside" and expect == "stays" and len(ok) and len(_rel(name)[0]) else 0
            assert after["build_beside"] == before["build_beside"] + moved, (road, joins, before, after)


def _flag_ids(sets):
    return [cm.MODE_NAMES[f] for f in sets]


# ---- a. modes x build shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", cm.FLAG_SETS, ids=_flag_ids(cm.FLAG_SETS))
@pytest.mark.parametrize("shape", cm.BUILD_SHAPES + ("triple_force_chained",))
def test_every_flag_set_on_every_build_shape(ctx, shape, flags):
    """all ten flag sets on the claimed road, the beside form and the exact path: aggregates only, rows in blocks of 512 and of 4096"""
    if shape == "triple_force_chained":
        ctx.set_option("force_chained", 1)
        shape = "triple"
    run_roads(ctx, ("mode", shape, flags), [flags])


# ---- b. the pass-1 instances and the gate -------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [cm.INNER, cm.FULL_OUTER], ids=_flag_ids([cm.INNER, cm.FULL_OUTER]))
@pytest.mark.parametrize("fan", [(216, 2), (217, 2), (436, 2)], ids=lambda f: "%dx%d" % f)
def test_both_claimed_instances_of_pass_1(ctx, fan, flags):
    """the last fan-out of the 16 384-tuple tiles, and the first and the last of the 12 288-tuple tiles (1024 threads x 3 vectors)"""
    run_roads(ctx, ("uniform", cm.OUTER), [flags], fan=fan, blocks=(None, 4096))


@pytest.mark.parametrize("flags", [cm.INNER, cm.FULL_OUTER], ids=_flag_ids([cm.INNER, cm.FULL_OUTER]))
@pytest.mark.parametrize("road", ["claimed", "beside"])
@pytest.mark.parametrize("fan", [(436, 2), (437, 2)], ids=lambda f: "%dx%d" % f)
def test_fan_out_436_is_the_last_that_is_claimed(ctx, fan, road, flags):
    """regions without slack and uniform keys: a claimed probe side must overflow.  At 436 x 2 it does, once; at 437 x 2 (8 192-tuple tiles,
    a pass 1 without a claimed instance) the same input falls back nowhere, because nothing was claimed"""
    assert not _fits(("uniform", cm.OUTER), fan, 0)
    run_roads(ctx, ("uniform", cm.OUTER), [flags], roads=(road,), fan=fan, slack=0, expect="falls_back" if fan[0] <= 436 else "not_claimed",
              blocks=(None, 4096))


# ---- c. exactly full, one row over ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [cm.INNER, cm.FULL_OUTER], ids=_flag_ids([cm.INNER, cm.FULL_OUTER]))
@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("kind", cm.DEALT)
def test_a_region_exactly_full_stays_and_one_row_more_falls_back(ctx, kind, road, flags):
    """option probe_slack = 0 and probe rows dealt to the regions by hand.  "when one is full" (include/hjgpu.h) is decided by `<=` in both
    passes: a region that its rows fill to the last tuple is no overflow, one row more is - in pass 2 alone (over_pass2), in pass 1
    alone (over_pass1)"""
    run_roads(ctx, ("dealt", kind), [flags], roads=(road,), slack=0, expect="stays" if kind.startswith("full") else "falls_back",
              blocks=(None, 512))


# ---- d. tiny and ragged probe sides -------------------------------------------------------------------------------------
RAGGED = (1, 15, 16, 17, 127, 16_384, 16_385, 50_002)          # 127 < P = 128; 16 384: one tile; 50 002: no multiple of 4


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("slack", [cm.DEFAULT_SLACK, 0])
@pytest.mark.parametrize("outer", RAGGED)
def test_tiny_and_ragged_probe_sides(ctx, outer, slack, road):
    """inner, anti- and right anti-join.  Without slack the random keys of the larger sizes overflow; with fewer probe rows than
    partitions a final region holds no tuple at all (cap2 = 0), and below 16 rows a pass-1 region holds none either (cap1 = 0): every
    row overflows.  Each of these falls back once, and the fallback's result is the exact path's.
    (1 and 15 rows without slack used to return HJGPU_EINVAL: pass 1 has no launch for regions of no tuples.)"""
    name = ("uniform", outer)
    cap1, cap2 = cm.region_caps(outer, cm.F1, cm.F2, slack)
    assert (cap2 == 0) == (slack == 0 and outer < cm.F1 * cm.F2) and (cap1 == 0) == (slack == 0 and outer < cm.F1)
    run_roads(ctx, name, [cm.INNER, cm.ANTI, cm.RIGHT_ANTI], roads=(road,), slack=slack, expect="stays" if slack else "falls_back",
              blocks=(None, 512))


# ---- e. state across calls ----------------------------------------------------------------------------------------------
def test_24_joins_back_to_back_across_modes_and_shapes(ctx):
    """one context, the beside form: the marks bitmap, final_offsets, the tickets and both streams are reused across two build shapes and
    five modes, every result checked with its rows"""
    names = [("mode", "unique", cm.INNER), ("mode", "triple", cm.INNER)]
    modes = [cm.RIGHT_OUTER, cm.INNER, cm.RIGHT_ANTI, cm.FULL_OUTER, cm.SEMI]
    fan = (cm.F1, cm.F2)
    assert all(_fits(n, fan, cm.DEFAULT_SLACK) for n in names)
    cols = [_upload(ctx, n) for n in names]
    _take(ctx, "beside")
    seen = set()
    for n in range(24):
        name, flags = names[n & 1], modes[n % 5]
        res, got = _join(ctx, cols[n & 1], name, flags, fan, 512 if n % 3 == 0 else 4096)
        _check(name, flags, res, got, (n, name, cm.MODE_NAMES[flags]))
        seen.add((n & 1, flags))
        assert ctx.counter("build_beside") == n + 1
    assert len(seen) == 10
    assert ctx.counter("probe_fallbacks") == 0 and ctx.counter("probe_exact") == 0
