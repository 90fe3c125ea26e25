"""GPU tests of hjgpu_join_partitions at its kernels' edges: the separate-column instances of join_body behind the caller's own
partitions and offsets (hjgpu_ops.hip) - several partitions, several table fills, probe partitions cut into several work items, the
chained fallback, the first-match walk and its `matched` bits, arbitrary partition starts, offsets that start beyond row 0.  The cases
and their references are tests/operator_cases.py's (checked on the CPU by tests/test_operator_cases.py); every case is run three ways -
aggregates without `out`, aggregates with `out`, and the rows after a lexsort - and every comparison is exact equality.

Every test takes a context of its own: options set here must not reach the session's other tests."""
import ctypes as C

import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd.api import PhjParams, Result
from helpers import numpy_join, materialised_rows, sort_rows
import operator_cases as oc

pytestmark = pytest.mark.gpu

BLOCKS = [256, 0]           # 0 = 65536


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
    return int(a.astype(np.uint64).sum(dtype=np.uint64)) & oc.M64


def params(lay, flags=0):
    return PhjParams(fanout1=lay.F1, fanout2=lay.F2, factor1=lay.f1, factor2=lay.f2 or 0, flags=flags)


class Device:
    """a case's columns and offsets in device memory"""

    def __init__(self, hj, rk, rv, sk, sv, roff, soff):
        col = lambda a: hj.column(a if len(a) else np.zeros(4, np.uint32))
        self.rk, self.rv, self.sk, self.sv = col(rk), col(rv), col(sk), col(sv)
        self.roff, self.soff = hj.column(roff, np.uint64), hj.column(soff, np.uint64)

    @classmethod
    def of(cls, hj, case):
        return cls(hj, case.rk, case.rv, case.sk, case.sv, case.roff, case.soff)

    def join(self, hj, prm, out=None):
        return hj.join_partitions(self.rk, self.rv, self.roff, self.sk, self.sv, self.soff, prm, out=out)

    def status(self, hj, prm, out=None):
        """(status, aggregates): the entry point itself, for the calls that are expected to fail"""
        r = Result()
        st = hj.lib.hjgpu_join_partitions(hj.handle, self.rk.ptr, self.rv.ptr, self.roff.ptr, self.sk.ptr, self.sv.ptr, self.soff.ptr,
                                          C.byref(prm), C.byref(r), hj._out(out), None)
        return st, r.as_tuple()


def output(hj, rows, block):
    cap = hj.output_capacity(1, 0, rows, block)
    assert cap % (block or 65536) == 0 and cap >= rows
    return (hj.column(cap), hj.column(cap), hj.column(cap), cap, block)


def rows_of(out, n):
    return sort_rows(out[0].download(n), out[1].download(n), out[2].download(n))


def check_three_ways(hj, dev, prm, want, want_rows, block):
    """aggregates without `out`, aggregates with `out`, rows after a lexsort"""
    assert dev.join(hj, prm) == want
    out = output(hj, want[0], block)
    assert dev.join(hj, prm, out=out) == want
    gk, go, gi = rows_of(out, want[0])
    assert np.array_equal(gk, want_rows[0]) and np.array_equal(go, want_rows[1]) and np.array_equal(gi, want_rows[2])


# ---- small geometry, offsets beyond 0, probe slices, table fills, the chained fallback, key values ------------------------------
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", oc.INNER_CASES)
def test_case_matches_numpy(ctx, name, block):
    case = oc.join_case(name)
    want, want_rows = case.reference()
    check_three_ways(ctx, Device.of(ctx, case), params(case.lay), want, want_rows, block)


@pytest.mark.parametrize("name", oc.FORCE_CHAINED_CASES)
def test_case_matches_numpy_on_chained_tables(ctx, name):
    """option "force_chained": every fill takes the chained fallback table"""
    ctx.set_option("force_chained", 1)
    case = oc.join_case(name)
    want, want_rows = case.reference()
    check_three_ways(ctx, Device.of(ctx, case), params(case.lay), want, want_rows, 256)


# ---- first match ---------------------------------------------------------------------------------------------------------
def check_first_match(hj, case, prm, block):
    ik, iv, ok, ov = case.real()
    count, sum_keys, sum_outer, sum_inner = case.unique_reference()
    dev = Device.of(hj, case)
    got = dev.join(hj, prm)
    assert got[:3] == (count, sum_keys, sum_outer)
    if sum_inner is not None:
        assert got[3] == sum_inner
    out = output(hj, count, block)
    got = dev.join(hj, prm, out=out)
    assert got[:3] == (count, sum_keys, sum_outer)
    # the dense prefix is exactly `count` rows: (key, outer_val) the probe rows with a partner, inner_val one of the key's copies
    gk, go, gi = (c.download(count) for c in out[:3])
    assert oc.unique_rows_match(ik, iv, ok, ov, gk, go, gi)
    assert got[3] == _sum(gi)
    if sum_inner is not None:
        assert got[3] == sum_inner


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("how", ["flag", "option"])
@pytest.mark.parametrize("name", oc.FIRST_MATCH_CASES)
def test_first_match(ctx, name, how, block):
    """HJGPU_FLAG_UNIQUE, and option "unique" with the flag clear.  The partition of 8193 rows is the DEDUP launch with multi_fill NULL:
    every probe row counts once although each of its key's copies sits in another fill, and with `out` the launch goes on in the blocks
    the first launch left open."""
    case = oc.join_case(name)
    if how == "option":
        ctx.set_option("unique", 1)
    check_first_match(ctx, case, params(case.lay, H.FLAG_UNIQUE if how == "flag" else 0), block)


@pytest.mark.parametrize("name", ["build_rows_8193", "key_values_two_level", "p2_minimum"])
def test_first_match_of_unique_build_keys_is_the_inner_join(ctx, name):
    """with unique build keys the flag changes nothing (include/hjgpu.h), whatever the number of fills: both launches, all rows"""
    case = oc.join_case(name)
    ik = case.real()[0]
    assert len(np.unique(ik)) == len(ik)
    want, want_rows = case.reference()
    check_three_ways(ctx, Device.of(ctx, case), params(case.lay, H.FLAG_UNIQUE), want, want_rows, 256)


# ---- partitions made three ways ----------------------------------------------------------------------------------------------
def test_partitions_made_three_ways(ctx):
    """by numpy, by hjgpu_partition twice, and two-level on the host: relations with duplicates on both sides and misses"""
    hj = ctx
    ik, iv, ok, ov = oc.three_ways_relations()
    want, want_rows = numpy_join(ik, iv, ok, ov), materialised_rows(ik, iv, ok, ov)
    # one level, by numpy
    lay = oc.Layout(oc.F_ONE, 143)
    rk, rv, roff = oc.partition_on_host(ik, iv, lay)
    sk, sv, soff = oc.partition_on_host(ok, ov, lay)
    check_three_ways(hj, Device(hj, rk, rv, sk, sv, roff, soff), params(lay), want, want_rows, 256)
    # the same level, by hjgpu_partition
    raw = [hj.column(x) for x in (ik, iv, ok, ov)]
    dev = Device(hj, np.zeros(len(ik), np.uint32), np.zeros(len(ik), np.uint32), np.zeros(len(ok), np.uint32), np.zeros(len(ok), np.uint32),
                 np.zeros(lay.P + 1, np.uint64), np.zeros(lay.P + 1, np.uint64))
    hj.partition(raw[0], raw[1], len(ik), lay.f1, lay.F1, dev.rk, dev.rv, dev.roff)
    hj.partition(raw[2], raw[3], len(ok), lay.f1, lay.F1, dev.sk, dev.sv, dev.soff)
    assert np.array_equal(dev.roff.download(), roff) and np.array_equal(dev.soff.download(), soff)
    check_three_ways(hj, dev, params(lay), want, want_rows, 256)
    # two levels, on the host
    lay2 = oc.Layout(oc.F_ONE, 13, oc.F_TWO, 11)
    rk, rv, roff = oc.partition_on_host(ik, iv, lay2)
    sk, sv, soff = oc.partition_on_host(ok, ov, lay2)
    check_three_ways(hj, Device(hj, rk, rv, sk, sv, roff, soff), params(lay2), want, want_rows, 0)


# ---- capacity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lead_37", "probe_rows_65537"])
def test_one_block_too_few_is_an_overflow_with_the_exact_count(ctx, name):
    case = oc.join_case(name)
    want, _ = case.reference()
    block = 256
    cap = (want[0] + block - 1) // block * block - block          # one block fewer than the rows fill
    assert cap >= block
    dev = Device.of(ctx, case)
    out = (ctx.column(cap), ctx.column(cap), ctx.column(cap), cap, block)
    st, got = dev.status(ctx, params(case.lay), out)
    assert st == H.api.EOVERFLOW
    assert got == want                                            # the aggregates do not depend on the rows' fate
    assert dev.join(ctx, params(case.lay)) == want                # and the context goes on


# ---- option "join_cfg" ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["build_rows_4097", "build_rows_8193", "build_rows_262145", "chained_3_16_5000_copies", "probe_rows_65537",
                                  "first_match_two_fills_probe_65537", "first_match_2_and_16_copies_own_payloads"])
def test_the_other_built_geometry(ctx, name):
    """"join_cfg" = "1024,14,2": JOIN_BUILT (join_kernels.hip) lists it with a _UNIQUE instance, launch_join_at<1024, 14, true> has the
    separate-column instances of both launches, and the plan takes its cap from the context's geometry - so the result is exactly the
    default geometry's, with fills of 8192 rows (the partition of 8193 rows still takes two)."""
    ctx.set_option("join_cfg", "1024,14,2")
    case = oc.join_case(name)
    if case.unique:
        check_first_match(ctx, case, params(case.lay, H.FLAG_UNIQUE), 256)
    else:
        want, want_rows = case.reference()
        check_three_ways(ctx, Device.of(ctx, case), params(case.lay), want, want_rows, 256)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_are_decided_before_anything_runs(ctx):
    hj = ctx
    case = oc.join_case("p2_minimum")
    dev = Device.of(hj, case)
    want, _ = case.reference()
    good = params(case.lay)

    def status(prm=good, **ptr):
        a = dict(rk=dev.rk.ptr, rv=dev.rv.ptr, roff=dev.roff.ptr, sk=dev.sk.ptr, sv=dev.sv.ptr, soff=dev.soff.ptr)
        a.update(ptr)
        r = Result()
        return hj.lib.hjgpu_join_partitions(hj.handle, a["rk"], a["rv"], a["roff"], a["sk"], a["sv"], a["soff"],
                                            C.byref(prm) if prm is not None else None, C.byref(r), None, None)

    # probe columns off 16-byte alignment
    for off in (4, 8, 12):
        assert status(sk=dev.sk.ptr + off) == H.api.EALIGN
        assert status(sv=dev.sv.ptr + off) == H.api.EALIGN
    # P < 2, P > 32768, fan-out 0, even factors
    f = case.lay.f1
    for prm in (PhjParams(fanout1=1, fanout2=1, factor1=f), PhjParams(fanout1=1, fanout2=0, factor1=f), PhjParams(fanout1=0, fanout2=4, factor1=f),
                PhjParams(fanout1=1024, fanout2=33, factor1=f, factor2=oc.F_TWO), PhjParams(fanout1=32769, fanout2=1, factor1=f),
                PhjParams(fanout1=2, fanout2=1, factor1=f + 1), PhjParams(fanout1=2, fanout2=3, factor1=f, factor2=oc.F_TWO + 1),
                PhjParams(fanout1=2, fanout2=1, factor1=f, table_factor=(2, 0)), PhjParams(fanout1=2, fanout2=1, factor1=f, table_factor=(0, 4))):
        assert status(prm) == H.api.EINVAL, (prm.fanout1, prm.fanout2, prm.factor1, prm.factor2)
    # NULL pointers
    for name in ("rk", "rv", "roff", "sk", "sv", "soff"):
        assert status(**{name: None}) == H.api.EINVAL, name
    assert status(None) == H.api.EINVAL
    # a join mode is not this entry point's
    assert status(params(case.lay, H.FLAG_SEMI)) == H.api.EINVAL
    # nothing of that disturbed the context
    assert dev.join(hj, good) == want
