"""GPU tests of hjgpu_npj_build / hjgpu_npj_probe on tables with ONE empty bucket (buckets = n + 1): every walk of an absent key goes all
the way to that bucket, most of them past the last bucket and on from bucket 0; build keys in 1, 2 and 40 copies; probe sides with
misses and a key 0 (which matches nothing).  8 buckets take the walk that reads groups of 4 buckets, 2 and 4097 the bucket-at-a-time
walk.  Cases: tests/operator_cases.py; exact equality against helpers.numpy_join / materialised_rows.

Every test takes a context of its own: option "unique" is set here."""
import numpy as np
import pytest

import hash_join_codes_knl_amd as H
from hash_join_codes_knl_amd.api import HjGpuError
from helpers import numpy_join, materialised_rows, sort_rows
import operator_cases as oc

pytestmark = pytest.mark.gpu


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


def built_table(hj, ik, iv, buckets):
    rk, rv = hj.column(ik), hj.column(iv)
    table = hj.column(np.full(buckets, 0x1111111111111111, np.uint64), np.uint64)          # the build clears it itself
    hj.npj_build(rk, rv, len(ik), table, buckets, oc.F_NPJ)
    return table


def output(hj, outer, rows, block):
    cap = hj.output_capacity(0, outer, rows, block)
    return (hj.column(cap), hj.column(cap), hj.column(cap), cap, block)


@pytest.mark.parametrize("block", [256, 0])
@pytest.mark.parametrize("n", oc.NPJ_ROWS)
def test_probe_of_a_full_table_matches_numpy(ctx, n, block):
    hj = ctx
    ik, iv, ok, ov = oc.npj_case(n)
    buckets = n + 1
    table = built_table(hj, ik, iv, buckets)
    # the table holds every build tuple once and one empty bucket
    got = np.sort(table.download())
    assert np.array_equal(got, np.sort(np.concatenate([np.zeros(1, np.uint64), (iv.astype(np.uint64) << np.uint64(32)) | ik.astype(np.uint64)])))
    want, want_rows = numpy_join(ik, iv, ok, ov), materialised_rows(ik, iv, ok, ov)
    sk, sv = hj.column(ok), hj.column(ov)
    assert hj.npj_probe(sk, sv, len(ok), table, buckets, oc.F_NPJ) == want
    out = output(hj, len(ok), want[0], block)
    assert hj.npj_probe(sk, sv, len(ok), table, buckets, oc.F_NPJ, out=out) == want
    gk, go, gi = sort_rows(*(c.download(want[0]) for c in out[:3]))
    assert np.array_equal(gk, want_rows[0]) and np.array_equal(go, want_rows[1]) and np.array_equal(gi, want_rows[2])


@pytest.mark.parametrize("n", oc.NPJ_ROWS)
def test_first_match_probe_of_a_full_table(ctx, n):
    """option "unique" reaches the operator-level probe: one row per probe tuple with a partner, the payload of one of the key's copies"""
    hj = ctx
    hj.set_option("unique", 1)
    ik, iv, ok, ov = oc.npj_case(n)
    buckets = n + 1
    table = built_table(hj, ik, iv, buckets)
    count, sum_keys, sum_outer, sum_inner = oc.unique_reference(ik, iv, ok, ov)
    assert (sum_inner is None) == (n > 1)
    sk, sv = hj.column(ok), hj.column(ov)
    got = hj.npj_probe(sk, sv, len(ok), table, buckets, oc.F_NPJ)
    assert got[:3] == (count, sum_keys, sum_outer) and (sum_inner is None or got[3] == sum_inner)
    out = output(hj, len(ok), count, 256)
    got = hj.npj_probe(sk, sv, len(ok), table, buckets, oc.F_NPJ, out=out)
    assert got[:3] == (count, sum_keys, sum_outer)
    gk, go, gi = (c.download(count) for c in out[:3])
    assert oc.unique_rows_match(ik, iv, ok, ov, gk, go, gi)
    assert got[3] == int(gi.astype(np.uint64).sum(dtype=np.uint64)) & oc.M64


def test_a_table_without_an_empty_bucket_is_refused(ctx):
    hj = ctx
    ik, iv, _, _ = oc.npj_case(7)
    rk, rv = hj.column(ik), hj.column(iv)
    table = hj.column(8, np.uint64)
    for buckets in (7, 6, 0):
        with pytest.raises(HjGpuError) as e:
            hj.npj_build(rk, rv, len(ik), table, buckets, oc.F_NPJ)
        assert e.value.status == H.api.EINVAL
    with pytest.raises(HjGpuError) as e:
        hj.npj_build(rk, rv, len(ik), table, 8, oc.F_NPJ + 1)                     # even factor
    assert e.value.status == H.api.EINVAL
    hj.npj_build(rk, rv, len(ik), table, 8, oc.F_NPJ)                             # and the context goes on


@pytest.mark.parametrize("n,at", [(1, 0), (7, 3), (4096, 4095)])
def test_a_build_key_zero_is_reported(ctx, n, at):
    hj = ctx
    ik, iv, _, _ = oc.npj_case(n)
    ik = ik.copy()
    ik[at] = 0
    rk, rv = hj.column(ik), hj.column(iv)
    table = hj.column(n + 1, np.uint64)
    with pytest.raises(HjGpuError) as e:
        hj.npj_build(rk, rv, n, table, n + 1, oc.F_NPJ)
    assert e.value.status == H.api.EZEROKEY
