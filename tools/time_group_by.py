#!/usr/bin/env python3
"""Times hjgpu_group_by with three and four key columns (hjgpu_get_stats: ms_join = the aggregation kernel, ms_total = the clears, the
aggregation and the emit) against three yardsticks on the same rows, masks and groups, all taken in the same process:

  (a) two keys        hjgpu_group_agg over (key 0, p), where p is the further key columns packed into one uint32 column beforehand: the
                      code that this road leaves untouched;
  (b) (a) + the read  (a) plus hjgpu_stream_read_ms over one (three keys) or two (four keys) further columns: what a third and a fourth
                      key ought to cost;
  (c) today           what a caller did without the wide road: torch packs key columns 1 ... nkeys - 1 into p - timed by torch events - and
                      then calls (a); the pack is part of the time.  It works only while the packed value fits 32 bits.

Columns: row i belongs to group id(i) = ((i * 0x9E3779B1) mod 2^32) mod 1000; with three keys the tuple is the id's three decimal digits, with
four (id mod 10, id / 10 mod 10, id / 100 mod 5, id / 500); a = (i * 0x85EBCA6B + 5) mod 2^32 and b = (i * 0xC2B2AE35 + 7) mod 2^32.  Masks
(seeded: the same in every process): eighth - every row selected with probability 1/8; ones - every row, through a mask of all-ones words.
Aggregates: one SUM(a * b), and MIN(a) + MAX(b).
Every call is checked against torch: the group count, the sum of the counts against the popcount of the mask, the aggregates' totals against
torch's own over the selected rows (modulo 2^64 for the sum, the overall extremes for MIN and MAX), and the wide call's rows, sorted by
tuple, against the rows of (a).

usage: python tools/time_group_by.py [--procs 5] [--reps 3] [--rows N] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first round of calls of a process is a warm-up that is not timed.  It prints each child's medians and, per row, the median
over the children; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASKS = ["eighth", "ones"]
M_ID, M_A, M_B = 0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35
GROUPS = 1000
BASES = {3: (10, 10, 10), 4: (10, 10, 5, 2)}
CAPACITY = 1 << 17
M64 = (1 << 64) - 1


def mask_words(kind, n):
    words = (n + 31) // 32
    w = np.full(words, 0xFFFFFFFF, np.uint32)
    if kind == "eighth":
        rng = np.random.default_rng(1)
        for _ in range(3):
            w &= rng.integers(0, 2**32, size=words, dtype=np.uint64).astype(np.uint32)
    return w


def child(a):
    import torch
    torch.cuda.init()
    import hash_join_codes_knl_amd as H
    n = a.rows
    assert n % 32 == 0, "--rows must be a multiple of 32 (whole mask words, 16-byte aligned columns in one allocation)"
    dev = torch.device("cuda")
    cols = torch.empty(7 * n, dtype=torch.int32, device=dev)         # key 0 ... key 3, a, b, p: one allocation
    key = [cols[c * n:(c + 1) * n] for c in range(4)]
    va, vb, packed = cols[4 * n:5 * n], cols[5 * n:6 * n], cols[6 * n:]
    step = 1 << 26
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        i = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        va[lo:hi] = (i * M_A + 5).to(torch.int32)
        vb[lo:hi] = (i * M_B + 7).to(torch.int32)
    del i
    u32 = lambda t: t.to(torch.int64) & 0xFFFFFFFF                    # noqa: E731
    kout = [torch.empty(CAPACITY, dtype=torch.int32, device=dev) for _ in range(4)]
    k2 = [torch.empty(CAPACITY, dtype=torch.int32, device=dev) for _ in range(2)]      # (a)'s own key outputs: the wide call's stay for the comparison
    cout = [torch.empty(CAPACITY, dtype=torch.int64, device=dev) for _ in range(2)]
    aout = [[torch.empty(CAPACITY, dtype=torch.int64, device=dev) for _ in range(2)] for _ in range(2)]       # the wide call's, (a)'s
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    MUL, MIN, MAX = H.AGG_SUM_MUL, H.AGG_MIN, H.AGG_MAX
    res = {}

    def fill_keys(nkeys):
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            ids = ((torch.arange(lo, hi, dtype=torch.int64, device=dev) * M_ID) & 0xFFFFFFFF) % GROUPS
            for c, base in enumerate(BASES[nkeys]):
                key[c][lo:hi] = (ids % base if c < nkeys - 1 else ids).to(torch.int32)
                ids = ids // base

    def pack(nkeys):
        """key columns 1 ... nkeys - 1 in one uint32 column: one torch kernel per further column"""
        b1, b2 = BASES[nkeys][1], BASES[nkeys][1] * BASES[nkeys][2]
        torch.add(key[1], key[2], alpha=b1, out=packed)
        if nkeys == 4:
            packed.add_(key[3], alpha=b2)

    with H.HjGpu(0) as hj:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        masks = {}
        for kind in MASKS:                                            # the masks and torch's own totals over the selected rows
            host = mask_words(kind, n)
            words = torch.from_numpy(host.view(np.int32)).to(dev)
            t = dict(selected=0, sum_ab=0, min_a=1 << 32, max_b=-1)
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                m = ((words[lo // 32:hi // 32].view(-1, 1) >> shifts) & 1).view(-1).bool()
                x, y = u32(va[lo:hi])[m], u32(vb[lo:hi])[m]
                t["selected"] += int(m.sum().item())
                t["sum_ab"] += int((x * y).sum().item()) & M64         # (the products wrap in int64 as they do modulo 2^64)
                t["min_a"], t["max_b"] = min(t["min_a"], int(x.min().item())), max(t["max_b"], int(y.max().item()))
            del m, x, y
            t["sum_ab"] &= M64
            masks[kind] = (words, t)
        total_u64 = lambda x, J: int(x[:J].sum().item()) & M64         # noqa: E731

        def checked(J, counts, outs, name, t, what):
            assert J == GROUPS and total_u64(counts, J) == t["selected"], what
            if name == "SUM_MUL":
                assert total_u64(outs[0], J) == t["sum_ab"], what
            else:
                assert int(outs[0][:J].min().item()) == t["min_a"] and int(outs[1][:J].max().item()) == t["max_b"], what

        for nkeys in (3, 4):
            fill_keys(nkeys)
            kptr = [k.data_ptr() for k in key[:nkeys]]
            two = [key[0].data_ptr(), packed.data_ptr()]
            read_ms = statistics.median(hj.stream_read_ms(key[1].data_ptr(), 4 * n * (nkeys - 2) // 65536 * 65536) for _ in range(a.reps))
            for kind in MASKS:
                words, t = masks[kind]
                for name, aggs in (("SUM_MUL", [(MUL, va.data_ptr(), vb.data_ptr())]), ("MIN+MAX", [(MIN, va.data_ptr()), (MAX, vb.data_ptr())])):
                    wide, agg2, packs = [], [], []
                    na = len(aggs)
                    for rep in range(a.reps + 1):                    # rep 0: warm-up
                        J = hj.group_by(words.data_ptr(), n, kptr, aggs, [x.data_ptr() for x in kout[:nkeys]], [x.data_ptr() for x in aout[0][:na]],
                                        cout[0].data_ptr(), capacity=CAPACITY)
                        st = hj.stats()
                        checked(J, cout[0], aout[0], name, t, (nkeys, kind, name, "wide"))
                        if rep:
                            wide.append((st["ms_join"], st["ms_total"]))
                        packed.zero_()
                        ev[0].record()
                        pack(nkeys)
                        ev[1].record()
                        torch.cuda.synchronize()
                        J2 = hj.group_agg(words.data_ptr(), n, two, aggs, [x.data_ptr() for x in k2], [x.data_ptr() for x in aout[1][:na]],
                                          cout[1].data_ptr(), capacity=CAPACITY)
                        st2 = hj.stats()
                        checked(J2, cout[1], aout[1], name, t, (nkeys, kind, name, "two keys"))
                        if rep:
                            agg2.append((st2["ms_join"], st2["ms_total"]))
                            packs.append(ev[0].elapsed_time(ev[1]))
                        # the rows of both, sorted by tuple
                        b1, b2 = BASES[nkeys][1], BASES[nkeys][1] * BASES[nkeys][2]
                        pw = u32(kout[1][:J]) + u32(kout[2][:J]) * b1 + (u32(kout[3][:J]) * b2 if nkeys == 4 else 0)
                        ow, o2 = torch.argsort(u32(kout[0][:J]) | (pw << 32)), torch.argsort(u32(k2[0][:J]) | (u32(k2[1][:J]) << 32))
                        assert bool((u32(kout[0][:J])[ow] == u32(k2[0][:J])[o2]).all().item()) and bool((pw[ow] == u32(k2[1][:J])[o2]).all().item()), (nkeys, kind, name, "tuples")
                        for x, y in zip([cout[0]] + aout[0][:na], [cout[1]] + aout[1][:na]):
                            assert bool((x[:J][ow] == y[:J][o2]).all().item()), (nkeys, kind, name, "rows")
                    med = lambda rows, f: statistics.median(r[f] for r in rows)     # noqa: E731
                    res["%d keys, %s, %s" % (nkeys, name, kind)] = {
                        "wide_join": med(wide, 0), "wide_total": med(wide, 1), "two_join": med(agg2, 0), "two_total": med(agg2, 1),
                        "read_ms": read_ms, "pack_ms": statistics.median(packs)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for p in range(a.procs):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rows", str(a.rows)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                     # nothing more is started behind a process that failed
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if p == 0:
            print("%d rows, %d groups; ms, medians of %d calls per process after one untimed round; join = ms_join (the aggregation kernel), total = ms_total; "
                  "wide = hjgpu_group_by, two = hjgpu_group_agg over (key 0, the packed further keys), read = hjgpu_stream_read_ms of the further key "
                  "columns, pack = torch packing them" % (a.rows, GROUPS, a.reps))
        for k, v in runs[-1].items():
            print("process %d: %-28s %s" % (p, k, "  ".join("%s %.3f" % (f, v[f]) for f in v)), flush=True)
    print("%-28s %9s %10s | %9s %9s | %8s %11s | %8s %11s | %9s %9s" % ("median of %d processes" % a.procs, "wide join", "wide total", "(a) join", "(a) total", "read",
                                                                     "(b) total", "pack", "(c) total", "wide/(b)", "wide/(c)"))
    for k in runs[0]:
        m = {f: statistics.median(r[k][f] for r in runs) for f in runs[0][k]}
        b, c = m["two_total"] + m["read_ms"], m["two_total"] + m["pack_ms"]
        print("%-28s %9.3f %10.3f | %9.3f %9.3f | %8.3f %11.3f | %8.3f %11.3f | %9.2f %9.2f" % (k, m["wide_join"], m["wide_total"], m["two_join"], m["two_total"],
                                                                                           m["read_ms"], b, m["pack_ms"], c, m["wide_total"] / b, m["wide_total"] / c))


if __name__ == "__main__":
    main()
