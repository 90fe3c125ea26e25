#!/usr/bin/env python3
"""Times hjgpu_group_sum (hjgpu_get_stats: ms_join = the aggregation kernel, ms_total = the clears, the aggregation and the emit) on two key
columns and one measure column against two yardsticks taken in the same process and on the same columns:
  read   hjgpu_stream_read_ms over the bytes the call must read: the mask, the two key columns and the measure column;
  today  what a caller does without it: hjgpu_compact_selected of the three columns, then torch - the two keys packed into one int64,
         torch.unique(return_inverse=True), and index_add_ for the counts and the sums - timed by torch events around all of it.

Columns: row i belongs to group id(i) = ((i * 0x9E3779B1) mod 2^32) mod D - the groups are spread over the rows at random, so a lane's four
rows hardly ever share a tuple: the fold gains nothing here - with the keys (3 id + 1, id xor 0x5A5A5A5A) and the measure
(i * 0x85EBCA6B + 5) mod 2^32.  Masks (seeded: the same in every process): eighth - every row selected with probability 1/8 (the AND of
three random bitmaps); ones - every row (selectivity 1, through a mask of all-ones words).
Every call is checked: the group count against D, the sum of the counts against the popcount of the mask, the sum of the sums against
torch's total of the measure over the selected rows (modulo 2^64), and - in every process's first timed round - the sorted
(tuple, count, sum) rows against the rows of the torch yardstick.

usage: python tools/time_group_sum.py [--procs 5] [--reps 3] [--rows N] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first round of calls of a process is a warm-up that is not timed.  It prints each child's medians and the medians over the
children with both ratios; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASKS = ["eighth", "ones"]
M_ID, M_VAL = 0x9E3779B1, 0x85EBCA6B
CAPACITY = 1 << 17


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
    cols = torch.empty(3 * n, dtype=torch.int32, device=dev)         # key 0, key 1, the measure: one allocation
    k0, k1, val = cols[:n], cols[n:2 * n], cols[2 * n:]
    step = 1 << 26
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        val[lo:hi] = (torch.arange(lo, hi, dtype=torch.int64, device=dev) * M_VAL + 5).to(torch.int32)
    dense = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)]       # the yardstick's compacted columns
    kout = [torch.empty(CAPACITY, dtype=torch.int32, device=dev) for _ in range(2)]
    cout, sout = torch.empty(CAPACITY, dtype=torch.int64, device=dev), torch.empty(CAPACITY, dtype=torch.int64, device=dev)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    res = {}
    with H.HjGpu(0) as hj:
        G = hj.counter("group_lds_groups")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for D in (1, 7, 1000, G, 100_000):
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                ids = ((torch.arange(lo, hi, dtype=torch.int64, device=dev) * M_ID) & 0xFFFFFFFF) % D
                k0[lo:hi] = (ids * 3 + 1).to(torch.int32)
                k1[lo:hi] = (ids ^ 0x5A5A5A5A).to(torch.int32)
            del ids
            for kind in MASKS:
                host = mask_words(kind, n)
                words = torch.from_numpy(host.view(np.int32)).to(dev)
                selected, total = 0, 0                               # the generator's totals over the selected rows
                for lo in range(0, n, step):
                    hi = min(lo + step, n)
                    m = ((words[lo // 32:hi // 32].view(-1, 1) >> shifts) & 1).view(-1).bool()
                    selected += int(m.sum().item())
                    total += int((val[lo:hi].to(torch.int64) & 0xFFFFFFFF)[m].sum().item())
                del m
                total &= (1 << 64) - 1
                t_join, t_total, t_today = [], [], []
                for rep in range(a.reps + 1):                        # rep 0: warm-up
                    J = hj.group_sum(words.data_ptr(), n, [k0.data_ptr(), k1.data_ptr()], [val.data_ptr()], [x.data_ptr() for x in kout],
                                     [sout.data_ptr()], cout.data_ptr(), capacity=CAPACITY)
                    st = hj.stats()
                    assert J == D, (D, kind, J)
                    assert int(cout[:J].sum().item()) == selected, (D, kind, "counts")
                    assert int(sout[:J].sum().item()) & ((1 << 64) - 1) == total, (D, kind, "sums")
                    if rep:
                        t_join.append(st["ms_join"])
                        t_total.append(st["ms_total"])
                    if rep <= 1:                                     # the yardstick: one warm-up, one timed round
                        ev[0].record()
                        got = hj.compact_selected(words.data_ptr(), n, [k0.data_ptr(), k1.data_ptr(), val.data_ptr()], [x.data_ptr() for x in dense], capacity=n)
                        key = (dense[0][:got].to(torch.int64) & 0xFFFFFFFF) | (dense[1][:got].to(torch.int64) << 32)
                        uniq, inv = torch.unique(key, return_inverse=True)
                        counts = torch.zeros(len(uniq), dtype=torch.int64, device=dev).index_add_(0, inv, torch.ones_like(inv))
                        sums = torch.zeros(len(uniq), dtype=torch.int64, device=dev).index_add_(0, inv, dense[2][:got].to(torch.int64) & 0xFFFFFFFF)
                        ev[1].record()
                        torch.cuda.synchronize()
                        assert got == selected and len(uniq) == D
                        if rep:
                            t_today.append(ev[0].elapsed_time(ev[1]))
                            mine = (kout[0][:J].to(torch.int64) & 0xFFFFFFFF) | (kout[1][:J].to(torch.int64) << 32)
                            order = torch.argsort(mine)
                            assert bool((mine[order] == uniq).all().item()), (D, kind, "tuples")
                            assert bool((cout[:J][order] == counts).all().item()) and bool((sout[:J][order] == sums).all().item()), (D, kind, "rows")
                        del key, uniq, inv, counts, sums
                read_bytes = host.nbytes + 12 * n
                read_ms = statistics.median(hj.stream_read_ms(cols.data_ptr(), min(read_bytes, 12 * n) // 65536 * 65536) for _ in range(a.reps))
                res["%d groups, %s" % (D, kind)] = {"join": statistics.median(t_join), "total": statistics.median(t_total),
                                                    "today": statistics.median(t_today), "read_ms": read_ms, "selected": selected}
                del words
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
            print("%d rows, 2 key columns, 1 measure; ms, medians of %d calls per process after one untimed round; join = hjgpu_group_sum ms_join "
                  "(the aggregation kernel), total = ms_total, read = hjgpu_stream_read_ms of the mask and the three columns, today = "
                  "hjgpu_compact_selected + torch.unique + index_add_ (one timed round per process)" % (a.rows, a.reps))
        for k, v in runs[-1].items():
            print("process %d: %-28s join %8.3f total %8.3f read %7.3f today %9.3f" % (p, k, v["join"], v["total"], v["read_ms"], v["today"]), flush=True)
    print("%-28s %12s %9s %9s %8s %10s %11s %12s" % ("median of %d processes" % a.procs, "selected", "join", "total", "read", "today", "total/read", "today/total"))
    for k in runs[0]:
        med = {f: statistics.median(r[k][f] for r in runs) for f in ("join", "total", "today", "read_ms")}
        print("%-28s %12d %9.3f %9.3f %8.3f %10.3f %11.2f %12.1f" % (k, runs[0][k]["selected"], med["join"], med["total"], med["read_ms"], med["today"],
                                                                   med["total"] / med["read_ms"], med["today"] / med["total"]))


if __name__ == "__main__":
    main()
