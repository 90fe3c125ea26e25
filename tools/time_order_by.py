#!/usr/bin/env python3
"""Times hjgpu_order_by (hjgpu_get_stats: ms_total = the initial permutation, the sorting passes and the gather) against the same
ordering by torch on the same device, in the same process: successive stable sorts from the last key to the first -
torch.sort(stable=True, descending=...) of the key gathered through the permutation so far - then index_select per carried column (and
torch.nonzero of the unpacked mask in front, where there is a mask), timed by torch events.  This comparison is the yardstick.

The cases:
  LDS road      1000 and L groups (L = hjgpu_get_counter "order_lds_rows"): two uint32 keys ascending and one uint64 sum descending, three
                carried columns (two uint32, one uint64), every row selected.
  device road   one uint32 key ascending and one carried uint32 column at 2^20, 2^24 and 2^28 rows with every row selected (no mask); the
                same at 2^28 rows with one row in eight selected by a mask; two uint32 keys (the first with 1000 distinct values) at 2^24 rows.
Keys: key 0 of row i = (i * 0x9E3779B1 mod 2^32) >> 1 - below 2^31, so that torch's int32 order is the unsigned order -, for two and three
keys taken modulo 1000 / 30, the last key then (i * 0x85EBCA6B + 5 mod 2^32) >> 1; the sum column = (i * 0xC2B2AE35 + 7) mod 2^40 (below
2^63: torch has no uint64 sort).  The mask is seeded: the same in every process.
Every timed result is checked against torch's before it is trusted: the count, the row numbers and every carried column, for equality
(torch's stable sorts keep ties in row order, descending ones too: the operator's tie rule).

usage: python tools/time_order_by.py [--procs 3] [--reps 5] [--max-log2 28] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first call of every case in a process is a warm-up that is not timed.  It prints each child's medians and, per case, the
median over the children; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M_0, M_1, M_S = 0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35


def mask_words(n):
    """one row in eight"""
    rng = np.random.default_rng(1)
    w = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    for _ in range(3):
        w &= rng.integers(0, 2**32, size=len(w), dtype=np.uint64).astype(np.uint32)
    return w


def child(a):
    import torch
    torch.cuda.init()
    import hash_join_codes_knl_amd as H
    from hash_join_codes_knl_amd.api import ORDER_DESC, ORDER_WIDE
    dev = torch.device("cuda")
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    res = {}

    def columns(n, nkeys, wide_sum):
        step = 1 << 26
        k = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(nkeys)]
        s = torch.empty(n, dtype=torch.int64, device=dev) if wide_sum else None
        pay = torch.empty(n, dtype=torch.int32, device=dev)
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            i = torch.arange(lo, hi, dtype=torch.int64, device=dev)
            x = ((i * M_0) & 0xFFFFFFFF) >> 1
            last = (((i * M_1 + 5) & 0xFFFFFFFF) >> 1).to(torch.int32)
            if nkeys == 1:
                k[0][lo:hi] = x.to(torch.int32)
            else:
                k[0][lo:hi] = (x % 1000).to(torch.int32)
                if nkeys == 3:
                    k[1][lo:hi] = (x % 30).to(torch.int32)
                k[nkeys - 1][lo:hi] = last
            if wide_sum:
                s[lo:hi] = (i * M_S + 7) & ((1 << 40) - 1)
            pay[lo:hi] = (i ^ 0x5A5A5A5A).to(torch.int32)
        return k, s, pay

    def by_torch(keys, cols, words, n):
        """[(tensor, descending)] from the first key to the last; returns (permutation, carried columns)"""
        perm = None
        if words is not None:
            perm = torch.nonzero(((words.view(-1, 1) >> shifts) & 1).view(-1)[:n]).view(-1)
        for t, desc in reversed(keys):
            o = torch.sort(t if perm is None else t.index_select(0, perm), stable=True, descending=desc).indices
            perm = o if perm is None else perm.index_select(0, o)
        return perm, [c.index_select(0, perm) for c in cols]

    with H.HjGpu(0) as hj:
        L = hj.counter("order_lds_rows")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        cases = [("LDS road, %d groups, 3 keys, 3 columns" % g, g, 3, True, False) for g in (1000, L)]
        cases += [("device road, 2^%d rows, 1 key, 1 column" % e, 1 << e, 1, False, False) for e in (20, 24, 28) if e <= a.max_log2]
        if a.max_log2 >= 28:
            cases.append(("device road, 2^28 rows, 1 key, 1 column, 1 in 8 selected", 1 << 28, 1, False, True))
        cases.append(("device road, 2^%d rows, 2 keys, 1 column" % min(24, a.max_log2), 1 << min(24, a.max_log2), 2, False, False))
        for name, n, nkeys, wide_sum, masked in cases:
            k, s, pay = columns(n, nkeys, wide_sum)
            words = torch.from_numpy(mask_words(n).view(np.int32)).to(dev) if masked else None
            if wide_sum:                                              # two uint32 keys, the uint64 sum descending; both keys and the sum carried
                keys_t = [(k[0], False), (k[1], False), (s, True)]
                keys_h = [(k[0].data_ptr(), 0), (k[1].data_ptr(), 0), (s.data_ptr(), ORDER_WIDE | ORDER_DESC)]
                cols_t, cols_h = [k[0], k[1], s], [(k[0].data_ptr(), 0), (k[1].data_ptr(), 0), (s.data_ptr(), ORDER_WIDE)]
            else:
                keys_t = [(x, False) for x in k]
                keys_h = [(x.data_ptr(), 0) for x in k]
                cols_t, cols_h = [pay], [(pay.data_ptr(), 0)]
            outs = [torch.empty_like(c) for c in cols_t]
            rows = torch.empty(n, dtype=torch.int32, device=dev)
            ours, theirs = [], []
            for rep in range(a.reps + 1):                            # rep 0: warm-up
                for o in outs + [rows]:
                    o.zero_()
                J = hj.order_by(words.data_ptr() if masked else None, n, keys_h, cols_h, [o.data_ptr() for o in outs], rows.data_ptr(), limit=n)
                st = hj.stats()
                torch.cuda.synchronize()
                ev[0].record()
                perm, want = by_torch(keys_t, cols_t, words, n)
                ev[1].record()
                torch.cuda.synchronize()
                assert J == len(perm), (name, J, len(perm))
                assert bool((rows[:J].to(torch.int64) & 0xFFFFFFFF == perm).all().item()), (name, "row numbers")
                for o, w in zip(outs, want):
                    assert bool((o[:J] == w).all().item()), (name, "a carried column")
                if rep:
                    ours.append((st["ms_total"], st["ms_histogram"], st["ms_join"], st["ms_close_gaps"]))
                    theirs.append(ev[0].elapsed_time(ev[1]))
                del perm, want
            med = lambda f: statistics.median(r[f] for r in ours)     # noqa: E731
            res[name] = {"order_by": med(0), "permutation": med(1), "passes": med(2), "gather": med(3), "torch": statistics.median(theirs), "selected": J}
            del k, s, pay, outs, rows, words
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log2", type=int, default=28, help="the largest device-road case (smaller: a rehearsal)")
    ap.add_argument("--timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for p in range(a.procs):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--max-log2", str(a.max_log2)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                     # nothing more is started behind a process that failed
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if p == 0:
            print("ms, medians of %d calls per process after one untimed call; order_by = hjgpu_get_stats' ms_total = permutation (the initial one) + passes + "
                  "gather; torch = stable sorts from the last key to the first plus index_select per column, by torch events; every result checked against torch's" % a.reps)
        for k, v in runs[-1].items():
            print("process %d: %-58s %s" % (p, k, "  ".join("%s %.3f" % (f, v[f]) if f != "selected" else "selected %d" % v[f] for f in v)), flush=True)
    print("%-58s %9s | %11s %9s %9s | %9s | %14s" % ("median of %d processes" % a.procs, "order_by", "permutation", "passes", "gather", "torch", "order_by/torch"))
    for k in runs[0]:
        m = {f: statistics.median(r[k][f] for r in runs) for f in runs[0][k]}
        print("%-58s %9.3f | %11.3f %9.3f %9.3f | %9.3f | %14.2f" % (k, m["order_by"], m["permutation"], m["passes"], m["gather"], m["torch"], m["order_by"] / m["torch"]))


if __name__ == "__main__":
    main()
