#!/usr/bin/env python3
"""Times hjgpu_group_agg (hjgpu_get_stats: ms_join = the aggregation kernel, ms_total = the clears, the aggregation and the emit) in three
comparisons, every one taken in the same process and on the same columns as its yardstick (tools/time_group_sum.py's columns and masks):

  1. the cost of generality   hjgpu_group_agg with one unsigned SUM against hjgpu_group_sum with one measure, two key columns, alternating
                              call by call, for 1, 7, 1000 and G ("group_lds_groups") groups;
  2. the scalar road          nkeys == 0 with one SUM, one SUM(a * b) and all four functions, against hjgpu_stream_read_ms over the bytes
                              the call must read, and the SUM against hjgpu_group_sum over an all-zero key column - the only way to a
                              scalar aggregate inside the library without it;
  3. against leaving          SUM(a * b) and MIN + MAX with two keys at 1000 groups against hjgpu_compact_selected plus torch (the int64
                              product, torch.unique, index_add_ / scatter_reduce), timed by torch events around all of it.

Columns: row i belongs to group id(i) = ((i * 0x9E3779B1) mod 2^32) mod D with the keys (3 id + 1, id xor 0x5A5A5A5A), a = (i * 0x85EBCA6B + 5)
mod 2^32 and b = (i * 0xC2B2AE35 + 7) mod 2^32.  Masks (seeded: the same in every process): eighth - every row selected with probability
1/8; ones - every row, through a mask of all-ones words.
Every call is checked: the group count, the sum of the counts against the popcount of the mask, and every aggregate against torch's own
value over the selected rows - the totals for the grouped calls of parts 1 and 3 (modulo 2^64 for the sums, the overall extreme for MIN and
MAX), the values themselves on the scalar road, and in part 3's timed round the sorted rows against the rows of the torch yardstick.

usage: python tools/time_group_agg.py [--procs 5] [--reps 3] [--rows N] [--timeout SECONDS] [--parts 123]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first round of calls of a process is a warm-up that is not timed.  It prints each child's medians and, per row, the median
over the children and hjgpu_group_sum's own min-to-max spread over them (part 1's margin); it only prints."""
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
    cols = torch.empty(4 * n, dtype=torch.int32, device=dev)         # key 0, key 1, a, b: one allocation
    k0, k1, va, vb = cols[:n], cols[n:2 * n], cols[2 * n:3 * n], cols[3 * n:]
    step = 1 << 26
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        i = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        va[lo:hi] = (i * M_A + 5).to(torch.int32)
        vb[lo:hi] = (i * M_B + 7).to(torch.int32)
    del i
    u32 = lambda t: t.to(torch.int64) & 0xFFFFFFFF                    # noqa: E731
    kout = [torch.empty(CAPACITY, dtype=torch.int32, device=dev) for _ in range(2)]
    cout = torch.empty(CAPACITY, dtype=torch.int64, device=dev)
    aout = [torch.empty(CAPACITY, dtype=torch.int64, device=dev) for _ in range(4)]
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    SUM, MUL, MIN, MAX = H.AGG_SUM, H.AGG_SUM_MUL, H.AGG_MIN, H.AGG_MAX
    res = {}

    def fill_keys(D):
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            ids = ((torch.arange(lo, hi, dtype=torch.int64, device=dev) * M_ID) & 0xFFFFFFFF) % D
            k0[lo:hi] = (ids * 3 + 1).to(torch.int32)
            k1[lo:hi] = (ids ^ 0x5A5A5A5A).to(torch.int32)

    with H.HjGpu(0) as hj:
        G = hj.counter("group_lds_groups")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        masks = {}
        for kind in MASKS:                                            # the masks and torch's own totals over the selected rows
            host = mask_words(kind, n)
            words = torch.from_numpy(host.view(np.int32)).to(dev)
            t = dict(selected=0, sum_a=0, sum_ab=0, min_a=1 << 32, max_a=-1, max_b=-1)
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                m = ((words[lo // 32:hi // 32].view(-1, 1) >> shifts) & 1).view(-1).bool()
                x, y = u32(va[lo:hi])[m], u32(vb[lo:hi])[m]
                t["selected"] += int(m.sum().item())
                t["sum_a"] += int(x.sum().item())
                t["sum_ab"] += int((x * y).sum().item()) & M64         # (the products wrap in int64 as they do modulo 2^64)
                t["min_a"], t["max_a"], t["max_b"] = min(t["min_a"], int(x.min().item())), max(t["max_a"], int(x.max().item())), max(t["max_b"], int(y.max().item()))
            del m, x, y
            t["sum_a"] &= M64
            t["sum_ab"] &= M64
            masks[kind] = (words, host.nbytes, t)
        total_u64 = lambda x, J: int(x[:J].sum().item()) & M64         # noqa: E731
        kptr, optr = [k0.data_ptr(), k1.data_ptr()], [x.data_ptr() for x in kout]

        if "1" in a.parts:
            for D in (1, 7, 1000, G):
                fill_keys(D)
                for kind in MASKS:
                    words, _, t = masks[kind]
                    times = {"sum": [], "agg": []}
                    for rep in range(a.reps + 1):                    # rep 0: warm-up
                        for which in ("sum", "agg"):
                            if which == "sum":
                                J = hj.group_sum(words.data_ptr(), n, kptr, [va.data_ptr()], optr, [aout[0].data_ptr()], cout.data_ptr(), capacity=CAPACITY)
                            else:
                                J = hj.group_agg(words.data_ptr(), n, kptr, [(SUM, va.data_ptr())], optr, [aout[0].data_ptr()], cout.data_ptr(), capacity=CAPACITY)
                            st = hj.stats()
                            assert J == D and total_u64(cout, J) == t["selected"] and total_u64(aout[0], J) == t["sum_a"], (which, D, kind)
                            if rep:
                                times[which].append((st["ms_join"], st["ms_total"]))
                    res["1: %d groups, %s" % (D, kind)] = {"sum_join": statistics.median(x[0] for x in times["sum"]), "sum_total": statistics.median(x[1] for x in times["sum"]),
                                                          "agg_join": statistics.median(x[0] for x in times["agg"]), "agg_total": statistics.median(x[1] for x in times["agg"])}

        if "2" in a.parts:
            k0.zero_()                                                # the yardstick's constant key column
            shapes = [("SUM", [(SUM, va.data_ptr())], 1), ("SUM_MUL", [(MUL, va.data_ptr(), vb.data_ptr())], 2),
                      ("all four", [(SUM, va.data_ptr()), (MUL, va.data_ptr(), vb.data_ptr()), (MIN, va.data_ptr()), (MAX, vb.data_ptr())], 2)]
            for kind in MASKS:
                words, mask_bytes, t = masks[kind]
                for name, aggs, ncols in shapes:
                    times, via = [], []
                    for rep in range(a.reps + 1):
                        J = hj.group_agg(words.data_ptr(), n, [], aggs, [], [x.data_ptr() for x in aout[:len(aggs)]], cout.data_ptr(), capacity=CAPACITY)
                        st = hj.stats()
                        got = [int(x[0].item()) & M64 for x in aout[:len(aggs)]]
                        want = {"SUM": [t["sum_a"]], "SUM_MUL": [t["sum_ab"]], "all four": [t["sum_a"], t["sum_ab"], t["min_a"], t["max_b"]]}[name]
                        assert J == 1 and int(cout[0].item()) == t["selected"] and got == want, (name, kind, got, want)
                        if rep:
                            times.append((st["ms_join"], st["ms_total"]))
                        if name == "SUM":                             # today: hjgpu_group_sum over the all-zero key column
                            J = hj.group_sum(words.data_ptr(), n, kptr[:1], [va.data_ptr()], optr[:1], [aout[0].data_ptr()], cout.data_ptr(), capacity=CAPACITY)
                            st = hj.stats()
                            assert J == 1 and int(cout[0].item()) == t["selected"] and int(aout[0][0].item()) & M64 == t["sum_a"], (kind, "constant key")
                            if rep:
                                via.append((st["ms_join"], st["ms_total"]))
                    # as many bytes as the call must read - the mask and its columns - from the head of the columns' allocation
                    read_ms = statistics.median(hj.stream_read_ms(cols.data_ptr(), (mask_bytes + 4 * n * ncols) // 65536 * 65536) for _ in range(a.reps))
                    row = {"agg_join": statistics.median(x[0] for x in times), "agg_total": statistics.median(x[1] for x in times), "read_ms": read_ms}
                    if via:
                        row.update(sum_join=statistics.median(x[0] for x in via), sum_total=statistics.median(x[1] for x in via))
                    res["2: scalar %s, %s" % (name, kind)] = row

        if "3" in a.parts:
            D = 1000
            fill_keys(D)
            dense = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]      # the yardstick's compacted columns
            for kind in MASKS:
                words, _, t = masks[kind]
                for name, aggs in (("SUM_MUL", [(MUL, va.data_ptr(), vb.data_ptr())]), ("MIN+MAX", [(MIN, va.data_ptr()), (MAX, vb.data_ptr())])):
                    times, today = [], []
                    for rep in range(a.reps + 1):
                        J = hj.group_agg(words.data_ptr(), n, kptr, aggs, optr, [x.data_ptr() for x in aout[:len(aggs)]], cout.data_ptr(), capacity=CAPACITY)
                        st = hj.stats()
                        assert J == D and total_u64(cout, J) == t["selected"], (name, kind)
                        if name == "SUM_MUL":
                            assert total_u64(aout[0], J) == t["sum_ab"], (name, kind)
                        else:
                            assert int(aout[0][:J].min().item()) == t["min_a"] and int(aout[1][:J].max().item()) == t["max_b"], (name, kind)
                        if rep:
                            times.append((st["ms_join"], st["ms_total"]))
                        if rep <= 1:                                  # the yardstick: one warm-up, one timed round
                            ev[0].record()
                            got = hj.compact_selected(words.data_ptr(), n, kptr + [va.data_ptr(), vb.data_ptr()], [x.data_ptr() for x in dense], capacity=n)
                            key = u32(dense[0][:got]) | (dense[1][:got].to(torch.int64) << 32)
                            uniq, inv = torch.unique(key, return_inverse=True)
                            if name == "SUM_MUL":
                                mine = [torch.zeros(len(uniq), dtype=torch.int64, device=dev).index_add_(0, inv, u32(dense[2][:got]) * u32(dense[3][:got]))]
                            else:
                                mine = [torch.full((len(uniq),), 1 << 32, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, u32(dense[2][:got]), "amin"),
                                        torch.full((len(uniq),), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, u32(dense[3][:got]), "amax")]
                            ev[1].record()
                            torch.cuda.synchronize()
                            assert got == t["selected"] and len(uniq) == D
                            if rep:
                                today.append(ev[0].elapsed_time(ev[1]))
                                tup = u32(kout[0][:J]) | (kout[1][:J].to(torch.int64) << 32)
                                order = torch.argsort(tup)
                                assert bool((tup[order] == uniq).all().item()), (name, kind, "tuples")
                                for x, y in zip(aout, mine):
                                    assert bool((x[:J][order] == y).all().item()), (name, kind, "rows")
                            del key, uniq, inv, mine
                    res["3: %s, %d groups, %s" % (name, D, kind)] = {"agg_join": statistics.median(x[0] for x in times), "agg_total": statistics.median(x[1] for x in times),
                                                                  "today": statistics.median(today)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--parts", default="123")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for p in range(a.procs):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rows", str(a.rows), "--parts", a.parts]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                     # nothing more is started behind a process that failed
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if p == 0:
            print("%d rows; ms, medians of %d calls per process after one untimed round; join = ms_join (the aggregation kernel), total = ms_total; "
                  "agg = hjgpu_group_agg, sum = hjgpu_group_sum on the same columns (part 2: over an all-zero key column), read = hjgpu_stream_read_ms "
                  "of the mask and the aggregates' columns, today = hjgpu_compact_selected + torch (one timed round per process)" % (a.rows, a.reps))
        for k, v in runs[-1].items():
            print("process %d: %-34s %s" % (p, k, "  ".join("%s %.3f" % (f, v[f]) for f in v)), flush=True)
    print("%-34s %9s %9s %9s %9s %19s %8s %10s" % ("median of %d processes" % a.procs, "agg join", "agg total", "sum join", "sum total", "sum total min..max", "read", "today"))
    for k in runs[0]:
        med = {f: statistics.median(r[k][f] for r in runs) for f in runs[0][k]}
        spread = "%.3f..%.3f" % (min(r[k]["sum_total"] for r in runs), max(r[k]["sum_total"] for r in runs)) if "sum_total" in med else "-"
        cell = lambda f: "%9.3f" % med[f] if f in med else "%9s" % "-"      # noqa: E731
        print("%-34s %s %s %s %s %19s %s %s" % (k, cell("agg_join"), cell("agg_total"), cell("sum_join"), cell("sum_total"), spread,
                                                  ("%8.3f" % med["read_ms"]) if "read_ms" in med else "%8s" % "-", ("%10.3f" % med["today"]) if "today" in med else "%10s" % "-"))


if __name__ == "__main__":
    main()
