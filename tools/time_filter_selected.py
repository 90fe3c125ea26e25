#!/usr/bin/env python3
"""Times hjgpu_filter_selected (hjgpu_get_stats ms_total: the clear of the count word and the kernel) against what a torch caller runs today,
and never the new code: in the same process and on the same columns torch evaluates (c >= lo) & (c <= hi) per predicate, ANDs them to one
bool per row and packs it by a shift-and-sum over a (-1, 32) view into int32 words (ANDed with the mask's words where there is a mask),
timed by torch events.  Beside it: the compares alone, without the pack, and hjgpu_stream_read_ms of the bytes the call must read - the
mask, and every 128-byte column line one of whose rows can still pass (capped at the size of the columns' allocation) - for orientation.

Data: every column and the mask repeat with a period of 2^22 rows that numpy draws from a seeded generator (the same in every process), so
numpy gives the exact count of all rows - whole periods times the period's count plus the remainder's - and the expected words; the device
streams distinct addresses all the same.  Values lie in [0, 2^31): torch's int32 compares and the library's unsigned ones agree.  Every call
is checked: the count, and the first 2^16 words of the bitmap, against numpy; torch's words against the library's, all of them.
Layouts of column 0 (predicate 0 = [0, rate * 2^31 - 1]): pass rates 1, 1/8 and 1/64 at random; clustered - runs of 4096 rows, each run
passing with probability 1/8.  Columns 1 and 2 pass one row in two at random ([0, 2^30 - 1] and [2^29, 2^29 + 2^30 - 1]).
Shapes: 1 and 3 predicates; no mask, and a random mask at density 1/2.

usage: python tools/time_filter_selected.py [--procs 5] [--reps 3] [--rows N] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first round of calls of a process is a warm-up that is not timed.  It prints each child's medians, the medians over the
children, torch's spread (highest minus lowest process), new / read, and at the end the conditions; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PERIOD = 1 << 22                                                    # rows
LAYOUTS = [("rate 1", 1.0), ("rate 1/8", 0.125), ("rate 1/64", 1.0 / 64), ("clustered 1/8", 0.125)]
RUN = 4096                                                          # rows per run of the clustered layout
SAMPLE = 1 << 16                                                    # words compared with numpy
LATER = [(0, (1 << 30) - 1), (1 << 29, (1 << 29) + (1 << 30) - 1)]  # predicates 1 and 2


def period_columns():
    rng = np.random.default_rng(1)
    c = [rng.integers(0, 1 << 31, PERIOD, dtype=np.int64).astype(np.uint32) for _ in range(3)]
    runs = rng.random(PERIOD // RUN) < 0.125                        # the clustered column 0: a run's rows all below, or all above, the bound
    low = rng.integers(0, 1 << 28, PERIOD, dtype=np.int64)
    clustered = np.where(np.repeat(runs, RUN), low, low + (1 << 28)).astype(np.uint32)
    mask = rng.integers(0, 1 << 32, PERIOD // 32, dtype=np.uint64).astype(np.uint32)
    return c, clustered, mask


def tiled(period, n, torch, dev):
    """a device tensor of n int32 that repeats the host period"""
    p = torch.from_numpy(period.view(np.int32)).to(dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    full = n // len(period)
    out[:full * len(period)].view(full, len(period))[:] = p
    out[full * len(period):] = p[:n - full * len(period)]
    return out


def total(per_period, n, unit):
    """the sum over n rows of a per-unit array (unit rows per element) that repeats with the period"""
    full, rem = divmod(n, PERIOD)
    return full * int(per_period.sum(dtype=np.int64)) + int(per_period[:rem // unit].sum(dtype=np.int64))


def child(a):
    import torch
    torch.cuda.init()
    import hash_join_codes_knl_amd as H
    n = a.rows
    assert n % 32 == 0 and n >= 32 * SAMPLE, "--rows must be a multiple of 32 and at least 2^21"
    dev = torch.device("cuda")
    hc, hclustered, hmask = period_columns()
    cols = torch.empty(3 * n, dtype=torch.int32, device=dev)         # the three columns, one allocation
    for c in range(3):
        cols[c * n:(c + 1) * n] = tiled(hc[c], n, torch, dev)
    col = [cols[c * n:(c + 1) * n] for c in range(3)]
    words = tiled(hmask, n // 32, torch, dev)
    out = torch.empty(n // 32, dtype=torch.int32, device=dev)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    res = {}
    with H.HjGpu(0) as hj:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for layout, rate in LAYOUTS:
            h0 = hc[0]
            if layout.startswith("clustered"):
                col[0][:] = tiled(hclustered, n, torch, dev)
                h0 = hclustered
            hcols = [h0, hc[1], hc[2]]
            for npreds in (1, 3):
                preds = [(0, int(rate * (1 << 31)) - 1)] + LATER[:npreds - 1]
                for masked in (False, True):
                    # numpy, over one period: the rows that pass, and the lines whose rows can still pass in front of every column
                    alive = np.unpackbits(hmask.view(np.uint8), bitorder="little").astype(bool) if masked else np.ones(PERIOD, bool)
                    lines = []
                    for x, (lo, hi) in zip(hcols, preds):
                        lines.append(alive.reshape(-1, 32).any(axis=1))
                        alive = alive & (x >= lo) & (x <= hi)
                    want_count = total(alive, n, 1)
                    want_words = np.packbits(alive[:32 * SAMPLE], bitorder="little").view(np.uint32)
                    read_bytes = (n // 8 if masked else 0) + sum(128 * total(l, n, 32) for l in lines)
                    t_new, t_torch, t_cmp = [], [], []
                    for rep in range(a.reps + 1):                   # rep 0: warm-up
                        got = hj.filter_selected(words.data_ptr() if masked else None, n, [x.data_ptr() for x in col[:npreds]], preds, out.data_ptr())
                        st = hj.stats()
                        assert got == want_count, (layout, npreds, masked, got, want_count)
                        assert np.array_equal(out[:SAMPLE].cpu().numpy().view(np.uint32), want_words), (layout, npreds, masked, "words")
                        ev[0].record()
                        m = (col[0] >= preds[0][0]) & (col[0] <= preds[0][1])
                        for x, (lo, hi) in zip(col[1:npreds], preds[1:]):
                            m &= (x >= lo) & (x <= hi)
                        ev[1].record()
                        packed = (m.view(-1, 32).to(torch.int32) << shifts).sum(dim=1, dtype=torch.int32)
                        if masked:
                            packed &= words
                        ev[2].record()
                        torch.cuda.synchronize()
                        assert torch.equal(packed, out), (layout, npreds, masked, "torch's words differ")
                        del m, packed
                        if rep:
                            t_new.append(st["ms_total"])
                            t_torch.append(ev[0].elapsed_time(ev[2]))
                            t_cmp.append(ev[0].elapsed_time(ev[1]))
                    read_ms = statistics.median(hj.stream_read_ms(cols.data_ptr(), min(read_bytes, 12 * n) // 65536 * 65536) for _ in range(a.reps))
                    res["%s, %d pred%s, %s" % (layout, npreds, "s" if npreds > 1 else "", "mask 1/2" if masked else "no mask")] = {
                        "new": statistics.median(t_new), "torch": statistics.median(t_torch), "compares": statistics.median(t_cmp),
                        "read_ms": read_ms, "passing": want_count, "bytes": read_bytes}
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
            print("%d rows; ms, medians of %d calls per process after one untimed round; new = hjgpu_filter_selected ms_total, torch = compares ANDed to "
                  "a bool + shift-and-sum pack into int32 words (& the mask's words), compares = the same without the pack, read = "
                  "hjgpu_stream_read_ms of the bytes the call must read" % (a.rows, a.reps))
        for k, v in runs[-1].items():
            print("process %d: %-40s new %8.3f torch %8.3f compares %8.3f read %7.3f" % (p, k, v["new"], v["torch"], v["compares"], v["read_ms"]), flush=True)
    print("%-40s %12s %9s %9s %9s %9s %8s %9s %7s" % ("median of %d processes" % a.procs, "passing", "new", "torch", "spread", "compares", "read", "new/read", "TB/s"))
    med = {}
    for k in runs[0]:
        tt = [r[k]["torch"] for r in runs]
        med[k] = {f: statistics.median(r[k][f] for r in runs) for f in ("new", "torch", "compares", "read_ms")}
        med[k]["spread"] = max(tt) - min(tt)
        print("%-40s %12d %9.3f %9.3f %9.3f %9.3f %8.3f %9.2f %7.2f" % (k, runs[0][k]["passing"], med[k]["new"], med[k]["torch"], med[k]["spread"],
                                                                       med[k]["compares"], med[k]["read_ms"], med[k]["new"] / med[k]["read_ms"],
                                                                       runs[0][k]["bytes"] / med[k]["new"] / 1e9))
    for layout in ("rate 1/8", "rate 1"):
        for mask in ("no mask", "mask 1/2"):
            v = med["%s, 3 preds, %s" % (layout, mask)]
            holds = v["new"] <= v["torch"] - v["spread"]
            print("condition (3 predicates, %s, %s: new median %.3f <= torch median %.3f - torch spread %.3f): %s"
                  % (layout, mask, v["new"], v["torch"], v["spread"], "holds" if holds else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
