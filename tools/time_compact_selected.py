#!/usr/bin/env python3
"""Times hjgpu_compact_selected (hjgpu_get_stats ms_total: the counting launch and the compaction) against what a caller runs today, and never
the new code: in the same process and on the same columns torch runs masked_select once per column on a bool mask that was prepared outside
the timed span (the row numbers, where asked for, are torch.nonzero of that mask), timed by torch events.  Beside it: the same torch calls
with the unpacking of the bitmap to bool inside the span, and hjgpu_stream_read_ms of the bytes the call must read (the mask twice and every
128-byte line of every column whose mask word is not 0; capped at the size of the input columns' allocation) - for orientation only.

Columns: column c holds (row * odd_c + c) mod 2^32, so any output can be checked without its input.  Every call is checked: the count against
the popcount of the mask, and the sum of the first 2^16 rows of every output (the row numbers included) against numpy.
Masks (seeded: the same in every process): ones; half, eighth, sixtyfourth - random, every row selected with probability 1/2, 1/8, 1/64 (the
AND of one, three, six random bitmaps); clustered - runs of 4096 rows, each run selected with probability 1/8.
Shapes: 1 column; 3 columns; 3 columns and the row numbers.

usage: python tools/time_compact_selected.py [--procs 5] [--reps 3] [--rows N] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first round of calls of a process is a warm-up that is not timed.  It prints each child's medians, the medians over the
children, torch's spread (highest minus lowest process), the achieved TB/s, and at the end the conditions; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASKS = ["ones", "half", "eighth", "sixtyfourth", "clustered"]
SHAPES = [("1col", 1, False), ("3cols", 3, False), ("3cols+rows", 3, True)]
MULT = [0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35]
RUN = 4096                                                          # rows per run of the clustered mask
SAMPLE = 1 << 16


def mask_words(kind, n):
    words = (n + 31) // 32
    rng = np.random.default_rng(MASKS.index(kind) + 1)
    if kind == "ones":
        return np.full(words, 0xFFFFFFFF, np.uint32)
    if kind == "clustered":
        runs = rng.random((n + RUN - 1) // RUN) < 0.125
        return np.repeat(np.where(runs, 0xFFFFFFFF, 0).astype(np.uint32), RUN // 32)[:words].copy()
    w = np.full(words, 0xFFFFFFFF, np.uint32)
    for _ in range({"half": 1, "eighth": 3, "sixtyfourth": 6}[kind]):
        w &= rng.integers(0, 2**32, size=words, dtype=np.uint64).astype(np.uint32)
    return w


def popcount(words):
    total = 0
    for lo in range(0, len(words), 1 << 22):
        total += int(np.unpackbits(words[lo:lo + (1 << 22)].view(np.uint8)).sum(dtype=np.int64))
    return total


def child(a):
    import torch
    torch.cuda.init()
    import hash_join_codes_knl_amd as H
    n = a.rows
    assert n % 32 == 0, "--rows must be a multiple of 32 (whole mask words, 16-byte aligned columns in one allocation)"
    dev = torch.device("cuda")
    cols = torch.empty(3 * n, dtype=torch.int32, device=dev)         # the three input columns, one allocation
    step = 1 << 26
    for c in range(3):
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            cols[c * n + lo:c * n + hi] = (torch.arange(lo, hi, dtype=torch.int64, device=dev) * MULT[c] + c).to(torch.int32)
    col = [cols[c * n:(c + 1) * n] for c in range(3)]
    outs = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)]
    rows_out = torch.empty(n, dtype=torch.int32, device=dev)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    res = {}
    with H.HjGpu(0) as hj:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for kind in MASKS:
            host = mask_words(kind, n)
            J = popcount(host)
            live = int(np.count_nonzero(host))                       # 32-row groups with a selected row: their lines are read
            first = np.flatnonzero(np.unpackbits(host[:SAMPLE].view(np.uint8), bitorder="little"))[:SAMPLE].astype(np.uint64)
            m = min(len(first), J)
            want = [int(((first[:m] * MULT[c] + c) & 0xFFFFFFFF).sum(dtype=np.uint64)) for c in range(3)] + [int(first[:m].sum(dtype=np.uint64))]
            words = torch.from_numpy(host.view(np.int32)).to(dev)

            def unpack():
                return ((words.view(-1, 1) >> shifts) & 1).view(-1)[:n].bool()
            mask = unpack()
            for name, ncols, rows in SHAPES:
                t_new, t_torch, t_unpack = [], [], []
                for rep in range(a.reps + 1):                       # rep 0: warm-up
                    got = hj.compact_selected(words.data_ptr(), n, [x.data_ptr() for x in col[:ncols]], [x.data_ptr() for x in outs[:ncols]],
                                              rows_out.data_ptr() if rows else None, capacity=n)
                    st = hj.stats()
                    assert got == J, (kind, name, got, J)
                    for c in range(ncols):
                        assert int(outs[c][:m].to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) == want[c], (kind, name, c)
                    if rows:
                        assert int(rows_out[:m].to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) == want[3], (kind, name, "rows")
                    ev[0].record()
                    mask2 = unpack()
                    ev[1].record()
                    sel = [torch.masked_select(x, mask) for x in col[:ncols]]
                    if rows:
                        sel.append(torch.nonzero(mask).flatten())
                    ev[2].record()
                    torch.cuda.synchronize()
                    assert all(len(x) == J for x in sel) and bool((mask2 == mask).all().item())
                    del sel, mask2
                    if rep:
                        t_new.append(st["ms_total"])
                        t_torch.append(ev[1].elapsed_time(ev[2]))
                        t_unpack.append(ev[0].elapsed_time(ev[2]))
                read_bytes = 2 * host.nbytes + ncols * live * 128
                moved = read_bytes + 4 * (ncols + (1 if rows else 0)) * J
                read_ms = statistics.median(hj.stream_read_ms(cols.data_ptr(), min(read_bytes, 12 * n) // 65536 * 65536) for _ in range(a.reps))
                res[kind + " " + name] = {"new": statistics.median(t_new), "torch": statistics.median(t_torch),
                                          "torch_unpack": statistics.median(t_unpack), "read_ms": read_ms, "selected": J, "bytes": moved}
            del mask, words
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
            print("%d rows; ms, medians of %d calls per process after one untimed round; new = hjgpu_compact_selected ms_total, torch = masked_select "
                  "per column (+ nonzero for the row numbers) on a prepared bool mask, +unpack = the same with the bitmap's unpacking inside the span, "
                  "read = hjgpu_stream_read_ms of the bytes the call must read" % (a.rows, a.reps))
        for k, v in runs[-1].items():
            print("process %d: %-24s new %8.3f torch %8.3f +unpack %8.3f read %7.3f" % (p, k, v["new"], v["torch"], v["torch_unpack"], v["read_ms"]), flush=True)
    print("%-24s %12s %9s %9s %9s %9s %8s %7s" % ("median of %d processes" % a.procs, "selected", "new", "torch", "spread", "+unpack", "read", "TB/s"))
    med = {}
    for k in runs[0]:
        tt = [r[k]["torch"] for r in runs]
        med[k] = {f: statistics.median(r[k][f] for r in runs) for f in ("new", "torch", "torch_unpack", "read_ms")}
        med[k]["spread"] = max(tt) - min(tt)
        print("%-24s %12d %9.3f %9.3f %9.3f %9.3f %8.3f %7.2f" % (k, runs[0][k]["selected"], med[k]["new"], med[k]["torch"], med[k]["spread"],
                                                                 med[k]["torch_unpack"], med[k]["read_ms"], runs[0][k]["bytes"] / med[k]["new"] / 1e9))
    for kind, d in (("half", "1/2"), ("eighth", "1/8")):
        v = med[kind + " 3cols"]
        holds = v["new"] <= v["torch"] - v["spread"]
        print("condition (3 columns, density %s: new median %.3f <= torch median %.3f - torch spread %.3f): %s"
              % (d, v["new"], v["torch"], v["spread"], "holds" if holds else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
