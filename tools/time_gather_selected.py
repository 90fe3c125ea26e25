#!/usr/bin/env python3
"""Times hjgpu_gather_selected (hjgpu_get_stats ms_total: the clear of the count words and the kernel) against what a torch caller runs
today, and never the new code: in the same process and on the same buffers torch views the row numbers as int32 (HJGPU_NULL_VAL is -1
there), clamps them with `where` (under a mask: after unpacking the mask's words to one bool per row), runs index_select per column, puts
the NULLs back with a second `where` per column and packs the gathered rows' bitmap by the filter tool's shift-and-sum over a (-1, 32) view
- timed by torch events.  Beside it, for orientation: "read" = hjgpu_stream_read_ms over as many bytes as the call streams (the index, the
mask, the written columns and bitmap), and for the large source "lines" = hjgpu_random_line_read_ms of gathered x ncols independent line
reads out of the source columns' allocation - what the element-granular gather costs as memory-side requests.

Data: the index and the mask repeat with a period of 2^22 rows that numpy draws from a seeded generator (the same in every process): row
numbers uniform in [0, src_rows), a NULL share of them replaced by HJGPU_NULL_VAL; the mask at density 1/2.  So numpy gives every call's
exact counts - whole periods times the period's count plus the remainder's -, and every call is checked against them: the counts, the first
2^16 rows of every output column and the bitmap's first words against numpy (source column c holds row * an odd constant of its own modulo
2^32), and torch's columns and words against the library's, all of them.
Shapes: 1, 2 and 4 columns; no mask and a random mask at density 1/2; NULL share 0 and 1/8; sources of 2^20 rows (a dimension that the
caches hold) and of 2^30 rows (random lines from HBM).

usage: python tools/time_gather_selected.py [--procs 5] [--reps 3] [--rows N] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first round of calls of a process is a warm-up that is not timed.  It prints each child's medians, the medians over the
children, torch's spread (highest minus lowest process), new / read, new / lines, and at the end the conditions; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PERIOD = 1 << 22                                                    # rows
SAMPLE = 1 << 16                                                    # rows compared with numpy
NULL = 0xFFFFFFFF
MULT = [0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F]             # source column c holds row * MULT[c] mod 2^32 (odd constants)
SOURCES = [("2^20", 1 << 20), ("2^30", 1 << 30)]
NULL_SHARES = [("0", 0.0), ("1/8", 0.125)]


def period_data(src_rows, share):
    rng = np.random.default_rng(1)
    idx = rng.integers(0, src_rows, PERIOD, dtype=np.int64).astype(np.uint32)
    idx[rng.random(PERIOD) < share] = NULL
    mask = rng.integers(0, 1 << 32, PERIOD // 32, dtype=np.uint64).astype(np.uint32)
    return idx, mask


def tiled(period, n, torch, dev):
    """a device tensor of n int32 that repeats the host period"""
    p = torch.from_numpy(period.view(np.int32)).to(dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    full = n // len(period)
    out[:full * len(period)].view(full, len(period))[:] = p
    out[full * len(period):] = p[:n - full * len(period)]
    return out


def total(per_row, n):
    """the sum over n rows of a per-row array that repeats with the period"""
    full, rem = divmod(n, PERIOD)
    return full * int(per_row.sum(dtype=np.int64)) + int(per_row[:rem].sum(dtype=np.int64))


def child(a):
    import torch
    torch.cuda.init()
    import hash_join_codes_knl_amd as H
    n = a.rows
    assert n % 32 == 0 and n >= SAMPLE, "--rows must be a multiple of 32 and at least 2^16"
    dev = torch.device("cuda")
    arena = torch.empty(9 * n, dtype=torch.int32, device=dev)       # the index, four output columns, torch's four: one allocation to stream over
    idx, outs, touts = arena[:n], [arena[(1 + c) * n:(2 + c) * n] for c in range(4)], [arena[(5 + c) * n:(6 + c) * n] for c in range(4)]
    bits = torch.empty(n // 32, dtype=torch.int32, device=dev)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    null = torch.full((), -1, dtype=torch.int32, device=dev)        # HJGPU_NULL_VAL as int32
    res = {}
    with H.HjGpu(0) as hj:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for sname, src_rows in SOURCES:
            srcs = torch.empty(4 * src_rows, dtype=torch.int32, device=dev)
            src = [srcs[c * src_rows:(c + 1) * src_rows] for c in range(4)]
            for c in range(4):                                      # row * MULT[c] mod 2^32: int32 arithmetic wraps
                src[c].copy_(torch.arange(src_rows, dtype=torch.int32, device=dev))
                src[c].mul_(MULT[c] - (1 << 32) if MULT[c] >> 31 else MULT[c])
            for share_name, share in NULL_SHARES:
                hidx, hmask = period_data(src_rows, share)
                idx[:] = tiled(hidx, n, torch, dev)
                words = tiled(hmask, n // 32, torch, dev)
                hsel = np.unpackbits(hmask.view(np.uint8), bitorder="little").astype(bool)
                for masked in (False, True):
                    good = (hidx != NULL) & (hsel if masked else True)
                    want_count = total(good, n)
                    want_words = np.packbits(good[:SAMPLE], bitorder="little").view(np.uint32)
                    for ncols in (1, 2, 4):
                        want_cols = [np.where(good[:SAMPLE], (hidx[:SAMPLE].astype(np.uint64) * np.uint64(MULT[c])).astype(np.uint32), NULL).astype(np.uint32)
                                     for c in range(ncols)]
                        t_new, t_torch = [], []
                        for rep in range(a.reps + 1):               # rep 0: warm-up
                            got = hj.gather_selected(words.data_ptr() if masked else None, idx.data_ptr(), n, [s.data_ptr() for s in src[:ncols]], src_rows,
                                                     [o.data_ptr() for o in outs[:ncols]], bits.data_ptr())
                            st = hj.stats()
                            what = (sname, share_name, masked, ncols)
                            assert got == (want_count, 0), (what, got, want_count)
                            assert np.array_equal(bits[:SAMPLE // 32].cpu().numpy().view(np.uint32), want_words), (what, "words")
                            for c in range(ncols):
                                assert np.array_equal(outs[c][:SAMPLE].cpu().numpy().view(np.uint32), want_cols[c]), (what, "column", c)
                            ev[0].record()
                            valid = idx >= 0                        # (HJGPU_NULL_VAL is -1 as int32; every row number is below 2^31)
                            if masked:
                                valid &= ((words.view(-1, 1) >> shifts) & 1).view(-1).to(torch.bool)
                            safe = torch.where(valid, idx, 0)
                            for c in range(ncols):
                                torch.where(valid, src[c].index_select(0, safe), null, out=touts[c])
                            packed = (valid.view(-1, 32).to(torch.int32) << shifts).sum(dim=1, dtype=torch.int32)
                            ev[1].record()
                            torch.cuda.synchronize()
                            assert all(torch.equal(touts[c], outs[c]) for c in range(ncols)) and torch.equal(packed, bits), (what, "torch's columns or words differ")
                            del valid, safe, packed
                            if rep:
                                t_new.append(st["ms_total"])
                                t_torch.append(ev[0].elapsed_time(ev[1]))
                        streamed = 4 * n + (n // 8 if masked else 0) + 4 * n * ncols + n // 8
                        read_ms = statistics.median(hj.stream_read_ms(arena.data_ptr(), min(streamed, 24 * n) // 65536 * 65536) for _ in range(a.reps))
                        lines_ms = None
                        if src_rows > 1 << 24:
                            lines_ms = statistics.median(hj.random_line_read_ms(srcs.data_ptr(), 4 * src_rows * ncols, want_count * ncols) for _ in range(a.reps))
                        res["src %s, %d col%s, %s, NULL %s" % (sname, ncols, "s" if ncols > 1 else "", "mask 1/2" if masked else "no mask", share_name)] = {
                            "new": statistics.median(t_new), "torch": statistics.median(t_torch), "read_ms": read_ms, "lines_ms": lines_ms,
                            "gathered": want_count, "bytes": streamed}
            del srcs, src
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
            print("%d rows; ms, medians of %d calls per process after one untimed round; new = hjgpu_gather_selected ms_total, torch = where + "
                  "index_select per column + where + shift-and-sum pack, read = hjgpu_stream_read_ms of the streamed bytes, lines = "
                  "hjgpu_random_line_read_ms of gathered x ncols line reads (large source)" % (a.rows, a.reps))
        for k, v in runs[-1].items():
            print("process %d: %-48s new %9.3f torch %9.3f read %8.3f lines %s" % (p, k, v["new"], v["torch"], v["read_ms"],
                                                                                  "%8.3f" % v["lines_ms"] if v["lines_ms"] is not None else "       -"), flush=True)
    print("%-48s %12s %9s %9s %9s %8s %9s %9s %10s" % ("median of %d processes" % a.procs, "gathered", "new", "torch", "spread", "read", "new/read", "lines", "new/lines"))
    med = {}
    for k in runs[0]:
        tt = [r[k]["torch"] for r in runs]
        med[k] = {f: statistics.median(r[k][f] for r in runs) for f in ("new", "torch", "read_ms")}
        med[k]["spread"] = max(tt) - min(tt)
        lines = statistics.median(r[k]["lines_ms"] for r in runs) if runs[0][k]["lines_ms"] is not None else None
        print("%-48s %12d %9.3f %9.3f %9.3f %8.3f %9.2f %9s %10s" % (k, runs[0][k]["gathered"], med[k]["new"], med[k]["torch"], med[k]["spread"], med[k]["read_ms"],
                                                                    med[k]["new"] / med[k]["read_ms"], "%9.3f" % lines if lines is not None else "-",
                                                                    "%10.2f" % (med[k]["new"] / lines) if lines is not None else "-"))
    for sname, _ in SOURCES:
        v = med["src %s, 2 cols, no mask, NULL 1/8" % sname]
        holds = v["new"] <= v["torch"] - v["spread"]
        print("condition (2 columns, source of %s rows, no mask, NULL share 1/8: new median %.3f <= torch median %.3f - torch spread %.3f): %s"
              % (sname, v["new"], v["torch"], v["spread"], "holds" if holds else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
