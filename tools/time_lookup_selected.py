#!/usr/bin/env python3
"""Times hjgpu_lookup_selected (values + bits; hjgpu_get_stats ms_total) under masks of several kinds against the plain hjgpu_lookup,
values + bits, on the same columns in the same process - what a caller runs today before ANDing the bitmaps, and never the new code.
The relations come from hjgpu_generate_select at selectivity 0.5 (unique build keys); everything is resident, the first round of calls
is a warm-up that is not timed (it also grows the workspace); the variants alternate in one process.  A build size "L" is the
context's hjgpu_get_counter "lookup_lds_rows" (the LDS road); larger ones take the NPJ road.  The mask's own price is
hjgpu_stream_read_ms of its bytes in the same process.

Masks (the same in every process: seeded): ones; eighth and sixtyfourth - random, every row selected with probability 1/8, 1/64 (the
AND of three, six random bitmaps); clustered - runs of 4096 rows, each run selected with probability 1/8.

usage: python tools/time_lookup_selected.py [--procs 5] [--reps 3] [--inners L,1000000,8000000,64000000] [--outer N] [--timeout SECONDS]
Without --child the script runs, per build size, --procs fresh child processes one after the other, each under its own time limit, and
stops at the first one that fails.  Every call is checked against aggregates computed for its mask: the first child of a build size
computes them with numpy from the downloaded key column and the plain look-up's outputs, the others receive them.  It prints each
child's medians, the medians over the children, the plain look-up's spread (highest minus lowest ms_total of the children), and at the
end the conditions; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASKS = ["ones", "eighth", "sixtyfourth", "clustered"]
RUN = 4096                                                          # rows per run of the clustered mask


def mask_words(kind, outer):
    words = (outer + 31) // 32
    rng = np.random.default_rng(MASKS.index(kind) + 1)
    if kind == "ones":
        return np.full(words, 0xFFFFFFFF, np.uint32)
    if kind == "clustered":
        runs = rng.random((outer + RUN - 1) // RUN) < 0.125
        return np.repeat(np.where(runs, 0xFFFFFFFF, 0).astype(np.uint32), RUN // 32)[:words].copy()
    w = np.full(words, 0xFFFFFFFF, np.uint32)
    for _ in range(3 if kind == "eighth" else 6):
        w &= rng.integers(0, 2**32, size=words, dtype=np.uint64).astype(np.uint32)
    return w


def expected(keys, vals, hit_words, sel_words, outer):
    """count, sum_keys, 0, sum_inner_vals over the rows that are selected and have a match, in pieces of 2^25 rows"""
    both = hit_words & sel_words
    count = sk = sv = 0
    step = 1 << 25
    for lo in range(0, outer, step):
        hi = min(lo + step, outer)
        m = np.unpackbits(both[lo // 32:(hi + 31) // 32].view(np.uint8), bitorder="little")[:hi - lo].astype(bool)
        count += int(m.sum())
        sk += int(keys[lo:hi][m].sum(dtype=np.uint64))
        sv += int(vals[lo:hi][m].sum(dtype=np.uint64))
    return [count, sk & (2**64 - 1), 0, sv & (2**64 - 1)]


def child(a):
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    import hash_join_codes_knl_amd as H
    fi, fo = 0x2545F491, 0x9E3779B1
    with H.HjGpu(0) as hj:
        L = hj.counter("lookup_lds_rows")
        inner = L if a.inner == "L" else int(a.inner)
        lds = inner <= L
        ik, iv, ok, ov = hj.column(inner), hj.column(inner), hj.column(a.outer), hj.column(a.outer)
        exp = tuple(hj.generate_select(1, inner, a.outer, 0, inner, 0, a.outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov))
        ov.free()                                                       # a look-up reads no probe payloads
        vals, bits = hj.column(a.outer, placed=True), hj.column((a.outer + 31) // 32)
        host = {k: mask_words(k, a.outer) for k in MASKS}
        masks = {k: hj.column(w) for k, w in host.items()}
        want = {"plain": [exp[0], exp[1], 0, exp[3]]}
        if a.expect:
            want.update(json.loads(a.expect))
        else:
            assert list(hj.lookup(ik, iv, inner, ok, a.outer, vals_out=vals, match_bits=bits)) == want["plain"]
            keys, pv, pb = ok.download(), vals.download(), bits.download()
            for k in MASKS:
                want[k] = expected(keys, pv, pb, host[k], a.outer)
            del keys, pv, pb
        times = {k: [] for k in ["plain"] + MASKS}
        for rep in range(a.reps + 1):                                   # rep 0: warm-up
            for name in times:
                if name == "plain":
                    got = list(hj.lookup(ik, iv, inner, ok, a.outer, vals_out=vals, match_bits=bits))
                else:
                    got = list(hj.lookup_selected(ik, iv, inner, ok, a.outer, select_bits=masks[name], vals_out=vals, match_bits=bits))
                assert got == want[name], (name, got, want[name])
                st = hj.stats()
                assert st["ms_close_gaps"] == 0
                assert (st["buckets"] == 0 and st["fanout1"] == 1) == lds, (name, st)
                if rep:
                    times[name].append(st["ms_total"])
        mask_ms = statistics.median(hj.stream_read_ms(masks["ones"], masks["ones"].n * 4) for _ in range(a.reps + 1))
    res = {"inner": inner, "lds": lds, "mask_read": mask_ms, "want": {k: want[k] for k in MASKS}}
    res.update({k: statistics.median(v) for k, v in times.items()})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inners", default="L,1000000,8000000,64000000")
    ap.add_argument("--inner", default="0", help="(--child) build rows, or L")
    ap.add_argument("--expect", default="", help="(--child) the masks' expected aggregates, JSON; empty: compute them")
    ap.add_argument("--outer", type=int, default=1_000_000_000)
    ap.add_argument("--timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    conditions = []
    for inner in a.inners.split(","):
        runs, expect = [], ""
        for p in range(a.procs):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                   "--inner", inner, "--outer", str(a.outer), "--expect", expect]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                 # nothing more is started behind a process that failed
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            expect = json.dumps(runs[-1].pop("want"))
            if p == 0:
                print("%d x %d M, selectivity 0.5, %s road; ms_total, medians of %d calls per process; plain = hjgpu_lookup, the others = "
                      "hjgpu_lookup_selected under that mask, all values + bits; mask_read = hjgpu_stream_read_ms of the mask"
                      % (runs[0]["inner"], a.outer // 10**6, "LDS" if runs[0]["lds"] else "NPJ", a.reps))
            print("process %d: %s" % (p, " ".join("%s %.3f" % (k, runs[-1][k]) for k in ["plain"] + MASKS + ["mask_read"])), flush=True)
        med = {k: statistics.median(r[k] for r in runs) for k in ["plain"] + MASKS + ["mask_read"]}
        pp = [r["plain"] for r in runs]
        spread = max(pp) - min(pp)
        selected = {k: int(np.unpackbits(mask_words(k, a.outer).view(np.uint8), bitorder="little")[:a.outer].sum()) for k in MASKS}
        print("%-12s %9s %14s %22s" % ("median of %d" % a.procs, "ms_total", "selected rows", "ns per selected row"))
        print("%-12s %9.3f %14d %22.4f   (lowest %.3f, highest %.3f, spread %.3f)" % ("plain", med["plain"], a.outer, med["plain"] * 1e6 / a.outer,
                                                                                     min(pp), max(pp), spread))
        for k in MASKS:
            print("%-12s %9.3f %14d %22.4f" % (k, med[k], selected[k], med[k] * 1e6 / selected[k]))
        print("%-12s %9.3f" % ("mask_read", med["mask_read"]), flush=True)
        road = "LDS" if runs[0]["lds"] else "NPJ"
        if road == "NPJ" and runs[0]["inner"] == 8_000_000:
            conditions.append(("NPJ road, 8 M build rows, random mask of density 1/8: selected median %.3f <= plain median %.3f - plain spread %.3f"
                               % (med["eighth"], med["plain"], spread), med["eighth"] <= med["plain"] - spread))
            conditions.append(("NPJ road, 8 M build rows, all-ones mask: selected median %.3f <= plain median %.3f + plain spread %.3f + mask read %.3f"
                               % (med["ones"], med["plain"], spread, med["mask_read"]), med["ones"] <= med["plain"] + spread + med["mask_read"]))
        if road == "LDS":
            for k, d in (("ones", "1"), ("eighth", "1/8")):
                conditions.append(("LDS road, %d build rows, density %s: selected median %.3f <= plain median %.3f + plain spread %.3f + mask read %.3f"
                                   % (runs[0]["inner"], d, med[k], med["plain"], spread, med["mask_read"]),
                                   med[k] <= med["plain"] + spread + med["mask_read"]))
    for text, holds in conditions:
        print("condition (%s): %s" % (text, "holds" if holds else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
