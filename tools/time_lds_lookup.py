#!/usr/bin/env python3
"""Times hjgpu_lookup on its LDS road (values + bits, bits only, aggregate-only; hjgpu_get_stats ms_join / ms_total) against
hjgpu_npj_lookup, values + bits, on the same columns in the same process - the road the same call took before.  The relations come from
hjgpu_generate_select at selectivity 0.5 (unique build keys); everything is resident, the first round of calls is a warm-up that is not
timed (it also grows the workspace); the variants alternate in one process.  A build size "L" is the context's hjgpu_get_counter "lookup_lds_rows".

usage: python tools/time_lds_lookup.py [--procs 5] [--reps 3] [--inners 1000,4096,L] [--outer N] [--timeout SECONDS]
Without --child the script runs, per build size, --procs fresh child processes one after the other, each under its own time limit, and
stops at the first one that fails; it prints each child's medians, the median over the children and the NPJ road's spread (highest minus
lowest ms_total of the children), then whether the LDS road's median ms_total (values + bits) is at most the NPJ road's median minus that
spread.  Every call is checked against the generator's expected aggregates, and by hjgpu_get_stats for the road it took."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ["lds_both", "lds_bits", "lds_agg", "npj_both"]


def child(a):
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    import hash_join_codes_knl_amd as H
    fi, fo = 0x2545F491, 0x9E3779B1
    with H.HjGpu(0) as hj:
        inner = hj.counter("lookup_lds_rows") if a.inner == "L" else int(a.inner)
        assert inner <= hj.counter("lookup_lds_rows"), "the build side is beyond the LDS road"
        ik, iv, ok, ov = hj.column(inner), hj.column(inner), hj.column(a.outer), hj.column(a.outer)
        exp = tuple(hj.generate_select(1, inner, a.outer, 0, inner, 0, a.outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov))
        ov.free()                                                       # a look-up reads no probe payloads
        vals, bits = hj.column(a.outer, placed=True), hj.column((a.outer + 31) // 32)
        want = (exp[0], exp[1], 0, exp[3])
        times = {k: [] for k in VARIANTS}
        for rep in range(a.reps + 1):                                   # rep 0: warm-up
            for name, fn, v, b in (("lds_both", hj.lookup, vals, bits), ("lds_bits", hj.lookup, None, bits), ("lds_agg", hj.lookup, None, None),
                                   ("npj_both", hj.npj_lookup, vals, bits)):
                got = tuple(fn(ik, iv, inner, ok, a.outer, vals_out=v, match_bits=b))
                assert got == want, (name, got, want)
                st = hj.stats()
                assert st["ms_close_gaps"] == 0
                assert (st["buckets"] == 0 and st["fanout1"] == 1) == name.startswith("lds"), (name, st)
                if rep:
                    times[name].append((st["ms_build"], st["ms_join"], st["ms_total"]))
    res = {"inner": inner}
    for k, v in times.items():
        for i, part in enumerate(("build", "join", "total")):
            res["%s_%s" % (k, part)] = statistics.median(x[i] for x in v)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inners", default="1000,4096,L")
    ap.add_argument("--inner", default="0", help="(--child) build rows, or L")
    ap.add_argument("--outer", type=int, default=1_000_000_000)
    ap.add_argument("--timeout", type=int, default=100, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    all_hold = True
    for inner in a.inners.split(","):
        runs = []
        for p in range(a.procs):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                   "--inner", inner, "--outer", str(a.outer)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                 # nothing more is started behind a process that failed
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            if p == 0:
                print("%d x %d M, selectivity 0.5; ms, medians of %d calls per process; lds_* = hjgpu_lookup, npj_both = hjgpu_npj_lookup, values + bits"
                      % (runs[0]["inner"], a.outer // 10**6, a.reps))
            print("process %d: %s" % (p, " ".join("%s %.3f" % kv for kv in runs[-1].items() if kv[0] != "inner")), flush=True)
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        print("%-12s %9s %9s %9s" % ("median of %d" % a.procs, "ms_build", "ms_join", "ms_total"))
        for k in VARIANTS:
            print("%-12s %9.3f %9.3f %9.3f" % (k, med[k + "_build"], med[k + "_join"], med[k + "_total"]))
        nn = [r["npj_both_total"] for r in runs]
        spread = max(nn) - min(nn)
        holds = med["lds_both_total"] <= med["npj_both_total"] - spread
        all_hold = all_hold and holds
        print("hjgpu_npj_lookup ms_total: median %.3f, lowest %.3f, highest %.3f, spread %.3f; hjgpu_lookup (values + bits) ms_total %.3f: %s"
              % (med["npj_both_total"], min(nn), max(nn), spread, med["lds_both_total"],
                 "at most the median minus the spread" if holds else "ABOVE the median minus the spread"), flush=True)
    print("condition (LDS road's median ms_total, values + bits <= NPJ road's median ms_total - its spread, every shape): %s"
          % ("holds" if all_hold else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
