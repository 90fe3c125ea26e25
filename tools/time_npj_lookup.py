#!/usr/bin/env python3
"""Times the positional NPJ look-up (hjgpu_npj_lookup: values + bits, bits only, aggregate-only; hjgpu_get_stats ms_build / ms_join /
ms_total) against the way to get the same information from the joins: hjgpu_npj with HJGPU_FLAG_LEFT_OUTER | HJGPU_FLAG_UNIQUE, materialised
into columns of hjgpu_output_capacity rows, the probe payload column holding row numbers (ms_join + ms_close_gaps, ms_total; the scatter
by row number that a caller still has to do afterwards is NOT in it).  The relations come from hjgpu_generate_select at selectivity 0.5
(unique build keys); everything is resident and the workspace is reserved before anything is timed; the variants alternate in one process.

usage: python tools/time_npj_lookup.py [--procs 5] [--reps 3] [--inners 1000000,8000000,64000000] [--outer N] [--timeout SECONDS]
Without --child the script runs, per build size, --procs fresh child processes one after the other, each under its own time limit, and
stops at the first one that fails; it prints each child's medians, the median over the children and the join's spread (highest minus
lowest ms_join + ms_close_gaps of the children), then whether the look-up's ms_join (values + bits) stays within the join's median plus
that spread.  Every call is checked against the generator's expected aggregates."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOOKUPS = ["lookup_both", "lookup_bits", "lookup_agg"]


def child(a):
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    import numpy as np
    import hash_join_codes_knl_amd as H
    from hash_join_codes_knl_amd.api import NpjParams
    fi, fo = 0x2545F491, 0x9E3779B1
    with H.HjGpu(0) as hj:
        ik, iv, ok, ov = hj.column(a.inner), hj.column(a.inner), hj.column(a.outer), hj.column(a.outer)
        exp = tuple(hj.generate_select(1, a.inner, a.outer, 0, a.inner, 0, a.outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov))
        ov.upload(np.arange(a.outer, dtype=np.uint32))                  # the join's probe payloads: row numbers
        hj.reserve(a.inner, a.outer)
        cap = hj.output_capacity(0, a.outer, a.outer)
        cols = [hj.column(cap, placed=True) for _ in range(3)]
        out = (cols[0], cols[1], cols[2], cap, 0)
        vals, bits = hj.column(a.outer, placed=True), hj.column((a.outer + 31) // 32)
        want = (exp[0], exp[1], 0, exp[3])
        times = {k: [] for k in LOOKUPS + ["join"]}
        for rep in range(a.reps + 1):                                   # rep 0: warm-up
            for name, v, b in (("lookup_both", vals, bits), ("lookup_bits", None, bits), ("lookup_agg", None, None)):
                got = tuple(hj.npj_lookup(ik, iv, a.inner, ok, a.outer, vals_out=v, match_bits=b))
                assert got == want, (name, got, want)
                st = hj.stats()
                assert st["ms_close_gaps"] == 0
                if rep:
                    times[name].append((st["ms_build"], st["ms_join"], st["ms_total"]))
            prm = NpjParams(); prm.flags = H.FLAG_LEFT_OUTER | H.FLAG_UNIQUE
            got = tuple(hj.npj(ik, iv, a.inner, ok, ov, a.outer, params=prm, out=out))
            assert got[0] == a.outer and got[3] == exp[3], (got, exp)
            st = hj.stats()
            if rep:
                times["join"].append((st["ms_build"], st["ms_join"] + st["ms_close_gaps"], st["ms_total"]))
    res = {}
    for k, v in times.items():
        for i, part in enumerate(("build", "join", "total")):
            res["%s_%s" % (k, part)] = statistics.median(x[i] for x in v)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inners", default="1000000,8000000,64000000")
    ap.add_argument("--inner", type=int, default=0, help="(--child) build rows")
    ap.add_argument("--outer", type=int, default=1_000_000_000)
    ap.add_argument("--timeout", type=int, default=150, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    all_hold = True
    for inner in (int(x) for x in a.inners.split(",")):
        print("%d M x %d M, selectivity 0.5; ms, medians of %d calls per process; join = hjgpu_npj LEFT_OUTER | UNIQUE, materialised, its "
              "`join` column is ms_join + ms_close_gaps" % (inner // 10**6, a.outer // 10**6, a.reps))
        runs = []
        for p in range(a.procs):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                   "--inner", str(inner), "--outer", str(a.outer)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                 # nothing more is started behind a process that failed
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("process %d: %s" % (p, " ".join("%s %.3f" % kv for kv in runs[-1].items())), flush=True)
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        print("%-12s %9s %9s %9s" % ("median of %d" % a.procs, "ms_build", "join", "ms_total"))
        for k in LOOKUPS + ["join"]:
            print("%-12s %9.3f %9.3f %9.3f" % (k, med[k + "_build"], med[k + "_join"], med[k + "_total"]))
        jj = [r["join_join"] for r in runs]
        spread = max(jj) - min(jj)
        over = med["lookup_both_join"] - med["join_join"]
        holds = over <= spread
        all_hold = all_hold and holds
        print("join ms_join + ms_close_gaps: median %.3f, lowest %.3f, highest %.3f, spread %.3f; look-up (values + bits) ms_join %.3f: %+.3f, %s"
              % (med["join_join"], min(jj), max(jj), spread, med["lookup_both_join"], over, "within" if holds else "BEYOND the spread"), flush=True)
    print("condition (look-up ms_join, values + bits <= join's ms_join + ms_close_gaps + its spread, every shape): %s" % ("holds" if all_hold else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
