#!/usr/bin/env python3
"""Join-phase and whole-join time (hjgpu_get_stats ms_join / ms_total; the bitmap's clear, the marking launches and the tail kernel are
all inside ms_join) of RIGHT_SEMI, RIGHT_ANTI, RIGHT_OUTER, SEMI and INNER joins at 64 M x 1 G, aggregate-only and materialised, the
variants alternating in one process on the same relations - and of the alternative the right semi-join replaces: HJGPU_FLAG_SEMI with
the sides swapped (1 G build side, 64 M probe side; ms_total).  The relations come from hjgpu_generate_select at selectivity 0.5: half
of the probe tuples have a match, and exactly half of the (unique) build keys occur in the probe side.

usage: python tools/time_right_semi_anti.py [--procs 5] [--reps 3] [--inner N --outer N] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the
first one that fails; it prints each child's medians, the median over the children and RIGHT_OUTER's spread (highest minus lowest
aggregate-only ms_join of the children), then whether the aggregate-only ms_join of RIGHT_SEMI and of RIGHT_ANTI stays within
RIGHT_OUTER's median plus that spread.  Every join is checked: INNER against the generator's expected aggregates, SEMI is its count
and probe-side sums, the swapped SEMI gives the matched build tuples (RIGHT_SEMI) and, subtracted from the build columns' sums, the
unmatched ones (RIGHT_ANTI; inner - inner / 2 of them by the generator's construction), RIGHT_OUTER is INNER plus those."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = [("inner", 0), ("semi", 2), ("right_outer", 16), ("right_semi", 32), ("right_anti", 64)]
M64 = (1 << 64) - 1


def child(a):
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    import hash_join_codes_knl_amd as H
    from hash_join_codes_knl_amd.api import PhjParams
    fi, fo = 0x2545F491, 0x9E3779B1
    with H.HjGpu(0) as hj:
        ik, iv, ok, ov = hj.column(a.inner), hj.column(a.inner), hj.column(a.outer), hj.column(a.outer)
        exp = tuple(hj.generate_select(1, a.inner, a.outer, 0, a.inner, 0, a.outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov))
        s_in = hj.column_sums(ik, a.inner, fi, fo)
        # the alternative: the build tuples with a match, S as the build side and R as the probe side
        prm = PhjParams(); prm.flags = H.FLAG_SEMI
        swapped = []
        for rep in range(a.reps + 1):
            semi = hj.phj(ok, ov, a.outer, ik, iv, a.inner, params=prm)
            st = hj.stats()
            if rep:
                swapped.append((st["ms_join"], st["ms_total"]))
        un = (a.inner - semi[0], (s_in[0] - semi[1]) & M64, (s_in[1] - semi[2]) & M64)
        assert un[0] == a.inner - a.inner // 2, un
        want = {"inner": exp, "semi": (exp[0], exp[1], exp[2], 0),
                "right_outer": (exp[0] + un[0], (exp[1] + un[1]) & M64, exp[2], (exp[3] + un[2]) & M64),
                "right_semi": (semi[0], semi[1], 0, semi[2]), "right_anti": (un[0], un[1], 0, un[2])}
        cap = hj.output_capacity(1, a.outer, want["right_outer"][0])
        cols = [hj.column(cap, placed=True) for _ in range(3)]
        out = (cols[0], cols[1], cols[2], cap, 0)
        times = {"%s_%s" % (n, m): [] for n, _ in VARIANTS for m in ("agg", "rows")}
        for rep in range(a.reps + 1):                         # rep 0: warm-up
            for rows in (False, True):
                for name, flag in VARIANTS:
                    prm = PhjParams(); prm.flags = flag
                    got = tuple(hj.phj(ik, iv, a.inner, ok, ov, a.outer, params=prm, out=out if rows else None))
                    assert got == want[name], (name, got, want[name])
                    if rep:
                        st = hj.stats()
                        times["%s_%s" % (name, "rows" if rows else "agg")].append((st["ms_join"], st["ms_total"]))
    res = {}
    times["swapped_semi_agg"] = swapped
    for k, v in times.items():
        res[k + "_join"] = statistics.median(x[0] for x in v)
        res[k + "_total"] = statistics.median(x[1] for x in v)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=64_000_000)
    ap.add_argument("--outer", type=int, default=1_000_000_000)
    ap.add_argument("--timeout", type=int, default=150, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    print("%d M x %d M, selectivity 0.5, half of the build keys present; ms, medians of %d joins per process" % (a.inner // 10**6, a.outer // 10**6, a.reps))
    runs = []
    for p in range(a.procs):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
               "--inner", str(a.inner), "--outer", str(a.outer)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                 # nothing more is started behind a process that failed
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("process %d: %s" % (p, " ".join("%s %.3f" % kv for kv in runs[-1].items())), flush=True)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    print("median over %d processes: %s" % (a.procs, " ".join("%s %.3f" % kv for kv in med.items())))
    ro = [r["right_outer_agg_join"] for r in runs]
    spread = max(ro) - min(ro)
    print("right_outer aggregate-only ms_join: median %.3f, lowest %.3f, highest %.3f, spread %.3f" % (med["right_outer_agg_join"], min(ro), max(ro), spread))
    holds = True
    for n in ("right_semi", "right_anti"):
        over = med[n + "_agg_join"] - med["right_outer_agg_join"]
        ok = over <= spread
        holds = holds and ok
        print("%s aggregate-only ms_join %.3f: %+.3f against right_outer, %s its spread" % (n, med[n + "_agg_join"], over, "within" if ok else "BEYOND"))
    print("ms_total, aggregate-only: right_semi %.3f, semi with the sides swapped (%d M build, %d M probe) %.3f = %.2f x"
          % (med["right_semi_agg_total"], a.outer // 10**6, a.inner // 10**6, med["swapped_semi_agg_total"],
             med["swapped_semi_agg_total"] / med["right_semi_agg_total"]))
    print("condition (right_semi, right_anti <= right_outer + its spread): %s" % ("holds" if holds else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
