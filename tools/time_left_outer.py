#!/usr/bin/env python3
"""Join-phase time (hjgpu_get_stats ms_join) of inner, _UNIQUE, LEFT_OUTER and LEFT_OUTER | UNIQUE joins at 64 M x 1 G, selectivity 0.5
(hjgpu_generate_select), aggregate-only and materialised, the variants alternating in one process on the same relations.

usage: python tools/time_left_outer.py [--procs 5] [--reps 3] [--inner N --outer N]
Without --child the script runs --procs fresh child processes one after the other and prints each child's medians and the median over
the children.  Every join is checked: inner and _UNIQUE against the generator's expected aggregates; both left outer joins against the
same count (|S|), the probe columns' sums (hjgpu_column_sums) and the inner join's sum_inner_vals (unique build keys)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = [("inner", 0), ("unique", 1), ("left_outer", 8), ("left_outer_unique", 9)]


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
        exp = hj.generate_select(1, a.inner, a.outer, 0, a.inner, 0, a.outer, fi, fo, 0.0, 0.5, ik, iv, ok, ov)
        sums = hj.column_sums(ok, a.outer, fo, fi)
        outer_exp = (a.outer, sums[0], sums[1], exp[3])
        # rows: the left outer join's are |S| (matched + NULL rows)
        cap = hj.output_capacity(1, a.outer, a.outer)
        cols = [hj.column(cap, placed=True) for _ in range(3)]
        out = (cols[0], cols[1], cols[2], cap, 0)
        times = {"%s_%s" % (n, m): [] for n, _ in VARIANTS for m in ("agg", "rows")}
        for rep in range(a.reps + 1):                         # rep 0: warm-up
            for rows in (False, True):
                got = {}
                for name, flag in VARIANTS:
                    prm = PhjParams(); prm.flags = flag
                    got[name] = tuple(hj.phj(ik, iv, a.inner, ok, ov, a.outer, params=prm, out=out if rows else None))
                    if rep:
                        times["%s_%s" % (name, "rows" if rows else "agg")].append(hj.stats()["ms_join"])
                assert got["inner"] == tuple(exp) and got["unique"] == tuple(exp), (got, exp)
                assert got["left_outer"] == outer_exp and got["left_outer_unique"] == outer_exp, (got, outer_exp)
    print(json.dumps({k: statistics.median(v) for k, v in times.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=64_000_000)
    ap.add_argument("--outer", type=int, default=1_000_000_000)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for p in range(a.procs):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--inner", str(a.inner), "--outer", str(a.outer)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("process %d: %s" % (p, " ".join("%s %.3f" % kv for kv in runs[-1].items())), flush=True)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    print("median over %d processes (ms_join): %s" % (a.procs, " ".join("%s %.3f" % kv for kv in med.items())))
    for m in ("agg", "rows"):
        print("%s: left_outer / inner %.3f, left_outer_unique / unique %.3f, unique / inner %.3f"
              % (m, med["left_outer_" + m] / med["inner_" + m], med["left_outer_unique_" + m] / med["unique_" + m],
                 med["unique_" + m] / med["inner_" + m]))


if __name__ == "__main__":
    main()
