#!/usr/bin/env python3
"""Join-phase time (hjgpu_get_stats ms_join: the bitmap's clear, the probe launches and the tail kernel that reports the unmatched build
tuples are all inside it) of INNER, LEFT_OUTER, RIGHT_OUTER and FULL_OUTER joins at 64 M x 1 G, aggregate-only and materialised, the
variants alternating in one process on the same relations.  The relations come from hjgpu_generate_select at selectivity 0.5: half of
the probe tuples have a match, and exactly half of the (unique) build keys occur in the probe side.

usage: python tools/time_right_full_outer.py [--procs 5] [--reps 3] [--inner N --outer N]
Without --child the script runs --procs fresh child processes one after the other and prints each child's medians and the median over
the children.  Every join is checked: INNER against the generator's expected aggregates, LEFT_OUTER against |S| and the probe columns'
sums; RIGHT_OUTER and FULL_OUTER are those plus the unmatched build tuples - inner - inner / 2 of them by the generator's construction,
their sums from the build columns' sums minus a semi-join with the roles swapped (once, untimed)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = [("inner", 0), ("left_outer", 8), ("right_outer", 16), ("full_outer", 24)]
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
        s_out, s_in = hj.column_sums(ok, a.outer, fo, fi), hj.column_sums(ik, a.inner, fi, fo)
        prm = PhjParams(); prm.flags = H.FLAG_SEMI
        semi = hj.phj(ok, ov, a.outer, ik, iv, a.inner, params=prm)       # the build tuples with a match, R as the probe side
        un = (a.inner - semi[0], (s_in[0] - semi[1]) & M64, (s_in[1] - semi[2]) & M64)
        assert un[0] == a.inner - a.inner // 2, un
        left = (a.outer, s_out[0], s_out[1], exp[3])
        want = {"inner": exp, "left_outer": left,
                "right_outer": (exp[0] + un[0], (exp[1] + un[1]) & M64, exp[2], (exp[3] + un[2]) & M64),
                "full_outer": (left[0] + un[0], (left[1] + un[1]) & M64, left[2], (left[3] + un[2]) & M64)}
        cap = hj.output_capacity(1, a.outer, want["full_outer"][0])
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
                        times["%s_%s" % (name, "rows" if rows else "agg")].append(hj.stats()["ms_join"])
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
    print("median over %d processes (ms_join, tail kernel included): %s" % (a.procs, " ".join("%s %.3f" % kv for kv in med.items())))
    for m in ("agg", "rows"):
        print("%s: right_outer / inner %.3f, full_outer / left_outer %.3f, left_outer / inner %.3f"
              % (m, med["right_outer_" + m] / med["inner_" + m], med["full_outer_" + m] / med["left_outer_" + m],
                 med["left_outer_" + m] / med["inner_" + m]))


if __name__ == "__main__":
    main()
