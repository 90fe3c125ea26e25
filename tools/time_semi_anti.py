#!/usr/bin/env python3
"""Join-phase time (hjgpu_get_stats ms_join) of inner, _UNIQUE, SEMI and ANTI joins at 64 M x 1 G, selectivity 0.5 (hjgpu_generate_select),
aggregate-only and materialised, the variants alternating in one process on the same relations.

usage: python tools/time_semi_anti.py [--procs 5] [--reps 3] [--inner N --outer N]
Without --child the script runs --procs fresh child processes one after the other and prints each child's medians and the median over
the children.  Every join is checked: SEMI's aggregates against the generator's expected ones, SEMI + ANTI against all of S."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = [("inner", 0), ("unique", 1), ("semi", 2), ("anti", 4)]


def child(a):
    import numpy as np
    try:
        import torch
        torch.cuda.init()
    except ImportError:
        pass
    import hash_join_codes_knl_amd as H
    from hash_join_codes_knl_amd.api import PhjParams
    m64 = (1 << 64) - 1
    with H.HjGpu(0) as hj:
        ik, iv, ok, ov = hj.column(a.inner), hj.column(a.inner), hj.column(a.outer), hj.column(a.outer)
        exp = hj.generate_select(1, a.inner, a.outer, 0, a.inner, 0, a.outer, 0x2545F491, 0x9E3779B1, 0.0, 0.5, ik, iv, ok, ov)
        cap = hj.output_capacity(1, a.outer, a.outer)
        cols = [hj.column(cap, placed=True) for _ in range(3)]
        out = (cols[0], cols[1], cols[2], cap, 0)
        times = {"%s_%s" % (n, m): [] for n, _ in VARIANTS for m in ("agg", "rows")}
        for rep in range(a.reps + 1):                         # rep 0: warm-up
            for rows in (False, True):
                got = {}
                for name, flag in VARIANTS:
                    prm = PhjParams(); prm.flags = flag
                    got[name] = hj.phj(ik, iv, a.inner, ok, ov, a.outer, params=prm, out=out if rows else None)
                    if rep:
                        times["%s_%s" % (name, "rows" if rows else "agg")].append(hj.stats()["ms_join"])
                assert got["inner"] == exp and got["unique"] == exp and got["semi"][:3] == exp[:3], (got, exp)
                assert got["semi"][0] + got["anti"][0] == a.outer
                assert (got["semi"][1] + got["anti"][1]) & m64 == int(ok.download().astype(np.uint64).sum(dtype=np.uint64)) & m64
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
        u = med["unique_" + m]
        print("%s: semi / unique %.3f, anti / unique %.3f, unique / inner %.3f" % (m, med["semi_" + m] / u, med["anti_" + m] / u,
                                                                                u / med["inner_" + m]))


if __name__ == "__main__":
    main()
