#!/usr/bin/env python3
"""Times hjgpu_lookup_wide with two and four key columns (hjgpu_get_stats: ms_histogram = the clear of the table and the build, ms_join = the
look-up kernel, ms_total = all of it) against four yardsticks on the same row counts, masks and hit rate, all taken in the same process:

  (a) one key         hjgpu_lookup_selected under option no_broadcast (the NPJ road) on ONE key column - the tuple's number -, both outputs;
  (b) (a) + the read  (a) plus hjgpu_stream_read_ms over the further nkeys - 1 probe columns: what further key columns ought to cost;
  (c) today           what a caller does without the wide look-up while the tuple packs into 32 bits: torch packs the probe columns into
                      one uint32 column - timed by torch events - and then calls (a); the pack is part of the time;
  (d) the ceiling     hjgpu_random_line_read_ms with the wide table's bytes and the number of selected rows: the memory system's rate for
                      one independent request per row.

Columns: tuple number u in [1, 2 * inner] has the key columns (u & 0x3FFF, u >> 14) with two keys and (u & 0xFF, u >> 8 & 0xFF, u >> 16 &
0xFF, u >> 24) with four, so that the pack is u itself; the build side holds u = 1 ... inner in a scattered order with the payload (u *
0x85EBCA6B) mod 2^32; probe row i carries u(i) = ((i * 0x9E3779B1) mod 2^32) mod (2 * inner) + 1: half the probe tuples are present.  Masks
(seeded: the same in every process): eighth - every row selected with probability 1/8; ones - every row, through a mask of all-ones words.
Every call is checked against torch before it is timed: the aggregates, every value and every word of the bitmap.

usage: python tools/time_lookup_wide.py [--procs 3] [--reps 3] [--rows N] [--inner 1048576 8388608 67108864] [--timeout SECONDS]
Without --child the script runs --procs fresh child processes one after the other, each under its own time limit, and stops at the first one
that fails.  The first round of calls of a process is a warm-up that is not timed.  It prints each child's medians and, per row, the median
over the children; it only prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASKS = ["ones", "eighth"]
M_ID, M_PAY, M_ORDER = 0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35
SHIFTS = {2: (0, 14), 4: (0, 8, 16, 24)}
WIDTH = {2: (0x3FFF, 0xFFFFFFFF), 4: (0xFF, 0xFF, 0xFF, 0xFF)}
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


def mask_words(kind, n):
    words = (n + 31) // 32
    w = np.full(words, 0xFFFFFFFF, np.uint32)
    if kind == "eighth":
        rng = np.random.default_rng(1)
        for _ in range(3):
            w &= rng.integers(0, 2**32, size=words, dtype=np.uint64).astype(np.uint32)
    return w


def slots_of(inner, load=0.5):
    return (max(16, inner + 1, int(inner / load)) + 7) // 8 * 8


def child(a):
    import torch
    torch.cuda.init()
    import hash_join_codes_knl_amd as H
    n = a.rows
    assert n % 32 == 0, "--rows must be a multiple of 32 (whole mask words, 16-byte aligned columns in one allocation)"
    dev = torch.device("cuda")
    cols = torch.empty(7 * n, dtype=torch.int32, device=dev)         # u, key 0 ... key 3, the packed column, the values: one allocation
    num, key, packed, vals = cols[:n], [cols[(1 + c) * n:(2 + c) * n] for c in range(4)], cols[5 * n:6 * n], cols[6 * n:]
    bits = torch.empty(n // 32, dtype=torch.int32, device=dev)
    step = 1 << 26
    u32 = lambda t: t.to(torch.int64) & M32                           # noqa: E731
    shifts = torch.arange(32, dtype=torch.int64, device=dev)
    res = {}

    with H.HjGpu(0) as hj, H.HjGpu(0) as one:
        one.set_option("no_broadcast", 1)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        masks = {kind: torch.from_numpy(mask_words(kind, n).view(np.int32)).to(dev) for kind in MASKS}

        def checked(inner, words, got, what):
            """the call's aggregates, values and bitmap against torch's own over the same rows"""
            count = sum_k = sum_p = 0
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                u = u32(num[lo:hi])
                sel = ((u32(words[lo // 32:hi // 32]).view(-1, 1) >> shifts) & 1).view(-1).bool()
                hit = sel & (u <= inner)
                pay = (u * M_PAY) & M32
                assert bool((u32(vals[lo:hi]) == torch.where(hit, pay, torch.full_like(pay, M32))).all().item()), (what, "values")
                assert bool((u32(bits[lo // 32:hi // 32]) == (hit.view(-1, 32).to(torch.int64) << shifts).sum(dim=1)).all().item()), (what, "bits")
                count += int(hit.sum().item())
                sum_k += int((u32(key[0][lo:hi]) if what[0] == "wide" else u)[hit].sum().item())
                sum_p += int(pay[hit].sum().item())
            assert tuple(got) == (count, sum_k & M64, 0, sum_p & M64), (what, got, (count, sum_k, sum_p))
            return count

        for inner in a.inner:
            assert inner & (inner - 1) == 0 and 2 * inner <= 1 << 28, "--inner: powers of two up to 2^27"
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                i = torch.arange(lo, hi, dtype=torch.int64, device=dev)
                num[lo:hi] = (((i * M_ID) & M32) % (2 * inner) + 1).to(torch.int32)
            j = torch.arange(inner, dtype=torch.int64, device=dev)
            bu = ((j * M_ORDER) & (inner - 1)) + 1                    # 1 ... inner, scattered (an odd multiplier modulo a power of two)
            bnum, bpay = bu.to(torch.int32), ((bu * M_PAY) & M32).to(torch.int32)
            del i, j
            for nkeys in (2, 4):
                bkey = [((bu >> s) & w).to(torch.int32) for s, w in zip(SHIFTS[nkeys], WIDTH[nkeys])]
                for c, (s, w) in enumerate(zip(SHIFTS[nkeys], WIDTH[nkeys])):
                    for lo in range(0, n, step):
                        hi = min(lo + step, n)
                        key[c][lo:hi] = ((u32(num[lo:hi]) >> s) & w).to(torch.int32)

                def pack():
                    """the probe columns in one uint32 column: one torch kernel per further column"""
                    torch.add(key[0], key[1], alpha=1 << SHIFTS[nkeys][1], out=packed)
                    for c in range(2, nkeys):
                        packed.add_(key[c], alpha=1 << SHIFTS[nkeys][c])

                table_bytes = slots_of(inner) * (16 if nkeys == 2 else 32)
                scratch = torch.empty(table_bytes // 4, dtype=torch.int32, device=dev)
                read_ms = statistics.median(hj.stream_read_ms(key[1].data_ptr(), 4 * n * (nkeys - 1) // 65536 * 65536) for _ in range(a.reps))
                for kind in MASKS:
                    words = masks[kind]
                    wide, single, packs, selected = [], [], [], 0
                    for rep in range(a.reps + 1):                    # rep 0: warm-up, and the check against torch
                        got = hj.lookup_wide([k.data_ptr() for k in bkey], bpay.data_ptr(), inner, [k.data_ptr() for k in key[:nkeys]], n,
                                             select_bits=words.data_ptr(), vals_out=vals.data_ptr(), match_bits=bits.data_ptr())
                        st = hj.stats()
                        if rep == 0:
                            assert st["buckets"] == slots_of(inner), st
                            checked(inner, words, got, ("wide", inner, nkeys, kind))
                        else:
                            wide.append((st["ms_histogram"], st["ms_join"], st["ms_total"]))
                        packed.zero_()
                        ev[0].record()
                        pack()
                        ev[1].record()
                        torch.cuda.synchronize()
                        got = one.lookup_selected(bnum.data_ptr(), bpay.data_ptr(), inner, packed.data_ptr(), n, select_bits=words.data_ptr(),
                                                  vals_out=vals.data_ptr(), match_bits=bits.data_ptr())
                        st1 = one.stats()
                        if rep == 0:
                            assert st1["fanout1"] == 0 and st1["buckets"] > 0, st1      # the NPJ road
                            selected = int((u32(words).view(-1, 1) >> shifts & 1).sum().item())
                            checked(inner, words, got, ("one key", inner, nkeys, kind))
                        else:
                            single.append(st1["ms_total"])
                            packs.append(ev[0].elapsed_time(ev[1]))
                    line_ms = statistics.median(hj.random_line_read_ms(scratch.data_ptr(), table_bytes // 64 * 64, selected) for _ in range(a.reps))
                    med = lambda rows, f: statistics.median(r[f] for r in rows)     # noqa: E731
                    res["2^%d build rows, %d keys, %s" % (inner.bit_length() - 1, nkeys, kind)] = {
                        "wide_build": med(wide, 0), "wide_join": med(wide, 1), "wide_total": med(wide, 2), "one_total": statistics.median(single),
                        "read_ms": read_ms, "pack_ms": statistics.median(packs), "line_ms": line_ms}
                del scratch
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--inner", type=int, nargs="+", default=[1 << 20, 1 << 23, 1 << 26])
    ap.add_argument("--timeout", type=int, default=280, help="seconds one child process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for p in range(a.procs):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rows", str(a.rows),
               "--inner"] + [str(x) for x in a.inner]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                     # nothing more is started behind a process that failed
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if p == 0:
            import hash_join_codes_knl_amd as H
            print("library %s; %d probe rows, half of the probe tuples present; ms, medians of %d calls per process after one untimed, checked round; "
                  "build / join / total = hjgpu_lookup_wide's ms_histogram / ms_join / ms_total; (a) = hjgpu_lookup_selected's ms_total under "
                  "no_broadcast on one key column, read = hjgpu_stream_read_ms of the further probe columns, pack = torch packing the probe "
                  "columns, (d) = hjgpu_random_line_read_ms of the wide table's bytes, one read per selected row" % (H.library_hash(), a.rows, a.reps))
        for k, v in runs[-1].items():
            print("process %d: %-36s %s" % (p, k, "  ".join("%s %.3f" % (f, v[f]) for f in v)), flush=True)
    print("%-36s %8s %9s %10s | %9s | %8s %9s | %8s %9s | %8s | %9s %8s" % ("median of %d processes" % a.procs, "build", "join", "total", "(a)", "read", "(b)",
                                                                        "pack", "(c)", "(d)", "total/(b)", "join/(d)"))
    for k in runs[0]:
        m = {f: statistics.median(r[k][f] for r in runs) for f in runs[0][k]}
        b, c = m["one_total"] + m["read_ms"], m["one_total"] + m["pack_ms"]
        print("%-36s %8.3f %9.3f %10.3f | %9.3f | %8.3f %9.3f | %8.3f %9.3f | %8.3f | %9.2f %8.2f" % (
            k, m["wide_build"], m["wide_join"], m["wide_total"], m["one_total"], m["read_ms"], b, m["pack_ms"], c, m["line_ms"],
            m["wide_total"] / b, m["wide_join"] / m["line_ms"]))


if __name__ == "__main__":
    main()
