#!/usr/bin/env python3
"""Compares the gfx950 machine code of two trees kernel by kernel (CPU only: needs hipcc, no GPU).
usage: python tools/isa_diff.py <tree-or-.s A> <tree-or-.s B> [source ...]   (sources: files of csrc/, default: the five kernel sources)
A tree is a checkout of this repository (a parent commit's, say: `git archive <commit> | tar -x -C <dir>`); its sources are compiled as
tests/device_compile.py compiles them.  Comments and the numbers of local labels are dropped.  Prints the symbols only one side has, per
differing symbol both sides' instruction counts and resources and the head of the diff, and the count of identical symbols; exit
status 0 only if both sides hold the same symbols and every one is identical."""
import difflib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from device_compile import compile_device, split_kernels

SOURCES = ["join_kernels.hip", "npj_kernels.hip", "partition_kernels.hip", "gen_kernels.hip", "audit_kernels.hip"]


def kernels(path, sources):
    """({symbol: instruction lines}, {demangled name: resources}) of an assembly file or of a tree's sources"""
    if os.path.isfile(path):
        texts, res = [open(path).read()], {}
    else:
        csrc = os.path.join(path, "hash_join_codes_knl_amd", "csrc")
        done = [compile_device(s, csrc) for s in sources]
        texts, res = [t for t, _ in done], {k: v for _, r in done for k, v in r.items()}
    out = {}
    for text in texts:
        for sym, body in split_kernels(text).items():
            lines = [l.split(";")[0].rstrip() for l in body.splitlines()]
            out[sym] = [re.sub(r"\.LBB\d+_\d+", "L", l) for l in lines if l.strip()]
    return out, res


def main():
    sources = sys.argv[3:] or SOURCES
    (a, ra), (b, rb) = kernels(sys.argv[1], sources), kernels(sys.argv[2], sources)
    for side, only in (("A", sorted(set(a) - set(b))), ("B", sorted(set(b) - set(a)))):
        for sym in only:
            print("only in %s: %s" % (side, sym))
    differ = [k for k in sorted(a) if k in b and a[k] != b[k]]
    plain = dict(zip(differ, subprocess.run(["c++filt"], input="\n".join(differ), capture_output=True, text=True).stdout.splitlines()))
    for k in differ:
        d = [x for x in difflib.unified_diff(a[k], b[k], lineterm="", n=0) if not x.startswith(("---", "+++", "@@"))]
        print("DIFF %s\n  instructions %d -> %d, %d diff lines" % (plain[k], len(a[k]), len(b[k]), len(d)))
        for r in (ra.get(plain[k]), rb.get(plain[k])):
            if r:
                print("  vgpr %(vgpr)d scratch %(scratch)d vspill %(vspill)d sspill %(sspill)d occupancy %(occ)d" % r)
        print("\n".join("    " + x for x in d[:8]))
    same = sum(1 for k in a if k in b and a[k] == b[k])
    print("A %d symbols, B %d symbols: %d identical, %d differ, %d only in A, %d only in B"
          % (len(a), len(b), same, len(differ), len(set(a) - set(b)), len(set(b) - set(a))))
    return 0 if set(a) == set(b) and not differ else 1


if __name__ == "__main__":
    sys.exit(main())
