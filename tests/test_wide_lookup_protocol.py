"""CPU test of the table of hjgpu_lookup_wide (hash_join_codes_knl_amd/csrc/wide_lookup_layout.hpp): the claim-then-store insert that
wide_lookup_build_kernel runs in device memory, instantiated over atomic claim words in host memory and raced by 16 threads, and the find
of wide_lookup_kernel once they have joined (tests/cpp_wide_lookup_protocol.cpp, a stand-alone program).  The tuples are {0, 1, 0x80000000,
0xFFFFFFFF}^nkeys for nkeys 2, 3 and 4 - every prefix is shared -, every other one is inserted, some three times, at the default load and
into a table of inserts + 1 slots, where the walks wrap round.  Every inserted tuple is found with the payload of one of its copies, every
other tuple is a miss, occupied slots == inserts, unused key words are 0.  The program also checks the slot sizes and the slots formula.  It
is built once plain and once with the thread sanitizer: the claim words are atomics, and a slot's key words are its winner's alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", [[], ["-fsanitize=thread"]], ids=["plain", "tsan"])
def test_the_insert_raced_by_16_threads_the_find_and_the_sizes(tmp_path, sanitizer):
    exe = tmp_path / "wide_lookup_protocol"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread"] + sanitizer +
                          ["-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_wide_lookup_protocol.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 10_000, out.stdout
