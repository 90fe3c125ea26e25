"""CPU test of the wide table of hjgpu_group_by (hash_join_codes_knl_amd/csrc/wide_group_layout.hpp): the insert-or-find walk that
wide_group_kernel runs over LDS and device memory, instantiated over atomic 64-bit words in host memory and raced by 16 threads
(tests/cpp_wide_group_protocol.cpp, a stand-alone program).  The tuples are {0, 1, 0x80000000, 0xFFFFFFFF}^nkeys for nkeys 3 and 4 - every
prefix is shared -, the table has twice as many slots, the home slot is cut to 4 bits.  Every tuple ends in exactly one slot, every
occupied slot holds nkeys non-zero words and zero words behind them, the counts add up to the inserts; under a claim limit the table holds
no more slots than the limit; a full table reports "no slot" and does not spin.  The program also checks the header's sizes.  It is built
once plain and once with the thread sanitizer: the protocol's words are atomics and nothing else is shared."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", [[], ["-fsanitize=thread"]], ids=["plain", "tsan"])
def test_the_walk_raced_by_16_threads_and_the_sizes(tmp_path, sanitizer):
    exe = tmp_path / "wide_group_protocol"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread"] + sanitizer +
                          ["-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_wide_group_protocol.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 700, out.stdout
