"""CPU test of hjgpu_group_by's argument checks (hash_join_codes_knl_amd/csrc/colop_checks.hpp check_group_by): plain host C++;
tests/cpp_group_by_checks.cpp is a stand-alone program built with the address and undefined-behaviour sanitizers.  From one valid call with
four keys and four aggregates over fabricated pointers, in the blocking and in the device-count form, every single deviation gives the
stated status: nkeys 0 to 4 accepted and 5 refused with "nkeys" (also at n == 0), a NULL entry among the first nkeys of either key array,
the aggregates' refusals with their index, every alignment, every overlap of a written operand - each of the four key outputs among them -
with the mask, an input and another output, the n == 0 accept with NULL everywhere, the device count word's alignment and overlap; and
hjgpu_group_agg's own limit of two keys stays where it was."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_deviation_from_a_valid_call(tmp_path):
    exe = tmp_path / "group_by_checks"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_group_by_checks.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 3_000, out.stdout
