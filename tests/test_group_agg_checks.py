"""CPU test of hjgpu_group_agg's argument checks (hash_join_codes_knl_amd/csrc/colop_checks.hpp check_group_agg) and of the aggregate
functions' transform (csrc/agg_layout.hpp).  Both are plain host C++; tests/cpp_group_agg_checks.cpp is a stand-alone program built with the
address and undefined-behaviour sanitizers.  From one valid call over fabricated pointers, in the blocking and in the device-count form,
every single deviation gives the stated status: each function and flag refusal and each d_a / d_b rule with the aggregate's index in the
text, the limits on naggs, nkeys and capacity, every alignment, every overlap of a written operand, the n == 0 accept, the nkeys == 0 accept
with NULL key arrays, the device count word's alignment and overlap.  The transform: SUM, SUM(a * b), MIN and MAX, unsigned and signed, over
edge values, folded from the tables' initial word 0 and turned back, against the definition."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_deviation_from_a_valid_call_and_the_transform(tmp_path):
    exe = tmp_path / "group_agg_checks"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_group_agg_checks.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 10_000, out.stdout
