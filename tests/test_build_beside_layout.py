"""CPU test of the CU split of a join whose build side is partitioned beside its probe side
(hash_join_codes_knl_amd/csrc/build_beside_layout.hpp: how many CUs the build side's chain on the side stream gets and how many the probe
side's passes keep).  The header is plain arithmetic; tests/cpp_build_beside.cpp walks 1 ... 304 CUs, option "build_cus" 0 ... 400 and
relations from empty to 2^33 rows."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_sides_get_a_cu_or_there_is_no_overlap(tmp_path):
    exe = tmp_path / "build_beside"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_build_beside.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
