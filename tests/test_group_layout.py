"""CPU test of hjgpu_group_sum's tables (hash_join_codes_knl_amd/csrc/group_layout.hpp: the slot, the size rule of the merge table, the LDS
table's geometry and hash).  The header is plain host / device arithmetic shared with the launchers and kernels of csrc/gen_kernels.hip;
tests/cpp_group_layout.cpp checks the merge-table size rule for capacities 0, 1, 511, 512, 513, 2^20, 2^32 and around every power of two,
and the slot-layout sizes against the LDS budget of a compute unit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_sizes_and_slot_layout(tmp_path):
    exe = tmp_path / "group_layout"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_group_layout.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
