"""CPU test of hjgpu_gather_selected's row classification and geometry (hash_join_codes_knl_amd/csrc/gather_layout.hpp: the kernel
classifies every row - gathered, NULL, out of range - before it forms a source address).  The header is plain host / device arithmetic
shared with the entry points and the kernel of csrc/gen_kernels.hip; tests/cpp_gather_layout.cpp compares classify() with the definition
for selected in {0, 1} and every pair (index, src_rows) of the boundary set {0, 1, 2, 2^30 - 1, 2^30, 2^31, 2^32 - 2, 2^32 - 1}: 2 x 8^2
cases, and checks grid_of / step_rows."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_classification_agrees_with_the_definition(tmp_path):
    exe = tmp_path / "gather_layout"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_gather_layout.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: 128 cases"), out.stdout
