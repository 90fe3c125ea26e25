"""CPU test of the LDS layout of a K6 workgroup (hash_join_codes_knl_amd/csrc/scatter_layout.hpp: the arrays scatter_kernel carves out of
its dynamic LDS, and the byte count from which the launcher chooses a geometry, refuses a launch and sizes the grid).  The header is
plain arithmetic shared by the kernel and the host code of csrc/partition_kernels.hip; tests/cpp_scatter_layout.cpp walks every
(block, vpt) pair the dispatcher lists, F from 1 to 1024, carry on and off, pass 2 on and off."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arrays_are_disjoint_aligned_and_sum_to_the_launchers_bytes(tmp_path):
    exe = tmp_path / "scatter_layout"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_scatter_layout.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
