"""CPU test of hjgpu_compact_selected's geometry (hash_join_codes_knl_amd/csrc/compact_layout.hpp: how the rows [0, n) are cut into one
contiguous range of whole chunks per workgroup, and which mask words a range's count pass reads).  The header is plain host arithmetic
shared with the launchers and kernels of csrc/gen_kernels.hip; tests/cpp_compact_layout.cpp walks the ranges on the host for n from 0
through every tail of the GPU tests, around multiples of a chunk and of a grid of chunks, and up to 2^40, with 1, 2, 512 and 2048 ranges."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranges_cover_the_rows_and_stay_inside_the_mask(tmp_path):
    exe = tmp_path / "compact_layout"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_compact_layout.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
