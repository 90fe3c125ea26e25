"""CPU test of hjgpu_filter_selected's predicate arithmetic (hash_join_codes_knl_amd/csrc/filter_layout.hpp: the host normalises a
predicate {lo, hi, flags} to {bias, lo', span, invert}, the kernel tests a value with one subtract and one compare).  The header is plain
host / device arithmetic shared with the entry points and the kernel of csrc/gen_kernels.hip; tests/cpp_filter_layout.cpp compares
normalise() + passes() with the definition - lo <= x <= hi in uint32 or int32 order, inverted under NOT - for every flag combination and
all triples of the boundary set {0, 1, 2, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF}: 4 x 9^3 cases."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normalised_predicates_agree_with_the_definition(tmp_path):
    exe = tmp_path / "filter_layout"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_filter_layout.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: 2916 cases"), out.stdout
