"""CPU test of the column operators' argument checks (hash_join_codes_knl_amd/csrc/colop_checks.hpp: one operand table and one rule - every
pointer aligned, no written range shares a byte with another range unless it is the very pointer of the input it names - behind the heads
of hjgpu_compact_selected, hjgpu_group_sum, hjgpu_filter_selected, hjgpu_gather_selected and the selected look-ups' mask).  The header is
plain host C++; tests/cpp_colop_checks.cpp compares it with the hand-written checkers it replaced (tests/cpp_colop_checks_parent.hpp) over
fabricated pointers: every single deviation from a valid call gives the same status and the same "overlaps", every pair of deviations on
two operands the same decision, the legal in-place calls are accepted and refused once moved by a vector."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checks_agree_with_the_checkers_they_replaced(tmp_path):
    exe = tmp_path / "colop_checks"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_colop_checks.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 100_000, out.stdout
