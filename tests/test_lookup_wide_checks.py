"""CPU test of hjgpu_lookup_wide's argument checks (hash_join_codes_knl_amd/csrc/colop_checks.hpp check_lookup_wide): plain host C++;
tests/cpp_lookup_wide_checks.cpp is a stand-alone program built with the address and undefined-behaviour sanitizers.  From one valid call
with four keys, a mask and both outputs over fabricated pointers, in the blocking and in the device-result form, every single deviation
gives the stated status and text: nkeys 0, 1 and 5 refused with "nkeys" (1 names hjgpu_lookup_selected), a NULL entry among the first nkeys
of either key array, a NULL payload column, the load's range, every alignment, every overlap of every written operand with the mask, a key
column, the payload column and the other written operands, the in-place pair accepted and any other overlap of the two bitmaps refused,
and the empty sides accepted with NULL where nothing is read."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_deviation_from_a_valid_call(tmp_path):
    exe = tmp_path / "lookup_wide_checks"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_lookup_wide_checks.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 300, out.stdout
