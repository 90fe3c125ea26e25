"""CPU test of hjgpu_order_by's argument checks (hash_join_codes_knl_amd/csrc/colop_checks.hpp check_order_by): plain host C++;
tests/cpp_order_by_checks.cpp is a stand-alone program built with the address and undefined-behaviour sanitizers.  From one valid call with
four keys of mixed width, direction and signedness, eight carried columns, a mask and the row numbers over fabricated pointers, in the
blocking and in the device-count form, every single deviation gives the stated status and text: nkeys 0 (which names
hjgpu_compact_selected) and 5, ncols 9, each NULL - the arrays, the count, and every pointer among the first nkeys / ncols entries, by its
index -, each flag bit outside those defined and each reserved word, by index, n beyond 0xFFFFFFFF, every misalignment, every overlap of
every output and of the device count word with the mask, every key column, every carried input and every other output - over the first
min(limit, n) elements of an output, no further -, and n == 0 accepted with NULL everywhere."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_deviation_from_a_valid_call(tmp_path):
    exe = tmp_path / "order_by_checks"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_order_by_checks.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 2000, out.stdout
