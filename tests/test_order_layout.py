"""CPU test of hash_join_codes_knl_amd/csrc/order_layout.hpp, the plain-arithmetic header that hjgpu_order_by's launchers and kernels
share: tests/cpp_order_layout.cpp is a stand-alone program built with the address and undefined-behaviour sanitizers.  The ranges of the
device road tile [0, n), start on chunk boundaries and keep the tail in the last non-empty range, for n from 0 through a few chunks, at
the road switch and at the largest n; the normalisation orders all pairs of the edge values, 32- and 64-bit, under all four combinations
of direction and signedness as the plain C++ comparison does, and a pass's digit of a column's word is the digit of the normalised key;
and a host emulation of the whole pass sequence - the device road's histogram per range, scan over (digit, range) and chunk-by-chunk
scatter, and the LDS road's travelling key with its skipped passes - equals std::stable_sort with the composite comparator for 1 to 4
keys of mixed width, direction and signedness."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranges_normalisation_and_the_pass_sequence(tmp_path):
    exe = tmp_path / "order_layout"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_order_layout.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: "), out.stdout
    assert int(out.stdout.split()[1]) > 1000, out.stdout
