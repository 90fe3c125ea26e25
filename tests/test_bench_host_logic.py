"""CPU tests of bench.py's host-side logic (no GPU): argument defaults of the contract, the CPU allowance
the CPU baseline uses, that a GPU-less run fails loudly instead of falling back to anything, and what --dump-outputs
writes; GPU tests run a small bench and check its line, its dumped outputs and what --full adds to a plain run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_usable_cpus_respects_affinity_and_quota(tmp_path, monkeypatch):
    import bench
    n = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)
    assert n <= len(os.sched_getaffinity(0))
    # a cgroup quota of 2.5 CPUs caps an 8-CPU affinity mask at 3 threads; "max" leaves it alone
    real_open = open

    def fake_open(path, *a, **k):
        if path == "/sys/fs/cgroup/cpu.max":
            return real_open(tmp_path / "cpu.max", *a, **k)
        return real_open(path, *a, **k)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(8)))
    monkeypatch.setattr("builtins.open", fake_open)
    (tmp_path / "cpu.max").write_text("250000 100000\n")
    assert bench.usable_cpus() == 3
    (tmp_path / "cpu.max").write_text("max 100000\n")
    assert bench.usable_cpus() == 8
    (tmp_path / "cpu.max").write_text("1600000 100000\n")
    assert bench.usable_cpus() == 8


def test_bench_defaults_follow_the_contract():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for flag, default in (("--gpus", "default=1"), ("--steps", "default=10"), ("--warmup", "default=2"),
                          ("--inner", "default=64_000_000"), ("--outer", "default=1_000_000_000")):
        line = [l for l in src.splitlines() if 'add_argument("%s"' % flag in l]
        assert line and default in line[0], (flag, line)


def test_bench_without_a_gpu_fails_loudly():
    """No CPU fallback: on a box without a GPU the bench must exit non-zero, not print a number."""
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("a GPU is present")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--cpu-outer", "0",
                        "--inner", "1000", "--outer", "10000"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.startswith("{") and '"value"' in l]


def test_library_hash_covers_every_source_of_the_library(tmp_path, monkeypatch):
    """evidence headers name the LIBRARY: two trees that differ only in the orchestration (hjgpu_multi.hip) hash differently,
    while the kernel hash - which gates PMC traffic - stays"""
    import shutil
    from hash_join_codes_knl_amd import build as B
    k0, l0 = B.kernel_hash(), B.library_hash()
    root = tmp_path / "tree"
    shutil.copytree(B.CSRC, root / "hash_join_codes_knl_amd" / "csrc")
    (root / "include").mkdir()
    shutil.copy(os.path.join(B.ROOT, "include", "hjgpu.h"), root / "include" / "hjgpu.h")
    monkeypatch.setattr(B, "CSRC", str(root / "hash_join_codes_knl_amd" / "csrc"))
    monkeypatch.setattr(B, "ROOT", str(root))
    assert (B.kernel_hash(), B.library_hash()) == (k0, l0)
    with open(root / "hash_join_codes_knl_amd" / "csrc" / "hjgpu_multi.hip", "a") as f:
        f.write("\n// one more line in the orchestration\n")
    assert B.kernel_hash() == k0 and B.library_hash() != l0
    with open(root / "include" / "hjgpu.h", "a") as f:
        f.write("\n")
    l1 = B.library_hash()
    with open(root / "hash_join_codes_knl_amd" / "csrc" / "exchange_layout.hpp", "a") as f:
        f.write("\n")
    assert B.library_hash() != l1


def test_bench_steps_must_be_a_positive_count():
    """--steps is the number of timed steps and ms_per_step their wall clock divided by it: zero steps is refused"""
    import bench
    assert bench.parse(["--steps", "7", "--warmup", "0"]).steps == 7
    for bad in (["--steps", "0"], ["--steps", "-2"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_bench_full_is_off_by_default():
    """a plain run measures the headline only; --full adds the measurements that take runs of their own"""
    import bench
    assert bench.parse([]).full is False
    assert bench.parse(["--full"]).full is True


def test_bench_dump_outputs_holds_the_aggregates_exactly(tmp_path):
    """--dump-outputs: the four uint64 aggregates as float64, and as 32-bit words that float64 holds exactly"""
    import numpy as np
    import bench
    vals = [1_000_000_000, (1 << 64) - 1, (1 << 53) + 1, 0]
    names = bench.dump_outputs(str(tmp_path / "out"), vals)
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == [n + ".npy" for n in names] == ["result.npy", "result_u32_words.npy"]
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) < 64 << 20
    res = np.load(tmp_path / "out" / "result.npy")
    words = np.load(tmp_path / "out" / "result_u32_words.npy")
    assert res.dtype == words.dtype == np.float64 and res.shape == (4,) and words.shape == (4, 2)
    assert res.tolist() == [float(v) for v in vals]
    assert [(int(hi) << 32) | int(lo) for hi, lo in words] == vals


@pytest.mark.gpu
def test_bench_dumps_what_its_last_timed_step_returned(tmp_path):
    """A small bench run: the line reports the timed steps asked for, and the dumped arrays are its join result"""
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--cpu-outer", "0",
           "--no-secondary", "--inner", "1000000", "--outer", "8000000", "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["checksum_ok"] is True
    r = line["result"]
    want = [r["count"], r["sum_keys"], r["sum_outer_vals"], r["sum_inner_vals"]]
    words = np.load(tmp_path / "out" / "result_u32_words.npy")
    assert [(int(hi) << 32) | int(lo) for hi, lo in words] == want
    assert np.load(tmp_path / "out" / "result.npy").tolist() == [float(v) for v in want]


@pytest.mark.gpu
def test_bench_plain_run_leaves_the_extras_to_full():
    """Without --full the line has no CPU baseline and no streaming-read ceiling; with it, both are measured and the
    CPU restatement's checksum agrees.  The headline itself is checked in both runs."""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
            "--inner", "1000000", "--outer", "8000000"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full"])):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        got = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(got) == 1
        lines[name] = json.loads(got[0])
        assert lines[name]["checksum_ok"] is True and lines[name]["steps"] == 2 and lines[name]["warmup"] == 1
    plain, full = lines["plain"], lines["full"]
    assert "cpu_baseline" not in plain and "secondary" not in plain
    assert plain["empirical_stream_read_GBs"] is None and plain["roofline"]["frac_of_stream_read"] is None
    assert full["empirical_stream_read_GBs"] > 0 and full["roofline"]["frac_of_stream_read"] > 0
    assert full["cpu_baseline"]["value"] is not None and "checksum ok" in full["cpu_baseline"]["sample"]
