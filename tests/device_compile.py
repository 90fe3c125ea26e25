"""One device-only compile of a kernel source per test session (hipcc cross-compiles without a GPU): the ISA text and the
compiler's kernel-resource remarks come from the same run, shared by test_kernel_resources.py, the *_isa.py tests and tools/isa_diff.py."""
import collections
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc")


@functools.lru_cache(maxsize=None)
def compile_device(source, csrc=CSRC):
    """(assembly text, {demangled kernel name: resources}) of csrc/<source> for gfx950 at the library's optimisation level"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, source + ".s")
        p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-DHJGPU_KERNEL_HASH=\"isa\"", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, source), "-o", out],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        text = open(out).read()
    rows, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = m.group(2)
            rows[cur] = {}
        elif cur:
            rows[cur][m.group(1).split(" [")[0]] = m.group(2)
    names = list(rows)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines() if names else []
    res = {}
    for mangled, name in zip(names, plain):
        r = rows[mangled]
        res[name.strip()] = dict(vgpr=int(r.get("VGPRs", 0)), vspill=int(r.get("VGPRs Spill", 0)), sspill=int(r.get("SGPRs Spill", 0)),
                                 scratch=int(r.get("ScratchSize", 0)), occ=int(r.get("Occupancy", 0)))
    return text, res


def split_kernels(text, name=""):
    """{mangled symbol: body up to s_endpgm} of the kernels in an assembly text whose (unmangled) name starts with `name` (default: every kernel)"""
    out = {}
    for m in re.finditer(r"^(_Z%s\w+):\s*; @" % (r"\d+" + name if name else ""), text, re.M):
        out[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    return out


def instances(source, name=""):
    """({mangled symbol: body}, resources) of the instances of kernel `name` in csrc/<source>"""
    text, res = compile_device(source)
    return split_kernels(text, name), res


STORE = re.compile(r"^(global|flat|buffer)_store_(\w+)")


def _stores(body):
    """Counter{(width of a global store: dword, dwordx4 ..., non-temporal?): n} of a kernel body"""
    stores = collections.Counter()
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        hit = STORE.match(line)
        if hit:
            stores[(hit.group(2), " nt" in line)] += 1
    return stores


SLOAD = re.compile(r"s_load_dword(?:x(\d+))?\s+s\[?[\d:]+\]?,\s*s\[\d+:\d+\],\s*0x([0-9a-f]+)")


def kernarg_bytes(body):
    """the kernel-argument bytes the instance's scalar loads read (offsets are bytes into the argument struct)"""
    covered = set()
    for m in SLOAD.finditer(body):
        off, n = int(m.group(2), 16), int(m.group(1) or 1)
        covered.update(range(off, off + 4 * n))
    return covered
