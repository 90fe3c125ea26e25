"""CPU test (hipcc cross-compiles without a GPU): the kernels of hjgpu_order_by in gen_kernels.hip exist for gfx950 in exactly the six
planned instances - the LDS road's one kernel, the iota, and the device road's histogram, scan, scatter and gather -, use no scratch and
no spills, store every global word non-temporally and through global_ instructions alone, and the LDS road's workgroup fits its LDS and
holds order_layout.hpp's rows.  Plus the two entry points in the library, in EXPORTS and on HjGpu, and the header's constants against api's.
Stores and resources only."""
import os
import re
import subprocess

import pytest

from device_compile import compile_device, _stores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "gen_kernels.hip"
ENTRY_POINTS = ["hjgpu_order_by", "hjgpu_order_by_async"]
INSTANCES = {"_Z16order_lds_kernel12OrderLdsArgs", "_Z17order_iota_kernelPjyyPy", "_Z22order_histogram_kernel13OrderPassArgs",
             "_Z17order_scan_kernel13OrderPassArgs", "_Z20order_scatter_kernel13OrderPassArgs", "_Z19order_gather_kernel15OrderGatherArgs"}
LDS_BYTES_PER_CU = 160 * 1024


def kernel_texts():
    """{mangled symbol: the kernel's whole text, from its label to the end of its function}"""
    text, _ = compile_device(SOURCE)
    out = {}
    for m in re.finditer(r"^(_Z\d+order_\w+):\s*; @", text, re.M):
        out[m.group(1)] = text[m.end():text.find(".Lfunc_end", m.end())]
    return out


def layout_constant(name):
    header = open(os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc", "order_layout.hpp")).read()
    return int(re.search(r"\b%s = (\d+)" % name, header).group(1))


def test_every_planned_instance_exists():
    assert set(kernel_texts()) == INSTANCES, sorted(kernel_texts())


def test_no_scratch_no_spills():
    _, res = compile_device(SOURCE)
    rows = {k: v for k, v in res.items() if re.match(r"(void )?order_\w+_kernel\(", k)}
    assert len(rows) == len(INSTANCES), sorted(rows)
    bad = {k: v for k, v in rows.items() if v["scratch"] or v["vspill"] or v["sspill"]}
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_every_global_store_is_non_temporal_and_nothing_is_flat(name):
    body = kernel_texts()[name]
    ins = [line.split(";")[0].strip() for line in body.splitlines() if line.split(";")[0].strip()]
    stores = _stores(body)
    assert stores and not {s: n for s, n in stores.items() if not s[1]}, stores
    assert not [i for i in ins if i.startswith("flat_") or i.startswith("scratch_")], [i for i in ins if i.startswith("flat_") or i.startswith("scratch_")]


def test_the_lds_roads_workgroup_fits_its_lds():
    """one workgroup of LDS_BLOCK lanes holds LDS_ROWS row numbers and 64-bit keys beside the ranking tables; the device road's scatter
    leaves room for order_layout.hpp's RESIDENT workgroups per CU"""
    text, res = compile_device(SOURCE)
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S*order_\S*)\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text, re.M)}
    assert set(lds) == INSTANCES, sorted(lds)
    rows, block = layout_constant("LDS_BLOCK") * layout_constant("LDS_ITEMS"), layout_constant("LDS_BLOCK")
    assert rows >= 4096 and block == 1024
    assert rows * 12 <= lds["_Z16order_lds_kernel12OrderLdsArgs"] <= LDS_BYTES_PER_CU, lds
    resident = layout_constant("RESIDENT")
    assert lds["_Z20order_scatter_kernel13OrderPassArgs"] * resident <= LDS_BYTES_PER_CU, lds
    occ = {k: v["occ"] for k, v in res.items() if re.match(r"(void )?order_(scatter|histogram)_kernel\(", k)}
    assert len(occ) == 2 and all(v >= resident for v in occ.values()), occ
    # the LDS road's 16 waves are 4 per SIMD
    assert [v["occ"] for k, v in res.items() if k.startswith("order_lds_kernel(")] == [4], res


def test_entry_points_in_the_library_and_the_binding():
    import hash_join_codes_knl_amd as H
    lib = H.load_library()
    assert not [s for s in ENTRY_POINTS if not hasattr(lib, s)]
    assert not [s for s in ENTRY_POINTS if s not in H.EXPORTS]
    assert not [s for s in ENTRY_POINTS if not callable(getattr(H.HjGpu, s[len("hjgpu_"):], None))]


def test_constants_match_the_header(tmp_path):
    """the HJGPU_ORDER_* constants and the two structs' sizes as gcc reads them from include/hjgpu.h equal api's"""
    import ctypes
    from hash_join_codes_knl_amd import api
    src = tmp_path / "constants.c"
    src.write_text('#include <stdio.h>\n#include "hjgpu.h"\nint main(void){printf("%u %u %u %u %u %zu %zu\\n", HJGPU_ORDER_MAX_KEYS, HJGPU_ORDER_MAX_COLS, '
                   'HJGPU_ORDER_DESC, HJGPU_ORDER_SIGNED, HJGPU_ORDER_WIDE, sizeof(hjgpu_order_key), sizeof(hjgpu_order_column));return 0;}\n')
    exe = tmp_path / "constants"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [api.ORDER_MAX_KEYS, api.ORDER_MAX_COLS, api.ORDER_DESC, api.ORDER_SIGNED, api.ORDER_WIDE,
                   ctypes.sizeof(api.OrderKey), ctypes.sizeof(api.OrderColumn)] == [4, 8, 1, 2, 4, 16, 24], got
    assert (layout_constant("MAX_KEYS"), layout_constant("MAX_COLS")) == (api.ORDER_MAX_KEYS, api.ORDER_MAX_COLS)
