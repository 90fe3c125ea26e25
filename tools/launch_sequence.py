"""Every road of the PHJ / NPJ enqueue path once, at small shapes ("Roads of the PHJ enqueue path").

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_sequence.py
    python tools/launch_sequence.py --summarise DIR/.../*_kernel_trace.csv > profiles/r14_launch_sequence.txt

With --multi in both forms: the roads of the multi-GPU joins instead ("Roads of a CPRA step"), on ONE device - the
loopback transport puts the ranks of a world of 2 or 3 on device 0, RCCL runs at world 1 - through HjComm.  With more than one rank
every rank enqueues from its own host thread, so the order between the ranks' launches is timing: those roads' lines are printed sorted.
tests/test_gpu_cpra_roads.py checks what they compute.

The first form runs the roads against the library HJGPU_LIBRARY names (default: the tree's own).  One column_sums_kernel launch
precedes every road, so the second form can cut the kernel trace into roads and print, per road, the ordered list of
(kernel, grid, workgroup, LDS bytes).  Two builds enqueue the same work exactly when their lists are equal (plain diff).
Option "placement" is 1 on every context (the placement search's probe launches depend on timing); all seeds are fixed.
tests/test_gpu_phj_roads.py runs the same roads and checks what they compute."""
import csv
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M64 = (1 << 64) - 1
INNER, OUTER, OUTER_BATCHED = 5_003, 40_009, 7_300_003      # (the batched road engages from test_gpu_shapes.py's probe size on)
BATCH_TUPLES = 300_000                                      # test_gpu_shapes.py test_batched_probe_side_partitioning
GROUP_FROM, GROUP_INNER = 1000, 5000                        # test_gpu_grouped.py: 2 groups of the 5 003 build rows
FACTOR1 = 0x2C1B3C6D                                        # the exchange-level hash of the pre-partitioned road
GROUP_INNER_SHARE = 1250                                    # a rank's share of the build side at world 2 (2 501 rows): 2 groups or more
DELIMITER = "column_sums_kernel"


def relations(outer=OUTER, seed=14):
    """build: INNER rows over 4 000 distinct keys (1 003 of them twice); probe: `outer` rows, about half of them with a build key.
    Keys are never 0 (NPJ's empty bucket), payloads never 0xFFFFFFFF (the outer joins' NULL)."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, 2**32 - 1, size=12_000, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    base, miss = pool[:4000], pool[4000:]
    ik = np.concatenate([base, base[:INNER - 4000]])
    iv = rng.integers(0, 2**32 - 1, size=INNER, dtype=np.uint64).astype(np.uint32)
    ok = np.where(rng.random(outer) < 0.5, base[rng.integers(0, 3000, size=outer)], miss[rng.integers(0, len(miss), size=outer)]).astype(np.uint32)
    ov = rng.integers(0, 2**32 - 1, size=outer, dtype=np.uint64).astype(np.uint32)
    return ik, iv, ok, ov


def mulhi_hash(keys, factor, n):
    x = (keys.astype(np.uint64) * np.uint64(factor)) & np.uint64(0xFFFFFFFF)
    return ((x * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def add(a, b):
    return tuple((int(x) + int(y)) & M64 for x, y in zip(a, b))


def prm(**kw):
    import hash_join_codes_knl_amd as H
    kw.setdefault("fanout1", 8)
    kw.setdefault("fanout2", 4)
    return H.PhjParams(**kw)


class Run:
    """one road's context, relations and device columns"""

    def __init__(self, rel, options=()):
        import hash_join_codes_knl_amd as H
        self.H, self.hj, self.made = H, H.HjGpu(0), []
        self.ik, self.iv, self.ok, self.ov = rel
        for k, v in (("placement", 1),) + tuple(options):
            self.hj.set_option(k, v)
        self.rk, self.rv, self.sk, self.sv = (self.col(a) for a in rel)

    def col(self, a, dtype=np.uint32):
        if not isinstance(a, (int, np.integer)) and len(a) == 0:
            a = 4
        c = self.hj.column(a, dtype)
        self.made.append(c)
        return c

    def rows_out(self, rows, algorithm=1, block=256):
        cap = self.hj.output_capacity(algorithm, len(self.ok), rows, block)
        return tuple(self.col(np.zeros(max(cap, 4), np.uint32)) for _ in range(3)) + (cap, block)

    def whole(self):
        return (self.rk, self.rv, len(self.ik), self.sk, self.sv, len(self.ok))

    def result_of(self, d_res):
        return tuple(int(x) for x in d_res.download())

    def close(self):
        for c in self.made:
            c.free()
        self.hj.close()


def out_rows(out, n):
    return tuple(c.download(n) for c in out[:3])


# ---- the roads: fn(Run) -> {"agg": aggregates, "rows": (keys, outer_vals, inner_vals) or None, "stats": hjgpu_get_stats} ------------------
def road_phj(r, params=None, **kw):
    agg = r.hj.phj(*r.whole(), params or prm(), **kw)
    return {"agg": agg, "stats": r.hj.stats()}


def road_async(r):
    d_res = r.col(4, np.uint64)
    r.hj.phj_async(*r.whole(), prm(), d_res)
    r.hj.get_async_status()
    return {"agg": r.result_of(d_res), "stats": r.hj.stats()}


def road_overlapped(r):
    """the build side is there already: an event recorded on the null stream, torch's where torch shares the process (conftest.py)"""
    d_res = r.col(4, np.uint64)
    if "torch" in sys.modules:
        import torch
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        r.hj.phj_overlapped_async(*r.whole(), prm(), d_res, None, ready.cuda_event)
    else:
        hip = ctypes.CDLL("libamdhip64.so")
        ev = ctypes.c_void_p()
        assert hip.hipEventCreate(ctypes.byref(ev)) == 0 and hip.hipEventRecord(ev, None) == 0
        r.hj.phj_overlapped_async(*r.whole(), prm(), d_res, None, ev)
    r.hj.get_async_status()
    if "torch" not in sys.modules:
        assert hip.hipEventDestroy(ev) == 0
    return {"agg": r.result_of(d_res), "stats": r.hj.stats()}


def road_build_probe(r):
    cut = (len(r.ok) * 3 // 7) & ~15
    r.hj.phj_build(r.rk, r.rv, len(r.ik), len(r.ok) - cut, prm())
    a = r.hj.phj_probe(r.sk, r.sv, cut)
    b = r.hj.phj_probe(r.sk.ptr + 4 * cut, r.sv.ptr + 4 * cut, len(r.ok) - cut)
    return {"agg": add(a, b), "stats": r.hj.stats()}


def road_prepartitioned(r, counted):
    """two senders' pieces of 8 exchange-level partitions each, partitioned on the host; one receiver owns all 8"""
    fanout, f2 = 8, 4

    def pieces(keys, vals):
        half = (len(keys) // 2) & ~15
        tuples, offs, counts = [], [0], []
        for b, e in ((0, half), (half, len(keys))):
            p1 = mulhi_hash(keys[b:e], FACTOR1, fanout)
            order = np.argsort(p1, kind="stable")
            tuples.append(((vals[b:e].astype(np.uint64) << np.uint64(32)) | keys[b:e].astype(np.uint64))[order])
            offs.append(offs[-1] + (e - b))
            counts.append(np.bincount(p1 * f2 + mulhi_hash(keys[b:e], 0x85EBCA6B, f2), minlength=fanout * f2))
        return np.concatenate(tuples + [np.zeros(2, np.uint64)]), offs, np.concatenate(counts).astype(np.uint64)

    tr, offr, _ = pieces(r.ik, r.iv)
    ts, offs, cs = pieces(r.ok, r.ov)
    dr, ds, d_res = r.col(tr, np.uint64), r.col(ts, np.uint64), r.col(4, np.uint64)
    r.hj.phj_build_prepartitioned(dr, r.hj.prepartitioned(FACTOR1, fanout, 0, fanout, offr), max(len(r.ok), 1 << 16), r.H.PhjParams(fanout2=f2))
    lay = r.hj.prepartitioned(FACTOR1, fanout, 0, fanout, offs)
    if counted:
        r.hj.phj_probe_prepartitioned_counted_async(ds, lay, r.col(cs, np.uint64), d_res)
    else:
        r.hj.phj_probe_prepartitioned_async(ds, lay, d_res)
    r.hj.get_async_status()
    return {"agg": r.result_of(d_res), "stats": r.hj.stats()}


def road_cpra(r, chunks):
    agg = r.hj.cpra(*r.whole(), prm(chunks=chunks))
    return {"agg": agg, "stats": r.hj.stats()}


def road_rows(r, flags, rows, two_columns=False):
    """a mode that marks build rows, materialised: `rows` result rows"""
    out = r.rows_out(rows)
    agg = r.hj.phj(*r.whole(), prm(flags=flags), out=out)
    k, o, i = out_rows(out, agg[0])
    return {"agg": agg, "rows": (k, i) if two_columns else (k, o, i), "stats": r.hj.stats()}


def road_npj(r):
    agg = r.hj.npj(*r.whole())
    vals, bits = r.col(len(r.ok)), r.col((len(r.ok) + 31) // 32)
    look = r.hj.npj_lookup(r.rk, r.rv, len(r.ik), r.sk, len(r.ok), None, vals, bits)
    return {"agg": agg, "stats": r.hj.stats(), "lookup": look, "lookup_vals": vals.download(), "lookup_bits": bits.download()}


def road_join_host(r, algorithm):
    agg, stats = r.hj.join_host(algorithm, r.ik, r.iv, r.ok, r.ov, prm() if algorithm else None)
    return {"agg": agg, "stats": stats}


def _inner_rows(r):
    """rows of the inner join (the right outer join adds the build rows without a partner)"""
    lo, hi = np.searchsorted(np.sort(r.ik), r.ok, "left"), np.searchsorted(np.sort(r.ik), r.ok, "right")
    return int((hi - lo).sum())


NAMES = ["01 phj", "02 phj exact_probe_counts", "03 phj merged_plan 0", "04 phj_async", "05 phj_overlapped_async", "06 phj_build + 2 phj_probe",
         "07a prepartitioned", "07b prepartitioned counted", "08a cpra 8 chunks", "08b cpra 12 chunks", "09 one pass", "10 dense2", "11 batch_tuples",
         "12 grouped device-planned", "13 grouped host-planned", "14 audit", "15 right outer rows", "16 right semi rows",
         "17 full outer empty probe", "18 npj + npj_lookup", "19a join_host phj", "19b join_host npj"]


def roads():
    """[(name, options, relations, fn)] in the order of NAMES"""
    import hash_join_codes_knl_amd as H
    rel = relations()
    empty = rel[:2] + (rel[2][:0], rel[3][:0])
    grouped = (("group_from", GROUP_FROM), ("group_always", 1), ("group_inner", GROUP_INNER))
    unmatched = int((~np.isin(rel[0], rel[2])).sum())
    table = [
        ("01 phj", (), rel, road_phj),
        ("02 phj exact_probe_counts", (("exact_probe_counts", 1),), rel, road_phj),
        ("03 phj merged_plan 0", (("merged_plan", 0),), rel, road_phj),
        ("04 phj_async", (), rel, road_async),
        ("05 phj_overlapped_async", (), rel, road_overlapped),
        ("06 phj_build + 2 phj_probe", (), rel, road_build_probe),
        ("07a prepartitioned", (), rel, lambda r: road_prepartitioned(r, False)),
        ("07b prepartitioned counted", (), rel, lambda r: road_prepartitioned(r, True)),
        ("08a cpra 8 chunks", (), rel, lambda r: road_cpra(r, 8)),
        ("08b cpra 12 chunks", (), rel, lambda r: road_cpra(r, 12)),
        ("09 one pass", (), rel, lambda r: road_phj(r, prm(fanout1=32, fanout2=1))),
        ("10 dense2", (("dense2", 1),), rel, road_phj),
        ("11 batch_tuples", (("batch_tuples", BATCH_TUPLES),), relations(OUTER_BATCHED), road_phj),
        ("12 grouped device-planned", grouped, rel, lambda r: road_phj(r, H.PhjParams())),
        ("13 grouped host-planned", grouped + (("group_device", 0),), rel, lambda r: road_phj(r, H.PhjParams())),
        ("14 audit", (("audit", 1),), rel, road_phj),
        ("15 right outer rows", (), rel, lambda r: road_rows(r, H.FLAG_RIGHT_OUTER, _inner_rows(r) + unmatched)),
        ("16 right semi rows", (), rel, lambda r: road_rows(r, H.FLAG_RIGHT_SEMI, INNER - unmatched, two_columns=True)),
        ("17 full outer empty probe", (), empty, lambda r: road_rows(r, H.FLAG_FULL_OUTER, INNER)),
        ("18 npj + npj_lookup", (), rel, road_npj),
        ("19a join_host phj", (), rel, lambda r: road_join_host(r, 1)),
        ("19b join_host npj", (), rel, lambda r: road_join_host(r, 0)),
    ]
    assert [t[0] for t in table] == NAMES
    return table


# ---- the multi-GPU roads: fn(MultiRun) -> {"agg": aggregates, "rows": (keys, outer_vals, inner_vals) or None, "stats": hjgpu_multi_stats} ---
def bounds(n, parts, alignment=16):
    """thread_beg / thread_end (npj.cpp:516-529): how the hosts cut a relation into the ranks' chunks"""
    part = (n // parts) & ~(alignment - 1)
    return [(part * t, n if t + 1 == parts else part * (t + 1)) for t in range(parts)]


class MultiRun:
    """one road's communicator (fresh buffers), relations and device columns"""

    def __init__(self, world, transport, rel, comm_options=(), ctx_options=()):
        import hash_join_codes_knl_amd as H
        self.H, self.made, self.rel = H, [], rel
        self.comm = H.HjComm.local(world, [0] * world, H.TRANSPORT_RCCL if transport == "rccl" else H.TRANSPORT_LOOPBACK)
        for ctx in self.comm.ctx:
            for k, v in (("placement", 1),) + tuple(ctx_options):
                ctx.set_option(k, v)
        for k, v in comm_options:
            self.comm.set_option(k, v)

    def col(self, g, a):
        c = self.comm.ctx[g].column(np.concatenate([a, np.zeros(4, a.dtype)]))
        self.made.append(c)
        return c

    def chunked(self, rcuts=None, scuts=None):
        """both relations in chunks, one per rank"""
        ik, iv, ok, ov = self.rel
        G = self.comm.nranks
        rcuts, scuts = rcuts or bounds(len(ik), G), scuts or bounds(len(ok), G)
        return [(self.col(g, ik[rb:re]), self.col(g, iv[rb:re]), re - rb, self.col(g, ok[sb:se]), self.col(g, ov[sb:se]), se - sb)
                for g, ((rb, re), (sb, se)) in enumerate(zip(rcuts, scuts))]

    def replicated(self, root=0):
        """the build side on the root, the probe side in chunks"""
        ik, iv, ok, ov = self.rel
        return [(self.col(g, ik) if g == root else None, self.col(g, iv) if g == root else None, len(ik), self.col(g, ok[sb:se]), self.col(g, ov[sb:se]), se - sb)
                for g, (sb, se) in enumerate(bounds(len(ok), self.comm.nranks))]

    def rows_out(self, shards, rows, block=256):
        outs = []
        for g, sh in enumerate(shards):
            cap = self.comm.ctx[g].output_capacity(1, sh[5], rows, block)
            outs.append(tuple(self.col(g, np.zeros(max(cap, 4), np.uint32)) for _ in range(3)) + (cap, block))
        return outs

    def close(self):
        for c in self.made:
            c.free()
        self.comm.close()


def mroad_cpra(m, params=None, cuts=None):
    agg, st = m.comm.cpra_multi(m.chunked(*(cuts or ())), params or prm(), 3)
    return {"agg": agg, "stats": st}


def mroad_cpra_rows(m):
    """every rank's columns hold the whole result: a rank's rows are the first `counts[g]` of its columns"""
    shards = m.chunked()
    outs = m.rows_out(shards, 2 * len(m.rel[2]))
    agg, st, counts = m.comm.cpra_multi_rows(shards, outs, prm(), 3)
    cols = tuple(np.concatenate([o[i].download(n) for o, n in zip(outs, counts)]) for i in range(3))
    return {"agg": agg, "rows": cols, "stats": st}


def mroad_replicated(m, algorithm):
    shards = m.replicated()
    agg, st = m.comm.phj_multi(shards, 0, prm()) if algorithm else m.comm.npj_multi(shards, 0)
    return {"agg": agg, "stats": st}


def mroad_join_host(m, algorithm, rows):
    ik, iv, ok, ov = m.rel
    if not rows:
        agg, st = m.comm.join_host_multi(algorithm, ik, iv, ok, ov, prm())
        return {"agg": agg, "stats": st}
    agg, st, cols = m.comm.join_host_rows_multi(algorithm, ik, iv, ok, ov, 2 * len(ok), prm())
    return {"agg": agg, "rows": cols, "stats": st}


def _one_rank_empty(world=3):
    """rank 1 holds nothing of either relation"""
    def cuts(n):
        (b0, e0), (_, e1) = bounds(n, world - 1)
        return [(b0, e0), (e0, e0), (e0, e1)]
    return cuts(INNER), cuts(OUTER)


MULTI_NAMES = ["20a cpra loopback 2 in place", "20b cpra loopback 2 exchange_in_place 0", "20c cpra loopback 2 cpra_fused_counts 0",
               "20d cpra loopback 2 cpra_two_level 1", "20e cpra loopback 2 grouped", "20f cpra loopback 2 rows", "21 cpra loopback 3 one rank empty",
               "22a cpra rccl 1 cpra_k 24", "22b cpra rccl 1 self_via_rccl", "23a join_host_multi cpra", "23b join_host_multi phj",
               "23c join_host_rows_multi cpra", "23d join_host_rows_multi phj", "24a phj_multi loopback 2", "24b npj_multi loopback 2"]
# more than one rank: the ranks' host threads enqueue side by side, the summary sorts the road's lines
SORTED = {n for n in MULTI_NAMES if not n.startswith("22")}


def multi_roads():
    """[(name, world, transport, communicator options, context options, fn)] in the order of MULTI_NAMES; all on the relations of roads()"""
    import hash_join_codes_knl_amd as H
    grouped = (("group_from", GROUP_FROM), ("group_always", 1), ("group_inner", GROUP_INNER_SHARE))
    table = [
        ("20a cpra loopback 2 in place", 2, "loopback", (), (), mroad_cpra),
        ("20b cpra loopback 2 exchange_in_place 0", 2, "loopback", (("exchange_in_place", 0),), (), mroad_cpra),
        ("20c cpra loopback 2 cpra_fused_counts 0", 2, "loopback", (("cpra_fused_counts", 0),), (), mroad_cpra),
        ("20d cpra loopback 2 cpra_two_level 1", 2, "loopback", (("cpra_two_level", 1),), (), mroad_cpra),
        ("20e cpra loopback 2 grouped", 2, "loopback", (("cpra_grouped", 2),), grouped, lambda m: mroad_cpra(m, H.PhjParams())),
        ("20f cpra loopback 2 rows", 2, "loopback", (), (), mroad_cpra_rows),
        ("21 cpra loopback 3 one rank empty", 3, "loopback", (), (), lambda m: mroad_cpra(m, cuts=_one_rank_empty())),
        ("22a cpra rccl 1 cpra_k 24", 1, "rccl", (("cpra_k", 24),), (), mroad_cpra),
        ("22b cpra rccl 1 self_via_rccl", 1, "rccl", (("self_via_rccl", 1),), (), mroad_cpra),
        ("23a join_host_multi cpra", 2, "loopback", (), (), lambda m: mroad_join_host(m, 2, False)),
        ("23b join_host_multi phj", 2, "loopback", (), (), lambda m: mroad_join_host(m, 1, False)),
        ("23c join_host_rows_multi cpra", 2, "loopback", (), (), lambda m: mroad_join_host(m, 2, True)),
        ("23d join_host_rows_multi phj", 2, "loopback", (), (), lambda m: mroad_join_host(m, 1, True)),
        ("24a phj_multi loopback 2", 2, "loopback", (), (), lambda m: mroad_replicated(m, 1)),
        ("24b npj_multi loopback 2", 2, "loopback", (), (), lambda m: mroad_replicated(m, 0)),
    ]
    assert [t[0] for t in table] == MULTI_NAMES
    return table


def run_multi_road(world, transport, comm_options, ctx_options, fn, rel=None):
    m = MultiRun(world, transport, rel or relations(), comm_options, ctx_options)
    try:
        return fn(m)
    finally:
        m.close()


def run_road(options, rel, fn):
    r = Run(rel, options)
    try:
        return fn(r)
    finally:
        r.close()


def main(multi=False):
    try:
        import torch                    # (its own HIP runtime has to initialise first where both live in one process, as in bench.py)
        torch.cuda.init()
    except ImportError:
        pass
    import hash_join_codes_knl_amd as H
    print("library", H.build.lib_path(), "hash", H.library_hash())
    with H.HjGpu(0) as mark:
        d = mark.column(np.arange(1024, dtype=np.uint32))
        for name, world, transport, comm_options, ctx_options, fn in (multi_roads() if multi else ()):
            mark.column_sums(d, 1024, 1, 3)              # the delimiter in front of the road
            mark.synchronize()
            got = run_multi_road(world, transport, comm_options, ctx_options, fn)
            st = got["stats"]
            print("%-40s agg %s joins %d self_copies %d groups %d" % (name, got["agg"], st["joins"], st["self_copies"], st["join"]["groups"]), flush=True)
        for name, options, rel, fn in (() if multi else roads()):
            mark.column_sums(d, 1024, 1, 3)              # the delimiter in front of the road
            mark.synchronize()
            got = run_road(options, rel, fn)
            st = got["stats"]
            print("%-32s agg %s fanout %dx%d batches %d groups %d" % (name, got["agg"], st["fanout1"], st["fanout2"], st["batches"], st["groups"]), flush=True)
        d.free()


def summarise(path, names=NAMES):
    """the kernel trace of main() -> one block per road"""
    with open(path, newline="") as fh:
        trace = sorted(csv.DictReader(fh), key=lambda t: int(t["Dispatch_Id"]))
    blocks = []
    for t in trace:
        kernel = t["Kernel_Name"]
        if DELIMITER in kernel:
            blocks.append((names[len(blocks)] if len(blocks) < len(names) else "road %d" % len(blocks), []))
            continue
        if not blocks:
            continue
        grid = "x".join(t["Grid_Size_" + a] for a in "XYZ")
        wg = "x".join(t["Workgroup_Size_" + a] for a in "XYZ")
        blocks[-1][1].append("%s grid %s wg %s lds %s" % (kernel, grid, wg, t.get("LDS_Block_Size", t.get("Group_Segment_Size", "?"))))
    for name, lines in blocks:
        print("\n== %s%s" % (name, " (sorted)" if name in SORTED else ""))
        print("\n".join(sorted(lines) if name in SORTED else lines))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--multi"]
    multi = "--multi" in sys.argv[1:]
    if len(args) == 2 and args[0] == "--summarise":
        summarise(args[1], MULTI_NAMES if multi else NAMES)
    else:
        main(multi)
