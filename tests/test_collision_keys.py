"""CPU test of tests/collision_keys.py: the numpy port of the grouped operators' hashes and the key tuples crafted to collide in their
tables (the inputs of tests/test_gpu_group_collisions.py).

tests/cpp_collision_keys.cpp includes csrc/group_layout.hpp and csrc/wide_group_layout.hpp and writes, for the tuples of a file,
hj_group::mix / lds_home and hj_wide::hash / lds_home, and the layouts' constants.  The port must equal it on random and edge tuples, and
every crafted set must - by the compiled functions, not the port - consist of distinct tuples, have the homes it was asked for and
satisfy the counting conditions its scenario rests on.  So a changed hash or table size fails here; the GPU tests do not quietly turn into
tests of random keys."""
import os
import subprocess

import numpy as np
import pytest

import collision_keys as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def headers(tmp_path_factory):
    """f(keys [S, nkeys]) -> (mix, its lds_home, wide hash, its lds_home) [S] uint64 each, and the constants, by the headers"""
    tmp = tmp_path_factory.mktemp("collision_keys")
    exe = tmp / "collision_keys"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "hash_join_codes_knl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp_collision_keys.cpp"), "-o", str(exe)])

    def run(keys):
        keys = np.asarray(keys, np.uint32)
        four = np.zeros((len(keys), 4), np.uint32)
        four[:, :keys.shape[1]] = keys
        src, dst = tmp / "in.bin", tmp / "out.bin"
        src.write_bytes(np.array([keys.shape[1], len(keys)], np.uint32).tobytes() + four.tobytes())
        out = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        consts = {f[0]: (int(f[1]), int(f[2])) for f in (line.split() for line in out.stdout.splitlines())}
        words = np.fromfile(dst, np.uint64).reshape(len(keys), 4)
        return words[:, 0], words[:, 1], words[:, 2], words[:, 3], consts
    return run


def header_hash(headers, keys):
    """the hash and the LDS home that the tables of a tuple's layout use, by the headers"""
    m, mh, w, wh, _ = headers(keys)
    return (m, mh) if keys.shape[1] <= C.NARROW.MAX_KEYS else (w, wh)


def check_port(headers, keys):
    nkeys = keys.shape[1]
    m, mh, w, wh, _ = headers(keys)
    k1 = keys[:, 1] if nkeys > 1 else np.zeros(len(keys), np.uint32)
    assert np.array_equal(C.mix(C.tuple_of(keys[:, 0], k1)), m)
    assert np.array_equal(C.lds_home(m, 2), mh)
    assert np.array_equal(C.unmix(m), C.tuple_of(keys[:, 0], k1)), "unmix is not the inverse of the headers' mix"
    if nkeys >= 3:
        assert np.array_equal(C.wide_hash(keys), w) and np.array_equal(C.lds_home(w, nkeys), wh)
    h, home = header_hash(headers, keys)
    assert np.array_equal(C.hash_of(keys), h) and np.array_equal(C.lds_home(h, nkeys), home)


@pytest.mark.parametrize("nkeys", [1, 2, 3, 4])
def test_the_port_equals_the_headers(headers, nkeys):
    rng = np.random.default_rng(nkeys)
    check_port(headers, rng.integers(0, 1 << 32, (10_000, nkeys), dtype=np.uint64).astype(np.uint32))
    edge = np.array([0, 0xFFFFFFFF, 0x80000000], np.uint32)
    check_port(headers, np.stack([np.full(nkeys, e, np.uint32) for e in edge]))                                    # all zero, all ones, 0x80000000
    check_port(headers, np.stack(np.meshgrid(*[edge] * nkeys, indexing="ij"), axis=-1).reshape(-1, nkeys))          # and every mixture of them


def test_the_constants_equal_the_headers(headers):
    consts = headers(np.zeros((1, 4), np.uint32))[4]
    for name in ("MAX_KEYS", "LOG2_LDS_SLOTS", "LDS_SLOTS", "LDS_PROBES", "LDS_GROUPS", "MIN_MERGE_SLOTS"):
        assert consts[name] == (getattr(C.NARROW, name), getattr(C.WIDE, name)), name
    for name in ("LOG2_LDS_SLOTS", "LDS_SLOTS", "LDS_PROBES", "LDS_GROUPS", "MIN_MERGE_SLOTS"):
        assert consts[name] == (getattr(C, name),) * 2, name
    assert consts["BLOCK"] == (C.BLOCK_ROWS // 4,) * 2
    for name, capacity in (("MERGE_SLOTS_511", 511), ("MERGE_SLOTS_3000", 3000), ("MERGE_SLOTS_2_19", 1 << 19)):
        assert consts[name] == (C.merge_slots(capacity),) * 2, name
    assert C.merge_slots(511) == 1024 and C.merge_slots(1 << 19) == 1 << 20


def test_the_generators(headers):
    """solve and scan in every form give what they were asked for, raise when they cannot, and repeat themselves"""
    forms = [lambda: C.solve(300, 2, lds=2045, merge_bits=20, merge_home=C.WRAP20, seed=3),
             lambda: C.solve(300, 3, lds=7, seed=4),
             lambda: C.solve(300, 4, merge_bits=20, merge_home=5, seed=5),
             lambda: C.solve(300, 4, lds=2045, merge_bits=20, merge_home=C.WRAP20, seed=6, fixed_t01=(1, 2))]
    for f in forms:
        keys = f()
        assert np.array_equal(keys, f()) and len(np.unique(keys, axis=0)) == 300
    keys = forms[3]()
    assert (keys[:, 0] == 1).all() and (keys[:, 1] == 2).all()
    h, home = header_hash(headers, keys)
    assert (home == 2045).all() and ((h & np.uint64(0xFFFFF)) == C.WRAP20).all()
    for nkeys in (1, 2, 3, 4):
        for column in range(nkeys):
            keys = C.scan(300, nkeys, column, C.FIXED[:nkeys], lds=2045)
            h, home = header_hash(headers, keys)
            assert (home == 2045).all() and len(np.unique(keys[:, column])) == 300
            assert all((keys[:, c] == C.FIXED[c]).all() for c in range(nkeys) if c != column)
    keys = C.scan(300, 1, 0, (0,), merge_bits=10, merge_home=5)
    assert ((header_hash(headers, keys)[0] & np.uint64(1023)) == 5).all()
    with pytest.raises(ValueError):
        C.scan(10_000, 1, 0, (0,), lds=5)                          # about 2000 of the 2^22 values have a given LDS home
    with pytest.raises(AssertionError):
        C.scan(10, 1, 0, (0,), lds=5, merge_bits=10, merge_home=5)  # a scan pins one home
    ids = C.cover_ids(3 * 4096 + 5, np.arange(4096), seed=1)
    assert all(len(np.unique(ids[lo:lo + 4096])) == 4096 for lo in (0, 4096, 8192))


def lds_runs(homes, slots):
    """the occupied slots of a linear-probing table of `slots` slots that took tuples with these homes (whatever the order and however
    long the walks): [slots] bool"""
    occ = np.zeros(slots, bool)
    for s in homes:
        s = int(s)
        while occ[s]:
            s = (s + 1) % slots
        occ[s] = True
    return occ


def run_through(occ, slot):
    """the length of the circular run of occupied slots through `slot`"""
    n = len(occ)
    assert occ[slot] and not occ.all()
    lo = hi = slot
    while occ[(lo - 1) % n]:
        lo -= 1
    while occ[(hi + 1) % n]:
        hi += 1
    return hi - lo + 1


@pytest.mark.parametrize("name,nkeys", C.CASES)
def test_crafted_sets(headers, name, nkeys):
    s = C.SCENARIOS[name]
    lay = C.layout_of(nkeys)
    keys, crafted = C.scenario(name, nkeys)
    again = C.scenario.__wrapped__(name, nkeys)
    assert np.array_equal(again[0], keys) and again[1] == crafted == s["count"], "the same arguments, another set"
    S = len(keys)
    assert S == 1 + crafted + C.EXTRAS and len(np.unique(keys, axis=0)) == S and not keys[0].any() and keys[1:].any(axis=1).all()
    h, home = header_hash(headers, keys)
    ch, chome = h[1:1 + crafted], home[1:1 + crafted]
    lds, bits, merge_home = C.pinned(name, nkeys)
    # the homes it was asked for
    if lds is not None:
        assert (chome == lds).all()
    if bits:
        assert ((ch & np.uint64((1 << bits) - 1)) == merge_home).all()
    if "column" in s:                                               # tuples that differ in one column alone
        col = s["column"] % nkeys
        assert all((keys[1:1 + crafted, c] == C.FIXED[c]).all() for c in range(nkeys) if c != col) and len(np.unique(keys[1:1 + crafted, col])) == crafted
    if "fixed_t01" in s:                                            # tuples that share key words 0 and 1
        assert (keys[1:1 + crafted, 0] == s["fixed_t01"][0]).all() and (keys[1:1 + crafted, 1] == s["fixed_t01"][1]).all()
    # the rows: every whole workgroup has a selected row of every crafted tuple under either mask, the all-zero tuple a count of its own
    ids, sels = C.masked_rows(name, nkeys)
    n = s["n"]
    assert len(ids) == n <= 40_000 and n // C.BLOCK_ROWS in (1, 8) and set(sels) == {"null", "half"}
    assert sels["null"].all() and 0.4 * n < sels["half"].sum() < 0.6 * n
    for sel in sels.values():
        assert C.present(name, nkeys, ids, sel).all() and C.tuple0_stands_out(ids, sel)
    # the counting conditions
    overflow = s.get("overflow", False)
    if not overflow:
        assert S < lay.LDS_GROUPS, "a workgroup's table may fill up: rows would leave it for that reason"
    if lds is not None:
        occ = lds_runs(home[0 if nkeys > C.NARROW.MAX_KEYS else 1:], lay.LDS_SLOTS)         # (the all-zero tuple has a hashed slot in the wide layout only)
        if crafted <= lay.LDS_PROBES:                               # a, b: everything lives in LDS, after walks of up to `crafted` slots
            assert run_through(occ, lds) >= crafted
            widest = max(run_through(occ, int(x)) for x in np.flatnonzero(occ))
            assert widest + 1 <= lay.LDS_PROBES, "a row may leave the LDS table by the probe bound"
        else:                                                       # c, f, h: slots lds ... lds + LDS_PROBES - 1 are all a tuple of this home can take
            assert crafted - lay.LDS_PROBES >= 44
        if lds + crafted > lay.LDS_SLOTS:                           # b and the wrapped forms: the walk passes the table's last slot
            assert lds + min(crafted, lay.LDS_PROBES) > lay.LDS_SLOTS and occ[lay.LDS_SLOTS - 1] and occ[0]
    caps = C.capacities(name, nkeys)
    assert caps and (nkeys == 1 or caps == s["capacities"])
    if bits:
        for capacity in caps:
            slots = C.merge_slots(S if capacity is None else capacity)
            assert slots <= 1 << bits, "the merge table uses hash bits that the set does not pin"
            mh = ch & np.uint64(slots - 1)
            assert (mh == mh[0]).all()
            if s["home"] == C.WRAP20 or overflow:
                assert int(mh[0]) == slots - 3 and crafted > 3      # the chain passes the table's last slot
            else:
                assert int(mh[0]) == s["home"] and int(mh[0]) + crafted < slots
            if overflow:
                assert capacity < slots < crafted, "more tuples than the merge table has slots"
            else:
                assert S <= capacity if capacity is not None else True
