"""Key tuples crafted to collide in the grouped operators' tables (plain numpy, no GPU).

hjgpu_group_sum, hjgpu_group_agg and hjgpu_group_by keep their groups in open-addressed tables with linear probing whose load the code
fixes, so only the keys can make a walk long.  They can: hj_group::mix (csrc/group_layout.hpp) is splitmix64's finaliser, a bijection of
64 bits, and hj_wide::hash (csrc/wide_group_layout.hpp) is mix(mix(t01) + t23 * odd), so a tuple with a chosen hash is computed, not
searched for.  This module is a numpy port of those functions, the inverse of mix, two ways to make tuples with a given home in a
workgroup's LDS table (the hash's top LOG2_LDS_SLOTS bits) and / or in the merge table (its low bits) - solve() and scan() - and the
crafted sets of tests/test_gpu_group_collisions.py (scenario()).  tests/test_collision_keys.py pins the port and every crafted set to the
headers themselves, compiled with g++: a changed hash or table size fails there, on the CPU."""
import functools
from types import SimpleNamespace

import numpy as np

U64 = np.uint64
M64 = (1 << 64) - 1


def _layout(max_keys):
    lay = SimpleNamespace(MAX_KEYS=max_keys, LOG2_LDS_SLOTS=11, LDS_PROBES=256, MIN_MERGE_SLOTS=1024)
    lay.LDS_SLOTS = 1 << lay.LOG2_LDS_SLOTS
    lay.LDS_GROUPS = lay.LDS_SLOTS // 2
    return lay


NARROW = _layout(2)                     # hj_group: one and two key columns (hjgpu_group_sum, hjgpu_group_agg)
WIDE = _layout(4)                       # hj_wide: three and four key columns (hjgpu_group_by)
# both layouts agree (test_collision_keys checks each against its header)
LOG2_LDS_SLOTS, LDS_SLOTS, LDS_PROBES, LDS_GROUPS, MIN_MERGE_SLOTS = (NARROW.LOG2_LDS_SLOTS, NARROW.LDS_SLOTS, NARROW.LDS_PROBES,
                                                                     NARROW.LDS_GROUPS, NARROW.MIN_MERGE_SLOTS)
BLOCK_ROWS = 4096                       # the rows a workgroup of the grouped roads owns per trip: BLOCK = 1024 lanes, 4 rows each
SCAN = 1 << 22                          # the values scan() runs its one column over
SCAN_MERGE_BITS = 10                    # the most merge-home bits a scan pins: about 4000 hits

MIX1, MIX2, GOLDEN = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0x9E3779B97F4A7C15
INV1, INV2, INV_GOLDEN = pow(MIX1, -1, 1 << 64), pow(MIX2, -1, 1 << 64), pow(GOLDEN, -1, 1 << 64)


def layout_of(nkeys):
    return NARROW if nkeys <= NARROW.MAX_KEYS else WIDE


def _u64(x):
    return np.asarray(x).astype(U64)


def mix(x):
    """hj_group::mix"""
    x = _u64(x).copy()
    x ^= x >> U64(30); x *= U64(MIX1)
    x ^= x >> U64(27); x *= U64(MIX2)
    x ^= x >> U64(31)
    return x


def unmix(h):
    """the inverse of mix: mix(unmix(h)) == h == unmix(mix(h))"""
    x = _u64(h).copy()
    x ^= (x >> U64(31)) ^ (x >> U64(62)); x *= U64(INV2)
    x ^= (x >> U64(27)) ^ (x >> U64(54)); x *= U64(INV1)
    x ^= (x >> U64(30)) ^ (x >> U64(60))
    return x


def tuple_of(k0, k1):
    """hj_group::tuple_of"""
    return _u64(k0) | (_u64(k1) << U64(32))


def lds_home(h, nkeys=2):
    """hj_group::lds_home / hj_wide::lds_home"""
    return (_u64(h) >> U64(64 - layout_of(nkeys).LOG2_LDS_SLOTS)).astype(np.uint32)


def wide_hash(keys):
    """hj_wide::hash of the key words of tuples [S, 3 or 4] (a missing fourth key is the word 0)"""
    keys = np.asarray(keys)
    k3 = keys[:, 3] if keys.shape[1] > 3 else np.zeros(len(keys), np.uint32)
    return mix(mix(tuple_of(keys[:, 0], keys[:, 1])) + tuple_of(keys[:, 2], k3) * U64(GOLDEN))


def hash_of(keys):
    """the 64 bits both tables of a tuple's layout take its homes from; keys: [S, nkeys]"""
    keys = np.asarray(keys)
    nkeys = keys.shape[1]
    if nkeys <= NARROW.MAX_KEYS:
        return mix(tuple_of(keys[:, 0], keys[:, 1] if nkeys == 2 else np.zeros(len(keys), np.uint32)))
    return wide_hash(keys)


def merge_slots(capacity):
    """hj_group::merge_slots / hj_wide::merge_slots"""
    s = MIN_MERGE_SLOTS
    while s < 2 * capacity:
        s <<= 1
    return s


def _split(t):
    return (t & U64(0xFFFFFFFF)).astype(np.uint32), (t >> U64(32)).astype(np.uint32)


def chosen_hashes(count, nkeys, lds=None, merge_bits=0, merge_home=0, seed=0):
    """count distinct 64-bit words with the top LOG2_LDS_SLOTS bits `lds` (None: free) and the low merge_bits bits merge_home, the free
    bits from a seeded generator"""
    top = layout_of(nkeys).LOG2_LDS_SLOTS
    assert 0 <= merge_bits <= 64 - top and 0 <= merge_home < 1 << merge_bits
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 64, 2 * count + 16, dtype=U64)
    if lds is not None:
        assert 0 <= lds < 1 << top
        h = (h & U64(M64 >> top)) | U64(lds << (64 - top))
    h = (h & U64(M64 ^ ((1 << merge_bits) - 1))) | U64(merge_home)
    _, first = np.unique(h, return_index=True)
    h = h[np.sort(first)][:count]
    if len(h) < count:
        raise ValueError("too few free bits for %d distinct hashes" % count)
    return h


def _distinct(keys, count, what):
    keys = keys[(keys != 0).any(axis=1)]                # the all-zero tuple is every test's own, never a crafted one
    _, first = np.unique(keys, axis=0, return_index=True)
    keys = keys[np.sort(first)]
    if len(keys) < count:
        raise ValueError("%s: %d distinct tuples, %d wanted" % (what, len(keys), count))
    return np.ascontiguousarray(keys[:count])


def solve(count, nkeys, lds=None, merge_bits=0, merge_home=0, seed=0, fixed_t01=None):
    """count distinct tuples [count, nkeys] of 2 to 4 keys with the given homes, by inverting the hash.  Two keys: the tuple word is
    unmix(h).  Three: key 2 is drawn, t01 solved.  Four: t23 is drawn and t01 solved, or - fixed_t01 = (key 0, key 1) - t01 is fixed and
    t23 solved: tuples that share key words 0 and 1"""
    assert 2 <= nkeys <= 4 and (fixed_t01 is None or nkeys == 4)
    spare = 8                                           # (a drawn hash may be the all-zero tuple's)
    h = chosen_hashes(count + spare, nkeys, lds, merge_bits, merge_home, seed)
    rng = np.random.default_rng(seed + 77)
    if nkeys == 2:
        cols = _split(unmix(h))
    elif fixed_t01 is not None:
        t01 = tuple_of(np.array(fixed_t01[:1], np.uint32), np.array(fixed_t01[1:], np.uint32))
        t23 = (unmix(h) - mix(t01)) * U64(INV_GOLDEN)
        cols = (np.full(len(h), fixed_t01[0], np.uint32), np.full(len(h), fixed_t01[1], np.uint32)) + _split(t23)
    else:
        t23 = rng.integers(0, 1 << (32 if nkeys == 3 else 64), len(h), dtype=U64)
        cols = _split(unmix(unmix(h) - t23 * U64(GOLDEN))) + _split(t23)[:nkeys - 2]
    return _distinct(np.stack(cols, axis=1), count, "solve")


def scan(count, nkeys, column, fixed, lds=None, merge_bits=0, merge_home=0):
    """count distinct tuples [count, nkeys] of 1 to 4 keys that differ in `column` alone - the other columns hold fixed[c] - found by
    running that column over 0 .. SCAN - 1.  Pins the LDS home or a merge home of at most SCAN_MERGE_BITS bits, not both"""
    assert 1 <= nkeys <= 4 and 0 <= column < nkeys and len(fixed) == nkeys
    assert (lds is None) != (merge_bits == 0), "a scan pins one home"
    assert merge_bits <= SCAN_MERGE_BITS and 0 <= merge_home < 1 << max(merge_bits, 1)
    keys = np.empty((SCAN, nkeys), np.uint32)
    for c in range(nkeys):
        keys[:, c] = np.arange(SCAN, dtype=np.uint32) if c == column else np.uint32(fixed[c])
    h = hash_of(keys)
    hit = lds_home(h, nkeys) == lds if lds is not None else (h & U64((1 << merge_bits) - 1)) == U64(merge_home)
    return _distinct(keys[hit], count, "scan")


def cover_ids(n, owners, seed):
    """n ids of [0, S), S = max(owners) + 1, such that every run of BLOCK_ROWS rows - what one workgroup sees - holds every id: row i takes
    owners[i % len(owners)], and the rows of every block are permuted by a seeded permutation.  An id named more than once in owners
    has that many times the rows"""
    owners = np.asarray(owners)
    assert len(owners) <= BLOCK_ROWS and set(owners.tolist()) == set(range(int(owners.max()) + 1))
    ids = owners[np.arange(n) % len(owners)]
    rng = np.random.default_rng(seed)
    for lo in range(0, n, BLOCK_ROWS):
        ids[lo:lo + BLOCK_ROWS] = rng.permutation(ids[lo:lo + BLOCK_ROWS])
    return ids


# ---- the crafted sets of tests/test_gpu_group_collisions.py ----------------------------------------------------------------------------
ONE_TABLE = BLOCK_ROWS + 37             # two workgroups, the second one a tail: one workgroup's table suffices
EIGHT_TABLES = 8 * BLOCK_ROWS + 37      # eight whole workgroups and a tail
EXTRAS = 50                             # unrelated random tuples beside every crafted set
TUPLE0_ROWS = 4                         # the all-zero tuple has this many times the rows of any other
WRAP20 = 0xFFFFD                        # the low 20 bits of a hash whose merge home is slots - 3 in every table of up to 2^20 slots
MID = 1000                              # an LDS home in mid-table
FIXED = (0, 0xFFFFFFFF, 0x80000000, 1)  # the columns a wide scan holds fixed

# name: crafted tuples, LDS home (None: free), merge-home bits and value for two keys and more (one key: at most SCAN_MERGE_BITS of
# them, by scan), rows, the capacities beside J (None) that the test runs at, the key counts
SCENARIOS = {
    "a_lds_chain":        dict(count=200, lds=MID, bits=0, home=0, n=ONE_TABLE, capacities=(None,), nkeys=(1, 2, 3, 4)),
    "b_lds_wrap":         dict(count=200, lds=LDS_SLOTS - 3, bits=0, home=0, n=ONE_TABLE, capacities=(None,), nkeys=(1, 2, 3, 4)),
    "c_probe_bound":      dict(count=LDS_PROBES + 44, lds=MID, bits=0, home=0, n=EIGHT_TABLES, capacities=(None,), nkeys=(1, 2, 3, 4)),
    "c_probe_bound_wrap": dict(count=LDS_PROBES + 44, lds=LDS_SLOTS - 3, bits=0, home=0, n=EIGHT_TABLES, capacities=(None,), nkeys=(1, 2, 3, 4)),
    "d_merge_chain":      dict(count=300, lds=None, bits=20, home=5, n=EIGHT_TABLES, capacities=(None, 1 << 19), nkeys=(1, 2, 3, 4)),
    "e_merge_wrap":       dict(count=300, lds=None, bits=20, home=WRAP20, n=EIGHT_TABLES, capacities=(None, 3000), nkeys=(1, 2, 3, 4)),
    # (one key has 32 bits to choose and a scan pins one home: no one-key form)
    "f_both_tables":      dict(count=LDS_PROBES + 44, lds=MID, bits=20, home=WRAP20, n=EIGHT_TABLES, capacities=(None, 3000), nkeys=(2, 3, 4)),
    "g_overflow_chain":   dict(count=1100, lds=None, bits=10, home=WRAP20 & 1023, n=EIGHT_TABLES, capacities=(511,), nkeys=(1, 2, 3, 4), overflow=True),
    "h_wide_last_key":    dict(count=LDS_PROBES + 44, lds=MID, bits=0, home=0, n=ONE_TABLE, capacities=(None,), nkeys=(3, 4), column=-1),
    "h_wide_first_key":   dict(count=LDS_PROBES + 44, lds=LDS_SLOTS - 3, bits=0, home=0, n=ONE_TABLE, capacities=(None,), nkeys=(3, 4), column=0),
    "h_wide_shared_t01":  dict(count=LDS_PROBES + 44, lds=MID, bits=20, home=WRAP20, n=EIGHT_TABLES, capacities=(None, 3000), nkeys=(4,),
                               fixed_t01=(0x80000000, 0xFFFFFFFF)),
}
CASES = [(name, nkeys) for name, s in SCENARIOS.items() for nkeys in s["nkeys"]]


def pinned(name, nkeys):
    """(LDS home or None, merge-home bits, merge home) that scenario `name` pins with nkeys key columns"""
    s = SCENARIOS[name]
    bits = min(s["bits"], SCAN_MERGE_BITS) if nkeys == 1 else s["bits"]
    return s["lds"], bits, s["home"] & ((1 << bits) - 1)


def capacities(name, nkeys):
    """the capacities (None: the group count J) scenario `name` runs at: one key pins SCAN_MERGE_BITS bits of a merge home, which only the
    smallest table's home is"""
    s = SCENARIOS[name]
    return tuple(c for c in s["capacities"] if nkeys > 1 or merge_slots(c or 0) <= 1 << SCAN_MERGE_BITS)


@functools.lru_cache(maxsize=None)
def scenario(name, nkeys):
    """(tuples [S, nkeys] uint32, crafted): row 0 is the all-zero tuple, rows 1 ... crafted the crafted set, the rest EXTRAS random
    tuples.  The same arguments give the same set"""
    s = SCENARIOS[name]
    assert nkeys in s["nkeys"]
    lds, bits, home = pinned(name, nkeys)
    seed = 1000 * sorted(SCENARIOS).index(name) + nkeys
    if "column" in s:
        made = scan(s["count"], nkeys, s["column"] % nkeys, FIXED[:nkeys], lds=lds)
    elif nkeys == 1:
        made = scan(s["count"], 1, 0, (0,), lds=lds, merge_bits=bits, merge_home=home)
    else:
        made = solve(s["count"], nkeys, lds, bits, home, seed, fixed_t01=s.get("fixed_t01"))
    extras = np.random.default_rng(seed + 500).integers(1, 1 << 32, (EXTRAS, nkeys), dtype=np.uint64).astype(np.uint32)
    keys = np.concatenate([np.zeros((1, nkeys), np.uint32), made, extras])
    assert len(np.unique(keys, axis=0)) == len(keys), "an unrelated tuple equals a crafted one"
    keys.setflags(write=False)
    return keys, len(made)


def rows_of(name, nkeys, seed=0):
    """the ids [n] of scenario `name`'s rows (indices into scenario()'s tuples): every workgroup meets every tuple, the all-zero tuple
    TUPLE0_ROWS times as often as any other"""
    keys, _ = scenario(name, nkeys)
    owners = np.concatenate([np.arange(len(keys)), np.zeros(TUPLE0_ROWS - 1, np.int64)])
    return cover_ids(SCENARIOS[name]["n"], owners, seed)


def present(name, nkeys, ids, sel):
    """[whole workgroups, crafted] bool: the workgroup has a selected row of the crafted tuple"""
    keys, crafted = scenario(name, nkeys)
    blocks = len(ids) // BLOCK_ROWS
    return np.stack([np.bincount(ids[b * BLOCK_ROWS:(b + 1) * BLOCK_ROWS][sel[b * BLOCK_ROWS:(b + 1) * BLOCK_ROWS]], minlength=len(keys))[1:1 + crafted] > 0
                     for b in range(blocks)])


def tuple0_stands_out(ids, sel):
    counts = np.bincount(ids[sel])
    return counts[0] > 0 and not (counts[1:] == counts[0]).any()


@functools.lru_cache(maxsize=None)
def masked_rows(name, nkeys):
    """(ids, {"null": every row, "half": a random half}) of scenario `name`: under either mask every whole workgroup has a selected row of
    every crafted tuple, and the all-zero tuple has a row count of its own.  The half mask is rng.random(n) < 0.5 under the first seed that
    does so; where the rows per tuple and workgroup are too few for any seed to do (the overflow scenario: 1100 tuples in 4096 rows), the
    first row of each missing tuple is switched on"""
    ids = rows_of(name, nkeys)
    n = len(ids)
    sels = {"null": np.ones(n, bool)}
    for seed in range(64):
        sel = np.random.default_rng(seed).random(n) < 0.5
        if present(name, nkeys, ids, sel).all() and tuple0_stands_out(ids, sel):
            break
    else:
        assert SCENARIOS[name].get("overflow"), (name, nkeys, "no seed keeps every crafted tuple in every workgroup")
        sel = np.random.default_rng(0).random(n) < 0.5
        for b, row in enumerate(present(name, nkeys, ids, sel)):
            block = ids[b * BLOCK_ROWS:(b + 1) * BLOCK_ROWS]
            for t in np.flatnonzero(~row) + 1:
                sel[b * BLOCK_ROWS + np.flatnonzero(block == t)[0]] = True
    sels["half"] = sel
    for sel in sels.values():
        assert present(name, nkeys, ids, sel).all() and tuple0_stands_out(ids, sel), (name, nkeys)
        sel.setflags(write=False)
    ids.setflags(write=False)
    return ids, sels
