"""Cases for sd_object_index_merge_objects (include/sd_cas.h; csrc/object_index.h, merge Objects:
"Object `from` IS Object `to`"), shared by tests/test_object_index_merge.py (sd_cpu_object_index_*)
and tests/test_gpu_object_index_merge.py (the kernels and the device entry).  They build on
tests/object_index_duplicates_cases.py: the same pools and the dict statement of every earlier
call.  Every list asserts the property it exists for, so a wrong edit cannot quietly shrink a sweep.

An index under test offers what the duplicates cases ask for, and
    merge_objects(from_ids, to_ids) -> (moved, coalesced)       SdCasError on a contradiction
A script is a list of the earlier cases' operations, ("merge_objects", from, to),
("contradiction", from, to) and ("read",), applied in order to one index that starts empty.

Nothing here touches a device or the library.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import object_index_cases as oc
from tests import object_index_duplicates_cases as dc
from tests import object_index_owners_cases as wc

U = np.uint64
M64 = oc.M64
E = dc.E
TILE = 256  # csrc/sliced.h: a slice is one tile up to 262 144 entries and two tiles beyond


class Contradiction(Exception):
    """one `from` with two different `to`"""


def phi_of(frm, to):
    phi = {}
    for f, t in zip(np.asarray(frm, U).tolist(), np.asarray(to, U).tolist()):
        if phi.setdefault(f, t) != t:
            raise Contradiction(f)
    return phi


class DictMerge(dc.DictDuplicates):
    """dc.DictDuplicates with the merge rule of object_index.h word for word: phi applied once
    and simultaneously to the relation {(key, id): links}; links of pairs that meet add up in u64."""

    def merge_objects(self, frm, to):
        phi = phi_of(frm, to)  # refused before anything changes
        moved = sum(1 for (_, v) in self.d if phi.get(v, v) != v)
        if moved == 0:
            return 0, 0
        after = {}
        for (k, v), c in self.d.items():
            p = (k, phi.get(v, v))
            after[p] = (after.get(p, 0) + c) & M64
        before = len(self.d)
        self.d, self._g = after, None
        return moved, before - len(after)


def arr(*xs):
    return np.array(xs, dtype=U)


def relation_rows(d):
    """the rows an insert takes to build the relation of d afresh: each pair once per link"""
    k, v, c = d.export_links()
    assert int(c.max(initial=0)) < 1 << 20
    return np.repeat(k, c.astype(np.int64)), np.repeat(v, c.astype(np.int64))


def compare(x, d, make_twin=None, probes=None, what=""):
    """x equals the dict statement: the count, export_links, links() and lookup of every entry
    (and of the probes); with make_twin, the arrays are those of a fresh index of x's kind built
    from the statement's relation, and the twin finds every key (its directory was built for the
    same count)."""
    want, got = d.export_links(), x.export_links()
    assert len(x) == len(d) == len(got[0]), what
    for a, b in zip(want, got):
        assert a.shape == b.shape and np.array_equal(a, b), what
    q = want[0] if probes is None else np.concatenate([want[0], probes[0]])
    qi = want[1] if probes is None else np.concatenate([want[1], probes[1]])
    la, lb = d.lookup(q), x.lookup(q)
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]), (what, "lookup")
    assert np.array_equal(d.links(q, qi), x.links(q, qi)), (what, "links")
    if make_twin is not None:
        t = make_twin()
        t.insert(*relation_rows(d))
        for a, b in zip(t.export_links(), got):
            assert a.shape == b.shape and np.array_equal(a, b), (what, "fresh twin")
        if hasattr(t, "close"):
            t.close()


def check_merge(x, d, frm, to, make_twin=None, probes=None, what=""):
    want = d.merge_objects(frm, to)
    got = x.merge_objects(frm, to)
    assert got == want, (what, got, want)
    compare(x, d, make_twin, probes, what)
    return got


# ------------------------------------------------------------------ seeded scripts
MERGE_SEEDS = (31, 32, 33, 34)
MERGE_OPS = 40
MERGE_KINDS = ("coalesced", "moved_only", "no_op", "swap", "cycle3", "chain", "absent_from", "self_map", "repeats",
               "to_is_new", "first_owner_changed", "contradiction")


def seeded_script(seed: int):
    """A script of MERGE_OPS operations over wc.pools(seed), generated against the dict statement:
    merge_objects mixed with insert, the three removals, apply and the reads by Object and by key.
    Over the script the maps coalesce entries, only move them, move nothing, swap two ids, turn
    three, chain (a -> b, b -> c), name ids nobody holds, map an id to itself, repeat pairs, send
    ids to one nobody holds and change a key's first owner; and one map contradicts itself."""
    rng = np.random.default_rng(seed)
    keys, ids = wc.pools(seed)
    d = DictMerge()
    script, seen = [], Counter()

    def draw(m):
        return keys[rng.integers(0, len(keys), m)], ids[rng.integers(0, len(ids), m)]

    for step in range(MERGE_OPS):
        kind = "insert" if step < 2 else "contradiction" if step == MERGE_OPS // 2 else ("merge", "insert", "remove", "remove_keys", "remove_objects", "apply", "read",
                                          "contradiction")[int(rng.choice(8, p=[0.45, 0.2, 0.05, 0.03, 0.05, 0.07, 0.1, 0.05]))]
        if kind == "insert":
            op = ("insert",) + draw(int(rng.choice([5, 60, 300])))
        elif kind == "remove":
            op = ("remove",) + draw(20)
        elif kind == "remove_keys":
            op = ("remove", keys[rng.integers(0, len(keys), 2)], None)
        elif kind == "remove_objects":
            op = ("remove_objects", ids[rng.integers(0, len(ids), 1)])
        elif kind == "apply":
            op = ("apply",) + draw(10) + draw(30)
        elif kind == "read":
            op = ("read",)
        elif kind == "contradiction":
            a, b, c = (int(x) for x in ids[rng.permutation(len(ids))[:3]])
            op = ("contradiction", arr(a, int(ids[0]), a), arr(b, int(ids[1]), c if rng.integers(0, 2) else a))
            seen["contradiction"] += 1
        else:
            held = sorted({p[1] for p in d.d})
            pick = [int(x) for x in ids[rng.permutation(len(ids))]]
            shape = seen["merges"] % 6  # every shape in turn
            seen["merges"] += 1
            if shape == 0 and len(held) >= 2:    # several ids to one that is held
                f = held[1:1 + int(rng.integers(1, 4))]
                t = [held[0]] * len(f)
            elif shape == 1:
                f, t = [pick[0], pick[1]], [pick[1], pick[0]]
                seen["swap"] += 1
            elif shape == 2:
                f, t = [pick[0], pick[1], pick[2]], [pick[1], pick[2], pick[0]]
                seen["cycle3"] += 1
            elif shape == 3:
                f, t = [pick[0], pick[1]], [pick[1], pick[2]]
                seen["chain"] += 1
            elif shape == 4:                     # to an id nobody holds, an absent from, a self map, repeats
                new = int(oc.splitmix(seed * 100 + step, 1)[0])
                f, t = [pick[0], pick[1], new ^ 1, pick[2], pick[0]], [new, new, pick[3], pick[2], new]
                seen["to_is_new"] += 1
                seen["absent_from"] += 1
                seen["self_map"] += 1
                seen["repeats"] += 1
            else:                                # only ids nobody holds, or nothing at all
                f = [int(x) ^ 2 for x in oc.splitmix(seed * 100 + step, int(rng.integers(0, 3)))]
                t = [pick[0]] * len(f)
            o = rng.permutation(len(f))
            op = ("merge_objects", arr(*f)[o], arr(*t)[o])
            first = d.first_owners()
            moved, coalesced = DictMerge.merge_objects(d, op[1], op[2])
            seen["coalesced" if coalesced else "moved_only" if moved else "no_op"] += 1
            seen["first_owner_changed"] += int(first != d.first_owners())
            script.append(op)
            continue
        script.append(op)
        if op[0] not in ("read", "contradiction"):
            getattr(d, op[0])(*op[1:])
    assert all(seen[w] > 0 for w in MERGE_KINDS), (seed, seen)
    return script


def script_probes(seed: int):
    """(keys, ids) asked of links() and lookup() after every operation: the whole pool crossed"""
    keys, ids = wc.pools(seed)
    return np.repeat(keys, len(ids)), np.tile(ids, len(keys))


def run_merge_script(name, script, make_a, make_b, probes=None, make_twin=None):
    """Apply the script to a (the statement) and b.  After every operation the return values are
    equal and compare() holds; a contradiction is refused by both with b's export bit-unchanged; a
    read compares duplicate_entries(0, 2), duplicate_stats and the orphans among the pool's ids."""
    a, b = make_a(), make_b()
    for step, op in enumerate(script):
        what = (name, step, op[0])
        if op[0] == "read":
            for p, q in zip(a.duplicate_entries(0, 2), b.duplicate_entries(0, 2)):
                assert np.array_equal(p, q), what
            assert np.array_equal(a.duplicate_stats(), b.duplicate_stats()), what
            ids = probes[1] if probes is not None else arr(0, M64)
            assert np.array_equal(a.orphans(ids), b.orphans(ids)), what
            continue
        if op[0] == "contradiction":
            before = [x.copy() for x in b.export_links()]
            for x in (a, b):
                try:
                    x.merge_objects(op[1], op[2])
                except Contradiction:
                    pass
                except Exception as e:  # the library's refusal
                    assert getattr(e, "rc", None) == -1, what
                else:
                    raise AssertionError(what)
            assert all(np.array_equal(p, q) for p, q in zip(before, b.export_links())), what
            continue
        ra, rb = getattr(a, op[0])(*op[1:]), getattr(b, op[0])(*op[1:])
        if isinstance(ra, tuple):
            assert len(ra) == len(rb) and all(
                np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for p, q in zip(ra, rb)), what
        else:
            assert ra == rb, what
        compare(b, a, make_twin, probes, what)
    return a, b


# ------------------------------------------------------------------ shapes
ENTRY_COUNTS = (0, 1, 255, 256, 257, 1000, 262_144)  # 262 401: slice_straddle_case
MAP_SIZES = (1, 255, 256, 257, 5000)


def counted_case(n: int):
    """(keys, ids, from, to): n entries, two owners per key (the last key one when n is odd), and a
    map under which, by the key's position modulo 5, the second owner meets the first (101 -> 1),
    goes to an id nobody holds (102 -> 9999), changes with a later one (103 <-> 104), both owners
    go (4 -> 1 while 104 -> 103) and nothing happens (105 -> 105); 77 owns nothing."""
    nk = (n + 1) // 2
    ks = oc.random_keys(nk, 7000 + n) if nk else E
    j = np.arange(nk, dtype=U)
    k = np.concatenate([ks, ks[: n - nk]])
    v = np.concatenate([j % U(5) + U(1), (j % U(5) + U(101))[: n - nk]])
    assert len(k) == n
    o = np.argsort(oc.splitmix(n + 3, n)) if n else np.zeros(0, np.int64)
    return k[o], v[o], arr(101, 102, 103, 104, 105, 4, 77), arr(1, 9999, 104, 103, 105, 1, 1)


def pool_case():
    """(keys, ids, the 300 ids of the pool): 1000 entries, 200 keys with five owners each"""
    pool = oc.splitmix(4242, 300)
    ks = oc.random_keys(200, 4243)
    pick = np.stack([np.argsort(oc.splitmix(5000 + j, 300))[:5] for j in range(200)])
    return np.repeat(ks, 5), pool[pick.reshape(-1)], pool


def sized_map(pool, size: int):
    """`size` rows: distinct `from` ids, the first 100 (at most) of the pool and the rest ids nobody
    holds, each sent to an id of the pool's other 200; 5000 rows are 2500 pairs named twice."""
    distinct = size if size < 5000 else size // 2
    have = min(distinct, 100)
    f = np.concatenate([pool[:have], oc.splitmix(777 + size, distinct - have) | U(1 << 63)])
    assert len(np.unique(f)) == distinct and not np.isin(f[have:], pool).any()
    t = pool[100 + (np.arange(distinct) * 7) % 200]
    if size >= 5000:
        f, t = np.concatenate([f, f]), np.concatenate([t, t])
    o = np.argsort(oc.splitmix(size, len(f)))
    assert len(f) == size
    return f[o], t[o]


def straddle_at(n: int, pos: int, run: int, seed: int):
    """n entries in which one key's run of `run` owners (ids 100 .. 100 + run - 1) lies across
    position `pos`, every other entry being the only owner (id 10) of its key.  Returns (keys, ids,
    the key)."""
    ks = np.sort(oc.random_keys(n - run + 1, seed))
    p0 = pos - run // 2
    key = ks[p0]
    keys = np.concatenate([ks, np.full(run - 1, key, U)])
    ids = np.concatenate([np.full(len(ks), 10, U), U(101) + np.arange(run - 1, dtype=U)])
    ids[p0] = 100
    o = np.lexsort((ids, keys))
    assert keys[o][pos - 1] == keys[o][pos] == key and ids[o][pos - 1] != 10 and ids[o][pos] != 10
    assert len(keys) == n
    return keys, ids, key


def tile_straddle_case():
    """600 entries, a run of 6 owners across positions 255 | 256 (two tiles)"""
    return straddle_at(600, TILE, 6, 321)


def slice_straddle_case():
    """262 401 entries: a slice of the sliced passes is two tiles, so positions 511 | 512 are the
    last of one slice and the first of the next; a run of 6 owners lies across them."""
    n = 262_401
    per = -(-(-(-n // 1024)) // TILE) * TILE
    assert per == 2 * TILE
    return straddle_at(n, per, 6, 322)


def run_maps(first: int = 100, run: int = 6):
    """name -> (from, to) for a run of ids first .. first + run - 1: every owner of the run to ONE
    id, so leaving entries on both sides of the border coalesce"""
    own = U(first) + np.arange(run, dtype=U)
    return {"to_lowest_in_run": (own[1:], np.full(run - 1, own[0], U)),
            "to_highest_in_run": (own[:-1], np.full(run - 1, own[-1], U)),
            "to_absent_below": (own, np.full(run, 3, U)),
            "to_absent_above": (own, np.full(run, M64, U))}


LONG = 600  # owners of one key: the run spans three tiles


def long_run_case():
    """(keys, ids, key, owners): LONG owners of one key among 900 other entries"""
    other = oc.random_keys(900, 654)
    key = other[7] ^ U(1 << 20)
    owners = np.sort(oc.splitmix(655, LONG) | U(4))  # none is 0, 1, 2 or 3
    assert key not in other.tolist() and len(np.unique(owners)) == LONG and LONG > 2 * TILE
    keys = np.concatenate([other, np.full(LONG, key, U)])
    ids = np.concatenate([np.full(900, 1, U), owners])
    sh = np.argsort(oc.splitmix(657, len(keys)))
    return keys[sh], ids[sh], key, owners


def long_run_maps(owners):
    """name -> (from, to, coalesced): all LONG owners end at one id"""
    mid = owners[LONG // 2]
    rest = owners[owners != mid]
    return {"to_in_run": (rest, np.full(LONG - 1, mid, U), LONG - 1),
            "to_absent": (owners, np.full(LONG, 2, U), LONG - 1),
            # the target is itself sent on: the owners meet at `mid`, mid's own entry goes to 3
            "to_is_a_from": (np.concatenate([rest, arr(mid)]), np.concatenate([np.full(LONG - 1, mid, U), arr(3)]),
                             LONG - 2)}


def dir_bits_case():
    """(keys, ids, from, to): 34 entries, 17 keys with owners 1 and 2; 2 -> 1 leaves 17: the
    count crosses 32, where oi_dir_bits (object_index_host.cpp: (16 << b) <= n) steps from 2 to 1"""
    ks = oc.random_keys(17, 91)
    assert [oc.dir_bits(n) for n in (34, 32, 31, 17)] == [2, 2, 1, 1]
    return np.concatenate([ks, ks]), np.concatenate([np.full(17, 1, U), np.full(17, 2, U)]), arr(2), arr(1)


def extremes_case():
    """keys 0 and 2^64 - 1 owned by ids 0, 5 and 2^64 - 1"""
    k = arr(0, 0, 0, M64, M64, M64, 7)
    v = arr(0, 5, M64, 0, 5, M64, 5)
    maps = {"max_to_zero": (arr(M64), arr(0)), "zero_to_max": (arr(0), arr(M64)),
            "swap_extremes": (arr(0, M64), arr(M64, 0)), "five_to_max_and_zero_to_five": (arr(5, 0), arr(M64, 5))}
    return k, v, maps


def permutation_maps():
    """on keys owned by a subset of ids 1, 2, 3: name -> (from, to)"""
    return {"swap": (arr(1, 2), arr(2, 1)), "cycle3": (arr(1, 2, 3), arr(2, 3, 1)), "chain": (arr(1, 2), arr(2, 3))}


def permutation_pairs():
    """seven keys owned by every non-empty subset of {1, 2, 3}, with 1, 2 and 3 links"""
    ks = np.sort(oc.random_keys(7, 17))
    k, v = [], []
    for j, key in enumerate(ks.tolist()):
        for b, o in enumerate((1, 2, 3)):
            if (j + 1) >> b & 1:
                k += [key] * o
                v += [o] * o
    return arr(*k), arr(*v)


def shard_case():
    """(keys, ids, from, to) handed to every part: keys of every shard with two or three owners"""
    k, v, f, t = counted_case(1000)
    return np.concatenate([k, k[::3]]), np.concatenate([v, np.full(len(k[::3]), 1, U)]), f, t


def split_relation():
    """(keys, ids): 40 keys; every fourth has one owner, the others two to four, overlapping so
    that the components chain (key j is owned by Objects j, j + 1, ...)"""
    ks = oc.random_keys(40, 55)
    k, v = [], []
    for j, key in enumerate(ks.tolist()):
        owners = 1 if j % 4 == 0 else 2 + j % 3
        for o in range(owners):
            k += [key] * (1 + (j + o) % 2)
            v += [1000 + 10 * (j // 8) + j % 8 + o] * (1 + (j + o) % 2)
    return arr(*k), arr(*v)
