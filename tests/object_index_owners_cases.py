"""Cases for the Object index's owners mode (include/sd_cas.h: SD_OBJECT_INDEX_OWNERS), shared
by tests/test_object_index_owners.py (the numpy mirrors and sd_cpu_*) and
tests/test_gpu_object_index_owners.py (the kernels and the device entries).  They build on
tests/object_index_cases.py and tests/object_index_remove_cases.py: the same key sets, the same
histories.  Every list asserts the property it exists for, so a wrong edit cannot quietly shrink
a sweep.

An index under test offers, over uint64 arrays,
    insert(keys, ids) -> entries created
    remove(keys, ids or None) / remove_objects(ids) -> (dropped pairs [r, 2], r)
    links(keys, ids) -> link counts;  lookup(keys) -> (first owners, found)
    export_links() -> (keys, ids, links);  len()
    scan(records int64 [m, 2], chunk) -> (grouped records, owner, existing, new heads)
A script is a list of ("insert", keys, ids) / ("remove", keys, ids or None) /
("remove_objects", ids) operations applied in order to one index that starts empty.

Nothing here touches a device or the library.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import object_index_cases as oc
from tests import object_index_remove_cases as rc

U = np.uint64
M64 = oc.M64
ENTRY_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4097)
LARGE = 262_144 + 300  # > 1024 workgroups x 256 entries: a workgroup's slice is two tiles
RUN = 3000             # owners of one key: a bucket far over 16 entries that spans many tiles
COPIES = 70_000        # copies of one pair in one call


class DictOwners:
    """The owners mode of include/sd_cas.h word for word over a dict (key, id) -> links."""

    def __init__(self, nparts=1, part=0):
        self.nparts, self.part = nparts, part
        self.d = {}

    def __len__(self):
        return len(self.d)

    def _mine(self, k):
        return (((k >> 48) * self.nparts) >> 16) == self.part

    def insert(self, keys, ids):
        """each pair of this shard adds one link to (k, v); created at 1 if absent"""
        taken = 0
        for p in zip(keys.tolist(), ids.tolist()):
            if not self._mine(p[0]):
                continue
            taken += p not in self.d
            self.d[p] = self.d.get(p, 0) + 1
        return taken

    def _drop(self, gone):
        pairs = sorted(gone)  # ascending (key, id): python ints compare as the u64 they are
        for p in pairs:
            del self.d[p]
        return np.array(pairs, dtype=U).reshape(-1, 2), len(pairs)

    def remove(self, keys, ids=None):
        if ids is None:  # every entry of each listed key goes
            want = set(keys.tolist())
            return self._drop({p for p in self.d if p[0] in want})
        gone = set()
        for p, asked in Counter(zip(keys.tolist(), ids.tolist())).items():  # pairs naming one entry add up
            if p in self.d:
                if asked >= self.d[p]:  # asking for more is not an error
                    gone.add(p)
                else:
                    self.d[p] -= asked
        return self._drop(gone)

    def remove_objects(self, ids):
        want = set(ids.tolist())
        return self._drop({p for p in self.d if p[1] in want})  # whatever its links

    def links(self, keys, ids):
        return np.array([self.d.get(p, 0) for p in zip(keys.tolist(), ids.tolist())], dtype=U)

    def first_owners(self):
        """key -> its smallest Object id: the first owner"""
        t = {}
        for k, v in sorted(self.d):
            t.setdefault(k, v)
        return t

    def lookup(self, q):
        t = self.first_owners()
        ql = q.tolist()
        return np.array([t.get(k, 0) for k in ql], dtype=U), np.array([k in t for k in ql], dtype=np.uint8)

    def export_links(self):
        ps = sorted(self.d)
        return (np.array([p[0] for p in ps], dtype=U), np.array([p[1] for p in ps], dtype=U),
                np.array([self.d[p] for p in ps], dtype=U))


# ------------------------------------------------------------------ seeded scripts
SCRIPT_SEEDS = (11, 12, 13, 14)
SCRIPT_OPS = 36


def pools(seed: int):
    """(keys, ids) a script draws from: the u64 edges, a shared prefix, uniform keys; ids with 0
    and 2^64 - 1.  Few of each, so pairs repeat and one key has several owners."""
    keys = np.concatenate([oc.edge_keys(), oc.shared_prefix_keys(8, seed), oc.random_keys(17, 500 + seed)])
    ids = np.concatenate([np.array([0, M64], dtype=U), oc.splitmix(600 + seed, 8)])
    assert len(np.unique(keys)) == 32 and len(np.unique(ids)) == 10
    return keys, ids


def seeded_script(seed: int):
    """A script of SCRIPT_OPS operations generated against the dict statement, so that removals
    with ids ask for fewer links than held, exactly as many and more, name absent pairs and
    present keys with another id, and repeat pairs."""
    rng = np.random.default_rng(seed)
    keys, ids = pools(seed)
    d = DictOwners()
    script = []
    seen = Counter()

    def draw(m):
        return keys[rng.integers(0, len(keys), m)], ids[rng.integers(0, len(ids), m)]

    for step in range(SCRIPT_OPS):
        kind = "insert" if step < 3 else ("insert", "remove", "remove_keys", "remove_objects")[
            int(rng.choice(4, p=[0.4, 0.35, 0.1, 0.15]))]
        if kind == "insert":
            k, v = draw(int(rng.choice([1, 5, 60, 300])))
            op = ("insert", k, v)
        elif kind == "remove":
            held = list(d.d.items())
            rows = []
            for j in rng.permutation(len(held))[:6]:
                (k, v), c = held[j]
                ask = (max(c - 1, 1), c, c + 2)[int(rng.integers(0, 3))]
                seen["less" if ask < c else "equal" if ask == c else "more"] += 1
                rows += [(k, v)] * ask
                rows.append((k, v ^ 1))  # a present key with another id
            ak, av = draw(4)
            rows += list(zip(ak.tolist(), av.tolist()))
            rows = [rows[j] for j in rng.permutation(len(rows))]
            op = ("remove", np.array([r[0] for r in rows], dtype=U), np.array([r[1] for r in rows], dtype=U))
        elif kind == "remove_keys":
            op = ("remove", keys[rng.integers(0, len(keys), 3)], None)
            seen["keys"] += 1
        else:
            op = ("remove_objects", np.concatenate([ids[rng.integers(0, len(ids), 2)], oc.splitmix(seed + step, 1)]))
            seen["objects"] += 1
        script.append(op)
        getattr(d, op[0])(*op[1:])
    assert all(seen[w] > 0 for w in ("less", "equal", "more", "keys", "objects")), (seed, seen)
    return script


def scan_records(seed: int):
    """int64 records (key, file index) for the owner rule: keys of the pool, each several times,
    and keys no index has."""
    keys, _ = pools(seed)
    k = np.concatenate([keys, keys[::2], keys[::3], oc.random_keys(20, 900 + seed)])
    k = k[np.argsort(oc.splitmix(seed + 5, len(k)))]
    return np.stack([k, np.arange(len(k), dtype=U)], axis=1).view(np.int64)


# ------------------------------------------------------------------ shapes
def shaped_pairs(n: int):
    """n distinct (key, id) pairs, unsorted, with what an entry count is tested for: the u64
    edge keys and a shared prefix, ids 0 and 2^64 - 1, equal ids under different keys, runs of
    equal keys at both ends of the index, and neighbouring keys with the same id sets."""
    if n == 0:
        return np.zeros(0, U), np.zeros(0, U)
    if n < 15:
        return oc.edge_keys()[:n].copy(), np.array([0, M64, 7, 7, 7, 0, M64], dtype=U)[:n]
    e = oc.edge_keys()
    k = [0, 0, 0, 1, 1, 1, M64, M64, M64 - 1, M64 - 1]  # runs at both ends; neighbours, same id sets
    v = [0, 5, M64, 0, 5, M64, 0, M64, 0, M64]
    k += [int(x) for x in e[2:5]]
    v += [7, 7, 7]                                       # equal ids under different keys
    rest = n - len(k)
    sp = oc.shared_prefix_keys(max(rest // 4, 1))
    uni = oc.random_keys(rest, 4000 + n)
    uni = uni[~np.isin(uni, e)]
    body_k = np.concatenate([sp, sp[: len(sp) // 2], uni])[:rest]   # half of the prefix keys own twice
    body_v = np.concatenate([np.full(len(sp), 3, U), np.full(len(sp) // 2, 9, U), oc.vals_for(uni, 41) | U(16)])[:rest]
    keys = np.concatenate([np.array(k, dtype=U), body_k])
    vals = np.concatenate([np.array(v, dtype=U), body_v])
    assert len(keys) == n == len(set(zip(keys.tolist(), vals.tolist()))), n
    order = np.argsort(oc.splitmix(n + 1, n))
    return keys[order], vals[order]


def shape_script(n: int):
    """The index of n entries built in one shuffled insert with every third pair named twice and
    every fifth three times; removals with ids asking one link of every pair (asked < held,
    = held), then three of a quarter (> held, = held); a removal without ids; a removal by
    Object; the refill; everything removed, and an insert into the emptied index."""
    k, v = shaped_pairs(n)
    j = np.arange(n)
    rep = 1 + (j % 3 == 0) + (j % 5 == 0)
    ik, iv = np.repeat(k, rep), np.repeat(v, rep)
    sh = np.argsort(oc.splitmix(n + 2, len(ik)))
    q = slice(0, None, 4)
    script = [("insert", ik[sh], iv[sh]), ("expect_count", n),
              ("remove", k, v),
              ("remove", np.repeat(k[q], 3), np.repeat(v[q], 3)),
              ("remove", k[1::7].copy(), None),
              ("remove_objects", np.array([7, M64, 3, 12345], dtype=U)),
              ("insert", ik, iv), ("expect_count", n),
              ("remove", np.concatenate([ik, ik]), np.concatenate([iv, iv])), ("expect_count", 0),
              ("insert", k[::-1].copy(), v[::-1].copy()), ("expect_count", n)]
    return script


def straddle_case():
    """An index of 600 entries in which positions 255 and 256 -- the last of one tile, the first
    of the next -- are the two owners of one key.  Returns (keys, ids, the key)."""
    ks = np.sort(oc.random_keys(599, 321))
    keys = np.concatenate([ks, ks[255:256]])
    ids = np.concatenate([np.full(599, 10, U), np.array([4], dtype=U)])
    o = np.lexsort((ids, keys))
    assert keys[o][255] == keys[o][256] == ks[255] and ids[o][255] == 4 and ids[o][256] == 10
    return keys, ids, ks[255]


def long_run_case():
    """RUN owners of one key among 2000 other entries: (keys, ids, the key, its owners)."""
    other = oc.random_keys(2000, 654)
    key = other[7] ^ U(1 << 20)
    owners = oc.splitmix(655, RUN)
    assert key not in other.tolist() and len(np.unique(owners)) == RUN
    assert oc.dir_bits(2000 + RUN) >= 1 and RUN > 16 * 8 and RUN > 4 * 256
    keys = np.concatenate([other, np.full(RUN, key, U)])
    ids = np.concatenate([oc.vals_for(other, 656), owners])
    sh = np.argsort(oc.splitmix(657, len(keys)))
    return keys[sh], ids[sh], key, owners


def growth_steps():
    """Three inserts that grow the buffers twice (capacity 16 -> 40 -> 240, directory bits 0, 2,
    4), every pair named twice in the last."""
    (g1, v1), (g2, v2), (g3, v3) = oc.insert_cases()["three_growth"]
    assert [len(g1), len(g1) + len(g2), len(g2) + len(g3)] == [10, 40, 240]
    return [(g1, v1), (g2, v2), (np.concatenate([g3, g3]), np.concatenate([v3, v3]))]


def shard_case():
    """(keys, ids, removal keys, removal ids, Object ids) handed to every part of nparts 1, 2,
    3, 8: pairs of every shard with repeats, removals that take one of two links, the last
    link and absent pairs."""
    keys, vals, rk, rids = rc.shard_case()
    k = np.concatenate([keys, keys[::2], keys[:50]])
    v = np.concatenate([vals, vals[::2], vals[:50] ^ U(1)])
    o = np.argsort(keys)
    at = np.minimum(np.searchsorted(keys[o], rk), len(keys) - 1)
    hit = keys[o][at] == rk
    rv = np.where(hit, vals[o][at], U(1))  # the right id for the present keys
    assert hit.any() and not hit.all() and len(np.unique(rk[hit])) < int(hit.sum())  # repeats: both links go
    return k, v, rk, rv, rids


# ------------------------------------------------------------------ histories
class OwnersHistory(rc.History):
    """rc.History under the owners-mode cycle of INTEGRATION.md §6:

      scan                                 the owners as before; then ONE insert of (key, Object
                                           id) for every record, linked and created alike
      a file_path (c, O) deleted           remove of the pair (c, O) with the id given
      a file_path changed A -> B on O      remove (A, O), insert (B, O)
      the orphan remover                   remove_objects(ids)

    The DB is never asked who else owns a cas_id: owners_of raises.  After every event the
    entries equal the DB's (cas_id, Object) -> file_path count relation and the first owner of
    every key equals truth()."""

    def __init__(self, seed: int):
        super().__init__(seed)
        self.count["kept_other_links"] = 0

    def owners_of(self, cas_list):
        raise AssertionError("the owners-mode cycle never asks the DB for owners")

    def relation(self):
        return dict(Counter((int(self.cas_of[f], 16), o) for f, o in enumerate(self.obj_of)
                            if o >= 0 and self.cas_of[f] is not None))

    def check(self, index, what):
        k, v, c = index.export_links()
        got = dict(zip(zip(k.tolist(), v.tolist()), c.tolist()))
        assert len(got) == len(k) == len(index) and got == self.relation(), what
        assert all(a < b for a, b in zip(zip(k.tolist(), v.tolist()), zip(k[1:].tolist(), v[1:].tolist()))), what
        t = self.truth()
        ks = np.array(sorted(t), dtype=U)
        assert set(k.tolist()) == set(t), what
        ids, found = index.lookup(ks)
        assert found.all() and ids.tolist() == [t[x] for x in sorted(t)], what

    def scan(self, index):
        n = int(self.rng.integers(1, 251))
        base = len(self.cas_of)
        cas = [None if self.rng.random() < 0.08 else self.pool[int(self.rng.integers(0, rc.POOL))] for _ in range(n)]
        if n > 3:
            cas[1] = cas[0] = cas[0] or self.pool[0]
        self.cas_of += cas
        self.obj_of += [-1] * n
        before = len(self.objects)
        out = {}
        for s in range(0, n, rc.CHUNK):
            step = range(base + s, min(base + n, base + s + rc.CHUNK))
            rc._assign_step(step, self.cas_of, self.objects, self.obj_cas, out)
            self.where += [(self.scans, s // rc.CHUNK)] * (len(self.objects) - len(self.where))
        for f, o in out.items():
            self.obj_of[f] = o
        creator = {self.objects[o][0]: o for o in range(before, len(self.objects))}
        recs = np.array([(int(c, 16), i) for i, c in enumerate(cas) if c is not None],
                        dtype=U).reshape(-1, 2).view(np.int64)
        r, owner, existing, new = index.scan(recs, rc.CHUNK)
        ids = np.zeros(len(r), U)
        for j in range(len(r)):
            f = base + int(r[j, 1])
            ids[j] = int(owner[j]) if existing[j] else creator[base + int(owner[j])]
            assert int(ids[j]) == out[f], ("scan owner", f)
            self.count["linked"] += int(existing[j])
        if len(r):  # every record's pair; the new entries are the pairs the relation gains
            had = set(zip(*[a.tolist() for a in index.export_links()[:2]]))
            want = len(set(zip(r[:, 0].view(U).tolist(), ids.tolist())) - had)
            assert index.insert(r[:, 0].view(U).copy(), ids) == want
        self.scans += 1
        self.count["scan"] += 1

    def delete_file(self, index):
        live = self.live_files()
        if not live:
            return
        f = live[int(self.rng.integers(0, len(live)))]
        o, c = self.obj_of[f], self.cas_of[f]
        first_before = self.truth().get(int(c, 16)) if c is not None else None
        self.objects[o].remove(f)
        self.obj_of[f] = -1
        self._refresh(o)
        if c is not None:
            pairs, r = index.remove(np.array([int(c, 16)], U), np.array([o], U))
            still = c in self.obj_cas[o]
            assert r == (0 if still else 1) and pairs.tolist() == ([] if still else [[int(c, 16), o]])
            self.count["kept_other_links"] += int(still)
            self._account(first_before, c, o)
        self.count["delete"] += 1

    def change_content(self, index):
        live = [f for f in self.live_files() if self.cas_of[f] is not None]
        if not live:
            return
        f = live[int(self.rng.integers(0, len(live)))]
        o, a = self.obj_of[f], self.cas_of[f]
        b = self.pool[int(self.rng.integers(0, rc.POOL))]
        if b == a:
            return
        first_a = self.truth().get(int(a, 16))
        first_b = self.truth().get(int(b, 16))
        self.cas_of[f] = b
        self._refresh(o)
        index.remove(np.array([int(a, 16)], U), np.array([o], U))
        index.insert(np.array([int(b, 16)], U), np.array([o], U))
        self.count["moved_to_earlier_object"] += int(first_b is not None and first_b > o)
        if a not in self.obj_cas[o]:
            self._account(first_a, a, o)
        self.count["change"] += 1

    def remove_orphans(self, index):
        alive = [o for o in range(len(self.objects)) if self.objects[o]]
        victims = [alive[int(i)] for i in self.rng.integers(0, len(alive), min(len(alive), 3))] if alive else []
        before = self.truth()
        held = self.relation()
        shadowed = sorted({o for k, o in before.items()
                           for p in range(o + 1, len(self.objects))
                           if self.where[p] == self.where[o] and "%016x" % k in self.obj_cas[p]})
        if shadowed:
            victims.append(shadowed[int(self.rng.integers(0, len(shadowed)))])
        for o in victims:
            for f in self.objects[o]:
                self.obj_of[f] = -1
            self.objects[o] = []
            self.obj_cas[o] = set()
        ids = [o for o in range(len(self.objects)) if not self.objects[o] and o not in self.gone]
        ids += victims[:1]  # a repeated id
        pairs, r = index.remove_objects(np.array(ids, U))
        assert r == len(pairs) and pairs.tolist() == [list(p) for p in sorted(held) if p[1] in set(victims)]
        for k, o in pairs.tolist():
            self._account(before[k], "%016x" % k, o)
        self.gone |= set(ids)
        self.count["orphans"] += 1


def check_owner_history_counts(total: dict):
    """Over rc.HISTORY_SEEDS: every event kind, a deletion that leaves the pair's other links, a
    first owner replaced by a same-step duplicate's Object, a vanished key, a change that moves
    a key to an earlier Object."""
    assert rc.HISTORY_EVENTS >= 25
    assert all(total[k] > 0 for k in ("scan", "delete", "change", "orphans", "linked", "kept_other_links",
                                      "replaced_by_same_chunk_duplicate", "key_vanished",
                                      "moved_to_earlier_object")), total
