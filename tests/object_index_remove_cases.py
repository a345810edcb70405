"""Case generators for the Object index's removals, shared by tests/test_object_index_remove.py
(the numpy mirrors and sd_cpu_*) and tests/test_gpu_object_index_remove.py (the kernels and
the device entries).  They build on tests/object_index_cases.py: the same index sizes, counts
and key sets.  Every list asserts the property it exists for, so a wrong edit cannot quietly
shrink a sweep.

A case is a script: a list of operations applied in order to one index that starts empty,
    ("insert", keys, object ids)           keep-first insert
    ("remove", keys, object ids or None)   removal by key, conditional where ids are given
    ("remove_objects", object ids)         removal by Object
all uint64 arrays.  The histories (the last part of the file) are the host cycle of
INTEGRATION.md §6 driven against oracle.identifier_spec._assign_step.

Nothing here touches a device or the library.
"""
from __future__ import annotations

import numpy as np

from oracle.identifier_spec import _assign_step
from tests import object_index_cases as oc

U = np.uint64
M64 = oc.M64
KINDS = ("uniform", "edges", "shared_prefix")
LARGE = 300_007  # > 1024 workgroups x 256: a workgroup's slice of the sliced grid is two tiles


def _present(keys: np.ndarray, q: np.ndarray) -> np.ndarray:
    return np.isin(q, keys)


def _wrong_key(k: np.ndarray) -> np.ndarray:
    """A third of the keys, chosen by their bits: every conditional pair of such a key carries a
    wrong id (so the entry stays unless another pair is right)."""
    with np.errstate(over="ignore"):
        return ((k * U(0x9E3779B97F4A7C15)) >> U(60)) % U(3) == U(0)


def conditional_ids(keys: np.ndarray, vals: np.ndarray, rk: np.ndarray):
    """Ids for the removal keys rk against the index (keys, vals): the right id for two thirds
    of the present keys, a wrong one (right ^ 1) for the others and anything for absent keys;
    and, where there is room, pairs 0 and 1 name the same key, the first wrongly, the second
    rightly.  Returns (rk, ids): rk is a copy with that pair written in."""
    rk = rk.copy()
    order = np.argsort(keys)
    sk, sv = keys[order], vals[order]
    twin = None
    if len(rk) >= 2 and len(sk):
        w = sk[_wrong_key(sk)]
        twin = w[0] if len(w) else sk[0]
        rk[0] = rk[1] = twin
    ids = oc.splitmix(4242, len(rk))
    if len(sk) and len(rk):
        at = np.minimum(np.searchsorted(sk, rk), len(sk) - 1)
        hit = sk[at] == rk
        ids[hit] = sv[at[hit]]
        wrong = hit & _wrong_key(rk)
        ids[wrong] ^= U(1)
        if twin is not None:
            right = sv[np.searchsorted(sk, twin)]
            ids[0], ids[1] = right ^ U(1), right
    return rk, ids


def by_key_scripts(kind: str):
    """(name, script) per index size and form: the index is built once, then for every removal
    count m the keys oc.queries(keys, m) are removed (present with repeats, absent between two
    keys, below the minimum, above the maximum) and the index is filled up again."""
    assert kind in KINDS
    out = []
    seen = {"right": 0, "wrong": 0, "twin": 0, "absent": 0, "repeat": 0}
    for n in oc.INDEX_SIZES:
        keys = oc.key_sets(n)[kind]
        vals = oc.vals_for(keys, 31)
        for form in ("unconditional", "conditional"):
            script = [("insert", keys, vals)]
            for m in oc.QUERY_COUNTS:
                rk = oc.queries(keys, m)
                if form == "conditional":
                    rk, ids = conditional_ids(keys, vals, rk)
                    hit = _present(keys, rk)
                    wrong = hit & _wrong_key(rk)
                    seen["right"] += int((hit & ~wrong).sum())
                    seen["wrong"] += int(wrong.sum())
                    seen["twin"] += int(m >= 2 and n >= 1)
                    script.append(("remove", rk, ids))
                else:
                    seen["absent"] += int((~_present(keys, rk)).sum())
                    seen["repeat"] += m - len(np.unique(rk))
                    script.append(("remove", rk, None))
                script.append(("insert", keys, vals))
            out.append((f"{kind}-{n}-{form}", script))
    assert len(out) == 2 * len(oc.INDEX_SIZES) == 22
    assert all(v > 0 for v in seen.values()), seen
    return out


ID_SET = np.concatenate([np.array([0, M64], dtype=U), oc.splitmix(808, 14)])  # the Objects of by_object_scripts
ABSENT_IDS = oc.splitmix(909, 16)                                           # Objects that own nothing


def by_object_scripts():
    """(name, script) per index size: values drawn from 16 ids (0 and 2^64 - 1 among them), so
    one Object owns many keys; removed are ids owning nothing, then for every count m a list
    with repeats over half of the ids and the absent ones (refilled after each), then every
    id, which empties the index; an insert into the emptied index ends the script."""
    assert len(np.unique(np.concatenate([ID_SET, ABSENT_IDS]))) == 32
    pool = np.concatenate([ID_SET[::2], ABSENT_IDS])  # 0 is in it, 2^64 - 1 is not
    assert 0 in pool.tolist() and M64 not in pool.tolist()
    out = []
    for n in oc.INDEX_SIZES:
        keys = oc.random_keys(n, 3000 + n)
        vals = ID_SET[(oc.splitmix(3100 + n, n) % U(len(ID_SET))).astype(np.int64)] if n else np.zeros(0, U)
        if n >= 255:
            assert len(np.unique(vals)) == 16 and {0, M64} <= set(vals.tolist())
        script = [("insert", keys, vals), ("remove_objects", ABSENT_IDS)]
        for m in oc.QUERY_COUNTS:
            ids = pool[(oc.splitmix(3200 + m, m) % U(len(pool))).astype(np.int64)] if m else np.zeros(0, U)
            assert m < 63 or len(np.unique(ids)) < m  # repeated ids
            script += [("remove_objects", ids), ("insert", keys, vals)]
        script += [("remove_objects", np.concatenate([ID_SET, ID_SET[:3]])), ("expect_empty",),
                   ("insert", keys[::-1].copy(), vals[::-1].copy())]
        out.append((f"objects-{n}", script))
    assert len(out) == len(oc.INDEX_SIZES)
    return out


def fixed_scripts():
    """name -> script: the first entry, the last entry and one whole directory bucket removed;
    three_growth run backwards (240 -> 40 -> 10 -> 0 entries, directory bits 4 -> 2 -> 0 -> 0)
    and an insert into the emptied index; nothing removed from an empty index."""
    n = 4097
    keys = np.sort(oc.random_keys(n, 61))
    vals = oc.vals_for(keys, 62)
    bits = oc.dir_bits(n)
    mid = keys[n // 2] >> U(64 - bits)
    bucket = keys[(keys >> U(64 - bits)) == mid]
    assert bits == 9 and 1 <= len(bucket) < n and int(bucket[0]) > int(keys[0]) and int(bucket[-1]) < int(keys[-1])
    (g1, v1), (g2, v2), (g3, v3) = oc.insert_cases()["three_growth"]
    sizes = [240, 40, 10, 0]
    assert [len(g3) - len(g1), len(g2), len(g1)] == [200, 30, 10]
    assert [oc.dir_bits(s) for s in sizes] == [4, 2, 0, 0]
    few = oc.random_keys(5, 63)
    return {
        "first": [("insert", keys, vals), ("remove", keys[:1], None)],
        "last": [("insert", keys, vals), ("remove", keys[-1:], None)],
        "first_and_last": [("insert", keys, vals), ("remove", keys[[0, -1]], vals[[0, -1]])],
        "one_bucket": [("insert", keys, vals), ("remove", bucket[::-1].copy(), None),
                       ("remove", bucket, None)],  # the second finds nothing
        "three_growth_backwards": [("insert", g1, v1), ("insert", g2, v2), ("insert", g3, v3),
                                   ("expect_count", 240), ("remove", g3[:200], None), ("expect_count", 40),
                                   ("remove", g2, v2), ("expect_count", 10), ("remove_objects", v1),
                                   ("expect_empty",), ("insert", g3, v3), ("expect_count", 210)],
        "empty_index": [("remove", few, None), ("remove", few, few), ("remove_objects", few),
                        ("remove", np.zeros(0, U), None), ("remove_objects", np.zeros(0, U)), ("expect_empty",)],
    }


def large_script():
    """One index of 300 007 entries: every other entry dropped by key; runs of 1000 consecutive
    entries dropped and kept by Object (a tile all flagged, a tile none flagged, in every
    slice); all but one dropped by key."""
    keys = np.sort(oc.random_keys(LARGE, 71))
    vals = (np.arange(LARGE, dtype=U) // U(1000))  # the Object of entry i: i // 1000
    per_wg = -(-LARGE // 1024)
    assert LARGE > 1024 * 256 and per_wg > 256  # the second tile of every workgroup has entries
    odd_runs = np.arange(1, LARGE // 1000 + 1, 2, dtype=U)
    lone = keys[123_456:123_457]
    return [("insert", keys, vals), ("remove", keys[::2].copy(), None), ("expect_count", LARGE // 2),
            ("insert", keys, vals), ("remove_objects", odd_runs), ("expect_count", LARGE - 150_000),
            ("insert", keys, vals), ("remove", keys[keys != lone[0]][::-1].copy(), None), ("expect_count", 1),
            ("remove", lone, vals[123_456:123_457]), ("expect_empty",)]


def shard_case():
    """(keys, vals, removal keys, removal Object ids) for the shard tests: every part of
    nparts 1, 2, 3, 8 is handed the same lists."""
    keys = np.concatenate([oc.random_keys(3000, 21), oc.edge_keys()])
    vals = ID_SET[(oc.splitmix(23, len(keys)) % U(len(ID_SET))).astype(np.int64)]
    rk = np.concatenate([oc.queries(keys, 2000), oc.edge_keys()[::2]])
    for nparts in oc.NPARTS:
        d = (((rk >> U(48)) * U(nparts)) >> U(16)).astype(np.int64)  # oi_dest_of
        assert set(d.tolist()) == set(range(nparts))             # the list holds keys of every shard
    return keys, vals, rk, ID_SET[::3].copy()


# ------------------------------------------------------------------ histories
HISTORY_SEEDS = (1, 2, 3, 4, 5, 6)
HISTORY_EVENTS = 30
CHUNK = 7          # identifier steps of 7 files: many steps per scan, duplicates inside and across them
POOL = 60          # cas_ids a history draws from


class History:
    """A seeded sequence of events on a library -- scans of <= 250 files over a pool of ~60
    cas_ids (empty files included), file deletions, content changes and orphan removals --
    with the oracle's tables (`objects`, `obj_cas` of oracle.identifier_spec, in which a
    removed Object stays as an empty tombstone) as the truth, and the host cycle of
    INTEGRATION.md §6 applied to the index under test:

      a file_path (c, O) deleted          conditional remove of (c, O); keep-first insert of the
                                          DB's remaining owners of c, in DB order
      a file_path changed A -> B on O     conditional remove of (A, O); B removed if its entry
                                          names a later Object than O; insert the DB's owners
                                          of {A, B}
      the orphan remover                  remove_objects(ids); insert the DB's owners of the
                                          removed keys

    Object ids are the positions in `objects` (DB order).  An orphan-removal event first takes
    every file_path of a few Objects away in the DB alone (a directory removed at once: the
    host leaves those to the orphan remover, whose remove_objects drops all their keys); where
    there is one, a first owner whose same-step duplicate's Object lives on is among them.

    `index` offers insert / remove / remove_objects / lookup / export over uint64 arrays, and
    scan(records int64 [m, 2], chunk) -> (grouped records, owner, existing, new heads)."""

    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.pool = ["%016x" % int(x) for x in oc.splitmix(7000 + seed, POOL)]
        self.cas_of, self.obj_of = [], []          # per file (ids never reused); obj_of -1 = deleted
        self.objects, self.obj_cas = [], []        # the oracle's tables
        self.where = []                            # per Object: (scan number, step) that created it
        self.gone = set()                          # Objects the orphan remover has deleted
        self.scans = 0
        self.count = {"scan": 0, "delete": 0, "change": 0, "orphans": 0,
                      "replaced_by_same_chunk_duplicate": 0, "key_vanished": 0, "moved_to_earlier_object": 0,
                      "linked": 0}

    # -- the DB
    def live_files(self):
        return [f for f, o in enumerate(self.obj_of) if o >= 0]

    def owners_of(self, cas_list):
        """(key, Object) of every live Object owning one of the cas_ids, in DB order"""
        pairs = [(int(c, 16), o) for o in range(len(self.objects)) for c in cas_list if c in self.obj_cas[o]]
        return np.array([p[0] for p in pairs], U), np.array([p[1] for p in pairs], U)

    def _refresh(self, o):
        self.obj_cas[o] = {self.cas_of[f] for f in self.objects[o] if self.cas_of[f] is not None}

    def truth(self):
        t = {}
        for o, cs in enumerate(self.obj_cas):
            for c in cs:
                t.setdefault(int(c, 16), o)
        return t

    def check(self, index, what):
        k, v = index.export()
        t = self.truth()
        assert len(k) == len(t) and np.all(k[1:] > k[:-1]), what
        assert dict(zip(k.tolist(), v.tolist())) == t, what

    # -- events
    def scan(self, index):
        n = int(self.rng.integers(1, 251))
        base = len(self.cas_of)
        cas = [None if self.rng.random() < 0.08 else self.pool[int(self.rng.integers(0, POOL))] for _ in range(n)]
        if n > 3:
            cas[1] = cas[0] = cas[0] or self.pool[0]   # a duplicate inside the first step
        self.cas_of += cas
        self.obj_of += [-1] * n
        before = len(self.objects)
        out = {}
        # the truth: step by step, each against the Objects of the steps before (mod.rs:136-333)
        for s in range(0, n, CHUNK):
            step = range(base + s, min(base + n, base + s + CHUNK))
            _assign_step(step, self.cas_of, self.objects, self.obj_cas, out)
            self.where += [(self.scans, s // CHUNK)] * (len(self.objects) - len(self.where))
        for f, o in out.items():
            self.obj_of[f] = o
        creator = {self.objects[o][0]: o for o in range(before, len(self.objects))}
        # the index under test: the whole scan at once against the index as it stood, file
        # indices local to the scan (its steps start at its first file)
        recs = np.array([(int(c, 16), i) for i, c in enumerate(cas) if c is not None],
                        dtype=U).reshape(-1, 2).view(np.int64)
        r, owner, existing, new = index.scan(recs, CHUNK)
        for j in range(len(r)):
            f = base + int(r[j, 1])
            got = int(owner[j]) if existing[j] else creator[base + int(owner[j])]
            assert got == out[f], ("scan owner", f)
            self.count["linked"] += int(existing[j])
        if len(new):
            ids = np.array([creator[base + int(f)] for f in new[:, 1]], U)
            assert index.insert(new[:, 0].copy(), ids) == len(new)
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
            index.remove(np.array([int(c, 16)], U), np.array([o], U))
            k, v = self.owners_of([c])
            index.insert(k, v)
            self._account(first_before, c, o)
        self.count["delete"] += 1

    def _account(self, first_before, c, o):
        """o lost cas c: did the first owner change, and to what?"""
        now = self.truth().get(int(c, 16))
        if first_before == o and now != o:
            if now is None:
                self.count["key_vanished"] += 1
            elif self.where[now] == self.where[o]:
                self.count["replaced_by_same_chunk_duplicate"] += 1

    def change_content(self, index):
        live = [f for f in self.live_files() if self.cas_of[f] is not None]
        if not live:
            return
        f = live[int(self.rng.integers(0, len(live)))]
        o, a = self.obj_of[f], self.cas_of[f]
        b = self.pool[int(self.rng.integers(0, POOL))]
        if b == a:
            return
        first_a = self.truth().get(int(a, 16))
        first_b = self.truth().get(int(b, 16))
        self.cas_of[f] = b
        self._refresh(o)
        kb = np.array([int(b, 16)], U)
        index.remove(np.array([int(a, 16)], U), np.array([o], U))
        ids, found = index.lookup(kb)
        if found[0] and int(ids[0]) > o:
            index.remove(kb, None)
        self.count["moved_to_earlier_object"] += int(first_b is not None and first_b > o)
        k, v = self.owners_of([a, b])
        index.insert(k, v)
        if a not in self.obj_cas[o]:
            self._account(first_a, a, o)
        self.count["change"] += 1

    def remove_orphans(self, index):
        alive = [o for o in range(len(self.objects)) if self.objects[o]]
        victims = [alive[int(i)] for i in self.rng.integers(0, len(alive), min(len(alive), 3))] if alive else []
        before = self.truth()
        # and, where there is one, a first owner whose same-step duplicate's Object lives on
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
        assert r == len(pairs) and set(pairs[:, 1].tolist()) <= set(ids)
        assert {int(k) for k, o in before.items() if o in set(victims)} == set(pairs[:, 0].tolist())
        cas = ["%016x" % int(k) for k in pairs[:, 0]]
        k, v = self.owners_of(cas)
        index.insert(k, v)
        for c, o in zip(cas, pairs[:, 1].tolist()):
            self._account(int(o), c, int(o))
        self.gone |= set(ids)
        self.count["orphans"] += 1

    def run(self, index, events: int = HISTORY_EVENTS):
        self.scan(index)
        self.check(index, "first scan")
        for e in range(1, events):
            kind = ("scan", "delete", "change", "orphans")[int(self.rng.choice(4, p=[0.25, 0.3, 0.3, 0.15]))]
            {"scan": self.scan, "delete": self.delete_file, "change": self.change_content,
             "orphans": self.remove_orphans}[kind](index)
            self.check(index, (e, kind))
        return self.count


def check_history_counts(total: dict):
    """Over HISTORY_SEEDS every kind of event ran and each of the outcomes the cycle exists for
    happened: a removed first owner replaced by a surviving same-chunk duplicate's Object, a
    key gone for good, a content change that moved a key to an earlier Object."""
    assert HISTORY_EVENTS >= 25
    assert all(total[k] > 0 for k in ("scan", "delete", "change", "orphans", "linked",
                                      "replaced_by_same_chunk_duplicate", "key_vanished",
                                      "moved_to_earlier_object")), total
