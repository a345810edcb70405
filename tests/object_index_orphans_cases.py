"""Cases for the view by Object of an owners-mode index (include/sd_cas.h:
sd_object_index_object_links, sd_object_index_orphans), shared by
tests/test_object_index_orphans.py (the numpy mirror and the sd_cpu_* twin) and
tests/test_gpu_object_index_orphans.py (the kernels and the device entries).  They build on
tests/object_index_owners_cases.py and tests/object_index_apply_cases.py: the same shapes, pools
and histories.  Every list asserts the property it exists for, so a wrong edit cannot quietly
shrink a sweep.

An index under test offers what the apply cases ask for, and
    object_links(ids, stride=1, m=None) -> (links, entries)     uint64 [m]
    orphans(ids, stride=1, m=None) -> the distinct ids without an entry, ascending
    apply_orphans(rm_keys, rm_ids, in_keys, in_ids) -> (dropped pairs, r, taken, orphans)

Nothing here touches a device or the library.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import object_index_apply_cases as ac
from tests import object_index_cases as oc
from tests import object_index_owners_cases as wc
from tests import object_index_remove_cases as rc

U = np.uint64
M64 = oc.M64
E = ac.E
LDS_IDS = 1024  # object_index.hip OI_LDS_IDS: lists of at most this many ids are searched in LDS
HIGH = 1 << 63


class DictOrphans(ac.DictApply):
    """The rule of object_index.h over wc.DictOwners' relation (key, id) -> links, word for word:
    entries(o) = the entries whose id is o, links(o) = the sum of their links, o is unowned iff
    entries(o) == 0."""

    def _totals(self):
        links, entries = Counter(), Counter()
        for (k, o), c in self.d.items():
            links[o] += c
            entries[o] += 1
        return links, entries

    def object_links(self, ids, stride=1, m=None):
        ids = listed(ids, stride, m)
        links, entries = self._totals()
        return (np.array([links[o] for o in ids.tolist()], dtype=U),
                np.array([entries[o] for o in ids.tolist()], dtype=U))

    def orphans(self, ids, stride=1, m=None):
        ids = listed(ids, stride, m)
        entries = self._totals()[1]
        return np.array(sorted({o for o in ids.tolist() if entries[o] == 0}), dtype=U)

    def apply_orphans(self, rk, rv, ik, iv):
        pairs, r, taken = self.apply(rk, rv, ik, iv)
        return pairs, r, taken, self.orphans(pairs[:, 1].copy())


def listed(ids, stride=1, m=None):
    """the m ids a call reads: element j is ids[j * stride]"""
    ids = np.asarray(ids, U).reshape(-1)
    m = (len(ids) + stride - 1) // stride if m is None else m
    return ids[: (m - 1) * stride + 1: stride] if m else ids[:0]


# ------------------------------------------------------------------ id lists
def id_lists(k, v):
    """name -> ids for an index that holds the pairs (k, v): one case per name."""
    have = np.unique(v)
    absent = oc.splitmix(7700 + len(k), 40)
    absent = absent[~np.isin(absent, have)]
    assert len(absent) >= 30
    one = have[:1] if len(have) else absent[:1]
    high = np.array([M64, M64 - 1, HIGH, HIGH + 5, HIGH - 1, 0, 5, 1], dtype=U)  # orphans ascend UNSIGNED
    keyish = np.unique(k)[:6]  # ids equal to key values: to be matched against vals, never keys
    mixed = np.concatenate([have[:300], absent[:7], have[:300][::3], absent[:3], high])
    mixed = mixed[np.argsort(oc.splitmix(len(k) + 9, len(mixed)))]
    out = {"empty": E, "one": one, "repeats": np.repeat(one, 9), "all_absent": absent,
           "all_present": have[np.argsort(oc.splitmix(3, len(have)))], "above_2_63": high,
           "equals_a_key": np.concatenate([keyish, one]), "mixed": mixed}
    assert len(out) == 8 and (high >= U(HIGH)).sum() == 4
    return out


def lds_lists(vals):
    """Lists around the LDS staging threshold for an index with the Object ids `vals` (more than
    LDS_IDS + 1 distinct): LDS_IDS - 1, LDS_IDS and LDS_IDS + 1 ids, every second one present;
    and more than LDS_IDS ids of which fewer are distinct (searched in global memory, d small)."""
    have = np.unique(vals)
    assert len(have) > LDS_IDS + 1
    absent = oc.splitmix(8800, LDS_IDS + 8)
    absent = absent[~np.isin(absent, have)]
    out = {}
    for m in (LDS_IDS - 1, LDS_IDS, LDS_IDS + 1):
        ids = np.concatenate([have[: (m + 1) // 2], absent[: m // 2]])
        assert len(ids) == m == len(np.unique(ids))
        out[f"m_{m}"] = ids[np.argsort(oc.splitmix(m, m))]
    rep = np.concatenate([have[:350], absent[:350], have[:350], absent[:350], have[:100]])
    assert len(rep) > LDS_IDS and len(np.unique(rep)) == 700
    out["m_1500_d_700"] = rep
    return out


def one_owner_case():
    """1025 entries (five workgroups), all of one Object, with 1 to 3 links each."""
    k = oc.random_keys(1025, 4321)
    ik = np.concatenate([k, k[::2], k[::5]])
    return ik, np.full(len(ik), 77, U), np.array([77, 78, 77, 0], dtype=U)


def many_copies_case():
    """One pair inserted wc.COPIES (70 000) times, another pair of the same Object once, and a
    second Object: links(9) = 70 001 over two entries."""
    k = np.concatenate([np.full(wc.COPIES, 42, U), np.array([43, 44], dtype=U)])
    v = np.concatenate([np.full(wc.COPIES, 9, U), np.array([9, 10], dtype=U)])
    ids = np.array([9, 10, 11], dtype=U)
    return k, v, ids, (np.array([wc.COPIES + 1, 1, 0], dtype=U), np.array([2, 1, 0], dtype=U))


def long_run_lists():
    """wc.long_run_case(): the RUN (3000) owners of one key, every one of them listed (more ids
    than the LDS holds) with absent ids and the key's own value between them."""
    keys, ids, key, owners = wc.long_run_case()
    q = np.concatenate([owners, oc.splitmix(659, 50), np.array([key], dtype=U)])
    return keys, ids, q[np.argsort(oc.splitmix(660, len(q)))]


def check_lists(x, d, lists, what=""):
    """object_links and orphans of x equal the statement's d for every list; the orphans are
    distinct and ascend as u64; entries == 0 exactly for the orphans."""
    for name, ids in lists.items():
        gl, ge = x.object_links(ids)
        wl, we = d.object_links(ids)
        assert np.array_equal(gl, wl) and np.array_equal(ge, we), (what, name, "object_links")
        go, wo = x.orphans(ids), d.orphans(ids)
        assert go.dtype == U and np.array_equal(go, wo), (what, name, "orphans")
        assert np.all(go[1:] > go[:-1]), (what, name)
        assert set(go.tolist()) == set(np.asarray(ids, U)[ge == 0].tolist()), (what, name)


def removed_rows_case():
    """(pairs, removal list): 40 Objects of 15 pairs each, Objects 30.. with two links per pair.
    The removal takes every pair of Objects 0..9 (they become orphans), one pair of each of
    10..19 (they keep the others), one link of every pair of 30..39 (no entry leaves), and
    absent pairs."""
    k = oc.random_keys(600, 1212)
    v = np.arange(600, dtype=U) % U(40)
    two = v >= U(30)
    gone, one = v < U(10), (v >= U(10)) & (v < U(20)) & (np.arange(600) < 40)
    rk = np.concatenate([k[gone], k[one], k[two], oc.random_keys(5, 1313)])
    rv = np.concatenate([v[gone], v[one], v[two], np.arange(5, dtype=U)])
    sh = np.argsort(oc.splitmix(1414, len(rk)))
    assert int(one.sum()) == 10
    return np.concatenate([k, k[two]]), np.concatenate([v, v[two]]), rk[sh], rv[sh]


def check_stride_2(x, d, what=""):
    """Real d_removed_out rows: the id column read at stride 2 answers as the ids copied out."""
    k, v, rk, rv = removed_rows_case()
    for i in (x, d):
        i.insert(k, v)
    got, want = x.apply_orphans(rk, rv, E, E), d.apply_orphans(rk, rv, E, E)
    pairs = got[0]
    assert got[1:3] == want[1:3] and np.array_equal(pairs, want[0]) and len(pairs) > 20, what
    assert np.array_equal(got[3], want[3]) and 0 < len(got[3]) < len(np.unique(pairs[:, 1])), what
    flat = np.ascontiguousarray(pairs).reshape(-1)
    r = len(pairs)
    assert np.array_equal(x.orphans(flat[1:], 2, r), want[3]), what
    gl, ge = x.object_links(flat[1:], 2, r)
    wl, we = d.object_links(pairs[:, 1].copy())
    assert np.array_equal(gl, wl) and np.array_equal(ge, we), what
    # stride 2 from element 0 reads the key column: keys are no Object ids here
    assert np.array_equal(x.orphans(flat, 2, r), d.orphans(pairs[:, 0].copy())), what


def shard_case():
    """(pairs of every shard with repeats, ids: owners of one shard, of several, of none)."""
    k, v, _, _, rids = wc.shard_case()
    ids = np.concatenate([np.unique(v)[::2], rids, oc.splitmix(31, 9), np.unique(v)[:5]])
    return k, v, ids


# ------------------------------------------------------------------ histories
class OrphansHistory(ac.ApplyHistory):
    """ac.ApplyHistory with the orphan cycle of INTEGRATION.md §6, which asks the DB neither for
    owners nor for orphans (both queries raise):

      candidates     the Object ids of the pairs that left the index since the last pass (the
                     reports of apply), and every Object that lost a file_path without a cas_id
      casless[O]     the host's count of O's file_paths without a cas_id, adjusted when a scan
                     creates one, when one is deleted, and when a file is emptied or un-emptied
      the pass       orphans(candidates); an Object is deleted iff the index lists it AND
                     casless[O] == 0; no remove_objects call

    A removed directory is one coalesced apply.  After every pass the deleted Objects equal the
    DB's Objects without a file_path; after every event object_links of all live Objects equals
    the relation's sums."""

    def __init__(self, seed: int):
        super().__init__(seed)
        self.candidates, self.casless, self.ever_linked = set(), Counter(), set()
        self.count.update({"orphaned_by_last_link": 0, "candidate_kept_other_cas": 0, "saved_by_casless": 0,
                           "orphan_never_indexed": 0, "emptied": 0, "unemptied": 0, "deleted_casless": 0,
                           "directory": 0})

    def orphans_of_db(self):
        raise AssertionError("the orphan cycle never scans the DB for Objects without file_paths")

    # -- the host's bookkeeping
    def _left(self, pairs):
        self.candidates |= set(pairs[:, 1].tolist())

    def scan(self, index):
        base, before = len(self.cas_of), len(self.objects)
        super().scan(index)
        for f in range(base, len(self.cas_of)):
            if self.cas_of[f] is None:
                self.casless[self.obj_of[f]] += 1
        self.ever_linked |= {self.obj_of[f] for f in range(base, len(self.cas_of)) if self.cas_of[f] is not None}
        assert len(self.objects) >= before

    def delete_file(self, index):
        live = self.live_files()
        if not live:
            return
        # every third deletion takes a file_path without a cas_id where there is one
        empty = [f for f in live if self.cas_of[f] is None]
        f = empty[int(self.rng.integers(0, len(empty)))] if empty and self.rng.random() < 0.34 else \
            live[int(self.rng.integers(0, len(live)))]
        o, c = self.obj_of[f], self.cas_of[f]
        first_before = self.truth().get(int(c, 16)) if c is not None else None
        self.objects[o].remove(f)
        self.obj_of[f] = -1
        self._refresh(o)
        if c is None:
            self.casless[o] -= 1
            self.candidates.add(o)
            self.count["deleted_casless"] += 1
        else:
            pairs, r, taken = index.apply(np.array([int(c, 16)], U), np.array([o], U), E, E)
            self._left(pairs)
            self.count["kept_other_links"] += int(r == 0)
            self._account(first_before, c, o)
        self.count["delete"] += 1

    def change_content(self, index):
        n_before = self.count["change"]
        had = self.relation()
        super().change_content(index)
        if self.count["change"] != n_before:
            self._left(np.array(sorted(set(had) - set(self.relation())), dtype=U).reshape(-1, 2))
            self.ever_linked |= {o for _, o in self.relation()}

    def burst(self, index):
        had = self.relation()
        super().burst(index)
        self._left(np.array(sorted(set(had) - set(self.relation())), dtype=U).reshape(-1, 2))
        self.ever_linked |= {o for _, o in self.relation()}

    def empty_file(self, index):
        """a watcher update takes a file_path to empty content: its cas_id becomes None on its Object"""
        live = [f for f in self.live_files() if self.cas_of[f] is not None]
        if not live:
            return
        # every second time the only file_path with content of its Object, where there is one: the
        # Object then owns nothing in the index and lives on through its empty file_path
        lone = [f for f in live if sum(self.cas_of[g] is not None for g in self.objects[self.obj_of[f]]) == 1]
        pick = lone if lone and self.rng.random() < 0.5 else live
        f = pick[int(self.rng.integers(0, len(pick)))]
        o, c = self.obj_of[f], self.cas_of[f]
        first_before = self.truth().get(int(c, 16))
        self.cas_of[f] = None
        self._refresh(o)
        pairs, r, taken = index.apply(np.array([int(c, 16)], U), np.array([o], U), E, E)
        self._left(pairs)
        self.casless[o] += 1
        if c not in self.obj_cas[o]:
            self._account(first_before, c, o)
        self.count["emptied"] += 1

    def unempty_file(self, index):
        """... and from empty content to a cas_id, on the same Object"""
        live = [f for f in self.live_files() if self.cas_of[f] is None]
        if not live:
            return
        f = live[int(self.rng.integers(0, len(live)))]
        o = self.obj_of[f]
        b = self.pool[int(self.rng.integers(0, rc.POOL))]
        self.cas_of[f] = b
        self._refresh(o)
        index.apply(E, E, np.array([int(b, 16)], U), np.array([o], U))
        self.casless[o] -= 1
        self.candidates.add(o)  # it lost a file_path without a cas_id
        self.ever_linked.add(o)
        self.count["unemptied"] += 1

    def remove_orphans(self, index):
        """A directory removed at once -- every file_path of a few Objects, delivered as ONE
        coalesced apply -- and then the orphan pass."""
        alive = [o for o in range(len(self.objects)) if self.objects[o]]
        victims = [alive[int(i)] for i in self.rng.integers(0, len(alive), min(len(alive), 3))] if alive else []
        before = self.truth()
        held = self.relation()
        shadowed = sorted({o for k, o in before.items()
                           for p in range(o + 1, len(self.objects))
                           if self.where[p] == self.where[o] and "%016x" % k in self.obj_cas[p]})
        if shadowed:
            victims.append(shadowed[int(self.rng.integers(0, len(shadowed)))])
        rm = []
        for o in sorted(set(victims)):
            for f in self.objects[o]:
                self.obj_of[f] = -1
                if self.cas_of[f] is None:
                    self.casless[o] -= 1
                    self.candidates.add(o)
                else:
                    rm.append((int(self.cas_of[f], 16), o))
            self.objects[o] = []
            self.obj_cas[o] = set()
        rm = [rm[j] for j in self.rng.permutation(len(rm))]
        pairs, r, taken, now = index.apply_orphans(np.array([p[0] for p in rm], dtype=U),
                                                   np.array([p[1] for p in rm], dtype=U), E, E)
        assert taken == 0 and pairs.tolist() == [list(p) for p in sorted(held) if p[1] in set(victims)]
        assert set(now.tolist()) == {o for o in set(pairs[:, 1].tolist())}  # every pair of a victim left
        self._left(pairs)
        for k, o in pairs.tolist():
            self._account(before[k], "%016x" % k, o)
        self.count["directory"] += 1
        self.orphan_pass(index)

    def orphan_pass(self, index):
        cand = np.array(sorted(self.candidates), dtype=U)
        cand = cand[np.argsort(oc.splitmix(len(cand) + 1, len(cand)))] if len(cand) else cand
        found = index.orphans(np.concatenate([cand, cand[:1]]))  # a repeated id
        delete = [o for o in found.tolist() if self.casless[o] == 0]
        want = [o for o in range(len(self.objects)) if not self.objects[o] and o not in self.gone]
        assert sorted(delete) == want, (delete, want)
        links, entries = index.object_links(cand)
        for o, e in zip(cand.tolist(), entries.tolist()):
            self.count["candidate_kept_other_cas"] += int(e > 0)
        for o in found.tolist():
            self.count["saved_by_casless"] += int(self.casless[o] > 0)
        for o in delete:
            self.count["orphaned_by_last_link" if o in self.ever_linked else "orphan_never_indexed"] += 1
        assert all(v >= 0 for v in self.casless.values())
        self.gone |= set(delete)
        self.candidates.clear()
        self.count["orphans"] += 1

    def check_object_links(self, index, what):
        live = [o for o in range(len(self.objects)) if self.objects[o]]
        ids = np.array(live + sorted(self.gone)[:5], dtype=U)
        links, entries = Counter(), Counter()
        for (k, o), c in self.relation().items():
            links[o] += c
            entries[o] += 1
        gl, ge = index.object_links(ids)
        assert gl.tolist() == [links[o] for o in ids.tolist()], what
        assert ge.tolist() == [entries[o] for o in ids.tolist()], what
        # and the host's map is the DB's count of file_paths without a cas_id
        assert all(self.casless[o] == sum(self.cas_of[f] is None for f in self.objects[o]) for o in live), what

    def run(self, index, events: int = rc.HISTORY_EVENTS + 10):
        self.scan(index)
        self.check(index, "first scan")
        kinds = {"scan": self.scan, "delete": self.delete_file, "change": self.change_content,
                 "orphans": self.remove_orphans, "burst": self.burst, "empty": self.empty_file,
                 "unempty": self.unempty_file}
        names = sorted(kinds)
        for e in range(1, events):
            kind = names[int(self.rng.choice(len(names), p=[0.1, 0.1, 0.2, 0.1, 0.15, 0.2, 0.15]))]
            kinds[kind](index)
            self.check(index, (e, kind))
            self.check_object_links(index, (e, kind))
        self.orphan_pass(index)
        return self.count


def check_orphan_history_counts(total: dict):
    """Over rc.HISTORY_SEEDS: every event kind ran, and each outcome the cycle exists for happened
    at least once: an Object orphaned by its last link, a candidate that kept links under another
    cas_id, a candidate saved only by a file_path without a cas_id, an orphan that never had an
    indexed link."""
    assert all(total[k] > 0 for k in ("scan", "delete", "change", "orphans", "burst", "emptied", "unemptied",
                                      "deleted_casless", "directory", "orphaned_by_last_link",
                                      "candidate_kept_other_cas", "saved_by_casless", "orphan_never_indexed")), total
