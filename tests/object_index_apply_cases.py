"""Cases for sd_object_index_apply (include/sd_cas.h: removals, then insertions, of an
owners-mode index in one call), shared by tests/test_object_index_apply.py (the numpy mirror and
sd_cpu_object_index_apply) and tests/test_gpu_object_index_apply.py (the kernels and the device
entry).  They build on tests/object_index_owners_cases.py: the same pools, shapes and histories.
Every list asserts the property it exists for, so a wrong edit cannot quietly shrink a sweep.

An index under test offers what the owners cases ask for, and
    apply(rm_keys, rm_ids, in_keys, in_ids) -> (dropped pairs [r, 2], r, taken)
A script is a list of the owners cases' operations and ("apply", rm_keys, rm_ids, in_keys,
in_ids), applied in order to one index that starts empty.

Nothing here touches a device or the library.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import object_index_cases as oc
from tests import object_index_owners_cases as wc
from tests import object_index_remove_cases as rc

U = np.uint64
M64 = oc.M64
E = np.zeros(0, U)  # an empty list


class DictApply(wc.DictOwners):
    """wc.DictOwners with the apply rule of include/sd_cas.h word for word."""

    def apply(self, rm_keys, rm_ids, in_keys, in_ids):
        asked = Counter(zip(rm_keys.tolist(), rm_ids.tolist()))
        added = Counter(p for p in zip(in_keys.tolist(), in_ids.tolist()) if self._mine(p[0]))
        gone, taken = [], 0
        for p in set(asked) | set(added):
            held = self.d.get(p, 0)
            kept = 0 if held == 0 or (asked[p] != 0 and asked[p] >= held) else held - asked[p]
            after = kept + added[p]
            if held > 0 and after == 0:
                gone.append(p)
                del self.d[p]
            elif after > 0:
                taken += held == 0
                self.d[p] = after
        gone.sort()
        return np.array(gone, dtype=U).reshape(-1, 2), len(gone), taken


# ------------------------------------------------------------------ seeded scripts
APPLY_SEEDS = (21, 22, 23, 24)
APPLY_OPS = 40
APPLY_KINDS = tuple(f"{a}_{b}" for a in ("less", "equal", "more") for b in ("none", "some"))


def seeded_script(seed: int):
    """A script of APPLY_OPS operations over wc.pools(seed), generated against the dict
    statement: apply mixed with insert and the three removals.  Over the script the removal
    lists ask fewer links than held, as many and more, each with and without links of the same
    pair in the insertion list (so a pair is dropped and re-added in one call), name absent
    pairs and present keys with another id; both lists repeat pairs."""
    rng = np.random.default_rng(seed)
    keys, ids = wc.pools(seed)
    d = DictApply()
    script, seen = [], Counter()

    def draw(m):
        return keys[rng.integers(0, len(keys), m)], ids[rng.integers(0, len(ids), m)]

    for step in range(APPLY_OPS):
        kind = "insert" if step < 2 else ("apply", "insert", "remove", "remove_keys", "remove_objects")[
            int(rng.choice(5, p=[0.6, 0.15, 0.1, 0.05, 0.1]))]
        if kind == "insert":
            op = ("insert",) + draw(int(rng.choice([5, 60, 300])))
        elif kind == "remove":
            k, v = draw(20)
            op = ("remove", k, v)
        elif kind == "remove_keys":
            op = ("remove", keys[rng.integers(0, len(keys), 2)], None)
        elif kind == "remove_objects":
            op = ("remove_objects", ids[rng.integers(0, len(ids), 1)])
        else:
            held = list(d.d.items())
            rm, ins = [], []
            for j in rng.permutation(len(held))[:8]:
                (k, v), c = held[j]
                ask = (max(c - 1, 1), c, c + 2)[int(rng.integers(0, 3))]
                add = int(rng.integers(0, 2)) * int(rng.integers(1, 4))
                how = "less" if ask < c else "equal" if ask == c else "more"
                seen[how + ("_some" if add else "_none")] += 1
                seen["drop_and_re_add"] += int(ask >= c and add > 0)
                rm += [(k, v)] * ask
                ins += [(k, v)] * add
                seen["repeats_rm"] += int(ask > 1)
                seen["repeats_in"] += int(add > 1)
                if (k, v ^ 1) not in d.d:
                    rm.append((k, v ^ 1))  # a present key with another id
                    seen["other_id"] += 1
            ak, av = draw(4)
            absent = [p for p in zip(ak.tolist(), av.tolist()) if p not in d.d]
            seen["absent"] += len(absent)
            rm += absent
            nk, nv = draw(int(rng.choice([0, 3, 40])))  # new pairs, and more links for present ones
            ins += list(zip(nk.tolist(), nv.tolist()))
            rm = [rm[j] for j in rng.permutation(len(rm))]
            ins = [ins[j] for j in rng.permutation(len(ins))]
            op = ("apply", np.array([p[0] for p in rm], dtype=U), np.array([p[1] for p in rm], dtype=U),
                  np.array([p[0] for p in ins], dtype=U), np.array([p[1] for p in ins], dtype=U))
        script.append(op)
        getattr(d, op[0])(*op[1:])
    want = APPLY_KINDS + ("drop_and_re_add", "absent", "other_id", "repeats_rm", "repeats_in")
    assert all(seen[w] > 0 for w in want), (seed, seen)
    return script


# ------------------------------------------------------------------ shapes
def fresh_pairs(n: int, salt: int, k, v):
    """n distinct pairs none of which is among (k, v), unsorted: uniform keys, and -- from 4 on
    -- a smaller and a larger id under k's smallest and largest key where those are free."""
    if n == 0:
        return E, E
    nk = oc.random_keys(n, 9000 + salt)
    nv = oc.vals_for(nk, 61 + salt) | U(32)
    have = set(zip(k.tolist(), v.tolist()))
    if n >= 4 and len(k):
        lo, hi = int(k.min()), int(k.max())
        for j, p in enumerate(((lo, 1), (lo, M64 - 1), (hi, 1), (hi, M64 - 1))):
            if p not in have:
                nk[j], nv[j] = p
    assert len(set(zip(nk.tolist(), nv.tolist()))) == n and not (set(zip(nk.tolist(), nv.tolist())) & have)
    return nk, nv


def entry_count_script(n: int):
    """On the index of wc.shaped_pairs(n): every fourth entry leaves while as many new pairs
    enter (the count stands, the prefixes do not); all leave, none enter; all leave and n new
    pairs enter; none leave, pairs enter at rank 0 and at rank n; an apply on the empty index."""
    k, v = wc.shaped_pairs(n)
    q = slice(0, None, 4)
    f1k, f1v = fresh_pairs(len(k[q]), n, k, v)
    f2k, f2v = fresh_pairs(n, n + 1, k, v)
    script = [("apply", E, E, k, v), ("expect_count", n),                    # on the empty index
              ("apply", k[q].copy(), v[q].copy(), f1k, f1v), ("expect_count", n),
              ("apply", np.concatenate([k, f1k]), np.concatenate([v, f1v]), E, E), ("expect_count", 0),
              ("apply", k, v, E, E), ("expect_count", 0),                     # removals from the empty index
              ("insert", k, v),
              ("apply", k, v, f2k, f2v), ("expect_count", n)]
    # rank 0 and rank n: below the smallest pair and above the largest of what is there now
    lo, hi = (0, 0), (M64, M64)
    have = set(zip(f2k.tolist(), f2v.tolist()))
    assert lo not in have and hi not in have
    script += [("apply", E, E, np.array([lo[0], hi[0]], dtype=U), np.array([lo[1], hi[1]], dtype=U)),
               ("expect_count", n + 2)]
    return script


def large_script():
    """wc.LARGE entries (a slice of the sliced passes is two tiles); 1 % leave and 1 % enter,
    then half of those leave again while a third of the first leavers come back."""
    k, v = wc.shaped_pairs(wc.LARGE)
    c = wc.LARGE // 100
    out = np.argsort(oc.splitmix(77, wc.LARGE))[:c]
    fk, fv = fresh_pairs(c, 5, k, v)
    back = k[out][::3].copy(), v[out][::3].copy()
    assert c > 2600
    return [("insert", k, v), ("apply", k[out], v[out], fk, fv), ("expect_count", wc.LARGE),
            ("apply", fk[::2].copy(), fv[::2].copy()) + back,
            ("expect_count", wc.LARGE - (c + 1) // 2 + len(back[0]))]


def straddle_scripts():
    """On wc.straddle_case() (positions 255 | 256 hold the two owners, ids 4 and 10, of one
    key): name -> script.  Every script starts from the 600 entries."""
    keys, ids, key = wc.straddle_case()
    o = np.lexsort((ids, keys))
    sk, sv = keys[o], ids[o]
    assert (int(sk[255]), int(sv[255]), int(sk[256]), int(sv[256])) == (int(key), 4, int(key), 10)
    one = lambda a, b: (np.array([a], dtype=U), np.array([b], dtype=U))  # noqa: E731
    before_255 = (int(sk[254]), int(sv[254]) + 1)   # ranks at 255: directly before the entry at 255
    assert sk[254] < key
    cases = {
        # an entering pair lands between the two owners (rank 256)
        "between": [("apply", E, E) + one(key, 7)],
        # the leaving entry is position 255 while the entering pair ranks at 256
        "leave_255_enter_256": [("apply",) + one(key, 4) + one(key, 7)],
        # the leaving entry is position 256 while the entering pair ranks at 255
        "leave_256_enter_255": [("apply",) + one(key, 10) + one(*before_255)],
        # an entering pair directly before and directly after a leaving entry
        "around_leaving_255": [("apply",) + one(key, 4) + (np.array([before_255[0], key], dtype=U),
                                                           np.array([before_255[1], 7], dtype=U))],
        "around_leaving_256": [("apply",) + one(key, 10) + (np.array([key, key], dtype=U), np.array([7, 11], dtype=U))],
    }
    return keys, ids, key, {name: [("insert", keys, ids)] + s + [("expect_count", 600 + len(s[0][3]) - len(s[0][1]))]
                            for name, s in cases.items()}


def long_run_script():
    """In wc.long_run_case()'s RUN owners of one key every second owner leaves and RUN / 2 new
    owners of that key enter."""
    keys, ids, key, owners = wc.long_run_case()
    new = oc.splitmix(658, wc.RUN // 2)
    assert not np.isin(new, owners).any() and len(np.unique(new)) == wc.RUN // 2
    so = np.sort(owners)
    return keys, ids, key, [("insert", keys, ids),
                            ("apply", np.full(wc.RUN // 2, key, U), so[::2].copy(), np.full(wc.RUN // 2, key, U), new),
                            ("expect_count", 2000 + wc.RUN)]


def dir_bits_script():
    """Crossing 16 entries (directory bits 0 <-> 1) in both directions, one call each."""
    k, v = wc.shaped_pairs(15)
    fk, fv = fresh_pairs(6, 3, k, v)
    assert [oc.dir_bits(n) for n in (15, 19, 14)] == [0, 1, 0]
    return [("insert", k, v),
            ("apply", k[:2].copy(), v[:2].copy(), fk, fv), ("expect_count", 19),       # 15 - 2 + 6: up
            ("apply", np.concatenate([fk, k[2:3]]), np.concatenate([fv, v[2:3]]), k[:2].copy(), v[:2].copy()),
            ("expect_count", 14)]                                                      # 19 - 7 + 2: down


def growth_script():
    """Entering - leaving exceeds the spare capacity twice, with the pairs of wc.growth_steps()
    (10, then 37, then 242 entries against capacities 16 and 37): each step's pairs enter while
    a few of the step before leave."""
    (g1, v1), (g2, v2), (g3, v3) = wc.growth_steps()
    assert oc.dir_bits(10) < oc.dir_bits(37) < oc.dir_bits(242)
    return [("apply", E, E, g1, v1), ("expect_count", 10),
            ("apply", g1[:3].copy(), v1[:3].copy(), g2, v2), ("expect_count", 37),
            ("apply", np.concatenate([g2[:5], g2[:5]]), np.concatenate([v2[:5], v2[:5]]), g3, v3),
            ("expect_count", 242)]


def in_place_case():
    """(keys, ids of an index in which every pair holds 3 links; an apply after which nothing
    leaves or enters: one link less, two less and one more, one more, two less and two more)."""
    k, v = wc.shaped_pairs(1025)
    a, b, c, d = (slice(j, None, 4) for j in range(4))
    rm = np.concatenate([k[a], k[b], k[b], k[d], k[d]]), np.concatenate([v[a], v[b], v[b], v[d], v[d]])
    ins = np.concatenate([k[b], k[c], k[d], k[d]]), np.concatenate([v[b], v[c], v[d], v[d]])
    want = np.full(1025, 3, U)
    want[a], want[b], want[c], want[d] = 2, 2, 4, 3
    return (np.tile(k, 3), np.tile(v, 3)), rm, ins, (k, v, want)


# ------------------------------------------------------------------ histories
class ApplyHistory(wc.OwnersHistory):
    """wc.OwnersHistory with the one-call cycle of INTEGRATION.md §6:

      a file_path (c, O) deleted           apply with an empty insertion list
      a file_path changed A -> B on O      ONE apply: (A, O) goes, (B, O) comes
      a burst                              several deletions, content changes and newly linked
                                           file_paths of existing Objects, coalesced: ONE apply

    Coalescing keeps the events' order in one respect: a link that came earlier in the burst and
    goes again is struck from the insertion list instead of joining the removal list, because
    the call takes links before it adds them.  A link that goes and comes back stays in both
    lists (the drop-and-re-add of one pair).  owners_of still raises; after every event check()
    holds."""

    def __init__(self, seed: int):
        super().__init__(seed)
        self.count.update({"burst": 0, "burst_drop_and_re_add": 0, "change_kept_count": 0})

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
            pairs, r, taken = index.apply(np.array([int(c, 16)], U), np.array([o], U), E, E)
            still = c in self.obj_cas[o]
            assert taken == 0 and r == (0 if still else 1) and pairs.tolist() == ([] if still else [[int(c, 16), o]])
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
        had_b = b in self.obj_cas[o]
        self.cas_of[f] = b
        self._refresh(o)
        n = len(index)
        pairs, r, taken = index.apply(np.array([int(a, 16)], U), np.array([o], U), np.array([int(b, 16)], U),
                                      np.array([o], U))
        gone = a not in self.obj_cas[o]
        assert r == int(gone) and taken == int(not had_b) and len(index) == n - r + taken
        self.count["change_kept_count"] += int(r == 1 and taken == 1)
        self.count["moved_to_earlier_object"] += int(first_b is not None and first_b > o)
        if gone:
            self._account(first_a, a, o)
        self.count["change"] += 1

    def burst(self, index):
        """Deletions, content changes (one of them back to a cas_id that another event of the
        burst took the last link of) and new file_paths of existing Objects, in the DB first;
        then the coalesced lists in one apply."""
        before = self.relation()
        rm, ins = [], []

        def went(p):
            """the coalescing rule: a link that came earlier in the burst and goes again never
            reaches the index (the removals apply before the insertions, so it could not be taken)"""
            if p in ins:
                ins.remove(p)
            else:
                rm.append(p)
        for _ in range(int(self.rng.integers(3, 9))):
            live = [f for f in self.live_files() if self.cas_of[f] is not None]
            if not live:
                break
            f = live[int(self.rng.integers(0, len(live)))]
            o, a = self.obj_of[f], self.cas_of[f]
            what = int(self.rng.integers(0, 3))
            if what == 0:  # deleted
                self.objects[o].remove(f)
                self.obj_of[f] = -1
                went((int(a, 16), o))
            elif what == 1:  # changed A -> B
                b = self.pool[int(self.rng.integers(0, rc.POOL))]
                self.cas_of[f] = b
                went((int(a, 16), o)), ins.append((int(b, 16), o))
            else:  # a new file_path of O: with a cas_id the burst took from O if there is one
                mine = [p for p in rm if p[1] == o]
                c = "%016x" % mine[0][0] if mine else self.pool[int(self.rng.integers(0, rc.POOL))]
                self.cas_of.append(c), self.obj_of.append(o), self.objects[o].append(len(self.cas_of) - 1)
                ins.append((int(c, 16), o))
            self._refresh(o)
        # and a file moved away whose copy stays behind: the only link of (A, O) goes to another
        # cas_id and a new file_path of O brings it back -- the pair is dropped and re-added
        now = self.relation()
        lone = [f for f in self.live_files() if self.cas_of[f] is not None
                and now[(int(self.cas_of[f], 16), self.obj_of[f])] == 1 == before.get((int(self.cas_of[f], 16), self.obj_of[f]))
                and (int(self.cas_of[f], 16), self.obj_of[f]) not in ins + rm]
        if lone:
            f = lone[int(self.rng.integers(0, len(lone)))]
            o, a = self.obj_of[f], self.cas_of[f]
            self.cas_of[f] = [c for c in self.pool if c != a][int(self.rng.integers(0, rc.POOL - 1))]
            went((int(a, 16), o)), ins.append((int(self.cas_of[f], 16), o))
            self.cas_of.append(a), self.obj_of.append(o), self.objects[o].append(len(self.cas_of) - 1)
            ins.append((int(a, 16), o))
            self._refresh(o)
        after = self.relation()
        asked, added = Counter(rm), Counter(ins)
        self.count["burst_drop_and_re_add"] += sum(1 for p in asked if asked[p] >= before.get(p, 0) > 0 and added[p] > 0)
        pairs, r, taken = index.apply(np.array([p[0] for p in rm], dtype=U), np.array([p[1] for p in rm], dtype=U),
                                      np.array([p[0] for p in ins], dtype=U), np.array([p[1] for p in ins], dtype=U))
        assert pairs.tolist() == [list(p) for p in sorted(set(before) - set(after))] and r == len(pairs)
        assert taken == len(set(after) - set(before))
        self.count["burst"] += 1

    def run(self, index, events: int = rc.HISTORY_EVENTS):
        self.scan(index)
        self.check(index, "first scan")
        for e in range(1, events):
            kind = ("scan", "delete", "change", "orphans", "burst")[int(self.rng.choice(5, p=[0.2, 0.2, 0.25, 0.15, 0.2]))]
            {"scan": self.scan, "delete": self.delete_file, "change": self.change_content,
             "orphans": self.remove_orphans, "burst": self.burst}[kind](index)
            self.check(index, (e, kind))
        return self.count


def check_apply_history_counts(total: dict):
    """Over rc.HISTORY_SEEDS: what wc.check_owner_history_counts asks, and bursts occurred, a
    burst dropped and re-added one pair, a change left the count of entries unchanged."""
    wc.check_owner_history_counts(total)
    assert all(total[k] > 0 for k in ("burst", "burst_drop_and_re_add", "change_kept_count")), total
