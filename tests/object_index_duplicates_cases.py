"""Cases for the view by key of an owners-mode index (include/sd_cas.h:
sd_object_index_key_links, sd_object_index_duplicates, sd_object_index_duplicate_entries,
sd_object_index_duplicate_stats), shared by tests/test_object_index_duplicates.py (the numpy
mirror and the sd_cpu_* twin) and tests/test_gpu_object_index_duplicates.py (the kernels and the
device entries).  They build on tests/object_index_owners_cases.py and
tests/object_index_orphans_cases.py: the same shapes, pools and histories.  Every builder asserts
the premise it exists for (a run really crosses the border it is for), so a wrong edit cannot
quietly shrink a sweep.

An index under test offers what the orphans cases ask for, and
    key_links(keys) -> (links, owners)                                   uint64 [m]
    duplicates(min_links, min_owners) -> (keys, first, links, owners)    ascending keys
    duplicate_entries(min_links, min_owners) -> (keys, ids, links)       in (key, id) order
    duplicate_stats() -> uint64 [8]

Nothing here touches a device or the library.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from tests import object_index_cases as oc
from tests import object_index_orphans_cases as pc
from tests import object_index_owners_cases as wc
from tests.sliced_cases import BLOCKS, TILE, slice_len

U = np.uint64
M64 = oc.M64
E = pc.E
MIN_OWNERS = (0, 1, 2, wc.RUN, wc.RUN + 1)


def min_links_for(largest: int):
    """the thresholds on links(k) for an index whose largest links(k) is `largest`"""
    return (0, 1, 2, 3, largest, min(largest + 1, M64), M64)


class DictDuplicates(pc.DictOrphans):
    """The rule of object_index.h over the relation (key, id) -> links, as a dict group-by:
    owners(k) = the entries with key k, links(k) = the sum of their links, first(k) = the smallest
    id among them; k qualifies iff links(k) >= min_links and owners(k) >= min_owners, 0 meaning 1.
    The group-by is kept until the relation changes."""

    _g = None

    def insert(self, *a):
        self._g = None
        return super().insert(*a)

    def remove(self, *a):
        self._g = None
        return super().remove(*a)

    def remove_objects(self, *a):
        self._g = None
        return super().remove_objects(*a)

    def apply(self, *a):
        self._g = None
        return super().apply(*a)

    def _groups(self):
        if self._g is None:
            links, owners, first = Counter(), Counter(), {}
            for (k, o), c in self.d.items():
                links[k] += c
                owners[k] += 1
                first[k] = min(first.get(k, o), o)
            self._g = (links, owners, first)
        return self._g

    def _qualifying(self, min_links, min_owners):
        links, owners, _ = self._groups()
        return {k for k in links if links[k] >= max(min_links, 1) and owners[k] >= max(min_owners, 1)}

    def key_links(self, keys):
        links, owners, _ = self._groups()
        q = np.asarray(keys, U).tolist()
        return np.array([links[k] for k in q], dtype=U), np.array([owners[k] for k in q], dtype=U)

    def duplicates(self, min_links=0, min_owners=0):
        links, owners, first = self._groups()
        ks = sorted(self._qualifying(min_links, min_owners))
        return tuple(np.array([t[k] for k in ks], dtype=U) for t in ({k: k for k in ks}, first, links, owners))

    def duplicate_entries(self, min_links=0, min_owners=0):
        want = self._qualifying(min_links, min_owners)
        ps = sorted(p for p in self.d if p[0] in want)
        return (np.array([p[0] for p in ps], dtype=U), np.array([p[1] for p in ps], dtype=U),
                np.array([self.d[p] for p in ps], dtype=U))

    def duplicate_stats(self):
        links, owners, _ = self._groups()
        l2 = [k for k in links if links[k] >= 2]
        o2 = [k for k in links if owners[k] >= 2]
        return np.array([len(links), len(self.d), sum(links.values()), len(l2), sum(links[k] for k in l2), len(o2),
                         sum(owners[k] for k in o2), max(links.values(), default=0)], dtype=U)


# ------------------------------------------------------------------ the numpy mirror's reading
def mirror_view(export_links):
    """(keys, ids, links) of export_links -> the four answers' functions, through the host
    mirrors of spacedrive_amd.dedup (np.unique and np.add.reduceat): what a user does today."""
    from spacedrive_amd import dedup
    k, v, c = export_links
    return {"key_links": lambda q: dedup.owners_key_links_host(k, v, c, q),
            "duplicates": lambda ml=0, mo=0: dedup.owners_duplicates_host(k, v, c, ml, mo),
            "duplicate_entries": lambda ml=0, mo=0: dedup.owners_duplicate_entries_host(k, v, c, ml, mo),
            "duplicate_stats": lambda: dedup.owners_duplicate_stats_host(k, v, c)}


# ------------------------------------------------------------------ key lists
def key_lists(index_keys):
    """name -> query keys for an index that holds `index_keys` (with repeats for the owners): one
    list per count of oc.QUERY_COUNTS from oc.queries -- present keys, absent ones (key + 1,
    below the minimum, above the maximum, uniform misses) -- with the u64 edge keys and a key
    three times written over the head of the longer ones."""
    have = np.unique(np.asarray(index_keys, U))
    out = {}
    for m in oc.QUERY_COUNTS:
        q = oc.queries(have, m, seed=5 + m).copy()
        if m >= 63:
            e = oc.edge_keys()
            q[: len(e)] = e
            q[len(e): len(e) + 3] = have[len(have) // 2] if len(have) else U(9)
            q = q[np.argsort(oc.splitmix(m + 17, m))]
            present = np.isin(q, have)
            assert len(np.unique(q)) < m and {0, M64} <= set(q.tolist())
            assert len(have) == 0 or (present.any() and not present.all()), m
        out[f"m_{m}"] = q
    assert len(out) == len(oc.QUERY_COUNTS)
    return out


# ------------------------------------------------------------------ shapes
def shaped_case(n: int):
    """wc.ENTRY_COUNTS through wc.shaped_pairs: runs at both ends of the index, the edge keys 0
    and 2^64 - 1, a shared prefix; links 1 to 3 via shape_script's insert.  (insert keys, ids)."""
    op = wc.shape_script(n)[0]
    assert op[0] == "insert"
    if n >= 15:
        k, _ = wc.shaped_pairs(n)
        s = np.sort(k)
        assert s[0] == s[2] == 0 and s[-1] == s[-2] == U(M64)  # runs at both ends
    return op[1], op[2]


def straddle_case():
    """wc.straddle_case: the two owners of one key at positions 255 and 256."""
    keys, ids, key = wc.straddle_case()
    return keys, ids


def wave_straddle_case():
    """200 entries in which positions 63 and 64 -- the last lane of one wave, the first of the
    next -- are the two owners of one key."""
    ks = np.sort(oc.random_keys(199, 322))
    keys = np.concatenate([ks, ks[63:64]])
    ids = np.concatenate([np.full(199, 10, U), np.array([4], dtype=U)])
    o = np.lexsort((ids, keys))
    assert keys[o][63] == keys[o][64] == ks[63] and keys[o][62] != ks[63] != keys[o][65]
    return keys, ids


def border_runs_case():
    """wc.LARGE entries (a slice is two tiles) with runs placed on the workgroup-slice borders:
    one that crosses a border by three entries either side, one that ends exactly at a border,
    one that begins exactly at one, one of three slices' length and more (it covers three whole
    slices, so its partial sums combine across workgroups), and the index's last entries.
    Every third pair carries two links, every fifth three.  -> (insert keys, ids, the runs as
    (first position, length) in the index)."""
    n = wc.LARGE
    per = slice_len(n)
    assert per == 2 * TILE and n > BLOCKS * TILE
    s = np.sort(oc.random_keys(n, 4242))
    runs = [(100 * per - 3, 6), (300 * per - 5, 5), (400 * per, 4), (200 * per - 100, 3 * per + 150), (n - 70, 70)]
    for a, ln in runs:
        s[a:a + ln] = s[a]
    for a, ln in runs:  # the premise: each run is exactly there, and crosses what it is for
        assert (s[a:a + ln] == s[a]).all() and (a == 0 or s[a - 1] != s[a]) and (a + ln == n or s[a + ln] != s[a])
    a, ln = runs[0]
    assert a // per + 1 == (a + ln - 1) // per
    assert (runs[1][0] + runs[1][1]) % per == 0 and runs[2][0] % per == 0
    a, ln = runs[3]
    assert (a + ln - 1) // per - a // per == 4  # two partial slices around three whole ones
    ids = oc.splitmix(4243, n)  # distinct pairs: position i of the index is position i of s
    assert len(np.unique(ids)) == n
    j = np.arange(n)
    rep = 1 + (j % 3 == 0) + (j % 5 == 0)
    ik, iv = np.repeat(s, rep), np.repeat(ids, rep)
    sh = np.argsort(oc.splitmix(4244, len(ik)))
    return ik[sh], iv[sh], runs


def long_run_case():
    """wc.long_run_case: RUN owners of one key over about twelve slices of one tile."""
    keys, ids, key, owners = wc.long_run_case()
    n = len(keys)
    assert slice_len(n) == TILE and wc.RUN // TILE >= 11
    return keys, ids, key


def one_key_case():
    """1025 entries of one key (five workgroups, one group)."""
    return np.full(1025, 1 << 40, U), np.arange(1025, dtype=U) * U(3)


def distinct_keys_case():
    """1025 distinct keys: no duplicate at all."""
    k = oc.random_keys(1025, 4545)
    return k, oc.vals_for(k, 46)


def many_copies_case():
    """pc.many_copies_case: wc.COPIES links on one pair, beside a key with two owners."""
    k, v, _, _ = pc.many_copies_case()
    k = np.concatenate([k, np.array([43, 43], dtype=U)])
    v = np.concatenate([v, np.array([11, 12], dtype=U)])
    return k, v


def small_cases():
    """name -> (insert keys, ids): every case but the wc.LARGE one"""
    out = {f"n_{n}": shaped_case(n) for n in wc.ENTRY_COUNTS}
    out.update({"straddle_255_256": straddle_case(), "straddle_63_64": wave_straddle_case(),
                "long_run": long_run_case()[:2], "one_key_1025": one_key_case(),
                "distinct_1025": distinct_keys_case(), "many_copies": many_copies_case(), "empty": (E, E)})
    assert len(out) == len(wc.ENTRY_COUNTS) + 7
    return out


# ------------------------------------------------------------------ the check
def check_view(x, ref, what="", lists=None):
    """Every answer of the view by key of x equals ref's (the dict statement, or the numpy mirror
    as a dict of functions): duplicates and duplicate_entries under the full cross of thresholds,
    the stats and their identities, key_links for every key list."""
    r = ref if isinstance(ref, dict) else {n: getattr(ref, n) for n in ("key_links", "duplicates",
                                                                       "duplicate_entries", "duplicate_stats")}
    ek, ei, el = x.export_links()
    allk, allf, alll, allo = r["duplicates"](0, 0)
    largest = int(alll.max()) if len(alll) else 0
    for ml in min_links_for(largest):
        for mo in MIN_OWNERS:
            got, want = x.duplicates(ml, mo), r["duplicates"](ml, mo)
            assert len(got) == 4 and all(g.dtype == U and np.array_equal(g, w) for g, w in zip(got, want)), (what, ml, mo)
            assert np.all(got[0][1:] > got[0][:-1]), (what, ml, mo)
            ge, we = x.duplicate_entries(ml, mo), r["duplicate_entries"](ml, mo)
            assert len(ge) == 3 and all(g.dtype == U and np.array_equal(g, w) for g, w in zip(ge, we)), (what, ml, mo)
            assert len(ge[0]) == int(got[3].sum()) and int(ge[2].sum()) == int(got[2].sum()), (what, ml, mo)
    # (0, 0): every key, and the entries are export_links row for row
    ge = x.duplicate_entries(0, 0)
    assert np.array_equal(ge[0], ek) and np.array_equal(ge[1], ei) and np.array_equal(ge[2], el), what
    assert np.array_equal(allk, np.unique(ek)), what
    # above the largest: nothing
    assert len(x.duplicates(min(largest + 1, M64), 0)[0]) == 0 or largest == M64, what
    st = x.duplicate_stats()
    assert st.dtype == U and np.array_equal(st, r["duplicate_stats"]()), (what, st)
    s = [int(t) for t in st]
    assert s[0] == len(allk) and s[1] == len(ek) and s[2] == int(el.sum()) and s[7] == largest, what
    assert s[3] == len(x.duplicates(2, 0)[0]) and s[5] == len(x.duplicates(0, 2)[0]), what
    assert s[4] == int(x.duplicates(2, 0)[2].sum()) and s[6] == int(x.duplicates(0, 2)[3].sum()), what
    # surplus Objects are entries beyond the first of their key; redundant file_paths likewise
    assert s[1] - s[0] == s[6] - s[5] and s[2] - s[0] == s[4] - s[3] and s[2] >= s[1] >= s[0], what
    for name, q in (key_lists(ek) if lists is None else lists).items():
        gl, go = x.key_links(q)
        wl, wo = r["key_links"](q)
        assert gl.dtype == U and np.array_equal(gl, wl) and np.array_equal(go, wo), (what, name)
        assert np.array_equal(go > 0, np.isin(q, ek)), (what, name)


# ------------------------------------------------------------------ shards
def shard_case():
    """pairs of every shard of nparts 1, 2, 3, 8 with repeats and second owners"""
    k, v, _ = pc.shard_case()
    return k, v


# ------------------------------------------------------------------ histories
class DuplicatesHistory(pc.OrphansHistory):
    """pc.OrphansHistory, after every event of which duplicates(2, 0) and duplicates(0, 2) equal
    the group-by of the DB's (cas_id, Object) -> file_path count relation."""

    def __init__(self, seed: int):
        super().__init__(seed)
        self.count.update({"content_with_copies": 0, "content_split_over_objects": 0, "duplicates_checked": 0})

    def check(self, index, what):
        super().check(index, what)
        links, owners, first = Counter(), Counter(), {}
        for (k, o), c in self.relation().items():
            links[k] += c
            owners[k] += 1
            first[k] = min(first.get(k, o), o)
        for (ml, mo), name in (((2, 0), "content_with_copies"), ((0, 2), "content_split_over_objects")):
            ks = sorted(k for k in links if links[k] >= max(ml, 1) and owners[k] >= max(mo, 1))
            got = index.duplicates(ml, mo)
            assert got[0].tolist() == ks and got[1].tolist() == [first[k] for k in ks], (what, ml, mo)
            assert got[2].tolist() == [links[k] for k in ks] and got[3].tolist() == [owners[k] for k in ks], (what, ml, mo)
            self.count[name] += len(ks)
        self.count["duplicates_checked"] += 1


def check_duplicates_history_counts(total: dict):
    """Over rc.HISTORY_SEEDS: what the orphan cycle asks for, and both kinds of duplicate were
    there to be found."""
    pc.check_orphan_history_counts(total)
    assert total["duplicates_checked"] > 0 and total["content_with_copies"] > 0, total
    assert total["content_split_over_objects"] > 0, total
