"""The view by key of an owners-mode index (include/sd_cas.h: sd_object_index_key_links,
sd_object_index_duplicates, sd_object_index_duplicate_entries, sd_object_index_duplicate_stats)
on a machine without a GPU: the numpy mirror (dedup.owners_*_host: np.unique and
np.add.reduceat over export_links) and the library's host twin (sd_cpu_object_index_key_links,
_duplicates, _duplicate_entries, _duplicate_stats) against a dict statement of object_index.h's
rule on the cases of tests/object_index_duplicates_cases.py; the capacity rule; the refusals; the
shards' rows concatenated; the histories; the stand-alone selftest."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from spacedrive_amd import dedup
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from spacedrive_amd.device import HostObjectIndex
from tests import object_index_cases as oc
from tests import object_index_duplicates_cases as dc
from tests import object_index_owners_cases as wc
from tests import object_index_remove_cases as rc
from tests.test_object_index_orphans import HostOrphans, MirrorOrphans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64
E = dc.E
FILL = U(0xA5A5A5A5A5A5A5A5)


class MirrorDuplicates(MirrorOrphans):
    """the group-by a user of export_links runs on the host today"""

    def key_links(self, q):
        return dc.mirror_view(self.export_links())["key_links"](q)

    def duplicates(self, ml=0, mo=0):
        return dc.mirror_view(self.export_links())["duplicates"](ml, mo)

    def duplicate_entries(self, ml=0, mo=0):
        return dc.mirror_view(self.export_links())["duplicate_entries"](ml, mo)

    def duplicate_stats(self):
        return dc.mirror_view(self.export_links())["duplicate_stats"]()


class HostDuplicates(HostOrphans):
    pass  # device.HostObjectIndex has the four calls


IMPLS = {"mirror": MirrorDuplicates, "sd_cpu": HostDuplicates}


def built(make, k, v):
    """(index under test, the dict statement) holding the same links"""
    x, d = make(), dc.DictDuplicates()
    assert x.insert(k, v) == d.insert(k, v)
    return x, d


# ------------------------------------------------------------------ 1. the dict statement
def test_dict_statement_by_hand():
    """The rule of object_index.h on a few pairs, written out.  This tests the dict statement
    that every other test compares with, not the library."""
    d = dc.DictDuplicates()
    M = dc.M64
    #        key 10: owners 5 (2 links), 3 (1)   key 20: owner 5   key M: owners 1, 2   key 0: owner 9 (3 links)
    d.insert(np.array([10, 10, 10, 20, M, M, 0, 0, 0], U), np.array([5, 5, 3, 5, 2, 1, 9, 9, 9], U))
    assert [a.tolist() for a in d.duplicates()] == [[0, 10, 20, M], [9, 3, 5, 1], [3, 3, 1, 2], [1, 2, 1, 2]]
    assert [a.tolist() for a in d.duplicates(2, 0)] == [[0, 10, M], [9, 3, 1], [3, 3, 2], [1, 2, 2]]
    assert [a.tolist() for a in d.duplicates(0, 2)] == [[10, M], [3, 1], [3, 2], [2, 2]]
    assert [a.tolist() for a in d.duplicates(3, 2)] == [[10], [3], [3], [2]]
    assert d.duplicates(4, 0)[0].tolist() == [] and d.duplicates(0, 3)[0].tolist() == []
    assert [a.tolist() for a in d.duplicate_entries(0, 2)] == [[10, 10, M, M], [3, 5, 1, 2], [1, 2, 1, 1]]
    assert d.duplicate_stats().tolist() == [4, 6, 9, 3, 8, 2, 4, 3]
    links, owners = d.key_links(np.array([M, 11, 10, 10, 0], U))
    assert links.tolist() == [2, 0, 3, 3, 3] and owners.tolist() == [2, 0, 2, 2, 1]
    assert dc.DictDuplicates().duplicate_stats().tolist() == [0] * 8


# ------------------------------------------------------------------ 2. the cases
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_small_cases_equal_dict_statement(impl):
    """wc.ENTRY_COUNTS through wc.shaped_pairs, the owners at positions 255/256 and 63/64, RUN
    owners of one key, 1025 entries of one key, 1025 distinct keys, 70 000 links on one pair, an
    empty index: the full cross of thresholds, the stats, key_links of every query count."""
    for name, (k, v) in dc.small_cases().items():
        x, d = built(IMPLS[impl], k, v)
        dc.check_view(x, d, name)


def test_named_runs_are_found():
    """what each shape exists for, by hand"""
    x, _ = built(HostDuplicates, *dc.straddle_case())
    assert [a.tolist() for a in x.duplicates(0, 2)][1:] == [[4], [2], [2]]
    x, _ = built(HostDuplicates, *dc.wave_straddle_case())
    assert [a.tolist() for a in x.duplicates(0, 2)][1:] == [[4], [2], [2]]
    keys, ids, key = dc.long_run_case()
    x, _ = built(HostDuplicates, keys, ids)
    assert [a.tolist() for a in x.duplicates(0, wc.RUN)] == [[int(key)], [int(ids[keys == key].min())], [wc.RUN], [wc.RUN]]
    assert x.duplicates(0, wc.RUN + 1)[0].tolist() == []
    assert [int(a[0]) for a in x.key_links(np.array([key], U))] == [wc.RUN, wc.RUN]
    x, _ = built(HostDuplicates, *dc.one_key_case())
    assert x.duplicate_stats().tolist() == [1, 1025, 1025, 1, 1025, 1, 1025, 1025]
    x, _ = built(HostDuplicates, *dc.distinct_keys_case())
    assert x.duplicate_stats().tolist() == [1025, 1025, 1025, 0, 0, 0, 0, 1] and len(x.duplicates(2, 0)[0]) == 0
    x, _ = built(HostDuplicates, *dc.many_copies_case())
    assert [a.tolist() for a in x.duplicates(2, 0)] == [[42, 43], [9, 9], [wc.COPIES, 3], [1, 3]]


def test_border_runs_equal_mirror_and_dict():
    """wc.LARGE entries with runs on the workgroup-slice borders and one of three slices' length"""
    k, v, runs = dc.border_runs_case()
    x, d = built(HostDuplicates, k, v)
    m = MirrorDuplicates()
    m.insert(k, v)
    assert len(x) == wc.LARGE
    dc.check_view(x, d, "border runs")
    dc.check_view(m, d, "border runs, mirror", lists={})
    got = x.duplicates(0, 4)
    ek = x.export_links()[0]
    assert got[3].tolist() == [ln for _, ln in sorted(runs)]  # the placed runs, and no other
    assert got[0].tolist() == [int(ek[a]) for a, _ in sorted(runs)]


# ------------------------------------------------------------------ 3. capacity
def test_capacity_short_by_one_writes_nothing():
    k, v = dc.shard_case()
    x, d = built(HostDuplicates, k, v)
    L = lib()
    for entries, ncols, want in ((False, 4, d.duplicates(0, 2)), (True, 3, d.duplicate_entries(0, 2))):
        fn = L.sd_cpu_object_index_duplicate_entries if entries else L.sd_cpu_object_index_duplicates
        call = x.duplicate_entries if entries else x.duplicates
        n = len(want[0])
        assert n > 3
        assert all(np.array_equal(g, w) for g, w in zip(call(0, 2, capacity=n), want))
        with pytest.raises(SdCasError) as e:
            call(0, 2, capacity=n - 1)
        assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == n
        outs = [np.full(n + 3, FILL, U) for _ in range(ncols)]
        count = ctypes.c_uint64(0)
        assert fn(x.handle, 0, 2, *(o.ctypes.data for o in outs), n - 1, ctypes.byref(count)) == SD_ERR_CAPACITY
        assert count.value == n and all((o == FILL).all() for o in outs)
        # a single output given and a short capacity: still refused
        assert fn(x.handle, 0, 2, *([None] * (ncols - 1)), outs[-1].ctypes.data, n - 1,
                  ctypes.byref(count)) == SD_ERR_CAPACITY and (outs[-1] == FILL).all()
        assert fn(x.handle, 0, 2, *(o.ctypes.data for o in outs), n, ctypes.byref(count)) == 0 and count.value == n
        assert all(np.array_equal(o[:n], w) and (o[n:] == FILL).all() for o, w in zip(outs, want))
        # every output NULL: the call only counts, whatever the capacity; count may be NULL too
        count.value = 0
        assert fn(x.handle, 0, 2, *([None] * ncols), 0, ctypes.byref(count)) == 0 and count.value == n
        assert fn(x.handle, 0, 2, *([None] * ncols), 0, None) == 0
        # each output alone
        for j in range(ncols):
            one = np.full(n + 3, FILL, U)
            args = [None] * ncols
            args[j] = one.ctypes.data
            assert fn(x.handle, 0, 2, *args, n, ctypes.byref(count)) == 0
            assert np.array_equal(one[:n], want[j]) and (one[n:] == FILL).all(), (entries, j)


# ------------------------------------------------------------------ 4. fences
def test_refusals_and_empty_inputs():
    L = lib()
    k = np.arange(1, 4, dtype=U)
    out = np.full(8, FILL, U)
    count = ctypes.c_uint64(9)
    p, o = k.ctypes.data, out.ctypes.data
    first = HostObjectIndex()
    first.insert(k, k)
    assert L.sd_cpu_object_index_key_links(first.handle, p, 3, o, o) == -1  # a first-mode index
    assert L.sd_cpu_object_index_duplicates(first.handle, 0, 0, o, o, o, o, 8, ctypes.byref(count)) == -1
    assert L.sd_cpu_object_index_duplicate_entries(first.handle, 0, 0, o, o, o, 8, ctypes.byref(count)) == -1
    assert L.sd_cpu_object_index_duplicate_stats(first.handle, o) == -1
    for call in (lambda: first.key_links(k), first.duplicates, first.duplicate_entries, first.duplicate_stats):
        with pytest.raises(SdCasError):
            call()
    x = HostDuplicates()
    x.insert(k, k)
    assert L.sd_cpu_object_index_key_links(x.handle, None, 3, o, o) == -1
    assert L.sd_cpu_object_index_key_links(None, p, 3, o, o) == -1
    assert L.sd_cpu_object_index_duplicates(None, 0, 0, o, o, o, o, 8, ctypes.byref(count)) == -1
    assert L.sd_cpu_object_index_duplicate_entries(None, 0, 0, o, o, o, 8, ctypes.byref(count)) == -1
    assert L.sd_cpu_object_index_duplicate_stats(None, o) == -1
    assert L.sd_cpu_object_index_duplicate_stats(x.handle, None) == -1
    assert (out == FILL).all()
    # m == 0: valid, nothing written
    assert L.sd_cpu_object_index_key_links(x.handle, None, 0, o, o) == 0 and (out == FILL).all()
    assert len(x.key_links(E)[0]) == 0
    # either output of key_links may be NULL
    assert L.sd_cpu_object_index_key_links(x.handle, p, 3, None, o) == 0 and out[:3].tolist() == [1, 1, 1]
    # an empty index: counts 0, stats all 0, nothing written
    y = HostDuplicates()
    out[:] = FILL
    assert L.sd_cpu_object_index_duplicates(y.handle, 0, 0, o, o, o, o, 0, ctypes.byref(count)) == 0 and count.value == 0
    count.value = 9
    assert L.sd_cpu_object_index_duplicate_entries(y.handle, 0, 0, o, o, o, 0, ctypes.byref(count)) == 0
    assert count.value == 0 and (out == FILL).all()
    assert y.duplicate_stats().tolist() == [0] * 8
    assert [a.tolist() for a in y.key_links(np.array([7, 0], U))] == [[0, 0], [0, 0]]
    # the device entries refuse null arguments before any HIP call
    assert L.sd_object_index_key_links(None, None, None, 0, None, None, None) == -1
    assert L.sd_object_index_duplicates(None, None, 0, 0, None, None, None, None, 0, None, None) == -1
    assert L.sd_object_index_duplicate_entries(None, None, 0, 0, None, None, None, 0, None, None) == -1
    assert L.sd_object_index_duplicate_stats(None, None, None, None) == -1


# ------------------------------------------------------------------ 5. shards
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_shards_rows_concatenate_to_the_unsharded_answer(impl):
    """Every part of nparts 1, 2, 3, 8 is handed the same pairs: the parts' rows of duplicates and
    duplicate_entries concatenated in rank order are the unsharded index's, still ascending; the
    stats add up ([7] the maximum); key_links add up."""
    make = IMPLS[impl]
    k, v = dc.shard_case()
    whole = make()
    whole.insert(k, v)
    q = dc.key_lists(k)["m_257"]
    assert len(whole.duplicates(0, 2)[0]) > 3 and len(whole.duplicates(2, 0)[0]) > len(whole.duplicates(0, 2)[0])
    for nparts in oc.NPARTS:
        parts = [make(nparts, part) for part in range(nparts)]
        for x in parts:
            x.insert(k, v)
        for ml, mo in ((0, 0), (2, 0), (0, 2), (3, 2)):
            got = dedup.combine_duplicates([x.duplicates(ml, mo) for x in parts])
            assert all(np.array_equal(g, w) for g, w in zip(got, whole.duplicates(ml, mo))), (nparts, ml, mo)
            got = dedup.combine_duplicates([x.duplicate_entries(ml, mo) for x in parts])
            assert all(np.array_equal(g, w) for g, w in zip(got, whole.duplicate_entries(ml, mo))), (nparts, ml, mo)
        assert np.array_equal(dedup.combine_duplicate_stats([x.duplicate_stats() for x in parts]), whole.duplicate_stats())
        gl, go = dedup.combine_key_links([x.key_links(q) for x in parts])
        wl, wo = whole.key_links(q)
        assert np.array_equal(gl, wl) and np.array_equal(go, wo), nparts
        if nparts > 1:
            assert sum(len(x) > 0 for x in parts) > 1


# ------------------------------------------------------------------ 6. histories
def history_totals(make):
    total = {}
    for seed in rc.HISTORY_SEEDS:
        for k, v in dc.DuplicatesHistory(seed).run(make()).items():
            total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_histories_keep_the_duplicate_groups(impl):
    """dc.DuplicatesHistory: after every event duplicates(2, 0) and duplicates(0, 2) equal the
    group-by of the DB's relation."""
    total = history_totals(IMPLS[impl])
    print("history totals", total)
    dc.check_duplicates_history_counts(total)


# ------------------------------------------------------------------ 7. the selftest
def test_object_index_duplicates_selftest():
    """The stand-alone selftest of the sd_cpu_object_index_* view by key (a key -> (links,
    owners, first) model in C++ on seeded relations, thresholds, capacities and refusals, and
    concurrent reads), plain build; `make sanitize-object-index-duplicates` runs it under ASan +
    UBSan and TSan (profiles/object_index/duplicates_sanitize_*.txt)."""
    b = subprocess.run(["make", "-C", CSRC, "-j8", "object-index-duplicates-selftest"], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "object_index_duplicates_selftest")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "object_index_duplicates_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
