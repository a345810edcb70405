"""The view by Object of an owners-mode index (include/sd_cas.h: sd_object_index_object_links,
sd_object_index_orphans) on a machine without a GPU: the numpy mirror
(dedup.owners_object_links_host, dedup.owners_orphans_host) and the library's host twin
(sd_cpu_object_index_object_links, sd_cpu_object_index_orphans) against a dict statement of
object_index.h's rule on the shapes and id lists of tests/object_index_orphans_cases.py; the
capacity rule; the refusals; the shard sums and intersection; the histories under the orphan
cycle of INTEGRATION.md §6 (no DB scan for orphans); the stand-alone selftest."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from spacedrive_amd import dedup
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from spacedrive_amd.device import HostObjectIndex
from tests import object_index_cases as oc
from tests import object_index_orphans_cases as pc
from tests import object_index_owners_cases as wc
from tests import object_index_remove_cases as rc
from tests.test_object_index_apply import HostApply, MirrorApply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64
E = pc.E
FILL = U(0xA5A5A5A5A5A5A5A5)


class MirrorOrphans(MirrorApply):
    def object_links(self, ids, stride=1, m=None):
        return dedup.owners_object_links_host(self.vals, self.cnt, pc.listed(ids, stride, m))

    def orphans(self, ids, stride=1, m=None):
        return dedup.owners_orphans_host(self.vals, pc.listed(ids, stride, m))

    def apply_orphans(self, rk, rv, ik, iv):
        pairs, r, taken = self.apply(rk, rv, ik, iv)
        return pairs, r, taken, self.orphans(pairs[:, 1].copy())


class HostOrphans(HostApply):
    def apply_orphans(self, rk, rv, ik, iv):
        pairs, taken, orphans = HostObjectIndex.apply(self, rk, rv, ik, iv, orphans=True)
        return pairs, len(pairs), taken, orphans


IMPLS = {"mirror": MirrorOrphans, "sd_cpu": HostOrphans}


def built(make, k, v):
    """(index under test, the dict statement) holding the same links"""
    x, d = make(), pc.DictOrphans()
    assert x.insert(k, v) == d.insert(k, v)
    return x, d


# ------------------------------------------------------------------ 1. the dict statement
def test_dict_statement_by_hand():
    """The rule of object_index.h on a few pairs, written out.  This tests the dict statement
    that every other test compares with, not the library."""
    d = pc.DictOrphans()
    d.insert(np.array([10, 10, 10, 20, 30, 5], U), np.array([5, 5, 3, 5, 0, 1 << 63], U))
    links, entries = d.object_links(np.array([5, 3, 9, 5, 0, 10, 1 << 63], U))
    assert links.tolist() == [3, 1, 0, 3, 1, 0, 1] and entries.tolist() == [2, 1, 0, 2, 1, 0, 1]
    assert d.orphans(np.array([1 << 63, 9, (1 << 64) - 1, 10, 9, 5, 1], U)).tolist() == [1, 9, 10, (1 << 64) - 1]
    assert d.orphans(E).tolist() == [] and d.object_links(E)[0].tolist() == []
    # stride 2 over (key, id) rows: the id column
    rows = np.array([[10, 5], [20, 9], [30, 3]], U).reshape(-1)
    assert d.orphans(rows[1:], 2, 3).tolist() == [9] and d.object_links(rows[1:], 2, 3)[0].tolist() == [3, 0, 1]
    assert pc.DictOrphans().orphans(np.array([7, 7, 2], U)).tolist() == [2, 7]  # an empty index: all of them


# ------------------------------------------------------------------ 2. shapes and id lists
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_entry_counts_and_id_lists_equal_dict_statement(impl):
    """0, 1, 15/16/17, 255/256/257, 1023/1024/1025, 4097 entries (links 1 to 3), each with the
    eight id lists: empty, one id, repeats of one, all absent, all present, ids above 2^63, ids
    equal to key values, a shuffled mix."""
    for n in wc.ENTRY_COUNTS:
        op = wc.shape_script(n)[0]
        x, d = built(IMPLS[impl], op[1], op[2])
        assert len(x) == n
        pc.check_lists(x, d, pc.id_lists(*wc.shaped_pairs(n)), n)


def test_sd_cpu_large_shape_equals_mirror_and_dict():
    op = wc.shape_script(wc.LARGE)[0]
    x, d = built(HostOrphans, op[1], op[2])
    m = MirrorOrphans()
    m.insert(op[1], op[2])
    lists = pc.id_lists(*wc.shaped_pairs(wc.LARGE))
    pc.check_lists(x, d, lists, "large")
    pc.check_lists(m, d, lists, "large mirror")


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_one_owner_long_run_copies_and_threshold(impl):
    make = IMPLS[impl]
    k, v, ids = pc.one_owner_case()
    x, d = built(make, k, v)
    pc.check_lists(x, d, {"one owner": ids}, "one owner")
    assert x.object_links(ids)[1].tolist() == [1025, 0, 1025, 0]
    keys, vals, q = pc.long_run_lists()
    x, d = built(make, keys, vals)
    pc.check_lists(x, d, {"long run": q}, "long run")
    assert int((x.object_links(q)[1] == 1).sum()) == wc.RUN
    k, v, ids, (wl, we) = pc.many_copies_case()
    x, d = built(make, k, v)
    gl, ge = x.object_links(ids)
    assert np.array_equal(gl, wl) and np.array_equal(ge, we) and x.orphans(ids).tolist() == [11]
    pc.check_lists(x, d, {"copies": ids}, "copies")
    # every entry its own Object; lists of LDS_IDS - 1, LDS_IDS, LDS_IDS + 1 ids
    keys = oc.random_keys(4097, 77)
    vals = np.arange(4097, dtype=U) * U(3)
    x, d = built(make, keys, vals)
    pc.check_lists(x, d, pc.lds_lists(vals), "threshold")


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_stride_2_over_removed_rows(impl):
    pc.check_stride_2(IMPLS[impl](), pc.DictOrphans(), impl)


# ------------------------------------------------------------------ 3. capacity
def test_capacity_short_by_one_writes_nothing():
    k, v, ids = pc.shard_case()
    x, d = built(HostOrphans, k, v)
    want = d.orphans(ids)
    n = len(want)
    assert n > 3
    assert np.array_equal(x.orphans(ids, capacity=n), want)
    with pytest.raises(SdCasError) as e:
        x.orphans(ids, capacity=n - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == n
    out = np.full(n + 3, FILL, U)
    count = ctypes.c_uint64(0)
    q = np.ascontiguousarray(ids)
    L = lib()
    assert L.sd_cpu_object_index_orphans(x.handle, q.ctypes.data, 1, q.size, out.ctypes.data, n - 1,
                                         ctypes.byref(count)) == SD_ERR_CAPACITY
    assert count.value == n and (out == FILL).all()
    assert L.sd_cpu_object_index_orphans(x.handle, q.ctypes.data, 1, q.size, out.ctypes.data, n, ctypes.byref(count)) == 0
    assert count.value == n and np.array_equal(out[:n], want) and (out[n:] == FILL).all()
    # orphans_out == NULL still reports the count; either output of object_links may be NULL
    count.value = 0
    assert L.sd_cpu_object_index_orphans(x.handle, q.ctypes.data, 1, q.size, None, 0, ctypes.byref(count)) == 0
    assert count.value == n
    only = np.full(q.size, FILL, U)
    assert L.sd_cpu_object_index_object_links(x.handle, q.ctypes.data, 1, q.size, None, only.ctypes.data) == 0
    assert np.array_equal(only, d.object_links(ids)[1])
    assert L.sd_cpu_object_index_object_links(x.handle, q.ctypes.data, 1, q.size, only.ctypes.data, None) == 0
    assert np.array_equal(only, d.object_links(ids)[0])


# ------------------------------------------------------------------ 4. fences
def test_refusals_and_empty_inputs():
    L = lib()
    k = np.arange(1, 4, dtype=U)
    out = np.full(8, FILL, U)
    count = ctypes.c_uint64(9)
    p, o = k.ctypes.data, out.ctypes.data
    first = HostObjectIndex()
    first.insert(k, k)
    assert L.sd_cpu_object_index_object_links(first.handle, p, 1, 3, o, o) == -1  # a first-mode index
    assert L.sd_cpu_object_index_orphans(first.handle, p, 1, 3, o, 8, ctypes.byref(count)) == -1
    with pytest.raises(SdCasError):
        first.orphans(k)
    with pytest.raises(SdCasError):
        first.object_links(k)
    x = HostOrphans()
    x.insert(k, k)
    for stride in (0, 3, 4, 1 << 40):
        assert L.sd_cpu_object_index_object_links(x.handle, p, stride, 1, o, o) == -1, stride
        assert L.sd_cpu_object_index_orphans(x.handle, p, stride, 1, o, 8, ctypes.byref(count)) == -1, stride
    assert L.sd_cpu_object_index_orphans(x.handle, None, 1, 3, o, 8, ctypes.byref(count)) == -1
    assert L.sd_cpu_object_index_object_links(None, p, 1, 3, o, o) == -1
    assert (out == FILL).all()
    # m == 0: valid, count 0, nothing written
    assert L.sd_cpu_object_index_orphans(x.handle, None, 1, 0, o, 8, ctypes.byref(count)) == 0 and count.value == 0
    assert L.sd_cpu_object_index_object_links(x.handle, None, 2, 0, o, o) == 0 and (out == FILL).all()
    assert len(x.orphans(E)) == 0 and len(x.object_links(E)[0]) == 0
    # an empty index: every distinct id is an orphan
    y = HostOrphans()
    assert y.orphans(np.array([7, 7, 1 << 63, 2], U)).tolist() == [2, 7, 1 << 63]
    assert y.object_links(np.array([7, 2], U))[1].tolist() == [0, 0]
    # the device entries refuse null arguments before any HIP call
    assert L.sd_object_index_object_links(None, None, None, 1, 0, None, None, None) == -1
    assert L.sd_object_index_orphans(None, None, None, 1, 0, None, 0, None, None) == -1


# ------------------------------------------------------------------ 5. shards
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_shard_sums_and_intersection_are_the_unsharded_answer(impl):
    """Every part of nparts 1, 2, 3, 8 is handed the same pairs and the same ids: the parts'
    links and entries add up to the unsharded index's, and the intersection of their orphan
    lists is its orphan list (dedup.combine_object_links / combine_orphans)."""
    make = IMPLS[impl]
    k, v, ids = pc.shard_case()
    whole = make()
    whole.insert(k, v)
    wl, we = whole.object_links(ids)
    wo = whole.orphans(ids)
    assert 0 < len(wo) < len(np.unique(ids)) and int(we.max()) > 1
    for nparts in oc.NPARTS:
        parts = [make(nparts, part) for part in range(nparts)]
        for x in parts:
            x.insert(k, v)
        gl, ge = dedup.combine_object_links([x.object_links(ids) for x in parts])
        assert np.array_equal(gl, wl) and np.array_equal(ge, we), nparts
        lists = [x.orphans(ids) for x in parts]
        assert np.array_equal(dedup.combine_orphans(lists), wo), nparts
        if nparts > 1:
            assert any(len(p) > len(wo) for p in lists)  # a shard alone lists more than the whole


# ------------------------------------------------------------------ 6. histories
def history_totals(make):
    total = {}
    for seed in rc.HISTORY_SEEDS:
        for k, v in pc.OrphansHistory(seed).run(make()).items():
            total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_histories_with_the_orphan_cycle(impl):
    """pc.OrphansHistory: the Objects an orphan pass deletes come from the index's reports, the
    host's count of file_paths without a cas_id and sd_object_index_orphans alone, and equal the
    DB's Objects without a file_path after every pass."""
    total = history_totals(IMPLS[impl])
    print("history totals", total)
    pc.check_orphan_history_counts(total)


def test_histories_on_the_dict_statement():
    """The statement itself reaches every outcome, so a shortfall elsewhere is a fault of the
    code.  This tests the dict statement and the history's cycle, not the library."""
    class D(pc.DictOrphans):
        def scan(self, recs, chunk):
            r, rep, _ = dedup.group_host(recs)
            t = self.first_owners()
            return (r,) + tuple(dedup.owners_indexed_host(r, rep, np.array(sorted(t), dtype=U),
                                                          np.array([t[k] for k in sorted(t)], dtype=U), chunk))
    pc.check_orphan_history_counts(history_totals(D))


# ------------------------------------------------------------------ 7. the selftest
def test_object_index_orphans_selftest():
    """The stand-alone selftest of sd_cpu_object_index_object_links / _orphans (an Object ->
    (links, entries) model in C++ on seeded relations, strides, capacities and refusals, and
    concurrent reads), plain build; `make sanitize-object-index-orphans` runs it under ASan +
    UBSan and TSan (profiles/object_index/orphans_sanitize_*.txt)."""
    b = subprocess.run(["make", "-C", CSRC, "-j8", "object-index-orphans-selftest"], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "object_index_orphans_selftest")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "object_index_orphans_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
