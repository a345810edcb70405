"""The Object index's owners mode (include/sd_cas.h: SD_OBJECT_INDEX_OWNERS) on a machine
without a GPU: the numpy mirrors (dedup.owners_*_host) and the library's host twin
(sd_cpu_object_index_create_ex and the sd_cpu_* calls in that mode) against a dict statement of
the header's semantics on seeded scripts and on the shapes of
tests/object_index_owners_cases.py; the histories under the owners-mode cycle of INTEGRATION.md
§6 (no DB query for owners) against oracle/identifier_spec.py; the shard union; the capacity
rule, which covers the link counts; the fence between the two modes; the stand-alone selftest."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from spacedrive_amd import dedup
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from spacedrive_amd.device import HostObjectIndex
from tests import object_index_cases as oc
from tests import object_index_owners_cases as wc
from tests import object_index_remove_cases as rc
from tests.test_object_index_remove import HostIndexR, MirrorIndexR
from tests.test_object_index_remove import run_script_against as run_first_mode_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64


class MirrorOwners:
    """The numpy mirrors of the owners mode behind the interface of the indexes under test."""

    def __init__(self, nparts=1, part=0):
        self.nparts, self.part = nparts, part
        self.keys, self.vals, self.cnt = np.zeros(0, U), np.zeros(0, U), np.zeros(0, U)

    def __len__(self):
        return len(self.keys)

    def insert(self, keys, ids):
        self.keys, self.vals, self.cnt, taken = dedup.owners_insert_host(self.keys, self.vals, self.cnt, keys, ids,
                                                                         self.nparts, self.part)
        return taken

    def remove(self, keys, ids=None):
        self.keys, self.vals, self.cnt, pairs = dedup.owners_remove_host(self.keys, self.vals, self.cnt, keys, ids)
        return pairs, len(pairs)

    def remove_objects(self, ids):
        self.keys, self.vals, self.cnt, pairs = dedup.owners_remove_objects_host(self.keys, self.vals, self.cnt, ids)
        return pairs, len(pairs)

    def links(self, keys, ids):
        return dedup.owners_links_host(self.keys, self.vals, self.cnt, keys, ids)

    def lookup(self, q):
        q = np.asarray(q, U)
        at = np.searchsorted(self.keys, q)  # the lower bound: a key's smallest Object id
        ok = at < len(self.keys)
        found = np.zeros(len(q), np.uint8)
        found[ok] = self.keys[at[ok]] == q[ok]
        ids = np.zeros(len(q), U)
        ids[found == 1] = self.vals[at[found == 1]]
        return ids, found

    def export_links(self):
        return self.keys, self.vals, self.cnt

    def scan(self, recs, chunk):
        r, rep, _ = dedup.group_host(recs)
        return (r,) + tuple(dedup.owners_indexed_host(r, rep, self.keys, self.vals, chunk))


class HostOwners(HostObjectIndex):
    def __init__(self, nparts=1, part=0):
        super().__init__(nparts, part, owners=True)

    def scan(self, recs, chunk):
        r, rep, _ = dedup.group_host(recs)
        return (r,) + tuple(self.owners(r, rep, chunk))


IMPLS = {"mirror": (MirrorOwners, MirrorIndexR), "sd_cpu": (HostOwners, HostIndexR)}  # (owners mode, first mode)


def apply(index, op):
    if op[0] == "expect_count":
        assert len(index) == op[1], op
        return None
    return getattr(index, op[0])(*op[1:])


def same_result(a, b) -> bool:
    if a is None or isinstance(a, int):
        return a == b
    return a[1] == b[1] and a[0].shape == b[0].shape and np.array_equal(a[0], b[0])


def same_scan(a, b) -> bool:
    return all(np.array_equal(np.asarray(x).view(U) if np.asarray(x).dtype.itemsize == 8 else x,
                              np.asarray(y).view(U) if np.asarray(y).dtype.itemsize == 8 else y) for x, y in zip(a, b))


def run_owner_script(name, script, make_a, make_b, probes=None, make_first=None):
    """Apply the script to two owners-mode indexes (a: the statement or the mirror).  After
    every operation the return values (the count created, or the dropped pairs in ascending
    (key, id) order and their count), export_links and the count are equal; with `probes`
    (keys, ids, records) so are links() and lookup(); with `make_first`, lookup and the owner
    rule of b equal those of a first-mode index built from the first owner of each of a's keys."""
    a, b = make_a(), make_b()
    for step, op in enumerate(script):
        ra, rb = apply(a, op), apply(b, op)
        assert same_result(ra, rb), (name, step, op[0])
        ea, eb = a.export_links(), b.export_links()
        assert len(a) == len(b) == len(eb[0]), (name, step)
        assert all(np.array_equal(x, y) for x, y in zip(ea, eb)), (name, step, op[0])
        k, v, c = eb
        assert np.all((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))) and np.all(c >= 1), (name, step)
        if op[0].startswith("remove"):
            pairs, r = rb
            assert pairs.shape == (r, 2) and not b.links(pairs[:, 0].copy(), pairs[:, 1].copy()).any(), (name, step)
        if probes is None:
            continue
        pk, pv, recs = probes
        assert np.array_equal(a.links(pk, pv), b.links(pk, pv)), (name, step, "links")
        la, lb = a.lookup(pk), b.lookup(pk)
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]), (name, step, "lookup")
        if make_first is not None and step % 4 == 3:
            first = make_first()
            fk, fv = a.lookup(np.unique(ea[0]))[0], np.unique(ea[0])
            assert first.insert(fv, fk) == len(fv)
            fl = first.lookup(pk)
            assert np.array_equal(fl[0], lb[0]) and np.array_equal(fl[1], lb[1]), (name, step, "first-mode lookup")
            assert same_scan(first.scan(recs, 7), b.scan(recs, 7)), (name, step, "first-mode owners")
            if hasattr(first, "close"):
                first.close()
    return a, b


def script_probes(seed):
    keys, ids = wc.pools(seed)
    pk = np.concatenate([np.repeat(keys, len(ids)), oc.random_keys(5, 77 + seed)])
    pv = np.concatenate([np.tile(ids, len(keys)), ids[:5]])
    return pk, pv, wc.scan_records(seed)


# ------------------------------------------------------------------ 1. the dict statement
def test_dict_statement_by_hand():
    """The rules of the header on a few pairs, written out.  This tests the dict statement that
    every other test compares with (tests/object_index_owners_cases.py), not the library."""
    d = wc.DictOwners()
    k = np.array([10, 10, 10, 20, 10, 30, 10], U)
    v = np.array([5, 3, 5, 1, 5, 0, 3], U)
    assert d.insert(k, v) == 4  # (10,3) (10,5) (20,1) (30,0): repeated pairs add up
    assert [a.tolist() for a in d.export_links()] == [[10, 10, 20, 30], [3, 5, 1, 0], [2, 3, 1, 1]]
    assert d.lookup(np.array([10, 20, 25], U))[0].tolist() == [3, 1, 0]  # the first owner: the smallest id
    # one link of (10,5), both of (10,3), three of (20,1) (more than held), a wrong id, an absent key
    pairs, r = d.remove(np.array([10, 10, 10, 20, 20, 20, 30, 40], U), np.array([5, 3, 3, 1, 1, 1, 9, 0], U))
    assert pairs.tolist() == [[10, 3], [20, 1]] and r == 2
    assert [a.tolist() for a in d.export_links()] == [[10, 30], [5, 0], [2, 1]]
    assert d.lookup(np.array([10], U))[0].tolist() == [5]  # the next owner became the answer
    assert d.insert(np.array([10, 10], U), np.array([7, 2], U)) == 2
    pairs, r = d.remove(np.array([10, 99], U), None)  # every entry of the key
    assert pairs.tolist() == [[10, 2], [10, 5], [10, 7]] and len(d) == 1
    pairs, r = d.remove_objects(np.array([0, 0, 4], U))  # whatever its links
    assert pairs.tolist() == [[30, 0]] and len(d) == 0


@pytest.mark.parametrize("impl", sorted(IMPLS))
@pytest.mark.parametrize("seed", wc.SCRIPT_SEEDS)
def test_seeded_scripts_equal_dict_statement(impl, seed):
    owners, first = IMPLS[impl]
    a, b = run_owner_script(seed, wc.seeded_script(seed), wc.DictOwners, owners, script_probes(seed), first)
    assert len(wc.seeded_script(seed)) == wc.SCRIPT_OPS


# ------------------------------------------------------------------ 2. histories
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_histories_never_ask_the_db_for_owners(impl):
    """rc.History's seeded events under the owners-mode cycle (wc.OwnersHistory: owners_of
    raises): after every event the entries equal the DB's link relation and the first owners
    equal truth(); over the seeds every outcome the mode exists for happened."""
    total = {}
    for seed in rc.HISTORY_SEEDS:
        for k, v in wc.OwnersHistory(seed).run(IMPLS[impl][0]()).items():
            total[k] = total.get(k, 0) + v
    print("history totals", total)
    wc.check_owner_history_counts(total)


def test_histories_on_the_dict_statement():
    """The statement itself reaches every outcome, so a shortfall elsewhere is a fault of the code.
    This tests the dict statement and the history's cycle, not the library."""
    class D(wc.DictOwners):
        def scan(self, recs, chunk):
            r, rep, _ = dedup.group_host(recs)
            t = self.first_owners()
            ks = np.array(sorted(t), dtype=U)
            return (r,) + tuple(dedup.owners_indexed_host(r, rep, ks, np.array([t[k] for k in sorted(t)], dtype=U), chunk))
    total = {}
    for seed in rc.HISTORY_SEEDS:
        for k, v in wc.OwnersHistory(seed).run(D()).items():
            total[k] = total.get(k, 0) + v
    wc.check_owner_history_counts(total)


# ------------------------------------------------------------------ 3. shapes
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_entry_counts_equal_dict_statement(impl):
    for n in wc.ENTRY_COUNTS:
        run_owner_script(n, wc.shape_script(n), wc.DictOwners, IMPLS[impl][0])
    assert [oc.dir_bits(n) for n in (15, 16, 17)] == [0, 1, 1]


def test_sd_cpu_large_shape_equals_mirror():
    _, b = run_owner_script("large", wc.shape_script(wc.LARGE), MirrorOwners, HostOwners)
    assert len(b) == wc.LARGE


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_runs_of_equal_keys(impl):
    """Two owners across positions 255 | 256; RUN owners of one key, removed by key at once."""
    make = IMPLS[impl][0]
    keys, ids, key = wc.straddle_case()
    script = [("insert", keys, ids), ("remove", np.array([key], U), np.array([10], U)), ("insert", keys, ids),
              ("remove", np.array([key], U), np.array([4], U)), ("remove", np.array([key, key], U), np.array([4, 10], U)),
              ("insert", keys, ids), ("remove", np.array([key], U), None)]
    _, b = run_owner_script("straddle", script, wc.DictOwners, make, (keys, ids, wc.scan_records(1)))
    assert len(b) == 598
    keys, ids, key, owners = wc.long_run_case()
    script = [("insert", keys, ids), ("remove", np.full(5, key, U), owners[:5].copy()),
              ("remove_objects", owners[100:110].copy()), ("insert", keys, ids),
              ("remove", np.array([key], U), None), ("expect_count", 2000), ("insert", keys, ids)]
    a, b = run_owner_script("long run", script, wc.DictOwners, make, (keys, ids, wc.scan_records(2)))
    assert b.lookup(np.array([key], U))[0].tolist() == [int(owners.min())]
    pairs, r = b.remove(np.array([key], U), None)
    assert r == wc.RUN and np.array_equal(pairs[:, 1], np.sort(owners))


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_insert_shapes(impl):
    """m = 1; COPIES copies of one pair give one entry with COPIES links; present and absent
    pairs shuffled in one batch; growth across two reallocations."""
    make = IMPLS[impl][0]
    x = make()
    one_k, one_v = np.array([oc.M64], U), np.array([0], U)
    assert x.insert(one_k, one_v) == 1 and x.insert(one_k, one_v) == 0
    assert [a.tolist() for a in x.export_links()] == [[oc.M64], [0], [2]]
    assert x.insert(np.full(wc.COPIES, 42, U), np.full(wc.COPIES, 9, U)) == 1
    assert [a.tolist() for a in x.export_links()] == [[42, oc.M64], [9, 0], [wc.COPIES, 2]]
    pairs, r = x.remove(np.full(wc.COPIES - 1, 42, U), np.full(wc.COPIES - 1, 9, U))
    assert r == 0 and x.links(np.array([42], U), np.array([9], U)).tolist() == [1]
    k, v = wc.shaped_pairs(1025)
    half = np.concatenate([k[::2], k[::2]]), np.concatenate([v[::2], v[::2]])
    mixed = np.argsort(oc.splitmix(3, 1025))
    script = [("insert",) + half, ("insert", k[mixed], v[mixed])] + [("insert", gk, gv) for gk, gv in wc.growth_steps()]
    run_owner_script("insert shapes", script, wc.DictOwners, make, (k, v, wc.scan_records(3)))


# ------------------------------------------------------------------ 4. shards
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_shard_union_is_the_unsharded_result(impl):
    """Every part of nparts 1, 2, 3, 8 is handed the same lists: the parts' entries, links and
    dropped pairs, concatenated in part order, are the unsharded index's."""
    make = IMPLS[impl][0]
    k, v, rk, rv, rids = wc.shard_case()
    for by in ("pairs", "keys", "objects"):
        def removal(x):
            return x.remove(rk, rv) if by == "pairs" else x.remove(rk, None) if by == "keys" else x.remove_objects(rids)
        whole = make()
        w_taken = whole.insert(k, v)
        w_pairs, w_r = removal(whole)
        w = whole.export_links()
        assert 0 < w_r < w_taken
        for nparts in oc.NPARTS:
            parts, ps, taken = [], [], 0
            for part in range(nparts):
                x = make(nparts, part)
                taken += x.insert(k, v)
                pairs, r = removal(x)
                assert r == len(pairs) and np.all(dedup.dest_of(pairs[:, 0].copy(), nparts) == part)
                parts.append(x.export_links()), ps.append(pairs)
            assert taken == w_taken, (by, nparts)
            for j in range(3):
                assert np.array_equal(np.concatenate([p[j] for p in parts]), w[j]), (by, nparts, j)
            assert np.array_equal(np.concatenate(ps), w_pairs), (by, nparts)


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("by", ["pairs", "keys", "objects"])
def test_capacity_short_by_one_changes_nothing_links_included(by):
    k, v, rk, rv, rids = wc.shard_case()
    x, m = HostOwners(), MirrorOwners()
    x.insert(k, v), m.insert(k, v)

    def removal(i, **kw):
        return i.remove(rk, rv, **kw) if by == "pairs" else i.remove(rk, None, **kw) if by == "keys" \
            else i.remove_objects(rids, **kw)
    before = [a.copy() for a in x.export_links()]
    want_pairs, want = removal(m)
    assert want > 1
    if by == "pairs":  # some survivor gives up a link: the refused call must not have taken it
        assert (dedup.owners_links_host(*before, m.keys, m.vals) > m.cnt).any()
    with pytest.raises(SdCasError) as e:
        removal(x, capacity=want - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == want
    assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))  # entries AND links
    # the raw call: nothing is written on the error; d_removed_out == NULL still reports *removed
    out = np.full((want + 3, 2), 0xA5A5A5A5A5A5A5A5, U)
    removed = ctypes.c_uint64(0)
    a = np.ascontiguousarray(rids if by == "objects" else rk)
    b = np.ascontiguousarray(rv)

    def call(outp, cap):
        if by == "objects":
            return lib().sd_cpu_object_index_remove_objects(x.handle, a.ctypes.data, a.size, outp, cap,
                                                            ctypes.byref(removed))
        return lib().sd_cpu_object_index_remove(x.handle, a.ctypes.data, b.ctypes.data if by == "pairs" else None,
                                                a.size, outp, cap, ctypes.byref(removed))
    assert call(out.ctypes.data, want - 1) == SD_ERR_CAPACITY and removed.value == want
    assert (out == U(0xA5A5A5A5A5A5A5A5)).all()
    assert all(np.array_equal(p, q) for p, q in zip(before, x.export_links()))
    removed.value = 0
    assert call(None, 0) == 0 and removed.value == want
    assert all(np.array_equal(p, q) for p, q in zip(m.export_links(), x.export_links()))


# ------------------------------------------------------------------ 5. the fence between the modes
def test_links_calls_refuse_a_first_mode_index():
    L = lib()
    x = HostObjectIndex()
    k = np.arange(3, dtype=U)
    x.insert(k, k)
    out = np.zeros(3, U)
    assert x.flags == 0 and HostOwners().flags == 1
    assert L.sd_cpu_object_index_links(x.handle, k.ctypes.data, k.ctypes.data, 3, out.ctypes.data) == -1
    assert L.sd_cpu_object_index_export_links(x.handle, out.ctypes.data, out.ctypes.data, out.ctypes.data, 3) == -1
    with pytest.raises(SdCasError):
        x.links(k, k)
    with pytest.raises(SdCasError):
        x.export_links()
    assert not out.any() and len(x) == 3


@pytest.mark.parametrize("case", sorted(rc.fixed_scripts()))
def test_create_ex_without_the_flag_is_create(case):
    """An index from create_ex(flags 0) equals one from create on the fixed removal scripts."""
    class ViaEx(HostIndexR):
        def __init__(self, nparts=1, part=0):
            self.nparts, self.part, self.owners_mode = nparts, part, False
            h = ctypes.c_void_p()
            assert lib().sd_cpu_object_index_create_ex(nparts, part, 0, ctypes.byref(h)) == 0
            self.handle = h
    _, b = run_first_mode_script(case, rc.fixed_scripts()[case], HostIndexR, ViaEx)
    assert b.flags == 0


def test_argument_checks_do_not_cross_the_boundary():
    """Null and invalid arguments: SD_ERR_INVALID, for the device entries before any HIP call."""
    L = lib()
    h = ctypes.c_void_p()
    f = ctypes.c_int(7)
    k = np.arange(3, dtype=U)
    assert L.sd_object_index_create_ex(None, 1, 0, 1, ctypes.byref(h)) == -1 and not h.value
    assert L.sd_object_index_flags(None, ctypes.byref(f)) == -1 and f.value == 7
    assert L.sd_object_index_links(None, None, None, None, 0, None, None) == -1
    assert L.sd_object_index_export_links(None, None, None, None, None, 0, None) == -1
    assert L.sd_cpu_object_index_create_ex(1, 0, 1, None) == -1
    assert L.sd_cpu_object_index_create_ex(1, 0, 2, ctypes.byref(h)) == -1  # an unknown flag
    assert L.sd_cpu_object_index_create_ex(0, 0, 1, ctypes.byref(h)) == -1
    assert L.sd_cpu_object_index_create_ex(3, 3, 1, ctypes.byref(h)) == -1
    assert L.sd_cpu_object_index_flags(None, ctypes.byref(f)) == -1
    assert L.sd_cpu_object_index_links(None, None, None, 0, None) == -1
    assert L.sd_cpu_object_index_export_links(None, None, None, None, 0) == -1
    x = HostOwners()
    x.insert(k, k)
    assert L.sd_cpu_object_index_flags(x.handle, None) == -1
    assert L.sd_cpu_object_index_links(x.handle, k.ctypes.data, None, 3, k.ctypes.data) == -1
    assert L.sd_cpu_object_index_links(x.handle, None, None, 0, None) == 0  # m == 0: a no-op
    assert L.sd_cpu_object_index_export_links(x.handle, None, None, None, 3) == -1
    out = np.zeros(3, U)
    assert L.sd_cpu_object_index_export_links(x.handle, out.ctypes.data, out.ctypes.data, out.ctypes.data, 2) == SD_ERR_CAPACITY
    assert not out.any() and len(x) == 3 and x.links(k, k).tolist() == [1, 1, 1]


def test_hex_calls_follow_the_mode():
    x, m = HostOwners(), MirrorOwners()
    keys = oc.random_keys(50, 81)
    ids = np.arange(50, dtype=U) % U(5)
    for i in (x, m):
        i.insert(keys, ids), i.insert(keys[:20], ids[:20])
    cas = ["%016x" % int(k) for k in keys[:30]]
    assert x.remove_hex(cas, ids[:30]) == m.remove(keys[:30], ids[:30])[1] == 10
    assert x.remove_hex(cas[:5]) == m.remove(keys[:5], None)[1] == 5
    assert all(np.array_equal(p, q) for p, q in zip(m.export_links(), x.export_links()))


# ------------------------------------------------------------------ 6. the selftest
def test_object_index_owners_selftest():
    """The stand-alone selftest of the host twin's owners mode (the dict statement in C++ on
    seeded scripts and on the shapes above, and concurrent reads between writes), plain build;
    `make sanitize-object-index-owners` runs it under ASan + UBSan and TSan
    (profiles/object_index/owners_sanitize_*.txt)."""
    b = subprocess.run(["make", "-C", CSRC, "-j8", "object-index-owners-selftest"], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "object_index_owners_selftest")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "object_index_owners_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
