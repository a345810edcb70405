"""sd_object_index_apply (include/sd_cas.h: the removal list, then the insertion list, of an
owners-mode index in one call) on a machine without a GPU: the numpy mirror
(dedup.owners_apply_host) and the library's host twin (sd_cpu_object_index_apply) against a
dict statement of the header's rule on seeded scripts and on the shapes of
tests/object_index_apply_cases.py, and against a twin index given remove then insert; the
capacity rule; the refusals; the shard union; the histories under the one-call cycle of
INTEGRATION.md §6; the stand-alone selftest."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from spacedrive_amd import dedup
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from spacedrive_amd.device import HostObjectIndex
from tests import object_index_apply_cases as ac
from tests import object_index_cases as oc
from tests import object_index_owners_cases as wc
from tests import object_index_remove_cases as rc
from tests.test_object_index_owners import HostOwners, MirrorOwners, script_probes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64
E = ac.E


class MirrorApply(MirrorOwners):
    def apply(self, rk, rv, ik, iv):
        self.keys, self.vals, self.cnt, pairs, taken = dedup.owners_apply_host(self.keys, self.vals, self.cnt, rk, rv,
                                                                               ik, iv, self.nparts, self.part)
        return pairs, len(pairs), taken


class HostApply(HostOwners):
    def apply(self, rk, rv, ik, iv, **kw):
        pairs, taken = HostObjectIndex.apply(self, rk, rv, ik, iv, **kw)
        return pairs, len(pairs), taken


IMPLS = {"mirror": MirrorApply, "sd_cpu": HostApply}


def do(index, op):
    if op[0] == "expect_count":
        assert len(index) == op[1], op
        return None
    return getattr(index, op[0])(*op[1:])


def do_two_calls(index, op):
    """the operation on a twin that has no apply: remove with ids, then insert"""
    if op[0] != "apply":
        return do(index, op)
    index.remove(op[1], op[2])
    index.insert(op[3], op[4])
    return None


def same(a, b) -> bool:
    if a is None or isinstance(a, int):
        return a == b
    return len(a) == len(b) and all(
        (x.shape == y.shape and np.array_equal(x, y)) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def exports_equal(a, b) -> bool:
    ea, eb = a.export_links(), b.export_links()
    return len(a) == len(b) == len(eb[0]) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(ea, eb))


def run_apply_script(name, script, make_a, make_b, probes=None, make_twin=None):
    """Apply the script to a (the statement or the mirror) and b.  After every operation the
    return values (for apply: the dropped pairs in ascending (key, id) order, their count and
    taken), export_links and the count are equal, the entries ascend strictly with links >= 1
    and no dropped pair is left; with `probes` (keys, ids) so are links() and lookup(); with
    `make_twin`, an index of b's kind given remove then insert exports the same arrays."""
    a, b = make_a(), make_b()
    t = make_twin() if make_twin is not None else None
    for step, op in enumerate(script):
        ra, rb = do(a, op), do(b, op)
        assert same(ra, rb), (name, step, op[0], ra, rb)
        assert exports_equal(a, b), (name, step, op[0])
        k, v, c = b.export_links()
        assert np.all((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (v[1:] > v[:-1]))) and np.all(c >= 1), (name, step)
        if op[0] == "apply":
            pairs, r, taken = rb
            assert pairs.shape == (r, 2) and not b.links(pairs[:, 0].copy(), pairs[:, 1].copy()).any(), (name, step)
        if t is not None:
            do_two_calls(t, op)
            assert exports_equal(t, b), (name, step, op[0], "remove then insert")
        if probes is not None:
            pk, pv = probes[:2]
            assert np.array_equal(a.links(pk, pv), b.links(pk, pv)), (name, step, "links")
            la, lb = a.lookup(pk), b.lookup(pk)
            assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]), (name, step, "lookup")
    return a, b


# ------------------------------------------------------------------ 1. the dict statement
def test_dict_statement_by_hand():
    """The rule of the header on a few pairs, written out.  This tests the dict statement that
    every other test compares with (tests/object_index_apply_cases.py), not the library."""
    d = ac.DictApply()
    assert d.insert(np.array([10, 10, 10, 20, 30, 30], U), np.array([5, 5, 3, 1, 0, 0], U)) == 4
    # (10,5) held 2: asked 1, added 0 -> 1.  (10,3) held 1: asked 1, added 2 -> stays with 2, in no report.
    # (20,1) held 1: asked 3 (more than held) -> leaves.  (30,0) held 2: asked 0, added 1 -> 3.
    # (40,7) absent: asked 1 is a no-op, added 1 -> enters.  (10,4): another id of a present key: a no-op.
    pairs, r, taken = d.apply(np.array([10, 10, 20, 20, 20, 40, 10], U), np.array([5, 3, 1, 1, 1, 7, 4], U),
                              np.array([10, 10, 30, 40], U), np.array([3, 3, 0, 7], U))
    assert pairs.tolist() == [[20, 1]] and r == 1 and taken == 1
    assert [a.tolist() for a in d.export_links()] == [[10, 10, 30, 40], [3, 5, 0, 7], [2, 1, 3, 1]]
    twin = wc.DictOwners()
    twin.insert(np.array([10, 10, 10, 20, 30, 30], U), np.array([5, 5, 3, 1, 0, 0], U))
    twin.remove(np.array([10, 10, 20, 20, 20, 40, 10], U), np.array([5, 3, 1, 1, 1, 7, 4], U))
    twin.insert(np.array([10, 10, 30, 40], U), np.array([3, 3, 0, 7], U))
    assert twin.d == d.d
    assert d.apply(E, E, E, E)[1:] == (0, 0) and len(d) == 4


@pytest.mark.parametrize("impl", sorted(IMPLS))
@pytest.mark.parametrize("seed", ac.APPLY_SEEDS)
def test_seeded_scripts_equal_dict_statement(impl, seed):
    script = ac.seeded_script(seed)
    assert len(script) == ac.APPLY_OPS and sum(op[0] == "apply" for op in script) >= 10
    run_apply_script(seed, script, ac.DictApply, IMPLS[impl], script_probes(seed), IMPLS[impl])


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_entry_counts_equal_dict_statement(impl):
    for n in wc.ENTRY_COUNTS:
        run_apply_script(n, ac.entry_count_script(n), ac.DictApply, IMPLS[impl], None, IMPLS[impl])


def test_sd_cpu_large_shape_equals_mirror():
    _, b = run_apply_script("large", ac.large_script(), MirrorApply, HostApply, None, HostApply)
    assert len(b) > wc.LARGE - wc.LARGE // 100


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_straddle_long_run_and_copies(impl):
    make = IMPLS[impl]
    keys, ids, key, scripts = ac.straddle_scripts()
    assert len(scripts) == 5
    for name, script in scripts.items():
        run_apply_script(name, script, ac.DictApply, make, (keys, ids), make)
    keys, ids, key, script = ac.long_run_script()
    _, b = run_apply_script("long run", script, ac.DictApply, make, (keys, ids), make)
    assert int(b.export_links()[2].max()) == 1
    # COPIES copies of one pair in each list: the pair stays, with COPIES links
    x = make()
    assert x.insert(np.array([42, 43], U), np.array([9, 9], U)) == 2
    many = np.full(wc.COPIES, 42, U), np.full(wc.COPIES, 9, U)
    pairs, r, taken = x.apply(*many, *many)
    assert (r, taken) == (0, 0) and [a.tolist() for a in x.export_links()] == [[42, 43], [9, 9], [wc.COPIES, 1]]
    pairs, r, taken = x.apply(*many, E, E)
    assert pairs.tolist() == [[42, 9]] and taken == 0 and len(x) == 1


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_directory_bits_and_growth(impl):
    run_apply_script("dir bits", ac.dir_bits_script(), ac.DictApply, IMPLS[impl], None, IMPLS[impl])
    run_apply_script("growth", ac.growth_script(), ac.DictApply, IMPLS[impl], None, IMPLS[impl])


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_nothing_leaves_or_enters_only_links_change(impl):
    build, rm, ins, (k, v, want) = ac.in_place_case()
    x = IMPLS[impl]()
    assert x.insert(*build) == 1025
    k0, v0, c0 = (a.copy() for a in x.export_links())
    assert (c0 == 3).all()
    pairs, r, taken = x.apply(*rm, *ins)
    k1, v1, c1 = x.export_links()
    assert (r, taken, len(pairs)) == (0, 0, 0) and np.array_equal(k0, k1) and np.array_equal(v0, v1)
    assert np.array_equal(x.links(k, v), want) and not np.array_equal(c0, c1)
    assert np.array_equal(x.lookup(k)[1], np.ones(1025, np.uint8))


# ------------------------------------------------------------------ 3. capacity
def capacity_case():
    """(build pairs, removal list, insertion list): entries that leave, entries that only change
    their count (both ways) and pairs that would enter."""
    k, v, rk, rv, _ = wc.shard_case()
    fk, fv = ac.fresh_pairs(40, 9, k, v)
    return (k, v), (rk, rv), (np.concatenate([fk, k[:50]]), np.concatenate([fv, v[:50]]))


def test_capacity_short_by_one_changes_nothing():
    build, rm, ins = capacity_case()
    x, m = HostApply(), MirrorApply()
    x.insert(*build), m.insert(*build)
    before = [a.copy() for a in x.export_links()]
    want_pairs, want, want_taken = m.apply(*rm, *ins)
    assert want > 1 and want_taken == 40
    held = dedup.owners_links_host(*before, m.keys, m.vals)
    assert ((held > m.cnt) & (held > 0)).any() and ((held < m.cnt) & (held > 0)).any()  # counts only, both ways
    with pytest.raises(SdCasError) as e:
        x.apply(*rm, *ins, capacity=want - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == want
    assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    # the raw call: nothing is written on the error; removed_out == NULL still reports
    out = np.full((want + 3, 2), 0xA5A5A5A5A5A5A5A5, U)
    removed, taken = ctypes.c_uint64(0), ctypes.c_uint64(7)
    arrs = [np.ascontiguousarray(a) for a in rm + ins]

    def call(outp, cap):
        return lib().sd_cpu_object_index_apply(x.handle, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[0].size,
                                               arrs[2].ctypes.data, arrs[3].ctypes.data, arrs[2].size, outp, cap,
                                               ctypes.byref(removed), ctypes.byref(taken))
    assert call(out.ctypes.data, want - 1) == SD_ERR_CAPACITY and removed.value == want and taken.value == 0
    assert (out == U(0xA5A5A5A5A5A5A5A5)).all()
    assert all(np.array_equal(p, q) for p, q in zip(before, x.export_links()))
    assert call(out.ctypes.data, want) == 0 and (removed.value, taken.value) == (want, want_taken)
    assert np.array_equal(out[:want], want_pairs) and (out[want:] == U(0xA5A5A5A5A5A5A5A5)).all()
    assert exports_equal(m, x)
    y = HostApply()
    y.insert(*build)
    assert lib().sd_cpu_object_index_apply(
        y.handle, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[0].size, arrs[2].ctypes.data, arrs[3].ctypes.data,
        arrs[2].size, None, 0, ctypes.byref(removed), None) == 0 and removed.value == want
    assert exports_equal(m, y)


# ------------------------------------------------------------------ 4. fences
def test_refusals_and_no_ops():
    L = lib()
    k = np.arange(1, 4, dtype=U)
    first = HostObjectIndex()
    first.insert(k, k)
    r, t = ctypes.c_uint64(9), ctypes.c_uint64(9)
    p = k.ctypes.data
    assert L.sd_cpu_object_index_apply(first.handle, p, p, 3, p, p, 3, None, 0, ctypes.byref(r), ctypes.byref(t)) == -1
    with pytest.raises(SdCasError):
        first.apply(k, k, k, k)
    assert len(first) == 3 and np.array_equal(first.export()[0], k)
    x = HostApply()
    x.insert(k, k)
    before = [a.copy() for a in x.export_links()]
    assert L.sd_cpu_object_index_apply(x.handle, p, None, 3, p, p, 3, None, 0, ctypes.byref(r), ctypes.byref(t)) == -1
    assert L.sd_cpu_object_index_apply(x.handle, None, p, 3, None, None, 0, None, 0, None, None) == -1
    assert L.sd_cpu_object_index_apply(x.handle, None, None, 0, p, None, 3, None, 0, None, None) == -1
    assert L.sd_cpu_object_index_apply(None, None, None, 0, None, None, 0, None, 0, None, None) == -1
    assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    # both lists empty: a no-op that reports zeros
    assert L.sd_cpu_object_index_apply(x.handle, None, None, 0, None, None, 0, None, 0, ctypes.byref(r),
                                       ctypes.byref(t)) == 0 and (r.value, t.value) == (0, 0)
    pairs, n_removed, n_taken = x.apply(E, E, E, E)
    assert (len(pairs), n_removed, n_taken) == (0, 0, 0) and len(x) == 3
    assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    # the device entries refuse null arguments before any HIP call
    assert L.sd_object_index_apply(None, None, None, None, 0, None, None, 0, None, 0, None, None, None) == -1
    assert L.sd_object_index_apply_hex(None, None, None, None, 0, None, None, 0, None, None) == -1


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_one_empty_list_is_insert_or_remove_on_a_twin(impl):
    k, v, rk, rv, _ = wc.shard_case()
    x, t = IMPLS[impl](), IMPLS[impl]()
    pairs, r, taken = x.apply(E, E, k, v)
    assert r == 0 and taken == t.insert(k, v) > 0 and exports_equal(t, x)
    pairs, r, taken = x.apply(rk, rv, E, E)
    t_pairs, t_r = t.remove(rk, rv)
    assert taken == 0 and r == t_r > 0 and np.array_equal(pairs, t_pairs) and exports_equal(t, x)


# ------------------------------------------------------------------ 5. shards
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_shard_union_is_the_unsharded_result(impl):
    """Every part of nparts 1, 2, 3, 8 is handed the same lists: the parts' entries, links and
    dropped pairs, concatenated in part order, and the sum of taken are the unsharded index's."""
    make = IMPLS[impl]
    build, rm, ins = capacity_case()
    whole = make()
    whole.insert(*build)
    w_pairs, w_r, w_taken = whole.apply(*rm, *ins)
    w = whole.export_links()
    assert w_r > 1 and w_taken == 40
    for nparts in oc.NPARTS:
        parts, ps, taken = [], [], 0
        for part in range(nparts):
            x = make(nparts, part)
            x.insert(*build)
            pairs, r, tk = x.apply(*rm, *ins)
            assert r == len(pairs) and np.all(dedup.dest_of(pairs[:, 0].copy(), nparts) == part)
            assert np.all(dedup.dest_of(x.export_links()[0].copy(), nparts) == part)
            parts.append(x.export_links()), ps.append(pairs)
            taken += tk
        assert taken == w_taken, nparts
        for j in range(3):
            assert np.array_equal(np.concatenate([p[j] for p in parts]), w[j]), (nparts, j)
        assert np.array_equal(np.concatenate(ps), w_pairs), nparts


# ------------------------------------------------------------------ 6. histories
def history_totals(make):
    total = {}
    for seed in rc.HISTORY_SEEDS:
        for k, v in ac.ApplyHistory(seed).run(make()).items():
            total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_histories_with_the_one_call_cycle(impl):
    """rc.History's seeded events under ac.ApplyHistory: a content change is one apply, a deleted
    file_path an apply with an empty insertion list, a burst one apply of the coalesced lists;
    after every event the entries equal the DB's link relation and the first owners truth()."""
    total = history_totals(IMPLS[impl])
    print("history totals", total)
    ac.check_apply_history_counts(total)


def test_histories_on_the_dict_statement():
    """The statement itself reaches every outcome, so a shortfall elsewhere is a fault of the
    code.  This tests the dict statement and the history's cycle, not the library."""
    class D(ac.DictApply):
        def scan(self, recs, chunk):
            r, rep, _ = dedup.group_host(recs)
            t = self.first_owners()
            return (r,) + tuple(dedup.owners_indexed_host(r, rep, np.array(sorted(t), dtype=U),
                                                          np.array([t[k] for k in sorted(t)], dtype=U), chunk))
    ac.check_apply_history_counts(history_totals(D))


# ------------------------------------------------------------------ 8. the selftest
def test_object_index_apply_selftest():
    """The stand-alone selftest of sd_cpu_object_index_apply (a (key, id) -> links model in C++
    on seeded scripts and shapes, against a twin given remove then insert), plain build; `make
    sanitize-object-index-apply` runs it under ASan + UBSan and TSan
    (profiles/object_index/apply_sanitize_*.txt)."""
    b = subprocess.run(["make", "-C", CSRC, "-j8", "object-index-apply-selftest"], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "object_index_apply_selftest")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "object_index_apply_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
