"""Removal from the Object index (include/sd_cas.h: sd_object_index_remove*,
sd_cpu_object_index_remove*) on a machine without a GPU: the numpy mirrors
(dedup.index_remove_host / index_remove_objects_host) against a dict statement of the
semantics, the library's host twin against the mirrors on every list of
tests/object_index_remove_cases.py, the histories (scans, deletions, content changes, orphan
removals under the host cycle of INTEGRATION.md §6) against oracle/identifier_spec.py, the
shard union, the capacity rule, the argument checks and the stand-alone selftest."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from spacedrive_amd import dedup
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from spacedrive_amd.device import HostObjectIndex
from tests import object_index_cases as oc
from tests import object_index_remove_cases as rc
from tests.test_object_index import MirrorIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64


class MirrorIndexR(MirrorIndex):
    """tests/test_object_index.py's mirror index with the removal mirrors."""

    def remove(self, keys, ids=None):
        self.keys, self.vals, pairs = dedup.index_remove_host(self.keys, self.vals, keys, ids)
        return pairs, len(pairs)

    def remove_objects(self, ids):
        self.keys, self.vals, pairs = dedup.index_remove_objects_host(self.keys, self.vals, ids)
        return pairs, len(pairs)

    def scan(self, recs, chunk):
        r, rep, _ = dedup.group_host(recs)
        return (r,) + tuple(self.owners(r, rep, chunk))


class HostIndexR(HostObjectIndex):
    def scan(self, recs, chunk):
        r, rep, _ = dedup.group_host(recs)
        return (r,) + tuple(self.owners(r, rep, chunk))


IMPLS = {"mirror": MirrorIndexR, "sd_cpu": HostIndexR}


# ------------------------------------------------------------------ the dict statement
class DictIndex:
    """The semantics of include/sd_cas.h word for word over a dict."""

    def __init__(self):
        self.d = {}

    def __len__(self):
        return len(self.d)

    def insert(self, keys, vals):
        taken = 0
        for k, v in zip(keys.tolist(), vals.tolist()):
            if k not in self.d:
                self.d[k] = v
                taken += 1
        return taken

    def _drop(self, gone):
        pairs = [(k, self.d.pop(k)) for k in sorted(gone)]
        return np.array(pairs, dtype=U).reshape(-1, 2), len(pairs)

    def remove(self, keys, ids=None):
        ks = keys.tolist()
        vs = [None] * len(ks) if ids is None else ids.tolist()
        return self._drop({k for k, v in zip(ks, vs) if k in self.d and (v is None or self.d[k] == v)})

    def remove_objects(self, ids):
        want = set(ids.tolist())
        return self._drop({k for k, v in self.d.items() if v in want})

    def export(self):
        ks = sorted(self.d)
        return np.array(ks, dtype=U), np.array([self.d[k] for k in ks], dtype=U)


def apply(index, op):
    """One operation of a script -> what it returns (None for the expectations)."""
    if op[0] == "insert":
        return index.insert(op[1], op[2])
    if op[0] == "remove":
        return index.remove(op[1], op[2])
    if op[0] == "remove_objects":
        return index.remove_objects(op[1])
    if op[0] == "expect_empty":
        assert len(index) == 0
    elif op[0] == "expect_count":
        assert len(index) == op[1]
    else:
        raise AssertionError(op[0])
    return None


def same_result(a, b) -> bool:
    if a is None or isinstance(a, int):
        return a == b
    return a[1] == b[1] and np.array_equal(a[0], b[0])


def run_script_against(name, script, make_a, make_b, lookups=True):
    """Apply the script to two indexes; after every operation the results (the count taken,
    or the dropped pairs in ascending key order and their count) and the exports are equal;
    after a removal every exported key is found and every dropped key is missed."""
    a, b = make_a(), make_b()
    for step, op in enumerate(script):
        ra, rb = apply(a, op), apply(b, op)
        assert same_result(ra, rb), (name, step, op[0])
        (ka, va), (kb, vb) = a.export(), b.export()
        assert len(a) == len(b) == len(ka), (name, step)
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), (name, step, op[0])
        assert np.all(kb[1:] > kb[:-1]), (name, step)
        if op[0].startswith("remove"):
            pairs, r = rb
            assert pairs.shape == (r, 2) and np.all(pairs[1:, 0] > pairs[:-1, 0]), (name, step)
            if lookups and hasattr(b, "lookup"):
                ids, found = b.lookup(kb)
                assert found.all() and np.array_equal(ids, vb), (name, step)
                ids, found = b.lookup(pairs[:, 0])
                assert not found.any() and not ids.any(), (name, step)
    return a, b


def small(scripts, limit=4097):
    """The scripts whose index has at most `limit` entries (the dict statement walks them in
    Python; the mirrors are vectorised and take no other path at a larger size)."""
    return [(n, s) for n, s in scripts if len(s[0][1]) <= limit]


# ------------------------------------------------------------------ mirrors == the dict statement
@pytest.mark.parametrize("kind", rc.KINDS)
def test_mirror_by_key_equals_dict_statement(kind):
    scripts = small(rc.by_key_scripts(kind))
    assert len(scripts) == 2 * (len(oc.INDEX_SIZES) - 1)
    for name, script in scripts:
        run_script_against(name, script, DictIndex, MirrorIndexR)


def test_mirror_by_object_and_fixed_equal_dict_statement():
    scripts = small(rc.by_object_scripts()) + list(rc.fixed_scripts().items())
    assert len(scripts) == len(oc.INDEX_SIZES) - 1 + 6
    for name, script in scripts:
        run_script_against(name, script, DictIndex, MirrorIndexR)


def test_mirror_statement_by_hand():
    """The rules of the header on six entries, written out."""
    k = np.array([10, 20, 30, 40, 50, 60], U)
    v = np.array([1, 2, 1, 3, 0, oc.M64], U)
    # by key: 20 unconditionally (twice), 30 with the wrong id, 40 wrongly then rightly, 45 absent
    nk, nv, gone = dedup.index_remove_host(k, v, np.array([20, 30, 40, 45, 40, 20], U), None)
    assert nk.tolist() == [10, 50, 60] and gone.tolist() == [[20, 2], [30, 1], [40, 3]]
    nk, nv, gone = dedup.index_remove_host(k, v, np.array([20, 30, 40, 45, 40, 20], U), np.array([2, 9, 9, 1, 3, 7], U))
    assert nk.tolist() == [10, 30, 50, 60] and nv.tolist() == [1, 1, 0, oc.M64]
    assert gone.tolist() == [[20, 2], [40, 3]]
    # by Object: 1 owns two keys; 0 and 2^64 - 1 are ids like any other; 7 owns nothing
    nk, nv, gone = dedup.index_remove_objects_host(k, v, np.array([1, 7, 1, 0], U))
    assert nk.tolist() == [20, 40, 60] and gone.tolist() == [[10, 1], [30, 1], [50, 0]]
    nk, nv, gone = dedup.index_remove_objects_host(k, v, np.array([oc.M64], U))
    assert nk.tolist() == [10, 20, 30, 40, 50] and gone.tolist() == [[60, oc.M64]]
    nk, nv, gone = dedup.index_remove_host(np.zeros(0, U), np.zeros(0, U), k, None)
    assert len(nk) == len(nv) == 0 and gone.shape == (0, 2)


# ------------------------------------------------------------------ sd_cpu_* == the mirrors
@pytest.mark.parametrize("kind", rc.KINDS)
def test_sd_cpu_by_key_equals_mirror(kind):
    for name, script in rc.by_key_scripts(kind):
        run_script_against(name, script, MirrorIndexR, HostIndexR)


def test_sd_cpu_by_object_equals_mirror():
    for name, script in rc.by_object_scripts():
        run_script_against(name, script, MirrorIndexR, HostIndexR)


@pytest.mark.parametrize("case", sorted(rc.fixed_scripts()))
def test_sd_cpu_fixed_cases_equal_mirror(case):
    run_script_against(case, rc.fixed_scripts()[case], MirrorIndexR, HostIndexR)


def test_sd_cpu_large_shape_equals_mirror():
    _, b = run_script_against("large", rc.large_script(), MirrorIndexR, HostIndexR)
    assert len(b) == 0


def test_sd_cpu_remove_hex():
    keys = oc.random_keys(300, 81)
    vals = oc.vals_for(keys, 82)
    x, m = HostIndexR(), MirrorIndexR()
    x.insert(keys, vals), m.insert(keys, vals)
    cas = ["%016x" % int(k) for k in keys[:100]]
    ids = vals[:100].copy()
    ids[::2] ^= U(1)
    assert x.remove_hex(cas, ids) == m.remove(keys[:100], ids)[1] == 50
    assert x.remove_hex(cas) == m.remove(keys[:100])[1] == 50
    assert np.array_equal(x.export()[0], m.keys) and np.array_equal(x.export()[1], m.vals)


# ------------------------------------------------------------------ histories
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_histories_equal_the_oracle(impl):
    """Seeded histories of >= 25 events under the host cycle: after every event the scan's
    owners equal _assign_step's and the exported index equals {cas_id -> first live owner};
    over the seeds every outcome the cycle exists for happened (rc.check_history_counts)."""
    total = {}
    for seed in rc.HISTORY_SEEDS:
        for k, v in rc.History(seed).run(IMPLS[impl]()).items():
            total[k] = total.get(k, 0) + v
    rc.check_history_counts(total)


# ------------------------------------------------------------------ shards
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_shard_union_is_the_unsharded_result(impl):
    """Every part of nparts 1, 2, 3, 8 is handed the same removal list: the parts' exports and
    dropped pairs, concatenated in part order, are the unsharded index's."""
    keys, vals, rk, rids = rc.shard_case()
    for by in ("key", "object"):
        whole = IMPLS[impl]()
        whole.insert(keys, vals)
        w_pairs, w_r = whole.remove(rk) if by == "key" else whole.remove_objects(rids)
        wk, wv = whole.export()
        assert 0 < w_r < len(keys)
        for nparts in oc.NPARTS:
            ks, vs, ps = [], [], []
            for part in range(nparts):
                x = IMPLS[impl](nparts, part)
                x.insert(keys, vals)
                pairs, r = x.remove(rk) if by == "key" else x.remove_objects(rids)
                k, v = x.export()
                assert r == len(pairs) and np.all(dedup.dest_of(pairs[:, 0].copy(), nparts) == part)
                ks.append(k), vs.append(v), ps.append(pairs)
            assert np.array_equal(np.concatenate(ks), wk) and np.array_equal(np.concatenate(vs), wv), (by, nparts)
            assert np.array_equal(np.concatenate(ps), w_pairs), (by, nparts)


# ------------------------------------------------------------------ capacity, arguments
@pytest.mark.parametrize("by", ["key", "object"])
def test_capacity_short_by_one_changes_nothing(by):
    keys, vals, rk, rids = rc.shard_case()
    x, m = HostIndexR(), MirrorIndexR()
    x.insert(keys, vals), m.insert(keys, vals)
    want_pairs, want = m.remove(rk) if by == "key" else m.remove_objects(rids)
    assert want > 1
    before = [a.copy() for a in x.export()]
    with pytest.raises(SdCasError) as e:
        x.remove(rk, capacity=want - 1) if by == "key" else x.remove_objects(rids, capacity=want - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == want
    assert len(x) == len(keys) and all(np.array_equal(a, b) for a, b in zip(before, x.export()))
    # the raw call: nothing is written on the error, and nothing past the count on success
    out = np.full((want + 3, 2), 0xA5A5A5A5A5A5A5A5, U)
    removed = ctypes.c_uint64(0)
    a = np.ascontiguousarray(rk if by == "key" else rids)

    def call(cap):
        if by == "key":
            return lib().sd_cpu_object_index_remove(x.handle, a.ctypes.data, None, a.size, out.ctypes.data, cap,
                                                    ctypes.byref(removed))
        return lib().sd_cpu_object_index_remove_objects(x.handle, a.ctypes.data, a.size, out.ctypes.data, cap,
                                                        ctypes.byref(removed))
    assert call(want - 1) == SD_ERR_CAPACITY and removed.value == want
    assert (out == U(0xA5A5A5A5A5A5A5A5)).all() and len(x) == len(keys)
    assert call(want) == 0 and removed.value == want
    assert np.array_equal(out[:want], want_pairs) and (out[want:] == U(0xA5A5A5A5A5A5A5A5)).all()
    assert np.array_equal(x.export()[0], m.keys) and np.array_equal(x.export()[1], m.vals)


def test_argument_checks_do_not_cross_the_boundary():
    """Null and invalid arguments: SD_ERR_INVALID, for the device entries before any HIP call
    (SD_ERR_DEVICE would come back from one where there is no device).  That an index of
    another context is refused needs two contexts: tests/test_gpu_object_index_remove.py."""
    L = lib()
    n = ctypes.c_uint64(7)
    k = np.arange(3, dtype=U)
    assert L.sd_object_index_remove(None, None, None, None, 0, None, 0, None, None) == -1
    assert L.sd_object_index_remove(None, None, k.ctypes.data, None, 3, None, 0, ctypes.byref(n), None) == -1
    assert L.sd_object_index_remove_objects(None, None, None, 0, None, 0, None, None) == -1
    assert L.sd_object_index_remove_objects(None, None, k.ctypes.data, 3, None, 0, ctypes.byref(n), None) == -1
    assert L.sd_object_index_remove_hex(None, None, None, None, 0, None) == -1
    assert n.value == 7
    assert L.sd_cpu_object_index_remove(None, None, None, 0, None, 0, None) == -1
    assert L.sd_cpu_object_index_remove_objects(None, None, 0, None, 0, None) == -1
    x = HostIndexR()
    x.insert(k, k)
    assert L.sd_cpu_object_index_remove(x.handle, None, None, 2, None, 0, ctypes.byref(n)) == -1
    assert L.sd_cpu_object_index_remove_objects(x.handle, None, 2, None, 0, ctypes.byref(n)) == -1
    assert len(x) == 3
    # m == 0 is a no-op; no output buffer and no count are needed
    assert L.sd_cpu_object_index_remove(x.handle, None, None, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert L.sd_cpu_object_index_remove(x.handle, k.ctypes.data, None, 3, None, 0, None) == 0 and len(x) == 0
    pairs, r = x.remove_objects(k)
    assert r == 0 and pairs.shape == (0, 2)
    assert x.insert(k, k) == 3  # insert works on an emptied index


def test_object_index_remove_selftest():
    """The stand-alone selftest of the host twin's removals (the case lists above in C++, and
    concurrent lookups between removals), plain build; `make sanitize-object-index-remove`
    runs it under ASan + UBSan and TSan (profiles/object_index/remove_sanitize_*.txt)."""
    b = subprocess.run(["make", "-C", CSRC, "-j8", "object-index-remove-selftest"], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "object_index_remove_selftest")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "object_index_remove_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
