"""The Object index (include/sd_cas.h) on a machine without a GPU: the numpy mirrors
(dedup.owners_indexed_host / index_insert_host) and the library's host twin
(sd_cpu_object_index_*, sd_cpu_dedup_owners_indexed) against the literal restatement of
file_identifier/mod.rs:136-333 in oracle/identifier_spec.py, the insert semantics and key
edges on the case lists of tests/object_index_cases.py, the torch statement of the rule, and
the stand-alone selftest of the host code."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle.identifier_spec import _assign_step, identifier_replay
from spacedrive_amd import dedup
from spacedrive_amd.device import HostObjectIndex
from spacedrive_amd.identifier import object_owners_indexed
from tests import object_index_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64


def records_of(cas, base=0):
    """(key, global index) int64 records of the non-empty files, in file order."""
    rows = [(int(c, 16), base + i) for i, c in enumerate(cas) if c is not None]
    return np.array(rows, dtype=U).reshape(-1, 2).view(np.int64)


class MirrorIndex:
    """The numpy mirror behind the interface of HostObjectIndex."""

    def __init__(self, nparts=1, part=0):
        self.nparts, self.part = nparts, part
        self.keys, self.vals = np.zeros(0, U), np.zeros(0, U)

    def __len__(self):
        return len(self.keys)

    def insert(self, keys, vals):
        self.keys, self.vals, taken = dedup.index_insert_host(self.keys, self.vals, keys, vals, self.nparts, self.part)
        return taken

    def export(self):
        return self.keys, self.vals

    def lookup(self, q):
        q = np.asarray(q, U)
        at = np.searchsorted(self.keys, q)
        ok = at < len(self.keys)
        found = np.zeros(len(q), np.uint8)
        found[ok] = self.keys[at[ok]] == q[ok]
        ids = np.zeros(len(q), U)
        ids[found == 1] = self.vals[at[found == 1]]
        return ids, found

    def owners(self, records, rep, chunk_size=100):
        return dedup.owners_indexed_host(records, rep, self.keys, self.vals, chunk_size)


IMPLS = {"mirror": MirrorIndex, "sd_cpu": HostObjectIndex}


def scan(index, cas, base, chunk):
    """One scan of `cas` (file order, global indices from `base`) against `index`: the owner
    of every file (an Object id where `existing`, else a file index; an empty file owns
    itself), then the new heads inserted with Object id := the creator's global file index."""
    recs = records_of(cas, base)
    r, rep, _ = dedup.group_host(recs)
    owner, existing, new = index.owners(r, rep, chunk)
    out = np.arange(base, base + len(cas), dtype=U)
    if len(r):
        out[r[:, 1] - base] = owner
    if len(new):
        assert np.all(new[1:, 0] > new[:-1, 0])  # ascending keys, one per group
        assert index.insert(new[:, 0], new[:, 1]) == len(new)
    return out, existing, new


@pytest.mark.parametrize("impl", sorted(IMPLS))
@pytest.mark.parametrize("chunk", [1, 7, 100])
def test_two_scans_equal_one_replay(impl, chunk):
    """Scan A builds the index from its new heads; scan B's owners, taken through the index,
    equal identifier_replay(A + B)[len(A):] exactly -- with empty files, duplicates inside a
    chunk and across chunks and scans."""
    for trial, (na, nb) in enumerate([(3, 5), (10, 11), (40, 23)]):
        len_a, len_b = na * chunk, nb * chunk + (trial % 2) * (chunk // 2)
        cas = oc.scan_cas_ids(len_a + len_b, 100 * chunk + trial)
        assert None in cas or len(cas) < 20
        want, _ = identifier_replay(cas, chunk)
        index = IMPLS[impl]()
        got_a, ex_a, _ = scan(index, cas[:len_a], 0, chunk)
        assert not ex_a.any() and got_a.tolist() == want[:len_a]
        got_b, ex_b, _ = scan(index, cas[len_a:], len_a, chunk)
        assert got_b.tolist() == want[len_a:]
        if chunk > 1 and len_a >= 70:
            assert ex_b.any() and not ex_b.all()  # both branches of the rule ran
        # a third pass over B finds every group: nothing new, the same owners where they were links
        recs = records_of(cas[len_a:], len_a)
        r, rep, _ = dedup.group_host(recs)
        _, ex_c, new_c = index.owners(r, rep, chunk)
        assert ex_c.all() and len(new_c) == 0


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_prepopulated_objects_first_in_list_order_wins(impl):
    """Objects that own several cas_ids, two Objects owning the same cas_id: the step links to
    the first in list (DB) order -- _assign_step with `objects` / `obj_cas`."""
    rng = np.random.default_rng(5)
    for trial in range(20):
        pool = ["%016x" % int(x) for x in oc.splitmix(300 + trial, 30)]
        n_pre = int(rng.integers(1, 12))
        obj_cas = [set(rng.choice(pool[:20], size=int(rng.integers(1, 5)), replace=False).tolist())
                   for _ in range(n_pre)]
        objects = [[1000 + o] for o in range(n_pre)]
        n = int(rng.integers(1, 60))
        cas_of = [None if rng.random() < 0.1 else pool[int(rng.integers(0, 30))] for _ in range(n)]
        out = [-1] * n
        _assign_step(range(n), cas_of, [list(x) for x in objects], [set(s) for s in obj_cas], out)
        index = IMPLS[impl]()
        dump = [(int(c, 16), o) for o in range(n_pre) for c in sorted(obj_cas[o])]  # DB order: by Object
        index.insert(np.array([k for k, _ in dump], U), np.array([o for _, o in dump], U))
        assert len(index) == len(set().union(*obj_cas))
        r, rep, _ = dedup.group_host(records_of(cas_of))
        owner, existing, new = index.owners(r, rep, n)  # one step holds every file
        for j in range(len(r)):
            i = int(r[j, 1])
            if existing[j]:
                assert int(owner[j]) == out[i] < n_pre
            else:
                assert int(owner[j]) == i and out[i] >= n_pre  # a new Object of its own
        owned = set().union(*obj_cas)
        assert [int(k) for k in new[:, 0]] == sorted({int(c, 16) for c in cas_of if c is not None and c not in owned})


def model_insert(model: dict, keys, vals, nparts=1, part=0):
    taken = 0
    for k, v in zip(keys.tolist(), vals.tolist()):
        if int(dedup.dest_of(np.array([k], U), nparts)[0]) == part and k not in model:
            model[k] = v
            taken += 1
    return taken


@pytest.mark.parametrize("impl", sorted(IMPLS))
@pytest.mark.parametrize("case", sorted(oc.insert_cases()))
def test_insert_semantics(impl, case):
    """Keep first, against a dict: into an empty index, all present (the old value stays),
    duplicates in the input, below the minimum / above the maximum, three inserts across a
    growth and changes of the directory bits, the key edges, one bucket holding everything."""
    index, model = IMPLS[impl](), {}
    for keys, vals in oc.insert_cases()[case]:
        before = dict(model)
        assert index.insert(keys, vals) == model_insert(model, keys, vals)
        k, v = index.export()
        assert len(index) == len(model) == len(k)
        assert np.all(k[1:] > k[:-1])  # strictly ascending, unsigned
        assert dict(zip(k.tolist(), v.tolist())) == model
        assert all(model[x] == before[x] for x in before)  # an entry never changes
        ids, found = index.lookup(k)
        assert found.all() and np.array_equal(ids, v)  # the directory finds every key
        q = oc.queries(k, 257)
        ids, found = index.lookup(q)
        assert found.tolist() == [int(x in model) for x in q.tolist()]
        assert ids.tolist() == [model.get(x, 0) for x in q.tolist()]
    if case == "all_present":
        (k0, v0), _ = oc.insert_cases()[case]
        assert model == dict(zip(k0.tolist(), v0.tolist()))
    if case == "three_growth":
        assert [oc.dir_bits(n) for n in (10, 40, 240)] == [0, 2, 4]


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_shard_filter_union_is_the_unsharded_index(impl):
    keys = np.concatenate([oc.random_keys(500, 21), oc.edge_keys()])
    vals = oc.vals_for(keys, 22)
    whole = IMPLS[impl]()
    assert whole.insert(keys, vals) == len(keys)
    wk, wv = whole.export()
    for nparts in oc.NPARTS:
        got_k, got_v, total = [], [], 0
        for part in range(nparts):
            x = IMPLS[impl](nparts, part)
            taken = x.insert(keys, vals)
            k, v = x.export()
            assert taken == len(k) and np.all(dedup.dest_of(k, nparts) == part)
            got_k.append(k)
            got_v.append(v)
            total += taken
        assert total == len(keys)
        # the parts are contiguous prefix ranges: concatenated in order they are the whole index
        assert np.array_equal(np.concatenate(got_k), wk) and np.array_equal(np.concatenate(got_v), wv)


@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, 255, 256, 257, 4097])
def test_sd_cpu_lookup_sweep_equals_mirror(n):
    for name, keys in oc.key_sets(n).items():
        a, b = MirrorIndex(), HostObjectIndex()
        vals = oc.vals_for(keys, 31)
        assert a.insert(keys, vals) == b.insert(keys, vals) == n
        for m in oc.QUERY_COUNTS:
            q = oc.queries(keys, m)
            (ia, fa), (ib, fb) = a.lookup(q), b.lookup(q)
            assert np.array_equal(fa, fb) and np.array_equal(ia, ib), (name, n, m)


def test_torch_statement_equals_mirror():
    """identifier.object_owners_indexed (torch, keys in int64) == the numpy mirror, with keys
    on both sides of 2^63."""
    cas = oc.scan_cas_ids(900, 41)
    recs = records_of(cas)
    r, rep, _ = dedup.group_host(recs)
    known = np.unique(r[:, 0].view(U))[::2]
    keys = np.sort(np.concatenate([known, oc.edge_keys()]))
    vals = oc.vals_for(keys, 42)
    assert (keys >= U(1 << 63)).any() and (keys < U(1 << 63)).any()
    want, ex, _ = dedup.owners_indexed_host(r, rep, keys, vals, 7)
    t = torch.from_numpy
    got, gex = object_owners_indexed(t(r[:, 0].copy()), t(r[:, 1].copy()), t(rep.copy()), t(keys.view(np.int64)),
                                     t(vals.view(np.int64)), 7)
    assert np.array_equal(got.numpy().view(U), want) and np.array_equal(gex.numpy().astype(np.uint8), ex)
    assert ex.any() and not ex.all()


def test_argument_checks_do_not_cross_the_boundary():
    import ctypes
    from spacedrive_amd._native import lib
    h = ctypes.c_void_p()
    assert lib().sd_cpu_object_index_create(0, 0, ctypes.byref(h)) == -1
    assert lib().sd_cpu_object_index_create(2, 2, ctypes.byref(h)) == -1
    assert lib().sd_cpu_object_index_create(1, 0, None) == -1
    assert lib().sd_object_index_create(None, 1, 0, ctypes.byref(h)) == -1  # before any HIP call
    n = ctypes.c_uint64(7)
    assert lib().sd_object_index_count(None, ctypes.byref(n)) == -1
    assert lib().sd_object_index_lookup(None, None, None, 0, None, None, None) == -1
    assert lib().sd_dedup_owners_indexed(None, None, None, 0, None, 100, None, None, None, None, None) == -1
    x = HostObjectIndex()
    assert x.insert(np.zeros(0, U), np.zeros(0, U)) == 0 and len(x) == 0  # m == 0: a no-op
    owner, existing, new = x.owners(np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    assert len(owner) == len(existing) == len(new) == 0


def test_object_index_selftest():
    """The stand-alone selftest of the host code (policies, sd_cpu_object_index_*,
    sd_cpu_dedup_owners_indexed, concurrent lookups), plain build; `make
    sanitize-object-index` runs it under ASan + UBSan and TSan
    (profiles/object_index/sanitize_*.txt)."""
    b = subprocess.run(["make", "-C", CSRC, "-j8", "object-index-selftest"], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "object_index_selftest")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "object_index_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
