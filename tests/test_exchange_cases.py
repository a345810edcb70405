"""The exchange cases of tests/exchange_cases.py without a device: the lists' own counts and
self-checks, the per-rank expectations against one grouping of the whole library and against the
oracle's restatement of identifier_job_step (oracle/identifier_spec.py, mod.rs:136-333) with
steps of 7, what a grouping that trusts the arrival order would get wrong on the unordered
layouts, and sd_split_range at the totals whose ranks go idle.  tests/test_gpu_exchange.py runs
the same lists through sd_cas_dedup_mgpu on in-process ranks."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.identifier_spec import identifier_replay
from spacedrive_amd._native import check, lib
from spacedrive_amd.dedup import group_host
from spacedrive_amd.identifier import object_owners
from tests import exchange_cases as xc

U = np.uint64


def test_lists_count_their_cases():
    """Every list built once: its own assertions run, and the counts the GPU module asserts after
    its loops are the ones stated here."""
    assert len(xc.specs()) == xc.CASE_COUNT == 85
    assert len({s.name for s in xc.specs()}) == 85
    ran = 0
    for R in xc.RANKS:
        order = xc.gpu_order(R)
        assert sorted(order, key=lambda s: s.name) == sorted(xc.specs(R), key=lambda s: s.name)
        assert len(order) == xc.CASES_PER_R[R] == {2: 23, 3: 29, 8: 33}[R]
        for s in order:
            c = xc.case(s)  # builds it: the self-checks of the case run
            assert c.R == R and len(c.want) == len(c.hashes) == len(c.valid) == R
            assert all(h.shape == (k, 32) for h, (_, k, _) in zip(c.hashes, c.shards))
            ran += 1
        assert len(xc.variant_specs(R)) == {2: 7, 3: 8, 8: 9}[R]
        assert len(xc.capacity_specs(R)) == 2 and len(xc.indexed_specs(R)) == (6 if R in (2, 8) else 3)
    assert ran == xc.CASE_COUNT
    assert len(xc.split_cases()) == 15
    assert {s.layout for s in xc.specs()} == set(xc.LAYOUTS) and {s.dist for s in xc.specs()} == set(xc.DISTS)
    assert all(s.n_files == (4363 if s.dist == "one_group" else 3001) for s in xc.specs())
    for R in xc.RANKS:  # the uneven shards come from the five sizes, all of them at R = 8
        head = [k for _, k, _ in xc.layout("uneven", R, xc.N_FILES)][:-1]
        assert set(head) <= set(xc.UNEVEN_SIZES) and (R < 8 or set(head) == set(xc.UNEVEN_SIZES))


def test_ranks_concatenated_are_one_grouping_of_the_library():
    """The destinations ascend with the key, so every case's per-rank records, representatives and
    owners, laid end to end in rank order, are group_host and the Object rule over all valid
    records at once."""
    n = 0
    for c in xc.all_cases():
        gr, grep, gng = group_host(c.all_recs)
        own = object_owners(torch.from_numpy(np.ascontiguousarray(gr[:, 1])), torch.from_numpy(grep), xc.CHUNK).numpy()
        assert np.array_equal(np.concatenate([w.records for w in c.want]), gr), c.name
        assert np.array_equal(np.concatenate([w.rep for w in c.want]), grep), c.name
        assert np.array_equal(np.concatenate([w.owner for w in c.want]), own), c.name
        assert sum(w.n_groups for w in c.want) == gng and sum(c.need) == len(gr), c.name
        # every record where dest_of sends it, by the integer rule
        for d, w in enumerate(c.want):
            lo, hi = xc.dest_range(d, c.R)
            k = np.ascontiguousarray(w.records[:, 0]).view(U)
            assert w.m == 0 or (lo <= int(k.min()) and int(k.max()) < hi), (c.name, d)
        n += 1
    assert n == xc.CASE_COUNT


def _owners_by_file(c: xc.Case) -> np.ndarray:
    """the owner of every file 0 .. N - 1: a file without a record (invalid: no cas_id) owns itself"""
    got = np.arange(c.spec.n_files)
    for w in c.want:
        got[w.records[:, 1]] = w.owner
    return got


@pytest.mark.parametrize("R", xc.RANKS)
def test_owners_vs_reference_replay(R):
    """For the layouts whose indices are 0 .. N - 1: the Objects the owners imply are the ones
    identifier_replay creates over the hex cas_ids in file order, None for an invalid file,
    chunk_size = 7 -- two files share an Object exactly when they share an owner, and the Object
    is named by the file that created it.  The GPU test's expectation is thereby the oracle's."""
    n = 0
    for c in xc.all_cases(R):
        if c.spec.layout == "high_base":
            continue
        cas = [None] * c.spec.n_files
        for r, (b, k, _) in enumerate(c.shards):
            ok = np.ones(k, bool) if c.valid[r] is None else c.valid[r].astype(bool)
            for i in np.flatnonzero(ok):
                cas[b + i] = c.keys[r][i].astype(">u8").tobytes().hex()
        want, stats = identifier_replay(cas, chunk_size=xc.CHUNK)
        got = _owners_by_file(c)
        assert got.tolist() == want, c.name
        assert len(stats) == -(-c.spec.n_files // xc.CHUNK)
        if c.spec.dist == "step_straddle":  # equal cas_ids inside one step: an Object each
            rep_of = {}
            for w in c.want:
                rep_of.update(zip(w.records[:, 1].tolist(), w.rep.tolist()))
            twins = [i for i, r in rep_of.items() if r != i and r // xc.CHUNK == i // xc.CHUNK]
            assert twins and all(got[i] == i for i in twins), c.name
        n += 1
    assert n == xc.CASES_PER_R[R] - sum(1 for s in xc.specs(R) if s.layout == "high_base")


def test_unordered_layouts_defeat_a_grouping_that_trusts_arrival():
    """The sensitivity of the sweep, stated without a device: were sd_cas_dedup_mgpu_indexed to
    pass SD_DEDUP_INDEX_SORTED whatever plan.ascending says, the radix path would keep equal keys
    in arrival order and take the first-arriving record's index as rep.  On the descending and the
    rotated layouts with uniform, step_straddle and one_group keys that differs from the expected
    rep on some rank -- and on every ascending layout it does not."""
    hit, miss = [], 0
    for c in xc.all_cases():
        differs = [d for d in range(c.R) if not np.array_equal(xc.rep_by_arrival(c.recv[d])[1], c.want[d].rep)]
        if c.ascending:
            assert not differs, c.name
            miss += 1
        elif c.spec.dist in xc.MUST_MISORDER:
            assert differs and sum(xc.first_not_smallest(x) for x in c.recv) >= 1, c.name
            hit.append(c.name)
    assert len(hit) == 16 and miss == xc.CASE_COUNT - 21  # 21 unordered cases, 16 of them must misorder
    assert {n.split("-")[0] for n in hit} == set(xc.UNORDERED)
    assert {n.split("-")[1] for n in hit} == set(xc.MUST_MISORDER)


def test_split_range_with_idle_ranks():
    """sd_split_range through the CPU library at the totals of the GPU split test: blocks fewer
    than ranks leave ranks with no bytes and no slots of their own, which still size the CV buffer
    as the others do."""
    n = 0
    for total, R, nb, q, cv_bytes, ranks in xc.split_cases():
        for r, (off, length, b0, b1) in enumerate(ranks):
            o, ln, cb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            check(lib().sd_split_range(total, R, r, ctypes.byref(o), ctypes.byref(ln), ctypes.byref(cb)))
            assert (o.value, ln.value, cb.value) == (off, length, cv_bytes), (total, R, r)
            assert (length == 0) == (b0 == b1 or total == 0)
        n += 1
    assert n == xc.SPLIT_CASES
