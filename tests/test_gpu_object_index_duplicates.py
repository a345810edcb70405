"""sd_object_index_key_links, sd_object_index_duplicates, sd_object_index_duplicate_entries and
sd_object_index_duplicate_stats on the device (include/sd_cas.h; csrc/object_index.hip: the heads
of the runs of equal keys, a segmented sum per run, the selection compacted in order) -- run on
an MI355X: -m gpu.  Everything is bit-exact against the dict statement of object_index.h's rule
(tests/object_index_duplicates_cases.py) and the numpy mirror that
tests/test_object_index_duplicates.py pins to it.  Every output is written between 0xA5 guard
rows into pre-filled rows, so a write outside the rows a call owns, or a missing one, shows."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests import object_index_duplicates_cases as dc  # noqa: E402
from tests import object_index_owners_cases as wc  # noqa: E402
from tests import object_index_remove_cases as rc  # noqa: E402
from tests.test_gpu_object_index import Guarded, POISON, _run_ranks, dev, host_u64  # noqa: E402
from tests.test_gpu_object_index_orphans import DeviceOrphans  # noqa: E402
from tests.test_object_index_duplicates import MirrorDuplicates  # noqa: E402

U = np.uint64
E = dc.E
SLACK = 3  # rows of an output past the most a call can write


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


def stream():
    return torch.cuda.current_stream().cuda_stream


class DeviceDuplicates(DeviceOrphans):
    """DeviceOrphans with the view by key: the raw entries write into pre-filled rows between
    guard rows (the guards and the rows past the count must still hold the fill), and the
    wrappers of device.ObjectIndex must answer the same."""

    def key_links(self, q):
        q = np.asarray(q, U).reshape(-1)
        m = len(q)
        d = dev(q) if m else torch.empty(0, dtype=torch.int64, device="cuda")
        links, owners = Guarded(m + SLACK, 8, torch.int64), Guarded(m + SLACK, 8, torch.int64)
        assert lib().sd_object_index_key_links(self.ctx.handle, self.x.handle, d.data_ptr() if m else None, m,
                                               links.inner.data_ptr(), owners.inner.data_ptr(), stream()) == 0
        got = []
        for b in (links, owners):
            assert b.guards_intact() and (b.host()[m:] == POISON).all()
            got.append(b.host()[:m].view(U).reshape(-1).copy())
        wl, wo = self.x.key_links(d)
        assert np.array_equal(got[0], host_u64(wl)) and np.array_equal(got[1], host_u64(wo))
        return got[0], got[1]

    def _rows(self, fn, wrapper, ncols, ml, mo):
        count = ctypes.c_uint64(1 << 40)
        assert fn(self.ctx.handle, self.x.handle, ml, mo, *([None] * ncols), 0, ctypes.byref(count), stream()) == 0
        c = int(count.value)  # every output NULL: the call only counts
        assert c <= len(self)
        bufs = [Guarded(c + SLACK, 8, torch.int64) for _ in range(ncols)]
        count.value = 1 << 40
        assert fn(self.ctx.handle, self.x.handle, ml, mo, *(b.inner.data_ptr() for b in bufs), c, ctypes.byref(count),
                  stream()) == 0 and count.value == c
        got = []
        for b in bufs:
            a = b.host()
            assert b.guards_intact() and (a[c:] == POISON).all()
            got.append(a[:c].view(U).reshape(-1).copy())
        assert all(np.array_equal(g, host_u64(w)) for g, w in zip(got, wrapper(ml, mo)))
        return tuple(got)

    def duplicates(self, ml=0, mo=0):
        return self._rows(lib().sd_object_index_duplicates, self.x.duplicates, 4, ml, mo)

    def duplicate_entries(self, ml=0, mo=0):
        return self._rows(lib().sd_object_index_duplicate_entries, self.x.duplicate_entries, 3, ml, mo)

    def duplicate_stats(self):
        out = np.full(10, POISON, U)
        assert lib().sd_object_index_duplicate_stats(self.ctx.handle, self.x.handle, out[1:].ctypes.data, stream()) == 0
        assert out[0] == POISON and out[9] == POISON
        assert np.array_equal(out[1:9], self.x.duplicate_stats())
        return out[1:9].copy()


def built(ctx, k, v, nparts=1, part=0):
    """(device index, the dict statement) holding the same links"""
    x, d = DeviceDuplicates(ctx, nparts, part), dc.DictDuplicates(nparts, part)
    assert x.insert(k, v) == d.insert(k, v)
    return x, d


# ------------------------------------------------------------------ 1. the cases
def test_entry_counts_equal_dict_statement(ctx):
    """0, 1, 15/16/17, 255/256/257, 1023/1024/1025, 4097 entries through wc.shaped_pairs (runs at
    both ends of the index, the keys 0 and 2^64 - 1, a shared prefix, links 1 to 3): the full
    cross of thresholds, the stats, key_links of every query count."""
    for n in wc.ENTRY_COUNTS:
        x, d = built(ctx, *dc.shaped_case(n))
        assert len(x) == n
        dc.check_view(x, d, n)
        x.close()


def test_named_runs_equal_dict_statement(ctx):
    """The two owners of one key at positions 255/256 (two tiles) and 63/64 (two waves); RUN
    owners of one key over about twelve slices; 1025 entries of one key; 1025 distinct keys;
    70 000 links on one pair beside several owners; an empty index."""
    cases = dc.small_cases()
    for name in ("straddle_255_256", "straddle_63_64", "long_run", "one_key_1025", "distinct_1025", "many_copies",
                 "empty"):
        x, d = built(ctx, *cases[name])
        dc.check_view(x, d, name)
        x.close()
    keys, ids, key = dc.long_run_case()
    x, _ = built(ctx, keys, ids)
    assert [a.tolist() for a in x.duplicates(0, wc.RUN)] == [[int(key)], [int(ids[keys == key].min())], [wc.RUN], [wc.RUN]]
    assert [int(a[0]) for a in x.key_links(np.array([key], U))] == [wc.RUN, wc.RUN]
    x.close()


def test_border_runs_equal_mirror(ctx):
    """wc.LARGE entries (a slice is two tiles) with runs across, up to and from a workgroup-slice
    border, one of three slices' length and one at the index's end, against the numpy mirror
    (which the CPU suite pins to the dict statement on this case)."""
    k, v, runs = dc.border_runs_case()
    x, m = DeviceDuplicates(ctx), MirrorDuplicates()
    assert x.insert(k, v) == m.insert(k, v) == wc.LARGE
    dc.check_view(x, m, "border runs")
    got = x.duplicates(0, 4)
    assert got[3].tolist() == [ln for _, ln in sorted(runs)]
    # a key list in which the long run's key comes many times beside short runs
    ek = x.export_links()[0]
    q = np.concatenate([np.repeat(ek[runs[3][0]], 70), ek[::997], ek[[a for a, _ in runs]]])
    q = q[np.argsort(oc.splitmix(3, len(q)))]
    gl, go = x.key_links(q)
    wl, wo = m.key_links(q)
    assert np.array_equal(gl, wl) and np.array_equal(go, wo) and int((go == runs[3][1]).sum()) >= 71
    x.close()


# ------------------------------------------------------------------ 2. capacity and NULL outputs
def test_capacity_short_by_one_writes_nothing_and_null_outputs(ctx):
    k, v = dc.shard_case()
    x, d = built(ctx, k, v)
    L = lib()
    for entries, ncols, want in ((False, 4, d.duplicates(0, 2)), (True, 3, d.duplicate_entries(0, 2))):
        fn = L.sd_object_index_duplicate_entries if entries else L.sd_object_index_duplicates
        call = x.x.duplicate_entries if entries else x.x.duplicates
        n = len(want[0])
        assert n > 3
        outs = [Guarded(n + SLACK, 8, torch.int64) for _ in range(ncols)]
        with pytest.raises(SdCasError) as e:
            call(0, 2, out=tuple(o.inner for o in outs), capacity=n - 1)
        assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == n
        assert all((o._all() == POISON).all() for o in outs)  # nothing was written
        count = ctypes.c_uint64(0)
        # a single output given and a short capacity: still refused, nothing written
        assert fn(ctx.handle, x.x.handle, 0, 2, *([None] * (ncols - 1)), outs[-1].inner.data_ptr(), n - 1,
                  ctypes.byref(count), stream()) == SD_ERR_CAPACITY and count.value == n
        assert (outs[-1]._all() == POISON).all()
        got = call(0, 2, out=tuple(o.inner for o in outs), capacity=n)
        assert all(np.array_equal(host_u64(g), w) for g, w in zip(got, want))
        assert all(o.guards_intact() and (o.host()[n:] == POISON).all() for o in outs)
        # every combination of NULL outputs: the given ones are written, *count is the same
        for mask in range(1 << ncols):
            bufs = [Guarded(n + SLACK, 8, torch.int64) if (mask >> j) & 1 else None for j in range(ncols)]
            count.value = 1 << 40
            assert fn(ctx.handle, x.x.handle, 0, 2, *(None if b is None else b.inner.data_ptr() for b in bufs), n,
                      ctypes.byref(count), stream()) == 0 and count.value == n, mask
            for j, b in enumerate(bufs):
                if b is not None:
                    assert b.guards_intact() and (b.host()[n:] == POISON).all(), (mask, j)
                    assert np.array_equal(b.host()[:n].view(U).reshape(-1), want[j]), (mask, j)
        assert fn(ctx.handle, x.x.handle, 0, 2, *([None] * ncols), 0, None, stream()) == 0  # count may be NULL
    # either output of key_links may be NULL
    q = dc.key_lists(k)["m_257"]
    d_q = dev(q)
    for j in range(2):
        only = Guarded(len(q) + SLACK, 8, torch.int64)
        args = [None, None]
        args[j] = only.inner.data_ptr()
        assert L.sd_object_index_key_links(ctx.handle, x.x.handle, d_q.data_ptr(), len(q), *args, stream()) == 0
        assert only.guards_intact() and (only.host()[len(q):] == POISON).all()
        assert np.array_equal(only.host()[:len(q)].view(U).reshape(-1), d.key_links(q)[j])
    x.close()


# ------------------------------------------------------------------ 3. fences
def test_refusals_and_empty_inputs(ctx):
    first, x = ObjectIndex(ctx), DeviceDuplicates(ctx)
    k = dev(np.arange(1, 4, dtype=U))
    out = Guarded(8, 8, torch.int64)
    count = ctypes.c_uint64(9)
    host8 = np.full(8, 7, U)
    p, o, st = k.data_ptr(), out.inner.data_ptr(), stream()
    L = lib()
    try:
        first.insert(k, k), x.x.insert(k, k)
        c = ctypes.byref(count)
        # a first-mode index
        assert L.sd_object_index_key_links(ctx.handle, first.handle, p, 3, o, o, st) == -1
        assert L.sd_object_index_duplicates(ctx.handle, first.handle, 0, 0, o, o, o, o, 8, c, st) == -1
        assert L.sd_object_index_duplicate_entries(ctx.handle, first.handle, 0, 0, o, o, o, 8, c, st) == -1
        assert L.sd_object_index_duplicate_stats(ctx.handle, first.handle, host8.ctypes.data, st) == -1
        for call in (lambda: first.key_links(k), first.duplicates, first.duplicate_entries, first.duplicate_stats):
            with pytest.raises(SdCasError):
                call()
        # NULL d_keys with m > 0; an index of another context
        assert L.sd_object_index_key_links(ctx.handle, x.x.handle, None, 3, o, o, st) == -1
        from spacedrive_amd.device import Context
        other = Context(0)
        assert L.sd_object_index_key_links(other.handle, x.x.handle, p, 3, o, o, st) == -1
        assert L.sd_object_index_duplicates(other.handle, x.x.handle, 0, 0, o, o, o, o, 8, c, st) == -1
        assert L.sd_object_index_duplicate_entries(other.handle, x.x.handle, 0, 0, o, o, o, 8, c, st) == -1
        assert L.sd_object_index_duplicate_stats(other.handle, x.x.handle, host8.ctypes.data, st) == -1
        other.close()
        assert L.sd_object_index_duplicate_stats(ctx.handle, x.x.handle, None, st) == -1
        # m == 0: valid, nothing written
        assert L.sd_object_index_key_links(ctx.handle, x.x.handle, None, 0, o, o, st) == 0
        assert (out._all() == POISON).all()
        # an empty index: counts 0, stats all 0, nothing written; key_links answers 0 and 0
        y = DeviceDuplicates(ctx)
        assert L.sd_object_index_duplicates(ctx.handle, y.x.handle, 0, 0, o, o, o, o, 8, c, st) == 0 and count.value == 0
        count.value = 9
        assert L.sd_object_index_duplicate_entries(ctx.handle, y.x.handle, 0, 0, o, o, o, 8, c, st) == 0 and count.value == 0
        assert (out._all() == POISON).all()
        assert y.duplicate_stats().tolist() == [0] * 8
        assert [a.tolist() for a in y.key_links(np.array([7, 0], U))] == [[0, 0], [0, 0]]
        assert [len(a) for a in y.duplicates()] == [0] * 4 and [len(a) for a in y.duplicate_entries()] == [0] * 3
        y.close()
        assert len(x) == 3 and x.duplicate_stats().tolist() == [3, 3, 3, 0, 0, 0, 0, 1]
    finally:
        first.close(), x.close()


# ------------------------------------------------------------------ 4. stale scratch
def test_large_call_then_small_over_stale_scratch(ctx):
    """A by-Object call and the view of a 166 000-entry index, then small ones on that index (after
    most of it left) and on another, with the head positions, totals, flags and counts of the
    larger call stale and the buffers between tensors of random data."""
    junk = [torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda") for _ in range(3)]
    k = oc.random_keys(50_000, 51)
    k = np.concatenate([k, k, k[:50_000:3], k])
    v = np.arange(len(k), dtype=U) % U(40_000)
    big, bm = DeviceDuplicates(ctx), MirrorDuplicates()
    assert big.insert(k, v) == bm.insert(k, v)
    junk.append(torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda"))
    b = oc.random_keys(700, 52)
    b = np.concatenate([b, b[::2]])
    small, sm = DeviceDuplicates(ctx), MirrorDuplicates()
    small.insert(b, oc.vals_for(b, 53)), sm.insert(b, oc.vals_for(b, 53))
    few = {"few": np.concatenate([k[:5], np.array([0, dc.M64], U)])}
    ids = np.concatenate([np.arange(0, 60_000, dtype=U), oc.splitmix(54, 40_000)])
    # the by-Object call shares the scratch: its sorted ids and totals are stale under the view
    assert np.array_equal(big.orphans(ids), bm.orphans(ids))
    for t in ((0, 0), (2, 0), (0, 2)):
        assert all(np.array_equal(g, w) for g, w in zip(big.duplicates(*t), bm.duplicates(*t))), t
        assert all(np.array_equal(g, w) for g, w in zip(big.duplicate_entries(*t), bm.duplicate_entries(*t))), t
    assert np.array_equal(big.duplicate_stats(), bm.duplicate_stats())
    # most of the big index leaves: the next calls are small ones over the larger one's scratch
    gone = np.arange(0, 39_000, dtype=U)
    assert big.remove_objects(gone)[1] == bm.remove_objects(gone)[1]
    assert 1000 < len(big) < 6000
    for x, m, what in ((big, bm, "big, after the removal"), (small, sm, "small"), (big, bm, "big again")):
        junk.append(torch.randint(0, 255, (1 << 18,), dtype=torch.uint8, device="cuda"))
        assert np.array_equal(x.orphans(ids[:500]), m.orphans(ids[:500]))
        dc.check_view(x, m, what, lists=few if x is big else None)
    big.close(), small.close()


# ------------------------------------------------------------------ 5. shards
def test_three_in_process_ranks_concatenate(ctx):
    """Three ranks as threads of one process, each with its own context and its shard of the
    index, handed the same pairs at the same time: their rows concatenated in rank order are the
    unsharded answer, still ascending; the stats add up; key_links add up."""
    from spacedrive_amd.device import Context
    R = 3
    k, v = dc.shard_case()
    whole, d = built(ctx, k, v)
    q = dc.key_lists(k)["m_257"]
    want = {t: (whole.duplicates(*t), whole.duplicate_entries(*t)) for t in ((0, 0), (2, 0), (0, 2))}
    wst, wkl = whole.duplicate_stats(), whole.key_links(q)
    assert len(want[(0, 2)][0][0]) > 3
    ctxs = [Context(0) for _ in range(R)]
    idx = [ObjectIndex(ctxs[r], R, r, owners=True) for r in range(R)]
    d_k, d_v, d_q = dev(k), dev(v), dev(q)
    torch.cuda.synchronize()

    def rank(r):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            idx[r].insert(d_k, d_v)
            rows = {t: (tuple(host_u64(a) for a in idx[r].duplicates(*t)),
                        tuple(host_u64(a) for a in idx[r].duplicate_entries(*t))) for t in want}
            stats = idx[r].duplicate_stats()
            kl = tuple(host_u64(a) for a in idx[r].key_links(d_q))
            st.synchronize()
        return rows, stats, kl
    try:
        got = _run_ranks(R, rank)
        for t in want:
            for j in range(2):
                cat = dedup.combine_duplicates([g[0][t][j] for g in got])
                assert all(np.array_equal(a, w) for a, w in zip(cat, want[t][j])), (t, j)
        assert np.array_equal(dedup.combine_duplicate_stats([g[1] for g in got]), wst)
        gl, go = dedup.combine_key_links([g[2] for g in got])
        assert np.array_equal(gl, wkl[0]) and np.array_equal(go, wkl[1])
        assert sum(len(g[0][(0, 0)][0][0]) > 0 for g in got) > 1
    finally:
        for x in idx:
            x.close()
        for c in ctxs:
            c.close()
        whole.close()


# ------------------------------------------------------------------ 6. histories
def test_histories_keep_the_duplicate_groups(ctx):
    """dc.DuplicatesHistory on the device: after every event duplicates(2, 0) and duplicates(0, 2)
    equal the group-by of the DB's relation."""
    total = {}
    for seed in rc.HISTORY_SEEDS:
        x = DeviceDuplicates(ctx)
        for k, v in dc.DuplicatesHistory(seed).run(x).items():
            total[k] = total.get(k, 0) + v
        x.close()
    dc.check_duplicates_history_counts(total)
