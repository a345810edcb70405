"""sd_object_index_object_links and sd_object_index_orphans on the device (include/sd_cas.h;
csrc/object_index.hip: the listed ids sorted and made distinct, one pass over the entries, the
totals scattered / the orphans compacted in order) -- run on an MI355X: -m gpu.  Everything is
bit-exact against the dict statement of object_index.h's rule
(tests/object_index_orphans_cases.py) and the numpy mirror that
tests/test_object_index_orphans.py pins to it.  Every output is written between 0xA5 guard rows
into pre-filled rows, so a write outside the rows a call owns, or a missing one, shows."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests import object_index_orphans_cases as pc  # noqa: E402
from tests import object_index_owners_cases as wc  # noqa: E402
from tests import object_index_remove_cases as rc  # noqa: E402
from tests.test_gpu_object_index import Guarded, POISON, _run_ranks, dev, host_u64  # noqa: E402
from tests.test_gpu_object_index_apply import DeviceApply  # noqa: E402
from tests.test_object_index_orphans import MirrorOrphans  # noqa: E402

U = np.uint64
E = pc.E
SLACK = 3  # elements of an output past the most a call can write


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


class DeviceOrphans(DeviceApply):
    """DeviceApply with the view by Object: the raw entries write into pre-filled rows between
    guard rows (the guards and the rows past the count must still hold the fill), and the
    wrappers of device.ObjectIndex must answer the same."""

    def _ids(self, ids, stride, m):
        ids = np.asarray(ids, U).reshape(-1)
        m = (len(ids) + stride - 1) // stride if m is None else m
        return dev(ids) if len(ids) else torch.empty(0, dtype=torch.int64, device="cuda"), m

    def object_links(self, ids, stride=1, m=None):
        d, m = self._ids(ids, stride, m)
        links, entries = Guarded(m + SLACK, 8, torch.int64), Guarded(m + SLACK, 8, torch.int64)
        assert lib().sd_object_index_object_links(self.ctx.handle, self.x.handle, d.data_ptr() if m else None, stride, m,
                                                  links.inner.data_ptr(), entries.inner.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream) == 0
        got = []
        for b in (links, entries):
            assert b.guards_intact() and (b.host()[m:] == POISON).all()
            got.append(b.host()[:m].view(U).reshape(-1).copy())
        wl, we = self.x.object_links(d, stride=stride, m=m)
        assert np.array_equal(got[0], host_u64(wl)) and np.array_equal(got[1], host_u64(we))
        return got[0], got[1]

    def orphans(self, ids, stride=1, m=None):
        d, m = self._ids(ids, stride, m)
        out = Guarded(m + SLACK, 8, torch.int64)
        count = ctypes.c_uint64(1 << 40)
        assert lib().sd_object_index_orphans(self.ctx.handle, self.x.handle, d.data_ptr() if m else None, stride, m,
                                             out.inner.data_ptr(), m, ctypes.byref(count),
                                             torch.cuda.current_stream().cuda_stream) == 0
        c = int(count.value)
        assert c <= m and out.guards_intact() and (out.host()[c:] == POISON).all()
        got = out.host()[:c].view(U).reshape(-1).copy()
        assert np.array_equal(got, host_u64(self.x.orphans(d, stride=stride, m=m)))
        return got

    def apply_orphans(self, rk, rv, ik, iv):
        pairs, taken, orphans = self.x.apply(*(dev(a) for a in (rk, rv, ik, iv)), orphans=True)
        return host_u64(pairs).reshape(-1, 2), int(pairs.shape[0]), taken, host_u64(orphans)


def built(ctx, k, v, nparts=1, part=0):
    """(device index, the dict statement, the mirror) holding the same links"""
    x, d, m = DeviceOrphans(ctx, nparts, part), pc.DictOrphans(nparts, part), MirrorOrphans(nparts, part)
    assert x.insert(k, v) == d.insert(k, v) == m.insert(k, v)
    return x, d, m


# ------------------------------------------------------------------ 1. shapes and id lists
def test_entry_counts_and_id_lists_equal_dict_statement(ctx):
    """0, 1, 15/16/17, 255/256/257, 1023/1024/1025, 4097 entries (links 1 to 3), each with the
    eight id lists: empty, one id, repeats of one, all absent, all present, ids above 2^63, ids
    equal to key values, a shuffled mix."""
    for n in wc.ENTRY_COUNTS:
        op = wc.shape_script(n)[0]
        x, d, m = built(ctx, op[1], op[2])
        assert len(x) == n
        lists = pc.id_lists(*wc.shaped_pairs(n))
        pc.check_lists(x, d, lists, n)
        pc.check_lists(x, m, lists, (n, "mirror"))
        x.close()


def test_large_shape_equals_mirror(ctx):
    """262 144 + 300 entries: a workgroup's slice of the pass over the entries is two tiles."""
    op = wc.shape_script(wc.LARGE)[0]
    x, m = DeviceOrphans(ctx), MirrorOrphans()
    assert x.insert(op[1], op[2]) == m.insert(op[1], op[2]) == wc.LARGE
    pc.check_lists(x, m, pc.id_lists(*wc.shaped_pairs(wc.LARGE)), "large")
    x.close()


def test_one_owner_long_run_copies_and_threshold(ctx):
    """One Object owning all 1025 entries (every lane of five workgroups adds to one slot); RUN
    owners of one key, all listed (more ids than the LDS holds); 70 000 copies of one pair;
    lists of OI_LDS_IDS - 1, OI_LDS_IDS and OI_LDS_IDS + 1 ids, and more ids than that of which
    fewer are distinct."""
    k, v, ids = pc.one_owner_case()
    x, d, _ = built(ctx, k, v)
    pc.check_lists(x, d, {"one owner": ids}, "one owner")
    assert x.object_links(ids)[1].tolist() == [1025, 0, 1025, 0]
    x.close()
    keys, vals, q = pc.long_run_lists()
    x, d, _ = built(ctx, keys, vals)
    pc.check_lists(x, d, {"long run": q}, "long run")
    x.close()
    k, v, ids, (wl, we) = pc.many_copies_case()
    x, d, _ = built(ctx, k, v)
    gl, ge = x.object_links(ids)
    assert np.array_equal(gl, wl) and np.array_equal(ge, we) and x.orphans(ids).tolist() == [11]
    x.close()
    keys = oc.random_keys(4097, 77)
    vals = np.arange(4097, dtype=U) * U(3)
    x, d, _ = built(ctx, keys, vals)
    pc.check_lists(x, d, pc.lds_lists(vals), "threshold")
    x.close()


def test_hot_slots_across_a_large_index(ctx):
    """wc.LARGE entries of which one Object owns every tenth and another every seventh, listed
    among 500 others: the totals of the two slots that most lanes add to, against the mirror."""
    k = oc.random_keys(wc.LARGE, 99)
    j = np.arange(wc.LARGE)
    v = np.where(j % 10 == 0, U(1 << 63), np.where(j % 7 == 0, U(3), oc.vals_for(k, 5) | U(1 << 20)))
    x, m = DeviceOrphans(ctx), MirrorOrphans()
    assert x.insert(k, v) == m.insert(k, v)
    ids = np.concatenate([np.array([3, 1 << 63, 4], dtype=U), v[1:1000:2], oc.splitmix(98, 10)])
    pc.check_lists(x, m, {"hot": ids, "hot and many": np.concatenate([ids, v[:3000]])}, "hot")
    assert int(x.object_links(ids[:2])[1].min()) > wc.LARGE // 12
    x.close()


def test_stride_2_over_removed_rows(ctx):
    x = DeviceOrphans(ctx)
    pc.check_stride_2(x, pc.DictOrphans(), "device")
    # and remove / remove_objects with orphans=True read their own d_removed_out the same way
    k, v, rk, rv = pc.removed_rows_case()
    y, d, _ = built(ctx, k, v)
    pairs, r, orphans = y.x.remove(dev(rk), dev(rv), orphans=True)
    want = d.apply_orphans(rk, rv, E, E)
    assert r == want[1] and np.array_equal(host_u64(pairs).reshape(-1, 2), want[0])
    assert np.array_equal(host_u64(orphans), want[3]) and len(want[3]) == 10
    ids = np.array([12, 35, 12, 999], dtype=U)
    pairs, r, orphans = y.x.remove_objects(dev(ids), orphans=True)
    assert r == 14 + 15 and host_u64(orphans).tolist() == [12, 35]  # the listed Objects that owned entries
    x.close(), y.close()


def test_large_call_then_small_over_stale_scratch(ctx):
    """A 150 000-id call, then small ones on that index and on another, with the sorted ids, the
    slots and the totals of the larger call stale and the buffers between tensors of random
    data."""
    junk = [torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda") for _ in range(3)]
    k = oc.random_keys(150_000, 51)
    v = np.arange(150_000, dtype=U) % U(50_000)
    big, bm = DeviceOrphans(ctx), MirrorOrphans()
    big.insert(k, v), bm.insert(k, v)
    junk.append(torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda"))
    b = oc.random_keys(700, 52)
    small, sm = DeviceOrphans(ctx), MirrorOrphans()
    small.insert(b, oc.vals_for(b, 53)), sm.insert(b, oc.vals_for(b, 53))
    many = np.concatenate([np.arange(0, 100_000, dtype=U), oc.splitmix(54, 50_000)])
    few = np.array([49_999, 50_000, 7, 7, 1 << 63], dtype=U)
    for x, m, ids in ((big, bm, many), (big, bm, few), (small, sm, oc.vals_for(b, 53)[:40]), (big, bm, E),
                      (big, bm, many[::-1].copy()), (small, sm, few), (big, bm, few[:1])):
        junk.append(torch.randint(0, 255, (1 << 18,), dtype=torch.uint8, device="cuda"))
        pc.check_lists(x, m, {"ids": ids}, len(ids))
    big.close(), small.close()


# ------------------------------------------------------------------ 2. capacity
def test_capacity_short_by_one_writes_nothing(ctx):
    k, v, ids = pc.shard_case()
    x, d, _ = built(ctx, k, v)
    want = d.orphans(ids)
    n = len(want)
    assert n > 3
    d_ids = dev(ids)
    out = Guarded(n + SLACK, 8, torch.int64)
    with pytest.raises(SdCasError) as e:
        x.x.orphans(d_ids, d_orphans_out=out.inner, capacity=n - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == n
    assert (out._all() == POISON).all()  # nothing was written
    got = x.x.orphans(d_ids, d_orphans_out=out.inner, capacity=n)
    assert np.array_equal(host_u64(got), want) and out.guards_intact() and (out.host()[n:] == POISON).all()
    # d_orphans_out == NULL still reports the count; either output of object_links may be NULL
    count = ctypes.c_uint64(0)
    st = torch.cuda.current_stream().cuda_stream
    assert lib().sd_object_index_orphans(ctx.handle, x.x.handle, d_ids.data_ptr(), 1, len(ids), None, 0,
                                         ctypes.byref(count), st) == 0 and count.value == n
    only = Guarded(len(ids), 8, torch.int64)
    assert lib().sd_object_index_object_links(ctx.handle, x.x.handle, d_ids.data_ptr(), 1, len(ids), None,
                                              only.inner.data_ptr(), st) == 0
    assert only.guards_intact() and np.array_equal(only.host().view(U).reshape(-1), d.object_links(ids)[1])
    x.close()


# ------------------------------------------------------------------ 3. fences
def test_refusals_and_empty_inputs(ctx):
    first, x = ObjectIndex(ctx), DeviceOrphans(ctx)
    k = dev(np.arange(1, 4, dtype=U))
    st = torch.cuda.current_stream().cuda_stream
    out = Guarded(8, 8, torch.int64)
    count = ctypes.c_uint64(9)
    p, o = k.data_ptr(), out.inner.data_ptr()
    L = lib()
    try:
        first.insert(k, k), x.x.insert(k, k)
        assert L.sd_object_index_object_links(ctx.handle, first.handle, p, 1, 3, o, o, st) == -1  # a first-mode index
        assert L.sd_object_index_orphans(ctx.handle, first.handle, p, 1, 3, o, 8, ctypes.byref(count), st) == -1
        with pytest.raises(SdCasError):
            first.orphans(k)
        for stride in (0, 3, 4, 1 << 40):
            assert L.sd_object_index_object_links(ctx.handle, x.x.handle, p, stride, 1, o, o, st) == -1, stride
            assert L.sd_object_index_orphans(ctx.handle, x.x.handle, p, stride, 1, o, 8, ctypes.byref(count), st) == -1
        assert L.sd_object_index_orphans(ctx.handle, x.x.handle, None, 1, 3, o, 8, ctypes.byref(count), st) == -1
        from spacedrive_amd.device import Context
        other = Context(0)
        assert L.sd_object_index_orphans(other.handle, x.x.handle, p, 1, 3, o, 8, ctypes.byref(count), st) == -1
        other.close()
        # m == 0: valid, count 0, nothing written
        assert L.sd_object_index_orphans(ctx.handle, x.x.handle, None, 1, 0, o, 8, ctypes.byref(count), st) == 0
        assert count.value == 0
        assert L.sd_object_index_object_links(ctx.handle, x.x.handle, None, 2, 0, o, o, st) == 0
        assert (out._all() == POISON).all()
        # an empty index: every distinct id is an orphan
        y = DeviceOrphans(ctx)
        assert y.orphans(np.array([7, 7, 1 << 63, 2], U)).tolist() == [2, 7, 1 << 63]
        assert y.object_links(np.array([7, 2], U))[1].tolist() == [0, 0]
        y.close()
        assert len(x) == 3 and x.orphans(np.array([3, 4], U)).tolist() == [4]
    finally:
        first.close(), x.close()


# ------------------------------------------------------------------ 4. shards
def test_three_in_process_ranks_sum_and_intersect(ctx):
    """Three ranks as threads of one process, each with its own context and its shard of the
    index, handed the same pairs and the same ids at the same time: the sums of their links and
    entries and the intersection of their orphan lists are the unsharded answer."""
    from spacedrive_amd.device import Context
    R = 3
    k, v, ids = pc.shard_case()
    whole, d, _ = built(ctx, k, v)
    wl, we = whole.object_links(ids)
    wo = whole.orphans(ids)
    assert np.array_equal(wo, d.orphans(ids)) and 0 < len(wo) < len(np.unique(ids))
    ctxs = [Context(0) for _ in range(R)]
    idx = [ObjectIndex(ctxs[r], R, r, owners=True) for r in range(R)]
    d_k, d_v, d_ids = dev(k), dev(v), dev(ids)
    torch.cuda.synchronize()

    def rank(r):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            idx[r].insert(d_k, d_v)
            links, entries = idx[r].object_links(d_ids)
            orphans = idx[r].orphans(d_ids)
            st.synchronize()
        return host_u64(links), host_u64(entries), host_u64(orphans)
    try:
        got = _run_ranks(R, rank)
        gl, ge = dedup.combine_object_links([g[:2] for g in got])
        assert np.array_equal(gl, wl) and np.array_equal(ge, we)
        assert np.array_equal(dedup.combine_orphans([g[2] for g in got]), wo)
        assert any(len(g[2]) > len(wo) for g in got)
    finally:
        for x in idx:
            x.close()
        for c in ctxs:
            c.close()
        whole.close()


# ------------------------------------------------------------------ 5. histories
def test_histories_with_the_orphan_cycle(ctx):
    """pc.OrphansHistory on the device: no DB query for owners and none for orphans; after every
    pass the Objects deleted equal the DB's Objects without a file_path, after every event
    object_links of the live Objects equals the relation's sums."""
    total = {}
    for seed in rc.HISTORY_SEEDS:
        x = DeviceOrphans(ctx)
        for k, v in pc.OrphansHistory(seed).run(x).items():
            total[k] = total.get(k, 0) + v
        x.close()
    pc.check_orphan_history_counts(total)
