"""sd_object_index_merge_objects on the device (include/sd_cas.h; csrc/object_index.hip: the map
sorted, one flagging pass over the entries, the leaving entries' rows sorted and coalesced by a
scan, one fused merge-compaction) -- run on an MI355X: -m gpu.  Everything is bit-exact against
the dict statement of object_index.h's rule (tests/object_index_merge_cases.py) and against a twin
device index built fresh from the statement's relation.  The map is handed over between 0xA5
guard rows and must come back as it went."""
import ctypes
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd._native import SdCasError, lib  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests import object_index_merge_cases as mc  # noqa: E402
from tests.test_gpu_object_index import Guarded, dev, host_u64  # noqa: E402
from tests.test_gpu_object_index_duplicates import DeviceDuplicates  # noqa: E402

U = np.uint64
M64 = oc.M64
E = mc.E
arr = mc.arr


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


def guarded_map(f, t):
    """the map on the device, each list between guard rows"""
    bufs = []
    for a in (f, t):
        g = Guarded(max(len(a), 1), 8, torch.int64)
        if len(a):
            g.inner[:len(a)].copy_(dev(np.asarray(a, U)))
        bufs.append(g)
    return bufs


class DeviceMerge(DeviceDuplicates):
    """DeviceDuplicates with merge_objects: the map lies between guard rows; the guards and the map
    itself must be as they were after the call."""

    def merge_objects(self, f, t):
        f, t = np.asarray(f, U).reshape(-1), np.asarray(t, U).reshape(-1)
        gf, gt = guarded_map(f, t)
        m = len(f)
        try:
            return self.x.merge_objects(gf.inner[:m], gt.inner[:m])
        finally:
            for g, a in ((gf, f), (gt, t)):
                assert g.guards_intact() and np.array_equal(g.host().view(U).reshape(-1)[:m], a)


def built(ctx, k, v, nparts=1, part=0):
    """(device index, the dict statement) holding the same links"""
    x, d = DeviceMerge(ctx, nparts, part), mc.DictMerge(nparts, part)
    assert x.insert(k, v) == d.insert(k, v)
    return x, d


def twin_of(ctx, nparts=1, part=0):
    return lambda: DeviceMerge(ctx, nparts, part)


# ------------------------------------------------------------------ 1. the dict statement
@pytest.mark.parametrize("seed", mc.MERGE_SEEDS)
def test_seeded_scripts_equal_dict_statement(ctx, seed):
    """merge_objects (several ids to one, swaps, cycles, chains, ids nobody holds, self maps,
    repeats, a contradiction) mixed with insert, the three removals, apply and the reads by Object
    and by key: after every operation the return values, export_links, links(), lookup and the
    count are the statement's and the arrays those of a fresh device index built from it."""
    made = []

    def make():
        made.append(DeviceMerge(ctx))
        return made[-1]
    try:
        mc.run_merge_script(seed, mc.seeded_script(seed), mc.DictMerge, make, mc.script_probes(seed), make)
    finally:
        for x in made:
            x.close()


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("n", mc.ENTRY_COUNTS)
def test_entry_counts(ctx, n):
    """0, 1, 255 / 256 / 257, 1000 and 262 144 entries (the last: 1024 slices of one tile)"""
    k, v, f, t = mc.counted_case(n)
    x, d = built(ctx, k, v)
    assert len(x) == n
    moved, coalesced = mc.check_merge(x, d, f, t, twin_of(ctx), None, n)
    assert (moved > 0) == (coalesced > 0) == (n >= 2)
    assert mc.check_merge(x, d, f[::-1].copy(), t[::-1].copy(), twin_of(ctx), None, (n, "again"))[0] <= moved
    x.close()


@pytest.mark.parametrize("size", mc.MAP_SIZES)
def test_map_sizes(ctx, size):
    """maps of 1, 255, 256, 257 rows and of 5000 with every pair named twice"""
    k, v, pool = mc.pool_case()
    x, d = built(ctx, k, v)
    f, t = mc.sized_map(pool, size)
    moved, coalesced = mc.check_merge(x, d, f, t, twin_of(ctx), None, size)
    assert moved > 0 and (size < 255 or coalesced > 0)
    x.close()


def test_map_contents_that_change_nothing(ctx):
    """`from` ids nobody holds, from == to, an empty map, an empty index: nothing moves and the
    arrays stand"""
    k, v, pool = mc.pool_case()
    x, d = built(ctx, k, v)
    before = x.export_links()
    absent = oc.splitmix(1, 40) | U(1 << 63)
    for f, t in ((absent, pool[:40]), (pool[:50].copy(), pool[:50].copy()), (E, E),
                 (np.concatenate([absent, pool[:5]]), np.concatenate([pool[:40], pool[:5]]))):
        assert mc.check_merge(x, d, f, t, None, None, "no-op") == (0, 0)
        assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    e = DeviceMerge(ctx)
    assert e.merge_objects(pool[:3], pool[3:6]) == (0, 0) and len(e) == 0
    x.close(), e.close()


@pytest.mark.parametrize("case", ["tile", "slice"])
def test_runs_across_a_border(ctx, case):
    """one key's six owners across positions 255 | 256 (two tiles) and, at 262 401 entries, across
    511 | 512 (two slices): leaving entries on both sides coalesce to one id inside the run, below
    every id of it (the key's first owner changes: lookup) and above; then every other entry moves"""
    keys, ids, key = mc.tile_straddle_case() if case == "tile" else mc.slice_straddle_case()
    d0 = mc.DictMerge()
    d0.insert(keys, ids)
    maps = dict(mc.run_maps(), every_other_entry=(arr(10), arr(11)))
    for name in maps if case == "tile" else ("to_lowest_in_run", "to_absent_below", "to_absent_above", "every_other_entry"):
        f, t = maps[name]
        x, d = DeviceMerge(ctx), mc.DictMerge()
        x.insert(keys, ids)
        d.d = dict(d0.d)
        if name == "every_other_entry":
            assert mc.check_merge(x, d, f, t, twin_of(ctx), None, (case, name)) == (len(keys) - 6, 0)
        else:
            assert mc.check_merge(x, d, f, t, twin_of(ctx), None, (case, name)) == (len(f), 5)
            assert int(x.lookup(arr(key))[0][0]) == int(t[0])
        x.close()


def test_long_run_to_one_id(ctx):
    """600 owners of one key (three tiles) all sent to one id: an id of the run, an id nobody
    holds, and an id that is itself sent on"""
    keys, ids, key, owners = mc.long_run_case()
    for name, (f, t, coalesced) in mc.long_run_maps(owners).items():
        x, d = built(ctx, keys, ids)
        assert mc.check_merge(x, d, f, t, twin_of(ctx), None, name) == (len(f), coalesced)
        assert int(x.key_links(arr(key))[0][0]) == mc.LONG
        x.close()


def test_extremes_and_permutations(ctx):
    """ids and keys 0 and 2^64 - 1; a swap, a 3-cycle and a chain, applied simultaneously"""
    k, v, maps = mc.extremes_case()
    for name, (f, t) in maps.items():
        x, d = built(ctx, k, v)
        assert mc.check_merge(x, d, f, t, twin_of(ctx), None, name)[0] > 0
        x.close()
    k, v = mc.permutation_pairs()
    for name, (f, t) in mc.permutation_maps().items():
        x, d = built(ctx, k, v)
        mc.check_merge(x, d, f, t, twin_of(ctx), None, name)
        assert name == "chain" or len(x) == 12
        x.close()
    x, d = built(ctx, arr(5, 5, 6), arr(1, 2, 1))
    assert x.merge_objects(arr(1, 2), arr(2, 3)) == (3, 0)  # b's old entries go to c, a's to b
    assert [a.tolist() for a in x.export_links()] == [[5, 5, 6], [2, 3, 2], [1, 1, 1]]
    x.close()


def test_link_sums(ctx):
    """coalescing adds links of 1 and of 3 to a pair that already existed and stays; then links of
    2^32 + 1 (built by 64 inserts of 2^26 copies of one pair) to a pair that stays, and to one that
    enters"""
    k = np.concatenate([np.full(7, 9, U), np.full(3, 9, U), arr(9), arr(8)])
    v = np.concatenate([np.full(7, 1, U), np.full(3, 2, U), arr(9), arr(2)])
    x, d = built(ctx, k, v)
    assert mc.check_merge(x, d, arr(2, 9), arr(1, 1), twin_of(ctx)) == (3, 2)
    assert [a.tolist() for a in x.export_links()] == [[8, 9], [1, 1], [1, 11]]
    t0 = time.perf_counter()
    big = 1 << 26
    bk, bv = torch.full((big,), 9, dtype=torch.int64, device="cuda"), torch.full((big,), 2, dtype=torch.int64, device="cuda")
    for _ in range(64):
        x.x.insert(bk, bv)
    del bk, bv
    x.insert(arr(9, 9), arr(2, 3))
    torch.cuda.synchronize()
    print("2^32 + 1 links built in %.2f s" % (time.perf_counter() - t0))
    assert [a.tolist() for a in x.export_links()] == [[8, 9, 9, 9], [1, 1, 2, 3], [1, 11, (1 << 32) + 1, 1]]
    assert x.merge_objects(arr(2, 3), arr(1, 1)) == (2, 2)
    assert [a.tolist() for a in x.export_links()] == [[8, 9], [1, 1], [1, (1 << 32) + 13]]
    assert x.merge_objects(arr(1), arr(0)) == (2, 0)
    assert [a.tolist() for a in x.export_links()] == [[8, 9], [0, 0], [1, (1 << 32) + 13]]
    x.close()


def test_directory_bits_follow_the_count(ctx):
    """34 entries coalesce to 17: the count crosses 32, a threshold of oi_dir_bits; every key is
    still found"""
    k, v, f, t = mc.dir_bits_case()
    x, d = built(ctx, k, v)
    assert mc.check_merge(x, d, f, t, twin_of(ctx)) == (17, 17) and len(x) == 17
    assert np.array_equal(x.lookup(np.unique(k))[1], np.ones(17, np.uint8))
    x.close()


def test_shards_add_up_to_the_unsharded_result(ctx):
    """nparts = 4, every part given the same map: the concatenated exports are the unsharded
    index's, moved and coalesced add up"""
    k, v, f, t = mc.shard_case()
    whole, dw = built(ctx, k, v)
    w_moved, w_coalesced = mc.check_merge(whole, dw, f, t, twin_of(ctx))
    w = whole.export_links()
    whole.close()
    parts, moved, coalesced = [], 0, 0
    for part in range(4):
        x, d = built(ctx, k, v, 4, part)
        assert len(x) > 0
        mv, co = mc.check_merge(x, d, f, t, twin_of(ctx, 4, part), None, part)
        moved, coalesced = moved + mv, coalesced + co
        parts.append(x.export_links())
        x.close()
    assert (moved, coalesced) == (w_moved, w_coalesced) and w_coalesced > 0
    for j in range(3):
        assert np.array_equal(np.concatenate([p[j] for p in parts]), w[j]), j


# ------------------------------------------------------------------ 3. the first mode
def test_first_mode_relabels_in_place(ctx):
    keys = oc.random_keys(1000, 5)
    vals = np.arange(1000, dtype=U) % U(7)
    x = ObjectIndex(ctx)
    assert x.insert(dev(keys), dev(vals)) == 1000
    model = dict(zip(keys.tolist(), vals.tolist()))
    k0 = host_u64(x.export()[0])
    for f, t in ((arr(1, 2, 77), arr(2, 3, 1)), (arr(3, 4), arr(4, 3)), (arr(0, 0), arr(M64, M64)), (arr(99), arr(1))):
        phi = mc.phi_of(f, t)
        moved = sum(1 for o in model.values() if phi.get(o, o) != o)
        model = {k: phi.get(o, o) for k, o in model.items()}
        assert x.merge_objects(dev(f), dev(t)) == (moved, 0)
        k, v = (host_u64(a) for a in x.export())
        assert np.array_equal(k, k0) and v.tolist() == [model[q] for q in k.tolist()] and len(x) == 1000
        ids, found = x.lookup(dev(keys))
        assert bool(found.all()) and host_u64(ids).tolist() == [model[q] for q in keys.tolist()]
    before = [host_u64(a) for a in x.export()]
    with pytest.raises(SdCasError):
        x.merge_objects(dev(arr(5, 5)), dev(arr(1, 2)))
    assert all(np.array_equal(a, host_u64(b)) for a, b in zip(before, x.export()))
    x.close()


# ------------------------------------------------------------------ 4. fences
def test_contradictions_and_refusals_change_nothing(ctx):
    """a contradiction is SD_ERR_INVALID with the export bit-equal before and after; null lists
    and another context's index are refused by the host before any launch"""
    k, v, f, t = mc.counted_case(257)
    x, d = built(ctx, k, v)
    before = x.export_links()
    for cf, ct in ((arr(101, 102, 101), arr(1, 2, 3)), (arr(101, 101), arr(101, 1)), (arr(77, 77), arr(1, 2)),
                   (np.concatenate([f, arr(4)]), np.concatenate([t, arr(2)]))):
        with pytest.raises(SdCasError) as e:
            x.merge_objects(cf, ct)
        assert e.value.rc == -1
        assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    empty = DeviceMerge(ctx)
    with pytest.raises(SdCasError):
        empty.merge_objects(arr(1, 1), arr(2, 3))
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    mv, co = ctypes.c_uint64(9), ctypes.c_uint64(9)
    df, dt = dev(f), dev(t)
    assert L.sd_object_index_merge_objects(ctx.handle, x.x.handle, None, dt.data_ptr(), 1, None, None, st) == -1
    assert L.sd_object_index_merge_objects(ctx.handle, x.x.handle, df.data_ptr(), None, 1, None, None, st) == -1
    assert L.sd_object_index_merge_objects(None, x.x.handle, df.data_ptr(), dt.data_ptr(), 1, None, None, st) == -1
    from spacedrive_amd.device import Context
    other = Context(0)
    assert L.sd_object_index_merge_objects(other.handle, x.x.handle, df.data_ptr(), dt.data_ptr(), len(f), None, None,
                                           st) == -1
    other.close()
    assert L.sd_object_index_merge_objects(ctx.handle, x.x.handle, None, None, 0, ctypes.byref(mv), ctypes.byref(co),
                                           st) == 0 and (mv.value, co.value) == (0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    assert L.sd_object_index_merge_objects(ctx.handle, x.x.handle, df.data_ptr(), dt.data_ptr(), len(f), None, None,
                                           st) == 0  # no reports asked for
    d.merge_objects(f, t)
    mc.compare(x, d, twin_of(ctx))
    x.close(), empty.close()


def test_small_merge_over_stale_scratch(ctx):
    """a small merge straight after one that moved every entry of 262 144, and a merge straight
    after a duplicates call that used the index's scratch, amid tensors of random data"""
    junk = [torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda") for _ in range(3)]
    k, v, f, t = mc.counted_case(262_144)
    x, d = built(ctx, k, v)
    junk.append(torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda"))
    every = arr(1, 2, 3, 4, 5, 101, 102, 103, 104, 105)
    assert mc.check_merge(x, d, every, every + U(1000), None, None, "all move")[0] == 262_144
    assert mc.check_merge(x, d, arr(1101, 77), arr(1001, 5), None, None, "small after large")[1] > 0
    dk, di, _ = x.duplicate_entries(0, 2)
    assert len(dk) > 0
    assert mc.check_merge(x, d, arr(1103, 1104), arr(1104, 1103), None, None, "after duplicates")[0] > 0
    small, ds = built(ctx, *mc.counted_case(257)[:2])
    assert mc.check_merge(small, ds, f, t, twin_of(ctx), None, "another index")[1] > 0
    x.close(), small.close()
    del junk


# ------------------------------------------------------------------ 5. end to end
def test_duplicates_to_merge_map_to_merge_objects_to_orphans(ctx):
    """duplicate_entries(0, 2) on the device, merge_map on the host, merge_objects, then
    orphans(d_from) and duplicate_stats: no key has two owners, keys and links stand, every `from`
    owns nothing, coalesced is the drop in entries"""
    k, v = mc.split_relation()
    x, d = built(ctx, k, v)
    s0 = x.duplicate_stats()
    assert s0[5] > 0
    dk, di, _ = x.x.duplicate_entries(0, 2)
    f, t = dedup.merge_map(dk, di)
    d_from = dev(f)
    want = d.merge_objects(f, t)
    assert x.x.merge_objects(d_from, dev(t)) == want
    mc.compare(x, d, twin_of(ctx))
    s1 = x.duplicate_stats()
    assert s1[5] == 0 and s1[0] == s0[0] and s1[2] == s0[2]
    assert want[1] == int(s0[1] - s1[1]) > 0
    assert np.array_equal(host_u64(x.x.orphans(d_from)), f)
    assert len(x.orphans(t)) == 0
    x.close()
