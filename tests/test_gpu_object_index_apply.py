"""sd_object_index_apply on the device (include/sd_cas.h; csrc/object_index.hip: both lists
aggregated, one flagging pass, one fused merge-compaction) -- run on an MI355X: -m gpu.
Everything is bit-exact against the dict statement of the header's rule
(tests/object_index_apply_cases.py) or, at the sizes a dict walks too slowly, the numpy mirror
that tests/test_object_index_apply.py pins to it, and against a twin device index given remove
then insert.  The dropped pairs are written between 0xA5 guard rows into pre-filled rows, so a
write outside the rows a call owns, or a missing one, shows."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from spacedrive_amd.dedup import dest_of  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402
from tests import object_index_apply_cases as ac  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests import object_index_owners_cases as wc  # noqa: E402
from tests import object_index_remove_cases as rc  # noqa: E402
from tests.test_gpu_object_index import Guarded, POISON, dev, host_u64  # noqa: E402
from tests.test_gpu_object_index_owners import SLACK, DeviceOwners  # noqa: E402
from tests.test_object_index_apply import MirrorApply, capacity_case, exports_equal, run_apply_script  # noqa: E402
from tests.test_object_index_owners import script_probes  # noqa: E402

U = np.uint64
E = ac.E


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


class DeviceApply(DeviceOwners):
    """DeviceOwners with apply: the dropped pairs go into pre-filled rows between guard rows;
    the guards and the rows past the count must still hold the fill."""

    def apply(self, rk, rv, ik, iv):
        d = [dev(a) for a in (rk, rv, ik, iv)]
        taken = []

        def call(out, cap):
            pairs, t = self.x.apply(*d, d_removed_out=out, capacity=cap)
            taken.append(t)
            return pairs, len(pairs)
        pairs, r = self._removal(call, min(len(rk), len(self)))
        return pairs, r, taken[0]


def on_device(ctx, name, script, make_a, probes=None, twin=True):
    made = []

    def make():
        made.append(DeviceApply(ctx))
        return made[-1]
    try:
        return run_apply_script(name, script, make_a, make, probes, make if twin else None)
    finally:
        for x in made:
            x.close()


# ------------------------------------------------------------------ 1. the dict statement
@pytest.mark.parametrize("seed", ac.APPLY_SEEDS)
def test_seeded_scripts_equal_dict_statement(ctx, seed):
    """Seeded scripts that mix apply (asked <, = and > held, each with and without links added to
    the same pair; absent pairs; another id; repeats in both lists) with insert and the three
    removals: after every operation the return values, d_removed_out, export_links, links() and
    lookup equal the dict statement's, and the arrays those of a twin given remove then insert."""
    on_device(ctx, seed, ac.seeded_script(seed), ac.DictApply, script_probes(seed))


# ------------------------------------------------------------------ 2. shapes
def test_entry_counts_equal_dict_statement(ctx):
    """0, 1, 15/16/17, 255/256/257, 1023/1024/1025, 4097 entries: every fourth leaves while as
    many enter (the count stands, the directory must not); all leave; all leave and n enter;
    pairs enter at rank 0 and rank n; an apply on the empty index."""
    for n in wc.ENTRY_COUNTS:
        on_device(ctx, n, ac.entry_count_script(n), ac.DictApply)


def test_large_shape_equals_mirror(ctx):
    """262 144 + 300 entries (a slice of the sliced passes is two tiles), 1 % leave, 1 % enter."""
    on_device(ctx, "large", ac.large_script(), MirrorApply)


def test_straddle_long_run_and_copies(ctx):
    """Entering pairs and leaving entries at positions 255 | 256 (two tiles); RUN owners of one
    key, every second leaving while RUN / 2 enter; COPIES copies of one pair in each list."""
    keys, ids, key, scripts = ac.straddle_scripts()
    for name, script in scripts.items():
        on_device(ctx, name, script, ac.DictApply, (keys, ids))
    keys, ids, key, script = ac.long_run_script()
    on_device(ctx, "long run", script, ac.DictApply, (keys, ids))
    x = DeviceApply(ctx)
    assert x.insert(np.array([42, 43], U), np.array([9, 9], U)) == 2
    many = np.full(wc.COPIES, 42, U), np.full(wc.COPIES, 9, U)
    pairs, r, taken = x.apply(*many, *many)
    assert (r, taken) == (0, 0) and [a.tolist() for a in x.export_links()] == [[42, 43], [9, 9], [wc.COPIES, 1]]
    pairs, r, taken = x.apply(*many, E, E)
    assert pairs.tolist() == [[42, 9]] and taken == 0 and len(x) == 1
    x.close()


def test_directory_bits_and_growth(ctx):
    on_device(ctx, "dir bits", ac.dir_bits_script(), ac.DictApply)
    on_device(ctx, "growth", ac.growth_script(), ac.DictApply)


def test_nothing_leaves_or_enters_only_links_change(ctx):
    build, rm, ins, (k, v, want) = ac.in_place_case()
    x = DeviceApply(ctx)
    assert x.insert(*build) == 1025
    k0, v0, c0 = x.export_links()
    pairs, r, taken = x.apply(*rm, *ins)
    k1, v1, c1 = x.export_links()
    assert (r, taken, len(pairs)) == (0, 0, 0) and np.array_equal(k0, k1) and np.array_equal(v0, v1)
    assert (c0 == 3).all() and np.array_equal(x.links(k, v), want)
    assert np.array_equal(x.lookup(k)[1], np.ones(1025, np.uint8))
    x.close()


def test_large_apply_then_small_amid_random_data(ctx):
    """A 200 000-pair apply, then small ones on that index and on another, with the aggregated
    batches, the marks and the per-slice counts of the larger call stale and the buffers
    allocated between tensors of random data."""
    junk = [torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda") for _ in range(3)]
    big, bm = DeviceApply(ctx), MirrorApply()
    a = oc.random_keys(150_000, 51)
    av = np.arange(150_000, dtype=U) % U(50_000)
    junk.append(torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda"))
    small, sm = DeviceApply(ctx), MirrorApply()
    b = oc.random_keys(700, 52)
    vb = oc.vals_for(b, 53)
    steps = [(big, bm, (E, E, a, av)),
             (small, sm, (E, E, np.concatenate([b, b[:9]]), np.concatenate([vb, vb[:9]]))),
             (big, bm, (a[:100_000].copy(), av[:100_000].copy(), a[50_000:150_000] ^ U(1), av[50_000:150_000].copy())),
             (small, sm, (b[:5].copy(), vb[:5].copy(), b[3:6].copy(), vb[3:6].copy())),
             (big, bm, (a[:3].copy(), av[:3].copy(), a[:2].copy(), av[:2].copy())),
             (small, sm, (b[::2].copy(), vb[::2].copy(), b[:1].copy(), vb[:1] ^ U(1))),
             (big, bm, (a[100_000:100_004].copy(), av[100_000:100_004].copy(), E, E))]
    for x, m, args in steps:
        junk.append(torch.randint(0, 255, (1 << 18,), dtype=torch.uint8, device="cuda"))
        got, want = x.apply(*args), m.apply(*args)
        assert got[1:] == want[1:] and np.array_equal(got[0], want[0])
        assert exports_equal(m, x)
    probe = np.concatenate([a[:2000], b])
    assert np.array_equal(big.lookup(probe)[0], bm.lookup(probe)[0])
    assert len(big) > 100_000 and len(small) > 300
    big.close(), small.close()


# ------------------------------------------------------------------ 3. capacity
def test_capacity_short_by_one_changes_nothing(ctx):
    build, rm, ins = capacity_case()
    x, m = DeviceApply(ctx), MirrorApply()
    x.insert(*build), m.insert(*build)
    before = x.export_links()
    want_pairs, want, want_taken = m.apply(*rm, *ins)
    assert want > 1 and want_taken == 40
    held = dedup.owners_links_host(*before, m.keys, m.vals)
    assert ((held > m.cnt) & (held > 0)).any() and ((held < m.cnt) & (held > 0)).any()  # counts only, both ways
    d = [dev(a) for a in rm + ins]
    out = Guarded(want + SLACK, 16, torch.int64)
    with pytest.raises(SdCasError) as e:
        x.x.apply(*d, d_removed_out=out.inner, capacity=want - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == want
    assert (out._all() == POISON).all()  # nothing was written
    assert all(np.array_equal(p, q) for p, q in zip(before, x.export_links()))  # entries, links, no new pair
    assert np.array_equal(x.links(before[0], before[1]), before[2])
    assert not x.links(ins[0][:40].copy(), ins[1][:40].copy()).any()
    # with room for exactly the count
    pairs, taken = x.x.apply(*d, d_removed_out=out.inner, capacity=want)
    assert taken == want_taken and np.array_equal(host_u64(pairs).reshape(-1, 2), want_pairs)
    assert out.guards_intact() and (out.host()[want:] == POISON).all()
    assert exports_equal(m, x)
    # d_removed_out == NULL still reports *removed
    y = DeviceApply(ctx)
    y.insert(*build)
    removed, tk = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib().sd_object_index_apply(ctx.handle, y.x.handle, d[0].data_ptr(), d[1].data_ptr(), d[0].numel(),
                                       d[2].data_ptr(), d[3].data_ptr(), d[2].numel(), None, 0, ctypes.byref(removed),
                                       ctypes.byref(tk), torch.cuda.current_stream().cuda_stream) == 0
    assert (removed.value, tk.value) == (want, want_taken) and exports_equal(m, y)
    x.close(), y.close()


# ------------------------------------------------------------------ 4. fences
def test_refusals_and_no_ops(ctx):
    first, x = ObjectIndex(ctx), DeviceApply(ctx)
    k = dev(np.arange(1, 4, dtype=U))
    st = torch.cuda.current_stream().cuda_stream
    r, t = ctypes.c_uint64(9), ctypes.c_uint64(9)
    p = k.data_ptr()
    try:
        first.insert(k, k), x.x.insert(k, k)
        before = x.export_links()
        L = lib()
        assert L.sd_object_index_apply(ctx.handle, first.handle, p, p, 3, p, p, 3, None, 0, ctypes.byref(r),
                                       ctypes.byref(t), st) == -1
        with pytest.raises(SdCasError):
            first.apply(k, k, k, k)
        assert len(first) == 3 and np.array_equal(host_u64(first.export()[0]), np.arange(1, 4, dtype=U))
        assert L.sd_object_index_apply(ctx.handle, x.x.handle, p, None, 3, p, p, 3, None, 0, None, None, st) == -1
        assert L.sd_object_index_apply(ctx.handle, x.x.handle, None, p, 3, None, None, 0, None, 0, None, None, st) == -1
        assert L.sd_object_index_apply(ctx.handle, x.x.handle, None, None, 0, p, None, 3, None, 0, None, None, st) == -1
        from spacedrive_amd.device import Context
        other = Context(0)
        assert L.sd_object_index_apply(other.handle, x.x.handle, p, p, 3, p, p, 3, None, 0, None, None, st) == -1
        other.close()
        assert L.sd_object_index_apply(ctx.handle, x.x.handle, None, None, 0, None, None, 0, None, 0, ctypes.byref(r),
                                       ctypes.byref(t), st) == 0 and (r.value, t.value) == (0, 0)
        pairs, n_removed, n_taken = x.apply(E, E, E, E)
        assert (len(pairs), n_removed, n_taken) == (0, 0, 0)
        assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    finally:
        first.close(), x.close()


def test_one_empty_list_is_insert_or_remove_on_a_twin(ctx):
    k, v, rk, rv, _ = wc.shard_case()
    x, t = DeviceApply(ctx), DeviceApply(ctx)
    pairs, r, taken = x.apply(E, E, k, v)
    assert r == 0 and taken == t.insert(k, v) > 0 and exports_equal(t, x)
    pairs, r, taken = x.apply(rk, rv, E, E)
    t_pairs, t_r = t.remove(rk, rv)
    assert taken == 0 and r == t_r > 0 and np.array_equal(pairs, t_pairs) and exports_equal(t, x)
    x.close(), t.close()


# ------------------------------------------------------------------ 5. shards
def test_shard_union_is_the_unsharded_result(ctx):
    build, rm, ins = capacity_case()
    whole = DeviceApply(ctx)
    whole.insert(*build)
    w_pairs, w_r, w_taken = whole.apply(*rm, *ins)
    w = whole.export_links()
    whole.close()
    assert w_r > 1 and w_taken == 40
    for nparts in oc.NPARTS:
        parts, ps, taken = [], [], 0
        for part in range(nparts):
            x = DeviceApply(ctx, nparts, part)
            x.insert(*build)
            pairs, r, tk = x.apply(*rm, *ins)
            assert r == len(pairs) and np.all(dest_of(pairs[:, 0].copy(), nparts) == part)
            parts.append(x.export_links()), ps.append(pairs)
            taken += tk
            x.close()
        assert taken == w_taken, nparts
        for j in range(3):
            assert np.array_equal(np.concatenate([p[j] for p in parts]), w[j]), (nparts, j)
        assert np.array_equal(np.concatenate(ps), w_pairs), nparts


# ------------------------------------------------------------------ 6. histories
def test_histories_with_the_one_call_cycle(ctx):
    """ac.ApplyHistory on the device: a content change is one apply, a deleted file_path an apply
    with an empty insertion list, a burst one apply of the coalesced lists; the entries equal
    the DB's link relation and the first owners equal truth() after every event."""
    total = {}
    for seed in rc.HISTORY_SEEDS:
        x = DeviceApply(ctx)
        for k, v in ac.ApplyHistory(seed).run(x).items():
            total[k] = total.get(k, 0) + v
        x.close()
    ac.check_apply_history_counts(total)


# ------------------------------------------------------------------ 7. _hex
def test_apply_hex_equals_the_device_array_call(ctx):
    x, y, m = DeviceApply(ctx), DeviceApply(ctx), MirrorApply()
    keys = oc.random_keys(60, 81)
    ids = np.arange(60, dtype=U) % U(5)
    for i in (x, y, m):
        i.insert(keys[:50], ids[:50]), i.insert(keys[:20], ids[:20])
    cas = ["%016x" % int(k) for k in keys]
    rm, ins = slice(10, 40), slice(35, 60)
    want_pairs, want, want_taken = m.apply(keys[rm], ids[rm], keys[ins], ids[ins])
    assert x.x.apply_hex(cas[rm], ids[rm], cas[ins], ids[ins]) == (want, want_taken) and want == 15 and want_taken == 10
    got = y.apply(keys[rm], ids[rm], keys[ins], ids[ins])
    assert got[1:] == (want, want_taken) and np.array_equal(got[0], want_pairs)
    assert exports_equal(m, x) and exports_equal(y, x)
    # a malformed cas_id in either list: refused with nothing changed
    before = x.export_links()
    for bad_rm, bad_in in ((["%016X" % 0xABCDEF], cas[:1]), (cas[:1], ["0123456789abcdeg"])):
        with pytest.raises(SdCasError):
            x.x.apply_hex(cas[40:45] + bad_rm, np.arange(5 + len(bad_rm), dtype=U), cas[:3] + bad_in, np.arange(3 + len(bad_in), dtype=U))
    assert all(np.array_equal(a, b) for a, b in zip(before, x.export_links()))
    x.close(), y.close()
