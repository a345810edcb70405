"""The owners mode of the device-resident Object index (include/sd_cas.h:
SD_OBJECT_INDEX_OWNERS; csrc/object_index.hip) -- run on an MI355X: -m gpu.  Everything is
bit-exact against the dict statement of the header's semantics
(tests/object_index_owners_cases.py) or, at the sizes a dict walks too slowly, the numpy mirrors
that tests/test_object_index_owners.py pins to it; the histories go to
oracle/identifier_spec.py directly.  Dropped pairs and link counts are written between 0xA5
guard rows into pre-filled rows, so a write outside the rows a call owns, or a missing one,
shows."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup, synth  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from spacedrive_amd.dedup import dest_of, group_host, keys_from_hashes  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests import object_index_owners_cases as wc  # noqa: E402
from tests import object_index_remove_cases as rc  # noqa: E402
from tests.test_gpu_object_index import G, Guarded, POISON, _run_ranks, dev, host_u64, stage_and_hash  # noqa: E402
from tests.test_gpu_object_index_remove import DeviceIndexR  # noqa: E402
from tests.test_object_index_owners import MirrorOwners, run_owner_script, script_probes  # noqa: E402
from tests.test_object_index_remove import MirrorIndexR  # noqa: E402
from tests.test_object_index_remove import run_script_against as run_first_mode_script  # noqa: E402

U = np.uint64
SLACK = 3  # rows of d_removed_out past the most a call can drop


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


class DeviceOwners(DeviceIndexR):
    """device.ObjectIndex(owners=True) behind the interface of the CPU tests' indexes.  Every
    removal and every links() call writes into pre-filled rows between guard rows and checks
    that the guards and the rows past the count still hold the fill."""

    def __init__(self, ctx, nparts=1, part=0):
        self.ctx, self.x = ctx, ObjectIndex(ctx, nparts, part, owners=True)

    def remove(self, keys, ids=None):
        d_k, d_i = dev(keys), None if ids is None else dev(ids)
        return self._removal(lambda out, cap: self.x.remove(d_k, d_i, d_removed_out=out, capacity=cap),
                             len(self) if ids is None else min(len(keys), len(self)))

    def links(self, keys, ids):
        m = len(keys)
        out = Guarded(m, 8, torch.int64)
        d_k, d_i = dev(keys), dev(ids)
        assert lib().sd_object_index_links(self.ctx.handle, self.x.handle, d_k.data_ptr() if m else None,
                                           d_i.data_ptr() if m else None, m, out.inner.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream) == 0
        assert out.guards_intact()
        got = out.host().view(U).reshape(-1).copy()
        assert np.array_equal(got, host_u64(self.x.links(d_k, d_i)))
        return got

    def export_links(self):
        n = len(self)
        bufs = [Guarded(n + SLACK, 8, torch.int64) for _ in range(3)]
        assert lib().sd_object_index_export_links(self.ctx.handle, self.x.handle, *(b.inner.data_ptr() for b in bufs),
                                                  n, torch.cuda.current_stream().cuda_stream) == 0
        got = []
        for b in bufs:
            a = b._all()
            assert (a[:G] == POISON).all() and (a[G + n:] == POISON).all()  # the guards, and nothing past n rows
            got.append(a[G:G + n].view(U).reshape(-1).copy())
        assert all(np.array_equal(g, host_u64(t)) for g, t in zip(got, self.x.export_links()))
        return tuple(got)


def on_device(ctx, name, script, make_a, probes=None, first=False):
    made = []

    def make():
        made.append(DeviceOwners(ctx))
        return made[-1]

    def make_first():
        made.append(DeviceIndexR(ctx))
        return made[-1]
    try:
        return run_owner_script(name, script, make_a, make, probes, make_first if first else None)
    finally:
        for x in made:
            x.close()


# ------------------------------------------------------------------ 1. the dict statement
@pytest.mark.parametrize("seed", wc.SCRIPT_SEEDS)
def test_seeded_scripts_equal_dict_statement(ctx, seed):
    """Seeded scripts of insert / remove with ids (fewer links than held, as many, more, absent
    pairs, another id) / remove without ids / remove_objects: after every operation the return
    values, d_removed_out, export_links, links() and lookup equal the dict statement's, and
    lookup and sd_dedup_owners_indexed answer as a first-mode index of the first owners does."""
    on_device(ctx, seed, wc.seeded_script(seed), wc.DictOwners, script_probes(seed), first=True)


# ------------------------------------------------------------------ 2. histories
def test_histories_never_ask_the_db_for_owners(ctx):
    """rc.History's events under the owners-mode cycle on the device (owners_of raises): the
    entries equal the DB's link relation and the first owners equal truth() after every event."""
    total = {}
    for seed in rc.HISTORY_SEEDS:
        x = DeviceOwners(ctx)
        for k, v in wc.OwnersHistory(seed).run(x).items():
            total[k] = total.get(k, 0) + v
        x.close()
    wc.check_owner_history_counts(total)


# ------------------------------------------------------------------ 3. shapes
def test_entry_counts_equal_dict_statement(ctx):
    """0, 1, 15/16/17 (directory bits 0 -> 1), 255/256/257, 1023/1024/1025, 4097 entries with
    the u64 edge keys, ids 0 and 2^64 - 1, runs at both ends and neighbouring keys with the
    same id sets: asked <, = and > held, a removal without ids, by Object, everything, and an
    insert into the emptied index."""
    for n in wc.ENTRY_COUNTS:
        on_device(ctx, n, wc.shape_script(n), wc.DictOwners)


def test_large_shape_equals_mirror(ctx):
    """262 144 + 300 entries: a workgroup's slice of the sliced passes is two tiles."""
    _, b = on_device(ctx, "large", wc.shape_script(wc.LARGE), MirrorOwners)


def test_runs_of_equal_keys(ctx):
    """Two owners of one key across positions 255 | 256; RUN owners of one key (a bucket far
    over 16 entries, over many tiles), removed one by one, by Object and by key at once."""
    keys, ids, key = wc.straddle_case()
    script = [("insert", keys, ids), ("remove", np.array([key], U), np.array([10], U)), ("insert", keys, ids),
              ("remove", np.array([key], U), np.array([4], U)), ("remove", np.array([key, key], U), np.array([4, 10], U)),
              ("insert", keys, ids), ("remove", np.array([key], U), None), ("expect_count", 598)]
    on_device(ctx, "straddle", script, wc.DictOwners, (keys, ids, wc.scan_records(1)), first=True)
    keys, ids, key, owners = wc.long_run_case()
    script = [("insert", keys, ids), ("remove", np.full(5, key, U), owners[:5].copy()),
              ("remove_objects", owners[100:110].copy()), ("insert", keys, ids),
              ("remove", np.array([key], U), None), ("expect_count", 2000), ("insert", keys, ids),
              ("remove", np.array([key], U), None), ("expect_count", 2000)]
    on_device(ctx, "long run", script, wc.DictOwners, (keys, ids, wc.scan_records(2)), first=True)


def test_long_run_removed_by_key_into_the_wrappers_own_rows(ctx):
    """ObjectIndex.remove of one key with RUN owners, ids None and no d_removed_out: the
    wrapper sizes its own rows for every owner of the key (as HostObjectIndex.remove does) and
    returns all RUN dropped pairs in ascending id order; the other entries stay."""
    keys, ids, key, owners = wc.long_run_case()
    x, m = ObjectIndex(ctx, owners=True), MirrorOwners()
    try:
        assert x.insert(dev(keys), dev(ids)) == m.insert(keys, ids) == 2000 + wc.RUN
        pairs, r = x.remove(dev(np.array([key], U)))
        want, wr = m.remove(np.array([key], U), None)
        assert r == wr == wc.RUN and np.array_equal(host_u64(pairs).reshape(-1, 2), want)
        assert np.array_equal(want[:, 1], np.sort(owners)) and len(x) == 2000
        assert all(np.array_equal(host_u64(p), q) for p, q in zip(x.export_links(), m.export_links()))
    finally:
        x.close()


def test_insert_shapes(ctx):
    """m = 1; COPIES copies of one pair give one entry with COPIES links; present and absent
    pairs shuffled in one batch; growth across two reallocations."""
    x = DeviceOwners(ctx)
    one_k, one_v = np.array([oc.M64], U), np.array([0], U)
    assert x.insert(one_k, one_v) == 1 and x.insert(one_k, one_v) == 0
    assert [a.tolist() for a in x.export_links()] == [[oc.M64], [0], [2]]
    assert x.insert(np.full(wc.COPIES, 42, U), np.full(wc.COPIES, 9, U)) == 1
    assert [a.tolist() for a in x.export_links()] == [[42, oc.M64], [9, 0], [wc.COPIES, 2]]
    pairs, r = x.remove(np.full(wc.COPIES - 1, 42, U), np.full(wc.COPIES - 1, 9, U))
    assert r == 0 and x.links(np.array([42, 42], U), np.array([9, 8], U)).tolist() == [1, 0]
    x.close()
    k, v = wc.shaped_pairs(1025)
    half = np.concatenate([k[::2], k[::2]]), np.concatenate([v[::2], v[::2]])
    mixed = np.argsort(oc.splitmix(3, 1025))
    script = [("insert",) + half, ("insert", k[mixed], v[mixed])] + [("insert", gk, gv) for gk, gv in wc.growth_steps()]
    on_device(ctx, "insert shapes", script, wc.DictOwners, (k, v, wc.scan_records(3)))


def test_large_operation_then_small_amid_random_data(ctx):
    """A 300 000-pair insert and a 100 000-pair removal, then small operations on that index and
    on another one, with the sorted batch, the asked links, the flags and the per-workgroup
    counts of the larger calls stale and the buffers allocated between tensors of random data."""
    junk = [torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda") for _ in range(3)]
    big, bm = DeviceOwners(ctx), MirrorOwners()
    junk.append(torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda"))
    a = oc.random_keys(150_000, 51)
    ak = np.concatenate([a, a])
    av = np.concatenate([np.arange(150_000, dtype=U) % U(50_000), np.arange(150_000, dtype=U) % U(3)])
    small, sm = DeviceOwners(ctx), MirrorOwners()
    b = oc.random_keys(700, 52)
    vb = oc.vals_for(b, 53)
    steps = [(big, bm, "insert", (ak, av)),
             (small, sm, "insert", (np.concatenate([b, b[:9]]), np.concatenate([vb, vb[:9]]))),
             (big, bm, "remove", (ak[:100_000].copy(), av[:100_000].copy())),
             (small, sm, "remove", (b[:5].copy(), vb[:5].copy())),
             (big, bm, "insert", (a[:3].copy(), av[:3].copy())),
             (big, bm, "remove_objects", (np.arange(4, 20_000, 2, dtype=U),)),  # ~10 000 of ~200 000 entries
             (small, sm, "remove_objects", (vb[100:103].copy(),)),
             (big, bm, "remove", (a[:7].copy(), None)),
             (small, sm, "remove", (b[::2].copy(), vb[::2].copy()))]
    for x, m, op, args in steps:
        junk.append(torch.randint(0, 255, (1 << 18,), dtype=torch.uint8, device="cuda"))
        got, want = getattr(x, op)(*args), getattr(m, op)(*args)
        assert (got == want) if op == "insert" else (got[1] == want[1] and np.array_equal(got[0], want[0])), op
        assert all(np.array_equal(p, q) for p, q in zip(x.export_links(), m.export_links())), op
    probe = np.concatenate([a[:2000], b])
    assert np.array_equal(big.lookup(probe)[0], bm.lookup(probe)[0])
    assert np.array_equal(small.links(b, vb), sm.links(b, vb))
    assert len(big) > 100_000 and len(small) > 300
    big.close(), small.close()


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("by", ["pairs", "keys", "objects"])
def test_capacity_short_by_one_changes_nothing_links_included(ctx, by):
    k, v, rk, rv, rids = wc.shard_case()
    x, m = DeviceOwners(ctx), MirrorOwners()
    x.insert(k, v), m.insert(k, v)
    before = x.export_links()
    d_a, d_b = dev(rids if by == "objects" else rk), dev(rv)

    def removal(out, cap):
        if by == "objects":
            return x.x.remove_objects(d_a, d_removed_out=out, capacity=cap)
        return x.x.remove(d_a, d_b if by == "pairs" else None, d_removed_out=out, capacity=cap)
    want_pairs, want = m.remove(rk, rv) if by == "pairs" else m.remove(rk, None) if by == "keys" else m.remove_objects(rids)
    assert want > 1
    if by == "pairs":  # some survivor gives up a link: the refused call must not have taken it
        assert (dedup.owners_links_host(*before, m.keys, m.vals) > m.cnt).any()
    out = Guarded(want + SLACK, 16, torch.int64)
    with pytest.raises(SdCasError) as e:
        removal(out.inner, want - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == want
    assert (out._all() == POISON).all()  # nothing was written
    assert all(np.array_equal(p, q) for p, q in zip(before, x.export_links()))  # entries AND links
    assert np.array_equal(x.links(before[0], before[1]), before[2])
    # d_removed_out == NULL still reports *removed
    removed = ctypes.c_uint64(0)
    st = torch.cuda.current_stream().cuda_stream
    if by == "objects":
        rcode = lib().sd_object_index_remove_objects(ctx.handle, x.x.handle, d_a.data_ptr(), d_a.numel(), None, 0,
                                                     ctypes.byref(removed), st)
    else:
        rcode = lib().sd_object_index_remove(ctx.handle, x.x.handle, d_a.data_ptr(),
                                             d_b.data_ptr() if by == "pairs" else None, d_a.numel(), None, 0,
                                             ctypes.byref(removed), st)
    assert rcode == 0 and removed.value == want
    assert all(np.array_equal(p, q) for p, q in zip(m.export_links(), x.export_links()))
    # and with room for exactly the count, on a second index
    y = DeviceOwners(ctx)
    y.insert(k, v)
    d_a, d_b = dev(rids if by == "objects" else rk), dev(rv)
    if by == "objects":
        pairs, r = y.x.remove_objects(d_a, d_removed_out=out.inner, capacity=want)
    else:
        pairs, r = y.x.remove(d_a, d_b if by == "pairs" else None, d_removed_out=out.inner, capacity=want)
    assert r == want and np.array_equal(host_u64(pairs).reshape(-1, 2), want_pairs)
    assert out.guards_intact() and (out.host()[want:] == POISON).all()
    x.close(), y.close()


# ------------------------------------------------------------------ 4. shards
def test_shard_union_is_the_unsharded_result(ctx):
    k, v, rk, rv, rids = wc.shard_case()
    whole = DeviceOwners(ctx)
    w_taken = whole.insert(k, v)
    w_pairs, w_r = whole.remove(rk, rv)
    w = whole.export_links()
    whole.close()
    assert 0 < w_r < w_taken
    for nparts in oc.NPARTS:
        parts, ps, taken = [], [], 0
        for part in range(nparts):
            x = DeviceOwners(ctx, nparts, part)
            taken += x.insert(k, v)
            pairs, r = x.remove(rk, rv)
            assert r == len(pairs) and np.all(dest_of(pairs[:, 0].copy(), nparts) == part)
            parts.append(x.export_links()), ps.append(pairs)
            x.close()
        assert taken == w_taken, nparts
        for j in range(3):
            assert np.array_equal(np.concatenate([p[j] for p in parts]), w[j]), (nparts, j)
        assert np.array_equal(np.concatenate(ps), w_pairs), nparts


@pytest.fixture(scope="module")
def hashed(ctx):
    n = 8000
    sizes, cids, twins = synth.library(0, n, n, dup_frac=0.3)
    return sizes, stage_and_hash(ctx, sizes, cids, twins)


@pytest.mark.parametrize("R", [2, 3])
def test_dedup_mgpu_indexed_with_owners_mode_indexes(ctx, hashed, R):
    """sd_cas_dedup_mgpu_indexed over R in-process ranks, every rank handed the same dump of
    (cas_id, Object) pairs -- two owners for every known cas_id, several links each -- into its
    owners-mode shard: each rank's records, owners (the SMALLEST Object id), existing flags and
    new heads equal the host grouping's; an index sharded for another (nparts, part) makes
    every rank return SD_ERR_INVALID."""
    from spacedrive_amd.device import Comm, CommGroup, Context
    sizes, h = hashed
    n = len(sizes)
    valid = sizes != 0
    keys = keys_from_hashes(h)
    all_recs = np.stack([keys[valid].view(np.int64), np.arange(n)[valid]], axis=1)
    dst = dest_of(all_recs[:, 0].view(U), R)
    known = np.unique(keys[valid])[::2]
    first, later = oc.vals_for(known, 91) >> U(1), (oc.vals_for(known, 91) >> U(1)) + U(1 + (1 << 63))
    pk = np.concatenate([known, known, known[::3]])
    pv = np.concatenate([later, first, later[::3]])  # the later owner listed first: order does not matter
    cuts = [n * q // R for q in range(R + 1)]
    group = CommGroup(R)
    ctxs = [Context(0) for _ in range(R)]
    comms = [Comm(ctxs[r], None, R, r, group=group) for r in range(R)]
    d_hash = torch.from_numpy(h.reshape(-1).copy()).cuda()
    d_valid = torch.from_numpy(valid.astype(np.uint8)).cuda()
    d_pk, d_pv = dev(pk), dev(pv)
    idx = [ObjectIndex(ctxs[r], R, r, owners=True) for r in range(R)]
    mirrors = [MirrorOwners(R, r) for r in range(R)]
    for r in range(R):
        assert idx[r].insert(d_pk, d_pv) == mirrors[r].insert(pk, pv) > 0
    wrong = ObjectIndex(ctxs[1], R, 0, owners=True)
    torch.cuda.synchronize()

    def rank_call(r, index):
        lo, hi = cuts[r], cuts[r + 1]
        st = torch.cuda.Stream()
        runner = dedup.RcclDedup(ctxs[r], comms[r], d_hash.device, capacity=n)
        try:
            res = runner(d_hash[lo * 32:], d_valid[lo:], hi - lo, lo, stream=st, index=index(r))
        except SdCasError as e:
            return e.rc
        st.synchronize()
        return [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in res]

    try:
        got = _run_ranks(R, lambda r: rank_call(r, lambda q: idx[q]))
        bad = _run_ranks(R, lambda r: rank_call(r, lambda q: wrong if q == 1 else idx[q]))
        assert bad == [-1] * R
        for r in range(R):
            gr, grep, gng = group_host(all_recs[dst == r])
            w_owner, w_ex, w_new = dedup.owners_indexed_host(gr, grep, mirrors[r].keys, mirrors[r].vals, 100)
            recs, rep, ng, own, ex, new = got[r]
            assert ng == gng and np.array_equal(recs, gr) and np.array_equal(rep, grep), r
            assert np.array_equal(own.view(U), w_owner) and np.array_equal(ex, w_ex), r
            assert np.array_equal(new.view(U), w_new), r
            assert w_ex.any() and not w_ex.all() and len(w_new)
            assert (w_owner[w_ex == 1] < U(1 << 63)).all()  # the first owners, never the later ones
    finally:
        wrong.close()
        for x in idx:
            x.close()
        for c in comms:
            c.close()
        group.close()
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ 5. the fence between the modes
def test_links_calls_refuse_a_first_mode_index(ctx):
    x = ObjectIndex(ctx)
    o = ObjectIndex(ctx, owners=True)
    k = dev(np.arange(3, dtype=U))
    x.insert(k, k)
    out = Guarded(3, 8, torch.int64)
    st = torch.cuda.current_stream().cuda_stream
    p = out.inner.data_ptr()
    try:
        assert x.flags == 0 and o.flags == 1
        assert lib().sd_object_index_links(ctx.handle, x.handle, k.data_ptr(), k.data_ptr(), 3, p, st) == -1
        assert lib().sd_object_index_export_links(ctx.handle, x.handle, p, p, p, 3, st) == -1
        with pytest.raises(SdCasError):
            x.links(k, k)
        with pytest.raises(SdCasError):
            x.export_links()
        assert (out._all() == POISON).all() and len(x) == 3
        # argument errors and another context's index on an owners-mode index
        from spacedrive_amd.device import Context
        other = Context(0)
        o.insert(k, k)
        assert lib().sd_object_index_links(other.handle, o.handle, k.data_ptr(), k.data_ptr(), 3, p, st) == -1
        assert lib().sd_object_index_export_links(other.handle, o.handle, p, p, p, 3, st) == -1
        assert lib().sd_object_index_links(ctx.handle, o.handle, k.data_ptr(), None, 3, p, st) == -1
        assert lib().sd_object_index_export_links(ctx.handle, o.handle, p, p, p, 2, st) == SD_ERR_CAPACITY
        h = ctypes.c_void_p()
        assert lib().sd_object_index_create_ex(ctx.handle, 1, 0, 2, ctypes.byref(h)) == -1 and not h.value
        assert (out._all() == POISON).all()
        other.close()
    finally:
        x.close(), o.close()


@pytest.mark.parametrize("case", sorted(rc.fixed_scripts()))
def test_create_ex_without_the_flag_is_create(ctx, case):
    """An index made through create_ex(flags 0) equals the mirror, as one from create does, on
    the fixed removal scripts."""
    class ViaEx(DeviceIndexR):
        def __init__(self):
            self.ctx, self.x = ctx, ObjectIndex.__new__(ObjectIndex)
            self.x.ctx, self.x.nparts, self.x.part, self.x.owners_mode = ctx, 1, 0, False
            h = ctypes.c_void_p()
            assert lib().sd_object_index_create_ex(ctx.handle, 1, 0, 0, ctypes.byref(h)) == 0
            self.x.handle = h
    made = []

    def make():
        made.append(ViaEx())
        return made[-1]
    try:
        _, b = run_first_mode_script(case, rc.fixed_scripts()[case], MirrorIndexR, make)
        assert b.x.flags == 0
    finally:
        for x in made:
            x.close()


def test_scan_library_inserts_every_records_pair(ctx, tmp_path):
    """library.scan_library with an owners-mode index: the first scan of 300 files (duplicates
    inside and across steps of 7, empty files) inserts (key, Object id) for every record, the
    created ones under the ids the host gives; a second scan of the same files links every
    record to its cas_id's smallest Object id and adds one link each, creating no entry."""
    from spacedrive_amd.library import scan_library
    n = 300
    body = [bytes([j]) * (1 + 13 * j) for j in range(40)]
    which = (oc.splitmix(5, n) % U(len(body))).astype(np.int64)
    which[1] = which[0]
    paths, sizes = [], np.zeros(n, U)
    for i in range(n):
        data = b"" if i % 37 == 5 else body[which[i]]
        p = tmp_path / ("f%03d" % i)
        p.write_bytes(data)
        paths.append(str(p)), sizes.__setitem__(i, len(data))
    x, m = DeviceOwners(ctx), MirrorOwners()
    table = torch.arange(1000, 1000 + n, dtype=torch.int64, device="cuda")  # file f's Object gets id table[f]
    given = lambda files: table[files]  # noqa: E731 -- a gather sized to the files, as a host's mapping is: it
    #                                     must see creating file indices only, never a linked record's Object id
    r = scan_library(ctx, paths, sizes, chunk_size=7, index=x.x, object_id_of=given)
    recs, owner, ex, ids = (r[k].cpu().numpy() for k in ("records", "owner", "existing", "object_ids"))
    assert len(recs) == int((sizes != 0).sum()) and not ex.any() and np.array_equal(ids, owner + 1000)
    assert r["inserted"] == m.insert(recs[:, 0].view(U), ids.view(U)) == len(x) > 40  # same-step duplicates: own Objects
    assert all(np.array_equal(p, q) for p, q in zip(m.export_links(), x.export_links()))
    r2 = scan_library(ctx, paths, sizes, chunk_size=7, index=x.x, object_id_of=given)
    recs2, ex2, ids2 = (r2[k].cpu().numpy() for k in ("records", "existing", "object_ids"))
    assert ex2.all() and r2["inserted"] == 0 == m.insert(recs2[:, 0].view(U), ids2.view(U))
    assert np.array_equal(ids2.view(U), m.lookup(recs2[:, 0].view(U))[0])  # the smallest Object id of each key
    assert all(np.array_equal(p, q) for p, q in zip(m.export_links(), x.export_links()))
    assert int(m.cnt.sum()) == 2 * len(recs)
    x.close()


def test_hex_calls_follow_the_mode(ctx):
    x, m = DeviceOwners(ctx), MirrorOwners()
    keys = oc.random_keys(50, 81)
    ids = np.arange(50, dtype=U) % U(5)
    cas = ["%016x" % int(k) for k in keys]
    assert x.x.insert_hex(cas, ids) == m.insert(keys, ids) == 50
    assert x.x.insert_hex(cas[:20], ids[:20]) == m.insert(keys[:20], ids[:20]) == 0
    assert x.x.remove_hex(cas[:30], ids[:30]) == m.remove(keys[:30], ids[:30])[1] == 10
    assert x.x.remove_hex(cas[:5]) == m.remove(keys[:5], None)[1] == 5
    assert all(np.array_equal(p, q) for p, q in zip(m.export_links(), x.export_links()))
    x.close()
