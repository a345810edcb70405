"""Removal from the device-resident Object index (include/sd_cas.h: sd_object_index_remove,
_remove_objects, _remove_hex; csrc/object_index.hip) -- run on an MI355X: -m gpu.  Everything
is bit-exact against the numpy mirrors (dedup.index_remove_host / index_remove_objects_host),
which tests/test_object_index_remove.py pins to a dict statement of the header's semantics;
the histories go to oracle/identifier_spec.py directly.  The dropped pairs are written between
0xA5 guard rows into pre-filled rows, so a write outside the rows a call owns, or a missing
one, shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from spacedrive_amd.dedup import dest_of  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests import object_index_remove_cases as rc  # noqa: E402
from tests.test_gpu_object_index import Guarded, POISON, _run_ranks, dev, host_u64, stage_and_hash  # noqa: E402
from tests.test_object_index_remove import MirrorIndexR, run_script_against  # noqa: E402

U = np.uint64
SLACK = 3  # rows of d_removed_out past the most a call can drop


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


class DeviceIndexR:
    """device.ObjectIndex behind the interface of the CPU tests' indexes (uint64 numpy arrays).
    Every removal writes its dropped pairs into pre-filled rows between guard rows and checks
    that the guards and the rows past the count still hold the fill."""

    def __init__(self, ctx, nparts=1, part=0):
        self.ctx, self.x = ctx, ObjectIndex(ctx, nparts, part)

    def __len__(self):
        return len(self.x)

    def close(self):
        self.x.close()

    def insert(self, keys, vals):
        return self.x.insert(dev(keys), dev(vals))

    def _removal(self, call, bound):
        out = Guarded(bound + SLACK, 16, torch.int64)
        pairs, r = call(out.inner, bound + SLACK)
        assert out.guards_intact()
        rows = out.host().view(U).reshape(-1, 2)
        assert r <= bound and (out.host()[r:] == POISON).all()  # nothing past the count
        assert np.array_equal(host_u64(pairs).reshape(-1, 2), rows[:r])
        return rows[:r].copy(), r

    def remove(self, keys, ids=None):
        d_k, d_i = dev(keys), None if ids is None else dev(ids)
        return self._removal(lambda out, cap: self.x.remove(d_k, d_i, d_removed_out=out, capacity=cap),
                             min(len(keys), len(self)))

    def remove_objects(self, ids):
        d_i = dev(ids)
        return self._removal(lambda out, cap: self.x.remove_objects(d_i, d_removed_out=out, capacity=cap), len(self))

    def lookup(self, q):
        ids, found = self.x.lookup(dev(q))
        return host_u64(ids), found.cpu().numpy()

    def export(self):
        k, v = self.x.export()
        return host_u64(k), host_u64(v)

    def scan(self, recs, chunk):
        """sd_dedup_group + sd_dedup_owners_indexed on the scan's records"""
        m = len(recs)
        if m == 0:
            return recs, np.zeros(0, U), np.zeros(0, np.uint8), np.zeros((0, 2), U)
        d_r = dev(recs.reshape(-1))
        d_rep = torch.empty(m, dtype=torch.int64, device="cuda")
        self.ctx.dedup_group(d_r, m, d_rep)
        d_owner = torch.empty(m, dtype=torch.int64, device="cuda")
        d_ex = torch.empty(m, dtype=torch.uint8, device="cuda")
        d_new = torch.empty((m, 2), dtype=torch.int64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.x.owners(d_r, m, d_rep, d_owner, d_ex, d_new, d_n, chunk_size=chunk)
        n_new = int(d_n.item())
        return (d_r.cpu().numpy().reshape(m, 2), host_u64(d_owner), d_ex.cpu().numpy(),
                host_u64(d_new[:n_new]).reshape(-1, 2))


def run_on_device(ctx, name, script):
    """The script on the device index and the mirror: after every operation the result, the
    export (== the mirror, keys strictly ascending) and the count agree; after a removal every
    exported key is found by lookup and every dropped key is missed."""
    made = []

    def make():
        made.append(DeviceIndexR(ctx))
        return made[0]
    try:
        return run_script_against(name, script, MirrorIndexR, make)
    finally:
        for x in made:
            x.close()


# ------------------------------------------------------------------ sweeps and fixed cases
@pytest.mark.parametrize("kind", rc.KINDS)
def test_remove_by_key_sweep(ctx, kind):
    """sd_object_index_remove at every index size x removal count of the case lists,
    unconditional and conditional (right ids, wrong ids, one key named wrongly then rightly),
    over uniform keys, the u64 edges and a set that one directory bucket holds entirely."""
    scripts = rc.by_key_scripts(kind)
    for name, script in scripts:
        run_on_device(ctx, name, script)
    assert len(scripts) == 22


def test_remove_objects_sweep(ctx):
    """sd_object_index_remove_objects at every index size: ids owning nothing, repeated ids at
    every count, every id (the index ends empty, lookups miss everything, insert works)."""
    for name, script in rc.by_object_scripts():
        mirror, _ = run_on_device(ctx, name, script)
        assert len(mirror) == len(script[0][1])


@pytest.mark.parametrize("case", sorted(rc.fixed_scripts()))
def test_remove_fixed_cases(ctx, case):
    """The first entry, the last entry, one whole directory bucket; three_growth backwards
    (the directory bits fall 4 -> 2 -> 0 and the directory is rebuilt at each) and an insert
    into the emptied index; nothing from an empty index."""
    run_on_device(ctx, case, rc.fixed_scripts()[case])


def test_remove_large_shape(ctx):
    """300 007 entries, past 1024 workgroups x 256, so a workgroup's running base carries
    over tiles: every other entry, runs of 1000 dropped and kept, all but one, then the last."""
    run_on_device(ctx, "large", rc.large_script())


def test_remove_hex(ctx):
    keys = oc.random_keys(300, 81)
    vals = oc.vals_for(keys, 82)
    x, m = DeviceIndexR(ctx), MirrorIndexR()
    x.insert(keys, vals), m.insert(keys, vals)
    cas = ["%016x" % int(k) for k in keys[:100]]
    ids = vals[:100].copy()
    ids[::2] ^= U(1)
    assert x.x.remove_hex(cas, ids) == m.remove(keys[:100], ids)[1] == 50
    assert x.x.remove_hex(cas) == m.remove(keys[:100])[1] == 50
    assert np.array_equal(x.export()[0], m.keys) and np.array_equal(x.export()[1], m.vals)
    with pytest.raises(SdCasError):
        x.x.remove_hex(["00000000000000FG"])
    x.close()


def test_remove_default_buffers(ctx):
    """The wrappers without a caller's buffer: the pairs come back in a tensor of their own,
    regrown to the requirement when remove_objects drops more than its first guess."""
    keys = oc.random_keys(20_000, 83)
    vals = np.arange(20_000, dtype=U) % U(4)
    x, m = DeviceIndexR(ctx), MirrorIndexR()
    x.insert(keys, vals), m.insert(keys, vals)
    pairs, r = x.x.remove_objects(dev(np.array([1, 3], U)))
    want, wr = m.remove_objects(np.array([1, 3], U))
    assert r == wr == 10_000 and np.array_equal(host_u64(pairs).reshape(-1, 2), want)
    pairs, r = x.x.remove(dev(keys[:64]))
    want, wr = m.remove(keys[:64])
    assert r == wr == 32 and np.array_equal(host_u64(pairs).reshape(-1, 2), want)
    assert np.array_equal(x.export()[0], m.keys) and np.array_equal(x.export()[1], m.vals)
    x.close()


# ------------------------------------------------------------------ stale scratch
def test_large_removal_then_small_amid_random_data(ctx):
    """A removal by 70 000 Object ids from 300 000 entries, then small removals on that index
    and on another one, with the flags, sorted ids and per-workgroup counts of the larger
    call stale and the buffers allocated between tensors of random data."""
    junk = [torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda") for _ in range(3)]
    big, bm = DeviceIndexR(ctx), MirrorIndexR()
    junk.append(torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda"))
    a = oc.random_keys(300_000, 51)
    va = np.arange(300_000, dtype=U) % U(100_000)
    big.insert(a, va), bm.insert(a, va)
    small, sm = DeviceIndexR(ctx), MirrorIndexR()
    b = oc.random_keys(700, 52)
    vb = oc.vals_for(b, 53)
    small.insert(b, vb), sm.insert(b, vb)
    junk.append(torch.randint(0, 255, (1 << 18,), dtype=torch.uint8, device="cuda"))
    steps = [(big, bm, "remove_objects", (np.arange(0, 140_000, 2, dtype=U),)),
             (small, sm, "remove", (b[:5], None)),
             (big, bm, "remove", (a[:7], va[:7])),
             (small, sm, "remove_objects", (vb[100:103],)),
             (big, bm, "remove", (a[::3].copy(), None)),
             (small, sm, "remove", (b[::2].copy(), vb[::2].copy()))]
    for x, m, op, args in steps:
        junk.append(torch.randint(0, 255, (1 << 18,), dtype=torch.uint8, device="cuda"))
        (gp, gr), (wp, wr) = getattr(x, op)(*args), getattr(m, op)(*args)
        assert gr == wr and np.array_equal(gp, wp), op
        k, v = x.export()
        assert np.array_equal(k, m.keys) and np.array_equal(v, m.vals), op
        ids, found = x.lookup(k)
        assert found.all() and np.array_equal(ids, v)
        assert not x.lookup(wp[:, 0].copy())[1].any()
    assert 0 < len(big) < 150_000 and len(small) > 0
    big.close(), small.close()


# ------------------------------------------------------------------ capacity, arguments
@pytest.mark.parametrize("by", ["key", "object"])
def test_capacity_short_by_one_changes_nothing(ctx, by):
    keys, vals, rk, rids = rc.shard_case()
    x, m = DeviceIndexR(ctx), MirrorIndexR()
    x.insert(keys, vals), m.insert(keys, vals)
    want_pairs, want = m.remove(rk) if by == "key" else m.remove_objects(rids)
    assert want > 1
    before = x.export()
    out = Guarded(want + SLACK, 16, torch.int64)
    d_a = dev(rk if by == "key" else rids)
    with pytest.raises(SdCasError) as e:
        if by == "key":
            x.x.remove(d_a, d_removed_out=out.inner, capacity=want - 1)
        else:
            x.x.remove_objects(d_a, d_removed_out=out.inner, capacity=want - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == want
    assert (out._all() == POISON).all()  # nothing was written
    after = x.export()
    assert len(x) == len(keys) and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    ids, found = x.lookup(before[0])
    assert found.all() and np.array_equal(ids, before[1])
    # with room for exactly the count it goes through
    if by == "key":
        pairs, r = x.x.remove(d_a, d_removed_out=out.inner, capacity=want)
    else:
        pairs, r = x.x.remove_objects(d_a, d_removed_out=out.inner, capacity=want)
    assert r == want and np.array_equal(host_u64(pairs).reshape(-1, 2), want_pairs)
    assert out.guards_intact() and (out.host()[want:] == POISON).all()
    assert np.array_equal(x.export()[0], m.keys) and np.array_equal(x.export()[1], m.vals)
    x.close()


def test_index_of_another_context_is_refused(ctx):
    from spacedrive_amd.device import Context
    other = Context(0)
    x = DeviceIndexR(ctx)
    k = oc.random_keys(10, 91)
    x.insert(k, k)
    d_k = dev(k)
    st = torch.cuda.current_stream().cuda_stream
    try:
        assert lib().sd_object_index_remove(other.handle, x.x.handle, d_k.data_ptr(), None, 10, None, 0, None, st) == -1
        assert lib().sd_object_index_remove_objects(other.handle, x.x.handle, d_k.data_ptr(), 10, None, 0, None,
                                                    st) == -1
        assert lib().sd_object_index_remove_hex(other.handle, x.x.handle, b"0" * 16 + b"\0", None, 1, None) == -1
        assert lib().sd_object_index_remove(ctx.handle, x.x.handle, None, None, 10, None, 0, None, st) == -1
        assert len(x) == 10
        # no output buffer and no count: the entries still go
        assert lib().sd_object_index_remove(ctx.handle, x.x.handle, d_k.data_ptr(), None, 10, None, 0, None, st) == 0
        assert len(x) == 0 and not x.lookup(k)[1].any()
    finally:
        x.close()
        other.close()


# ------------------------------------------------------------------ histories
def test_histories_equal_the_oracle(ctx):
    """The histories of the CPU suite on the device: scans through sd_dedup_group +
    sd_dedup_owners_indexed, the host cycle through sd_object_index_remove / _remove_objects /
    _insert / _lookup; after every event the exported index == {cas_id -> first live owner}."""
    total = {}
    for seed in rc.HISTORY_SEEDS:
        x = DeviceIndexR(ctx)
        for k, v in rc.History(seed).run(x).items():
            total[k] = total.get(k, 0) + v
        x.close()
    rc.check_history_counts(total)


# ------------------------------------------------------------------ several ranks
@pytest.fixture(scope="module")
def hashed(ctx):
    from spacedrive_amd import synth
    n = 12000
    sizes, cids, twins = synth.library(0, n, n, dup_frac=0.3)
    return sizes, stage_and_hash(ctx, sizes, cids, twins)


@pytest.mark.parametrize("R", [2, 3])
def test_remove_objects_on_every_rank_equals_the_unsharded_index(ctx, hashed, R):
    """sd_cas_dedup_mgpu_indexed over R in-process ranks: scan the first half, insert the new
    heads, remove_objects with the SAME id list on every rank (each shard drops what it
    holds), scan the second half.  Exports, dropped pairs, and the second scan's records,
    owners, existing flags and new heads, concatenated in rank order, equal the single
    unsharded index's."""
    from spacedrive_amd.device import Comm, CommGroup, Context
    sizes, h = hashed
    n, half = len(sizes), len(sizes) // 2
    d_hash = torch.from_numpy(h.reshape(-1).copy()).cuda()
    d_valid = torch.from_numpy((sizes != 0).astype(np.uint8)).cuda()

    # the unsharded run
    whole = ObjectIndex(ctx)
    _, _, _, _, _, new1 = dedup.dedup_shard(ctx, d_hash[:half * 32], d_valid[:half], half, 0, index=whole)
    assert whole.insert(new1[:, 0].contiguous(), new1[:, 1].contiguous()) == len(new1) > 100
    # every third Object, three of them twice, and fifty ids no Object has
    rm = torch.cat([new1[::3, 1], new1[:9:3, 1], torch.arange(n, n + 50, device="cuda")]).contiguous()
    w_pairs, w_r = whole.remove_objects(rm)
    assert w_r == len(new1[::3])
    wk, wv = whole.export()
    w_recs, _, _, w_owner, w_ex, w_new = dedup.dedup_shard(ctx, d_hash[half * 32:], d_valid[half:], n - half, half,
                                                           index=whole)
    assert bool(w_ex.any()) and not bool(w_ex.all()) and len(w_new)

    group = CommGroup(R)
    ctxs = [Context(0) for _ in range(R)]
    comms = [Comm(ctxs[r], None, R, r, group=group) for r in range(R)]
    idx = [ObjectIndex(ctxs[r], R, r) for r in range(R)]
    runners = [dedup.RcclDedup(ctxs[r], comms[r], d_hash.device, capacity=n) for r in range(R)]
    torch.cuda.synchronize()

    def scan(r, lo_all, hi_all):
        cuts = [lo_all + (hi_all - lo_all) * q // R for q in range(R + 1)]
        lo, hi = cuts[r], cuts[r + 1]
        st = torch.cuda.Stream()
        res = runners[r](d_hash[lo * 32:], d_valid[lo:], hi - lo, lo, stream=st, index=idx[r])
        st.synchronize()
        return [t.clone() if isinstance(t, torch.Tensor) else t for t in res]

    try:
        first = _run_ranks(R, lambda r: scan(r, 0, half))
        for r in range(R):
            new = first[r][5]
            assert idx[r].insert(new[:, 0].contiguous(), new[:, 1].contiguous()) == len(new)
        assert torch.equal(torch.cat([first[r][5] for r in range(R)]), new1)
        dropped = [idx[r].remove_objects(rm) for r in range(R)]  # not collective: one rank after the other
        assert sum(d[1] for d in dropped) == w_r and all(d[1] > 0 for d in dropped)
        assert torch.equal(torch.cat([d[0] for d in dropped]), w_pairs)
        for r in range(R):
            assert np.all(dest_of(host_u64(dropped[r][0][:, 0].contiguous()), R) == r)
        exports = [idx[r].export() for r in range(R)]
        assert torch.equal(torch.cat([e[0] for e in exports]), wk) and torch.equal(torch.cat([e[1] for e in exports]), wv)
        second = _run_ranks(R, lambda r: scan(r, half, n))
        for j, want in ((0, w_recs), (3, w_owner), (4, w_ex), (5, w_new)):
            assert torch.equal(torch.cat([second[r][j] for r in range(R)]), want), j
    finally:
        whole.close()
        for x in idx:
            x.close()
        for c in comms:
            c.close()
        group.close()
        for c in ctxs:
            c.close()
