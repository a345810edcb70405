"""The device-resident Object index (include/sd_cas.h, csrc/object_index.hip) -- run on an
MI355X: -m gpu.  Everything is bit-exact against the numpy mirror (dedup.index_insert_host /
owners_indexed_host), which tests/test_object_index.py pins to the oracle's restatement of
file_identifier/mod.rs:136-333; the end-to-end test goes to the oracle directly.  Outputs sit
between 0xA5 guard rows and are pre-filled, so a write outside the rows a call owns, or a
missing one, shows."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup, synth  # noqa: E402
from spacedrive_amd._native import SdCasError  # noqa: E402
from spacedrive_amd.dedup import dest_of, group_host, keys_from_hashes  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests.test_object_index import MirrorIndex  # noqa: E402

U = np.uint64
G = 4  # guard rows either side of an output
POISON = 0xA5
NT = 16


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


class Guarded:
    """`rows` rows of `row_bytes` device bytes between G guard rows, all 0xA5."""

    def __init__(self, rows: int, row_bytes: int, dtype=torch.uint8):
        self.rows, self.row_bytes = rows, row_bytes
        self.raw = torch.full(((rows + 2 * G) * row_bytes,), POISON, dtype=torch.uint8, device="cuda")
        self.inner = self.raw[G * row_bytes:(G + rows) * row_bytes]
        if dtype != torch.uint8:
            self.inner = self.inner.view(dtype)

    def _all(self) -> np.ndarray:
        torch.cuda.synchronize()
        return self.raw.cpu().numpy().reshape(-1, self.row_bytes)

    def host(self) -> np.ndarray:
        return self._all()[G:G + self.rows]

    def guards_intact(self) -> bool:
        a = self._all()
        return bool((a[:G] == POISON).all() and (a[G + self.rows:] == POISON).all())


def dev(a: np.ndarray) -> torch.Tensor:
    """a u64 / i64 array as an int64 device tensor (the bit pattern)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def host_u64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(U)


def build(ctx, keys, vals, nparts=1, part=0):
    """(device index, mirror) holding the same pairs"""
    x, m = ObjectIndex(ctx, nparts, part), MirrorIndex(nparts, part)
    assert x.insert(dev(keys), dev(vals)) == m.insert(keys, vals)
    return x, m


def assert_equals_mirror(x: ObjectIndex, m: MirrorIndex, what=""):
    k, v = x.export()
    k, v = host_u64(k), host_u64(v)
    assert len(x) == len(m) == len(k), what
    assert np.all(k[1:] > k[:-1]), what  # strictly ascending, unsigned
    assert np.array_equal(k, m.keys) and np.array_equal(v, m.vals), what
    ids, found = x.lookup(dev(k))  # the directory, indirectly: every exported key is found
    assert bool(found.all()) and np.array_equal(host_u64(ids), v), what


# ------------------------------------------------------------------ lookup
@pytest.mark.parametrize("kind", ["uniform", "edges", "shared_prefix"])
def test_lookup_sweep(ctx, kind):
    """k_index_lookup at every index size x query count of the case lists: present keys,
    absent ones between two keys, below the minimum, above the maximum; keys on both sides
    of 2^63, neighbours, and a set that one directory bucket holds entirely."""
    compared = 0
    for n in oc.INDEX_SIZES:
        keys = oc.key_sets(n)[kind]
        vals = oc.vals_for(keys, 31)
        x, m = build(ctx, keys, vals)
        assert len(x) == n
        for q_n in oc.QUERY_COUNTS:
            q = oc.queries(keys, q_n)
            want_ids, want_found = m.lookup(q)
            d_ids, d_found = Guarded(q_n, 8, torch.int64), Guarded(q_n, 1)
            x.lookup(dev(q) if q_n else torch.zeros(1, dtype=torch.int64, device="cuda"), d_ids.inner, d_found.inner,
                     m=q_n)
            assert d_ids.guards_intact() and d_found.guards_intact(), (n, q_n)
            assert np.array_equal(d_found.host().reshape(-1), want_found), (n, q_n)
            assert np.array_equal(d_ids.host().view(U).reshape(-1), want_ids), (n, q_n)
            if n and q_n >= 63:
                assert want_found.any() and not want_found.all()
            compared += 1
        x.close()
    assert compared == len(oc.INDEX_SIZES) * len(oc.QUERY_COUNTS) == 77


# ------------------------------------------------------------------ insert
@pytest.mark.parametrize("case", sorted(oc.insert_cases()))
def test_insert_cases_equal_mirror(ctx, case):
    """The CPU case list on the device: export after each step == the mirror; count; keys
    strictly ascending; every exported key found."""
    x, m = ObjectIndex(ctx), MirrorIndex()
    for step, (keys, vals) in enumerate(oc.insert_cases()[case]):
        assert x.insert(dev(keys), dev(vals)) == m.insert(keys, vals), (case, step)
        assert_equals_mirror(x, m, (case, step))
    assert x.insert(torch.zeros(0, dtype=torch.int64, device="cuda"),
                    torch.zeros(0, dtype=torch.int64, device="cuda")) == 0  # m == 0: a no-op
    assert_equals_mirror(x, m, case)
    x.close()


def test_insert_shard_filter_and_hex(ctx):
    """Every part of nparts 1, 2, 3, 8 takes exactly its keys from the same dump (their union
    is the unsharded index), and sd_object_index_insert_hex reads the DB's strings."""
    keys = np.concatenate([oc.random_keys(3000, 21), oc.edge_keys()])
    vals = oc.vals_for(keys, 22)
    whole, wm = build(ctx, keys, vals)
    assert_equals_mirror(whole, wm)
    d_k, d_v = dev(keys), dev(vals)
    for nparts in oc.NPARTS:
        got = []
        for part in range(nparts):
            x, m = ObjectIndex(ctx, nparts, part), MirrorIndex(nparts, part)
            assert x.insert(d_k, d_v) == m.insert(keys, vals) == int((dest_of(keys, nparts) == part).sum())
            assert_equals_mirror(x, m, (nparts, part))
            got.append(m.keys)
            x.close()
        assert np.array_equal(np.concatenate(got), wm.keys)
    hx = ObjectIndex(ctx)
    assert hx.insert_hex(["%016x" % int(k) for k in keys], vals) == len(keys)
    assert_equals_mirror(hx, wm, "hex")
    with pytest.raises(SdCasError):
        hx.insert_hex(["00000000000000FG"], [1])
    hx.close()
    whole.close()


def test_large_insert_then_small_amid_random_data(ctx):
    """Bulk build of 300 000, then inserts of 70 000 (half present) and of 5 with the scratch
    of the larger calls stale, the index's buffers allocated between tensors of random data:
    export == the mirror each time."""
    junk = [torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda") for _ in range(3)]
    x, m = ObjectIndex(ctx), MirrorIndex()
    junk.append(torch.randint(0, 255, (1 << 20,), dtype=torch.uint8, device="cuda"))
    a = oc.random_keys(300_000, 51)
    b = np.concatenate([oc.random_keys(35_000, 52), a[:35_000]])
    for keys, salt in ((a, 1), (b, 2), (oc.random_keys(5, 53), 3), (a[:7], 4)):
        vals = oc.vals_for(keys, salt)
        junk.append(torch.randint(0, 255, (1 << 18,), dtype=torch.uint8, device="cuda"))
        assert x.insert(dev(keys), dev(vals)) == m.insert(keys, vals)
        assert_equals_mirror(x, m, salt)
    assert len(x) == 335_005 and oc.dir_bits(len(x)) == 15
    # the owners' per-workgroup counts after a larger call, on records that hit this index
    for n_rec, seed in ((50_000, 54), (300, 55)):
        r, rep = grouped_records(n_rec, seed)
        r[::3, 0] = a[:len(r[::3])].view(np.int64)
        r, rep, _ = group_host(r)
        owner, ex, new, n_new = run_owners(x, r, rep, 100)
        w_owner, w_ex, w_new = m.owners(r, rep, 100)
        assert np.array_equal(owner, w_owner) and np.array_equal(ex, w_ex) and np.array_equal(new, w_new), n_rec
        assert ex.any() and not ex.all() and n_new == len(w_new) > 0
    x.close()


# ------------------------------------------------------------------ owners
def grouped_records(m: int, seed: int):
    """m records grouped on the host: full-range keys with groups of equal ones, indices in
    no order over many identifier steps -> (records int64 [m, 2], rep int64 [m])."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 64, m // 2 + 1, dtype=U)
    keys = pool[rng.integers(0, len(pool), m)] if m else np.zeros(0, U)
    recs = np.stack([keys.view(np.int64), rng.permutation(m).astype(np.int64) * 3 + 5], axis=1).reshape(m, 2)
    r, rep, _ = group_host(recs)
    return r.reshape(m, 2), rep


def run_owners(x, r, rep, chunk, fill=POISON):
    m = len(r)
    d_owner, d_ex, d_new = Guarded(m, 8, torch.int64), Guarded(m, 1), Guarded(m, 16, torch.int64)
    d_n = Guarded(1, 8, torch.int64)
    d_r = dev(r.reshape(-1)) if m else torch.zeros(2, dtype=torch.int64, device="cuda")
    d_rep = dev(rep) if m else torch.zeros(1, dtype=torch.int64, device="cuda")
    x.owners(d_r, m, d_rep, d_owner.inner, d_ex.inner, d_new.inner, d_n.inner, chunk_size=chunk)
    for g in (d_owner, d_ex, d_new, d_n):
        assert g.guards_intact(), m  # no row >= m changes, in d_new_out either
    if m:
        assert np.array_equal(host_u64(d_r).view(np.int64), r.reshape(-1))  # the input is not written
    n_new = int(d_n.host().view(np.int64)[0, 0])
    return (d_owner.host().view(U).reshape(-1), d_ex.host().reshape(-1),
            d_new.host().view(U).reshape(-1, 2)[:n_new], n_new)


@pytest.mark.parametrize("m,chunk", [(0, 100), (1, 100), (4099, 7), (100_000, 100)])
def test_owners_indexed_equals_mirror(ctx, m, chunk):
    """sd_dedup_owners_indexed at hit shares 0, ~1/2 and 1: owners, existing and the new heads
    (ascending, == the mirror's), only m rows written, the head flag gone from d_existing."""
    r, rep = grouped_records(m, 70 + m)
    uniq = np.unique(r[:, 0].view(U)) if m else np.zeros(0, U)
    other = oc.random_keys(1000, 71)
    for share, known in (("0", other), ("1/2", np.concatenate([uniq[::2], other])), ("1", uniq)):
        x, mir = build(ctx, known, oc.vals_for(known, 72))
        owner, ex, new, n_new = run_owners(x, r, rep, chunk)
        w_owner, w_ex, w_new = mir.owners(r, rep, chunk)
        assert n_new == len(w_new), (m, share)
        assert np.array_equal(owner, w_owner) and np.array_equal(ex, w_ex), (m, share)
        assert np.array_equal(new, w_new) and np.all(new[1:, 0] > new[:-1, 0]), (m, share)
        if m > 1:
            assert {"0": not ex.any(), "1/2": ex.any() and not ex.all(), "1": ex.all()}[share]
        x.close()


def test_owners_indexed_null_index_is_dedup_owners(ctx):
    """index = NULL: the owners are sd_dedup_owners' on the same records, and d_existing,
    d_new_out and d_n_new are not touched."""
    from spacedrive_amd._native import check, lib
    m = 4099
    r, rep = grouped_records(m, 81)
    d_r, d_rep = dev(r.reshape(-1)), dev(rep)
    want = torch.empty(m, dtype=torch.int64, device="cuda")
    ctx.dedup_owners(d_r, m, d_rep, want, chunk_size=7)
    d_owner, d_ex, d_new, d_n = Guarded(m, 8, torch.int64), Guarded(m, 1), Guarded(m, 16), Guarded(1, 8)
    check(lib().sd_dedup_owners_indexed(ctx.handle, None, d_r.data_ptr(), m, d_rep.data_ptr(), 7,
                                        d_owner.inner.data_ptr(), d_ex.inner.data_ptr(), d_new.inner.data_ptr(),
                                        d_n.inner.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(d_owner.host().view(np.int64).reshape(-1), want.cpu().numpy())
    for g in (d_ex, d_new, d_n):
        assert (g._all() == POISON).all()
    assert d_owner.guards_intact()


# ------------------------------------------------------------------ end to end
def stage_and_hash(ctx, sizes, cids, twins):
    from spacedrive_amd.device import stage_plan
    n = len(sizes)
    ext, total = stage_plan(sizes)
    d_staged = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
    ctx.synth_stage_cas(dev(sizes.astype(U)), dev(cids.astype(U)), torch.from_numpy(twins.astype(np.int32)).cuda(),
                        d_ext, n, d_staged)
    out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    b = ctx.cas_batch(ext)
    b.run(d_staged, out)
    torch.cuda.synchronize()
    b.close()
    return out.cpu().numpy().reshape(-1, 32)


@pytest.fixture(scope="module")
def library(ctx):
    n = 30000
    sizes, cids, twins = synth.library(0, n, n, dup_frac=0.3)
    return sizes, cids, twins, stage_and_hash(ctx, sizes, cids, twins)


def test_two_scans_end_to_end_equal_the_oracle_replay(ctx, oracle_native):
    """Hash 20 000 synthetic files on the GPU; the first 10 000 go through dedup_shard from an
    empty index, the new heads are inserted (Object id := the creating file's index), the
    second 10 000 go through with global_base = 10 000: the combined owners equal
    identifier_replay of the oracle's cas_ids."""
    from oracle.identifier_spec import identifier_replay
    n, half = 20000, 10000
    sizes, cids, twins = synth.library(0, n, n, dup_frac=0.3)
    h = stage_and_hash(ctx, sizes, cids, twins)
    valid = (sizes != 0).astype(np.uint8)
    x = ObjectIndex(ctx)
    got = np.arange(n)
    linked = 0
    for base in (0, half):
        d_hash = torch.from_numpy(h[base:base + half].copy()).cuda()
        d_valid = torch.from_numpy(valid[base:base + half].copy()).cuda()
        recs, rep, ng, owner, existing, new = dedup.dedup_shard(ctx, d_hash, d_valid, half, base, index=x)
        got[recs[:, 1].cpu().numpy()] = owner.cpu().numpy()
        linked += int(existing.sum().item())
        assert len(new) + int(existing[torch.cat([torch.ones(1, dtype=torch.bool, device="cuda"),
                                                   recs[1:, 0] != recs[:-1, 0]])].sum().item()) == ng
        assert x.insert(new[:, 0].contiguous(), new[:, 1].contiguous()) == len(new)
    assert linked > 0
    ids = oracle_native.cas_ids_synth(sizes, cids, twins, nthreads=NT)
    cas = [None if sizes[i] == 0 else ids[i].tobytes().hex() for i in range(n)]
    want, _ = identifier_replay(cas)
    assert got.tolist() == want
    x.close()


# ------------------------------------------------------------------ multi-rank
def _run_ranks(R, fn):
    """fn(rank) on R threads (ctypes releases the GIL inside the library); results by rank,
    the first exception re-raised."""
    out, errs = [None] * R, []

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(R)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=180)
    assert not any(t.is_alive() for t in ts), "a rank thread did not finish"
    if errs:
        raise errs[0]
    return out


@pytest.mark.parametrize("R", [2, 3])
def test_dedup_mgpu_indexed_in_process_ranks(ctx, library, R):
    """sd_cas_dedup_mgpu_indexed over R in-process ranks on one GPU, 30 000 files, every rank
    handed the same dump of known Objects into its own shard of the index: each rank's output
    == the mirror for its prefix range; index = NULL on all ranks == sd_cas_dedup_mgpu; a
    rank with a wrongly sharded index makes EVERY rank return SD_ERR_INVALID together."""
    from spacedrive_amd.device import Comm, CommGroup, Context
    sizes, cids, twins, h = library
    n = len(sizes)
    valid = sizes != 0
    keys = keys_from_hashes(h)
    cuts = [0] + [int(c) for c in np.cumsum(np.random.default_rng(R).dirichlet(np.ones(R)) * n)[:-1]] + [n]
    all_recs = np.stack([keys[valid].view(np.int64), np.arange(n)[valid]], axis=1)
    dst = dest_of(all_recs[:, 0].view(U), R)
    known = np.unique(keys[valid])[::2]  # the library already has an Object for every other cas_id
    known_ids = oc.vals_for(known, 91)
    group = CommGroup(R)
    ctxs = [Context(0) for _ in range(R)]
    comms = [Comm(ctxs[r], None, R, r, group=group) for r in range(R)]
    d_hash = torch.from_numpy(h.reshape(-1).copy()).cuda()
    d_valid = torch.from_numpy(valid.astype(np.uint8)).cuda()
    d_known, d_known_ids = dev(known), dev(known_ids)
    idx = [ObjectIndex(ctxs[r], R, r) for r in range(R)]
    mirrors = [MirrorIndex(R, r) for r in range(R)]
    for r in range(R):
        assert idx[r].insert(d_known, d_known_ids) == mirrors[r].insert(known, known_ids) > 0
    wrong = ObjectIndex(ctxs[1], R, 0)  # rank 1 holding rank 0's shard
    torch.cuda.synchronize()

    def rank_call(r, index):
        lo, hi = cuts[r], cuts[r + 1]
        st = torch.cuda.Stream()
        runner = dedup.RcclDedup(ctxs[r], comms[r], d_hash.device, capacity=n)
        if index == "null":  # sd_cas_dedup_mgpu_indexed itself with index = NULL and no extra outputs
            m, ng, nn = ctxs[r].dedup_mgpu_indexed(comms[r], d_hash[lo * 32:], d_valid[lo:], hi - lo, lo,
                                                   runner.records, runner.rep, runner.owner, n, None, None, None,
                                                   stream=st)
            st.synchronize()
            return [runner.records[:m].cpu().numpy(), runner.rep[:m].cpu().numpy(), ng,
                    runner.owner[:m].cpu().numpy()], nn
        try:
            res = runner(d_hash[lo * 32:], d_valid[lo:], hi - lo, lo, stream=st, index=index(r))
        except SdCasError as e:
            return e.rc
        st.synchronize()
        return [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in res]

    try:
        got = _run_ranks(R, lambda r: rank_call(r, lambda q: idx[q]))
        plain = _run_ranks(R, lambda r: rank_call(r, lambda q: None))
        null = _run_ranks(R, lambda r: rank_call(r, "null"))
        bad = _run_ranks(R, lambda r: rank_call(r, lambda q: wrong if q == 1 else idx[q]))
        assert bad == [-1] * R  # SD_ERR_INVALID on every rank, nobody left waiting
        again = _run_ranks(R, lambda r: rank_call(r, lambda q: idx[q]))  # the communicators still work
        for r in range(R):
            gr, grep, gng = group_host(all_recs[dst == r])
            w_owner, w_ex, w_new = mirrors[r].owners(gr, grep, 100)
            for recs, rep, ng, own, ex, new in (got[r], again[r]):
                assert ng == gng and np.array_equal(recs, gr) and np.array_equal(rep, grep), r
                assert np.array_equal(own.view(U), w_owner) and np.array_equal(ex, w_ex), r
                assert np.array_equal(new.view(U), w_new), r
            assert w_ex.any() and not w_ex.all() and len(w_new)
            p_recs, p_rep, p_ng, p_own = plain[r]
            want_plain = np.where(gr[:, 1] // 100 == grep // 100, gr[:, 1], grep)
            assert p_ng == gng and np.array_equal(p_recs, gr) and np.array_equal(p_own, want_plain), r
            (n_recs, n_rep, n_ng, n_own), n_new = null[r]
            assert n_new == 0 and n_ng == p_ng and np.array_equal(n_recs, p_recs), r
            assert np.array_equal(n_rep, p_rep) and np.array_equal(n_own, p_own), r
    finally:
        wrong.close()
        for x in idx:
            x.close()
        for c in comms:
            c.close()
        group.close()
        for c in ctxs:
            c.close()
