"""The dedup exchange over ranks at empty, skewed and unordered shards -- run on an MI355X: -m gpu.

sd_cas_dedup_mgpu / sd_cas_dedup_mgpu_indexed over R = 2, 3 and 8 in-process ranks on one GPU
(RCCL refuses two ranks on one device), every case of tests/exchange_cases.py on ONE set of
communicators per R, in an order that shrinks and regrows each rank's send buffer.  Every output
sits between 0xA5 guard rows with a capacity of exactly what the rank receives -- none at all, and
NULL outputs, on a rank that receives nothing -- and is compared bit for bit with the module's
numpy expectation, which tests/test_exchange_cases.py pins to the oracle's identifier replay.
The split checksum over ranks with idle ranks closes the module.

Hang safety: every rank thread makes every collective call of a case, the only refusals provoked
are the ones all ranks reach together (capacity), and a rank thread that does not come back fails
its test once and every later one without starting anything."""
import hashlib
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError  # noqa: E402
from spacedrive_amd.device import Comm, CommGroup, Context, ObjectIndex, SplitChecksum  # noqa: E402
from spacedrive_amd.split import cpu_leaves, cpu_root  # noqa: E402
from tests import exchange_cases as xc  # noqa: E402
from tests import object_index_cases as oc  # noqa: E402
from tests.test_object_index import MirrorIndex  # noqa: E402

U = np.uint64
G = 4  # guard rows either side of an output
POISON = 0xA5
NT = 16
SPARE = 5
JOIN_S = 150  # past the in-process barrier's own bound, so a missing rank shows as its SD_ERR_COMM

_hung = []  # names of the calls that left a rank thread behind


@pytest.fixture(scope="module", autouse=True)
def _in_tree_library():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()


@pytest.fixture(params=[0, 1])
def dedup_variant(request):
    """sd_dedup_group: 0 = rocPRIM radix sort, 1 = LDS buckets (the default)."""
    from spacedrive_amd._native import lib
    assert lib().sd_cas_set_tuning(b"dedup_variant", request.param) == 0
    yield request.param
    lib().sd_cas_set_tuning(b"dedup_variant", 1)  # the default


class Guarded:
    """`rows` rows of `row_bytes` device bytes between G guard rows, all 0xA5; the calls get
    `inner` (None when there are no rows: the call gets NULL)."""

    def __init__(self, rows: int, row_bytes: int):
        self.rows, self.row_bytes = rows, row_bytes
        self.raw = torch.full(((rows + 2 * G) * row_bytes,), POISON, dtype=torch.uint8, device="cuda")
        self.inner = self.raw[G * row_bytes:(G + rows) * row_bytes] if rows else None

    def read(self):
        """(inner rows on the host, guards intact) from one download"""
        torch.cuda.synchronize()
        a = self.raw.cpu().numpy().reshape(-1, self.row_bytes)
        return a[G:G + self.rows], bool((a[:G] == POISON).all() and (a[G + self.rows:] == POISON).all())


def untouched(rows: np.ndarray) -> bool:
    return bool((rows == POISON).all())


def dev_u64(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def run_ranks(R: int, fn, what: str):
    """fn(rank) on R threads (ctypes releases the GIL inside the library) -> results by rank, the
    first exception re-raised.  A thread still alive after JOIN_S fails this test, and every later
    call fails before it starts a thread: nothing is tried again."""
    if _hung:
        pytest.fail(f"not started: a rank thread never came back from {_hung[0]}")
    out, errs = [None] * R, []

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(R)]
    for t in ts:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in ts:
        t.join(timeout=max(deadline - time.monotonic(), 0.0))
    if any(t.is_alive() for t in ts):
        _hung.append(what)
        pytest.fail(f"a rank thread did not finish {what}")
    if errs:
        raise errs[0]
    return out


class Ranks:
    """One communicator group of R in-process ranks on device 0, with a context, a communicator
    and a stream per rank, for every case of that R."""

    def __init__(self, R: int):
        self.R = R
        self.group = CommGroup(R)
        self.ctxs = [Context(0) for _ in range(R)]
        self.comms = [Comm(self.ctxs[r], None, R, r, group=self.group) for r in range(R)]
        self.streams = [torch.cuda.Stream() for _ in range(R)]

    def close(self):
        if _hung:  # a thread may still be inside the library with these handles
            return
        for c in self.comms:
            c.close()
        self.group.close()
        for c in self.ctxs:
            c.close()


@pytest.fixture(scope="module", params=xc.RANKS, ids=lambda R: f"R{R}")
def ranks(request):
    rk = Ranks(request.param)
    yield rk
    rk.close()


class Inputs:
    """A case's hash rows and masks on the device, one tensor per rank (None for n = 0 and for
    d_valid == NULL), and the sha256 of what was uploaded."""

    def __init__(self, c: xc.Case):
        self.hash = [torch.from_numpy(h.copy()).cuda() if len(h) else None for h in c.hashes]
        self.valid = [torch.from_numpy(v.copy()).cuda() if v is not None and len(v) else None for v in c.valid]
        self.sums = [(hashlib.sha256(h.tobytes()).hexdigest(), None if v is None else hashlib.sha256(v.tobytes()).hexdigest())
                     for h, v in zip(c.hashes, c.valid)]

    def unchanged(self, r: int) -> bool:
        h, v = self.hash[r], self.valid[r]
        got_h = hashlib.sha256(b"" if h is None else h.cpu().numpy().tobytes()).hexdigest()
        got_v = None if self.sums[r][1] is None else hashlib.sha256(b"" if v is None else v.cpu().numpy().tobytes()).hexdigest()
        return (got_h, got_v) == self.sums[r]


class Outputs:
    """One rank's guarded outputs at a capacity."""

    def __init__(self, cap: int, indexed: bool = False):
        self.cap = cap
        self.records, self.rep, self.owner = Guarded(cap, 16), Guarded(cap, 8), Guarded(cap, 8)
        self.existing, self.new = (Guarded(cap, 1), Guarded(cap, 16)) if indexed else (None, None)

    def all(self):
        return [g for g in (self.records, self.rep, self.owner, self.existing, self.new) if g is not None]


def call_ranks(rk: Ranks, c: xc.Case, inp: Inputs, outs, index=None):
    """The collective call on every rank -> per rank ("ok", m, n_groups, n_new) or ("refused", rc,
    needed)."""
    def rank(r):
        base, n, _ = c.shards[r]
        o = outs[r]
        try:
            if index is None:
                m, ng = rk.ctxs[r].dedup_mgpu(rk.comms[r], inp.hash[r], inp.valid[r], n, base, o.records.inner,
                                              o.rep.inner, o.owner.inner, o.cap, xc.CHUNK, rk.streams[r])
                nn = None
            else:
                m, ng, nn = rk.ctxs[r].dedup_mgpu_indexed(rk.comms[r], inp.hash[r], inp.valid[r], n, base,
                                                          o.records.inner, o.rep.inner, o.owner.inner, o.cap,
                                                          index[r], o.existing.inner, o.new.inner, xc.CHUNK,
                                                          rk.streams[r])
        except SdCasError as e:
            return "refused", e.rc, e.needed
        rk.streams[r].synchronize()
        return "ok", m, ng, nn
    return run_ranks(rk.R, rank, c.name)


def i64(rows: np.ndarray) -> np.ndarray:
    """[k, 8 j] bytes -> int64 [k, j]"""
    return np.ascontiguousarray(rows).view(np.int64)


def check_plain(c: xc.Case, inp: Inputs, outs, got, spare: int, tag=""):
    """m, n_groups, records, rep and owner of every rank equal the expectation; the rows past m, the
    guards and the inputs are as they were."""
    for r, w in enumerate(c.want):
        at = (c.name, r, tag)
        assert got[r][:3] == ("ok", w.m, w.n_groups), (at, got[r])
        assert outs[r].cap == w.m + spare
        recs, ok_a = outs[r].records.read()
        rep, ok_b = outs[r].rep.read()
        own, ok_c = outs[r].owner.read()
        assert ok_a and ok_b and ok_c, at
        assert np.array_equal(i64(recs[:w.m]).reshape(-1, 2), w.records), at
        assert np.array_equal(i64(rep[:w.m]).reshape(-1), w.rep), at
        assert np.array_equal(i64(own[:w.m]).reshape(-1), w.owner), at
        assert untouched(recs[w.m:]) and untouched(rep[w.m:]) and untouched(own[w.m:]), at
        assert len(recs) - w.m == spare
        assert inp.unchanged(r), at


def run_case(rk: Ranks, c: xc.Case, tag=""):
    """The case at exactly each rank's need (NULL outputs where that is 0), then once more with five
    spare rows, which stay 0xA5."""
    inp = Inputs(c)
    for spare in (0, SPARE):
        outs = [Outputs(need + spare) for need in c.need]
        check_plain(c, inp, outs, call_ranks(rk, c, inp, outs), spare, tag)


def test_every_case_at_exact_capacity(ranks):
    """Every case of this R, in gpu_order, on the same communicators."""
    t0 = time.perf_counter()
    ran = 0
    for s in xc.gpu_order(ranks.R):
        run_case(ranks, xc.case(s))
        ran += 1
    assert ran == xc.CASES_PER_R[ranks.R]  # the count tests/test_exchange_cases.py asserts
    print(f"\nexchange sweep R={ranks.R}: {ran} cases x 2 calls in {time.perf_counter() - t0:.2f} s")


def test_both_variants_on_unordered_and_overflowing_cases(ranks, dedup_variant):
    """The descending, rotated and one_group cases under dedup_variant 0 and 1: the radix path has
    to be told that the records are out of index order (and is, by plan.ascending and again in the
    overflow fallback); the bucket path orders every bucket itself."""
    t0 = time.perf_counter()
    ran = 0
    for s in xc.variant_specs(ranks.R):
        run_case(ranks, xc.case(s), f"variant {dedup_variant}")
        ran += 1
    assert ran == {2: 7, 3: 8, 8: 9}[ranks.R]
    print(f"\nvariant {dedup_variant} R={ranks.R}: {ran} cases x 2 calls in {time.perf_counter() - t0:.2f} s")


def test_capacity_one_short_refuses_every_rank(ranks):
    """The rank with the largest need one row short, every other rank exact: every rank returns
    SD_ERR_CAPACITY with its own need, no output row is written, and the same case then passes on
    the same communicators."""
    ran = 0
    for s in xc.capacity_specs(ranks.R):
        c = xc.case(s)
        inp = Inputs(c)
        short = int(np.argmax(c.need))
        assert c.need[short] >= 1
        outs = [Outputs(need - (r == short)) for r, need in enumerate(c.need)]
        got = call_ranks(ranks, c, inp, outs)
        for r in range(ranks.R):
            assert got[r] == ("refused", SD_ERR_CAPACITY, c.need[r]), (c.name, r, got[r])
            for g in outs[r].all():
                rows, ok = g.read()
                assert ok and untouched(rows), (c.name, r)
            assert inp.unchanged(r)
        run_case(ranks, c, "after the refusal")
        ran += 1
    assert ran == 2


def test_indexed_call(ranks):
    """sd_cas_dedup_mgpu_indexed with every other key known to the library: owner, existing, the
    new heads and n_new of every rank against the mirror of its shard; a rank that received nothing
    reports no new head."""
    ran = 0
    for s in xc.indexed_specs(ranks.R):
        c = xc.case(s)
        R = c.R
        known = np.unique(np.ascontiguousarray(c.all_recs[:, 0]).view(U))[::2]
        ids = oc.vals_for(known, 91)
        d_known, d_ids = dev_u64(known), dev_u64(ids)
        index = [ObjectIndex(ranks.ctxs[r], R, r) for r in range(R)]
        mirrors = [MirrorIndex(R, r) for r in range(R)]
        try:
            taken = [index[r].insert(d_known, d_ids) for r in range(R)]
            assert taken == [mirrors[r].insert(known, ids) for r in range(R)] and sum(taken) == len(known), c.name
            inp = Inputs(c)
            for spare in (0, SPARE):
                outs = [Outputs(need + spare, indexed=True) for need in c.need]
                got = call_ranks(ranks, c, inp, outs, index)
                for r, w in enumerate(c.want):
                    at = (c.name, r, spare)
                    w_owner, w_ex, w_new = mirrors[r].owners(w.records, w.rep, xc.CHUNK)
                    assert got[r] == ("ok", w.m, w.n_groups, len(w_new)), (at, got[r])
                    assert w.m or got[r][3] == 0
                    reads = [g.read() for g in outs[r].all()]
                    assert all(ok for _, ok in reads), at
                    recs, rep, own, ex, new = (rows for rows, _ in reads)
                    assert np.array_equal(i64(recs[:w.m]).reshape(-1, 2), w.records), at
                    assert np.array_equal(i64(rep[:w.m]).reshape(-1), w.rep), at
                    assert np.array_equal(i64(own[:w.m]).reshape(-1).view(U), w_owner), at
                    assert np.array_equal(ex[:w.m].reshape(-1), w_ex), at
                    assert np.array_equal(i64(new[:len(w_new)]).reshape(-1, 2).view(U), w_new), at
                    assert all(untouched(x[w.m:]) for x in (recs, rep, own, ex)) and untouched(new[len(w_new):]), at
                    assert inp.unchanged(r), at
                if s.dist == "uniform":
                    assert all(len(mirrors[r].owners(w.records, w.rep, xc.CHUNK)[2]) for r, w in enumerate(c.want))
        finally:
            if not _hung:
                for x in index:
                    x.close()
        ran += 1
    assert ran == (6 if ranks.R in (2, 8) else 3)


# ------------------------------------------------------------------ split checksums, idle ranks
@pytest.mark.parametrize("R", xc.SPLIT_RANKS)
def test_split_checksum_mgpu_idle_ranks(R, oracle_native):
    """sd_split_checksum_mgpu over R in-process ranks for files of fewer blocks than ranks: the idle
    ranks still take part in the in-place all-gather, and a one-block file's root is slot 0, which
    every rank but 0 has from the all-gather alone.  CV buffers of cv_bytes pre-filled with 0xA5:
    every rank's root is the oracle's BLAKE3, the slots below nb are cpu_leaves' on every rank, and
    the slots from nb on are still 0xA5 -- the padding is never read, or the root would differ."""
    cid = 903
    rk = Ranks(R)
    ran = 0
    try:
        for total, _, nb, q, cv_bytes, plan in [c for c in xc.split_cases() if c[1] == R]:
            host = np.zeros(total + 128, np.uint8)
            if total:
                host[:total] = np.frombuffer(oracle_native.synth_bytes(cid, 0, 0, total), np.uint8)
            want = oracle_native.checksum_synth_mt(total, cid, 0, nthreads=NT)
            leaves = cpu_leaves(host, total, 1, 0, nthreads=NT).reshape(-1, 32)
            assert len(leaves) == nb and cpu_root(leaves.reshape(-1), total) == want, total
            d = torch.from_numpy(host).cuda()
            splits = [SplitChecksum(rk.ctxs[r], total, R, r) for r in range(R)]
            assert [(s.offset, s.len, s.cv_bytes) for s in splits] == [(o, n, cv_bytes) for o, n, _, _ in plan]
            cvs = [Guarded(cv_bytes // 32, 32) for _ in range(R)]
            roots = [Guarded(1, 32) for _ in range(R)]
            torch.cuda.synchronize()

            def rank(r):
                splits[r].mgpu(rk.comms[r], d[splits[r].offset:], cvs[r].inner, roots[r].inner, stream=rk.streams[r])
                rk.streams[r].synchronize()

            run_ranks(R, rank, f"split checksum of {total} bytes over {R} ranks")
            for r in range(R):
                at = (total, R, r)
                slots, ok_a = cvs[r].read()
                root, ok_b = roots[r].read()
                assert ok_a and ok_b, at
                assert root.tobytes() == want, at
                assert len(slots) == R * q and np.array_equal(slots[:nb], leaves), at
                assert untouched(slots[nb:]), at
            for s in splits:
                s.close()
            ran += 1
    finally:
        rk.close()
    assert ran == len(xc.SPLIT_TOTALS)
