"""sd_cas_dedup_mgpu at one rank -- run on an MI355X: -m gpu.

One rank exchanges with nobody: its row goes to the host with one copy (no all-gather), and the
partition writes the records straight into d_records_out when capacity >= n (the direct path), or
into the communicator's buffer and from there with one device copy once the checks have passed
(the staged path).  Every case runs on an RCCL communicator of one rank and on an in-process group
of one, between 0xA5 guard rows, and is compared bit for bit with the host mirror
(dedup.group_host + identifier.object_owners).  The sizes are the edges of a 256-lane workgroup
and of the partition's 1024 slices.  The row the partition's scan now completes on the device
(counts, base, n, capacity, valid) has no accessor; an R = 2 in-process exchange with descending
index ranges, and one refused for capacity, read every field of it."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd import dedup, synth  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError  # noqa: E402
from spacedrive_amd.dedup import group_host, keys_from_hashes  # noqa: E402
from spacedrive_amd.device import Comm, CommGroup, ObjectIndex  # noqa: E402
from spacedrive_amd.identifier import object_owners  # noqa: E402
from tests import exchange_cases as xc  # noqa: E402
from tests.test_gpu_exchange import (Inputs, Outputs, Ranks, SPARE, call_ranks, i64, run_case,  # noqa: E402
                                     untouched)
from tests.test_gpu_parity import gpu_cas  # noqa: E402

SD_ERR_INVALID = -1
CHUNK = 100
BASE = 7_000_000  # a shard of a larger library
N_MAX = 5000
SIZES = (0, 1, 255, 256, 257, 1023, 1024, 1025, N_MAX)
PATTERNS = ("all", "none", "third", "null")


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


@pytest.fixture(scope="module")
def hashes(ctx):
    """cas hashes of a 5000-file library with duplicate groups, hashed on the device once; the
    smaller cases take its first n rows"""
    sizes, cids, twins = synth.library(0, N_MAX, N_MAX, dup_frac=0.3)
    h = gpu_cas(ctx, sizes, cids, twins).copy()
    assert len(np.unique(keys_from_hashes(h))) < N_MAX - 100  # groups exist
    return h, torch.from_numpy(h).cuda()


@pytest.fixture(scope="module")
def comms(ctx):
    """(name, communicator) of one rank over both transports, shared by every case"""
    rccl = dedup.make_comm(ctx)
    group = CommGroup(1)
    local = Comm(ctx, None, 1, 0, group=group)
    yield (("rccl", rccl), ("in-process", local))
    local.close()
    group.close()
    rccl.close()


def valid_of(pattern: str, n: int):
    """host mask (None: d_valid == NULL)"""
    if pattern == "null":
        return None
    if pattern == "all":
        return np.ones(n, np.uint8)
    if pattern == "none":
        return np.zeros(n, np.uint8)
    return (np.arange(n) % 3 != 0).astype(np.uint8)  # every third file invalid, the first among them


def mirror(h: np.ndarray, valid, n: int, base: int, chunk: int = CHUNK):
    """(m, n_groups, records, rep, owner) of the first n files"""
    ok = np.ones(n, bool) if valid is None else valid.astype(bool)
    keys = keys_from_hashes(h[:n]) if n else np.zeros(0, np.uint64)
    recs = np.stack([keys[ok].view(np.int64), np.arange(base, base + n, dtype=np.int64)[ok]], axis=1).reshape(-1, 2)
    gr, rep, ng = group_host(recs)
    own = object_owners(torch.from_numpy(gr[:, 1].copy()), torch.from_numpy(np.ascontiguousarray(rep)), chunk).numpy()
    return len(gr), ng, gr, rep, own


def call(ctx, comm, hashes, valid, n: int, base: int, outs: Outputs, stream):
    """-> ("ok", m, n_groups) or ("refused", rc, needed)"""
    d_hash = hashes[1][:n] if n else None  # n = 0: NULL d_hash32
    d_valid = None if valid is None or n == 0 else torch.from_numpy(valid).cuda()
    try:
        m, ng = ctx.dedup_mgpu(comm, d_hash, d_valid, n, base, outs.records.inner, outs.rep.inner, outs.owner.inner,
                               outs.cap, CHUNK, stream)
    except SdCasError as e:
        return "refused", e.rc, e.needed
    stream.synchronize()
    return "ok", m, ng


def check(outs: Outputs, got, want, at):
    m, ng, gr, rep, own = want
    assert got == ("ok", m, ng), (at, got)
    r, ok_a = outs.records.read()
    p, ok_b = outs.rep.read()
    o, ok_c = outs.owner.read()
    assert ok_a and ok_b and ok_c, at
    assert np.array_equal(i64(r[:m]).reshape(-1, 2), gr), at
    assert np.array_equal(i64(p[:m]).reshape(-1), rep), at
    assert np.array_equal(i64(o[:m]).reshape(-1), own), at
    assert untouched(r[m:]) and untouched(p[m:]) and untouched(o[m:]), at  # rows m .. capacity keep the poison
    assert len(r) == outs.cap


def all_poison(outs: Outputs) -> bool:
    reads = [g.read() for g in outs.all()]
    return all(ok and untouched(rows) for rows, ok in reads)


@pytest.mark.parametrize("n", SIZES)
def test_direct_path_every_valid_pattern(ctx, comms, hashes, n):
    """capacity >= n, with spare rows and at capacity == n exactly: both transports equal the mirror
    and write nothing past row m."""
    s = torch.cuda.Stream()
    for pattern in PATTERNS:
        valid = valid_of(pattern, n)
        want = mirror(hashes[0], valid, n, BASE)
        assert want[0] == {"all": n, "null": n, "none": 0, "third": n - math.ceil(n / 3)}[pattern]
        for cap in (n + SPARE, n):
            for name, comm in comms:
                outs = Outputs(cap)
                check(outs, call(ctx, comm, hashes, valid, n, BASE, outs, s), want, (n, pattern, cap, name))


@pytest.mark.parametrize("n", SIZES[1:])
def test_staged_path_at_the_requirement_and_one_short(ctx, comms, hashes, n):
    """capacity < n with a third of the files invalid: capacity == m succeeds and equals the mirror;
    capacity == m - 1 returns SD_ERR_CAPACITY with *m_out == m and moves nothing into the outputs."""
    s = torch.cuda.Stream()
    valid = valid_of("third", n)
    want = mirror(hashes[0], valid, n, BASE)
    m = want[0]
    assert m < n
    for name, comm in comms:
        outs = Outputs(m)
        check(outs, call(ctx, comm, hashes, valid, n, BASE, outs, s), want, (n, name))
        if m >= 1:
            short = Outputs(m - 1)
            assert call(ctx, comm, hashes, valid, n, BASE, short, s) == ("refused", SD_ERR_CAPACITY, m), (n, name)
            assert all_poison(short), (n, name)
            again = Outputs(m)  # the communicator goes on
            check(again, call(ctx, comm, hashes, valid, n, BASE, again, s), want, (n, name, "after the refusal"))


@pytest.mark.parametrize("staged", [False, True], ids=["direct", "staged"])
def test_no_state_of_an_earlier_call_survives(ctx, comms, hashes, staged):
    """n = 5000, 257, 0, 5000 on one communicator: every call equals its own mirror."""
    s = torch.cuda.Stream()
    for name, comm in comms:
        for k, n in enumerate((N_MAX, 257, 0, N_MAX)):
            valid = valid_of("third", n)
            want = mirror(hashes[0], valid, n, BASE + k)
            outs = Outputs(want[0] if staged else n + SPARE)
            check(outs, call(ctx, comm, hashes, valid, n, BASE + k, outs, s), want, (name, k, n))


def test_wrongly_sharded_index_refuses_and_moves_nothing(ctx, comms, hashes):
    """sd_cas_dedup_mgpu_indexed with an index sharded for (2, 0): SD_ERR_INVALID, every output
    keeps its poison (capacity >= n: the records must not have gone the direct way), and the next
    call on the communicator succeeds."""
    s = torch.cuda.Stream()
    n = 257
    valid = valid_of("third", n)
    want = mirror(hashes[0], valid, n, BASE)
    index = ObjectIndex(ctx, 2, 0)
    try:
        for name, comm in comms:
            outs = Outputs(n + SPARE, indexed=True)
            with pytest.raises(SdCasError) as e:
                ctx.dedup_mgpu_indexed(comm, hashes[1][:n], torch.from_numpy(valid).cuda(), n, BASE, outs.records.inner,
                                       outs.rep.inner, outs.owner.inner, outs.cap, index, outs.existing.inner,
                                       outs.new.inner, CHUNK, s)
            assert e.value.rc == SD_ERR_INVALID and "not sharded" in str(e.value), (name, str(e.value))
            s.synchronize()
            assert all_poison(outs), name
            ok = Outputs(n + SPARE)
            check(ok, call(ctx, comm, hashes, valid, n, BASE, ok, s), want, (name, "after the refusal"))
    finally:
        index.close()


def test_every_phase_is_still_timed(ctx, comms, hashes):
    """sd_comm_set_timing: all five phase durations of a one-rank call are finite and >= 0 (the
    exchange phases may read about 0), on the direct and on the staged path."""
    s = torch.cuda.Stream()
    n = N_MAX
    valid = valid_of("third", n)
    want = mirror(hashes[0], valid, n, BASE)
    for name, comm in comms:
        comm.set_timing(True)
        try:
            for cap in (n, want[0]):
                outs = Outputs(cap)
                check(outs, call(ctx, comm, hashes, valid, n, BASE, outs, s), want, (name, cap))
                ph = comm.last_phases()
                assert tuple(ph) == Comm.PHASES and len(ph) == 5
                assert all(math.isfinite(v) and v >= 0.0 for v in ph.values()), (name, ph)
        finally:
            comm.set_timing(False)


def test_row_written_by_the_scan_drives_an_exchange_of_two():
    """The row has no accessor, so two in-process ranks read it the way they use it: the counts
    size the receives and the valid total must equal their sum, base and n decide whether the
    records arrive in index order (a descending layout groups wrongly if they are misread), and
    the capacity refuses both ranks together with each rank's own need."""
    rk = Ranks(2)
    try:
        run_case(rk, xc.case(xc.gpu_order(2)[0]))
        run_case(rk, xc.case(xc.variant_specs(2)[0]))
        c = xc.case(xc.capacity_specs(2)[0])
        inp = Inputs(c)
        short = int(np.argmax(c.need))
        outs = [Outputs(need - (r == short)) for r, need in enumerate(c.need)]
        got = call_ranks(rk, c, inp, outs)
        for r in range(2):
            assert got[r] == ("refused", SD_ERR_CAPACITY, c.need[r]), (c.name, r, got[r])
            assert all_poison(outs[r]), (c.name, r)
        run_case(rk, c, "after the refusal")
    finally:
        rk.close()
