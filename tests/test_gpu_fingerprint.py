"""Fingerprints on an MI355X (-m gpu): the gather kernel byte for byte against the device
synth stager, the batch's two outputs and the host drop-in bit-exact on 32 bytes against
oracle.native, with the memory discipline of tests/test_gpu_shapes.py re-declared here: 0xA5
guard rows around every output, poisoned and random surroundings, an untouched input, a
second batch shape in between.  Lengths and placement: tests/fingerprint_cases.py."""
import hashlib
import threading
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd.device import stage_plan  # noqa: E402
from tests import fingerprint_cases as fc  # noqa: E402
from tests import shape_cases as sc  # noqa: E402

NT = 16  # oracle threads: the GPU box's host share per GPU
G = 4  # guard rows either side of an output
POISON = 0xA5


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = sd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


@contextmanager
def tuning(**kv):
    """Process-wide knobs set for one block and put back whatever happens in it."""
    keep = {k: sd.get_tuning(k) for k in kv}
    try:
        for k, v in kv.items():
            sd.set_tuning(k, v)
        yield
    finally:
        for k, v in keep.items():
            sd.set_tuning(k, v)


class Guarded:
    """`rows` rows of `row_bytes` device bytes between G guard rows, all 0xA5; the kernels get
    `inner`, and guards_intact() tells whether they kept to it."""

    def __init__(self, rows: int, row_bytes: int):
        self.rows, self.row_bytes = rows, row_bytes
        self.raw = torch.full(((rows + 2 * G) * row_bytes,), POISON, dtype=torch.uint8, device="cuda")
        self.inner = self.raw[G * row_bytes:(G + rows) * row_bytes]

    def _all(self) -> np.ndarray:
        torch.cuda.synchronize()
        return self.raw.cpu().numpy().reshape(-1, self.row_bytes)

    def host(self) -> np.ndarray:
        return self._all()[G:G + self.rows]

    def guards_intact(self) -> bool:
        a = self._all()
        return bool((a[:G] == POISON).all() and (a[G + self.rows:] == POISON).all())


def i64(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))


def device_files(ctx, lens, cids, twins, offs, total: int, surround: str) -> torch.Tensor:
    """The buffer on the device: sd_synth_fill(cid, twin, len) in each range; outside the
    ranges 0xA5 or seeded random bytes (the fill writes whole 8-byte words: the up to 7 bytes
    it zeroes after a range are put back)."""
    if surround == "random":
        host = np.random.default_rng(99).integers(0, 256, total, dtype=np.uint8)
    else:
        host = np.full(total, POISON, np.uint8)
    d = torch.from_numpy(host).cuda()
    for L, c, t, o in zip(lens, cids, twins, offs):
        if L:
            ctx.synth_fill(int(c), int(t), int(L), d[int(o):])
    for L, o in zip(lens, offs):
        e = int(o) + int(L)
        if L % 8:
            d[e:e + 8 - int(L) % 8] = torch.from_numpy(host[e:e + 8 - int(L) % 8]).cuda()
    torch.cuda.synchronize()
    return d


def sha(d: torch.Tensor) -> str:
    torch.cuda.synchronize()
    return hashlib.sha256(d.cpu().numpy().tobytes()).hexdigest()


def stager_bytes(ctx, lens, cids, twins, ext, total: int) -> np.ndarray:
    """sd_synth_stage_cas for the same files into a zeroed buffer at the same extents"""
    d = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
    ctx.synth_stage_cas(i64(lens.astype(np.uint64)).cuda(), i64(cids.astype(np.uint64)).cuda(),
                        torch.from_numpy(twins.astype(np.int32)).cuda(), d_ext, len(lens), d)
    torch.cuda.synchronize()
    return d.cpu().numpy()[:total]


def want_rows(oracle_native, lens, cids, twins):
    """(cas hashes [n, 32], checksums [n, 32]) from the oracle: BLAKE3 of the oracle-staged
    messages, and the synthetic files' checksums"""
    ext, total = stage_plan(lens)
    staged = oracle_native.stage_synth(lens, cids, twins, ext["msg_offset"], total)
    cas = oracle_native.checksums(staged, ext["msg_offset"], ext["msg_len"].astype(np.uint64), nthreads=NT)
    assert np.array_equal(cas[:, :8], oracle_native.cas_ids_synth(lens, cids, twins, nthreads=NT))
    return cas, oracle_native.checksums_synth(lens, cids, twins, nthreads=NT)


def bad_rows(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    assert got.shape == want.shape and got.shape[1] == 32
    return np.nonzero((got != want).any(axis=1))[0]


@pytest.fixture(scope="module")
def case(oracle_native):
    """The 90 files, placed; the oracle's 32-byte rows for them (computed once, never changed)."""
    lens, cids, twins = fc.cases()
    offs, total = fc.placement(lens)
    cas, sums = want_rows(oracle_native, lens, cids, twins)
    cas.setflags(write=False)
    sums.setflags(write=False)
    return dict(lens=lens, cids=cids, twins=twins, offs=offs, total=total, cas=cas, sums=sums)


def gather_into_guarded(ctx, case, surround: str):
    d = device_files(ctx, case["lens"], case["cids"], case["twins"], case["offs"], case["total"], surround)
    before = sha(d)
    b = ctx.fingerprint_batch(case["offs"], case["lens"])
    extra = 32  # rows past the messages: the gather's buffer holds more than it writes
    g = Guarded(b.staged_bytes // 128 + extra, 128)
    b.gather(d, g.inner)
    got = g.host().reshape(-1).copy()
    assert g.guards_intact()
    assert sha(d) == before  # the input is read-only
    b.close()
    return b, got


# ----------------------------------------------------- 1: gather == the synth stager
def test_gather_equals_the_synth_stager(ctx, case):
    lens = case["lens"]
    b, got = gather_into_guarded(ctx, case, "a5")
    ext, total = stage_plan(lens)
    assert b.staged_bytes == total and np.array_equal(b.extents, ext)
    assert (b.n, b.n_whole, b.n_sampled) == (90, 21, 69)
    assert b.file_bytes == int(lens.sum()) and b.gather_read_bytes == int(ext["msg_len"].sum()) - 8 * 90
    want = stager_bytes(ctx, lens, case["cids"], case["twins"], ext, total)
    covered = np.zeros(len(got), bool)
    compared = 0
    for i, e in enumerate(ext):
        lo = int(e["msg_offset"])
        hi = lo + (int(e["msg_len"]) + 127) // 128 * 128
        diff = np.nonzero(got[lo:hi] != want[lo:hi])[0]
        assert len(diff) == 0, (i, int(lens[i]), diff[:8].tolist())
        assert not covered[lo:hi].any()
        covered[lo:hi] = True
        compared += 1
    assert compared == 90
    assert covered[:total].all() and (~covered).sum() == 32 * 128
    assert (got[~covered] == POISON).all()  # nothing else is written


# ----------------------------------------------------- 2: surroundings
def test_gather_ignores_surroundings(ctx, case):
    _, a = gather_into_guarded(ctx, case, "a5")
    _, r = gather_into_guarded(ctx, case, "random")
    assert np.array_equal(a, r)


# ----------------------------------------------------- 3: run()
def run_guarded(batch, d):
    cas, sums = Guarded(batch.n, 32), Guarded(batch.n, 32)
    batch.run(d, cas.inner, sums.inner)
    got = cas.host().copy(), sums.host().copy()
    assert cas.guards_intact() and sums.guards_intact()
    return got


@pytest.mark.parametrize("sampled_wave_max", [0, 6144])
@pytest.mark.parametrize("whole_wave_max", [1 << 30, 0])
def test_run_interleaved_both_kernel_families(ctx, oracle_native, case, whole_wave_max, sampled_wave_max):
    """Whole and sampled files interleaved; the latency kernels (one wave / workgroup per file)
    and the throughput kernels (work lists, lanes + merge) both consume gathered messages."""
    nw = fc.N_WHOLE
    a = tuple(case[k][:nw] for k in ("lens", "cids", "twins"))
    b = tuple(case[k][nw:] for k in ("lens", "cids", "twins"))
    lens, cids, twins, is_b = sc.interleave(a, b, seed=11)
    want_cas, want_sums = np.empty((90, 32), np.uint8), np.empty((90, 32), np.uint8)
    want_cas[~is_b], want_cas[is_b] = case["cas"][:nw], case["cas"][nw:]
    want_sums[~is_b], want_sums[is_b] = case["sums"][:nw], case["sums"][nw:]
    offs, total = fc.placement(lens)
    d = device_files(ctx, lens, cids, twins, offs, total, "random")
    before = sha(d)
    with tuning(whole_wave_max=whole_wave_max, sampled_wave_max=sampled_wave_max):
        batch = ctx.fingerprint_batch(offs, lens)
        # a differently shaped batch over the same buffer: every third file, reversed
        pick = np.arange(90)[::3][::-1].copy()
        other = ctx.fingerprint_batch(offs[pick], lens[pick])
    got_cas, got_sums = run_guarded(batch, d)
    assert len(bad_rows(got_cas, want_cas)) == 0, lens[bad_rows(got_cas, want_cas)].tolist()
    assert len(bad_rows(got_sums, want_sums)) == 0, lens[bad_rows(got_sums, want_sums)].tolist()
    o_cas, o_sums = run_guarded(other, d)
    assert len(bad_rows(o_cas, want_cas[pick])) == 0 and len(bad_rows(o_sums, want_sums[pick])) == 0
    again_cas, again_sums = run_guarded(batch, d)  # fresh 0xA5 rows: nothing leans on the first run
    assert np.array_equal(again_cas, want_cas) and np.array_equal(again_sums, want_sums)
    assert sha(d) == before
    assert len(want_cas) == 90 and len(pick) == 30
    batch.close()
    other.close()


def test_empty_batch(ctx):
    b = ctx.fingerprint_batch([], [])
    assert b.n == 0 and b.staged_bytes == 0
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((64,), POISON, dtype=torch.uint8, device="cuda")
    b.run(d, out, out)
    b.gather(d, out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    b.close()
    with pytest.raises(sd.SdCasError):
        ctx.fingerprint_batch([8], [100])  # a start that is not 16-byte aligned


# ----------------------------------------------------- 4: 64-bit offsets and lengths
def test_offsets_and_lengths_beyond_4gib(ctx, oracle_native, golden, case):
    """A 4 GiB file first, then a file of 2^32 + 12345 bytes, then the whole-kind list at buffer
    offsets beyond 2^32: the gather's source addresses, its sample offsets and the le64 header
    in 64-bit arithmetic."""
    big = [(10_000, 1 << 32), (10_001, (1 << 32) + 12345)]
    nw = fc.N_WHOLE
    lens = np.concatenate([np.array([L for _, L in big], np.uint64), case["lens"][:nw]])
    cids = np.concatenate([np.array([c for c, _ in big], np.uint64), case["cids"][:nw]])
    twins = np.concatenate([np.zeros(2, np.uint32), case["twins"][:nw]])
    offs, total = fc.placement(lens)
    assert int(offs[1]) >= 1 << 32 and int(offs[2]) >= 1 << 33
    d = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    for L, c, t, o in zip(lens, cids, twins, offs):
        if L:
            ctx.synth_fill(int(c), int(t), int(L), d[int(o):])
    b = ctx.fingerprint_batch(offs, lens)
    got_cas, got_sums = run_guarded(b, d)
    del d
    torch.cuda.empty_cache()
    n = len(lens)
    assert n == 2 + nw
    assert np.array_equal(got_cas[:, :8], oracle_native.cas_ids_synth(lens, cids, twins, nthreads=NT))
    assert np.array_equal(got_cas[2:], case["cas"][:nw])
    assert np.array_equal(got_sums[2:], case["sums"][:nw])
    assert got_sums[0].tobytes().hex() == golden["bench_checksums"]["synth"][f"10000:{1 << 32}"]
    assert got_sums[1].tobytes() == oracle_native.checksum_synth_mt((1 << 32) + 12345, 10_001, 0, nthreads=NT)
    b.close()


# ----------------------------------------------------- 5: sd_fingerprints over host memory
def hex_rows(rows: np.ndarray, nbytes: int):
    return [bytes(r[:nbytes]).hex() for r in rows]


@pytest.fixture(scope="module")
def host_case(case):
    buf = fc.host_buffer(case["lens"], case["cids"], case["twins"], case["offs"], case["total"], "a5")
    return buf, hex_rows(case["cas"], 8), hex_rows(case["sums"], 32)


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
@pytest.mark.parametrize("window_mb", [256, 1])
def test_fingerprints_from_host_memory(ctx, case, host_case, memory, window_mb):
    """Every byte goes up once: the H2D bytes are the ranges' bytes plus one 57 352-byte
    message per large range.  With a 1 MiB window the ranges of 1 MiB + 1 and 3 MiB + 5 take
    the large-range path and the other 88 files fill several alternating windows."""
    buf, want17, want65 = host_case
    data = torch.from_numpy(buf).pin_memory() if memory == "pinned" else buf
    lens, offs = case["lens"], case["offs"]
    with tuning(fingerprint_window_mb=window_mb):
        s0 = sd.fingerprints_stats(0)
        ids, sums = sd.fingerprints(data, offs, lens, device=0)
        s1 = sd.fingerprints_stats(0)
    assert ids == want17 and sums == want65
    assert (ids, sums) == sd.cpu.fingerprints(buf, offs, lens)
    large = int((lens > (window_mb << 20)).sum())
    assert large == (2 if window_mb == 1 else 0)
    assert s1["large"] - s0["large"] == large
    assert s1["gathered"] - s0["gathered"] + large == 90
    assert s1["h2d_bytes"] - s0["h2d_bytes"] == int(lens.sum()) + 57352 * large


def test_fingerprints_copy_runs(ctx, oracle_native):
    """The copies of one window: neighbours share a run; a range after a hole of whole pages
    (never read: the caller's buffer may have nothing there) and a range of 1 MiB or more that
    would start mid-line each open a run of their own; an empty range sits between them."""
    page = 4096
    lens = np.array([5000, 300, 0, 70000, fc.MiB + 3, 123457, 16, 0], np.uint64)
    def up16(x):
        return (int(x) + 15) // 16 * 16

    offs = np.array([0, 5008, 5312, 5312 + 3 * page, 0, 0, 0, 0], np.uint64)
    offs[4] = up16(int(offs[3]) + int(lens[3])) + 48                 # mid-line: a 1 MiB range opens a run
    offs[5] = up16(int(offs[4]) + int(lens[4]) + 13)                 # continues that run
    offs[6] = up16(int(offs[5]) + int(lens[5]) + 5 * page + 7)       # after a hole
    offs[7] = offs[6] + 16
    assert all(int(o) % 16 == 0 for o in offs) and int(offs[4]) % 128 != 0
    cids = np.arange(31_000, 31_008, dtype=np.uint64)
    twins = np.zeros(8, np.uint32)
    total = int(offs[-1]) + 128
    buf = fc.host_buffer(lens, cids, twins, offs, total, "random")
    want = (hex_rows(oracle_native.cas_ids_synth(lens, cids, twins), 8),
            hex_rows(oracle_native.checksums_synth(lens, cids, twins), 32))
    s0 = sd.fingerprints_stats(0)
    got = sd.fingerprints(buf, offs, lens, device=0)
    s1 = sd.fingerprints_stats(0)
    assert got[0] == want[0] and got[1] == want[1]
    assert s1["h2d_bytes"] - s0["h2d_bytes"] == int(lens.sum()) and s1["gathered"] - s0["gathered"] == 8


def test_fingerprints_four_concurrent_callers(ctx, oracle_native):
    """Four threads on one context, each with its own files, through 1 MiB windows."""
    lens, _, twins = fc.cases()
    offs, total = fc.placement(lens)
    jobs = []
    for t in range(4):
        cids = np.arange(20_000 + 100 * t, 20_000 + 100 * t + 90, dtype=np.uint64)
        buf = fc.host_buffer(lens, cids, twins, offs, total, "random")
        want = (hex_rows(oracle_native.cas_ids_synth(lens, cids, twins, nthreads=NT), 8),
                hex_rows(oracle_native.checksums_synth(lens, cids, twins, nthreads=NT), 32))
        jobs.append([buf, want, None])

    def call(j):
        try:
            j[2] = sd.fingerprints(j[0], offs, lens, device=0)
        except Exception as e:  # noqa: BLE001 -- reported by the assertion below
            j[2] = e

    with tuning(fingerprint_window_mb=1):
        th = [threading.Thread(target=call, args=(j,)) for j in jobs]
        for x in th:
            x.start()
        for x in th:
            x.join()
    for t, (buf, want, got) in enumerate(jobs):
        assert not isinstance(got, Exception), got
        assert got[0] == want[0] and got[1] == want[1], t
    assert len({tuple(j[2][0]) for j in jobs}) == 4  # four different libraries


# ----------------------------------------------------- 6: sample twins
def test_twins_through_the_gpu(ctx, oracle_native):
    L = 200_000
    lens = np.array([L, L, L], np.uint64)
    cids, twins = np.array([77, 77, 77], np.uint64), np.array([0, 1, 2], np.uint32)
    offs, total = fc.placement(lens)
    d = device_files(ctx, lens, cids, twins, offs, total, "a5")
    b = ctx.fingerprint_batch(offs, lens)
    cas, sums = run_guarded(b, d)
    assert np.array_equal(cas[0], cas[1]) and np.array_equal(cas[0], cas[2])
    assert len({r.tobytes() for r in sums}) == 3
    assert np.array_equal(cas[:, :8], oracle_native.cas_ids_synth(lens, cids, twins))
    assert np.array_equal(sums, oracle_native.checksums_synth(lens, cids, twins))
    ids, hexsums = sd.fingerprints(fc.host_buffer(lens, cids, twins, offs, total, "a5"), offs, lens, device=0)
    assert ids[0] == ids[1] == ids[2] and len(set(hexsums)) == 3
    b.close()
