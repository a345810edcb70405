"""Shape sweeps and memory discipline of the hash and dedup kernels -- run on an MI355X: -m gpu.

tests/test_gpu_parity.py is bit-exact at the workload sizes; this module enumerates the
shapes the kernels branch on (tests/shape_cases.py) and makes four kinds of bug visible
that a right-sized, zero-filled, run-once test cannot see: a write outside the rows a call
owns (0xA5 guard rows around every output), a dependence on bytes outside the message
(random surroundings), a write into the input, and a missing write hidden by an earlier
run's scratch (a second batch shape in between, outputs pre-filled).  Every comparison is
on all 32 hash bytes against oracle.native, and every test asserts how many cases it
compared."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from spacedrive_amd._native import SD_KIND_WHOLE, SdCasError  # noqa: E402
from spacedrive_amd.dedup import group_host, partition_host  # noqa: E402
from spacedrive_amd.device import EXTENT_DTYPE, stage_plan  # noqa: E402
from tests import shape_cases as sc  # noqa: E402

NT = 16  # oracle threads: the GPU box's host share per GPU
G = 4  # guard rows either side of an output
POISON = 0xA5
MODES = {"latency": 1 << 30, "worklists": 0}  # "whole_wave_max": k_whole_wave | k_whole_items + k_whole_merge8


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    # the product library must be the in-tree HIP build
    maps = open("/proc/self/maps").read()
    assert "spacedrive_amd/libsdcas.so" in maps
    return c


@contextmanager
def tuning(**kv):
    """Process-wide knobs set for one block and put back whatever happens in it."""
    import spacedrive_amd as sd
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
    `inner` (optionally viewed as int64), and guards_intact() tells whether they kept to it."""

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
        """the inner rows, as bytes"""
        return self._all()[G:G + self.rows]

    def guards_intact(self) -> bool:
        a = self._all()
        return bool((a[:G] == POISON).all() and (a[G + self.rows:] == POISON).all())


def untouched(rows: np.ndarray) -> np.ndarray:
    """per row: still all 0xA5"""
    return (rows == POISON).all(axis=1)


def i64(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))


def stage(ctx, sizes, cids, twins, staged_bytes=None):
    """The cas messages of synthetic files written by the device stager at stage_plan's
    offsets -> (extents, device buffer); `staged_bytes` for a larger buffer that holds more
    than these messages."""
    ext, total = stage_plan(sizes)
    n = len(sizes)
    d_staged = torch.zeros((staged_bytes or total) + 64, dtype=torch.uint8, device="cuda")
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
    ctx.synth_stage_cas(i64(sizes.astype(np.uint64)).cuda(), i64(cids.astype(np.uint64)).cuda(),
                        torch.from_numpy(twins.astype(np.int32)).cuda(), d_ext, n, d_staged)
    return ext, d_staged


def run_rows(batch, d_in, n: int, fill: int = 0xFF) -> np.ndarray:
    """batch.run into n rows pre-filled with `fill` -> the rows"""
    out = torch.full((max(n, 1) * 32,), fill, dtype=torch.uint8, device="cuda")
    batch.run(d_in, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:n * 32].reshape(n, 32)


def oracle_rows(oracle_native, staged: np.ndarray, ext) -> np.ndarray:
    return oracle_native.checksums(staged, ext["msg_offset"], ext["msg_len"].astype(np.uint64), nthreads=NT)


def bad_rows(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    assert got.shape == want.shape and got.shape[1] == 32
    return np.nonzero((got != want).any(axis=1))[0]


# ----------------------------------------------------- A: whole-file tree sweep
@pytest.mark.parametrize("order", ["shuffled", "ascending"])
@pytest.mark.parametrize("mode", list(MODES))
def test_whole_tree_sweep(ctx, oracle_native, mode, order):
    """Every chunk count C = 1..101 of a whole-kind message, seven last-chunk lengths each
    (700 messages, every pair count P = 1..51), through k_whole_wave (one LDS tree per
    message) and through the work lists (pair items, then one or two k_whole_merge8 passes
    of groups of 1..8 nodes), there among 300 sampled files so that the rows scatter through
    idx and both halves of k_whole_items' grid have work."""
    cases = sc.sweep_a()
    whole = sc.cas_files(cases)
    if order == "shuffled":
        perm = np.random.default_rng(3).permutation(len(cases))
        cases = [cases[i] for i in perm]
        whole = tuple(x[perm] for x in whole)
    if mode == "worklists":
        sizes, cids, twins, is_sampled = sc.interleave(whole, sc.sampled_files(300), seed=4)
    else:
        sizes, cids, twins = whole
        is_sampled = np.zeros(len(cases), bool)
    label = np.full(len(sizes), -1)
    label[~is_sampled] = np.arange(len(cases))
    with tuning(whole_wave_max=MODES[mode]):
        ext, d_staged = stage(ctx, sizes, cids, twins)
        b = ctx.cas_batch(ext)
        assert b.n_whole == sc.SWEEP_A_COUNT and b.n_sampled == int(is_sampled.sum())
        assert (b.full_items + b.tail_items == 0) == (mode == "latency")  # the mode took effect
        got = run_rows(b, d_staged, len(sizes))
        b.close()
    assert ext["msg_len"][~is_sampled].tolist() == [L for _, _, L in cases]
    staged = d_staged.cpu().numpy()
    want = oracle_rows(oracle_native, staged, ext)
    mism = bad_rows(got, want)
    assert len(mism) == 0, [("sampled", int(sizes[i])) if is_sampled[i] else
                            (cases[label[i]][0], cases[label[i]][1], (cases[label[i]][0] + 1) // 2) for i in mism[:10]]
    assert np.array_equal(got[:, :8], oracle_native.cas_ids_synth(sizes, cids, twins, nthreads=NT))
    assert len(got) - int(is_sampled.sum()) == 700
    assert len(got) == (1000 if mode == "worklists" else 700)


# ----------------------------------------------------- B: checksum leaf and reduce sweep
def fill_files(ctx, lens, cids, twins, gap: int = 64):
    """Synthetic contents on the device, each range on a 128-byte line -> (offsets, buffer)"""
    offs, total = sc.place(lens, gap=gap)
    d = torch.zeros(total, dtype=torch.uint8, device="cuda")
    for L, o, c, t in zip(lens, offs, cids, twins):
        if L:
            ctx.synth_fill(int(c), int(t), int(L), d[o:])
    return offs, d


def want_checksums(oracle_native, lens, cids, twins) -> np.ndarray:
    """the C oracle's checksums of synthetic files; the long ones chunk-parallel"""
    lens_a, cids_a, twins_a = np.array(lens, np.uint64), np.array(cids, np.uint64), np.array(twins, np.uint32)
    long_ = lens_a > np.uint64(8 * sc.MiB)
    want = np.zeros((len(lens), 32), np.uint8)
    want[~long_] = oracle_native.checksums_synth(lens_a[~long_], cids_a[~long_], twins_a[~long_], nthreads=NT)
    for i in np.nonzero(long_)[0]:
        want[i] = np.frombuffer(oracle_native.checksum_synth_mt(int(lens[i]), int(cids[i]), int(twins[i]),
                                                                nthreads=NT), np.uint8)
    return want


def test_checksum_block_sweep(ctx, oracle_native):
    """k_ck_leaf inside one 1 MiB block: every chunk count C = 1..1024 -- every lanes_b =
    ceil(C / 4) in 1..256 of the odd-carry LDS tree, every last-lane chunk count 1..4 -- with
    last chunks of 1, 64, 65, 1023 and 1024 bytes, in a seeded shuffle so that each
    workgroup holds the blocks of two unrelated files: one batch of all 1132 files (566
    workgroups of two blocks), and one without the last file (the last workgroup holds one
    block)."""
    cases = sc.sweep_b_block()
    perm = np.random.default_rng(6).permutation(len(cases))
    cases = [cases[i] for i in perm]
    lens = [L for _, _, L in cases]
    cids = [20000 + int(i) for i in perm]
    twins = [int(i) % 3 for i in perm]
    offs, d = fill_files(ctx, lens, cids, twins)
    want = want_checksums(oracle_native, lens, cids, twins)
    compared = 0
    for count in (len(cases), len(cases) - 1):
        b = ctx.checksum_batch(offs[:count], lens[:count])
        assert b.blocks == count
        got = run_rows(b, d, count)
        b.close()
        mism = bad_rows(got, want[:count])
        assert len(mism) == 0, (count, [cases[i] for i in mism[:10]])
        compared += count
    assert compared == 1132 + 1131


def test_checksum_block_pairs(ctx, oracle_native):
    """Two unrelated files in one leaf workgroup (s_lanes / s_root / s_dst per block): a
    1-byte file beside a full block, an empty file beside a 1021-chunk one, either first."""
    compared = 0
    for k, lens in enumerate(sc.sweep_b_pairs()):
        cids, twins = [300 + 2 * k, 301 + 2 * k], [0, 1]
        offs, d = fill_files(ctx, lens, cids, twins)
        b = ctx.checksum_batch(offs, lens)
        assert b.blocks == 2
        got = run_rows(b, d, 2)
        b.close()
        assert len(bad_rows(got, want_checksums(oracle_native, lens, cids, twins))) == 0, lens
        compared += 2
    assert compared == 8


def test_checksum_last_blocks(ctx, oracle_native):
    """Files of 1..3 full blocks and a last block of 1..5 or 1023 chunks whose last chunk has
    1 or 1024 bytes: a partial block's CV beside full ones in k_ck_reduce."""
    lens = sc.sweep_b_last_blocks()
    cids, twins = list(range(400, 400 + len(lens))), [i % 2 for i in range(len(lens))]
    offs, d = fill_files(ctx, lens, cids, twins)
    b = ctx.checksum_batch(offs, lens)
    got = run_rows(b, d, len(lens))
    b.close()
    mism = bad_rows(got, want_checksums(oracle_native, lens, cids, twins))
    assert len(mism) == 0, [lens[i] for i in mism]
    assert len(got) == 36


def test_checksum_reduce_groups(ctx, oracle_native):
    """k_ck_reduce groups of 2, 3, 5, 7, 8, 9, 15, 16, 17 and 33 block CVs, the last block full
    or one byte short."""
    lens = sc.sweep_b_reduce()
    cids, twins = list(range(500, 500 + len(lens))), [0] * len(lens)
    offs, d = fill_files(ctx, lens, cids, twins)
    b = ctx.checksum_batch(offs, lens)
    got = run_rows(b, d, len(lens))
    b.close()
    mism = bad_rows(got, want_checksums(oracle_native, lens, cids, twins))
    assert len(mism) == 0, [lens[i] for i in mism]
    assert len(got) == 20


# ----------------------------------------------------- C: packed ranges, poisoned surroundings
def test_checksum_packed_ranges_ignore_surroundings(ctx, oracle_native):
    """sd_checksum_batch promises a buffer readable, not zero, up to the next 64-byte boundary
    after a range, and ranges aligned to 16 bytes only: ranges packed 0..48 bytes apart in
    random bytes, every start residue mod 128 under a range of >= 1 MiB, hashed twice with
    different bytes between and after the ranges -- the same hashes, the oracle's over the same
    buffer, and the buffer as it was."""
    offs, lens, total = sc.packed_ranges()
    rng = np.random.default_rng(12)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    inside = sc.range_mask(offs, lens, total)
    other = np.where(inside, data, rng.integers(0, 256, total, dtype=np.uint8))
    assert (other != data).sum() > 64 and np.array_equal(other[inside], data[inside])
    want = oracle_native.checksums(data, offs, lens, nthreads=NT)
    b = ctx.checksum_batch(offs, lens)
    compared = 0
    for host in (data, other):
        d = torch.from_numpy(host).cuda()
        got = run_rows(b, d, len(lens))
        assert np.array_equal(d.cpu().numpy(), host)  # the input is not written
        mism = bad_rows(got, want)
        assert len(mism) == 0, [(int(offs[i]) % 128, int(lens[i])) for i in mism[:10]]
        compared += len(got)
    b.close()
    assert compared == 2 * len(lens) and len(lens) >= 50


@pytest.mark.parametrize("mode", list(MODES))
def test_cas_messages_ignore_surroundings(ctx, oracle_native, mode):
    """A staged cas message is zero-padded to its next 64-byte boundary (the ABI); nothing
    else around it may matter.  The C <= 9 messages at 16-byte aligned starts 0, 16, 32 and 48
    past a 64-byte boundary, random bytes before each and after its padding, two fills: equal
    hashes, the oracle's, and the staged buffer as it was."""
    cases = sc.sweep_a_small()
    sizes, cids, twins = sc.cas_files(cases)
    ext, d_staged = stage(ctx, sizes, cids, twins)
    staged = d_staged.cpu().numpy()
    mlen = ext["msg_len"].astype(np.uint64)
    offs, total = sc.pack_messages(mlen)
    assert {int(o) % 64 for o in offs} == {0, 16, 32, 48}
    packed = ext.copy()
    packed["msg_offset"] = offs
    free = sc.message_surroundings(offs, mlen, total)
    ids = oracle_native.cas_ids_synth(sizes, cids, twins, nthreads=NT)
    runs = []
    with tuning(whole_wave_max=MODES[mode]):
        b = ctx.cas_batch(packed)
        for seed in (31, 32):
            host = np.where(free, np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8), 0).astype(np.uint8)
            for o, p, L in zip(ext["msg_offset"], offs, mlen):
                host[int(p):int(p + L)] = staged[int(o):int(o + L)]
            d = torch.from_numpy(host).cuda()
            got = run_rows(b, d, len(cases))
            assert np.array_equal(d.cpu().numpy(), host)  # the input is not written
            mism = bad_rows(got, oracle_rows(oracle_native, host, packed))
            assert len(mism) == 0, [cases[i] for i in mism[:10]]
            assert np.array_equal(got[:, :8], ids)
            runs.append(got)
        b.close()
    assert np.array_equal(runs[0], runs[1])
    assert len(runs[0]) + len(runs[1]) == 2 * 62


# ----------------------------------------------------- D: output canaries
@pytest.mark.parametrize("mode", list(MODES))
def test_cas_batch_writes_only_its_rows(ctx, oracle_native, mode):
    """sd_cas_batch_run / _run_part between guard rows: a mixed batch -- whole-kind messages of
    every ninth sweep-A shape, sampled files, and whole-kind messages longer than the work
    lists take (102409 B up to 3 MiB: the checksum kernels, then k_scatter_hash).  run writes
    every row; SD_PART_SAMPLED leaves every whole-kind row at 0xA5 and SD_PART_WHOLE every
    sampled one; the two together are run's rows; no guard row is touched."""
    cases = sc.sweep_a()[::9]
    sizes, cids, twins, is_s0 = sc.interleave(sc.cas_files(cases), sc.sampled_files(40), seed=19)
    # the first and the last row belong to the whole-file kernels: a row index off by one
    # either way lands in a guard row
    assert not is_s0[0] and not is_s0[-1] and sizes[0] <= 102400 and sizes[-1] <= 102400
    ext0, total0 = stage_plan(sizes)
    long_lens = [sc.WHOLE_MSG_MAX + 1, 200008, sc.MiB + 3077, 3 * sc.MiB + 8]
    n = len(sizes) + len(long_lens)
    is_long = np.zeros(n, bool)
    is_long[[1, n // 3, n // 2, n - 2]] = True
    ext = np.zeros(n, EXTENT_DTYPE)
    ext[~is_long] = ext0
    off = (total0 + 127) // 128 * 128
    long_offs = []
    for row, L in zip(np.nonzero(is_long)[0], long_lens):  # a file of 5000 bytes that grew since
        ext[row] = (5000, off, L, SD_KIND_WHOLE)
        long_offs.append(off)
        off = (off + L + 64 + 127) // 128 * 128
    is_sampled = np.zeros(n, bool)
    is_sampled[~is_long] = is_s0
    _, d_staged = stage(ctx, sizes, cids, twins, staged_bytes=off)
    for k, (o, L) in enumerate(zip(long_offs, long_lens)):
        ctx.synth_fill(900 + k, 0, L, d_staged[o:])
    want = oracle_rows(oracle_native, d_staged.cpu().numpy(), ext)
    assert not untouched(want).any()
    with tuning(whole_wave_max=MODES[mode]):
        b = ctx.cas_batch(ext)
        assert b.n_sampled == 40 and b.n_whole == len(cases) + len(long_lens)
        full, part_s, part_w = Guarded(n, 32), Guarded(n, 32), Guarded(n, 32)
        b.run(d_staged, full.inner)
        b.run_part(1, d_staged, part_s.inner)  # SD_PART_SAMPLED
        b.run_part(2, d_staged, part_w.inner)  # SD_PART_WHOLE
        torch.cuda.synchronize()
        b.close()
    for g in (full, part_s, part_w):
        assert g.guards_intact()
    assert len(bad_rows(full.host(), want)) == 0
    s, w = part_s.host(), part_w.host()
    assert untouched(s[~is_sampled]).all() and np.array_equal(s[is_sampled], want[is_sampled])
    assert untouched(w[is_sampled]).all() and np.array_equal(w[~is_sampled], want[~is_sampled])
    assert np.array_equal(np.where(is_sampled[:, None], s, w), full.host())
    assert n == 78 + 40 + 4


def test_checksum_batch_writes_only_its_rows(ctx, oracle_native):
    """sd_checksum_batch_run between guard rows: the block pairs of sweep B and a three-block
    file, in both orders."""
    lens = [L for pair in sc.sweep_b_pairs()[::2] for L in pair] + [2 * sc.MiB + 1029]
    cids, twins = list(range(600, 600 + len(lens))), [0] * len(lens)
    compared = 0
    for order in (slice(None), slice(None, None, -1)):
        ls, cs_, ts = lens[order], cids[order], twins[order]
        offs, d = fill_files(ctx, ls, cs_, ts)
        b = ctx.checksum_batch(offs, ls)
        out = Guarded(len(ls), 32)
        b.run(d, out.inner)
        torch.cuda.synchronize()
        b.close()
        assert out.guards_intact()
        assert len(bad_rows(out.host(), want_checksums(oracle_native, ls, cs_, ts))) == 0, ls
        compared += len(ls)
    assert compared == 10


@pytest.fixture(params=[0, 1])
def dedup_variant(request):
    """sd_dedup_group: 0 = rocPRIM radix sort, 1 = LDS buckets (the default)."""
    with tuning(dedup_variant=request.param):
        yield request.param


def group_records(m: int, seed: int) -> np.ndarray:
    """m records (key, index): full-range 64-bit keys with groups of equal ones, indices in
    no order and spread over many identifier steps"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 64, m // 2 + 1, dtype=np.uint64)
    keys = pool[rng.integers(0, len(pool), m)]
    return np.stack([keys.view(np.int64), rng.permutation(m).astype(np.int64) * 3 + 5], axis=1).reshape(m, 2)


def test_dedup_group_writes_only_m_rows(ctx, dedup_variant):
    """sd_dedup_group sorts d_records[m] in place and writes d_rep[m]: record counts m around
    64 and 512 and none at all, the rows past m guarded.  (Uniform keys: no bucket grows past a
    wave here; test_dedup_group_bucket_sizes sweeps the bucket sizes.)"""
    compared = 0
    for m in sc.GROUP_M:
        recs = group_records(m, 40 + m)
        gr, grep, gng = group_host(recs)
        d_recs, d_rep = Guarded(m, 16, torch.int64), Guarded(m, 8, torch.int64)
        d_recs.inner.copy_(torch.from_numpy(recs.reshape(-1)))
        ng = ctx.dedup_group(d_recs.inner, m, d_rep.inner, index_sorted=False)
        assert d_recs.guards_intact() and d_rep.guards_intact(), m
        assert ng == gng, m
        assert np.array_equal(d_recs.host().view(np.int64).reshape(m, 2), gr.reshape(m, 2)), m
        assert np.array_equal(d_rep.host().view(np.int64).reshape(m), grep), m
        compared += 1
    assert compared == 10


def group_guarded(ctx, recs: np.ndarray, index_sorted: bool, what, fill_rep=None):
    """sd_dedup_group on guarded record and rep rows: records, representatives and the group
    count bit-exact against group_host, the guards intact."""
    m = len(recs)
    gr, grep, gng = group_host(recs)
    d_recs, d_rep = Guarded(m, 16, torch.int64), Guarded(m, 8, torch.int64)
    d_recs.inner.copy_(torch.from_numpy(np.ascontiguousarray(recs).reshape(-1)))
    if fill_rep is not None:
        d_rep.raw[G * 8:(G + m) * 8] = fill_rep
    ng = ctx.dedup_group(d_recs.inner, m, d_rep.inner, index_sorted=index_sorted)
    assert d_recs.guards_intact() and d_rep.guards_intact(), what
    assert ng == gng, what
    got = d_recs.host().view(np.int64).reshape(m, 2)
    bad = np.nonzero((got != gr.reshape(m, 2)).any(axis=1))[0]
    assert len(bad) == 0, (what, "records", bad[:8].tolist())
    bad = np.nonzero(d_rep.host().view(np.int64).reshape(m) != grep)[0]
    assert len(bad) == 0, (what, "rep", bad[:8].tolist())


@pytest.mark.parametrize("layout", list(sc.BUCKET_LAYOUTS))
def test_dedup_group_bucket_sizes(ctx, dedup_variant, layout):
    """Every branch of the LDS-bucket grouping on the size s of a bucket, one size either side of
    each border: registers (s <= 64), one wave in LDS with a carry between its two 64-record
    chunks (<= 128), k_gb_sort_big with wmax[] across waves, carry_s across 1024-record chunks
    and two pairs per lane at P = 4096 (<= 4096), and the overflow to the radix path (4097, also
    with index_sorted, which the host has to drop).  One bucket of exactly s records per case
    (shape_cases.bucket_case), its runs of equal keys by `layout`: a head at 0, a late head, a
    head on every 64-multiple, a group across every 64-multiple."""
    compared = 0
    for s, srt, recs in sc.bucket_cases(layout):
        group_guarded(ctx, recs, srt, (layout, s, srt))
        compared += 1
    assert compared == 2 * sc.BUCKET_CASES_PER_LAYOUT[layout]


def test_dedup_group_many_big_buckets(ctx, dedup_variant):
    """More big buckets (130) than k_gb_sort_big has workgroups (128): two workgroups take a
    second bucket; and m = 129 x 64 records all in buckets of 129, the most big[] can be asked to
    list for its m."""
    compared = 0
    for name, gen in (("many", sc.many_big_case), ("all", sc.all_big_case)):
        for srt in (False, True):
            group_guarded(ctx, gen(srt), srt, (name, srt))
            compared += 1
    assert compared == 4


def test_dedup_group_spans_and_lg_borders(ctx, dedup_variant):
    """(key - kmin) >> shift for key spans of 0..3, either side of 2^lg, 2^32 and 2^63, and all of
    u64, from kmin 0, 1, a high prefix and the largest that fits; and record counts either side
    of the first steps of gb_lg."""
    compared = 0
    for span, kmin, srt, recs in sc.span_cases():
        group_guarded(ctx, recs, srt, ("span", span, kmin, srt))
        compared += 1
    for m, srt, recs in sc.lg_border_cases():
        group_guarded(ctx, recs, srt, ("m", m, srt))
        compared += 1
    assert compared == 45 + 6


def test_dedup_owners_writes_only_m_rows(ctx):
    """sd_dedup_owners writes d_owner[m]: the reference's link-or-create rule per record, the
    rows past m guarded."""
    compared = 0
    for m in sc.GROUP_M:
        gr, grep, _ = group_host(group_records(m, 60 + m))
        gr = gr.reshape(m, 2)
        d_owner = Guarded(m, 8, torch.int64)
        ctx.dedup_owners(torch.from_numpy(gr.copy()).cuda(), m, torch.from_numpy(grep.copy()).cuda(), d_owner.inner,
                         chunk_size=100)
        want = np.where(gr[:, 1] // 100 == grep // 100, gr[:, 1], grep)
        assert d_owner.guards_intact(), m
        assert np.array_equal(d_owner.host().view(np.int64).reshape(m), want), m
        compared += 1
    assert compared == 10


# ----------------------------------------------------- E: stale scratch
def test_cas_batches_do_not_lean_on_stale_scratch(ctx, oracle_native):
    """A CV slot or merge item a run fails to write must not be rescued by what an earlier
    batch left in the same scratch: batch X (sweep A, work lists), then a batch Y of another
    count and other sizes, then X again, each created anew and run once into rows of 0xFF."""
    cases = sc.sweep_a()
    perm = np.random.default_rng(3).permutation(len(cases))
    x = tuple(a[perm] for a in sc.cas_files(cases))
    rng = np.random.default_rng(17)
    y = sc.interleave((rng.integers(0, 102401, 523).astype(np.uint64), np.arange(523, dtype=np.uint64) + 7000,
                       np.zeros(523, np.uint32)), sc.sampled_files(31, cid0=8000), seed=18)[:3]
    compared = 0
    with tuning(whole_wave_max=0, sampled_wave_max=0):
        for sizes, cids, twins in (x, y, x):
            ext, d_staged = stage(ctx, sizes, cids, twins)
            b = ctx.cas_batch(ext)
            got = run_rows(b, d_staged, len(sizes), fill=0xFF)
            b.close()
            mism = bad_rows(got, oracle_rows(oracle_native, d_staged.cpu().numpy(), ext))
            assert len(mism) == 0, [int(sizes[i]) for i in mism[:10]]
            compared += len(got)
            del d_staged
    assert compared == 700 + 554 + 700


def test_checksum_batches_do_not_lean_on_stale_scratch(ctx, oracle_native):
    """The same for two checksum batches of different block counts (11 and 23 blocks): the block
    CVs and reduce levels of one must not be what the other reads."""
    M = sc.MiB
    x = [3 * M + 5, 1, 2 * M, 4 * M - 1]
    y = [5 * M - 1, 700 * 1024, 9 * M + 3, 0, 3 * M, 2 * M + 1]
    compared = 0
    for k, lens in enumerate((x, y, x)):
        cids, twins = list(range(700 + 10 * k, 700 + 10 * k + len(lens))), [0] * len(lens)
        offs, d = fill_files(ctx, lens, cids, twins)
        b = ctx.checksum_batch(offs, lens)
        assert b.blocks == (11 if lens is x else 23)
        got = run_rows(b, d, len(lens), fill=0xFF)
        b.close()
        assert len(bad_rows(got, want_checksums(oracle_native, lens, cids, twins))) == 0, lens
        compared += len(lens)
    assert compared == 4 + 6 + 4


def test_dedup_group_not_leaning_on_stale_scratch(ctx, dedup_variant):
    """The grouping's state lives in scratch the context keeps between calls: an overflowing
    bucket (4097: `overflow` set, one big[] entry), then one wave-LDS bucket (65: no big bucket
    at all), then one big bucket (129), each into rep rows of 0xFF.  An `overflow`, `nbig` or
    big[] entry left from the call before would send a call down the wrong path."""
    compared = 0
    for s, layout, srt in ((4097, "late", True), (65, "pairs_shifted", False), (129, "late5", True)):
        group_guarded(ctx, sc.bucket_case(s, layout, srt), srt, (s, layout, srt), fill_rep=0xFF)
        compared += 1
    assert compared == 3


# ----------------------------------------------------- F: sd_dedup_partition sweep
@pytest.mark.parametrize("nparts", sc.PART_NPARTS)
def test_dedup_partition_sweep(ctx, nparts):
    """k_part_count / k_part_scan / k_part_scatter over keys 0, 2^64 - 1 and one either side of
    every destination boundary, n around the 256-lane step (most of the 1024 slices empty),
    every mask kind and no mask, two index bases: counts, the valid count and the records --
    destination-major, input order within a destination -- against partition_host, with
    d_counts guarded past nparts and d_records untouched past the valid records."""
    compared = 0
    for n, base, kind, keys, h, valid in sc.partition_cases(nparts):
        use = np.ones(n, bool) if valid is None else valid.astype(bool)
        idx = np.arange(n, dtype=np.int64) + base
        hrecs, hcounts = partition_host(keys[use], idx[use], nparts)
        assert all(0 <= sc.dest_of_int(int(k), nparts) < nparts for k in keys[:6 + 3 * nparts])
        d_counts, d_recs = Guarded(nparts, 8, torch.int64), Guarded(n, 16, torch.int64)
        nv = ctx.dedup_partition(torch.from_numpy(h).cuda(), None if valid is None else torch.from_numpy(valid).cuda(),
                                 n, base, nparts, d_counts.inner, d_recs.inner)
        what = (nparts, n, base, kind)
        assert d_counts.guards_intact() and d_recs.guards_intact(), what
        assert nv == int(use.sum()), what
        assert d_counts.host().view(np.int64).reshape(-1).tolist() == hcounts.tolist(), what
        rows = d_recs.host()
        assert np.array_equal(rows[:nv].view(np.int64).reshape(nv, 2), hrecs.reshape(nv, 2)), what
        assert untouched(rows[nv:]).all(), what
        compared += 1
    assert compared == 96


@pytest.mark.parametrize("nparts", [0, 65])
def test_dedup_partition_rejects_nparts(ctx, nparts):
    """nparts outside 1..64: SD_ERR_INVALID, and nothing written."""
    n = 300
    h = sc.hashes_from_keys(sc.partition_keys(64, n, 5), 6)
    d_counts, d_recs = Guarded(64, 8, torch.int64), Guarded(n, 16, torch.int64)
    with pytest.raises(SdCasError) as e:
        ctx.dedup_partition(torch.from_numpy(h).cuda(), None, n, 0, nparts, d_counts.inner, d_recs.inner)
    assert e.value.rc == -1  # SD_ERR_INVALID
    for g in (d_counts, d_recs):
        assert g.guards_intact() and untouched(g.host()).all()
