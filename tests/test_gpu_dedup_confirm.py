"""sd_dedup_confirm (include/sd_cas.h, csrc/dedup_confirm.hip) -- run on an MI355X: -m gpu.
Every case of tests/dedup_confirm_cases.py down both paths (the default and "confirm_full_sort"
1), bit-exact against the dict model and so against each other; every output between 0xA5 guard
rows and pre-filled, so a write outside the rows a call owns, or a missing one, shows; the
capacity rule; the path counters; stale scratch; and end to end from planted bytes on the device."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError  # noqa: E402
from tests import dedup_confirm_cases as dc  # noqa: E402
from tests.test_gpu_object_index import Guarded, POISON, dev, host_u64  # noqa: E402

U = np.uint64
SPARE = 5  # set rows past the requirement: they keep their fill


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


@pytest.fixture(scope="module")
def cases():
    return dc.all_cases()


@pytest.fixture(autouse=True)
def adaptive_again():
    yield
    sd.set_tuning("confirm_full_sort", 0)


def upload(keys, hashes, valid):
    m = len(keys)
    d_keys = dev(keys) if m else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_hash = torch.from_numpy(np.ascontiguousarray(hashes, np.uint8).reshape(-1)).cuda() if m else \
        torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_valid = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).cuda()
    return d_keys, d_hash, d_valid


def run_guarded(ctx, d_keys, d_hash, d_valid, m, rows, capacity):
    """one call with every output guarded -> (rep, size, verdict, all set rows, n_sets, stats, rc)"""
    g_rep, g_size = Guarded(m, 8, torch.int64), Guarded(m, 8, torch.int64)
    g_verdict, g_sets = Guarded(m, 1), Guarded(rows, 24, torch.int64)
    rc = 0
    try:
        n_sets, stats = ctx.dedup_confirm(d_keys, d_hash, d_valid, m, g_rep.inner, g_size.inner, g_verdict.inner,
                                          g_sets.inner, capacity)
    except SdCasError as e:
        rc, n_sets, stats = e.rc, e.needed, e.stats
    for g in (g_rep, g_size, g_verdict, g_sets):
        assert g.guards_intact(), m
    return (g_rep.host().view(U).reshape(-1), g_size.host().view(U).reshape(-1), g_verdict.host().reshape(-1),
            g_sets.host().view(U).reshape(-1, 3), n_sets, stats, rc)


def assert_case(ctx, case, full: int):
    name, keys, hashes, valid, want, tie = case
    m, n = len(keys), len(want["sets"])
    sd.set_tuning("confirm_full_sort", full)
    before = ctx.dedup_confirm_stats()
    d_keys, d_hash, d_valid = upload(keys, hashes, valid)
    rep, size, verdict, sets, n_sets, stats, rc = run_guarded(ctx, d_keys, d_hash, d_valid, m, n + SPARE, n + SPARE)
    what = (name, full)
    assert rc == 0 and n_sets == n, what
    assert np.array_equal(rep, want["rep"]) and np.array_equal(size, want["size"]), what
    assert np.array_equal(verdict, want["verdict"]), what
    assert np.array_equal(sets[:n], want["sets"]) and (sets[n:] == U(0xA5A5A5A5A5A5A5A5)).all(), what
    assert np.array_equal(stats, want["stats"]), what
    dc.check_identities(stats)
    if m:  # the inputs are not written
        assert np.array_equal(host_u64(d_keys), keys) and np.array_equal(d_hash.cpu().numpy(), hashes.reshape(-1)), what
    after = ctx.dedup_confirm_stats()
    took_full = bool(full or tie) and m > 0
    assert after["full"] - before["full"] == (1 if took_full else 0), what
    assert after["prefix"] - before["prefix"] == (1 if m > 0 and not took_full else 0), what


def test_every_case_on_both_paths(ctx, cases):
    """Identical to the model -- and so to each other -- at the default and with the full-width
    sort forced; the counters say which path each call took."""
    for case in cases:
        for full in (0, 1):
            assert_case(ctx, case, full)


@pytest.mark.parametrize("m", dc.SLICE_COUNTS)
def test_both_paths_at_a_slice_border(ctx, m):
    """The counts at which a sliced pass's arithmetic changes (tests/sliced_cases.py), as the
    Object index has them in tests/test_gpu_object_index_slices.py: bit-exact and between guard
    rows down both paths."""
    case = dc.border_case(m)
    for full in (0, 1):
        assert_case(ctx, case, full)


def test_path_counters(ctx, cases):
    """The random mix and the uniform tie run finish on the prefix path; tails A, B, A take the
    full-width path."""
    by = {c[0]: c for c in cases}
    for name, key in (("random_mix", "prefix"), ("tie_uniform", "prefix"), ("tie_aba", "full")):
        _, keys, hashes, valid, want, _ = by[name]
        before = ctx.dedup_confirm_stats()
        rep, size, verdict, sets, stats = dedup.confirm_device(ctx, *upload(keys, hashes, valid))
        after = ctx.dedup_confirm_stats()
        other = "full" if key == "prefix" else "prefix"
        assert after[key] - before[key] == 1 and after[other] == before[other], name
        assert np.array_equal(host_u64(rep), want["rep"]) and np.array_equal(host_u64(sets).reshape(-1, 3), want["sets"]), name
        assert np.array_equal(verdict.cpu().numpy(), want["verdict"]) and np.array_equal(stats, want["stats"]), name
    assert by["tie_aba"][4]["rep"].tolist() == [0, 1, 0]


@pytest.mark.parametrize("full", [0, 1])
def test_capacity_one_short(ctx, cases, full):
    """SD_ERR_CAPACITY: the requirement in *n_sets, no set row written, the per-file outputs and
    the stats complete; and with exactly enough nothing past the rows; count-only calls."""
    sd.set_tuning("confirm_full_sort", full)
    for name in ("size_513_valid", "tie_among_others"):
        _, keys, hashes, valid, want, _ = next(c for c in cases if c[0] == name)
        m, n = len(keys), len(want["sets"])
        assert n >= 2
        d_keys, d_hash, d_valid = upload(keys, hashes, valid)
        for cap in (n - 1, 0):
            rep, size, verdict, sets, n_sets, stats, rc = run_guarded(ctx, d_keys, d_hash, d_valid, m, n + SPARE, cap)
            assert rc == SD_ERR_CAPACITY and n_sets == n and (sets == U(0xA5A5A5A5A5A5A5A5)).all(), (name, cap)
            assert np.array_equal(rep, want["rep"]) and np.array_equal(size, want["size"]), (name, cap)
            assert np.array_equal(verdict, want["verdict"]) and np.array_equal(stats, want["stats"]), (name, cap)
        rep, size, verdict, sets, n_sets, stats, rc = run_guarded(ctx, d_keys, d_hash, d_valid, m, n + SPARE, n)
        assert rc == 0 and np.array_equal(sets[:n], want["sets"]) and (sets[n:] == U(0xA5A5A5A5A5A5A5A5)).all()
        n_sets, stats = ctx.dedup_confirm(d_keys, d_hash, d_valid, m)  # every output NULL: only counts
        assert n_sets == n and np.array_equal(stats, want["stats"])


def test_invalid_arguments(ctx):
    from spacedrive_amd._native import lib
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    n = ctypes.c_uint64(0)
    for keys, hashes in ((None, d.data_ptr()), (d.data_ptr(), None)):
        rc = lib().sd_dedup_confirm(ctx.handle, keys, hashes, None, 2, None, None, None, None, 0, ctypes.byref(n), None, None)
        assert rc == -1
    assert lib().sd_dedup_confirm(ctx.handle, None, None, None, 0, None, None, None, None, 0, ctypes.byref(n), None, None) == 0
    assert n.value == 0


def test_large_then_small_on_one_context(ctx, cases):
    """The scratch is the context's and grow-only: a small call after a large one reads nothing
    the large one left behind."""
    by = {c[0]: c for c in cases}
    for full in (0, 1):
        assert_case(ctx, by["past_grid"], full)
        for name in ("size_65_valid", "tie_aba", "size_1", "extremes", "size_513"):
            assert_case(ctx, by[name], full)


def test_end_to_end_on_the_device(ctx):
    """Planted bytes filled on the device -> sd_fingerprint_batch_run -> keys_from_hashes_device ->
    sd_dedup_confirm; nothing comes back to the host before the verdicts.  The expectation follows
    from the plant alone."""
    files = dc.planted_files()
    lens = [L for L, _, _ in files]
    offs, off = [], 0
    for L in lens:
        offs.append(off)
        off = (off + L + 127) // 64 * 64
    data = torch.zeros(off + 64, dtype=torch.uint8, device="cuda")
    for (L, c, t), o in zip(files, offs):
        ctx.synth_fill(c, t, L, data[o:])
    fb = ctx.fingerprint_batch(offs, lens)
    n = len(files)
    d_cas = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_sum = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    fb.run(data, d_cas, d_sum)
    d_keys = dedup.keys_from_hashes_device(d_cas, ctx)
    rep, size, verdict, sets, stats = dedup.confirm_device(ctx, d_keys, d_sum)
    want_rep, want_size, want_verdict = dc.planted_expectation(files)
    assert host_u64(rep).tolist() == want_rep and host_u64(size).tolist() == want_size
    assert verdict.cpu().numpy().tolist() == want_verdict
    assert stats.tolist() == [28, 20, 4, 23, 4, 9, 3, 3]
    # the keys are the cas hashes' first 8 bytes, big-endian; the sets ascend by them
    keys = host_u64(d_keys)
    assert np.array_equal(keys, dedup.keys_from_hashes(d_cas.cpu().numpy().reshape(n, 32)))
    s = host_u64(sets).reshape(-1, 3)
    assert len(s) == 4 and np.all(s[1:, 0] >= s[:-1, 0]) and len({int(k) for k in s[:, 0]}) == 3  # 501: two sets, one key
    assert sorted(int(r) for r in s[:, 1]) == sorted({r for r, v in zip(want_rep, want_verdict) if v == dc.CONFIRMED})
    for (L, c, t), k in zip(files, keys):  # a twin shares its original's key
        if t:
            assert k == keys[files.index((L, c, 0))]
