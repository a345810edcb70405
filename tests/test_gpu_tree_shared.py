"""sd_checksum_tree_shared (include/sd_cas.h, csrc/tree_shared.hip) -- run on an MI355X: -m gpu.
Every case of tests/tree_shared_cases.py down both grouping paths (the default and
"confirm_full_sort" 1), bit-exact against the restatement and so against each other; every output
between 0xA5 guard rows and pre-filled, so a write outside the rows a call owns, or a missing one,
shows (a tie case at the default comes out right only if the full-width path ran: the prefix path
writes nothing then); min_blocks; the capacity rule; every combination of NULL outputs; stale
scratch; and end to end from real bytes on the device through ChecksumTree.run."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd import cpu  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError  # noqa: E402
from tests import tree_shared_cases as tc  # noqa: E402
from tests.test_gpu_object_index import Guarded  # noqa: E402

U = np.uint64
FILL = U(0xA5A5A5A5A5A5A5A5)
SPARE = 5  # pair rows past the requirement: they keep their fill


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


@pytest.fixture(scope="module")
def cases():
    return tc.all_cases()


@pytest.fixture(autouse=True)
def adaptive_again():
    yield
    sd.set_tuning("confirm_full_sort", 0)


def upload(nodes):
    flat = np.ascontiguousarray(nodes, np.uint8).reshape(-1)
    return torch.from_numpy(flat).cuda() if flat.size else torch.zeros(32, dtype=torch.uint8, device="cuda")


def run_guarded(ctx, lens, k, d_nodes, m, rows, capacity, min_blocks=0, mask=15):
    """one call with the outputs of `mask` guarded -> (rep, size, files, all pair rows, n_pairs, stats, rc)"""
    n = len(lens)
    g_rep, g_size = Guarded(m, 8, torch.int64), Guarded(m, 8, torch.int64)
    g_files, g_pairs = Guarded(n, 32, torch.int64), Guarded(rows, 32, torch.int64)
    rc = 0
    try:
        n_pairs, stats = ctx.checksum_tree_shared(lens, d_nodes, k, min_blocks, g_rep.inner if mask & 1 else None,
                                                  g_size.inner if mask & 2 else None, g_files.inner if mask & 4 else None,
                                                  g_pairs.inner if mask & 8 else None, capacity)
    except SdCasError as e:
        rc, n_pairs, stats = e.rc, e.needed, e.stats
    for g in (g_rep, g_size, g_files, g_pairs):
        assert g.guards_intact(), m
    return (g_rep.host().view(U).reshape(-1), g_size.host().view(U).reshape(-1), g_files.host().view(U).reshape(-1, 4),
            g_pairs.host().view(U).reshape(-1, 4), n_pairs, stats, rc)


def assert_case(ctx, case, full: int, min_blocks: int = 0, want=None):
    name, lens, k, nodes, want0, tie = case
    want = want0 if want is None else want
    m, rows = len(want["rep"]), len(want["pairs"])
    sd.set_tuning("confirm_full_sort", full)
    d_nodes = upload(nodes)
    rep, size, files, pairs, n_pairs, stats, rc = run_guarded(ctx, lens, k, d_nodes, m, rows + SPARE, rows + SPARE,
                                                              min_blocks)
    what = (name, full, min_blocks)
    assert rc == 0 and n_pairs == rows, what
    assert np.array_equal(rep, want["rep"]) and np.array_equal(size, want["size"]), what
    assert np.array_equal(files, want["files"]), what
    assert np.array_equal(pairs[:rows], want["pairs"]) and (pairs[rows:] == FILL).all(), what
    assert np.array_equal(stats, want["stats"]), what
    tc.check_identities({"files": files, "pairs": pairs[:rows], "stats": stats}, min_blocks)
    if m:  # the input is not written
        assert np.array_equal(d_nodes.cpu().numpy(), np.asarray(nodes, np.uint8).reshape(-1)), what


def test_every_case_on_both_paths(ctx, cases):
    """Identical to the restatement -- and so to each other -- at the default and with the full-width
    sort forced.  The cases that tie reach the right answer at the default only through the fallback."""
    assert {c[0] for c in cases if c[5]} == {"tie_aba", "tie_among_others"}
    for case in cases:
        for full in (0, 1):
            assert_case(ctx, case, full)


def test_large_then_small_on_one_context(ctx, cases):
    """The scratch is the context's and grow-only: a small call after a large one reads nothing the
    large one left behind."""
    by = {c[0]: c for c in cases}
    for full in (0, 1):
        assert_case(ctx, by["past_grid"], full)
        for name in ("slots_65", "tie_aba", "slots_1", "empty_files", "run_of_700", "no_files", "tail_other_holder"):
            assert_case(ctx, by[name], full)


@pytest.mark.parametrize("min_blocks", tc.MIN_BLOCKS)
def test_min_blocks(ctx, cases, min_blocks):
    """None, the floor, exactly a pair's count, one above and above all: the filter moves the rows and
    nothing else."""
    by = {c[0]: c for c in cases}
    for name in ("min_blocks", "run_of_700", "tail_other_holder", "slots_257"):
        _, lens, k, nodes, want0, _ = by[name]
        want = tc.shared_model(lens, k, nodes, min_blocks)
        assert np.array_equal(want["stats"], want0["stats"])
        assert_case(ctx, by[name], 0, min_blocks, want)


def test_capacity_exact_short_and_count_only(ctx, cases):
    """SD_ERR_CAPACITY: the requirement in *n_pairs, no pair row written, every other output and the
    stats complete; with exactly enough nothing past the rows; count-only calls."""
    for name in ("slots_257", "class_of_300"):
        _, lens, k, nodes, want, _ = next(c for c in cases if c[0] == name)
        m, rows = len(want["rep"]), len(want["pairs"])
        assert rows >= 3
        d_nodes = upload(nodes)
        for cap in (rows - 1, 0):
            rep, size, files, pairs, n_pairs, stats, rc = run_guarded(ctx, lens, k, d_nodes, m, rows + SPARE, cap)
            assert rc == SD_ERR_CAPACITY and n_pairs == rows and (pairs == FILL).all(), (name, cap)
            assert np.array_equal(rep, want["rep"]) and np.array_equal(size, want["size"]), (name, cap)
            assert np.array_equal(files, want["files"]) and np.array_equal(stats, want["stats"]), (name, cap)
        rep, size, files, pairs, n_pairs, stats, rc = run_guarded(ctx, lens, k, d_nodes, m, rows + SPARE, rows)
        assert rc == 0 and np.array_equal(pairs[:rows], want["pairs"]) and (pairs[rows:] == FILL).all()
        n_pairs, stats = ctx.checksum_tree_shared(lens, d_nodes, k)  # every output NULL: only counts
        assert n_pairs == rows and np.array_equal(stats, want["stats"])


def test_null_outputs_in_every_combination(ctx, cases):
    """Any output pointer may be NULL: the others are complete, the absent ones' buffers untouched."""
    from spacedrive_amd._native import lib
    _, lens, k, nodes, want, _ = next(c for c in cases if c[0] == "tail_other_holder")
    m, rows = len(want["rep"]), len(want["pairs"])
    d_nodes = upload(nodes)
    for mask in range(16):
        rep, size, files, pairs, n_pairs, stats, rc = run_guarded(ctx, lens, k, d_nodes, m, rows, rows, 0, mask)
        assert rc == 0 and n_pairs == rows and np.array_equal(stats, want["stats"]), mask
        for bit, got, key in ((1, rep, "rep"), (2, size, "size"), (4, files, "files"), (8, pairs, "pairs")):
            assert np.array_equal(got, want[key]) if mask & bit else (got == FILL).all(), (mask, key)
    ls = np.ascontiguousarray(lens, U)
    n_pairs = ctypes.c_uint64(77)  # and the two host outputs
    assert lib().sd_checksum_tree_shared(ctx.handle, ls.ctypes.data, len(ls), k, d_nodes.data_ptr(), 0, None, None, None,
                                         None, 0, None, None, None) == 0
    assert lib().sd_checksum_tree_shared(ctx.handle, ls.ctypes.data, len(ls), k, d_nodes.data_ptr(), 0, None, None, None,
                                         None, 0, ctypes.byref(n_pairs), None, None) == 0 and n_pairs.value == rows


def test_invalid_arguments(ctx):
    from spacedrive_amd._native import lib
    d = torch.zeros(256, dtype=torch.uint8, device="cuda")
    lens = np.array([5, 300_000], U)
    n = ctypes.c_uint64(0)

    def call(lens_p, count, k, nodes_p):
        return lib().sd_checksum_tree_shared(ctx.handle, lens_p, count, k, nodes_p, 0, None, None, None, None, 0,
                                             ctypes.byref(n), None, None)
    for k in (16, 21):
        assert call(lens.ctypes.data, 2, k, d.data_ptr()) == -1
        assert call(None, 0, k, None) == -1
    assert call(None, 2, 17, d.data_ptr()) == -1 and call(lens.ctypes.data, 2, 17, None) == -1
    assert call(lens.ctypes.data, 2, 17, d.data_ptr() + 8) == -1  # not 16-byte aligned
    assert call(lens.ctypes.data, 1 << 32, 17, d.data_ptr()) == -1
    assert call(None, 0, 17, None) == 0 and n.value == 0


def test_end_to_end_on_the_device(ctx):
    """Real bytes on the device -> ChecksumTree.run -> sd_checksum_tree_shared; the levels never
    leave the device.  Against the plant, and against the CPU chain on the same bytes."""
    contents, want_files, want_pairs = tc.scenario()
    buf, offs, lens = tc.scenario_buffer(contents)
    d_data = torch.from_numpy(buf).cuda()
    t = ctx.checksum_tree(offs, lens, 17)
    d_nodes = torch.zeros(32 * t.total_nodes, dtype=torch.uint8, device="cuda")
    d_roots = torch.zeros(32 * t.n, dtype=torch.uint8, device="cuda")
    t.run(d_data, d_nodes, d_roots)
    m = t.total_nodes
    rep, size, files, pairs, n_pairs, stats, rc = run_guarded(ctx, lens, 17, d_nodes, m, len(want_pairs) + SPARE,
                                                              len(want_pairs) + SPARE)
    assert rc == 0 and files.tolist() == want_files and pairs[:n_pairs].tolist() == want_pairs
    nodes, roots, _ = cpu.checksum_tree(buf, offs, lens, 17)
    assert np.array_equal(d_nodes.cpu().numpy().reshape(-1, 32), nodes)
    c_rep, c_size, c_files, c_pairs, c_stats = cpu.checksum_tree_shared(lens, nodes, 17)
    assert np.array_equal(rep, c_rep) and np.array_equal(size, c_size) and np.array_equal(files, c_files)
    assert np.array_equal(pairs[:n_pairs], c_pairs) and np.array_equal(stats, c_stats)
    assert stats.tolist()[:5] == [6, 34, 13, 7, 21] and stats.tolist()[6:] == [4, 2]
