"""The content-defined chunks on the device (include/sd_cas.h, content-defined chunks; csrc/cdc.hip,
csrc/tree_shared.hip) -- run on an MI355X: -m gpu.  Every case of tests/cdc_cases.py through the
scan, select and hash kernels: cuts and statistics against the numpy restatement, ids against the
oracle's BLAKE3, everything byte for byte against the CPU twins; the outputs between 0xA5 guard
rows; the shared report down both grouping paths, with min_chunks, the capacity rule and every
combination of NULL outputs; the refusals."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd import cdc, cpu  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from tests import cdc_cases as cc  # noqa: E402
from tests.test_cdc import BAD_PARAMS  # noqa: E402
from tests.test_gpu_object_index import Guarded  # noqa: E402

U = np.uint64
FILL = U(0xA5A5A5A5A5A5A5A5)
SPARE = 5


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = sd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


@pytest.fixture(scope="module")
def cases():
    return cc.all_cases()


@pytest.fixture(autouse=True)
def adaptive_again():
    yield
    sd.set_tuning("confirm_full_sort", 0)


def run_case(ctx, case, mask=3):
    """cut + hash with the outputs of `mask` (1 chunks, 2 ids) guarded -> (base, chunks, ids, stats,
    d_chunks, d_ids, the batch)"""
    name, buf, offs, lens, params, want = case
    d_data = torch.from_numpy(buf).cuda()
    c = sd.Cdc(ctx, offs, lens, params)
    m = c.cut(d_data)
    assert m == len(want["chunks"]), name
    g_chunks, g_ids = Guarded(m, 16, torch.int64), Guarded(m, 32)
    c.hash(d_data, g_chunks.inner if mask & 1 else None, g_ids.inner if mask & 2 else None)
    torch.cuda.synchronize()
    assert g_chunks.guards_intact() and g_ids.guards_intact(), name
    assert np.array_equal(d_data.cpu().numpy(), buf), name  # the input is not written
    return c.layout(), g_chunks.host().view(U).reshape(-1, 2), g_ids.host().reshape(-1, 32), c.stats(), g_chunks, g_ids, c


def assert_case(ctx, case):
    name, buf, offs, lens, params, want = case
    base, chunks, ids, stats, _, _, c = run_case(ctx, case)
    assert np.array_equal(base, want["base"]) and np.array_equal(chunks, want["chunks"]), name
    assert np.array_equal(stats, want["stats"]), (name, stats, want["stats"])
    assert np.array_equal(ids, want["ids"]), (name, np.flatnonzero((ids != want["ids"]).any(axis=1))[:8])
    c_base, c_chunks, c_stats = cpu.cdc_cut(buf, offs, lens, params)  # and the CPU twins, byte for byte
    assert np.array_equal(base, c_base) and np.array_equal(chunks, c_chunks) and np.array_equal(stats, c_stats), name
    assert np.array_equal(ids, cpu.cdc_hash(buf, offs, lens, c_base, c_chunks)), name
    c.close()


def test_gear_table():
    g = cpu.cdc_gear()
    assert np.array_equal(g, cc.GEAR) and int(g[0]) == 0x2df3228afbc5cb53 and int(g[255]) == 0xdd9fba0f5362ab8e


def test_every_case(ctx, cases):
    assert len(cases) >= 30 and {c[4] for c in cases} >= set(cc.PARAM_SETS)
    for case in cases:
        assert_case(ctx, case)


def test_many_chunks_and_many_files(ctx):
    """more than 1024 * 256 chunks in one batch, past a sliced grid; 70 000 files of 1 to 200 bytes"""
    many = cc.all_cases(True)
    assert len(many[0][5]["chunks"]) >= 1024 * 256 + 1 and len(many[1][3]) >= 70_000
    for case in many:
        assert_case(ctx, case)


def test_file_start_is_clipped(ctx, cases):
    """the bytes of a stand-alone file 16 bytes after another range's start: the same cuts and ids, so
    no byte of the neighbour warms the rolling value"""
    by = {c[0]: c for c in cases}
    pair, alone = run_case(ctx, by["starts_pair"]), run_case(ctx, by["starts_alone"])
    k = int(pair[0][1])
    assert np.array_equal(pair[1][k:], alone[1]) and np.array_equal(pair[2][k:], alone[2])


def test_recut_and_large_then_small(ctx, cases):
    """a batch cut and hashed twice gives the same; a small batch after a large one on the same
    context reads nothing the large one left behind"""
    by = {c[0]: c for c in cases}
    name, buf, offs, lens, params, want = by["params_default"]
    d_data = torch.from_numpy(buf).cuda()
    c = sd.Cdc(ctx, offs, lens, params)
    for _ in range(2):
        m = c.cut(d_data)
        d_ids = torch.zeros((m, 32), dtype=torch.uint8, device="cuda")
        c.hash(d_data, None, d_ids)
        assert np.array_equal(d_ids.cpu().numpy(), want["ids"]) and np.array_equal(c.stats(), want["stats"])
    c.close()
    for name in ("shift", "lengths_p8", "hash_big", "cand_at_len"):
        assert_case(ctx, by[name])


def test_hash_null_outputs(ctx, cases):
    case = next(c for c in cases if c[0] == "params_p8")
    want = case[5]
    for mask in range(4):
        _, chunks, ids, stats, _, _, c = run_case(ctx, case, mask)
        assert np.array_equal(chunks, want["chunks"]) if mask & 1 else (chunks == FILL).all(), mask
        assert np.array_equal(ids, want["ids"]) if mask & 2 else (ids == 0xA5).all(), mask
        c.close()


# ---------------------------------------------------------------- the shared report
def shared_guarded(ctx, base, d_chunks, d_ids, m, rows, capacity, min_chunks=0, mask=15):
    n = len(base) - 1
    g_rep, g_size = Guarded(m, 8, torch.int64), Guarded(m, 8, torch.int64)
    g_files, g_pairs = Guarded(n, 32, torch.int64), Guarded(rows, 32, torch.int64)
    rc = 0
    try:
        n_pairs, stats = cdc.shared(ctx, base, d_chunks, d_ids, min_chunks, g_rep.inner if mask & 1 else None,
                                    g_size.inner if mask & 2 else None, g_files.inner if mask & 4 else None,
                                    g_pairs.inner if mask & 8 else None, capacity)
    except SdCasError as e:
        rc, n_pairs, stats = e.rc, e.needed, e.stats
    for g in (g_rep, g_size, g_files, g_pairs):
        assert g.guards_intact()
    return {"rep": g_rep.host().view(U).reshape(-1), "size": g_size.host().view(U).reshape(-1),
            "files": g_files.host().view(U).reshape(-1, 4), "pairs": g_pairs.host().view(U).reshape(-1, 4),
            "stats": stats}, n_pairs, rc


@pytest.fixture(scope="module")
def shifted(ctx, cases):
    """the shift case cut and hashed on the device: (want, d_chunks, d_ids), the outputs kept resident"""
    case = next(c for c in cases if c[0] == "shift")
    base, chunks, ids, stats, g_chunks, g_ids, c = run_case(ctx, case)
    assert np.array_equal(chunks, case[5]["chunks"]) and np.array_equal(ids, case[5]["ids"])
    return case, g_chunks.inner, g_ids.inner


def assert_shared(ctx, want, d_chunks, d_ids, full, min_chunks=0):
    model = cc.shared_model(want["base"], want["chunks"], want["ids"], min_chunks)
    m, rows = len(want["chunks"]), len(model["pairs"])
    sd.set_tuning("confirm_full_sort", full)
    got, n_pairs, rc = shared_guarded(ctx, want["base"], d_chunks, d_ids, m, rows + SPARE, rows + SPARE, min_chunks)
    assert rc == 0 and n_pairs == rows, (full, min_chunks)
    for k in ("rep", "size", "files", "stats"):
        assert np.array_equal(got[k], model[k]), (k, full, min_chunks)
    assert np.array_equal(got["pairs"][:rows], model["pairs"]) and (got["pairs"][rows:] == FILL).all()
    got["pairs"] = got["pairs"][:rows]
    cc.check_identities(got, min_chunks)
    c = dict(zip(("rep", "size", "files", "pairs", "stats"), cpu.cdc_shared(want["base"], want["chunks"], want["ids"], min_chunks)))
    for k in c:
        assert np.array_equal(got[k], c[k]), k
    return got


def test_shift_is_found(ctx, shifted):
    """The reason for the feature.  5 bytes in front of, or in the middle of, 1 MiB: every chunk of the
    copy but at most 3 is redundant with its representative in the original, on both grouping paths;
    sd_checksum_tree_shared over the same two files finds no redundant block."""
    (name, buf, offs, lens, params, want), d_chunks, d_ids = shifted
    for full in (0, 1):
        got = assert_shared(ctx, want, d_chunks, d_ids, full)
        pairs = {(int(f), int(g)): int(c) for f, g, c, _ in got["pairs"]}
        for f in (1, 2):
            assert int(got["files"][f, 0]) - pairs[(f, 0)] <= 3 and pairs[(f, 0)] == int(got["files"][f, 2])
    d_data = torch.from_numpy(buf).cuda()
    t = ctx.checksum_tree(offs[:2], lens[:2], 17)
    d_nodes = torch.zeros(32 * t.total_nodes, dtype=torch.uint8, device="cuda")
    d_roots = torch.zeros(32 * t.n, dtype=torch.uint8, device="cuda")
    t.run(d_data, d_nodes, d_roots)
    _, stats = ctx.checksum_tree_shared(lens[:2], d_nodes, 17)
    assert int(stats[4]) == 0


def test_a_file_that_repeats_itself(ctx, cases):
    case = next(c for c in cases if c[0] == "twice")
    _, _, _, _, g_chunks, g_ids, c = run_case(ctx, case)
    for full in (0, 1):
        got = assert_shared(ctx, case[5], g_chunks.inner, g_ids.inner, full)
        st, files = got["stats"], got["files"]
        assert int(st[7]) > 0 and int(st[7]) == int(files[0, 2])
        assert got["pairs"].tolist() == [[1, 0, int(files[1, 0]), 1 << 18]]
        assert int(got["pairs"][:, 2].sum()) == int(st[4]) - int(st[7])


@pytest.mark.parametrize("min_chunks", [0, 1, 2, 700])
def test_shared_min_chunks(ctx, shifted, min_chunks):
    (_, _, _, _, _, want), d_chunks, d_ids = shifted
    got = assert_shared(ctx, want, d_chunks, d_ids, 0, min_chunks)
    assert len(got["pairs"]) >= 2


def test_shared_on_small_cases(ctx, cases):
    """the report over batches with empty files, one-byte files, constant bytes and equal chunks inside a file"""
    by = {c[0]: c for c in cases}
    for name in ("lengths_p8", "dense", "all_zero", "mask1_64_64", "starts_pair", "tile_lens"):
        _, _, _, _, g_chunks, g_ids, c = run_case(ctx, by[name])
        for full in (0, 1):
            assert_shared(ctx, by[name][5], g_chunks.inner, g_ids.inner, full)


def test_shared_capacity_exact_short_and_null_outputs(ctx, shifted):
    (_, _, _, _, _, want), d_chunks, d_ids = shifted
    model = cc.shared_model(want["base"], want["chunks"], want["ids"])
    m, rows = len(want["chunks"]), len(model["pairs"])
    assert rows >= 3
    for cap in (rows - 1, 0):  # one short, and none: the requirement, no row, everything else complete
        got, n_pairs, rc = shared_guarded(ctx, want["base"], d_chunks, d_ids, m, rows + SPARE, cap)
        assert rc == SD_ERR_CAPACITY and n_pairs == rows and (got["pairs"] == FILL).all(), cap
        for k in ("rep", "size", "files", "stats"):
            assert np.array_equal(got[k], model[k]), (k, cap)
    got, n_pairs, rc = shared_guarded(ctx, want["base"], d_chunks, d_ids, m, rows + SPARE, rows)  # exact
    assert rc == 0 and np.array_equal(got["pairs"][:rows], model["pairs"]) and (got["pairs"][rows:] == FILL).all()
    for mask in range(16):
        got, n_pairs, rc = shared_guarded(ctx, want["base"], d_chunks, d_ids, m, rows, rows, 0, mask)
        assert rc == 0 and n_pairs == rows and np.array_equal(got["stats"], model["stats"]), mask
        for bit, key in ((1, "rep"), (2, "size"), (4, "files"), (8, "pairs")):
            assert np.array_equal(got[key], model[key]) if mask & bit else (got[key] == FILL).all(), (mask, key)
    n_pairs, stats = cdc.shared(ctx, want["base"], d_chunks, d_ids)  # every output NULL: only counts
    assert n_pairs == rows and np.array_equal(stats, model["stats"])
    base = want["base"]
    assert lib().sd_cdc_shared(ctx.handle, base.ctypes.data, len(base) - 1, d_chunks.data_ptr(), d_ids.data_ptr(), 0, None,
                               None, None, None, 0, None, None, None) == 0
    n = ctypes.c_uint64(7)
    assert lib().sd_cdc_shared(ctx.handle, None, 0, None, None, 0, None, None, None, None, 0, ctypes.byref(n), None, None) == 0
    assert n.value == 0
    assert lib().sd_cdc_shared(ctx.handle, base.ctypes.data, len(base) - 1, d_chunks.data_ptr(), d_ids.data_ptr() + 8, 0,
                               None, None, None, None, 0, None, None, None) == -1
    assert lib().sd_cdc_shared(ctx.handle, base.ctypes.data, len(base) - 1, None, d_ids.data_ptr(), 0, None, None, None,
                               None, 0, None, None, None) == -1


# ---------------------------------------------------------------- refusals, files
def test_refusals(ctx):
    d = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    offs, lens = np.array([0, 1024], U), np.array([1000, 2000], U)
    h = ctypes.c_void_p()

    def create(o, ln, n, pr):
        p = cpu.CdcParams(*pr) if pr is not None else None
        return lib().sd_cdc_create(ctx.handle, None if o is None else o.ctypes.data, None if ln is None else ln.ctypes.data, n,
                                   None if p is None else ctypes.byref(p), ctypes.byref(h))
    for bad in BAD_PARAMS:
        assert create(offs, lens, 2, bad + (0,)) == -1, bad
    assert create(offs, lens, 2, (8, 64, 1024, 1)) == -1 and create(offs, lens, 2, None) == -1
    assert create(np.array([0, 1032], U), lens, 2, (8, 64, 1024, 0)) == -1  # a start not 16-byte aligned
    assert create(None, lens, 2, (8, 64, 1024, 0)) == -1
    assert create(np.array([0], U), np.array([64 * ((1 << 32) - 1)], U), 1, (8, 64, 1024, 0)) == -1  # the 2^32 bound
    c = sd.Cdc(ctx, offs, lens, (8, 64, 1024))
    out = np.zeros(8, U)
    assert lib().sd_cdc_layout(c.handle, out.ctypes.data) == -1 and lib().sd_cdc_stats(c.handle, out.ctypes.data) == -1
    assert lib().sd_cdc_hash(ctx.handle, c.handle, d.data_ptr(), None, None, None) == -1  # before any cut
    assert lib().sd_cdc_cut(ctx.handle, c.handle, d.data_ptr() + 8, None, None) == -1  # the buffer not 16-byte aligned
    assert lib().sd_cdc_cut(ctx.handle, c.handle, None, None, None) == -1
    m = c.cut(d)
    assert m == 2 + 1 and c.stats().tolist()[:2] == [2, 3000]  # zeros: cut at max_size only
    d_ids = torch.zeros(32 * m + 16, dtype=torch.uint8, device="cuda")
    assert lib().sd_cdc_hash(ctx.handle, c.handle, d.data_ptr(), None, d_ids.data_ptr() + 8, None) == -1
    c.close()
    e = sd.Cdc(ctx, offs[:0], lens[:0], None)  # no file
    assert e.cut(d) == 0 and e.layout().tolist() == [0] and not e.stats().any()
    e.hash(d, None, None)
    e.close()


def test_compare_files_on_the_device(ctx, tmp_path, cases):
    case = next(c for c in cases if c[0] == "shift")
    want = case[5]
    paths = []
    for i, f in enumerate(cc.shift_files()):
        p = tmp_path / f"f{i}"
        p.write_bytes(f.tobytes())
        paths.append(p)
    base, chunks, ids, stats = cdc.chunk_files(paths, case[4], device=True)
    assert np.array_equal(base, want["base"]) and np.array_equal(chunks, want["chunks"]) and np.array_equal(ids, want["ids"])
    files, pairs, sstats = cdc.compare_files(paths, case[4])
    model = cc.shared_model(want["base"], want["chunks"], want["ids"])
    assert np.array_equal(files, model["files"]) and np.array_equal(pairs, model["pairs"]) and np.array_equal(sstats, model["stats"])
