"""Checksum trees on the device (include/sd_cas.h, checksum trees): sd_checksum_tree_run / _roots /
_verify through k_ck_leaf_tree and the verify's sliced passes, on the cases of
tests/checksum_tree_cases.py -- the levels against the restated definitions (node by node, or by
the root identity and the position rule), the roots against the oracle and sd_checksum_batch_run,
every output between guard rows over garbage, and each call a second time on the same context
after a larger batch.  tests/test_checksum_tree.py holds the CPU twins to the same cases."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from spacedrive_amd import cpu  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from tests import checksum_tree_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

G = 4  # guard rows either side of an output
POISON = 0xA5
SD_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


class Guarded:
    """`rows` rows of `row_bytes` device bytes between G guard rows, all 0xA5 (the garbage the
    outputs are pre-filled with); the calls get `inner`"""

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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_guarded(ctx, b: tc.Batch, d_data=None):
    """sd_checksum_tree_run between guard rows -> (nodes, roots) on the host"""
    t = ctx.checksum_tree(b.offsets, b.lens, b.k)
    assert np.array_equal(t.node_base, b.node_base) and t.total_nodes == b.total and t.n == b.n
    nodes, roots = Guarded(b.total, 32), Guarded(b.n, 32)
    t.run(dev(b.data) if d_data is None else d_data, nodes.inner, roots.inner)
    out = nodes.host().copy(), roots.host().copy()
    assert nodes.guards_intact() and roots.guards_intact()
    t.close()
    return out


@pytest.fixture(scope="module")
def device_levels(ctx):
    """{k: (nodes, roots)} of the shape batches, computed once by _run and shared"""
    return {k: run_guarded(ctx, tc.shape_batch(k)) for k in tc.KS}


@pytest.mark.parametrize("k", tc.KS)
def test_run_levels_and_roots(ctx, device_levels, k):
    """every shape in one batch (workgroups shared by two files, a half-empty last workgroup, a
    start 16 bytes past a line): levels, roots, the position rule; then the same call again on the
    same context after a larger batch, over fresh garbage"""
    b, t = tc.shape_batch(k), tc.truncated_batch(k)
    nodes, roots = device_levels[k]
    tc.check_levels(b, nodes, roots, tc.direct_levels(k), "run")
    d_data = dev(b.data)
    cb = ctx.checksum_batch(b.offsets, b.lens)
    plain = Guarded(b.n, 32)
    cb.run(d_data, plain.inner)
    assert np.array_equal(plain.host(), roots) and plain.guards_intact()  # what sd_checksum_batch_run writes
    # a larger batch in between (the truncated twins beside the full files), then the first again
    both = tc.Batch([int(x) for x in b.lens] + [int(x) for x in t.lens], k, seed=5000)
    big_nodes, big_roots = run_guarded(ctx, both)
    tc.check_levels(both, big_nodes, big_roots, None, "run, larger batch")
    t_nodes, t_roots = run_guarded(ctx, t)
    tc.check_levels(t, t_nodes, t_roots, None, "run, truncated")
    tc.check_position_rule(b, nodes, t, t_nodes, "run")
    again = run_guarded(ctx, b, d_data)
    assert np.array_equal(again[0], nodes) and np.array_equal(again[1], roots)


@pytest.mark.parametrize("k", tc.KS)
def test_roots_from_levels(ctx, device_levels, k):
    """the roots from device levels and from levels the CPU twin computed: both the oracle's; a
    level that was tampered with changes exactly its file's root"""
    b = tc.shape_batch(k)
    t = ctx.checksum_tree(b.offsets, b.lens, k)
    twin_nodes, _, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
    assert np.array_equal(twin_nodes, device_levels[k][0])  # the two routes agree node by node
    bad = twin_nodes.copy()
    victim = int(np.argmax(b.nb))
    bad[int(b.node_base[victim]) + 1, 31] ^= 0x80
    for level, wrong in ((device_levels[k][0], []), (twin_nodes, []), (bad, [victim])):
        lv, roots = Guarded(b.total, 32), Guarded(b.n, 32)
        lv.inner.copy_(dev(level).reshape(-1))
        for _ in range(2):  # the second run reads the stale scratch of the first
            t.roots(lv.inner, roots.inner)
        got = roots.host()
        assert [i for i in range(b.n) if not np.array_equal(got[i], b.checksums[i])] == wrong
        assert roots.guards_intact() and np.array_equal(lv.host(), level)
    t.close()


@pytest.mark.parametrize("k", tc.KS)
def test_verify(ctx, device_levels, k):
    """the flips all in one call, against the device's level and the CPU twin's; a clean batch; a
    capacity one short; d_bad and the rows each NULL in turn; all between guard rows over garbage"""
    b = tc.shape_batch(k)
    _, want_rows, want_stats = tc.flips(b)
    want_bad = np.zeros(b.total, np.uint8)
    want_bad[[int(b.node_base[f]) + int(j) for f, j in want_rows]] = 1
    need = len(want_rows)
    t = ctx.checksum_tree(b.offsets, b.lens, k)
    d_clean, d_flip = dev(b.data), dev(tc.flipped(b))
    twin_nodes, _, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
    for level in (device_levels[k][0], twin_nodes):
        d_exp = dev(level).reshape(-1)
        # clean
        bad, rows = Guarded(b.total, 1), Guarded(b.total, 16, torch.int64)
        got_rows, stats, _ = t.verify(d_clean, d_exp, d_bad=bad.inner, d_rows_out=rows.inner)
        assert len(got_rows) == 0 and list(stats) == [b.n, b.total, 0, 0]
        assert not bad.host().any() and (rows.host() == POISON).all() and bad.guards_intact() and rows.guards_intact()
        # the flips; rows sized exactly
        bad, rows = Guarded(b.total, 1), Guarded(need, 16, torch.int64)
        got_rows, stats, _ = t.verify(d_flip, d_exp, d_bad=bad.inner, d_rows_out=rows.inner)
        assert np.array_equal(got_rows.cpu().numpy().astype(np.uint64), want_rows) and np.array_equal(stats, want_stats)
        assert np.array_equal(bad.host().reshape(-1), want_bad) and bad.guards_intact() and rows.guards_intact()
        # the wrapper's own rows buffer, and flags NULL
        got_rows, stats = t.verify(d_flip, d_exp)
        assert np.array_equal(got_rows.cpu().numpy().astype(np.uint64), want_rows) and np.array_equal(stats, want_stats)
        # rows NULL: counting only, the flags complete
        bad = Guarded(b.total, 1)
        got_rows, stats, _ = t.verify(d_flip, d_exp, d_bad=bad.inner, want_rows=False)
        assert len(got_rows) == 0 and np.array_equal(stats, want_stats)
        assert np.array_equal(bad.host().reshape(-1), want_bad) and bad.guards_intact()
        # both NULL
        got_rows, stats = t.verify(d_flip, d_exp, want_rows=False)
        assert np.array_equal(stats, want_stats)
        # a capacity one short: the requirement, flags and stats complete, no row written
        bad, rows = Guarded(b.total, 1), Guarded(need, 16, torch.int64)
        with pytest.raises(SdCasError) as e:
            t.verify(d_flip, d_exp, d_bad=bad.inner, d_rows_out=rows.inner, capacity=need - 1)
        assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == need and np.array_equal(e.value.stats, want_stats)
        assert np.array_equal(bad.host().reshape(-1), want_bad) and (rows.host() == POISON).all()
        assert bad.guards_intact() and rows.guards_intact()
    t.close()


def test_windowed_and_unwindowed_instantiations(ctx, device_levels):
    """g_windows picks k_ck_leaf_tree<true> for a launch of more waves than 4 x CUs.  A leaf
    workgroup is 8 waves over two 1 MiB leaf blocks, and a file of at most 1 MiB is one leaf block
    whatever its length, so CUs + 64 small files make 4 x (CUs + 64) waves: the windowed
    instantiation.  The shape batches (21 to 55 leaf blocks, at most 224 waves) took the
    unwindowed one; they are bit-exact in test_run_levels_and_roots."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = 17
    B = 1 << k
    n = cus + 64
    pattern = [1, 1024, 4097, 20000, B + 1, 2 * B + 5, 3 * B - 1, B]
    lens = [pattern[i % len(pattern)] + (i // len(pattern)) for i in range(n)] + [2 * tc.MIB + 1]
    b = tc.Batch(lens, k, seed=9000, odd_start=5)
    waves = 8 * ((b.leaf_blocks() + 1) // 2)
    assert waves > 4 * cus, (waves, cus)                                    # windowed
    assert 8 * ((tc.shape_batch(k).leaf_blocks() + 1) // 2) <= 4 * cus      # unwindowed
    nodes, roots = run_guarded(ctx, b)
    tc.check_levels(b, nodes, roots, None, "windowed")
    twin_nodes, twin_roots, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 16)
    assert np.array_equal(nodes, twin_nodes) and np.array_equal(roots, twin_roots)
    # verify takes the same instantiation
    t = ctx.checksum_tree(b.offsets, b.lens, k)
    d = b.data.copy()
    hit = [(7, 0), (n, 16), (n - 3, 0)]
    for f, j in hit:
        d[int(b.offsets[f]) + j * B] ^= 0xFF
    rows, stats = t.verify(dev(d), dev(nodes).reshape(-1))
    assert [tuple(r) for r in rows.cpu().tolist()] == sorted(hit) and list(stats) == [b.n, b.total, 3, 3]
    t.close()


def test_invalid_arguments(ctx):
    """refused with SD_ERR_INVALID before anything is launched: the outputs stay garbage"""
    L = lib()
    offs, lens = np.array([0, 1024], np.uint64), np.array([100, 200], np.uint64)
    h = ctypes.c_void_p()
    p = lambda a: None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)  # noqa: E731
    for k in (0, 16, 21, 1 << 20):
        assert L.sd_checksum_tree_create(ctx.handle, p(offs), p(lens), 2, k, ctypes.byref(h)) == SD_ERR_INVALID and not h.value
    assert L.sd_checksum_tree_create(ctx.handle, p(np.array([0, 1032], np.uint64)), p(lens), 2, 17, ctypes.byref(h)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_create(None, p(offs), p(lens), 2, 17, ctypes.byref(h)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_create(ctx.handle, None, p(lens), 2, 17, ctypes.byref(h)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_create(ctx.handle, p(offs), None, 2, 17, ctypes.byref(h)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_create(ctx.handle, p(offs), p(lens), 2, 17, None) == SD_ERR_INVALID
    t = ctx.checksum_tree(offs, lens, 17)
    data = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    nodes, roots, bad = Guarded(2, 32), Guarded(2, 32), Guarded(2, 1)
    rows = Guarded(2, 16, torch.int64)
    cnt, stats, base = ctypes.c_uint64(7), np.full(4, 7, np.uint64), np.zeros(3, np.uint64)
    s = torch.cuda.current_stream().cuda_stream
    run = lambda c, tr, d, nd, r: L.sd_checksum_tree_run(c, tr, p(d), p(nd), p(r), s)  # noqa: E731
    for args in ((None, t.handle, data, nodes.inner, roots.inner), (ctx.handle, None, data, nodes.inner, roots.inner),
                 (ctx.handle, t.handle, None, nodes.inner, roots.inner), (ctx.handle, t.handle, data, None, roots.inner),
                 (ctx.handle, t.handle, data, nodes.inner, None), (ctx.handle, t.handle, data, nodes.inner[8:], roots.inner)):
        assert run(*args) == SD_ERR_INVALID
    rts = lambda c, tr, nd, r: L.sd_checksum_tree_roots(c, tr, p(nd), p(r), s)  # noqa: E731
    for args in ((None, t.handle, nodes.inner, roots.inner), (ctx.handle, None, nodes.inner, roots.inner),
                 (ctx.handle, t.handle, None, roots.inner), (ctx.handle, t.handle, nodes.inner, None),
                 (ctx.handle, t.handle, nodes.inner[8:], roots.inner)):
        assert rts(*args) == SD_ERR_INVALID
    ver = lambda c, tr, d, e: L.sd_checksum_tree_verify(c, tr, p(d), p(e), p(bad.inner), p(rows.inner), 2,  # noqa: E731
                                                        ctypes.byref(cnt), p(stats), s)
    for args in ((None, t.handle, data, nodes.inner), (ctx.handle, None, data, nodes.inner),
                 (ctx.handle, t.handle, None, nodes.inner), (ctx.handle, t.handle, data, None),
                 (ctx.handle, t.handle, data, nodes.inner[8:])):
        assert ver(*args) == SD_ERR_INVALID
    assert L.sd_checksum_tree_layout(None, p(base)) == SD_ERR_INVALID and L.sd_checksum_tree_layout(t.handle, None) == SD_ERR_INVALID
    assert L.sd_checksum_tree_stats(None, p(stats)) == SD_ERR_INVALID and L.sd_checksum_tree_stats(t.handle, None) == SD_ERR_INVALID
    for g in (nodes, roots, bad, rows):
        assert (g.host() == POISON).all() and g.guards_intact()
    # and the same handles work once the arguments are right
    assert run(ctx.handle, t.handle, data, nodes.inner, roots.inner) == 0
    want = cpu.checksum_tree(np.zeros(4096, np.uint8), offs, lens, 17, 1)
    assert np.array_equal(nodes.host(), want[0]) and np.array_equal(roots.host(), want[1])
    t.close()
    # an empty batch is valid and launches nothing
    e = ctx.checksum_tree(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 17)
    assert e.n == 0 and e.total_nodes == 0 and list(e.node_base) == [0]
    rows_e, stats_e = e.verify(data, data)
    assert len(rows_e) == 0 and not stats_e.any()
    e.close()
