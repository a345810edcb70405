"""Listed blocks on the device (include/sd_cas.h, checksum trees, listed blocks):
sd_checksum_tree_blocks_run / _verify / _update through k_ck_blocks on the cases of
tests/checksum_blocks_cases.py -- the nodes against the pure-Python spec (directly, or by the root
identity against the oracle), against sd_checksum_tree_run's level and the CPU twin, every output
between guard rows over garbage.  tests/test_checksum_blocks.py holds the CPU twins to the same
cases."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from spacedrive_amd import cpu  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from tests import checksum_blocks_cases as bc  # noqa: E402
from tests import checksum_tree_cases as tc  # noqa: E402
from tests import high_counter_cases as hc  # noqa: E402

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


def open_list(ctx, bl: bc.BlockList):
    t = ctx.checksum_tree_blocks(bl.lens, bl.rows, bl.offsets, bl.k)
    assert (t.n, t.m, t.total_nodes) == (bl.n, bl.m, bl.total) and t.bytes_hashed == sum(bl.sizes)
    return t


def run_guarded(ctx, bl: bc.BlockList, d_data=None) -> np.ndarray:
    """sd_checksum_tree_blocks_run between guard rows -> the nodes [m, 32] on the host"""
    t = open_list(ctx, bl)
    out = Guarded(bl.m, 32)
    t.run(dev(bl.data) if d_data is None else d_data, out.inner)
    nodes = out.host().copy()
    assert out.guards_intact()
    t.close()
    return nodes


def tree_level(ctx, b: tc.Batch, data=None) -> tuple:
    """sd_checksum_tree_run of the files laid out contiguously -> (level, roots)"""
    t = ctx.checksum_tree(b.offsets, b.lens, b.k)
    nodes = torch.zeros(b.total * 32, dtype=torch.uint8, device="cuda")
    roots = torch.zeros(b.n * 32, dtype=torch.uint8, device="cuda")
    t.run(dev(b.data if data is None else data), nodes, roots)
    torch.cuda.synchronize()
    t.close()
    return nodes.cpu().numpy().reshape(-1, 32), roots.cpu().numpy().reshape(-1, 32)


@pytest.mark.parametrize("k", bc.KS)
def test_run_shape_list(ctx, k):
    """every block of the shape files, shuffled, scattered over 0xA5 junk, one start 16 bytes past a
    line: the direct rows against the spec, every file's root identity, sd_checksum_tree_run's level
    and the CPU twin on the same bytes; then the same list again on the same context"""
    bl, b = bc.shape_list(k), bc.shape_batch(k)
    d_data = dev(bl.data)
    nodes = run_guarded(ctx, bl, d_data)
    bc.check_list(bl, nodes, b, bc.direct_nodes(k), "run")
    assert np.array_equal(bc.level_of(bl, nodes), tree_level(ctx, b)[0])
    assert np.array_equal(nodes, cpu.checksum_tree_blocks(bl.data, bl.lens, bl.rows, bl.offsets, k, 8))
    assert np.array_equal(run_guarded(ctx, bl, d_data), nodes)


@pytest.mark.parametrize("k", bc.KS)
def test_run_high_counters(ctx, k):
    """blocks at chunk counters around 2^32 of files of 4 TiB, only they resident: a counter cut to
    32 bits gives another value (asserted where the expectation is built)"""
    bl = bc.high_list(k)
    assert np.array_equal(run_guarded(ctx, bl), bc.high_expected(k))


@pytest.mark.parametrize("k", bc.KS)
def test_run_packing_prefixes(ctx, k):
    """the first m of 33 small rows, m = 1 .. 33: at 16, 8, 4 and 2 items per workgroup the last
    workgroup is one short, full, and one over; m = 0 does nothing"""
    bl, want = bc.packing_list(k)
    d_data = dev(bl.data)
    for m in range(1, 34):
        assert np.array_equal(run_guarded(ctx, bl.prefix(m), d_data), want[:m]), (k, m)
    e = open_list(ctx, bl.prefix(0))
    out, lvl, roots = Guarded(1, 32), Guarded(bl.total, 32), Guarded(bl.n, 32)
    e.run(d_data, out.inner)
    rows, stats = e.verify(d_data, lvl.inner)
    e.update(d_data, lvl.inner, roots.inner)
    L, s = lib(), torch.cuda.current_stream().cuda_stream
    assert L.sd_checksum_tree_blocks_run(ctx.handle, e.handle, None, None, s) == 0
    assert len(rows) == 0 and not stats.any()
    for g in (out, lvl, roots):
        assert (g.host() == POISON).all() and g.guards_intact()
    e.close()


def test_windowed_and_unwindowed_instantiations(ctx):
    """g_windows picks k_ck_blocks<true> for a launch of more waves than 4 x CUs.  At k = 17 a
    workgroup of 8 waves holds 16 items, 2 per wave, so a list of more than 8 x CUs rows is
    windowed; the shape lists (16 rows) and the packing lists (33) are not."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = 17
    b = bc.windowed_batch(8 * cus)
    bl = bc.BlockList(b.lens, k, bc.every_row(b, 31), bc.blocks_of(b), seed=32, odd=7)
    assert bl.m > 8 * cus and bl.wave_count() > 4 * cus, (bl.m, cus)               # windowed
    for kk in bc.KS:
        assert bc.shape_list(kk).wave_count() <= 4 * cus and bc.packing_list(kk)[0].wave_count() <= 4 * cus
    nodes = run_guarded(ctx, bl)
    assert np.array_equal(nodes, cpu.checksum_tree_blocks(bl.data, bl.lens, bl.rows, bl.offsets, k, 16))
    bc.check_list(bl, nodes, b, None, "windowed")
    # verify and update take the same instantiation
    level = bc.level_of(bl, nodes)
    t = open_list(ctx, bl)
    d = bl.data.copy()
    hit = [5, bl.m // 2, bl.m - 1]
    for r in hit:
        d[int(bl.offsets[r])] ^= 0xFF
    rows, stats = t.verify(dev(d), dev(level).reshape(-1))
    assert np.array_equal(rows.cpu().numpy().astype(np.uint64), bl.rows[hit])
    assert list(stats) == [bl.n, bl.m, 3, len({int(bl.rows[r, 0]) for r in hit})]
    lv, roots = Guarded(bl.total, 32), Guarded(bl.n, 32)
    lv.inner.copy_(torch.full((bl.total * 32,), 0x11, dtype=torch.uint8, device="cuda"))
    t.update(dev(bl.data), lv.inner, roots.inner)
    assert np.array_equal(lv.host(), level) and np.array_equal(roots.host(), b.checksums)
    assert lv.guards_intact() and roots.guards_intact()
    t.close()


@pytest.mark.parametrize("k", bc.KS)
def test_verify(ctx, k):
    """the flips: rows in list order, flags, stats; a repeated row reported twice; a flip in a block
    that a second list omits not reported; a capacity one short; d_bad and the rows NULL in turn"""
    bl, b = bc.shape_list(k), bc.shape_batch(k)
    B = 1 << k
    level = tree_level(ctx, b)[0]
    d_exp = dev(level).reshape(-1)
    listed, unlisted = bc.flip_cases(k)
    t = open_list(ctx, bl)
    bad, rows = Guarded(bl.m, 1), Guarded(bl.m, 16, torch.int64)
    got, stats, _ = t.verify(dev(bl.data), d_exp, d_bad=bad.inner, d_rows_out=rows.inner)
    assert len(got) == 0 and list(stats) == [bl.n, bl.m, 0, 0]
    assert not bad.host().any() and (rows.host() == POISON).all() and bad.guards_intact() and rows.guards_intact()
    t.close()
    again = (listed[0][0], listed[0][1] // B)
    rep = bc.BlockList(bl.lens, k, [tuple(r) for r in bl.rows.tolist()] + [again], bc.blocks_of(b), seed=5, odd=2)
    d_flip = dev(bc.flipped_list(rep, listed + [unlisted]))
    want_bad, want_rows, want_stats = bc.expected_verify(rep, listed + [unlisted])
    assert int(want_stats[2]) == 5 and int(want_stats[3]) == 3 and tuple(want_rows[-1]) == again
    t = open_list(ctx, rep)
    bad, rows = Guarded(rep.m, 1), Guarded(5, 16, torch.int64)
    got, stats, _ = t.verify(d_flip, d_exp, d_bad=bad.inner, d_rows_out=rows.inner)
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want_rows) and np.array_equal(stats, want_stats)
    assert np.array_equal(bad.host().reshape(-1), want_bad) and bad.guards_intact() and rows.guards_intact()
    got, stats = t.verify(d_flip, d_exp)  # the wrapper's own rows buffer, flags NULL
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want_rows) and np.array_equal(stats, want_stats)
    bad = Guarded(rep.m, 1)
    got, stats, _ = t.verify(d_flip, d_exp, d_bad=bad.inner, want_rows=False)  # counting only
    assert len(got) == 0 and np.array_equal(stats, want_stats) and np.array_equal(bad.host().reshape(-1), want_bad)
    t.close()
    # the list without the last flip's block
    drop = [r for r, (f, j) in enumerate(rep.rows) if (int(f), int(j)) == (unlisted[0], unlisted[1] // B)]
    part = rep.without(drop)
    want_bad, want_rows, want_stats = bc.expected_verify(part, listed)
    assert len(drop) == 1 and int(want_stats[2]) == 4 and int(want_stats[3]) == 2
    t = open_list(ctx, part)
    bad, rows = Guarded(part.m, 1), Guarded(4, 16, torch.int64)
    got, stats, _ = t.verify(d_flip, d_exp, d_bad=bad.inner, d_rows_out=rows.inner)
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want_rows) and np.array_equal(stats, want_stats)
    assert np.array_equal(bad.host().reshape(-1), want_bad) and bad.guards_intact() and rows.guards_intact()
    # a capacity one short: the requirement, flags and stats complete, no row written
    bad, rows = Guarded(part.m, 1), Guarded(4, 16, torch.int64)
    with pytest.raises(SdCasError) as e:
        t.verify(d_flip, d_exp, d_bad=bad.inner, d_rows_out=rows.inner, capacity=3)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == 4 and np.array_equal(e.value.stats, want_stats)
    assert np.array_equal(bad.host().reshape(-1), want_bad) and (rows.host() == POISON).all()
    assert bad.guards_intact() and rows.guards_intact()
    t.close()


@pytest.mark.parametrize("k", bc.KS)
def test_update(ctx, k):
    """three changed blocks, one of them a one-node file's, patched into the level _run gave for the
    original bytes: the listed nodes are the changed data's, every other node is bit-identical, the
    roots are the oracle's BLAKE3 of the changed files and the old checksums of the others"""
    b, nb = bc.shape_batch(k), bc.changed_batch(k)
    full = bc.shape_list(k)
    old = bc.level_of(full, run_guarded(ctx, full))
    changes, rows = bc.update_case(k)
    bl = bc.BlockList(nb.lens, k, rows, bc.blocks_of(nb), seed=9, odd=1)
    t = open_list(ctx, bl)
    lv, roots = Guarded(b.total, 32), Guarded(b.n, 32)
    lv.inner.copy_(dev(old).reshape(-1))
    for _ in range(2):  # the second call reads the first's scratch and patched level
        t.update(dev(bl.data), lv.inner, roots.inner)
    level, got_roots = lv.host().copy(), roots.host().copy()
    assert lv.guards_intact() and roots.guards_intact()
    slots = bl.slots()
    rest = np.setdiff1d(np.arange(b.total), slots)
    assert np.array_equal(level[rest], old[rest]) and not any(np.array_equal(level[s], old[s]) for s in slots)
    twin_level, twin_roots = cpu.checksum_tree_blocks_update(bl.data, bl.lens, bl.rows, bl.offsets, old, k)
    assert np.array_equal(level, twin_level) and np.array_equal(got_roots, twin_roots)
    B = 1 << k
    for f, j in rows:  # the spec of the changed bytes where it is cheap
        size = bc.block_len(int(nb.lens[f]), j, k)
        if size <= 4097:
            data = nb.file(f)[j * B:j * B + size]
            want = tc.spec_nodes(data, k)[0].tobytes() if int(nb.nb[f]) == 1 else hc.spec_block_cv(data, j * B // 1024)
            assert level[int(nb.node_base[f]) + j].tobytes() == want, (k, f, j)
    touched = {f for f, _ in rows}
    for i in range(b.n):
        assert tc.spec_root(nb.level(level, i)) == nb.checksums[i].tobytes(), (k, i)
        assert got_roots[i].tobytes() == nb.checksums[i].tobytes(), (k, i)
        assert (got_roots[i].tobytes() == b.checksums[i].tobytes()) == (i not in touched), (k, i)
    t.close()
    # a repeated row: refused before any launch, the level as it was
    rep = bc.BlockList(nb.lens, k, rows + rows[:1], bc.blocks_of(nb), seed=9)
    t = open_list(ctx, rep)
    lv, roots = Guarded(b.total, 32), Guarded(b.n, 32)
    lv.inner.copy_(dev(old).reshape(-1))
    with pytest.raises(SdCasError) as e:
        t.update(dev(rep.data), lv.inner, roots.inner)
    assert e.value.rc == SD_ERR_INVALID
    assert np.array_equal(lv.host(), old) and (roots.host() == POISON).all() and lv.guards_intact()
    out = Guarded(rep.m, 32)
    t.run(dev(rep.data), out.inner)  # _run takes the same list
    assert np.array_equal(out.host()[-1], out.host()[0]) and out.guards_intact()
    t.close()


def test_invalid_arguments(ctx):
    """refused with SD_ERR_INVALID before anything is launched: the outputs stay garbage"""
    L = lib()
    B = 1 << 17
    lens = np.array([100, B + 1], np.uint64)
    rows, offs = np.array([[0, 0], [1, 1]], np.uint64), np.array([0, 1024], np.uint64)
    h = ctypes.c_void_p()
    p = lambda a: None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)  # noqa: E731

    def create(c=ctx.handle, ls=lens, k=17, rw=rows, of=offs, m=2, out=ctypes.byref(h)):
        return L.sd_checksum_tree_blocks_create(c, p(ls), 2, k, p(rw), p(of), m, out)

    assert create(rw=np.array([[2, 0], [1, 1]], np.uint64)) == SD_ERR_INVALID and not h.value   # file >= n_files
    assert create(rw=np.array([[0, 1], [1, 1]], np.uint64)) == SD_ERR_INVALID                   # block >= nb
    assert create(rw=np.array([[0, 0], [1, 2]], np.uint64)) == SD_ERR_INVALID
    assert create(of=np.array([0, 1032], np.uint64)) == SD_ERR_INVALID                          # not 16-byte aligned
    for k in (0, 16, 21, 1 << 20):
        assert create(k=k) == SD_ERR_INVALID and not h.value
    for kw in ({"c": None}, {"ls": None}, {"rw": None}, {"of": None}, {"out": None}):
        assert create(**kw) == SD_ERR_INVALID
    t = ctx.checksum_tree_blocks(lens, rows, offs, 17)
    data = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out, lvl, roots, bad = Guarded(2, 32), Guarded(3, 32), Guarded(2, 32), Guarded(2, 1)
    vrows = Guarded(2, 16, torch.int64)
    cnt, stats = ctypes.c_uint64(7), np.full(4, 7, np.uint64)
    s = torch.cuda.current_stream().cuda_stream
    run = lambda c, bl, d, o: L.sd_checksum_tree_blocks_run(c, bl, p(d), p(o), s)  # noqa: E731
    for args in ((None, t.handle, data, out.inner), (ctx.handle, None, data, out.inner), (ctx.handle, t.handle, None, out.inner),
                 (ctx.handle, t.handle, data, None), (ctx.handle, t.handle, data, out.inner[8:])):
        assert run(*args) == SD_ERR_INVALID
    ver = lambda c, bl, d, e: L.sd_checksum_tree_blocks_verify(c, bl, p(d), p(e), p(bad.inner), p(vrows.inner), 2,  # noqa: E731
                                                               ctypes.byref(cnt), p(stats), s)
    for args in ((None, t.handle, data, lvl.inner), (ctx.handle, None, data, lvl.inner), (ctx.handle, t.handle, None, lvl.inner),
                 (ctx.handle, t.handle, data, None), (ctx.handle, t.handle, data, lvl.inner[8:])):
        assert ver(*args) == SD_ERR_INVALID
    upd = lambda c, bl, d, nd, r: L.sd_checksum_tree_blocks_update(c, bl, p(d), p(nd), p(r), s)  # noqa: E731
    for args in ((None, t.handle, data, lvl.inner, roots.inner), (ctx.handle, None, data, lvl.inner, roots.inner),
                 (ctx.handle, t.handle, None, lvl.inner, roots.inner), (ctx.handle, t.handle, data, None, roots.inner),
                 (ctx.handle, t.handle, data, lvl.inner, None), (ctx.handle, t.handle, data, lvl.inner[8:], roots.inner)):
        assert upd(*args) == SD_ERR_INVALID
    assert L.sd_checksum_tree_blocks_stats(None, p(stats)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_blocks_stats(t.handle, None) == SD_ERR_INVALID
    for g in (out, lvl, roots, bad, vrows):
        assert (g.host() == POISON).all() and g.guards_intact()
    # and the same handle works once the arguments are right
    assert run(ctx.handle, t.handle, data, out.inner) == 0
    want = cpu.checksum_tree_blocks(np.zeros(4096, np.uint8), lens, rows, offs, 17, 1)
    assert np.array_equal(out.host(), want) and out.guards_intact()
    t.close()
