"""Block proofs on the device (include/sd_cas.h, checksum trees, block proofs):
sd_checksum_tree_blocks_prove (k_tree_levels, k_tree_proof_gather) and _verify_proofs (k_ck_blocks,
then the climb) on the cases of tests/checksum_proofs_cases.py.  A device proof is held to the
pure-Python climb reaching a root that came from elsewhere; every output sits between guard rows
over 0xA5.  tests/test_checksum_proofs.py holds the CPU twins to the same cases."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from spacedrive_amd import cpu  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from tests import checksum_blocks_cases as bc  # noqa: E402
from tests import checksum_proofs_cases as pc  # noqa: E402
from tests.test_gpu_checksum_blocks import POISON, Guarded, ctx, dev, open_list, run_guarded  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SD_ERR_INVALID = -1
_levels = {}


def real_level(k: int):
    """(level, roots) of the real files from the existing CPU tree, the roots held to the oracle"""
    if k not in _levels:
        b = pc.real_batch(k)
        nodes, roots, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
        assert np.array_equal(roots, b.checksums)
        _levels[k] = (nodes, roots)
    return _levels[k]


def prove_guarded(t, d_level) -> np.ndarray:
    """sd_checksum_tree_blocks_prove between guard rows -> the packed proofs [entries, 32]"""
    total = int(t.proof_base[t.m])
    out = Guarded(max(total, 1), 32)
    t.prove(d_level, out.inner)
    proofs = out.host()[:total].copy()
    assert out.guards_intact() and (total > 0 or (out.host() == POISON).all())
    return proofs


def verify_guarded(t, d_data, d_proofs, d_roots, **kw):
    """(rows uint64, stats, flags, nodes) of sd_checksum_tree_blocks_verify_proofs, every output guarded"""
    bad, rows, nodes = Guarded(t.m, 1), Guarded(t.m, 16, torch.int64), Guarded(t.m, 32)
    got, stats, _ = t.verify_proofs(d_data, d_proofs, d_roots, d_nodes_out=nodes.inner, d_bad=bad.inner,
                                    d_rows_out=rows.inner, **kw)
    got = got.cpu().numpy().astype(np.uint64)
    assert bad.guards_intact() and rows.guards_intact() and nodes.guards_intact()
    assert (rows.host()[len(got):] == POISON).all()
    return got, stats, bad.host().reshape(-1).copy(), nodes.host().copy()


@pytest.mark.parametrize("k", pc.KS)
def test_real_files_prove_and_verify(ctx, k):
    """nb = 1, 2, 3, 5, 8, 9 in one list, shuffled, with repeats, so the lanes of one wave climb 0 to
    4 levels: every device proof climbs, in pure Python, to the oracle's BLAKE3 of the file and
    equals the CPU twin's; verify_proofs passes every row against those checksums; d_nodes_out is
    _run's output; a second prove reads the first's scratch"""
    bl, b = pc.real_list(k), pc.real_batch(k)
    level, _ = real_level(k)
    t = open_list(ctx, bl)
    assert np.array_equal(t.proof_base, pc.proof_base(bl.lens, bl.rows, k))
    for r, (f, j) in enumerate(bl.rows):
        assert int(t.proof_base[r + 1] - t.proof_base[r]) == cpu.tree_proof_entries(int(bl.lens[int(f)]), int(j), k)
    d_level = dev(level).reshape(-1)
    proofs = prove_guarded(t, d_level)
    pc.check_proofs(bl.lens, bl.rows, k, level, proofs, [c.tobytes() for c in b.checksums], "device prove")
    assert np.array_equal(proofs, cpu.checksum_tree_blocks_prove(level, bl.lens, bl.rows, k)[0])
    assert np.array_equal(prove_guarded(t, d_level), proofs)
    d_data = dev(bl.data)
    rows, stats, bad, nodes = verify_guarded(t, d_data, dev(proofs).reshape(-1), dev(b.checksums).reshape(-1))
    assert len(rows) == 0 and not bad.any() and list(stats) == [bl.n, bl.m, 0, 0]
    assert np.array_equal(nodes, run_guarded(ctx, bl, d_data)) and np.array_equal(nodes, level[bl.slots()])
    got, stats = t.verify_proofs(d_data, dev(proofs).reshape(-1), dev(b.checksums).reshape(-1))  # every output NULL
    assert len(got) == 0 and list(stats) == [bl.n, bl.m, 0, 0]
    t.close()


def test_levels_alone(ctx):
    """random levels of 255, 256, 257 and 65 537 nodes (a short group, a full one, full + 1, two
    passes of stored levels): the proofs climb to tc.spec_root of the level and equal the CPU twin's;
    an unlisted file's level filled with garbage changes no proof"""
    lens, rows, level, roots = pc.level_case()
    t = ctx.checksum_tree_blocks(lens, rows, np.zeros(len(rows), np.uint64), pc.LEVEL_K)
    proofs = prove_guarded(t, dev(level).reshape(-1))
    pc.check_proofs(lens, rows, pc.LEVEL_K, level, proofs, roots, "device levels")
    assert np.array_equal(proofs, cpu.checksum_tree_blocks_prove(level, lens, rows, pc.LEVEL_K)[0])
    assert np.array_equal(prove_guarded(t, dev(pc.garbage_level()).reshape(-1)), proofs)
    t.close()


def test_deep_tree_and_high_counter(ctx):
    """k = 20, nb = 2^22 + 3 (three passes of stored levels, 23 levels): only the listed blocks'
    bytes exist, their level slots hold the existing CPU twin's nodes and every other slot is random;
    the root is the existing sd_cpu_checksum_tree_roots'.  Block 2^22 + 1 hashes chunk counters past
    2^32.  The device proofs pass the Python climb to that root, verify_proofs passes them, and one
    flipped byte of the high-counter block flags that row alone."""
    bl = pc.deep_list()
    k = pc.DEEP_K
    level = np.random.default_rng(77).integers(0, 256, (bl.total, 32), dtype=np.uint8)
    level[bl.slots()] = cpu.checksum_tree_blocks(bl.data, bl.lens, bl.rows, bl.offsets, k, 8)
    roots = cpu.checksum_tree_roots(level, bl.lens, k)
    t = open_list(ctx, bl)
    assert int(t.proof_base[bl.m]) == sum(pc.entries(pc.DEEP_NB, j) for j in pc.DEEP_BLOCKS)
    proofs = prove_guarded(t, dev(level).reshape(-1))
    pc.check_proofs(bl.lens, bl.rows, k, level, proofs, [r.tobytes() for r in roots], "deep")
    d_proofs, d_roots = dev(proofs).reshape(-1), dev(roots).reshape(-1)
    rows, stats, bad, nodes = verify_guarded(t, dev(bl.data), d_proofs, d_roots)
    assert len(rows) == 0 and not bad.any() and list(stats) == [bl.n, bl.m, 0, 0]
    assert np.array_equal(nodes, level[bl.slots()])
    r = pc.row_of(bl, 0, (1 << 22) + 1)
    d = bl.data.copy()
    d[int(bl.offsets[r]) + 500000] ^= 0x04
    rows, stats, bad, _ = verify_guarded(t, dev(d), d_proofs, d_roots)
    want_bad, want_rows, want_stats = pc.expected_flags(bl, [r])
    assert np.array_equal(bad, want_bad) and np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats)
    t.close()


def test_rejections_capacity_and_count_only(ctx):
    """each change flags exactly the rows concerned and leaves the others clean; then the capacity
    rule and the count-only mode on the case with the most rows"""
    k = 17
    bl, b = pc.real_list(k), pc.real_batch(k)
    t = open_list(ctx, bl)
    proofs = prove_guarded(t, dev(real_level(k)[0]).reshape(-1))
    cases = pc.rejections(bl, proofs, b.checksums)
    for name, data, pf, roots, want in cases:
        want_bad, want_rows, want_stats = pc.expected_flags(bl, want)
        rows, stats, bad, _ = verify_guarded(t, dev(data), dev(pf).reshape(-1), dev(roots).reshape(-1))
        assert np.array_equal(bad, want_bad), name
        assert np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats), name
    name, data, pf, roots, want = cases[2]
    assert name == "root" and len(want) >= 5
    want_bad, want_rows, want_stats = pc.expected_flags(bl, want)
    d_data, d_pf, d_roots = dev(data), dev(pf).reshape(-1), dev(roots).reshape(-1)
    bad, rows = Guarded(bl.m, 1), Guarded(len(want), 16, torch.int64)
    with pytest.raises(SdCasError) as e:
        t.verify_proofs(d_data, d_pf, d_roots, d_bad=bad.inner, d_rows_out=rows.inner, capacity=len(want) - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == len(want) and np.array_equal(e.value.stats, want_stats)
    assert np.array_equal(bad.host().reshape(-1), want_bad) and (rows.host() == POISON).all()
    got, stats, _ = t.verify_proofs(d_data, d_pf, d_roots, d_bad=bad.inner, d_rows_out=rows.inner)  # exactly enough
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want_rows) and rows.guards_intact()
    bad = Guarded(bl.m, 1)
    got, stats, _ = t.verify_proofs(d_data, d_pf, d_roots, d_bad=bad.inner, want_rows=False)
    assert len(got) == 0 and np.array_equal(stats, want_stats) and np.array_equal(bad.host().reshape(-1), want_bad)
    assert bad.guards_intact()
    t.close()


def test_empty_list_and_small_after_large(ctx):
    """m == 0 does nothing; a two-row list after the large ones of this context, whose pooled slot
    still holds their nodes and flags, flags its one bad row"""
    k = 17
    bl, b = pc.real_list(k), pc.real_batch(k)
    level, _ = real_level(k)
    e = open_list(ctx, bl.prefix(0))
    out, nodes, bad = Guarded(1, 32), Guarded(1, 32), Guarded(1, 1)
    assert list(e.proof_base) == [0]
    e.prove(dev(level).reshape(-1), out.inner)
    rows, stats, _ = e.verify_proofs(dev(bl.data), out.inner, dev(b.checksums).reshape(-1), d_nodes_out=nodes.inner,
                                     d_bad=bad.inner)
    L, s = lib(), torch.cuda.current_stream().cuda_stream
    assert L.sd_checksum_tree_blocks_prove(ctx.handle, e.handle, None, None, s) == 0
    assert L.sd_checksum_tree_blocks_verify_proofs(ctx.handle, e.handle, None, None, None, None, None, None, 0, None, None,
                                                   s) == 0
    assert len(rows) == 0 and not stats.any()
    for g in (out, nodes, bad):
        assert (g.host() == POISON).all() and g.guards_intact()
    e.close()
    big = open_list(ctx, bl)
    proofs = prove_guarded(big, dev(level).reshape(-1))
    d_roots = dev(b.checksums).reshape(-1)
    rows, _, _, _ = verify_guarded(big, dev(bl.data), dev(proofs).reshape(-1), d_roots)
    assert len(rows) == 0
    big.close()
    keep = [pc.row_of(bl, 6, 1), pc.row_of(bl, 4, 2)]
    small = bl.without([r for r in range(bl.m) if r not in keep])
    t = open_list(ctx, small)
    pf = prove_guarded(t, dev(level).reshape(-1))
    d = small.data.copy()
    d[int(small.offsets[1]) + 3] ^= 0x20
    rows, stats, bad, _ = verify_guarded(t, dev(d), dev(pf).reshape(-1), d_roots)
    assert list(bad) == [0, 1] and np.array_equal(rows, small.rows[1:]) and list(stats) == [small.n, 2, 1, 1]
    t.close()


def test_invalid_arguments(ctx):
    """refused with SD_ERR_INVALID before anything is launched: the outputs stay garbage"""
    L = lib()
    k = 17
    bl, b = pc.real_list(k), pc.real_batch(k)
    t = open_list(ctx, bl)
    total = int(t.proof_base[bl.m])
    p = lambda a: None if a is None else a.data_ptr()  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    d_level, d_data, d_roots = dev(real_level(k)[0]).reshape(-1), dev(bl.data), dev(b.checksums).reshape(-1)
    proofs, nodes, bad, rows = Guarded(total, 32), Guarded(bl.m, 32), Guarded(bl.m, 1), Guarded(bl.m, 16, torch.int64)
    cnt, stats = ctypes.c_uint64(7), np.full(4, 7, np.uint64)
    base = np.zeros(bl.m + 1, np.uint64)
    assert L.sd_checksum_tree_blocks_proof_layout(None, base.ctypes.data) == SD_ERR_INVALID
    assert L.sd_checksum_tree_blocks_proof_layout(t.handle, None) == SD_ERR_INVALID
    prove = lambda c, h, nd, o: L.sd_checksum_tree_blocks_prove(c, h, p(nd), p(o), s)  # noqa: E731
    for args in ((None, t.handle, d_level, proofs.inner), (ctx.handle, None, d_level, proofs.inner),
                 (ctx.handle, t.handle, None, proofs.inner), (ctx.handle, t.handle, d_level, None),
                 (ctx.handle, t.handle, d_level[8:], proofs.inner), (ctx.handle, t.handle, d_level, proofs.inner[8:])):
        assert prove(*args) == SD_ERR_INVALID
    ver = lambda c, h, d, pf, rt, nd: L.sd_checksum_tree_blocks_verify_proofs(  # noqa: E731
        c, h, p(d), p(pf), p(rt), p(nd), p(bad.inner), p(rows.inner), bl.m, ctypes.byref(cnt), stats.ctypes.data, s)
    ok = (ctx.handle, t.handle, d_data, proofs.inner, d_roots, nodes.inner)
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (3, proofs.inner[8:]), (4, d_roots[8:]),
                 (5, nodes.inner[8:])):
        args = list(ok)
        args[i] = v
        assert ver(*args) == SD_ERR_INVALID, i
    for g in (proofs, nodes, bad, rows):
        assert (g.host() == POISON).all() and g.guards_intact()
    # and the same handle works once the arguments are right
    assert prove(ctx.handle, t.handle, d_level, proofs.inner) == 0
    assert ver(*ok) == 0 and cnt.value == 0 and list(stats) == [bl.n, bl.m, 0, 0]
    assert not bad.host().any() and proofs.guards_intact()
    t.close()
