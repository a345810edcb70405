"""Range proofs on the device (include/sd_cas.h, checksum trees, range proofs):
sd_checksum_tree_blocks_prove_ranges (k_tree_levels, k_tree_range_gather) and _verify_range_proofs
(k_ck_blocks, k_tree_range_climb, then range_differs) on the cases of tests/checksum_ranges_cases.py.
A device proof is held bit for bit to the spec's and to the spec's climb reaching a root that came
from elsewhere; every output sits between guard rows over 0xA5.  tests/test_checksum_ranges.py holds
the CPU twins to the same cases."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from spacedrive_amd import cpu  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from tests import checksum_lane_cases as lc  # noqa: E402
from tests import checksum_proofs_cases as pc  # noqa: E402
from tests import checksum_ranges_cases as rc  # noqa: E402
from tests.test_gpu_checksum_blocks import POISON, Guarded, ctx, dev  # noqa: E402,F401

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


def open_ranges(ctx, rl: rc.RangeList):
    t = ctx.checksum_tree_blocks(rl.lens, rl.rows, rl.offsets, rl.k)
    t.set_ranges(rl.range_base)
    assert (t.n, t.m, t.q) == (rl.n, rl.m, rl.q) and np.array_equal(t.range_proof_base, rl.proof_base)
    return t


def prove_guarded(t, d_level) -> np.ndarray:
    """sd_checksum_tree_blocks_prove_ranges between guard rows -> the packed proofs [entries, 32]"""
    total = int(t.range_proof_base[t.q])
    out = Guarded(max(total, 1), 32)
    t.prove_ranges(d_level, out.inner)
    proofs = out.host()[:total].copy()
    assert out.guards_intact() and (total > 0 or (out.host() == POISON).all())
    return proofs


def verify_guarded(t, d_data, d_proofs, d_roots, **kw):
    """(ranges uint64 [count, 3], stats, flags, nodes) of _verify_range_proofs, every output guarded"""
    bad, rows, nodes = Guarded(t.q, 1), Guarded(t.q, 24, torch.int64), Guarded(t.m, 32)
    got, stats, _ = t.verify_range_proofs(d_data, d_proofs, d_roots, d_nodes_out=nodes.inner, d_bad=bad.inner,
                                          d_ranges_out=rows.inner, **kw)
    got = got.cpu().numpy().astype(np.uint64)
    assert bad.guards_intact() and rows.guards_intact() and nodes.guards_intact()
    assert (rows.host()[len(got):] == POISON).all()
    return got, stats, bad.host().reshape(-1).copy(), nodes.host().copy()


def test_prove_every_range_of_small_levels(ctx):
    """every (a, b) of every nb <= 33 in one list of random levels, no bytes: bit-equal to the spec,
    climbed by the spec to the level-wise root; a second prove reads the first's scratch"""
    rl, level, roots = rc.small_case()
    t = open_ranges(ctx, rl)
    d_level = dev(level).reshape(-1)
    proofs = prove_guarded(t, d_level)
    assert np.array_equal(proofs, rc.spec_proofs(rl, level, pc.spec_levels))
    rc.check_range_proofs(rl, level, proofs, roots, what="device prove")
    assert np.array_equal(prove_guarded(t, d_level), proofs)
    t.close()


@pytest.mark.parametrize("nbs,seed", [(rc.GROUP_NBS, 61), (rc.DEEP_NBS, 62)], ids=["groups", "three-passes"])
def test_prove_boundary_ranges(ctx, nbs, seed):
    """255 .. 513 nodes, then 65 537 and 131 073 (three passes of stored levels): [0, nb), [1, nb),
    [0, nb - 1), [1, nb - 1), [255, 257), [256, 512), [254, 256), [65 535, 65 537), the last block;
    an unlisted file of garbage sits between the listed ones"""
    rl, level, roots = rc.boundary_case(nbs, seed)
    t = open_ranges(ctx, rl)
    proofs = prove_guarded(t, dev(level).reshape(-1))
    assert np.array_equal(proofs, rc.spec_proofs(rl, level, lc.np_levels))
    rc.check_range_proofs(rl, level, proofs, roots, rc.np_range_climb, "device boundary")
    t.close()


@pytest.mark.parametrize("k", rc.KS)
def test_real_files_verify_and_mutations(ctx, k):
    """every range of every real file (nb = 1, 1, 1, 2, 3, 5, 8, 9) in one list over the files' own
    bytes: the device proofs equal the spec's, nothing is flagged against the oracle's checksums and no
    row is written, d_nodes_out is the level's nodes; each mutation flags exactly its ranges"""
    rl, b = rc.real_ranges(k), pc.real_batch(k)
    level, _ = real_level(k)
    t = open_ranges(ctx, rl)
    proofs = prove_guarded(t, dev(level).reshape(-1))
    assert np.array_equal(proofs, rc.spec_proofs(rl, level, pc.spec_levels))
    rc.check_range_proofs(rl, level, proofs, [c.tobytes() for c in b.checksums], what="device real")
    d_data, d_roots = dev(b.data), dev(b.checksums).reshape(-1)
    rows, stats, bad, nodes = verify_guarded(t, d_data, dev(proofs).reshape(-1), d_roots)
    assert len(rows) == 0 and not bad.any() and list(stats) == [rl.n, rl.q, 0, 0]
    assert np.array_equal(nodes, level[rl.slots()])
    got, stats = t.verify_range_proofs(d_data, dev(proofs).reshape(-1), d_roots)  # every output NULL
    assert len(got) == 0 and list(stats) == [rl.n, rl.q, 0, 0]
    cases = rc.mutations(rl, b.data, proofs, level)
    for name, data, pf, want in cases:
        want_bad, want_rows, want_stats = rl.expected(want)
        rows, stats, bad, _ = verify_guarded(t, dev(data), dev(pf).reshape(-1), d_roots)
        assert np.array_equal(bad, want_bad), (name, np.flatnonzero(bad != want_bad))
        assert np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats), name
        want_cpu = cpu.checksum_tree_blocks_verify_range_proofs(data, rl.lens, rl.rows, rl.offsets, rl.range_base, pf,
                                                                b.checksums, k, nthreads=8)
        assert np.array_equal(rows, want_cpu[0]) and np.array_equal(stats, want_cpu[1]), name
    # the capacity rule and the count-only mode on the case with the most ranges
    name, data, pf, want = cases[0]
    assert len(want) >= 5
    want_bad, want_rows, want_stats = rl.expected(want)
    d_data, d_pf = dev(data), dev(pf).reshape(-1)
    bad, rows = Guarded(rl.q, 1), Guarded(len(want), 24, torch.int64)
    with pytest.raises(SdCasError) as e:
        t.verify_range_proofs(d_data, d_pf, d_roots, d_bad=bad.inner, d_ranges_out=rows.inner, capacity=len(want) - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == len(want) and np.array_equal(e.value.stats, want_stats)
    assert np.array_equal(bad.host().reshape(-1), want_bad) and (rows.host() == POISON).all()
    got, stats, _ = t.verify_range_proofs(d_data, d_pf, d_roots, d_bad=bad.inner, d_ranges_out=rows.inner)  # exactly enough
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want_rows) and rows.guards_intact()
    got, stats, _ = t.verify_range_proofs(d_data, d_pf, d_roots, d_bad=bad.inner, want_rows=False)
    assert len(got) == 0 and np.array_equal(stats, want_stats) and bad.guards_intact()
    t.close()


def test_spliced_level_three_passes(ctx):
    """one k = 17 file of 66 537 blocks' worth of level, random nodes with real bytes spliced in: a
    520-block range [250, 770) (68 MB, groups 0 .. 3 of the first pass, three passes), the 2-block
    range [255, 257) across a group boundary, and the 1-byte last block.  All pass against the numpy
    root, d_nodes_out equals the oracle's nodes; one flipped byte in block 511 fails only the range
    that holds it"""
    rl, data, level, root = rc.splice_case()
    t = open_ranges(ctx, rl)
    proofs = prove_guarded(t, dev(level).reshape(-1))
    assert np.array_equal(proofs, rc.spec_proofs(rl, level, lc.np_levels))
    rc.check_range_proofs(rl, level, proofs, [root], rc.np_range_climb, "splice")
    d_proofs, d_roots = dev(proofs).reshape(-1), dev(np.frombuffer(root, np.uint8))
    rows, stats, bad, nodes = verify_guarded(t, dev(data), d_proofs, d_roots)
    assert len(rows) == 0 and not bad.any() and list(stats) == [1, 3, 0, 0]
    assert np.array_equal(nodes, level[rl.slots()])
    d = data.copy()
    d[(511 - 250) * (1 << rc.SPLICE_K) + 4242] ^= 0x02
    rows, stats, bad, _ = verify_guarded(t, dev(d), d_proofs, d_roots)
    want_bad, want_rows, want_stats = rl.expected([0])
    assert np.array_equal(bad, want_bad) and np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats)
    t.close()


def test_set_ranges_refusals_replacement_and_empty_list(ctx):
    """a range call before set_ranges is refused; a refused set_ranges leaves the ranges as they
    were; calling again replaces them; m == 0 does nothing"""
    L, s = lib(), torch.cuda.current_stream().cuda_stream
    k = 17
    rl, b = rc.real_ranges(k), pc.real_batch(k)
    level, _ = real_level(k)
    d_level, d_data, d_roots = dev(level).reshape(-1), dev(b.data), dev(b.checksums).reshape(-1)
    t = ctx.checksum_tree_blocks(rl.lens, rl.rows, rl.offsets, k)
    out, bad = Guarded(int(rl.proof_base[-1]), 32), Guarded(rl.q, 1)
    base = np.zeros(rl.q + 1, np.uint64)
    assert L.sd_checksum_tree_blocks_range_proof_layout(t.handle, base.ctypes.data) == SD_ERR_INVALID
    assert L.sd_checksum_tree_blocks_prove_ranges(ctx.handle, t.handle, d_level.data_ptr(), out.inner.data_ptr(), s) == SD_ERR_INVALID
    assert L.sd_checksum_tree_blocks_verify_range_proofs(ctx.handle, t.handle, d_data.data_ptr(), out.inner.data_ptr(),
                                                         d_roots.data_ptr(), None, bad.inner.data_ptr(), None, 0, None, None,
                                                         s) == SD_ERR_INVALID
    assert (out.host() == POISON).all() and (bad.host() == POISON).all()
    t.set_ranges(rl.range_base)
    proofs = prove_guarded(t, d_level)
    rb = rl.range_base
    i = rc.range_of(rl, 6, 2, 7)  # a range of five rows in the middle of the list
    r0 = int(rb[i])
    for wrong in (np.concatenate([[1], rb[1:]]),                    # a gap at the front
                  np.concatenate([rb[:-1], [rl.m - 1]]),            # base[q] != m
                  np.concatenate([rb[:i + 1], [r0], rb[i + 1:]]),   # an empty range
                  np.concatenate([rb[:i + 1], rb[i + 2:]]),         # two ranges merged: non-consecutive blocks
                  rb[:1]):                                          # q == 0 over a list with rows
        w = np.ascontiguousarray(wrong, np.uint64)
        assert L.sd_checksum_tree_blocks_set_ranges(t.handle, w.ctypes.data, len(w) - 1) == SD_ERR_INVALID
    assert L.sd_checksum_tree_blocks_set_ranges(None, rb.ctypes.data, rl.q) == SD_ERR_INVALID
    assert L.sd_checksum_tree_blocks_set_ranges(t.handle, None, rl.q) == SD_ERR_INVALID
    assert np.array_equal(prove_guarded(t, d_level), proofs)  # the list as it was
    rows, stats, _, _ = verify_guarded(t, d_data, dev(proofs).reshape(-1), d_roots)
    assert len(rows) == 0 and list(stats) == [rl.n, rl.q, 0, 0]
    # replaced: every row a range of its own -- the per-block proofs, byte for byte
    t.set_ranges(np.arange(rl.m + 1, dtype=np.uint64))
    ones = prove_guarded(t, d_level)
    assert ones.tobytes() == cpu.checksum_tree_blocks_prove(level, rl.lens, rl.rows, k)[0].tobytes()
    rows, stats, _, _ = verify_guarded(t, d_data, dev(ones).reshape(-1), d_roots)
    assert len(rows) == 0 and list(stats) == [rl.n, rl.m, 0, 0]
    t.close()
    e = ctx.checksum_tree_blocks(rl.lens, np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64), k)
    base = np.full(1, 7, np.uint64)
    assert L.sd_checksum_tree_blocks_range_proof_layout(e.handle, base.ctypes.data) == 0 and base[0] == 0
    e.set_ranges(np.zeros(1, np.uint64))
    assert L.sd_checksum_tree_blocks_prove_ranges(ctx.handle, e.handle, None, None, s) == 0
    assert L.sd_checksum_tree_blocks_verify_range_proofs(ctx.handle, e.handle, None, None, None, None, None, None, 0, None,
                                                         None, s) == 0
    e.close()
