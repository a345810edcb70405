"""Range proofs on the host (include/sd_cas.h, checksum trees, range proofs): the GPU-free
sd_checksum_tree_range_proof_entries and the twins sd_cpu_checksum_tree_blocks_prove_ranges /
_verify_range_proofs -- which plan the ranges, and climb them group by group, as the device does --
on the cases of tests/checksum_ranges_cases.py.  tests/test_gpu_checksum_ranges.py holds the kernels
to the same cases."""
import numpy as np
import pytest

from spacedrive_amd import cpu, tree
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError
from tests import checksum_lane_cases as lc
from tests import checksum_proofs_cases as pc
from tests import checksum_ranges_cases as rc

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


def verify(rl, data, proofs, roots, **kw):
    return cpu.checksum_tree_blocks_verify_range_proofs(data, rl.lens, rl.rows, rl.offsets, rl.range_base, proofs, roots,
                                                        rl.k, want_flags=True, want_nodes=True, nthreads=8, **kw)


def test_every_range_of_small_levels():
    """random-node levels, every (a, b) of every nb <= 33: the twin's proof equals the spec's and
    climbs, by the spec, to the level-wise root; the entry count is the closed form and <= 2h; the
    two spec climbs agree"""
    rl, level, roots = rc.small_case()
    for (f, a, b), want in zip(rl.ranges, np.diff(rl.proof_base)):
        got = cpu.tree_range_proof_entries(int(rl.lens[f]), a, b - a, rl.k)
        assert got == int(want) <= 2 * rc.height(rl.nb[f]), (f, a, b)
    proofs, base = cpu.checksum_tree_blocks_prove_ranges(level, rl.lens, rl.rows, rl.range_base, rl.k)
    assert np.array_equal(base, rl.proof_base)
    assert np.array_equal(proofs, rc.spec_proofs(rl, level, pc.spec_levels))
    rc.check_range_proofs(rl, level, proofs, roots, what="twin prove")
    for i in range(0, rl.q, 37):
        f, a, b = rl.ranges[i]
        o, pf = int(rl.node_base[f]), proofs[int(base[i]):int(base[i + 1])].tobytes()
        assert rc.np_range_climb(level[o + a:o + b], pf, rl.nb[f], a, b) == roots[f]


def test_one_block_is_the_block_proof_and_whole_files_are_empty():
    rl, level, _ = rc.small_case()
    ones = [i for i, (f, a, b) in enumerate(rl.ranges) if b == a + 1]
    sub = rc.RangeList(rl.lens, rl.k, [rl.ranges[i] for i in ones])
    assert sub.m == sub.q == sum(rc.SMALL_NBS)
    got, base = cpu.checksum_tree_blocks_prove_ranges(level, sub.lens, sub.rows, sub.range_base, sub.k)
    want, want_base = cpu.checksum_tree_blocks_prove(level, sub.lens, sub.rows, sub.k)
    assert np.array_equal(base, want_base) and got.tobytes() == want.tobytes()
    whole = rc.RangeList(rl.lens, rl.k, [(f, 0, nb) for f, nb in enumerate(rl.nb)])
    got, base = cpu.checksum_tree_blocks_prove_ranges(level, whole.lens, whole.rows, whole.range_base, whole.k)
    assert len(got) == 0 and not base.any() and rl.nb[0] == 1


def test_boundary_ranges_of_large_levels():
    """255 .. 513 and 65 537 / 131 073 nodes: ranges across the groups of 256 (the device's plan, run
    on the host), against the numpy spec"""
    for nbs, seed in ((rc.GROUP_NBS, 61), (rc.DEEP_NBS, 62)):
        rl, level, roots = rc.boundary_case(nbs, seed)
        proofs, base = cpu.checksum_tree_blocks_prove_ranges(level, rl.lens, rl.rows, rl.range_base, rl.k)
        assert np.array_equal(base, rl.proof_base)
        assert np.array_equal(proofs, rc.spec_proofs(rl, level, lc.np_levels))
        rc.check_range_proofs(rl, level, proofs, roots, rc.np_range_climb, "large")


@pytest.mark.parametrize("k", rc.KS)
def test_real_files_and_mutations(k):
    """every range of every real file in one list over the files' own bytes: nothing flagged against
    the oracle's checksums, the nodes are the level's; each mutation flags exactly its ranges"""
    rl, b = rc.real_ranges(k), pc.real_batch(k)
    level, _ = real_level(k)
    proofs, _ = cpu.checksum_tree_blocks_prove_ranges(level, rl.lens, rl.rows, rl.range_base, k)
    rc.check_range_proofs(rl, level, proofs, [c.tobytes() for c in b.checksums], what="real")
    rows, stats, bad, nodes = verify(rl, b.data, proofs, b.checksums)
    assert len(rows) == 0 and not bad.any() and list(stats) == [rl.n, rl.q, 0, 0]
    assert np.array_equal(nodes, level[rl.slots()])
    for name, data, pf, want in rc.mutations(rl, b.data, proofs, level):
        want_bad, want_rows, want_stats = rl.expected(want)
        rows, stats, bad, _ = verify(rl, data, pf, b.checksums)
        assert np.array_equal(bad, want_bad), (name, np.flatnonzero(bad != want_bad))
        assert np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats), name


def test_capacity_and_count_only():
    k = 17
    rl, b = rc.real_ranges(k), pc.real_batch(k)
    level, _ = real_level(k)
    proofs, _ = cpu.checksum_tree_blocks_prove_ranges(level, rl.lens, rl.rows, rl.range_base, k)
    name, data, pf, want = rc.mutations(rl, b.data, proofs, level)[0]
    want_bad, want_rows, want_stats = rl.expected(want)
    assert len(want) >= 5
    with pytest.raises(SdCasError) as e:
        verify(rl, data, pf, b.checksums, capacity=len(want) - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == len(want) and np.array_equal(e.value.stats, want_stats)
    rows, stats, bad, _ = verify(rl, data, pf, b.checksums, capacity=len(want))
    assert np.array_equal(rows, want_rows)
    rows, stats, bad, _ = verify(rl, data, pf, b.checksums, want_rows=False)
    assert len(rows) == 0 and np.array_equal(stats, want_stats) and np.array_equal(bad, want_bad)


def test_capacity_writes_no_row():
    from spacedrive_amd._native import lib
    import ctypes
    k = 17
    rl, b = rc.real_ranges(k), pc.real_batch(k)
    level, _ = real_level(k)
    proofs, _ = cpu.checksum_tree_blocks_prove_ranges(level, rl.lens, rl.rows, rl.range_base, k)
    name, data, pf, want = rc.mutations(rl, b.data, proofs, level)[0]
    out = np.full((len(want), 3), 0xA5A5A5A5, np.uint64)
    cnt = ctypes.c_uint64(0)
    roots = np.ascontiguousarray(b.checksums)
    rcode = lib().sd_cpu_checksum_tree_blocks_verify_range_proofs(
        data.ctypes.data, rl.lens.ctypes.data, rl.n, k, rl.rows.ctypes.data, rl.offsets.ctypes.data, rl.m,
        rl.range_base.ctypes.data, rl.q, pf.ctypes.data, roots.ctypes.data, None, None, out.ctypes.data, len(want) - 1,
        ctypes.byref(cnt), None, 4)
    assert rcode == SD_ERR_CAPACITY and cnt.value == len(want) and (out == 0xA5A5A5A5).all()


def test_refusals():
    """a gap, non-consecutive blocks, two files in one range, an empty range, base[q] != m, and the
    entry count's own refusals"""
    k = 17
    B = 1 << k
    lens = [8 * B, 5 * B]
    level = np.random.default_rng(7).integers(0, 256, (13, 32), dtype=np.uint8)
    rows = np.array([(0, 2), (0, 3), (0, 4), (1, 0), (1, 1)], np.uint64)
    good = [0, 3, 5]
    cpu.checksum_tree_blocks_prove_ranges(level, lens, rows, good, k)

    def refused(rows, base):
        with pytest.raises(SdCasError) as e:
            cpu.checksum_tree_blocks_prove_ranges(level, lens, rows, base, k)
        assert e.value.rc == SD_ERR_INVALID

    refused(rows, [1, 3, 5])                                               # a gap at the front
    refused(rows, [0, 3, 4])                                               # base[q] != m
    refused(rows, [0, 3, 3, 5])                                            # an empty range
    refused(rows, [0, 5, 3])                                               # descending
    refused(rows, [0, 4, 5])                                               # two files in one range
    refused(np.array([(0, 2), (0, 4), (0, 5), (1, 0), (1, 1)], np.uint64), good)   # non-consecutive blocks
    refused(np.array([(0, 3), (0, 2), (0, 1), (1, 0), (1, 1)], np.uint64), good)   # descending blocks
    refused(np.array([(0, 6), (0, 7), (0, 8), (1, 0), (1, 1)], np.uint64), good)   # past the file's end
    refused(rows, [0])                                                    # q == 0 with rows
    proofs, base = cpu.checksum_tree_blocks_prove_ranges(level, lens, np.zeros((0, 2), np.uint64), [0], k)  # q == 0, m == 0
    assert len(proofs) == 0 and list(base) == [0]
    for args in ((8 * B, 0, 0), (8 * B, 8, 1), (8 * B, 7, 2), (0, 1, 1)):
        with pytest.raises(SdCasError) as e:
            cpu.tree_range_proof_entries(args[0], args[1], args[2], k)
        assert e.value.rc == SD_ERR_INVALID
    for bad_k in (16, 21):
        with pytest.raises(SdCasError):
            cpu.tree_range_proof_entries(8 * B, 0, 1, bad_k)
    assert cpu.tree_range_proof_entries(0, 0, 1, k) == 0
    # the second half of a 100 GiB file at 128 KiB blocks: a = 25 << 14 is odd at levels 14, 17 and 18,
    # and a range that ends with the file has no right flank: 3 entries for 409 600 blocks
    assert cpu.tree_range_proof_entries(100 << 30, 409600, 409600, 17) == 3 == rc.range_entries(819200, 409600, 819200)


def test_prove_range_and_verify_range_file(tmp_path):
    k = 17
    b = pc.real_batch(k)
    level, roots = real_level(k)
    f = 7  # nb = 9, a 1-byte trailing block
    path = tmp_path / "file"
    path.write_bytes(b.file(f))
    length, nodes, checksum = int(b.lens[f]), b.level(level, f), roots[f].tobytes()
    for first, count in ((2, 5), (0, 9), (8, 1), (3, 1)):
        proof = tree.prove_range(nodes, length, first, count, k)
        assert len(proof) == 32 * rc.range_entries(9, first, first + count)
        assert tree.verify_range_file(path, length, checksum.hex(), first, count, proof, k)
        assert tree.verify_range_file(path, length, checksum, first, count, proof, k)
    assert tree.prove_range(nodes, length, 3, 1, k) == tree.prove_blocks(nodes, length, [3], k)
    proof = tree.prove_range(nodes, length, 2, 5, k)
    other = tree.prove_range(nodes, length, 1, 5, k)
    assert len(other) == len(proof) and not tree.verify_range_file(path, length, checksum, 2, 5, other, k)
    data = bytearray(b.file(f))
    data[4 * (1 << k) + 5] ^= 1
    path.write_bytes(bytes(data))
    assert not tree.verify_range_file(path, length, checksum, 2, 5, proof, k)
    assert tree.verify_range_file(path, length, checksum, 5, 4, tree.prove_range(nodes, length, 5, 4, k), k)
    with pytest.raises(ValueError):
        tree.prove_range(nodes, length, 5, 5, k)
