"""Every lane count of a tree node and every proof shape on the host: sd_cpu_checksum_tree_blocks /
_verify, sd_cpu_checksum_tree, sd_cpu_checksum_tree_blocks_prove / _verify_proofs on the cases of
tests/checksum_lane_cases.py, every node, root and proof byte against the oracle and the numpy
levels.  tests/test_gpu_checksum_lanes.py holds the kernels to the same cases."""
import numpy as np
import pytest

from spacedrive_amd import cpu
from tests import checksum_lane_cases as lc
from tests import checksum_proofs_cases as pc


def test_module_invariants():
    """the sweep is what it claims: every lane count 1 .. 2^(k-12), all four fills of the last lane,
    every chunk count at k = 17, E(k) inside the sweep, the proof sweep's row and entry counts"""
    for k in lc.KS:
        items = lc.lane_items(k)
        assert sorted({lc.lanes_of(x) for x in items}) == list(range(1, (1 << (k - 12)) + 1))
        assert {lc.last_fill(x) for x in items} == {1, 2, 3, 4}
        assert set(lc.edge_lanes(k)) <= {lc.lanes_of(x) for x in items}
        # a last lane of 1, 2 and 3 chunks under a tree of more than two lanes
        assert {lc.last_fill(x) for x in items if lc.lanes_of(x) > 2} == {1, 2, 3, 4}
    assert [len(lc.lane_items(k)) for k in lc.KS] == [128, 64, 128, 256]
    assert sorted(-(-x // 1024) for x in lc.lane_items(17)) == list(range(1, 129))
    lens, rows, level, proofs, pbase, _ = lc.proof_case()
    assert (len(rows), len(proofs)) == (lc.PROOF_ROWS, lc.PROOF_ENTRIES) and len({tuple(r) for r in rows.tolist()}) == len(rows)
    assert lc.PROOF_GARBAGE not in set(rows[:, 0].tolist())


def test_anchor_subtree_cv_is_the_spec():
    """native.subtree_cv against hc.spec_block_cv at 3, 5, 9 and 13 chunks, counter B / 1024"""
    got = lc.anchor()
    assert [c for c, _, _ in got] == [3, 5, 9, 13]
    for c, fast, spec in got:
        assert fast == spec, c


def test_numpy_proofs_are_the_spec():
    """np_levels / np_proof against the pure-Python pc.spec_levels / pc.spec_proof on small levels"""
    rng = np.random.default_rng(3)
    for nb in (1, 2, 3, 5, 6, 7, 12, 17, 33):
        level = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
        lv, spec = lc.np_levels(level), pc.spec_levels(level)
        assert len(lv) == len(spec)
        for j in range(nb):
            assert lc.np_proof(lv, j).tobytes() == pc.spec_proof(spec, j), (nb, j)


@pytest.mark.parametrize("k", lc.KS)
def test_twin_lane_list(k):
    """every item as a root and as a plain CV at counter B / 1024, node by node; _verify against the
    reference level flags nothing, and with three items' last bytes flipped exactly their six rows"""
    bl = lc.lane_list(k)
    want = lc.lane_expected(k)
    for nthreads in (1, 8):
        got = cpu.checksum_tree_blocks(bl.data, bl.lens, bl.rows, bl.offsets, k, nthreads)
        wrong = np.nonzero((got != want).any(axis=1))[0]
        assert len(wrong) == 0, [(k, lc.lanes_of(bl.sizes[r]), "root" if bl.is_root[r] else "cv") for r in wrong[:8]]
    level = lc.lane_level(k)
    rows, stats, bad = cpu.checksum_tree_blocks_verify(bl.data, bl.lens, bl.rows, bl.offsets, level, k, want_flags=True)
    assert len(rows) == 0 and not bad.any() and list(stats) == [bl.n, bl.m, 0, 0]
    d, want_bad, want_rows, want_stats = lc.lane_flips(k)
    rows, stats, bad = cpu.checksum_tree_blocks_verify(d, bl.lens, bl.rows, bl.offsets, level, k, want_flags=True)
    assert np.array_equal(bad, want_bad) and np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats)


@pytest.mark.parametrize("k", lc.KS)
def test_twin_whole_files(k):
    """the files len, B + len and q B + len laid out contiguously: every node and every root"""
    b = lc.tree_batch(k)
    nodes, roots, base = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
    assert np.array_equal(base, b.node_base)
    want = lc.tree_expected(k)
    for i in range(b.n):
        assert np.array_equal(b.level(nodes, i), b.level(want, i)), (k, i, int(b.lens[i]), lc.lanes_of(int(b.lens[i]) % (1 << k)))
    assert np.array_equal(roots, b.checksums)


def test_twin_proofs_from_levels():
    """about 9 600 rows of files of 1 .. 131 073 nodes: the packed proofs byte for byte against the
    numpy levels, proof_base against the closed form; garbage in the unlisted file changes nothing"""
    lens, rows, level, want, pbase, _ = lc.proof_case()
    proofs, base = cpu.checksum_tree_blocks_prove(level, lens, rows, lc.PROOF_K)
    assert np.array_equal(base, pbase)
    wrong = np.nonzero((proofs != want).any(axis=1))[0]
    assert len(wrong) == 0, proof_rows(wrong, lens, rows, pbase)
    again, _ = cpu.checksum_tree_blocks_prove(lc.proof_garbage_level(), lens, rows, lc.PROOF_K)
    assert np.array_equal(again, want)


def proof_rows(wrong, lens, rows, pbase) -> list:
    """the first (nb, j) whose proofs hold the entries `wrong`"""
    at = np.unique(np.searchsorted(pbase, wrong, side="right") - 1)[:8]
    return [(int(lens[int(rows[r, 0])]) >> lc.PROOF_K, int(rows[r, 1])) for r in at]


def test_twin_climb_real_bytes():
    """files of 1 .. 24, 31, 32 and 33 nodes, every block listed: the proofs from the oracle's level
    are the numpy proofs; _verify_proofs passes every row and hands back the level's nodes; one bit
    flipped in one entry of eleven rows flags those rows alone"""
    b, bl = lc.climb_batch(), lc.climb_list()
    level, want, pbase = lc.climb_reference()
    proofs, base = cpu.checksum_tree_blocks_prove(level, bl.lens, bl.rows, lc.CLIMB_K)
    assert np.array_equal(base, pbase) and np.array_equal(proofs, want)
    rows, stats, bad, nodes = cpu.checksum_tree_blocks_verify_proofs(bl.data, bl.lens, bl.rows, bl.offsets, want, b.checksums,
                                                                     lc.CLIMB_K, want_flags=True, want_nodes=True)
    assert not bad.any(), [(lc.CLIMB_NBS[int(f)], int(j)) for f, j in bl.rows[bad != 0][:8]]  # (nb, j)
    assert len(rows) == 0 and list(stats) == [bl.n, bl.m, 0, 0]
    assert np.array_equal(nodes, level[bl.slots()])
    flipped, hit = lc.climb_flips()
    want_bad, want_rows, want_stats = pc.expected_flags(bl, hit)
    rows, stats, bad = cpu.checksum_tree_blocks_verify_proofs(bl.data, bl.lens, bl.rows, bl.offsets, flipped, b.checksums,
                                                              lc.CLIMB_K, want_flags=True)
    assert np.array_equal(bad, want_bad) and np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats)
