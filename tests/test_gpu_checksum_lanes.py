"""Every lane count of a tree node and every proof shape on the device: k_ck_blocks
(sd_checksum_tree_blocks_run / _verify), k_ck_leaf_tree (sd_checksum_tree_run), k_tree_levels and
k_tree_proof_gather (_prove) and proof_climb (_verify_proofs) on the cases of
tests/checksum_lane_cases.py -- every node, root and proof byte against the oracle and the numpy
levels, every output between guard rows over 0xA5.  tests/test_checksum_lanes.py holds the CPU twins
to the same cases."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import checksum_lane_cases as lc  # noqa: E402
from tests import checksum_proofs_cases as pc  # noqa: E402
from tests.test_gpu_checksum_blocks import POISON, Guarded, ctx, dev, open_list, run_guarded  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def prove_guarded(t, d_level) -> np.ndarray:
    """sd_checksum_tree_blocks_prove between guard rows -> the packed proofs [entries, 32]"""
    total = int(t.proof_base[t.m])
    out = Guarded(total, 32)
    t.prove(d_level, out.inner)
    proofs = out.host().copy()
    assert out.guards_intact()
    return proofs


def verify_proofs_guarded(t, d_data, d_proofs, d_roots):
    """(rows uint64, stats, flags, nodes) of sd_checksum_tree_blocks_verify_proofs, every output guarded"""
    bad, rows, nodes = Guarded(t.m, 1), Guarded(t.m, 16, torch.int64), Guarded(t.m, 32)
    got, stats, _ = t.verify_proofs(d_data, d_proofs, d_roots, d_nodes_out=nodes.inner, d_bad=bad.inner, d_rows_out=rows.inner)
    got = got.cpu().numpy().astype(np.uint64)
    assert bad.guards_intact() and rows.guards_intact() and nodes.guards_intact()
    assert (rows.host()[len(got):] == POISON).all()
    return got, stats, bad.host().reshape(-1).copy(), nodes.host().copy()


def wrong_rows(bl: lc.LaneList, got, want) -> list:
    """(k, lanes, chunks in the last lane, role) of the first rows that differ"""
    wrong = np.nonzero((got != want).any(axis=1))[0]
    return [(bl.k, lc.lanes_of(bl.sizes[r]), lc.last_fill(bl.sizes[r]), "root" if bl.is_root[r] else "cv") for r in wrong[:8]]


@pytest.mark.parametrize("k", lc.KS)
def test_lane_list_run(ctx, k):
    """every item as a root and as a plain CV at counter B / 1024, shuffled so that roles and lane
    counts share workgroups: all 2 x items nodes bit for bit; then again on the same context"""
    bl = lc.lane_list(k)
    want = lc.lane_expected(k)
    d_data = dev(bl.data)
    nodes = run_guarded(ctx, bl, d_data)
    assert np.array_equal(nodes, want), wrong_rows(bl, nodes, want)
    again = run_guarded(ctx, bl, d_data)
    assert np.array_equal(again, want), wrong_rows(bl, again, want)


@pytest.mark.parametrize("k", lc.KS)
def test_lane_list_verify(ctx, k):
    """_verify against the reference level (random bytes in the slots never listed) flags nothing;
    with the last byte of a 1-lane, a 2^(k-13) + 1-lane and a 2^(k-12) - 1-lane item flipped it flags
    exactly the rows that hold them, both roles"""
    bl = lc.lane_list(k)
    d_level = dev(lc.lane_level(k).copy()).reshape(-1)
    t = open_list(ctx, bl)
    bad, rows = Guarded(bl.m, 1), Guarded(bl.m, 16, torch.int64)
    got, stats, _ = t.verify(dev(bl.data), d_level, d_bad=bad.inner, d_rows_out=rows.inner)
    assert len(got) == 0 and list(stats) == [bl.n, bl.m, 0, 0], wrong_rows(bl, bad.host(), np.zeros((bl.m, 1), np.uint8))
    assert not bad.host().any() and (rows.host() == POISON).all() and bad.guards_intact() and rows.guards_intact()
    d, want_bad, want_rows, want_stats = lc.lane_flips(k)
    bad, rows = Guarded(bl.m, 1), Guarded(6, 16, torch.int64)
    got, stats, _ = t.verify(dev(d), d_level, d_bad=bad.inner, d_rows_out=rows.inner)
    assert np.array_equal(bad.host().reshape(-1), want_bad)
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want_rows) and np.array_equal(stats, want_stats)
    assert bad.guards_intact() and rows.guards_intact()
    t.close()


@pytest.mark.parametrize("k", lc.KS)
def test_whole_files(ctx, k):
    """the files len, B + len and q B + len laid out contiguously through sd_checksum_tree_run: every
    node against the oracle's BLAKE3 (one-node files) or its CV of block j at counter j B / 1024,
    every root against the oracle; then again on the same handle"""
    b = lc.tree_batch(k)
    want = lc.tree_expected(k)
    t = ctx.checksum_tree(b.offsets, b.lens, k)
    assert t.total_nodes == b.total and np.array_equal(t.node_base, b.node_base)
    d_data = dev(b.data)
    for _ in range(2):
        nodes, roots = Guarded(b.total, 32), Guarded(b.n, 32)
        t.run(d_data, nodes.inner, roots.inner)
        got, got_roots = nodes.host().copy(), roots.host().copy()
        assert nodes.guards_intact() and roots.guards_intact()
        for i in range(b.n):
            length = int(b.lens[i])
            assert np.array_equal(b.level(got, i), b.level(want, i)), (k, i, length, lc.lanes_of(length % (1 << k)))
        assert np.array_equal(got_roots, b.checksums)
    t.close()


def test_proofs_from_levels(ctx):
    """about 9 600 shuffled rows of files of 1 .. 131 073 nodes of random levels: the packed proofs
    byte for byte against the numpy levels, proof_base against the closed form; a second _prove on the
    same handle, with garbage in the unlisted file's level, gives the same"""
    lens, rows, level, want, pbase, _ = lc.proof_case()
    t = ctx.checksum_tree_blocks(lens, rows, np.zeros(len(rows), np.uint64), lc.PROOF_K)
    assert np.array_equal(t.proof_base, pbase)
    for d_level in (dev(level.copy()).reshape(-1), dev(lc.proof_garbage_level()).reshape(-1)):
        proofs = prove_guarded(t, d_level)
        wrong = np.nonzero((proofs != want).any(axis=1))[0]
        at = np.unique(np.searchsorted(pbase, wrong, side="right") - 1)[:8]
        assert len(wrong) == 0, [(int(lens[int(rows[r, 0])]) >> lc.PROOF_K, int(rows[r, 1])) for r in at]
    t.close()


def test_climb_real_bytes(ctx):
    """files of 1 .. 24, 31, 32 and 33 nodes, every block listed, shuffled: the device proofs from the
    oracle's level are the numpy proofs; _verify_proofs passes every row and d_nodes_out is the
    level's rows; one bit flipped in one entry of eleven rows (every depth 0 .. 5 of the 33-node file,
    its carried block 32, row 0 of the files of 2, 3, 5 and 17 nodes) flags those rows alone"""
    b, bl = lc.climb_batch(), lc.climb_list()
    level, want, pbase = lc.climb_reference()
    t = open_list(ctx, bl)
    assert np.array_equal(t.proof_base, pbase)
    proofs = prove_guarded(t, dev(level.copy()).reshape(-1))
    assert np.array_equal(proofs, want)
    d_data, d_roots = dev(bl.data), dev(b.checksums).reshape(-1)
    rows, stats, bad, nodes = verify_proofs_guarded(t, d_data, dev(proofs).reshape(-1), d_roots)
    assert not bad.any(), [(lc.CLIMB_NBS[int(f)], int(j)) for f, j in bl.rows[bad != 0][:8]]  # (nb, j)
    assert len(rows) == 0 and list(stats) == [bl.n, bl.m, 0, 0]
    assert np.array_equal(nodes, level[bl.slots()])
    flipped, hit = lc.climb_flips()
    want_bad, want_rows, want_stats = pc.expected_flags(bl, hit)
    rows, stats, bad, _ = verify_proofs_guarded(t, d_data, dev(flipped).reshape(-1), d_roots)
    assert np.array_equal(bad, want_bad), (np.nonzero(bad)[0].tolist(), hit)
    assert np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats)
    t.close()
