"""Block proofs on the host (include/sd_cas.h, checksum trees, block proofs):
sd_checksum_tree_proof_entries, sd_cpu_checksum_tree_blocks_prove / _verify_proofs and tree.py's
prove_blocks / verify_proofs_file on the cases of tests/checksum_proofs_cases.py.  A proof under test
is held to the pure-Python climb reaching a root that came from elsewhere (the oracle's BLAKE3 of
the bytes, or tc.spec_root of a random level).  tests/test_gpu_checksum_proofs.py holds the kernels
to the same cases."""
import ctypes

import numpy as np
import pytest

from spacedrive_amd import cpu, tree
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from tests import checksum_proofs_cases as pc
from tests import checksum_tree_cases as tc

SD_ERR_INVALID = -1


def test_spec_climb_reaches_the_level_wise_root():
    """the rule itself, in pure Python: every climb of (node, spec proof) reproduces tc.spec_root"""
    rng = np.random.default_rng(1)
    for nb in list(range(1, 20)) + [31, 32, 33]:
        level = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
        lv, root = pc.spec_levels(level), tc.spec_root(level)
        assert len(lv) == pc.height(nb) + 1
        for j in range(nb):
            proof = pc.spec_proof(lv, j)
            assert len(proof) == 32 * pc.entries(nb, j)
            assert pc.spec_climb(level[j].tobytes(), proof, nb, j) == root, (nb, j)


@pytest.mark.parametrize("nb,j,p", [(5, 4, 1), (3, 2, 1), (513, 512, 1), (513, 0, 10), (1, 0, 0), (2, 1, 1), (256, 255, 8)])
def test_proof_entries_closed_form(nb, j, p):
    assert pc.entries(nb, j) == p
    for k in (17, 20):
        assert cpu.tree_proof_entries((nb - 1 << k) + 1, j, k) == p


def test_proof_entries_every_block_of_small_files():
    for nb in list(range(1, 40)) + [255, 256, 257, 511, 513]:
        for j in (range(nb) if nb < 255 else (0, 1, nb // 2, nb - 2, nb - 1)):
            assert cpu.tree_proof_entries(nb << 17, j, 17) == pc.entries(nb, j), (nb, j)


def test_invalid_arguments():
    v = ctypes.c_uint32(7)
    L = lib()
    assert L.sd_checksum_tree_proof_entries(1 << 17, 17, 1, ctypes.byref(v)) == SD_ERR_INVALID  # one block: no block 1
    assert L.sd_checksum_tree_proof_entries(0, 17, 1, ctypes.byref(v)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_proof_entries(1 << 30, 16, 0, ctypes.byref(v)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_proof_entries(1 << 30, 21, 0, ctypes.byref(v)) == SD_ERR_INVALID
    assert L.sd_checksum_tree_proof_entries(1 << 30, 17, 0, None) == SD_ERR_INVALID
    assert v.value == 7
    bl = pc.real_list(17)
    level, roots, _ = real_level(17)
    out = np.full((8, 32), 0xA5, np.uint8)
    for row in ([8, 0], [3, 2]):  # no such file, no such block
        rw = np.array([row], np.uint64)
        assert L.sd_cpu_checksum_tree_blocks_prove(level.ctypes.data, bl.lens.ctypes.data, bl.n, 17, rw.ctypes.data, 1,
                                                   out.ctypes.data) == SD_ERR_INVALID
    assert L.sd_cpu_checksum_tree_blocks_prove(None, bl.lens.ctypes.data, bl.n, 17, rw.ctypes.data, 1,
                                               out.ctypes.data) == SD_ERR_INVALID
    assert (out == 0xA5).all()
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_blocks_prove(level, bl.lens, np.array([[3, 2]], np.uint64), 17)
    assert e.value.rc == SD_ERR_INVALID
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_blocks_prove(np.zeros((1, 32), np.uint8), [5], [[0, 0]], 16)
    assert e.value.rc == SD_ERR_INVALID
    proofs, _ = cpu.checksum_tree_blocks_prove(level, bl.lens, bl.rows, 17)
    offs = bl.offsets.copy()
    offs[0] += 8  # a start that is not 16-byte aligned
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_blocks_verify_proofs(bl.data, bl.lens, bl.rows, offs, proofs, roots, 17)
    assert e.value.rc == SD_ERR_INVALID


_levels = {}


def real_level(k: int):
    """(level, roots, node_base) of the real files from the existing CPU tree, held to the oracle"""
    if k not in _levels:
        b = pc.real_batch(k)
        nodes, roots, base = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
        assert np.array_equal(roots, b.checksums)
        _levels[k] = (nodes, roots, base)
    return _levels[k]


@pytest.mark.parametrize("k", pc.KS)
def test_real_files_prove_and_verify(k):
    """nb = 1, 2, 3, 5, 8, 9 in one list, shuffled, with repeats: every proof climbs, in pure Python,
    to the oracle's BLAKE3 of the file; verify_proofs passes every row against those checksums and
    hands back the rows' nodes; proof_base is sd_checksum_tree_proof_entries row by row"""
    bl, b = pc.real_list(k), pc.real_batch(k)
    level, _, _ = real_level(k)
    proofs, base = cpu.checksum_tree_blocks_prove(level, bl.lens, bl.rows, k)
    assert np.array_equal(base, pc.proof_base(bl.lens, bl.rows, k))
    for r, (f, j) in enumerate(bl.rows):
        assert int(base[r + 1] - base[r]) == cpu.tree_proof_entries(int(bl.lens[int(f)]), int(j), k)
    pc.check_proofs(bl.lens, bl.rows, k, level, proofs, [c.tobytes() for c in b.checksums], "cpu prove")
    rows, stats, bad, nodes = cpu.checksum_tree_blocks_verify_proofs(bl.data, bl.lens, bl.rows, bl.offsets, proofs,
                                                                     b.checksums, k, want_flags=True, want_nodes=True)
    assert len(rows) == 0 and not bad.any() and list(stats) == [bl.n, bl.m, 0, 0]
    assert np.array_equal(nodes, cpu.checksum_tree_blocks(bl.data, bl.lens, bl.rows, bl.offsets, k, 8))
    assert np.array_equal(nodes, level[bl.slots()])


def test_levels_alone():
    """random levels of 255, 256, 257 and 65 537 nodes: the proofs climb to tc.spec_root of the
    level; an unlisted file's level filled with garbage changes no proof"""
    lens, rows, level, roots = pc.level_case()
    proofs, _ = cpu.checksum_tree_blocks_prove(level, lens, rows, pc.LEVEL_K)
    pc.check_proofs(lens, rows, pc.LEVEL_K, level, proofs, roots, "cpu levels")
    again, _ = cpu.checksum_tree_blocks_prove(pc.garbage_level(), lens, rows, pc.LEVEL_K)
    assert np.array_equal(again, proofs)


def test_rejections():
    k = 17
    bl, b = pc.real_list(k), pc.real_batch(k)
    proofs, _ = cpu.checksum_tree_blocks_prove(real_level(k)[0], bl.lens, bl.rows, k)
    for name, data, pf, roots, want in pc.rejections(bl, proofs, b.checksums):
        bad, rows, stats = pc.expected_flags(bl, want)
        got_rows, got_stats, got_bad = cpu.checksum_tree_blocks_verify_proofs(data, bl.lens, bl.rows, bl.offsets, pf,
                                                                              roots, k, want_flags=True)
        assert np.array_equal(got_bad, bad), name
        assert np.array_equal(got_rows, rows) and np.array_equal(got_stats, stats), name


def test_capacity_and_count_only():
    k = 17
    bl, b = pc.real_list(k), pc.real_batch(k)
    proofs, _ = cpu.checksum_tree_blocks_prove(real_level(k)[0], bl.lens, bl.rows, k)
    name, data, pf, roots, want = pc.rejections(bl, proofs, b.checksums)[2]
    assert name == "root" and len(want) >= 5
    bad, rows, stats = pc.expected_flags(bl, want)
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_blocks_verify_proofs(data, bl.lens, bl.rows, bl.offsets, pf, roots, k, capacity=len(want) - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == len(want) and np.array_equal(e.value.stats, stats)
    got_rows, got_stats = cpu.checksum_tree_blocks_verify_proofs(data, bl.lens, bl.rows, bl.offsets, pf, roots, k,
                                                                 capacity=len(want))
    assert np.array_equal(got_rows, rows)
    got_rows, got_stats = cpu.checksum_tree_blocks_verify_proofs(data, bl.lens, bl.rows, bl.offsets, pf, roots, k,
                                                                 want_rows=False)
    assert len(got_rows) == 0 and np.array_equal(got_stats, stats)


def test_empty_list():
    lens = pc.real_lens(17)
    none = np.zeros((0, 2), np.uint64)
    proofs, base = cpu.checksum_tree_blocks_prove(np.zeros((sum(tc.nodes_of(x, 17) for x in lens), 32), np.uint8), lens,
                                                  none, 17)
    assert len(proofs) == 0 and list(base) == [0]
    rows, stats = cpu.checksum_tree_blocks_verify_proofs(np.zeros(64, np.uint8), lens, none, np.zeros(0, np.uint64),
                                                         proofs, np.zeros((len(lens), 32), np.uint8), 17)
    assert len(rows) == 0 and not stats.any()
    L = lib()
    assert L.sd_cpu_checksum_tree_blocks_prove(None, None, 0, 17, None, 0, None) == 0
    assert L.sd_cpu_checksum_tree_blocks_verify_proofs(None, None, 0, 17, None, None, 0, None, None, None, None, None, 0,
                                                       None, None, 1) == 0


def test_file_round_trip(tmp_path):
    """the sender's prove_blocks, the receiver's verify_proofs_file with the checksum and the length
    alone; then one listed block is overwritten and named"""
    k = 17
    B = 1 << k
    data = np.random.default_rng(5).integers(0, 256, 9 * B + 333, dtype=np.uint8)
    p = tmp_path / "f"
    p.write_bytes(data.tobytes())
    hexsum, length, nodes = tree.file_checksum_tree(p, k)
    from oracle import native
    assert bytes.fromhex(hexsum) == native.checksums(np.concatenate([data, np.zeros(64, np.uint8)]), np.zeros(1, np.uint64),
                                                     np.array([length], np.uint64), nthreads=2)[0].tobytes()
    blocks = [9, 0, 4, 7, 4]
    proofs = tree.prove_blocks(nodes, length, blocks, k)
    assert len(proofs) == 32 * sum(cpu.tree_proof_entries(length, j, k) for j in blocks)
    assert tree.verify_proofs_file(p, length, hexsum, blocks, proofs, k) == []
    assert tree.verify_proofs_file(p, length, bytes.fromhex(hexsum), blocks, proofs, k) == []
    with open(p, "r+b") as f:
        f.seek(7 * B + 100)
        f.write(bytes([data[7 * B + 100] ^ 0xFF]))
    assert tree.verify_proofs_file(p, length, hexsum, blocks, proofs, k) == [7]
    with pytest.raises(ValueError):
        tree.prove_blocks(nodes, length, [10], k)
