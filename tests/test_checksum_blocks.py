"""Listed blocks on the host (include/sd_cas.h, checksum trees, listed blocks):
sd_cpu_checksum_tree_blocks / _verify / _update and the Python layer (cpu.checksum_tree_blocks*,
tree.verify_blocks_file, tree.update_file, tree.blocks_to_rehash) on the cases of
tests/checksum_blocks_cases.py, against the pure-Python spec and the oracle.
tests/test_gpu_checksum_blocks.py runs the same cases through k_ck_blocks."""
import ctypes
import os

import numpy as np
import pytest

from oracle import native
from spacedrive_amd import cpu, tree
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from tests import checksum_blocks_cases as bc
from tests import checksum_tree_cases as tc
from tests import high_counter_cases as hc

SD_ERR_INVALID = -1


def twin(bl: bc.BlockList, data=None, nthreads: int = 8) -> np.ndarray:
    return cpu.checksum_tree_blocks(bl.data if data is None else data, bl.lens, bl.rows, bl.offsets, bl.k, nthreads)


def check_updated_nodes(nb: tc.Batch, rows, level) -> None:
    """the listed nodes of a patched level: the spec of the changed bytes where it is cheap (the
    one-node file, the 1-byte block), sd_cpu_checksum_tree of the changed files for all of them"""
    k = nb.k
    B = 1 << k
    whole, _, _ = cpu.checksum_tree(nb.data, nb.offsets, nb.lens, k, 8)
    for f, j in rows:
        s = int(nb.node_base[f]) + j
        assert np.array_equal(level[s], whole[s]), (k, f, j)
        size = bc.block_len(int(nb.lens[f]), j, k)
        if size <= 4097:
            data = nb.file(f)[j * B:j * B + size]
            want = tc.spec_nodes(data, k)[0].tobytes() if int(nb.nb[f]) == 1 else hc.spec_block_cv(data, j * B // 1024)
            assert level[s].tobytes() == want, (k, f, j)


@pytest.mark.parametrize("nthreads", [1, 8])
@pytest.mark.parametrize("k", bc.KS)
def test_twin_shape_list(k, nthreads):
    """every block of the shape files, shuffled, scattered over junk: the direct rows against the
    spec, every file's root identity, and the level sd_cpu_checksum_tree gives for the same bytes"""
    bl, b = bc.shape_list(k), bc.shape_batch(k)
    nodes = twin(bl, nthreads=nthreads)
    bc.check_list(bl, nodes, b, bc.direct_nodes(k), "twin")
    level, _, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, nthreads)
    assert np.array_equal(bc.level_of(bl, nodes), level)


@pytest.mark.parametrize("k", bc.KS)
def test_twin_high_counters(k):
    """blocks at chunk counters 2^32 - 128 .. 2^32 + 128 of files of 4 TiB: only they are resident"""
    bl = bc.high_list(k)
    assert np.array_equal(twin(bl), bc.high_expected(k))


@pytest.mark.parametrize("k", bc.KS)
def test_twin_packing_prefixes(k):
    bl, want = bc.packing_list(k)
    for m in range(0, 34):
        assert np.array_equal(twin(bl.prefix(m)), want[:m]), (k, m)


@pytest.mark.parametrize("k", bc.KS)
def test_twin_verify(k):
    """the flips: rows in list order, flags, stats; a repeated row twice; a flip in a block the list
    omits not reported; a capacity one short"""
    bl, b = bc.shape_list(k), bc.shape_batch(k)
    level, _, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
    listed, unlisted = bc.flip_cases(k)
    rows, stats, bad = cpu.checksum_tree_blocks_verify(bl.data, bl.lens, bl.rows, bl.offsets, level, k, want_flags=True)
    assert len(rows) == 0 and list(stats) == [bl.n, bl.m, 0, 0] and not bad.any()
    # the flips, the big file's middle block listed a second time
    B = 1 << k
    again = (listed[0][0], listed[0][1] // B)
    rep = bc.BlockList(bl.lens, k, [tuple(r) for r in bl.rows.tolist()] + [again], bc.blocks_of(b), seed=5, odd=2)
    d = bc.flipped_list(rep, listed + [unlisted])
    want_bad, want_rows, want_stats = bc.expected_verify(rep, listed + [unlisted])
    assert int(want_stats[2]) == 5 and int(want_stats[3]) == 3 and tuple(want_rows[-1]) == again
    rows, stats, bad = cpu.checksum_tree_blocks_verify(d, rep.lens, rep.rows, rep.offsets, level, k, want_flags=True)
    assert np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats) and np.array_equal(bad, want_bad)
    rows, stats = cpu.checksum_tree_blocks_verify(d, rep.lens, rep.rows, rep.offsets, level, k, want_rows=False)
    assert len(rows) == 0 and np.array_equal(stats, want_stats)
    # a second list that omits the block of the last flip: that flip is not reported
    drop = [r for r, (f, j) in enumerate(rep.rows) if (int(f), int(j)) == (unlisted[0], unlisted[1] // B)]
    assert len(drop) == 1
    part = rep.without(drop)
    want_bad, want_rows, want_stats = bc.expected_verify(part, listed)
    rows, stats, bad = cpu.checksum_tree_blocks_verify(d, part.lens, part.rows, part.offsets, level, k, want_flags=True)
    assert np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats) and np.array_equal(bad, want_bad)
    assert int(stats[2]) == 4 and int(stats[3]) == 2
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_blocks_verify(d, part.lens, part.rows, part.offsets, level, k, capacity=3)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == 4 and np.array_equal(e.value.stats, want_stats)


@pytest.mark.parametrize("k", bc.KS)
def test_twin_update(k):
    """three changed blocks patched into the old level: the listed nodes are the changed data's,
    every other node is bit-identical, the roots are the oracle's of the changed files"""
    b, nb = bc.shape_batch(k), bc.changed_batch(k)
    changes, rows = bc.update_case(k)
    old, old_roots, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
    bl = bc.BlockList(nb.lens, k, rows, bc.blocks_of(nb), seed=9, odd=1)
    level, roots = cpu.checksum_tree_blocks_update(bl.data, bl.lens, bl.rows, bl.offsets, old, k)
    slots = bl.slots()
    rest = np.setdiff1d(np.arange(b.total), slots)
    assert np.array_equal(level[rest], old[rest]) and not any(np.array_equal(level[s], old[s]) for s in slots)
    check_updated_nodes(nb, rows, level)
    for i in range(b.n):
        assert tc.spec_root(nb.level(level, i)) == nb.checksums[i].tobytes(), (k, i)
        assert roots[i].tobytes() == nb.checksums[i].tobytes(), (k, i)
    touched = {f for f, _ in rows}
    assert all((roots[i].tobytes() == old_roots[i].tobytes()) == (i not in touched) for i in range(b.n))
    # a repeated row: refused, the level untouched
    rep = bc.BlockList(nb.lens, k, rows + rows[:1], bc.blocks_of(nb), seed=9)
    keep = old.copy()
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_blocks_update(rep.data, rep.lens, rep.rows, rep.offsets, keep, k)
    assert e.value.rc == SD_ERR_INVALID and np.array_equal(keep, old)
    rc = lib().sd_cpu_checksum_tree_blocks_update(rep.data.ctypes.data, rep.lens.ctypes.data, rep.n, k, rep.rows.ctypes.data,
                                                  rep.offsets.ctypes.data, rep.m, keep.ctypes.data,
                                                  np.zeros((rep.n, 32), np.uint8).ctypes.data, 1)
    assert rc == SD_ERR_INVALID and np.array_equal(keep, old)


def test_twin_invalid_arguments():
    L = lib()
    lens = np.array([100, (1 << 17) + 1], np.uint64)
    rows, offs = np.array([[0, 0], [1, 1]], np.uint64), np.array([0, 1024], np.uint64)
    data = np.zeros(4096, np.uint8)
    out = np.full((2, 32), 0xA5, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def run(d=data, ls=lens, k=17, rw=rows, of=offs, o=out, m=2):
        return L.sd_cpu_checksum_tree_blocks(p(d), p(ls), len(lens), k, p(rw), p(of), m, p(o), 1)

    assert run(rw=np.array([[2, 0], [1, 1]], np.uint64)) == SD_ERR_INVALID      # file >= n_files
    assert run(rw=np.array([[0, 1], [1, 1]], np.uint64)) == SD_ERR_INVALID      # block >= nb
    assert run(rw=np.array([[0, 0], [1, 2]], np.uint64)) == SD_ERR_INVALID
    assert run(of=np.array([0, 1032], np.uint64)) == SD_ERR_INVALID             # not 16-byte aligned
    for k in (0, 16, 21, 1 << 20):
        assert run(k=k) == SD_ERR_INVALID
    for kw in ({"d": None}, {"ls": None}, {"rw": None}, {"of": None}, {"o": None}):
        assert run(**kw) == SD_ERR_INVALID
    assert (out == 0xA5).all()
    assert run(m=0) == 0 and run(d=None, rw=None, of=None, o=None, m=0) == 0 and (out == 0xA5).all()
    assert run() == 0
    want = cpu.checksum_tree(np.zeros(1 << 18, np.uint8), [0, 4096], lens, 17, 1)[0]
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[2])  # 100 zeros; a zero byte at counter 128
    # m == 0: verify and update are no-ops
    cnt, stats = ctypes.c_uint64(7), np.full(4, 7, np.uint64)
    assert L.sd_cpu_checksum_tree_blocks_verify(None, p(lens), 2, 17, None, None, 0, None, None, None, 0,
                                                ctypes.byref(cnt), p(stats), 1) == 0
    assert cnt.value == 0 and not stats.any()
    assert L.sd_cpu_checksum_tree_blocks_update(None, p(lens), 2, 17, None, None, 0, None, None, 1) == 0


def test_blocks_to_rehash_complements_common_blocks():
    for k in (17, 20):
        B = 1 << k
        sizes = [0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 5 * B + 7, 9 * B]
        for a in sizes:
            for b in sizes:
                re, co = tree.blocks_to_rehash(a, b, k), tree.common_blocks(a, b, k)
                nb = max(1, -(-b // B))
                assert not set(re) & set(co) and re == sorted(re), (k, a, b)
                assert set(re) | {j for j in co if j < nb} == set(range(nb)), (k, a, b)
                if min(a, b) > B:
                    assert sorted(re + co) == list(range(nb)), (k, a, b)   # a partition of the new file's blocks
                else:
                    assert re == list(range(nb)) and co == []
    with pytest.raises(ValueError):
        tree.blocks_to_rehash(1, 2, 9)


@pytest.mark.parametrize("k", [17, 19])
def test_update_file_and_verify_blocks_file(tmp_path, k):
    """a write in place, an append and a truncation go through update_file reading only the listed
    blocks; verify_blocks_file names the listed blocks that differ"""
    B = 1 << k
    path = tmp_path / "f.bin"
    data = bytearray(native.synth_bytes(77, 0, 0, 5 * B + 300))
    path.write_bytes(data)
    hex0, length, nodes = tree.file_checksum_tree(path, k)
    assert tree.verify_blocks_file(path, length, nodes, [4, 0, 5, 2], k) == []
    # a write in place over blocks 1 and 2
    with open(path, "r+b") as f:
        f.seek(2 * B - 3)
        f.write(b"\x00" * 7)
    assert tree.verify_blocks_file(path, length, nodes, [5, 2, 0, 1], k) == [2, 1]
    assert tree.verify_blocks_file(path, length, nodes, [0, 3, 4, 5], k) == []
    hex1, nodes1 = tree.update_file(path, length, nodes, [1, 2], k)
    want = tree.file_checksum_tree(path, k)
    assert hex1 == want[0] != hex0 and np.array_equal(nodes1, want[2])
    # an append: the partial last block and the new ones
    with open(path, "ab") as f:
        f.write(native.synth_bytes(78, 0, 0, 2 * B + 11))
    new_len = length + 2 * B + 11
    re = tree.blocks_to_rehash(length, new_len, k)
    assert re == [5, 6, 7]
    hex2, nodes2 = tree.update_file(path, new_len, nodes1, re, k)
    want = tree.file_checksum_tree(path, k)
    assert (hex2, new_len) == want[:2] and np.array_equal(nodes2, want[2])
    with pytest.raises(ValueError):
        tree.update_file(path, new_len, nodes1, [5, 6], k)  # block 7 is new and not listed
    # a truncation to one block: its node turns into the root hash
    os.truncate(path, B - 9)
    re = tree.blocks_to_rehash(new_len, B - 9, k)
    assert re == [0]
    hex3, nodes3 = tree.update_file(path, B - 9, nodes2, re, k)
    want = tree.file_checksum_tree(path, k)
    assert (hex3, B - 9) == want[:2] and np.array_equal(nodes3, want[2])
    with pytest.raises(ValueError):
        tree.verify_blocks_file(path, new_len, nodes2, [3], k)  # the file no longer holds that block
