"""Checksum trees on the host (include/sd_cas.h, checksum trees): sd_cpu_checksum_tree / _roots /
_verify, sd_checksum_tree_nodes and the Python layer (cpu.checksum_tree*, tree.py) against the
restated definitions of tests/checksum_tree_cases.py; the stand-alone selftest's plain build.
tests/test_gpu_checksum_tree.py runs the same cases through the kernels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import native
from spacedrive_amd import _native, cpu, tree
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from tests import checksum_tree_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
SD_ERR_INVALID = -1


@pytest.mark.parametrize("nthreads", [1, 8])
@pytest.mark.parametrize("k", tc.KS)
def test_twin_levels_and_roots(k, nthreads):
    """every shape in one batch: levels node by node or by the root identity, roots against the
    oracle, the position rule against the truncated twin batch"""
    b, t = tc.shape_batch(k), tc.truncated_batch(k)
    nodes, roots, base = cpu.checksum_tree(b.data, b.offsets, b.lens, k, nthreads)
    assert np.array_equal(base, b.node_base)
    tc.check_levels(b, nodes, roots, tc.direct_levels(k), "twin")
    t_nodes, t_roots, _ = cpu.checksum_tree(t.data, t.offsets, t.lens, k, nthreads)
    tc.check_levels(t, t_nodes, t_roots, None, "twin, truncated")
    tc.check_position_rule(b, nodes, t, t_nodes, "twin")


@pytest.mark.parametrize("k", tc.KS)
def test_twin_roots_from_levels(k):
    b = tc.shape_batch(k)
    nodes, _, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
    roots = cpu.checksum_tree_roots(nodes, b.lens, k)
    assert np.array_equal(roots, b.checksums)
    # a level that was tampered with no longer belongs to the checksum
    bad = nodes.copy()
    i = int(np.argmax(b.nb))
    bad[int(b.node_base[i]) + 1, 5] ^= 0x10
    roots = cpu.checksum_tree_roots(bad, b.lens, k)
    assert [j for j in range(b.n) if not np.array_equal(roots[j], b.checksums[j])] == [i]


def test_node_counts_and_layout():
    for k in tc.KS:
        B = 1 << k
        lens = [0, 1, B - 1, B, B + 1, 2 * B, 2 * B + 1, 7 * B - 1, (1 << 40) + 1, (1 << 63) + 5]
        for length in lens:
            want = max(1, -(-length // B))
            assert cpu.tree_nodes(length, k) == want, (k, length)
        base = cpu.tree_node_base(lens[:-1], k)
        assert base[0] == 0 and list(np.diff(base)) == [max(1, -(-x // B)) for x in lens[:-1]]
    assert tc.nodes_of(2 * tc.MIB + 1, 17) == 17


def test_invalid_arguments():
    L = lib()
    n = ctypes.c_uint64(99)
    for k in (0, 10, 16, 21, 32, 1 << 31):
        assert L.sd_checksum_tree_nodes(1000, k, ctypes.byref(n)) == SD_ERR_INVALID, k
        with pytest.raises(SdCasError):
            cpu.tree_node_base([5], k)
    assert L.sd_checksum_tree_nodes(1000, 17, None) == SD_ERR_INVALID
    data = np.zeros(4096, np.uint8)
    offs, lens = np.array([0, 1024], np.uint64), np.array([100, 200], np.uint64)
    nodes, roots = np.full((2, 32), 0xA5, np.uint8), np.full((2, 32), 0xA5, np.uint8)
    bad, rows = np.full(2, 0xA5, np.uint8), np.full((2, 2), 0xA5A5, np.uint64)
    cnt, stats = ctypes.c_uint64(0), np.zeros(4, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def tree(d=data, o=offs, ln=lens, k=17, nd=nodes, r=roots):
        return L.sd_cpu_checksum_tree(p(d), p(o), p(ln), 2, k, p(nd), p(r), 2)

    def verify(d=data, o=offs, ln=lens, k=17, e=nodes):
        return L.sd_cpu_checksum_tree_verify(p(d), p(o), p(ln), 2, k, p(e), p(bad), p(rows), 2, ctypes.byref(cnt),
                                             p(stats), 2)

    for k in (16, 21):
        assert tree(k=k) == SD_ERR_INVALID and verify(k=k) == SD_ERR_INVALID
        assert L.sd_cpu_checksum_tree_roots(p(nodes), p(lens), 2, k, p(roots)) == SD_ERR_INVALID
    unaligned = np.array([0, 1032], np.uint64)
    assert tree(o=unaligned) == SD_ERR_INVALID and verify(o=unaligned) == SD_ERR_INVALID
    for kw in ({"d": None}, {"o": None}, {"ln": None}, {"nd": None}, {"r": None}):
        assert tree(**kw) == SD_ERR_INVALID, kw
    for kw in ({"d": None}, {"o": None}, {"ln": None}, {"e": None}):
        assert verify(**kw) == SD_ERR_INVALID, kw
    assert L.sd_cpu_checksum_tree_roots(None, p(lens), 2, 17, p(roots)) == SD_ERR_INVALID
    assert L.sd_cpu_checksum_tree_roots(p(nodes), None, 2, 17, p(roots)) == SD_ERR_INVALID
    assert L.sd_cpu_checksum_tree_roots(p(nodes), p(lens), 2, 17, None) == SD_ERR_INVALID
    # nothing was written by any refused call
    assert (nodes == 0xA5).all() and (roots == 0xA5).all() and (bad == 0xA5).all() and (rows == 0xA5A5).all()
    # an empty batch is valid
    assert L.sd_cpu_checksum_tree(None, None, None, 0, 17, None, None, 1) == 0
    assert L.sd_cpu_checksum_tree_verify(None, None, None, 0, 17, None, None, None, 0, ctypes.byref(cnt), p(stats), 1) == 0
    assert cnt.value == 0 and not stats.any()
    assert tree() == 0 and verify() == 0 and cnt.value == 0


@pytest.mark.parametrize("k", tc.KS)
def test_twin_verify(k):
    b = tc.shape_batch(k)
    nodes, _, _ = cpu.checksum_tree(b.data, b.offsets, b.lens, k, 8)
    _, want_rows, want_stats = tc.flips(b)
    # a clean batch: no row
    rows, stats, bad = cpu.checksum_tree_verify(b.data, b.offsets, b.lens, nodes, k, want_flags=True)
    assert len(rows) == 0 and list(stats) == [b.n, b.total, 0, 0] and not bad.any()
    # the flips, all at once, on 1 and 8 threads
    d = tc.flipped(b)
    for nthreads in (1, 8):
        rows, stats, bad = cpu.checksum_tree_verify(d, b.offsets, b.lens, nodes, k, want_flags=True, nthreads=nthreads)
        assert np.array_equal(rows, want_rows) and np.array_equal(stats, want_stats), (rows, stats)
        want_bad = np.zeros(b.total, np.uint8)
        want_bad[[int(b.node_base[f]) + int(j) for f, j in want_rows]] = 1
        assert np.array_equal(bad, want_bad)
    # counting only
    rows, stats = cpu.checksum_tree_verify(d, b.offsets, b.lens, nodes, k, want_rows=False)
    assert len(rows) == 0 and np.array_equal(stats, want_stats)
    # a capacity one short: the requirement, the flags complete, no row written
    L = lib()
    need = len(want_rows)
    buf, bad = np.full((need, 2), 0xA5A5, np.uint64), np.full(b.total, 7, np.uint8)
    cnt, stats = ctypes.c_uint64(0), np.zeros(4, np.uint64)
    rc = L.sd_cpu_checksum_tree_verify(d.ctypes.data, b.offsets.ctypes.data, b.lens.ctypes.data, b.n, k,
                                       nodes.ctypes.data, bad.ctypes.data, buf.ctypes.data, need - 1, ctypes.byref(cnt),
                                       stats.ctypes.data, 8)
    assert rc == SD_ERR_CAPACITY and cnt.value == need and (buf == 0xA5A5).all()
    assert np.array_equal(bad, want_bad) and np.array_equal(stats, want_stats)
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_verify(d, b.offsets, b.lens, nodes, k, capacity=need - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == need


def test_files(tmp_path):
    k = 17
    B = 1 << k
    length = 5 * B + 300
    data = bytearray(native.synth_bytes(77, 0, 0, length))
    path = tmp_path / "a.bin"
    path.write_bytes(data)
    hexd, got_len, nodes = tree.file_checksum_tree(path, k)
    assert got_len == length and nodes.shape == (6, 32)
    assert hexd == native.blake3(bytes(data)).hex() == cpu.file_checksum(path)
    assert tc.spec_root(nodes) == native.blake3(bytes(data))
    assert tree.verify_file(path, length, nodes, k) == []
    for at in (2 * B, length - 1):
        data[at] ^= 0x80
    path.write_bytes(data)
    assert tree.verify_file(path, length, nodes, k) == [2, 5]
    # a file whose length changed: the level no longer describes it
    path.write_bytes(data + b"x")
    with pytest.raises(ValueError):
        tree.verify_file(path, length, nodes, k)
    path.write_bytes(data[:-1])
    with pytest.raises(ValueError):
        tree.verify_file(path, length, nodes, k)
    # small and empty files: one node, the checksum itself
    for n in (0, 1, 5000):
        q = tmp_path / f"s{n}.bin"
        q.write_bytes(bytes(data[:n]))
        hexd, got_len, nodes = tree.file_checksum_tree(q, k)
        assert got_len == n and nodes.shape == (1, 32) and nodes.tobytes().hex() == hexd == native.blake3(bytes(data[:n])).hex()
        assert tree.verify_file(q, n, nodes, k) == []


def test_common_blocks_brute_force():
    """common_blocks against the node-by-node comparison of two spec levels of files that share
    their bytes: at 4 KiB blocks (the rule is arithmetic in the block size) every pair of lengths
    around the block boundaries"""
    k = 12
    B = 1 << k
    lens = [0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B + 100, 4 * B]
    data = native.synth_bytes(5, 0, 0, max(lens))
    levels = {n: tc.spec_nodes(data[:n], k) for n in lens}
    for a in lens:
        for b in lens:
            got = tree.common_blocks(a, b, k)
            la, lb = levels[a], levels[b]
            equal = [j for j in range(min(len(la), len(lb))) if np.array_equal(la[j], lb[j])]
            if a == b:  # the same file: every node is equal, the partial and the single one too
                assert equal == list(range(len(la))) and set(got) <= set(equal)
            else:  # the same bytes at another length: exactly the comparable blocks agree
                assert got == equal, (a, b, got, equal)


def test_checksum_tree_selftest():
    b = subprocess.run(["make", "-C", CSRC, "-j8", "checksum-tree-selftest"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "checksum_tree_selftest")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "checksum_tree_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_binding_covers_the_new_calls():
    names = {n for n, _, _ in _native.SIGNATURES}
    hdr = open(_native.HEADER).read()
    for f in ("sd_checksum_tree_nodes", "sd_checksum_tree_create", "sd_checksum_tree_destroy", "sd_checksum_tree_layout",
              "sd_checksum_tree_stats", "sd_checksum_tree_run", "sd_checksum_tree_roots", "sd_checksum_tree_verify",
              "sd_cpu_checksum_tree", "sd_cpu_checksum_tree_roots", "sd_cpu_checksum_tree_verify"):
        assert f in names and f + "(" in hdr, f
        assert f in open(os.path.join(ROOT, "integration", "rust", "sd-cas-sys", "src", "lib.rs")).read(), f
    assert "#define SD_CAS_ABI_VERSION 2" in hdr
    assert (_native.SD_TREE_BLOCK_LOG2_MIN, _native.SD_TREE_BLOCK_LOG2_MAX) == (17, 20)
