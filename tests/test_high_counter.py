"""Chunk counters past 2^32 and three-pass reduce trees on the host (tests/high_counter_cases.py):
the references pinned against each other and against tests/golden/high_counter.json, then the
library's CPU twins -- sd_cpu_split_leaves at every lane width on a slice whose counters cross
2^32, sd_cpu_split_root and sd_cpu_checksum_tree_roots on levels of more than 65 536 CVs.
tests/test_gpu_high_counter.py holds the kernels to the same cases."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import blake3_spec as b3
from oracle import native
from spacedrive_amd import cpu
from spacedrive_amd._native import check, lib
from spacedrive_amd.split import cpu_root, split_range
from tests import high_counter_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5


def block_bytes(b: int, length: int = hc.MIB) -> bytes:
    return native.synth_bytes(hc.CID, 0, b * hc.MIB, length)


# ------------------------------------------------------------- 1. the references pin each other
def test_golden_control_tells_a_truncated_counter(golden):
    """the masked-counter CV equals the true one for block B0 (counters up to 2^32 - 1) and differs
    for block B0 + 1: without that the cases could not tell a truncation from none"""
    g = golden["high_counter"]
    assert (g["content_id"], g["twin"], g["offset"], g["ranks"], g["rank"]) == (hc.CID, 0, hc.B0 * hc.MIB, hc.R, hc.RANK)
    lo, hi = g["blocks"]
    assert (lo["block"], lo["chunk0"]) == (hc.B0, 2 ** 32 - 1024) and (hi["block"], hi["chunk0"]) == (hc.B0 + 1, 2 ** 32)
    assert lo["cv"] == lo["cv_counter_mod_2_32"]
    assert hi["cv"] != hi["cv_counter_mod_2_32"]
    assert len({lo["cv"], hi["cv"], hi["cv_counter_mod_2_32"]}) == 3 and all(len(x["cv"]) == 64 for x in (lo, hi))


@pytest.mark.parametrize("simd", [0, -1])
def test_oracle_subtree_cv_against_the_spec(golden, simd):
    """native.subtree_cv, scalar and SIMD: the golden spec CVs of the full blocks either side of the
    wrap, and the spec computed live for the short block after them"""
    for blk in golden["high_counter"]["blocks"]:
        got = native.subtree_cv(block_bytes(blk["block"]), blk["chunk0"], simd).hex()
        assert got == blk["cv"], (blk["block"], simd)
        if blk["block"] > hc.B0:
            assert got != blk["cv_counter_mod_2_32"]
    case = hc.small_case()
    short = block_bytes(hc.B0 + 2, hc.SHORT_LAST)
    assert case.block_len(2) == len(short) and case.chunk0(2) == (hc.B0 + 2) * 1024
    want = hc.spec_block_cv(short, case.chunk0(2))
    assert native.subtree_cv(short, case.chunk0(2), simd) == want
    assert native.subtree_cv(np.frombuffer(short, np.uint8), case.chunk0(2), simd) == want
    assert hc.spec_block_cv(short, case.chunk0(2), 0xFFFFFFFF) != want
    # one chunk and one byte of it: the counter reaches scalar_chunk directly
    assert native.subtree_cv(short[:1024], 2 ** 32 + 5, simd) == hc.spec_block_cv(short[:1024], 2 ** 32 + 5)
    assert native.subtree_cv(short[:1], 2 ** 33, simd) == hc.spec_block_cv(short[:1], 2 ** 33)


def test_np_root_against_the_spec():
    """np_root: BLAKE3 itself for 1 .. 9 chunks, and the spec's parent tree for 255, 256 and 257
    random CVs, root and non-root"""
    data = native.synth_bytes(77, 0, 0, 9 * 1024)
    for c in range(1, 10):
        d = data[:c * 1024 - 5]
        cvs = [b3.chunk_cv(d[i * 1024:(i + 1) * 1024], i, c == 1) for i in range(c)]
        packed = np.frombuffer(b"".join(struct.pack("<8I", *cv) for cv in cvs), np.uint8).reshape(c, 32)
        assert hc.np_root(packed) == b3.blake3(d), c
        assert hc.np_root(packed.view("<u4")) == b3.blake3(d), c
    for n in (255, 256, 257):
        cvs = hc.random_cvs(n, n)
        words = [struct.unpack("<8I", r.tobytes()) for r in cvs]
        for root in (True, False):
            assert hc.np_root(cvs, root) == struct.pack("<8I", *hc.spec_merge(words, root)), (n, root)
    one = hc.random_cvs(1, 1)
    assert hc.np_root(one) == one[0].tobytes()
    three = hc.np_parents(hc.random_cvs(5, 5).view("<u4"))
    assert three.shape == (3, 8) and three[2].tobytes() == hc.random_cvs(5, 5)[4].tobytes()  # the odd node carried up


def test_split_arithmetic_matches_the_library():
    for case in (hc.small_case(), hc.wide_case(256), hc.wide_case(515 // 2), hc.cpu_case()):
        assert split_range(case.total, hc.R, hc.RANK) == (case.offset, case.len, case.cv_bytes)
    total = hc.EMPTY_RANK_TOTAL  # a rank that holds nothing
    assert split_range(total, 4096, 4095) == hc.split_arith(total, 4096, 4095)[1:] == (total, 0, 4096 * 32)


# ------------------------------------------------------------------------ 2. sd_cpu_split_leaves
@functools.lru_cache(maxsize=None)
def cpu_slice() -> tuple:
    """(the n = 40 slice uint8 [len + 64], the oracle's CV of each of its blocks uint8 [40, 32])"""
    case = hc.cpu_case()
    s = np.zeros(case.len + 64, np.uint8)
    s[:case.len] = np.frombuffer(native.synth_bytes(hc.CID, 0, case.offset, case.len), np.uint8)
    want = b"".join(native.subtree_cv(s[k * hc.MIB:k * hc.MIB + case.block_len(k)], case.chunk0(k)) for k in range(case.n))
    s.setflags(write=False)
    return s, np.frombuffer(want, np.uint8).reshape(case.n, 32)


def check_cpu_leaves(threads=(1, 3)) -> None:
    """every one of the rank's 40 slots is the oracle's CV at the block's 64-bit counter; every
    other byte of the cv_bytes buffer is untouched"""
    case = hc.cpu_case()
    s, want = cpu_slice()
    for nt in threads:
        cvs = np.full(case.cv_bytes + 64, POISON, np.uint8)
        check(lib().sd_cpu_split_leaves(s.ctypes.data, case.total, hc.R, hc.RANK, cvs.ctypes.data, nt))
        got = cvs[:case.cv_bytes].reshape(-1, 32)
        bad = [k for k in range(case.n) if not np.array_equal(got[hc.B0 + k], want[k])]
        assert not bad, (nt, bad)
        assert (got[:hc.B0] == POISON).all() and (got[hc.B0 + case.n:] == POISON).all() and (cvs[case.cv_bytes:] == POISON).all()


def test_cpu_split_leaves_past_2_32(golden):
    check_cpu_leaves((1, 3))
    _, want = cpu_slice()  # the first two slots are the spec's too
    assert [w.tobytes().hex() for w in want[:2]] == [b["cv"] for b in golden["high_counter"]["blocks"]]


@pytest.mark.parametrize("lanes", [4, 8, 16])
def test_cpu_split_leaves_past_2_32_simd_widths(lanes):
    """the same at each chunk-lane width the host supports, in a child process (the width is picked
    once per process)"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from spacedrive_amd import cpu\n"
            "print(cpu.simd_lanes())\n"
            "from tests import test_high_counter as t\n"
            "t.check_cpu_leaves((1, 3))\n") % ROOT
    env = dict(os.environ, SD_CPU_LANES=str(lanes))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = int(r.stdout.split()[0])
    assert got <= lanes
    if got < lanes:
        pytest.skip(f"host CPU runs {got} lanes at most")


# ------------------------------------------------------------------------- 3. deep roots, host
@pytest.mark.parametrize("count", hc.REDUCE_COUNTS)
def test_cpu_split_root_deep(count):
    cvs, total, want = hc.reduce_case(count)
    assert cpu_root(cvs, total) == want


@pytest.mark.parametrize("k", hc.KS)
def test_cpu_tree_roots_mixed_depths(k):
    """files that finish at passes 0 .. 3 in one batch, and the same files in reverse order; a
    single-node file's root is its node"""
    for counts in (hc.MIXED_COUNTS, hc.MIXED_COUNTS[::-1]):
        b = hc.MixedBatch(k, counts)
        assert [int(x) for x in cpu.tree_node_base(b.lens, k)] == [int(x) for x in b.node_base]
        nodes = b.nodes()
        got = cpu.checksum_tree_roots(nodes, b.lens, k)
        assert np.array_equal(got, b.roots())
        i = counts.index(1)
        assert got[i].tobytes() == nodes[int(b.node_base[i])].tobytes()
