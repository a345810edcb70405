"""Chunk counters past 2^32 and reduce trees of three passes: the references and the cases, shared
by tests/test_high_counter.py (the CPU twins) and tests/test_gpu_high_counter.py (the kernels).
No device and no library call in here: plain integers, numpy, and oracle/blake3_spec.py.

High counters.  compress() takes BLAKE3's chunk counter as two 32-bit words.  A slice of a file
hashed at its true position reaches counters past 2^32 without the 4 TiB before it:
2^22 - 1 = 2049 x 2047, so a file of B0 + n 1 MiB blocks (B0 = 2^22 - 1, 1 <= n <= 2047) over
R = 2050 ranks has q = ceil((B0 + n) / R) = 2047 blocks per rank and rank 2049 holds the blocks
[B0, B0 + n): about n MiB whose chunk counters run from 0xFFFFFC00 through 2^32 and on.  The low
word wraps exactly on a block boundary: block 0 of the slice has a high word of 0, every later
block a high word of 1.

Deep trees.  A reduce pass takes 256 CVs per workgroup, so a message of more than 65 536 CVs takes
three passes (65 537 -> 257 -> 2 -> 1).  A fourth pass needs more than 2^24 CVs, 512 MiB of them:
out of scope here.

The references:
  spec_block_cv(data, chunk0)  the non-root CV of one block of at most 1 MiB, from the spec's
                               chunk_cv and compress; Python integers cannot truncate the counter
  np_parents / np_root         BLAKE3's parent compression over a whole level in numpy uint32, one
                               level per call, the odd node carried up, ROOT on the final parent;
                               a restatement of the spec's G, rounds and permutation -- neither the
                               code under test nor the oracle
"""
import functools
import struct

import numpy as np

from oracle import blake3_spec as b3

MIB = 1 << 20
CHUNK = 1024
R = 2050              # ranks
RANK = R - 1          # the rank whose slice starts at block B0
B0 = 2 ** 22 - 1      # the block whose last chunk has counter 2^32 - 1
Q = 2047              # blocks per rank
CID = 4242            # the synthetic content the slices hold (twin 0)

assert B0 == RANK * Q and B0 * (MIB // CHUNK) == 2 ** 32 - 1024


def total_len(n: int, cut: int) -> int:
    """the file of B0 + n blocks whose last block is `cut` bytes short of 1 MiB"""
    return (B0 + n) * MIB - cut


def split_arith(total: int, nranks: int, rank: int) -> tuple:
    """(q, offset, length, cv_bytes) of include/sd_cas.h's sd_split_range, in plain integers; a
    rank past the last block holds nothing, at the file's end"""
    nb = max(1, -(-total // MIB))
    q = -(-nb // nranks)
    b0, b1 = min(rank * q, nb), min((rank + 1) * q, nb)
    off = min(total, b0 * MIB)
    return q, off, min(total, b1 * MIB) - off, nranks * q * 32


class LeafCase:
    """rank RANK's slice of n blocks, the last one `last` bytes long"""

    def __init__(self, n: int, last: int):
        assert 1 <= n <= Q and 1 <= last <= MIB
        self.n, self.last = n, last
        self.total = total_len(n, MIB - last)
        q, off, length, cv_bytes = split_arith(self.total, R, RANK)
        assert q == Q and off == B0 * MIB and length == (n - 1) * MIB + last and cv_bytes == R * Q * 32 == 134_283_200
        assert split_arith(self.total, R, RANK - 1)[1:3] == ((B0 - Q) * MIB, Q * MIB)  # the rank before it is full
        self.offset, self.len, self.cv_bytes = off, length, cv_bytes
        self.slots = cv_bytes // 32

    def block_len(self, k: int) -> int:
        return MIB if k < self.n - 1 else self.last

    def chunk0(self, k: int) -> int:
        """the counter of the first chunk of the slice's block k: past 2^32 for every k >= 1"""
        c = (B0 + k) * (MIB // CHUNK)
        assert (c >> 32) == (1 if k else 0) and (c + MIB // CHUNK - 1) >> 32 == (1 if k else 0)
        return c


EMPTY_RANK_TOTAL = 3 * MIB - 1   # a 3-block file over 4096 ranks: rank 4095 holds nothing
SHORT_LAST = 5 * CHUNK + 7       # a block of 5 full chunks and 7 bytes
WIDE_LAST = 1021 * CHUNK + 1     # 1021 full chunks and 1 byte


def small_case() -> LeafCase:
    """3 blocks: 2 workgroups, the second half empty -- a launch without priority windows"""
    return LeafCase(3, SHORT_LAST)


def wide_case(cus: int) -> LeafCase:
    """2 CUs + 3 blocks: more waves than 4 x CUs, so the windowed instantiation, its last workgroup
    half empty"""
    n = 2 * cus + 3
    assert n <= Q and n % 2 == 1 and 8 * ((n + 1) // 2) > 4 * cus and 8 * ((3 + 1) // 2) <= 4 * cus
    return LeafCase(n, WIDE_LAST)


def cpu_case() -> LeafCase:
    """what the host twins hash: 40 blocks"""
    return LeafCase(40, SHORT_LAST)


# ----------------------------------------------------------------------------- the spec, per block
def spec_merge(level, root: bool) -> list:
    """level-wise pairwise merge, the odd node carried up, ROOT (if asked) on the last parent"""
    level = [list(x) for x in level]
    while len(level) > 1:
        fl = b3.PARENT | (b3.ROOT if root and len(level) == 2 else 0)
        nxt = [b3.compress(b3.IV, level[i] + level[i + 1], 0, b3.BLOCK_LEN, fl)[:8] for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def spec_block_cv(data: bytes, chunk0: int, counter_mask: int = -1) -> bytes:
    """the non-root CV of one block of at most 1 MiB whose first chunk has counter chunk0;
    counter_mask = 0xFFFFFFFF is the control: what a 32-bit counter would give"""
    assert 0 < len(data) <= MIB
    nch = -(-len(data) // CHUNK)
    cvs = [b3.chunk_cv(data[c * CHUNK:(c + 1) * CHUNK], (chunk0 + c) & counter_mask, False) for c in range(nch)]
    return struct.pack("<8I", *spec_merge(cvs, False))


# --------------------------------------------------------------------- parents, a level at a time
_IV = np.array(b3.IV, np.uint32)


def _rotr(x: np.ndarray, n: int) -> np.ndarray:
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _g(s: list, a: int, b: int, c: int, d: int, mx: np.ndarray, my: np.ndarray) -> None:
    s[a] = s[a] + s[b] + mx
    s[d] = _rotr(s[d] ^ s[a], 16)
    s[c] = s[c] + s[d]
    s[b] = _rotr(s[b] ^ s[c], 12)
    s[a] = s[a] + s[b] + my
    s[d] = _rotr(s[d] ^ s[a], 8)
    s[c] = s[c] + s[d]
    s[b] = _rotr(s[b] ^ s[c], 7)


def _parent_cvs(blocks: np.ndarray, flags: int) -> np.ndarray:
    """uint32 [p, 16] (left CV || right CV) -> uint32 [p, 8]: compress(IV, block, 0, 64, flags)[:8]"""
    p = len(blocks)
    m = [np.ascontiguousarray(blocks[:, i]) for i in range(16)]
    s = [np.full(p, v, np.uint32) for v in b3.IV] + [np.full(p, v, np.uint32) for v in b3.IV[:4]]
    s += [np.zeros(p, np.uint32), np.zeros(p, np.uint32), np.full(p, b3.BLOCK_LEN, np.uint32), np.full(p, flags, np.uint32)]
    for r in range(7):
        _g(s, 0, 4, 8, 12, m[0], m[1])
        _g(s, 1, 5, 9, 13, m[2], m[3])
        _g(s, 2, 6, 10, 14, m[4], m[5])
        _g(s, 3, 7, 11, 15, m[6], m[7])
        _g(s, 0, 5, 10, 15, m[8], m[9])
        _g(s, 1, 6, 11, 12, m[10], m[11])
        _g(s, 2, 7, 8, 13, m[12], m[13])
        _g(s, 3, 4, 9, 14, m[14], m[15])
        if r != 6:
            m = [m[b3.MSG_PERMUTATION[i]] for i in range(16)]
    return np.stack([s[i] ^ s[i + 8] for i in range(8)], axis=1)


def np_parents(level: np.ndarray, root: bool = False) -> np.ndarray:
    """one level up: uint32 [n, 8] -> uint32 [ceil(n / 2), 8], the odd node carried up; ROOT (if
    asked) when the level has two nodes"""
    level = np.ascontiguousarray(level, np.uint32).reshape(-1, 8)
    n = len(level)
    assert n >= 2
    up = _parent_cvs(level[:n - (n & 1)].reshape(-1, 16), b3.PARENT | (b3.ROOT if root and n == 2 else 0))
    return np.concatenate([up, level[n - 1:]]) if n & 1 else up


def np_root(cvs, root: bool = True) -> bytes:
    """the top of the parent tree over CVs uint8 [n, 32] (or uint32 [n, 8]); one CV is its own top"""
    cvs = np.ascontiguousarray(cvs)
    level = (cvs.reshape(-1).view(np.uint8).view("<u4") if cvs.dtype == np.uint8 else cvs).astype(np.uint32).reshape(-1, 8)
    while len(level) > 1:
        level = np_parents(level, root)
    return level[0].astype("<u4").tobytes()


# ------------------------------------------------------------------------------- the reduce cases
def passes(c: int) -> int:
    """reduce passes of a message of c CVs: how often c -> ceil(c / 256) until 1"""
    k = 0
    while c > 1:
        c, k = -(-c // 256), k + 1
    return k


# 65 792 -> 257 -> 2; 65 793 -> 258, its last level-0 group holds one CV
REDUCE_COUNTS = (65_535, 65_536, 65_537, 65_792, 65_793, 131_071, 131_073, 196_609)
assert len(REDUCE_COUNTS) == 8 and [passes(c) for c in REDUCE_COUNTS] == [2, 2, 3, 3, 3, 3, 3, 3]
assert -(-65_537 // 256) == 257 and 65_537 % 256 == 1 and 257 % 256 == 1  # a count-1 group on levels 0 and 1
assert -(-65_792 // 256) == 257 and -(-65_793 // 256) == 258 and 65_793 % 256 == 1

# files that finish at passes 0, 1, 2 and 3, interleaved
MIXED_COUNTS = (1, 65_537, 2, 257, 65_536, 256, 65_793, 131_073, 3, 196_609, 258)
assert len(MIXED_COUNTS) == 11 and [passes(c) for c in MIXED_COUNTS] == [0, 3, 1, 2, 2, 1, 3, 3, 1, 3, 2]
assert sum(passes(c) == 3 for c in MIXED_COUNTS) >= 4 and sum(passes(c) == 3 for c in REDUCE_COUNTS) >= 4
KS = (17, 20)


def random_cvs(count: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (count, 32), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def reduce_case(count: int) -> tuple:
    """(CVs uint8 [count, 32], total_len, the root np_root gives): computed once, shared, read-only"""
    cvs = random_cvs(count, 7000 + count)
    cvs.setflags(write=False)
    total = count * MIB - 3
    assert split_arith(total, 1, 0) == (count, 0, total, count * 32)
    return cvs, total, np_root(cvs)


class MixedBatch:
    """the mixed batch for the tree roots at block size 2^k: file i has counts[i] nodes; no bytes"""

    def __init__(self, k: int, counts=MIXED_COUNTS):
        self.k, self.counts = k, tuple(counts)
        self.lens = np.array([c << k for c in counts], np.uint64) - np.uint64(3)
        assert all(max(1, -(-int(x) // (1 << k))) == c for x, c in zip(self.lens, counts))
        starts = np.concatenate([[0], np.cumsum((self.lens + np.uint64(64 + 127)) // np.uint64(128) * np.uint64(128))])
        self.offsets = starts[:-1].astype(np.uint64)  # only the plan sees them
        self.node_base = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        self.total = int(self.node_base[-1])
        self.n = len(counts)

    def nodes(self) -> np.ndarray:
        """uint8 [total, 32]: file i's level is mixed_level(counts[i]), whatever the order"""
        return np.concatenate([mixed_level(c)[0] for c in self.counts])

    def roots(self) -> np.ndarray:
        return np.frombuffer(b"".join(mixed_level(c)[1] for c in self.counts), np.uint8).reshape(-1, 32)


@functools.lru_cache(maxsize=None)
def mixed_level(count: int) -> tuple:
    """(random nodes uint8 [count, 32], their root): a one-node file's root is its node"""
    nodes = random_cvs(count, 9000 + count)
    nodes.setflags(write=False)
    root = np_root(nodes)
    assert count > 1 or root == nodes[0].tobytes()
    return nodes, root
