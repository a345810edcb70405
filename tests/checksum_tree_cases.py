"""The checksum trees' reference and cases (include/sd_cas.h, checksum trees), shared by
tests/test_checksum_tree.py (the CPU twins) and tests/test_gpu_checksum_tree.py (the kernels).

The reference is a restatement of the definitions over oracle/blake3_spec.py's chunk_cv and
compress, never the code under test:
  spec_nodes(data, k)   the level N_0 .. N_{nb-1} of a file at B = 2^k bytes
  spec_root(nodes)      the root of a level
The pure-Python spec hashes ~0.65 MB/s, so only a file set of at most DIRECT_BYTES per k is
compared node by node; every larger file is held to the root identity -- spec_root(the level under
test) == the oracle's BLAKE3 of the data, which a wrong, missing or misplaced node breaks, at nb
Python compressions -- and to the position rule.
"""
import functools
import struct

import numpy as np

from oracle import blake3_spec as b3
from oracle import native

KS = (17, 18, 19, 20)
MIB = 1 << 20
DIRECT_BYTES = 1_250_000  # ~1.2 MiB of pure-Python hashing per k


def _parent(left, right, root: bool) -> list:
    return b3.compress(b3.IV, list(left) + list(right), 0, b3.BLOCK_LEN, b3.PARENT | (b3.ROOT if root else 0))[:8]


def _merge(level, root: bool) -> list:
    """level-wise pairwise merge, the odd node carried up, ROOT (if asked) on the last parent"""
    level = list(level)
    while len(level) > 1:
        last = len(level) == 2
        nxt = [_parent(level[i], level[i + 1], root and last) for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def _pack(cv) -> bytes:
    return struct.pack("<8I", *cv)


def spec_nodes(data: bytes, k: int) -> np.ndarray:
    """uint8 [nb, 32]: the definitions, chunk by chunk"""
    B = 1 << k
    n = len(data)
    nb = max(1, -(-n // B))
    if nb == 1:  # the file's root hash itself
        nch = max(1, -(-n // b3.CHUNK_LEN))
        if nch == 1:
            return np.frombuffer(_pack(b3.chunk_cv(data, 0, True)), np.uint8).reshape(1, 32)
        cvs = [b3.chunk_cv(data[c * 1024:(c + 1) * 1024], c, False) for c in range(nch)]
        return np.frombuffer(_pack(_merge(cvs, True)), np.uint8).reshape(1, 32)
    out = []
    for j in range(nb):
        blk = data[j * B:(j + 1) * B]
        c0 = j * B // 1024
        cvs = [b3.chunk_cv(blk[c * 1024:(c + 1) * 1024], c0 + c, False) for c in range(-(-len(blk) // 1024))]
        out.append(_pack(_merge(cvs, False)))
    return np.frombuffer(b"".join(out), np.uint8).reshape(nb, 32)


def spec_root(nodes) -> bytes:
    """the root of a level uint8 [nb, 32]"""
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32)
    if len(nodes) == 1:
        return nodes[0].tobytes()
    return _pack(_merge([struct.unpack("<8I", r.tobytes()) for r in nodes], True))


def nodes_of(length: int, k: int) -> int:
    return max(1, -(-length // (1 << k)))


def shapes(k: int) -> list:
    """the smallest lengths at which the level can go wrong (the issue's list), in batch order"""
    B = 1 << k
    ls = [0, 1, 1024, 4096, 4097,            # the in-lane root boundary
          B - 1, B, B + 1,                   # nb 1 -> 2: the node turns from root to CV
          MIB - 1, MIB, MIB + 1,             # one leaf block -> two; nodes under a top that takes ROOT
          MIB + B + 1,                       # a second leaf block of one full and one partial node
          2 * MIB + 1,                       # both blocks of a workgroup from one file, and a third
          3 * MIB + 5 * (128 << 10) + 77]
    if k == 17:
        ls.append(32 * MIB + (128 << 10) + 1)  # 258 nodes: _roots takes a second reduce pass
    return ls


class Batch:
    """files laid out in one host buffer: starts on 128-byte lines, one of them 16 bytes past a
    line; the buffer zero to 64 bytes past the last file"""

    def __init__(self, lens, k: int, seed: int = 1000, odd_start: int = None):
        self.k = k
        self.lens = np.array(lens, np.uint64)
        n = len(lens)
        offs, cur = [], 0
        for i, length in enumerate(lens):
            if i == odd_start:
                cur += 16
            offs.append(cur)
            cur = (cur + length + 64 + 127) // 128 * 128
        self.offsets = np.array(offs, np.uint64)
        self.data = np.zeros(cur + 64, np.uint8)
        for i, (o, length) in enumerate(zip(offs, lens)):
            if length:
                self.data[o:o + length] = np.frombuffer(native.synth_bytes(seed + i, 0, 0, length), np.uint8)
        self.nb = np.array([nodes_of(int(x), k) for x in lens], np.uint64)
        self.node_base = np.concatenate([[0], np.cumsum(self.nb)]).astype(np.uint64)
        self.total = int(self.node_base[n])
        self.n = n

    def file(self, i: int) -> bytes:
        o, length = int(self.offsets[i]), int(self.lens[i])
        return self.data[o:o + length].tobytes()

    def level(self, nodes, i: int) -> np.ndarray:
        return np.asarray(nodes).reshape(-1, 32)[int(self.node_base[i]):int(self.node_base[i + 1])]

    def leaf_blocks(self) -> int:
        return int(sum(max(1, -(-int(x) // MIB)) for x in self.lens))

    @functools.cached_property
    def checksums(self) -> np.ndarray:
        """the oracle's BLAKE3 per file, uint8 [n, 32]"""
        return native.checksums(self.data, self.offsets, self.lens, nthreads=8)

    def truncated(self) -> "Batch":
        """the position rule's twin: every file of more than 2 B + 7 bytes cut by B + 7 bytes (so
        it keeps at least two blocks), with the same bytes"""
        B = 1 << self.k
        keep = [i for i in range(self.n) if int(self.lens[i]) - B - 7 > B]
        t = Batch([int(self.lens[i]) - B - 7 for i in keep], self.k)
        for j, i in enumerate(keep):
            o, length = int(t.offsets[j]), int(t.lens[j])
            t.data[o:o + length] = self.data[int(self.offsets[i]):int(self.offsets[i]) + length]
        t.source = keep
        return t


@functools.lru_cache(maxsize=None)
def shape_batch(k: int) -> Batch:
    """every shape in one batch: neighbouring leaf blocks of different files share a workgroup,
    the leaf blocks are odd in number (the last workgroup is half empty) and the 2 MiB + 1 file
    starts 16 bytes past a 128-byte line"""
    ls = shapes(k)
    b = Batch(ls, k, odd_start=ls.index(2 * MIB + 1))
    if b.leaf_blocks() % 2 == 0:
        b = Batch(ls + [5], k, odd_start=ls.index(2 * MIB + 1))
    assert b.leaf_blocks() % 2 == 1 and int(b.offsets[ls.index(2 * MIB + 1)]) % 128 == 16
    return b


@functools.lru_cache(maxsize=None)
def truncated_batch(k: int) -> Batch:
    return shape_batch(k).truncated()


@functools.lru_cache(maxsize=None)
def direct_levels(k: int) -> dict:
    """{file index: spec_nodes} for the files compared node by node: the tiny ones, then B + 1, B,
    B - 1 (a two-node file first) while DIRECT_BYTES lasts"""
    b = shape_batch(k)
    B = 1 << k
    ls = [int(x) for x in b.lens]
    order = [i for i, x in enumerate(ls) if x <= 4097] + [ls.index(B + 1), ls.index(B), ls.index(B - 1)]
    out, spent = {}, 0
    for i in order:
        if i in out or spent + ls[i] > DIRECT_BYTES:
            continue
        out[i] = spec_nodes(b.file(i), k)
        spent += ls[i]
    return out


def check_levels(b: Batch, nodes, roots, direct: dict = None, what="") -> None:
    """a level buffer and the roots against the reference: node by node where `direct` has the
    file, the root identity for every file, the roots bit-exact against the oracle"""
    nodes = np.asarray(nodes, np.uint8).reshape(-1, 32)
    roots = np.asarray(roots, np.uint8).reshape(-1, 32)
    assert len(nodes) == b.total and len(roots) == b.n, (what, len(nodes), b.total)
    for i in range(b.n):
        lvl = b.level(nodes, i)
        tag = (what, b.k, i, int(b.lens[i]))
        if direct and i in direct:
            assert np.array_equal(lvl, direct[i]), tag
        assert spec_root(lvl) == b.checksums[i].tobytes(), tag
        assert roots[i].tobytes() == b.checksums[i].tobytes(), tag


def check_position_rule(b: Batch, nodes, t: Batch, t_nodes, what="") -> None:
    """the nodes of the full blocks of data[:len - B - 7] equal those of data"""
    B = 1 << b.k
    for j, i in enumerate(t.source):
        full = int(t.lens[j]) // B
        assert full >= 1
        assert np.array_equal(t.level(t_nodes, j)[:full], b.level(nodes, i)[:full]), (what, b.k, i)


def flips(b: Batch) -> tuple:
    """(byte positions in b.data to flip, the expected (file, block) rows ascending, the expected
    stats): the first byte of a middle block, the last byte of a file, a byte of a partial last
    block, a byte of a one-block file"""
    B = 1 << b.k
    ls = [int(x) for x in b.lens]
    big, two, one = ls.index(3 * MIB + 5 * (128 << 10) + 77), ls.index(2 * MIB + 1), ls.index(4097)
    mid = int(b.nb[big]) // 2
    cases = [(big, mid * B), (two, ls[two] - 1), (big, ls[big] - 40), (one, 100)]
    assert (ls[big] - 40) // B == int(b.nb[big]) - 1 and ls[big] % B and mid not in (0, int(b.nb[big]) - 1)
    pos = [int(b.offsets[f]) + at for f, at in cases]
    rows = sorted({(f, at // B) for f, at in cases})
    stats = [b.n, b.total, len(rows), len({f for f, _ in rows})]
    return pos, np.array(rows, np.uint64).reshape(-1, 2), np.array(stats, np.uint64)


def flipped(b: Batch) -> np.ndarray:
    d = b.data.copy()
    for p in flips(b)[0]:
        d[p] ^= 0x01
    return d
