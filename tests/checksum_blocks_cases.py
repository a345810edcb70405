"""Listed blocks (include/sd_cas.h, checksum trees, listed blocks): the cases and their references,
shared by tests/test_checksum_blocks.py (the CPU twins) and tests/test_gpu_checksum_blocks.py (the
kernel).  No library call in here: numpy, the oracle, and the pure-Python spec.

The references, never the code under test:
  tc.spec_nodes / hc.spec_block_cv   a listed block's node, chunk by chunk
  tc.spec_root + the oracle's BLAKE3 the root identity: the level a list's nodes form, put back in
                                     block order, has the file's checksum as its root
The pure-Python spec hashes ~0.65 MB/s: the nodes compared directly stay inside tc.DIRECT_BYTES per k
(asserted below); every other node is held to the root identity.
"""
import functools

import numpy as np

from oracle import native
from tests import checksum_tree_cases as tc
from tests import high_counter_cases as hc

KS = tc.KS
JUNK = 0xA5


def shape_lens(k: int) -> list:
    B = 1 << k
    return [0, 1, 1024, 1025, 4096, 4097, B - 1, B, B + 1, B + 4097, 3 * B + 5 * 4096 + 77]


def block_len(length: int, j: int, k: int) -> int:
    B = 1 << k
    return 0 if length == 0 else min(B, length - j * B)


class BlockList:
    """rows (file, block) of files of lengths `lens`, each row's bytes somewhere in `data`: the
    starts on 128-byte lines in a shuffled order of their own, row `odd` 16 bytes past a line, and
    everything that is not a block's byte 0xA5 -- the gap after a block's last byte is junk"""

    def __init__(self, lens, k: int, rows, blocks: dict, seed: int = 1, odd: int = 0):
        self.k = k
        self.lens = np.array(lens, np.uint64)
        self.n = len(lens)
        self.rows = np.array(rows, np.uint64).reshape(-1, 2)
        self.m = len(self.rows)
        self.nb = np.array([tc.nodes_of(int(x), k) for x in lens], np.uint64)
        self.node_base = np.concatenate([[0], np.cumsum(self.nb)]).astype(np.uint64)
        self.total = int(self.node_base[-1])
        self.sizes = [block_len(int(lens[int(f)]), int(j), k) for f, j in self.rows]
        self.offsets = np.zeros(self.m, np.uint64)
        cur = 0
        for r in np.random.default_rng(seed).permutation(self.m):
            if r == odd:
                cur += 16
            self.offsets[r] = cur
            cur = (cur + self.sizes[r] + 64 + 127) // 128 * 128
        self.data = np.full(cur + 64, JUNK, np.uint8)
        for r, (f, j) in enumerate(self.rows):
            blk = blocks[(int(f), int(j))]
            assert len(blk) == self.sizes[r]
            self.data[int(self.offsets[r]):int(self.offsets[r]) + len(blk)] = np.frombuffer(blk, np.uint8)

    def slot(self, r: int) -> int:
        return int(self.node_base[int(self.rows[r, 0])]) + int(self.rows[r, 1])

    def slots(self) -> np.ndarray:
        return np.array([self.slot(r) for r in range(self.m)], np.int64)

    def prefix(self, m: int) -> "BlockList":
        """the first m rows over the same buffer"""
        p = object.__new__(BlockList)
        p.__dict__.update(self.__dict__)
        p.rows, p.offsets, p.sizes, p.m = self.rows[:m], self.offsets[:m], self.sizes[:m], m
        return p

    def without(self, drop) -> "BlockList":
        """the list without the rows in `drop`, over the same buffer"""
        keep = [r for r in range(self.m) if r not in set(drop)]
        p = object.__new__(BlockList)
        p.__dict__.update(self.__dict__)
        p.rows, p.offsets, p.sizes, p.m = self.rows[keep], self.offsets[keep], [self.sizes[r] for r in keep], len(keep)
        return p

    def wave_count(self) -> int:
        """waves of the launch: 512-lane workgroups of 512 >> (k - 12) items"""
        per_wg = 512 >> (self.k - 12)
        return 8 * -(-self.m // per_wg)


def blocks_of(b: tc.Batch) -> dict:
    """{(file, block): bytes} of every block of a batch's files"""
    B = 1 << b.k
    out = {}
    for i in range(b.n):
        data = b.file(i)
        for j in range(int(b.nb[i])):
            out[(i, j)] = data[j * B:(j + 1) * B]
    return out


def every_row(b: tc.Batch, seed: int) -> np.ndarray:
    """every block of every file, in a fixed shuffled order"""
    rows = np.array([(i, j) for i in range(b.n) for j in range(int(b.nb[i]))], np.uint64)
    return rows[np.random.default_rng(seed).permutation(len(rows))]


@functools.lru_cache(maxsize=None)
def shape_batch(k: int) -> tc.Batch:
    """the shape files laid out contiguously: what sd_checksum_tree_run and the oracle hash"""
    return tc.Batch(shape_lens(k), k, seed=2000)


@functools.lru_cache(maxsize=None)
def shape_list(k: int) -> BlockList:
    b = shape_batch(k)
    rows = every_row(b, 77 + k)
    bl = BlockList(shape_lens(k), k, rows, blocks_of(b), seed=78 + k, odd=3)
    assert int(bl.offsets[3]) % 128 == 16 and all(int(o) % 128 == 0 for r, o in enumerate(bl.offsets) if r != 3)
    assert bl.m == b.total and sorted(bl.slots()) == list(range(b.total))
    return bl


def high_counter_files(k: int) -> list:
    """[(length, [blocks])]: a 4097-byte block at counter exactly 2^32, and at k = 17 the blocks
    either side of it"""
    out = [((1 << 42) + 4097, [1 << (42 - k)])]
    if k == 17:
        B = 1 << 17
        out.append(((1 << 42) + B + 5, [(1 << 25) - 1, 1 << 25, (1 << 25) + 1]))
    return out


@functools.lru_cache(maxsize=None)
def high_list(k: int) -> BlockList:
    """only the listed blocks of the multi-TiB files are resident"""
    lens, rows, blocks = [], [], {}
    for f, (length, js) in enumerate(high_counter_files(k)):
        lens.append(length)
        for q, j in enumerate(js):
            rows.append((f, j))
            blocks[(f, j)] = native.synth_bytes(3000 + 10 * f + q, 0, 0, block_len(length, j, k))
    return BlockList(lens, k, rows, blocks, seed=5 + k, odd=0)


@functools.lru_cache(maxsize=None)
def high_expected(k: int) -> np.ndarray:
    """spec_block_cv per row of high_list(k); a counter cut to 32 bits gives another value"""
    bl = high_list(k)
    out = []
    for r, (f, j) in enumerate(bl.rows):
        o = int(bl.offsets[r])
        data = bl.data[o:o + bl.sizes[r]].tobytes()
        c0 = int(j) * ((1 << k) // 1024)
        want = hc.spec_block_cv(data, c0)
        if c0 + -(-len(data) // 1024) > 1 << 32:  # some chunk has a counter >= 2^32
            assert want != hc.spec_block_cv(data, c0, 0xFFFFFFFF)
        out.append(np.frombuffer(want, np.uint8))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def direct_nodes(k: int) -> dict:
    """{(file, block): the spec's 32 bytes} of shape_list(k): the files of at most 4097 bytes, both
    blocks of B + 1 (a full CV, then a 1-byte non-root chunk at counter B / 1024), the partial last
    block of the longest file (21 chunks).  With high_expected inside tc.DIRECT_BYTES."""
    b = shape_batch(k)
    B = 1 << k
    ls = shape_lens(k)
    out, spent = {}, 0
    for i, length in enumerate(ls):
        if length <= 4097 or length == B + 1:
            for j, node in enumerate(tc.spec_nodes(b.file(i), k)):
                out[(i, j)] = node.tobytes()
            spent += length
    big = len(ls) - 1
    j = int(b.nb[big]) - 1
    tail = b.file(big)[j * B:]
    assert len(tail) == 5 * 4096 + 77 and -(-len(tail) // 1024) == 21  # 21 chunks: the sixth lane holds one
    out[(big, j)] = hc.spec_block_cv(tail, j * B // 1024)
    spent += len(tail) + sum(high_list(k).sizes)
    assert spent <= tc.DIRECT_BYTES, (k, spent)
    return out


def level_of(bl: BlockList, nodes) -> np.ndarray:
    """a list's nodes (list order) put at their slots of the level layout; rows never listed stay 0"""
    nodes = np.asarray(nodes, np.uint8).reshape(-1, 32)
    assert len(nodes) == bl.m
    level = np.zeros((bl.total, 32), np.uint8)
    level[bl.slots()] = nodes
    return level


def check_list(bl: BlockList, nodes, b: tc.Batch, direct: dict = None, what="") -> None:
    """a full list's nodes against the reference: the direct rows bit for bit, every file's root
    identity against the oracle"""
    nodes = np.asarray(nodes, np.uint8).reshape(-1, 32)
    if direct:
        seen = 0
        for r, (f, j) in enumerate(bl.rows):
            want = direct.get((int(f), int(j)))
            if want is not None:
                assert nodes[r].tobytes() == want, (what, bl.k, int(f), int(j))
                seen += 1
        assert seen >= len(direct)
    level = level_of(bl, nodes)
    for i in range(b.n):
        assert tc.spec_root(b.level(level, i)) == b.checksums[i].tobytes(), (what, bl.k, i, int(b.lens[i]))


# ------------------------------------------------------------------------------------ packing
@functools.lru_cache(maxsize=None)
def packing_list(k: int) -> tuple:
    """(33 rows of small partial blocks -- the second blocks of files of B + 1 + i bytes, only those
    bytes resident, and six one-node files --, the spec's nodes [33, 32])"""
    B = 1 << k
    singles = [0, 5, 1024, 3000, 4097, 9000]
    lens = [B + 1 + i for i in range(27)] + singles
    rows, blocks, want = [], {}, []
    for f, length in enumerate(lens):
        j = 1 if length > B else 0
        data = native.synth_bytes(4000 + f, 0, 0, block_len(length, j, k))
        rows.append((f, j))
        blocks[(f, j)] = data
        want.append(np.frombuffer(hc.spec_block_cv(data, B // 1024), np.uint8) if j else tc.spec_nodes(data, k)[0])
    order = np.random.default_rng(11).permutation(33)
    bl = BlockList(lens, k, [rows[r] for r in order], blocks, seed=12, odd=1)
    return bl, np.stack([want[r] for r in order])


# ------------------------------------------------------------------------------------ windowed
def windowed_batch(rows_over: int) -> tc.Batch:
    """k = 17 files on the length pattern of test_windowed_and_unwindowed_instantiations with more
    than rows_over blocks between them"""
    B = 1 << 17
    pattern = [1, 1024, 4097, 20000, B + 1, 2 * B + 5, 3 * B - 1, B]
    lens, blocks, i = [], 0, 0
    while blocks <= rows_over:
        lens.append(pattern[i % len(pattern)] + i // len(pattern))
        blocks += tc.nodes_of(lens[-1], 17)
        i += 1
    return tc.Batch(lens, 17, seed=9100, odd_start=5)


# ------------------------------------------------------------------------------------ verify
def flip_cases(k: int) -> tuple:
    """((file, byte) flips of the shape files, the one among them whose block a second list omits):
    the first byte of a middle block, the last byte of a partial last block, a byte of a one-block
    file, and -- the omitted one -- a byte of another block"""
    B = 1 << k
    ls = shape_lens(k)
    big, two, one = len(ls) - 1, ls.index(B + 4097), ls.index(4097)
    listed = [(big, 2 * B), (big, ls[big] - 1), (one, 100)]
    unlisted = (two, B + 9)
    return listed, unlisted


def flipped_list(bl: BlockList, flips) -> np.ndarray:
    """bl.data with the byte `at` of file f flipped in every row that holds it"""
    B = 1 << bl.k
    d = bl.data.copy()
    for f, at in flips:
        for r, (rf, rj) in enumerate(bl.rows):
            if int(rf) == f and int(rj) == at // B:
                d[int(bl.offsets[r]) + at % B] ^= 0x01
    return d


def expected_verify(bl: BlockList, flips) -> tuple:
    """(bad uint8 [m], rows in list order, stats) of a list whose data holds `flips`"""
    B = 1 << bl.k
    hit = {(f, at // B) for f, at in flips}
    bad = np.array([1 if (int(f), int(j)) in hit else 0 for f, j in bl.rows], np.uint8)
    rows = bl.rows[bad != 0]
    stats = np.array([bl.n, bl.m, int(bad.sum()), len({int(f) for f, _ in rows})], np.uint64)
    return bad, rows, stats


# ------------------------------------------------------------------------------------ update
def update_case(k: int) -> tuple:
    """(byte changes (file, at) in three blocks, one of them a one-node file's; the rows to list)"""
    B = 1 << k
    ls = shape_lens(k)
    big, two, one = len(ls) - 1, ls.index(B + 1), ls.index(1025)
    changes = [(big, B + 5), (two, B), (one, 1024)]
    rows = [(f, at // B) for f, at in changes]
    return changes, rows


def changed_batch(k: int) -> tc.Batch:
    """shape_batch(k) with update_case's bytes changed: a copy, the shared batch stays as it is"""
    src = shape_batch(k)
    b = tc.Batch(shape_lens(k), k, seed=2000)
    assert np.array_equal(b.data, src.data)
    for f, at in update_case(k)[0]:
        b.data[int(b.offsets[f]) + at] ^= 0x40
    return b
