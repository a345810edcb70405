"""Range proofs (include/sd_cas.h, checksum trees, range proofs): the definitions restated over
tc._parent (oracle/blake3_spec.py's compress), and the cases shared by tests/test_checksum_ranges.py
(the CPU twins) and tests/test_gpu_checksum_ranges.py (the kernels).  No call of the code under test:
  range_entries(nb, a, b)               the closed form of a range proof's entry count
  spec_range_proof(levels, a, b)        the flanks of blocks [a, b), bottom-up, left before right
  spec_range_climb(nodes, proof, nb, a, b)  the root the range's nodes and a proof claim
  np_range_climb                        the same climb over hc.np_parents, for levels of 10^5 nodes
A proof certifies itself: the oracle for a proof under test is that the climb reaches a root that
came from elsewhere -- tc.spec_root / the numpy parent tree of a level of random nodes, or the
oracle's BLAKE3 of real bytes.
"""
import functools

import numpy as np

from tests import checksum_blocks_cases as bc
from tests import checksum_proofs_cases as pc
from tests import checksum_tree_cases as tc
from tests import high_counter_cases as hc

KS = pc.KS
height = pc.height


def range_entries(nb: int, a: int, b: int) -> int:
    """p: per level L < h, one for an odd lo = a >> L, one for an even hi = (b - 1) >> L with a node after it"""
    p, n = 0, nb
    for L in range(height(nb)):
        lo, hi = a >> L, (b - 1) >> L
        p += (lo & 1) + (hi % 2 == 0 and hi + 1 < n)
        n = -(-n // 2)
    return p


def _bytes(node) -> bytes:
    return node.astype("<u4").tobytes() if isinstance(node, np.ndarray) else tc._pack(node)


def spec_range_proof(levels: list, a: int, b: int) -> bytes:
    """levels: pc.spec_levels' or lc.np_levels' (the last one is the root)"""
    out = []
    for L in range(len(levels) - 1):
        lo, hi = a >> L, (b - 1) >> L
        if lo & 1:
            out.append(_bytes(levels[L][lo - 1]))
        if hi % 2 == 0 and hi + 1 < len(levels[L]):
            out.append(_bytes(levels[L][hi + 1]))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def _parent(left: tuple, right: tuple, root: bool) -> tuple:
    """every parent a valid climb forms is a node of the file's tree: the ranges of one file share them"""
    return tuple(tc._parent(left, right, root))


def spec_range_climb(nodes, proof: bytes, nb: int, a: int, b: int) -> bytes:
    """the root that N_a .. N_{b-1} (uint8 [b - a, 32]) and a proof claim for a file of nb nodes; the
    proof must be exactly range_entries(nb, a, b) entries long"""
    cur = [pc._cv(r) for r in np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32)]
    assert len(cur) == b - a
    n, at = nb, 0
    for L in range(height(nb)):
        lo, hi = a >> L, (b - 1) >> L
        assert len(cur) == hi - lo + 1
        if lo & 1:
            cur.insert(0, pc._cv(proof[at:at + 32]))
            at += 32
        if hi % 2 == 0 and hi + 1 < n:
            cur.append(pc._cv(proof[at:at + 32]))
            at += 32
        nxt = [_parent(cur[i], cur[i + 1], n == 2) for i in range(0, len(cur) - 1, 2)]
        if len(cur) & 1:  # the file's own carry: hi is its last node
            assert hi + 1 == n
            nxt.append(cur[-1])
        cur, n = nxt, -(-n // 2)
    assert at == len(proof) and len(cur) == 1, (at, len(proof), len(cur))
    return tc._pack(cur[0])


def np_range_climb(nodes, proof, nb: int, a: int, b: int) -> bytes:
    """spec_range_climb over hc.np_parents (uint32 rows), for ranges of 10^5 nodes"""
    as_u32 = lambda x: np.ascontiguousarray(x, np.uint8).reshape(-1).view("<u4").astype(np.uint32).reshape(-1, 8)  # noqa: E731
    cur, ent = as_u32(nodes), as_u32(np.frombuffer(bytes(proof), np.uint8))
    assert len(cur) == b - a
    n, at = nb, 0
    for L in range(height(nb)):
        lo, hi = a >> L, (b - 1) >> L
        if lo & 1:
            cur = np.concatenate([ent[at:at + 1], cur])
            at += 1
        if hi % 2 == 0 and hi + 1 < n:
            cur = np.concatenate([cur, ent[at:at + 1]])
            at += 1
        assert len(cur) & 1 == 0 or hi + 1 == n
        cur = hc.np_parents(cur, n == 2) if len(cur) > 1 else cur  # one node: the file's carry
        n = -(-n // 2)
    assert at == len(ent) and len(cur) == 1
    return cur[0].astype("<u4").tobytes()


# ------------------------------------------------------------------------------------ lists of ranges
class RangeList:
    """ranges [(file, a, b)] of files of `lens` as one block list: rows (f, a) .. (f, b - 1) range
    after range, range_base their prefix sum; offsets[r] (optional) from `place(f, j)`"""

    def __init__(self, lens, k: int, ranges, place=None):
        self.k, self.lens, self.ranges = k, np.array(lens, np.uint64), [(int(f), int(a), int(b)) for f, a, b in ranges]
        self.n, self.q = len(lens), len(self.ranges)
        self.nb = [tc.nodes_of(int(x), k) for x in lens]
        self.node_base = np.concatenate([[0], np.cumsum(self.nb)]).astype(np.int64)
        self.range_base = np.concatenate([[0], np.cumsum([b - a for _, a, b in self.ranges])]).astype(np.uint64)
        self.m = int(self.range_base[-1])
        self.rows = np.zeros((self.m, 2), np.uint64)
        for i, (f, a, b) in enumerate(self.ranges):
            r0 = int(self.range_base[i])
            self.rows[r0:r0 + b - a, 0] = f
            self.rows[r0:r0 + b - a, 1] = np.arange(a, b, dtype=np.uint64)
        self.offsets = np.zeros(self.m, np.uint64)
        if place:
            self.offsets = np.array([place(int(f), int(j)) for f, j in self.rows], np.uint64)
        self.proof_base = np.concatenate(
            [[0], np.cumsum([range_entries(self.nb[f], a, b) for f, a, b in self.ranges])]).astype(np.uint64)

    def slots(self) -> np.ndarray:
        return self.node_base[self.rows[:, 0].astype(np.int64)] + self.rows[:, 1].astype(np.int64)

    def expected(self, bad_ranges) -> tuple:
        """(flags uint8 [q], rows uint64 [count, 3], stats) when exactly `bad_ranges` fail"""
        bad = np.zeros(self.q, np.uint8)
        bad[list(bad_ranges)] = 1
        rows = np.array([(f, a, b - a) for i, (f, a, b) in enumerate(self.ranges) if bad[i]], np.uint64).reshape(-1, 3)
        stats = np.array([self.n, self.q, int(bad.sum()), len({int(f) for f in rows[:, 0]})], np.uint64)
        return bad, rows, stats


def every_range(nb: int) -> list:
    return [(a, b) for a in range(nb) for b in range(a + 1, nb + 1)]


def spec_proofs(rl: RangeList, level, levels_of) -> np.ndarray:
    """the packed spec proofs uint8 [entries, 32] of a list; levels_of(file's nodes) -> its levels"""
    level = np.asarray(level, np.uint8).reshape(-1, 32)
    lv = {f: levels_of(level[rl.node_base[f]:rl.node_base[f + 1]]) for f in sorted({f for f, _, _ in rl.ranges})}
    out = b"".join(spec_range_proof(lv[f], a, b) for f, a, b in rl.ranges)
    assert len(out) == 32 * int(rl.proof_base[-1])
    return np.frombuffer(out, np.uint8).reshape(-1, 32)


def check_range_proofs(rl: RangeList, level, proofs, roots, climb=spec_range_climb, what="") -> None:
    """every range's proof (packed by the closed form) climbs from the range's nodes of `level` to roots[f]"""
    level = np.asarray(level, np.uint8).reshape(-1, 32)
    proofs = np.asarray(proofs, np.uint8).reshape(-1, 32)
    assert len(proofs) == int(rl.proof_base[-1]), (what, len(proofs), int(rl.proof_base[-1]))
    for i, (f, a, b) in enumerate(rl.ranges):
        o = int(rl.node_base[f])
        got = climb(level[o + a:o + b], proofs[int(rl.proof_base[i]):int(rl.proof_base[i + 1])].tobytes(), rl.nb[f], a, b)
        assert got == bytes(roots[f]), (what, rl.k, i, f, a, b)


# ------------------------------------------------------------------------------------ random levels
SMALL_K = 17
SMALL_NBS = tuple(range(1, 34))


@functools.lru_cache(maxsize=None)
def small_case() -> tuple:
    """(RangeList of every (a, b) of every nb <= 33, the level layout of random nodes, [root per file])"""
    lens = [nb << SMALL_K for nb in SMALL_NBS]
    rl = RangeList(lens, SMALL_K, [(f, a, b) for f, nb in enumerate(SMALL_NBS) for a, b in every_range(nb)])
    level = np.random.default_rng(5150).integers(0, 256, (sum(SMALL_NBS), 32), dtype=np.uint8)
    roots = [tc.spec_root(level[rl.node_base[f]:rl.node_base[f + 1]]) for f in range(rl.n)]
    return rl, level, roots


GROUP_NBS = (255, 256, 257, 511, 513)   # a short group, a full one, full + 1, two groups less one, two plus one
DEEP_NBS = (65_537, 131_073)            # three passes


def boundary_ranges(nb: int) -> list:
    out = [(0, nb), (1, nb), (0, nb - 1), (1, nb - 1), (255, 257), (256, 512), (254, 256)]
    if nb in DEEP_NBS:
        out += [(65_535, 65_537), (nb - 1, nb)]
    return [(a, b) for a, b in out if a < b <= nb]


@functools.lru_cache(maxsize=None)
def boundary_case(nbs: tuple, seed: int) -> tuple:
    """(RangeList of boundary_ranges of each nb with an unlisted file of garbage between them, the
    level of random nodes, [numpy root per file])"""
    files = list(nbs[:1]) + [300] + list(nbs[1:])
    lens = [nb << SMALL_K for nb in files]
    rl = RangeList(lens, SMALL_K, [(f, a, b) for f, nb in enumerate(files) if f != 1 for a, b in boundary_ranges(nb)])
    level = np.random.default_rng(seed).integers(0, 256, (sum(files), 32), dtype=np.uint8)
    level[rl.node_base[1]:rl.node_base[2]] = 0x5A
    roots = [hc.np_root(level[rl.node_base[f]:rl.node_base[f + 1]]) for f in range(rl.n)]
    return rl, level, roots


# ------------------------------------------------------------------------------------ real bytes
@functools.lru_cache(maxsize=None)
def real_ranges(k: int) -> RangeList:
    """every range of every file of pc.real_batch(k) in one list; the rows of different ranges point
    at the same bytes, so the buffer is the batch's own"""
    b = pc.real_batch(k)
    B = 1 << k
    return RangeList(pc.real_lens(k), k, [(f, lo, hi) for f in range(b.n) for lo, hi in every_range(int(b.nb[f]))],
                     place=lambda f, j: int(b.offsets[f]) + j * B)


def range_of(rl: RangeList, f: int, a: int, b: int) -> int:
    return rl.ranges.index((f, a, b))


def mutations(rl: RangeList, data, proofs, level) -> list:
    """[(name, data, proofs, the ranges that must be flagged)] over real_ranges(k): files 6 (nb = 8)
    and 7 (nb = 9, a 1-byte trailing block); `level` is the batch's level layout"""
    k, B = rl.k, 1 << rl.k
    b = pc.real_batch(k)
    proofs = np.asarray(proofs, np.uint8).reshape(-1, 32)
    base = rl.proof_base
    out = []
    holds = lambda f, j: [i for i, (rf, lo, hi) in enumerate(rl.ranges) if rf == f and lo <= j < hi]  # noqa: E731
    # one byte of a middle block: every range of the file that holds the block
    d = data.copy()
    d[int(b.offsets[6]) + 3 * B + 70000] ^= 0x10
    out.append(("middle byte", d, proofs, holds(6, 3)))
    # the 1-byte trailing block
    d = data.copy()
    d[int(b.offsets[7]) + 8 * B] ^= 0x01
    out.append(("trailing byte", d, proofs, holds(7, 8)))
    # one bit of one proof entry
    i = range_of(rl, 7, 2, 5)
    assert int(base[i + 1] - base[i]) >= 2
    p = proofs.copy()
    p[int(base[i]) + 1, 9] ^= 0x01
    out.append(("proof bit", data, p, [i]))
    # the left and right entries of a level swapped: [3, 5) of nb = 8 has both at level 0
    i = range_of(rl, 6, 3, 5)
    p = proofs.copy()
    p[int(base[i])], p[int(base[i]) + 1] = proofs[int(base[i]) + 1], proofs[int(base[i])]
    out.append(("flanks swapped", data, p, [i]))
    # the proof of the same (a, b) for a file one block longer: [2, 9) of nb = 9 carries block 8 up,
    # at nb = 10 block 8 has a right sibling, whose entry comes first.  The receiver lays proofs out
    # by ITS length, so it reads the first entries of the longer proof.
    i = range_of(rl, 7, 2, 9)
    mine = int(base[i + 1] - base[i])
    nodes10 = np.concatenate([np.asarray(level, np.uint8).reshape(-1, 32)[rl.node_base[7]:rl.node_base[8]],
                              np.full((1, 32), 0x3C, np.uint8)])
    lp = np.frombuffer(spec_range_proof(pc.spec_levels(nodes10), 2, 9), np.uint8).reshape(-1, 32)
    assert len(lp) == range_entries(10, 2, 9) == mine + 1 and not np.array_equal(lp[:mine], proofs[int(base[i]):int(base[i + 1])])
    p = proofs.copy()
    p[int(base[i]):int(base[i + 1])] = lp[:mine]
    out.append(("longer file", data, p, [i]))
    return out


# ------------------------------------------------------------------------------------ the spliced level
SPLICE_K = 17
SPLICE_NB = 65_537 + 1000
SPLICE_RANGES = ((250, 770), (255, 257), (SPLICE_NB - 1, SPLICE_NB))


@functools.lru_cache(maxsize=None)
def splice_case() -> tuple:
    """one k = 17 file of 66 537 blocks' worth of LEVEL: random nodes with the oracle's nodes of real
    bytes spliced in at [250, 770) (68 MB: groups 0 .. 3 of pass 0, three passes), which holds [255,
    257), and at the last block (1 byte).  -> (RangeList whose rows point into `data`, data, the
    level, the numpy root)"""
    from oracle import native
    B = 1 << SPLICE_K
    length = (SPLICE_NB - 1) * B + 1
    assert tc.nodes_of(length, SPLICE_K) == SPLICE_NB
    run = np.frombuffer(native.synth_bytes(8100, 0, 0, 520 * B), np.uint8)
    data = np.concatenate([run, np.full(64, bc.JUNK, np.uint8), np.array([0x37], np.uint8), np.full(127, bc.JUNK, np.uint8)])
    last_off = 520 * B + 64
    place = lambda f, j: last_off if j == SPLICE_NB - 1 else (j - 250) * B  # noqa: E731
    rl = RangeList([length], SPLICE_K, [(0, a, b) for a, b in SPLICE_RANGES], place=place)
    level = np.random.default_rng(8101).integers(0, 256, (SPLICE_NB, 32), dtype=np.uint8)
    for j in range(250, 770):
        level[j] = np.frombuffer(native.subtree_cv(run[(j - 250) * B:(j - 249) * B], j * B // 1024), np.uint8)
    level[SPLICE_NB - 1] = np.frombuffer(native.subtree_cv(data[last_off:last_off + 1], (SPLICE_NB - 1) * B // 1024), np.uint8)
    return rl, data, level, hc.np_root(level)

