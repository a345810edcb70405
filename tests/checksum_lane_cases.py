"""Every lane count of a tree node and every proof shape (include/sd_cas.h, checksum trees): the
cases and their references, shared by tests/test_checksum_lanes.py (the CPU twins) and
tests/test_gpu_checksum_lanes.py (k_ck_blocks, k_ck_leaf_tree, k_tree_levels, k_tree_proof_gather,
proof_climb).  No library call in here: numpy, the oracle, hc.np_parents and the pure-Python spec.

A node of 2^k bytes is an LDS tree over 2^(k-12) lanes of 4 chunks, level-wise with the odd node
carried up and ROOT on the level of two nodes.  The lane sweep runs every lane count of that tree
with every fill of the last lane, as a root (a one-node file) and as a plain CV at a counter > 0.

The references, never the code under test, and fast enough for every node of every case:
  native.checksums          the oracle's BLAKE3: a one-node file's node, every file's root
  native.subtree_cv         the oracle's non-root CV of a block at a 64-bit counter; held to the
                            pure-Python spec in tests/test_high_counter.py and, for chunk counts that
                            are no power of two, by anchor() below
  np_levels / np_proof      every level of a file from hc.np_parents, and the siblings of a row
"""
import functools

import numpy as np

from oracle import native
from tests import checksum_blocks_cases as bc
from tests import checksum_proofs_cases as pc
from tests import checksum_tree_cases as tc
from tests import high_counter_cases as hc

KS = tc.KS
JUNK = bc.JUNK
LANE_CHUNKS = 4
TAILS = (1, 64, 65, 1023, 1024)  # the last chunk's bytes, rotating by the chunk count


def lanes_of(length: int) -> int:
    return -(-(-(-length // 1024)) // LANE_CHUNKS)


def last_fill(length: int) -> int:
    """the chunks in the last lane"""
    return -(-length // 1024) - LANE_CHUNKS * (lanes_of(length) - 1)


@functools.lru_cache(maxsize=None)
def lane_items(k: int) -> tuple:
    """item lengths 1024 (C - 1) + r: at k = 17 every chunk count C = 1 .. 128; at k = 18, 19, 20 one
    C per lane count l = 1 .. 2^(k-12), C = 4 l - (l mod 4), so the last lane holds 3, 2, 1, 4 chunks
    in rotation"""
    top = 1 << (k - 12)
    counts = list(range(1, 129)) if k == 17 else [LANE_CHUNKS * l - (l % 4) for l in range(1, top + 1)]
    items = tuple(1024 * (c - 1) + TAILS[c % len(TAILS)] for c in counts)
    assert len(items) == {17: 128, 18: 64, 19: 128, 20: 256}[k]
    assert all(0 < x <= 1 << k for x in items) and [-(-x // 1024) for x in items] == counts
    assert {lanes_of(x) for x in items} == set(range(1, top + 1))
    assert {last_fill(x) for x in items} == {1, 2, 3, 4}
    assert k != 17 or set(counts) == set(range(1, 129))
    assert {x % 1024 for x in items} == {t % 1024 for t in TAILS}
    return items


def edge_lanes(k: int) -> tuple:
    """E(k): the lane counts around a tree's first levels, a carry that survives every level but the
    last (2^(k-13) + 1), and the full tree"""
    half, top = 1 << (k - 13), 1 << (k - 12)
    e = (1, 2, 3, 4, 5, half - 1, half, half + 1, top - 1, top)
    assert set(e) <= {lanes_of(x) for x in lane_items(k)}
    return e


def anchor() -> list:
    """[(chunks, native.subtree_cv, hc.spec_block_cv)] of small partial items at counter B / 1024:
    the fast reference tied to the pure-Python spec where the chunk count is no power of two"""
    out = []
    for k, c in ((17, 3), (18, 5), (19, 9), (20, 13)):
        length = 1024 * (c - 1) + TAILS[c % len(TAILS)]
        data = native.synth_bytes(8800 + c, 0, 0, length)
        c0 = (1 << k) // 1024
        out.append((c, native.subtree_cv(data, c0), hc.spec_block_cv(data, c0)))
    return out


# ------------------------------------------------------------------------------------ listed blocks
class LaneList(bc.BlockList):
    """one list over one buffer: item i of lane_items(k) sits once in the buffer and is listed twice
    at that offset -- as block 0 of file 2 i, a one-node file of the item's length (ROOT), and as
    block 1 of file 2 i + 1 of B + len bytes (a plain CV at counter B / 1024, its full block not
    resident).  The rows are shuffled; the starts sit on 128-byte lines in a shuffled order of their
    own, item ODD_ITEM 16 bytes past a line; everything outside the items is 0xA5."""
    ODD_ITEM = 5

    def __init__(self, k: int, seed: int):
        B = 1 << k
        items = lane_items(k)
        rng = np.random.default_rng(seed)
        self.k = k
        self.items = items
        self.starts = np.zeros(len(items), np.uint64)
        cur = 0
        for i in rng.permutation(len(items)):
            if i == self.ODD_ITEM:
                cur += 16
            self.starts[i] = cur
            cur = (cur + items[i] + 64 + 127) // 128 * 128
        self.data = np.full(cur + 64, JUNK, np.uint8)
        for i, length in enumerate(items):
            s = int(self.starts[i])
            self.data[s:s + length] = rng.integers(0, 256, length, dtype=np.uint8)
        order = rng.permutation(2 * len(items))
        self.item_of = order // 2          # row -> item
        self.is_root = (order % 2) == 0    # row -> role
        self.lens = np.array([role * B + x for x in items for role in (0, 1)], np.uint64)
        self.n = len(self.lens)
        self.rows = np.array([(f, f % 2) for f in order], np.uint64)
        self.m = len(self.rows)
        self.offsets = self.starts[self.item_of]
        self.sizes = [items[i] for i in self.item_of]
        self.nb = np.array([tc.nodes_of(int(x), k) for x in self.lens], np.uint64)
        self.node_base = np.concatenate([[0], np.cumsum(self.nb)]).astype(np.uint64)
        self.total = int(self.node_base[-1])
        assert self.sizes == [bc.block_len(int(self.lens[int(f)]), int(j), k) for f, j in self.rows]
        assert int(self.starts[self.ODD_ITEM]) % 128 == 16
        assert all(int(s) % 128 == 0 for i, s in enumerate(self.starts) if i != self.ODD_ITEM)
        assert self.total == 3 * len(items) and len(set(self.slots().tolist())) == self.m
        # the shuffle mixes roles and lane counts inside the workgroups of 512 >> (k - 12) items
        per_wg = 512 >> (k - 12)
        groups = [slice(g, g + per_wg) for g in range(0, self.m, per_wg)]
        lanes = np.array([lanes_of(x) for x in self.sizes])
        assert sum(len(set(self.is_root[g].tolist())) == 2 for g in groups) * 4 >= len(groups)
        assert sum(len(set(lanes[g].tolist())) >= 2 for g in groups) * 4 >= 3 * len(groups)

    def item(self, i: int) -> np.ndarray:
        s = int(self.starts[i])
        return self.data[s:s + self.items[i]]


@functools.lru_cache(maxsize=None)
def lane_list(k: int) -> LaneList:
    return LaneList(k, 5100 + k)


@functools.lru_cache(maxsize=None)
def lane_expected(k: int) -> np.ndarray:
    """uint8 [m, 32], list order: the oracle's BLAKE3 of the item for a root row, the oracle's
    non-root CV at counter B / 1024 for the other"""
    bl = lane_list(k)
    roots = native.checksums(bl.data, bl.starts, np.array(bl.items, np.uint64), nthreads=8)
    c0 = (1 << k) // 1024
    cvs = np.stack([np.frombuffer(native.subtree_cv(bl.item(i), c0), np.uint8) for i in range(len(bl.items))])
    assert not (roots == cvs).all(axis=1).any()
    out = np.where(bl.is_root[:, None], roots[bl.item_of], cvs[bl.item_of])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lane_level(k: int) -> np.ndarray:
    """the level layout the list's rows belong to: the reference nodes at the listed slots, random
    bytes at the slots of the full blocks, which are never listed"""
    bl = lane_list(k)
    level = np.random.default_rng(5200 + k).integers(0, 256, (bl.total, 32), dtype=np.uint8)
    level[bl.slots()] = lane_expected(k)
    level.setflags(write=False)
    return level


def lane_flips(k: int) -> tuple:
    """(the data with the last byte of three items flipped -- the first items of 1, 2^(k-13) + 1 and
    2^(k-12) - 1 lanes --, expected flags, rows in list order, stats): both rows of each item"""
    bl = lane_list(k)
    B = 1 << k
    chosen = [next(i for i, x in enumerate(bl.items) if lanes_of(x) == want)
              for want in (1, (1 << (k - 13)) + 1, (1 << (k - 12)) - 1)]
    assert len(set(chosen)) == 3
    d = bl.data.copy()
    flips = []
    for i in chosen:
        d[int(bl.starts[i]) + bl.items[i] - 1] ^= 0x01
        flips += [(2 * i, bl.items[i] - 1), (2 * i + 1, B + bl.items[i] - 1)]
    bad, rows, stats = bc.expected_verify(bl, flips)
    assert int(bad.sum()) == 6 and sorted(np.nonzero(bad)[0]) == sorted(r for r in range(bl.m) if bl.item_of[r] in chosen)
    return d, bad, rows, stats


# ------------------------------------------------------------------------------------ whole files
@functools.lru_cache(maxsize=None)
def tree_lens(k: int) -> tuple:
    """the files `len` and B + len of the sweep (every item at k = 17, 18; the items of E(k) lanes at
    k = 19, 20), and for the items of E(k) lanes q B + len with the partial node last in a 1 MiB leaf
    block and first in the next one; in a shuffled order, so leaf blocks of unlike files share
    workgroups"""
    B = 1 << k
    items = lane_items(k)
    edge = [x for x in items if lanes_of(x) in edge_lanes(k)]
    sweep = items if k in (17, 18) else edge
    lens = [q * B + x for x in sweep for q in (0, 1)]
    qs = (1, 2) if k == 20 else ((1 << (20 - k)) - 1, 1 << (20 - k))
    for q in qs:
        assert q * B % tc.MIB == 0 or (q + 1) * B % tc.MIB == 0
    lens += [q * B + x for x in edge for q in qs]
    assert {lanes_of(x) for x in edge} == set(edge_lanes(k))
    order = np.random.default_rng(5300 + k).permutation(len(lens))
    return tuple(lens[i] for i in order)


@functools.lru_cache(maxsize=None)
def tree_batch(k: int) -> tc.Batch:
    b = tc.Batch(list(tree_lens(k)), k, seed=5400 + 1000 * k, odd_start=3)
    assert len(b.data) < 150 * tc.MIB and int(b.offsets[3]) % 128 == 16
    return b


def block_nodes(b: tc.Batch) -> np.ndarray:
    """uint8 [total, 32]: every node of every file of a batch from the oracle -- its BLAKE3 for a
    one-node file, the non-root CV of block j at counter j B / 1024 otherwise"""
    B = 1 << b.k
    out = np.zeros((b.total, 32), np.uint8)
    for i in range(b.n):
        o, length, base = int(b.offsets[i]), int(b.lens[i]), int(b.node_base[i])
        if int(b.nb[i]) == 1:
            out[base] = b.checksums[i]
            continue
        for j in range(int(b.nb[i])):
            blk = b.data[o + j * B:o + min(length, (j + 1) * B)]
            out[base + j] = np.frombuffer(native.subtree_cv(blk, j * B // 1024), np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def tree_expected(k: int) -> np.ndarray:
    out = block_nodes(tree_batch(k))
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------ proofs
def np_levels(nodes) -> list:
    """[level 0, level 1, .., the root] of a file's nodes uint8 [nb, 32] as uint32 [n, 8]: the odd
    node carried up, ROOT on the parent of the two-node level alone -- the root, which no proof holds"""
    level = np.ascontiguousarray(nodes, np.uint8).reshape(-1).view("<u4").astype(np.uint32).reshape(-1, 8)
    out = [level]
    while len(level) > 1:
        level = hc.np_parents(level, True)
        out.append(level)
    return out


def np_proof(levels: list, j: int) -> np.ndarray:
    """uint8 [p, 32]: the sibling (j >> L) ^ 1 of each level L below the root where it exists"""
    sib = [levels[L][(j >> L) ^ 1] for L in range(len(levels) - 1) if ((j >> L) ^ 1) < len(levels[L])]
    return np.array(sib, np.uint32).reshape(-1, 8).astype("<u4").view(np.uint8).reshape(-1, 32)


def np_proofs(level, lens, rows, k: int) -> tuple:
    """(the packed proofs uint8 [entries, 32] of the rows in list order, proof_base from the closed
    form pc.entries, {file: the root of its level})"""
    nbs = [tc.nodes_of(int(x), k) for x in lens]
    base = np.concatenate([[0], np.cumsum(nbs)])
    rows = np.asarray(rows, np.uint64).reshape(-1, 2)
    levels = {f: np_levels(level[int(base[f]):int(base[f + 1])]) for f in sorted({int(f) for f in rows[:, 0]})}
    parts = [np_proof(levels[int(f)], int(j)) for f, j in rows]
    pbase = np.concatenate([[0], np.cumsum([pc.entries(nbs[int(f)], int(j)) for f, j in rows])]).astype(np.uint64)
    assert [len(p) for p in parts] == np.diff(pbase).astype(np.int64).tolist()
    proofs = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    roots = {f: lv[-1][0].astype("<u4").tobytes() for f, lv in levels.items()}
    return proofs, pbase, roots


PROOF_K = 17
PROOF_NBS = tuple(range(1, 41)) + tuple(range(250, 263)) + tuple(range(508, 518)) + (
    773, 65_535, 65_536, 65_537, 65_538, 65_793, 131_073)
PROOF_GARBAGE = 60   # an unlisted file among them: its level may hold anything
PROOF_ROWS = 9_634   # 9 273 of the files of at most 520 nodes, 361 of the seven above
PROOF_ENTRIES = 86_258  # the sum of pc.entries over the rows


@functools.lru_cache(maxsize=None)
def proof_case() -> tuple:
    """(lens, rows shuffled, the level layout of random nodes, the numpy proofs, proof_base, roots):
    every row of the files of at most 520 nodes; of the larger ones the rows around the group
    boundaries of 256 and 65 536 nodes, the last two, and 40 seeded random ones"""
    nbs = list(PROOF_NBS)
    nbs.insert(PROOF_GARBAGE, 300)
    lens = [nb << PROOF_K for nb in nbs]
    rng = np.random.default_rng(5500)
    level = rng.integers(0, 256, (sum(nbs), 32), dtype=np.uint8)
    rows = []
    for f, nb in enumerate(nbs):
        if f == PROOF_GARBAGE:
            continue
        if nb <= 520:
            js = range(nb)
        else:
            fixed = sorted(j for j in {0, 1, 254, 255, 256, 257, 511, 512, 65_534, 65_535, 65_536, 65_537, nb - 2, nb - 1}
                           if j < nb)
            rest = np.setdiff1d(np.arange(nb), fixed)
            js = fixed + sorted(int(j) for j in rng.choice(rest, 40, replace=False))
        rows += [(f, j) for j in js]
    rows = np.array(rows, np.uint64)[rng.permutation(len(rows))]
    proofs, pbase, roots = np_proofs(level, lens, rows, PROOF_K)
    assert len(rows) == PROOF_ROWS and len(proofs) == int(pbase[-1]) == PROOF_ENTRIES, (len(rows), len(proofs))
    for a in (level, proofs, pbase, rows):
        a.setflags(write=False)
    return lens, rows, level, proofs, pbase, roots


def proof_garbage_level() -> np.ndarray:
    lens, _, level, _, _, _ = proof_case()
    nbs = [x >> PROOF_K for x in lens]
    lo = sum(nbs[:PROOF_GARBAGE])
    out = level.copy()
    out[lo:lo + nbs[PROOF_GARBAGE]] = 0x5A
    return out


# ------------------------------------------------------------------------------------ climb
CLIMB_K = 17
CLIMB_NBS = tuple(range(1, 25)) + (31, 32, 33)


@functools.lru_cache(maxsize=None)
def climb_batch() -> tc.Batch:
    B = 1 << CLIMB_K
    lens = [(nb - 1) * B + (1, 4097, B)[i % 3] for i, nb in enumerate(CLIMB_NBS)]
    b = tc.Batch(lens, CLIMB_K, seed=5600, odd_start=4)
    assert tuple(int(x) for x in b.nb) == CLIMB_NBS
    return b


@functools.lru_cache(maxsize=None)
def climb_list() -> bc.BlockList:
    """every block of every file, shuffled: the lanes of one wave climb 0 to 6 levels"""
    b = climb_batch()
    bl = bc.BlockList([int(x) for x in b.lens], CLIMB_K, bc.every_row(b, 5601), bc.blocks_of(b), seed=5602, odd=2)
    assert bl.m == b.total == sum(CLIMB_NBS)
    return bl


@functools.lru_cache(maxsize=None)
def climb_reference() -> tuple:
    """(the level from the oracle, the packed numpy proofs of climb_list's rows, proof_base); the
    numpy root of every level is the oracle's BLAKE3 of the file"""
    b, bl = climb_batch(), climb_list()
    level = block_nodes(b)
    proofs, pbase, roots = np_proofs(level, bl.lens, bl.rows, CLIMB_K)
    for f, root in roots.items():
        assert root == b.checksums[f].tobytes(), f
    for a in (level, proofs, pbase):
        a.setflags(write=False)
    return level, proofs, pbase


def climb_flips() -> tuple:
    """(proofs with one bit flipped in one entry of each chosen row, the rows that must be flagged).
    Of the nb = 33 file: the only entry of row j = 32 (the carried node meets its sibling on the
    two-node level, under ROOT), and the entry of depth d of row j = d + 1 for d = 0 .. 5, a row of
    its own per depth so that each flip has to be caught by itself; the first entry of row j = 0 of
    the files of 2, 3, 5 and 17 nodes."""
    bl = climb_list()
    _, proofs, pbase = climb_reference()
    p = proofs.copy()
    f33 = CLIMB_NBS.index(33)
    assert pc.entries(33, 32) == 1 and all(pc.entries(33, d + 1) == 6 for d in range(6))
    hits = [(f33, 32, 0)] + [(f33, d + 1, d) for d in range(6)] + [(CLIMB_NBS.index(nb), 0, 0) for nb in (2, 3, 5, 17)]
    bad_rows = []
    for q, (f, j, depth) in enumerate(hits):
        r = pc.row_of(bl, f, j)
        assert int(pbase[r]) + depth < int(pbase[r + 1])
        p[int(pbase[r]) + depth, (5 * q) % 32] ^= np.uint8(1 << (q % 8))
        bad_rows.append(r)
    assert len(set(bad_rows)) == len(hits) == 11
    return p, sorted(bad_rows)
