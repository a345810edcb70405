"""Block proofs (include/sd_cas.h, checksum trees, block proofs): the definitions restated over
oracle/blake3_spec.py's compress, and the cases shared by tests/test_checksum_proofs.py (the CPU
twins) and tests/test_gpu_checksum_proofs.py (the kernels).  No call of the code under test in the
references:
  spec_levels(nodes)            every level of a file, level-wise, the odd node carried
  entries(nb, j)                the closed form of a proof's entry count
  spec_proof(levels, j)         the siblings on block j's way up, bottom-up
  spec_climb(node, proof, nb, j)  the root a node and a proof claim
A proof certifies itself: the oracle for a proof under test is that spec_climb(node, proof) reaches
a root that came from elsewhere -- tc.spec_root of a level of random nodes, or the oracle's BLAKE3 of
real bytes -- never from the code under test.
"""
import functools
import struct

import numpy as np

from tests import checksum_blocks_cases as bc
from tests import checksum_tree_cases as tc

KS = (17, 20)
JUNK = bc.JUNK


def _cv(row) -> tuple:
    return struct.unpack("<8I", bytes(row))


def spec_levels(nodes) -> list:
    """[level 0, level 1, ..] as lists of 8-word tuples, down to the level of one node (the root)"""
    level = [_cv(r.tobytes()) for r in np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32)]
    out = [level]
    while len(level) > 1:
        n = len(level)
        nxt = [tuple(tc._parent(level[2 * i], level[2 * i + 1], n == 2)) for i in range(n // 2)]
        if n & 1:
            nxt.append(level[-1])
        out.append(nxt)
        level = nxt
    return out


def height(nb: int) -> int:
    return (nb - 1).bit_length()


def entries(nb: int, j: int) -> int:
    """p: the levels L < h at which (j >> L) ^ 1 < n_L"""
    p, n = 0, nb
    for L in range(height(nb)):
        p += ((j >> L) ^ 1) < n
        n = -(-n // 2)
    return p


def spec_proof(levels: list, j: int) -> bytes:
    out = []
    for L in range(len(levels) - 1):
        s = (j >> L) ^ 1
        if s < len(levels[L]):
            out.append(tc._pack(levels[L][s]))
    return b"".join(out)


def spec_climb(node: bytes, proof: bytes, nb: int, j: int) -> bytes:
    """the root (node, proof) claim for block j of a file of nb nodes; the proof must be exactly
    entries(nb, j) entries long"""
    cv, n, at = _cv(node), nb, 0
    for L in range(height(nb)):
        i = j >> L
        if (i ^ 1) < n:
            e = _cv(proof[at:at + 32])
            at += 32
            cv = tc._parent(e, cv, n == 2) if i & 1 else tc._parent(cv, e, n == 2)
        n = -(-n // 2)
    assert at == len(proof), (at, len(proof))
    return tc._pack(cv)


def proof_base(lens, rows, k: int) -> np.ndarray:
    base = [0]
    for f, j in np.asarray(rows, np.uint64).reshape(-1, 2):
        base.append(base[-1] + entries(tc.nodes_of(int(lens[int(f)]), k), int(j)))
    return np.array(base, np.uint64)


def check_proofs(lens, rows, k: int, level, proofs, roots, what="") -> None:
    """every row's proof (packed by proof_base) climbs from the row's node of `level` to roots[f]"""
    level = np.asarray(level, np.uint8).reshape(-1, 32)
    proofs = np.asarray(proofs, np.uint8).reshape(-1, 32)
    base = proof_base(lens, rows, k)
    assert len(proofs) == int(base[-1]), (what, len(proofs), int(base[-1]))
    nbs = [tc.nodes_of(int(x), k) for x in lens]
    node_base = np.concatenate([[0], np.cumsum(nbs)])
    for r, (f, j) in enumerate(np.asarray(rows, np.uint64).reshape(-1, 2)):
        f, j = int(f), int(j)
        got = spec_climb(level[int(node_base[f]) + j].tobytes(), proofs[int(base[r]):int(base[r + 1])].tobytes(), nbs[f], j)
        assert got == bytes(roots[f]), (what, k, r, f, j)


# ------------------------------------------------------------------------------------ real bytes
def real_lens(k: int) -> list:
    """nb = 1 (empty, 1 byte, B), 2 (ROOT on the only parent; a 1-byte trailing block), 3 (block 2
    carried once), 5 (block 4 carried twice), 8 (a full tree), 9 (full + 1, a 1-byte trailing block)"""
    B = 1 << k
    return [0, 1, B, B + 1, 2 * B + 4097, 4 * B + 77, 8 * B, 8 * B + 1]


@functools.lru_cache(maxsize=None)
def real_batch(k: int) -> tc.Batch:
    b = tc.Batch(real_lens(k), k, seed=6000 + k)
    assert [int(x) for x in b.nb] == [1, 1, 1, 2, 3, 5, 8, 9]
    return b


@functools.lru_cache(maxsize=None)
def real_list(k: int) -> bc.BlockList:
    """every block of every file in ONE list, shuffled, six of them twice: lanes of one wave climb
    0, 1, 2, 3 and 4 levels"""
    b = real_batch(k)
    rows = bc.every_row(b, 91 + k)
    rows = np.concatenate([rows, rows[[0, 3, 7, 11, 19, 28]]])
    rows = rows[np.random.default_rng(92 + k).permutation(len(rows))]
    return bc.BlockList(real_lens(k), k, rows, bc.blocks_of(b), seed=93 + k, odd=2)


def row_of(bl: bc.BlockList, f: int, j: int) -> int:
    """the first row that lists (f, j)"""
    return next(r for r, (rf, rj) in enumerate(bl.rows) if (int(rf), int(rj)) == (f, j))


def rows_of(bl: bc.BlockList, f: int, j: int = None) -> list:
    return [r for r, (rf, rj) in enumerate(bl.rows) if int(rf) == f and (j is None or int(rj) == j)]


# ------------------------------------------------------------------------------------ levels alone
LEVEL_K = 17
LEVEL_NBS = (255, 256, 257, 65537)  # a short group, a full one, full + 1, three passes of 256 to the root
GARBAGE_FILE = 2                    # an unlisted file between them: its level may hold anything


@functools.lru_cache(maxsize=None)
def level_case() -> tuple:
    """(lens, rows, the level layout of random nodes, {file: the expected root}): rows at j = 0, 255,
    256, nb - 2 and nb - 1 of every listed file; prove and climb depend on no byte"""
    nbs = list(LEVEL_NBS)
    nbs.insert(GARBAGE_FILE, 300)
    lens = [nb << LEVEL_K for nb in nbs]
    rng = np.random.default_rng(4242)
    level = rng.integers(0, 256, (sum(nbs), 32), dtype=np.uint8)
    rows = []
    for f, nb in enumerate(nbs):
        if f == GARBAGE_FILE:
            continue
        rows += [(f, j) for j in sorted({0, 255, 256, nb - 2, nb - 1}) if j < nb]
    rows = np.array(rows, np.uint64)[rng.permutation(len(rows))]
    base = np.concatenate([[0], np.cumsum(nbs)])
    roots = {f: tc.spec_root(level[int(base[f]):int(base[f + 1])]) for f in range(len(nbs)) if f != GARBAGE_FILE}
    return lens, rows, level, roots


def garbage_level() -> np.ndarray:
    """level_case's level with the unlisted file's nodes replaced"""
    lens, rows, level, _ = level_case()
    nbs = [x >> LEVEL_K for x in lens]
    lo = sum(nbs[:GARBAGE_FILE])
    out = level.copy()
    out[lo:lo + nbs[GARBAGE_FILE]] = 0x5A
    return out


# ------------------------------------------------------------------------------------ rejections
def rejections(bl: bc.BlockList, proofs, roots) -> list:
    """[(name, data, proofs, roots, the rows that must be flagged)] over real_list(k): each case
    changes one thing and must flag exactly the rows concerned.  Files: 6 has nb = 8 (every proof 3
    entries), 7 has nb = 9, 5 has nb = 5."""
    proofs = np.asarray(proofs, np.uint8).reshape(-1, 32)
    roots = np.asarray(roots, np.uint8).reshape(-1, 32)
    base = proof_base(bl.lens, bl.rows, bl.k)
    span = lambda r: slice(int(base[r]), int(base[r + 1]))  # noqa: E731
    out = []
    # one bit of a block's bytes: that row alone (a repeat of it holds bytes of its own)
    r = row_of(bl, 6, 3)
    d = bl.data.copy()
    d[int(bl.offsets[r]) + 70000] ^= 0x10
    out.append(("byte", d, proofs, roots, [r]))
    # one bit of one proof entry
    r = row_of(bl, 7, 2)
    p = proofs.copy()
    p[int(base[r]) + 1, 9] ^= 0x01
    out.append(("entry", bl.data, p, roots, [r]))
    # one bit of a file's root: every row of the file
    rt = roots.copy()
    rt[5, 31] ^= 0x80
    out.append(("root", bl.data, proofs, rt, rows_of(bl, 5)))
    # the proofs of two rows swapped (equal lengths: both of the nb = 8 file)
    a, b = row_of(bl, 6, 2), row_of(bl, 6, 5)
    p = proofs.copy()
    p[span(a)], p[span(b)] = proofs[span(b)], proofs[span(a)]
    out.append(("swapped", bl.data, p, roots, sorted([a, b])))
    # the proof of block j under row j ^ 1: it starts with N_{j^1}, the row's own node
    a, b = row_of(bl, 6, 6), row_of(bl, 6, 7)
    p = proofs.copy()
    p[span(b)] = proofs[span(a)]
    out.append(("sibling", bl.data, p, roots, [b]))
    # the last entry of a proof taken from the neighbouring file's
    a, b = row_of(bl, 6, 0), row_of(bl, 7, 0)
    p = proofs.copy()
    p[int(base[a + 1]) - 1] = proofs[int(base[b + 1]) - 1]
    out.append(("neighbour", bl.data, p, roots, [a]))
    return out


def expected_flags(bl: bc.BlockList, bad_rows) -> tuple:
    bad = np.zeros(bl.m, np.uint8)
    bad[list(bad_rows)] = 1
    rows = bl.rows[bad != 0]
    stats = np.array([bl.n, bl.m, int(bad.sum()), len({int(f) for f, _ in rows})], np.uint64)
    return bad, rows, stats


# ------------------------------------------------------------------------------------ the deep tree
DEEP_K = 20
DEEP_NB = (1 << 22) + 3
DEEP_LEN = ((1 << 22) + 2 << 20) + 4097
DEEP_BLOCKS = (0, 12345, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 22) + 2)


def deep_list() -> bc.BlockList:
    """blocks of a 4 TiB file at k = 20, only they resident (one second file of one block beside
    it): block 2^22 + 1 hashes chunk counters past 2^32, block 2^22 + 2 is the 4097-byte tail whose
    node is carried up"""
    from oracle import native
    lens = [DEEP_LEN, 5000]
    assert tc.nodes_of(DEEP_LEN, DEEP_K) == DEEP_NB and ((1 << 22) + 1) * 1024 > 1 << 32
    rows = [(0, j) for j in DEEP_BLOCKS] + [(1, 0)]
    blocks = {(f, j): native.synth_bytes(7000 + q, 0, 0, bc.block_len(lens[f], j, DEEP_K)) for q, (f, j) in enumerate(rows)}
    order = np.random.default_rng(8).permutation(len(rows))
    return bc.BlockList(lens, DEEP_K, [rows[r] for r in order], blocks, seed=9, odd=1)
