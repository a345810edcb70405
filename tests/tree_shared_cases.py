"""Cases for the shared blocks of a batch of levels (include/sd_cas.h: sd_checksum_tree_shared,
sd_cpu_checksum_tree_shared), shared by tests/test_tree_shared.py (the host sibling, the Python
wrappers) and tests/test_gpu_tree_shared.py (the kernels, down both grouping paths).  Every builder
asserts the premise it exists for, so a wrong edit cannot quietly shrink the sweep.

A case is (name, lens uint64 [n], block_log2, nodes uint8 [m, 32]).  Levels are crafted, not hashed:
random 32-byte nodes with planted equalities -- the call compares nodes as opaque values, so no
BLAKE3 is needed to exercise it.

shared_model restates the header's contract: rows of (block index, 32 bytes) grouped with np.unique
over a void view, the representative the first occurrence in slot order, everything else plain
loops.  It is written from the header's words, not from either implementation.

Nothing here touches a device or the library.
"""
from __future__ import annotations

import numpy as np

from tests.sliced_cases import BLOCKS, TILE, slice_len

U = np.uint64
PAST_GRID = BLOCKS * TILE + 1  # every workgroup's slice holds more than one tile


def blocks_of(length: int, k: int) -> int:
    return max(1, -(-int(length) // (1 << k)))


def layout(lens, k: int):
    """(node_base list [n + 1], file_of int64 [m], j_of int64 [m])"""
    nb = [blocks_of(L, k) for L in lens]
    base = [0]
    for b in nb:
        base.append(base[-1] + b)
    file_of = np.repeat(np.arange(len(nb), dtype=np.int64), nb) if nb else np.zeros(0, np.int64)
    j_of = np.arange(base[-1], dtype=np.int64) - np.array(base[:-1], np.int64)[file_of] if nb else np.zeros(0, np.int64)
    return base, file_of, j_of


def shared_model(lens, k: int, nodes, min_blocks: int = 0) -> dict:
    """-> rep, size (uint64 [m]), files (uint64 [n, 4]), pairs (uint64 [p, 4]), stats (uint64 [8])"""
    lens = [int(L) for L in lens]
    n, B = len(lens), 1 << k
    base, file_of, j_of = layout(lens, k)
    m = base[-1]
    nodes = np.asarray(nodes, np.uint8).reshape(m, 32)
    rows = np.zeros((m, 40), np.uint8)
    rows[:, :8] = j_of.astype(">u8").view(np.uint8).reshape(m, 8)
    rows[:, 8:] = nodes
    if m:
        _, first, inv, cnt = np.unique(rows.view(np.dtype((np.void, 40))).reshape(-1), return_index=True,
                                       return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        rep, size = first[inv], cnt[inv]  # first occurrence in slot order = the smallest slot of the class
        classes, classes2 = len(first), int((cnt >= 2).sum())
    else:
        rep, size, classes, classes2 = np.zeros(0, np.int64), np.zeros(0, np.int64), 0, 0
    files = [[base[f + 1] - base[f], 0, 0, 0] for f in range(n)]
    pair = {}
    for s in range(m):
        f, j = int(file_of[s]), int(j_of[s])
        if size[s] >= 2:
            files[f][1] += 1
        if rep[s] != s:
            by = min(B, max(0, lens[f] - j * B))
            files[f][2] += 1
            files[f][3] += by
            g = int(file_of[rep[s]])
            assert g < f
            row = pair.setdefault((f, g), [0, 0])
            row[0] += 1
            row[1] += by
    need = max(1, int(min_blocks))
    pairs = [(f, g, b, y) for (f, g), (b, y) in sorted(pair.items()) if b >= need]
    stats = [n, m, classes, classes2, sum(r[2] for r in files), sum(r[3] for r in files),
             sum(1 for r in files if r[2]), sum(1 for r in files if r[2] == r[0])]
    return {"rep": np.asarray(rep, U), "size": np.asarray(size, U), "files": np.array(files, U).reshape(-1, 4),
            "pairs": np.array(pairs, U).reshape(-1, 4), "stats": np.array(stats, U)}


def has_tie(lens, k: int, nodes) -> bool:
    """some slots share their block index and their first 8 node bytes and differ after them: what
    sends the grouping down the full-width path"""
    _, _, j_of = layout(lens, k)
    nd = np.asarray(nodes, np.uint8).reshape(len(j_of), 32)
    tails = {}
    for s in range(len(j_of)):
        tails.setdefault((int(j_of[s]), bytes(nd[s, :8])), set()).add(bytes(nd[s, 8:]))
    return any(len(t) >= 2 for t in tails.values())


def check_identities(want_or_got: dict, min_blocks: int = 0) -> None:
    st = [int(x) for x in want_or_got["stats"]]
    files, pairs = want_or_got["files"], want_or_got["pairs"]
    assert st[4] == st[1] - st[2] == int(files[:, 2].sum()) if len(files) else st[4] == 0, st
    assert st[5] == (int(files[:, 3].sum()) if len(files) else 0), st
    assert st[3] <= st[2] <= st[1] and st[7] <= st[6] <= max(st[0] - 1, 0), st
    if len(files):
        assert int(files[0, 2]) == 0 and int(files[:, 0].sum()) == st[1]  # file 0 is never redundant
    if min_blocks <= 1:
        assert int(pairs[:, 2].sum()) == st[4] and int(pairs[:, 3].sum()) == st[5], st
    if len(pairs):
        assert (pairs[:, 1] < pairs[:, 0]).all()
        order = [(int(f), int(g)) for f, g in pairs[:, :2]]
        assert order == sorted(set(order))  # ascending by (f, g), each pair once


# ---------------------------------------------------------------- builders
def fresh(rng, lens, k: int) -> np.ndarray:
    """random nodes for every slot (no two equal: 32 random bytes)"""
    return rng.integers(0, 256, (layout(lens, k)[0][-1], 32), dtype=np.uint8)


def plant(nodes, base, f: int, g: int, blocks) -> None:
    """file f's nodes at `blocks` become file g's at the same block indices"""
    for j in blocks:
        assert j < base[f + 1] - base[f] and j < base[g + 1] - base[g]
        nodes[base[f] + j] = nodes[base[g] + j]


def pooled(lens, k: int, seed: int):
    """random levels in which about a third of the files copy a random half of the blocks they have
    in common with one other file (earlier or later: representatives are not always the source)"""
    rng = np.random.default_rng(seed)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    n = len(lens)
    for f in range(n):
        if n < 2 or rng.random() > 1 / 3:
            continue
        g = int(rng.integers(0, n - 1))
        g += g >= f
        common = min(base[f + 1] - base[f], base[g + 1] - base[g])
        plant(nodes, base, f, g, [j for j in range(common) if rng.random() < 0.5])
    return np.array(lens, U), k, nodes


def lens_for(m: int, seed: int, k: int, most: int = 12):
    """file lengths of 1 .. `most` blocks, some a whole number of blocks, some empty, m slots in all"""
    rng = np.random.default_rng(seed)
    B, lens, left = 1 << k, [], m
    while left:
        nb = int(min(left, rng.integers(1, most + 1)))
        kind = rng.integers(0, 4)
        if kind == 0:
            lens.append(nb * B)  # an exact multiple
        elif kind == 1 and nb == 1:
            lens.append(0)  # an empty file
        else:
            lens.append((nb - 1) * B + int(rng.integers(1, B)))
        left -= nb
    assert sum(blocks_of(L, k) for L in lens) == m
    return lens


def size_cases():
    """a tile less one, a tile, a tile and one: the last lane, the edge, the second workgroup"""
    out = []
    for m in (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out.append((f"slots_{m}", *pooled(lens_for(m, 500 + m, 17), 17, 600 + m)))
    out.append(("slots_257_k20", *pooled(lens_for(TILE + 1, 520, 20), 20, 620)))
    return out


def past_grid_case():
    """BLOCKS * TILE + 1 slots: two tiles per slice.  2048 files of 128 blocks and a one-block file;
    a quarter of the files are copies of another with a few blocks changed"""
    k, B = 17, 1 << 17
    lens = [128 * B - (f % 3) * 777 for f in range(2048)] + [5]
    rng = np.random.default_rng(700)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    assert base[-1] == PAST_GRID and slice_len(PAST_GRID) == 2 * TILE
    for f in rng.choice(2048, 512, replace=False):
        g = int(rng.integers(0, 2047))
        g += g >= f
        plant(nodes, base, int(f), g, [j for j in range(128) if rng.random() < 0.97])
    return ("past_grid", np.array(lens, U), k, nodes)


def one_node_case():
    """only one-node files: every slot is block 0, a third of them equal to another"""
    lens = [1 + 1000 * i for i in range(60)] + [1 << 17] * 4
    return ("one_node_files", *pooled(lens, 17, 710))


def empty_case():
    """empty files share one node (the hash of the empty message) at 0 bytes, among others"""
    k = 17
    lens = [0, 300_000, 0, 0, 5, 0]
    rng = np.random.default_rng(720)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    for f in (2, 3, 5):
        plant(nodes, base, f, 0, [0])
    m = shared_model(lens, k, nodes)
    assert m["pairs"].tolist() == [[2, 0, 1, 0], [3, 0, 1, 0], [5, 0, 1, 0]] and m["stats"][5] == 0
    assert m["stats"][7] == 3  # wholly redundant, at no byte
    return ("empty_files", np.array(lens, U), k, nodes)


def big_class_case():
    """a class larger than a tile: 300 files of two blocks with equal block 0"""
    k, B = 17, 1 << 17
    lens = [B + 1 + f for f in range(300)]
    rng = np.random.default_rng(730)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    for f in range(1, 300):
        plant(nodes, base, f, 0, [0])
    m = shared_model(lens, k, nodes)
    assert int(m["size"].max()) == 300 > TILE and len(m["pairs"]) == 299 and (m["pairs"][:, 1] == 0).all()
    return ("class_of_300", np.array(lens, U), k, nodes)


def long_run_case():
    """a pair run that crosses tiles and slices: file 3 has 700 blocks, all of them file 1's; its
    slots straddle slices of one tile each, and so do its 700 records among the others'"""
    k, B = 17, 1 << 17
    lens = [90 * B + 7, 700 * B, 40 * B, 700 * B, 100 * B + 9, 90 * B + 7]
    rng = np.random.default_rng(740)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    plant(nodes, base, 3, 1, range(700))
    plant(nodes, base, 5, 0, range(91))  # the partial last block too
    plant(nodes, base, 4, 2, range(0, 40, 2))
    m = sum(blocks_of(L, k) for L in lens)
    assert slice_len(m) == TILE and base[3] // TILE < (base[4] - 1) // TILE - 1
    want = shared_model(lens, k, nodes)
    assert want["pairs"].tolist() == [[3, 1, 700, 700 * B], [4, 2, 20, 20 * B], [5, 0, 91, 90 * B + 7]]
    return ("run_of_700", np.array(lens, U), k, nodes)


def three_holders_case():
    """three holders of one block: both later ones point at the first"""
    k, B = 17, 1 << 17
    lens = [3 * B, 4 * B + 1, 2 * B, 5 * B]
    rng = np.random.default_rng(750)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    plant(nodes, base, 1, 0, [1])
    plant(nodes, base, 3, 0, [1])
    m = shared_model(lens, k, nodes)
    assert m["rep"][base[1] + 1] == m["rep"][base[3] + 1] == base[0] + 1 and m["size"][base[3] + 1] == 3
    assert m["pairs"].tolist() == [[1, 0, 1, B], [3, 0, 1, B]]
    return ("three_holders", np.array(lens, U), k, nodes)


def different_index_case():
    """equal nodes planted at DIFFERENT block indices must not match"""
    k, B = 17, 1 << 17
    lens = [4 * B, 4 * B, 6 * B]
    rng = np.random.default_rng(760)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    nodes[base[1] + 2] = nodes[base[0] + 1]
    nodes[base[2] + 5] = nodes[base[0] + 0]
    nodes[base[2] + 0] = nodes[base[2] + 3]  # and inside one file
    m = shared_model(lens, k, nodes)
    assert (m["size"] == 1).all() and len(m["pairs"]) == 0 and m["stats"][4] == 0
    return ("different_index", np.array(lens, U), k, nodes)


def tie_cases():
    """equal block index and equal first 8 node bytes with tails A, B, A: adjacency in the prefix
    order proves nothing, the full-width path has to run"""
    k, B = 17, 1 << 17
    h0, A, Bt = bytes(range(8)), bytes([0x11] * 24), bytes([0x22] * 24)
    out = []
    lens = [3 * B, 3 * B, 3 * B]
    rng = np.random.default_rng(770)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    for f, tail in enumerate((A, Bt, A)):
        nodes[base[f] + 1] = list(h0 + tail)
    m = shared_model(lens, k, nodes)
    assert [int(m["rep"][base[f] + 1]) for f in range(3)] == [1, 4, 1] and m["pairs"].tolist() == [[2, 0, 1, B]]
    out.append(("tie_aba", np.array(lens, U), k, nodes))
    # the same among other files, the tied slots at the partial last block of files of one length
    lens2, k2, nodes2 = pooled(lens_for(600, 771, 17) + [2 * B + 99] * 5, 17, 772)
    base2 = layout(lens2, k2)[0]
    n2 = len(lens2)
    for f, tail in zip(range(n2 - 5, n2), (A, Bt, A, Bt, Bt)):
        nodes2[base2[f] + 2] = list(h0 + tail)
    out.append(("tie_among_others", lens2, k2, nodes2))
    for c in out:
        assert has_tie(*c[1:]), c[0]
    # a run of equal (index, first 8 bytes) that is uniform: the prefix path finishes it
    nodes3 = nodes.copy()
    nodes3[base[1] + 1] = list(h0 + A)
    assert not has_tie(lens, k, nodes3)
    out.append(("tie_uniform", np.array(lens, U), k, nodes3))
    return out


def trailing_cases():
    k, B = 17, 1 << 17
    out = []
    # two files of equal non-multiple length share the partial last block: the bytes deficit
    lens = [4 * B + 1000, 4 * B + 1000]
    rng = np.random.default_rng(780)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    plant(nodes, base, 1, 0, [0, 2, 4])
    assert shared_model(lens, k, nodes)["pairs"].tolist() == [[1, 0, 3, 2 * B + 1000]]
    out.append(("tail_shared", np.array(lens, U), k, nodes))
    # a file whose length is an exact multiple: its last block is a full one
    lens = [4 * B, 4 * B, 5 * B]
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    plant(nodes, base, 1, 0, [3])
    plant(nodes, base, 2, 0, [2, 3])
    assert shared_model(lens, k, nodes)["pairs"].tolist() == [[1, 0, 1, B], [2, 0, 2, 2 * B]]
    out.append(("tail_exact_multiple", np.array(lens, U), k, nodes))
    # a last partial block whose representative is in a different file from the rest of the run
    lens = [5 * B, 4 * B + 77, 4 * B + 77, 4 * B + 77]
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    plant(nodes, base, 2, 0, [0, 1, 2, 3])
    plant(nodes, base, 2, 1, [4])
    plant(nodes, base, 3, 1, [0, 4])
    plant(nodes, base, 3, 0, [2])
    want = shared_model(lens, k, nodes)
    assert want["pairs"].tolist() == [[2, 0, 4, 4 * B], [2, 1, 1, 77], [3, 0, 1, B], [3, 1, 2, B + 77]]
    assert want["stats"][7] == 1  # file 2 alone is wholly redundant
    out.append(("tail_other_holder", np.array(lens, U), k, nodes))
    # the same at 1 MiB blocks
    B20 = 1 << 20
    lens = [3 * B20 + 5, 3 * B20 + 5, 2 * B20]
    nodes = fresh(rng, lens, 20)
    base = layout(lens, 20)[0]
    plant(nodes, base, 1, 0, [1, 3])
    plant(nodes, base, 2, 1, [0])
    assert shared_model(lens, 20, nodes)["pairs"].tolist() == [[1, 0, 2, B20 + 5], [2, 1, 1, B20]]
    out.append(("tail_k20", np.array(lens, U), 20, nodes))
    return out


def min_blocks_case():
    """pairs of 1, 3 and 5 blocks: min_blocks 0 and 1 keep all, 3 drops one, 4 two, 6 all"""
    k, B = 17, 1 << 17
    lens = [8 * B] * 4
    rng = np.random.default_rng(790)
    nodes = fresh(rng, lens, k)
    base = layout(lens, k)[0]
    plant(nodes, base, 1, 0, [7])
    plant(nodes, base, 2, 0, [0, 1, 2])
    plant(nodes, base, 3, 1, [1, 2, 3, 4, 5])
    for mb, rows in ((0, 3), (1, 3), (3, 2), (4, 1), (5, 1), (6, 0)):
        assert len(shared_model(lens, k, nodes, mb)["pairs"]) == rows
    return ("min_blocks", np.array(lens, U), k, nodes)


MIN_BLOCKS = (0, 1, 3, 4, 6)  # none, the floor, exactly a pair's count, one above, above all


def small_cases():
    """every case but the large one"""
    k = 17
    return ([("no_files", np.zeros(0, U), k, np.zeros((0, 32), np.uint8)),
             ("one_file", *pooled([5 * (1 << k) + 3], k, 800))] + size_cases() +
            [one_node_case(), empty_case(), big_class_case(), long_run_case(), three_holders_case(),
             different_index_case()] + tie_cases() + trailing_cases() + [min_blocks_case()])


_ALL = None


def all_cases():
    """the whole list, each with its model at min_blocks 0 and whether it ties, built once per process"""
    global _ALL
    if _ALL is None:
        _ALL = [(name, lens, k, nodes, shared_model(lens, k, nodes), has_tie(lens, k, nodes))
                for name, lens, k, nodes in small_cases() + [past_grid_case()]]
    return _ALL


# ---------------------------------------------------------------- real bytes (end to end)
def scenario():
    """Real files at 128 KiB blocks, 3 to 9 blocks each, and what must come out, from the plant alone:
    -> (contents: list of uint8 arrays, want_files rows (blocks, shared, redundant, redundant bytes),
    want_pairs).  File 0 is the original: 6 full blocks and a partial one."""
    B = 1 << 17
    rng = np.random.default_rng(900)
    a = rng.integers(0, 256, 6 * B + 1000, dtype=np.uint8)
    copy = a.copy()
    rewritten = a.copy()
    rewritten[2 * B + 17] ^= 1          # block 2
    rewritten[6 * B + 999] ^= 0x80      # block 6, the partial one
    cut3 = a[:3 * B].copy()             # truncated at a block boundary: its nodes are a's first three
    cut1 = a[:B].copy()                 # one block: its node is a root hash and matches nothing
    grown = np.concatenate([a, rng.integers(0, 256, 2 * B + B // 2, dtype=np.uint8)])  # 9 blocks
    contents = [a, copy, rewritten, cut3, cut1, grown]
    assert [blocks_of(len(c), 17) for c in contents] == [7, 7, 7, 3, 1, 9]
    want_files = [[7, 7, 0, 0], [7, 7, 7, len(a)], [7, 5, 5, 5 * B], [3, 3, 3, 3 * B], [1, 0, 0, 0],
                  [9, 6, 6, 6 * B]]
    want_pairs = [[1, 0, 7, len(a)], [2, 0, 5, 5 * B], [3, 0, 3, 3 * B], [5, 0, 6, 6 * B]]
    return contents, want_files, want_pairs


def scenario_buffer(contents):
    """(buffer uint8, offsets, lens): the files at 64-byte aligned starts, readable past the end"""
    offs, off = [], 0
    for c in contents:
        offs.append(off)
        off = (off + len(c) + 127) // 64 * 64
    buf = np.zeros(off + 64, np.uint8)
    for c, o in zip(contents, offs):
        buf[o:o + len(c)] = c
    return buf, offs, [len(c) for c in contents]
