"""Input generators shared by tests/test_gpu_shapes.py (the kernels) and
tests/test_shape_cases.py (the CPU path, the oracle and these generators themselves): the
shapes the hash and dedup kernels branch on, enumerated rather than sampled.  Every list
asserts its own length, so a wrong filter cannot quietly shrink a sweep.

Nothing here touches a device or the library.
"""
from __future__ import annotations

import numpy as np

MiB = 1 << 20
CHUNK = 1024
WHOLE_MSG_MAX = 102408  # 8 + 102400: the longest message the whole-file work lists take
M64 = (1 << 64) - 1

# ------------------------------------------------------------------ A: whole-file trees
SWEEP_A_R = (1, 63, 64, 65, 960, 1023, 1024)
SWEEP_A_COUNT = 700  # C = 1: 6 (r = 1 is under 8 bytes); C = 2..100: 7 each; C = 101: r = 1 only


def sweep_a():
    """Whole-kind cas messages of msg_len = 1024 (C - 1) + r for every chunk count C = 1..101
    and every r of SWEEP_A_R, kept where 8 <= msg_len <= 102408 -> [(C, r, msg_len)],
    ascending.  The file size is msg_len - 8; the message has P = (C + 1) // 2 chunk pairs."""
    cases = []
    for C in range(1, 102):
        for r in SWEEP_A_R:
            L = CHUNK * (C - 1) + r
            if 8 <= L <= WHOLE_MSG_MAX:
                cases.append((C, r, L))
    assert len(cases) == SWEEP_A_COUNT == 6 + 99 * 7 + 1
    assert [c for c in cases if c[0] == 101] == [(101, 1, 102401)]
    assert all((L + CHUNK - 1) // CHUNK == C for C, _, L in cases)
    assert sorted({(C + 1) // 2 for C, _, _ in cases}) == list(range(1, 52))  # every pair count
    assert sum(L for _, _, L in cases) < 40 * 1000 * 1000
    return cases


def sweep_a_small():
    """The cases of sweep_a with C <= 9 (one merge pass of <= 5 pair nodes): 6 + 8 x 7."""
    cases = [c for c in sweep_a() if c[0] <= 9]
    assert len(cases) == 62
    return cases


def cas_files(cases, cid0: int = 1000):
    """(sizes u64, cids u64, twins u32) of the synthetic files whose cas messages are `cases`."""
    sizes = np.array([L - 8 for _, _, L in cases], np.uint64)
    return sizes, np.arange(cid0, cid0 + len(cases), dtype=np.uint64), np.zeros(len(cases), np.uint32)


def sampled_files(n: int = 300, cid0: int = 5000):
    """n sampled-kind files (size > 102400) to interleave with a whole-file list."""
    sizes = np.uint64(102401) + np.arange(n, dtype=np.uint64) * np.uint64(4099)
    return sizes, np.arange(cid0, cid0 + n, dtype=np.uint64), np.zeros(n, np.uint32)


def interleave(a, b, seed: int):
    """Two (sizes, cids, twins) lists merged, the files of b at seeded random rows and each
    list in its own order -> (sizes, cids, twins, is_b)."""
    na, nb = len(a[0]), len(b[0])
    is_b = np.zeros(na + nb, bool)
    is_b[np.random.default_rng(seed).choice(na + nb, nb, replace=False)] = True
    out = []
    for x, y in zip(a, b):
        z = np.empty(na + nb, x.dtype)
        z[~is_b], z[is_b] = x, y
        out.append(z)
    return out[0], out[1], out[2], is_b


# ------------------------------------------------------- B: checksum leaf / reduce shapes
SWEEP_B_R = (1, 64, 65, 1023, 1024)
# chunk counts of one 1 MiB block at which every r is taken: one lane, the first odd carries,
# and each side of the 16-, 64-, 256- and 512-chunk subtrees and of the full block
SWEEP_B_ALL_R = tuple(list(range(1, 10)) + [15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513]
                      + list(range(1019, 1025)))
SWEEP_B_COUNT = 1024 + 4 * len(SWEEP_B_ALL_R)  # 1132


def sweep_b_block():
    """Files inside one 1 MiB block: every chunk count C = 1..1024, length 1024 (C - 1) + r
    with r rotating through SWEEP_B_R by C, and all five r for C in SWEEP_B_ALL_R
    -> [(C, r, length)]."""
    assert len(SWEEP_B_ALL_R) == 27
    cases = []
    for C in range(1, 1025):
        for r in (SWEEP_B_R if C in SWEEP_B_ALL_R else (SWEEP_B_R[C % 5],)):
            cases.append((C, r, CHUNK * (C - 1) + r))
    assert len(cases) == SWEEP_B_COUNT == 1132
    assert sorted({C for C, _, _ in cases}) == list(range(1, 1025))
    assert {((C + 3) // 4) for C, _, _ in cases} == set(range(1, 257))  # every lanes_b
    assert max(L for _, _, L in cases) == MiB and min(L for _, _, L in cases) == 1
    return cases


def sweep_b_stride():
    """The part of sweep_b_block the CPU tests run: the all-r classes and every C that is a
    multiple of 37."""
    cases = [c for c in sweep_b_block() if c[0] in SWEEP_B_ALL_R or c[0] % 37 == 0]
    assert len(cases) == 5 * 27 + 27  # 37 .. 999, none of them an all-r class
    return cases


def sweep_b_pairs():
    """Two unrelated files that share a leaf workgroup, each pair in both orders: a 1-byte
    file beside a full block, an empty file beside a 1021-chunk one."""
    a, b = (1, MiB), (0, CHUNK * 1020 + 5)
    return [a, a[::-1], b, b[::-1]]


def sweep_b_last_blocks():
    """Multi-block files whose last block holds C chunks, the last of r bytes."""
    lens = [b * MiB + CHUNK * (C - 1) + r for b in (1, 2, 3) for C in (1, 2, 3, 4, 5, 1023) for r in (1, CHUNK)]
    assert len(lens) == 36
    return lens


def sweep_b_reduce():
    """Block counts that are not powers of two, one either side of them, and one byte short."""
    lens = [b * MiB - d for b in (2, 3, 5, 7, 8, 9, 15, 16, 17, 33) for d in (0, 1)]
    assert len(lens) == 20
    return lens


def place(lens, align: int = 128, gap: int = 64):
    """Offsets of ranges laid one after the other, each on `align` with at least `gap` bytes
    after the one before -> (offsets, total buffer bytes)."""
    offs, off = [], 0
    for L in lens:
        offs.append(off)
        off = (off + int(L) + gap + align - 1) // align * align
    return offs, off + 64


# ------------------------------------------------------------------ C: packed ranges
PACKED_SMALL = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, MiB - 1)
PACKED_BIG = (MiB, MiB + 1, 2 * MiB + 5)


def packed_ranges():
    """About 60 byte ranges packed into one buffer with gaps of 0..48 bytes: every length of
    PACKED_SMALL and PACKED_BIG, every start 16-byte aligned, every residue 0, 16 .. 112 mod
    128 the start of a range of >= 1 MiB -> (offsets, lens, buffer bytes); the buffer ends 64
    bytes after the last range."""
    offs, lens = [], []
    end = 0
    small = iter(PACKED_SMALL * 8)

    def put(L, steps):
        nonlocal end
        start = (end + 15) // 16 * 16 + 16 * steps
        assert 0 <= start - end <= 48
        offs.append(start)
        lens.append(L)
        end = start + L

    for k, res in enumerate(range(0, 128, 16)):
        for j in range(4):
            put(next(small), (k + j) % 3)
        # 16-byte shims (no gap: the neighbour's bytes follow directly) until the residue is
        # at most two 16-byte steps away
        while (res - (end + 15) // 16 * 16) % 128 > 32:
            put((16, 15, 1)[len(offs) % 3], 0)
        put(PACKED_BIG[k % 3], (res - (end + 15) // 16 * 16) % 128 // 16)
        assert offs[-1] % 128 == res
    put(1, 0)
    offs_a, lens_a = np.array(offs, np.uint64), np.array(lens, np.uint64)
    assert 50 <= len(offs) <= 70, len(offs)
    assert set(PACKED_SMALL) | set(PACKED_BIG) <= set(lens)
    assert not (offs_a % np.uint64(16)).any()
    assert {int(o) % 128 for o, L in zip(offs, lens) if L >= MiB} == set(range(0, 128, 16))
    gaps = offs_a[1:] - (offs_a[:-1] + lens_a[:-1])
    assert gaps.max() <= 48 and (gaps == 0).any()  # unsigned: an overlap would wrap to 2^64
    return offs_a, lens_a, end + 64


def range_mask(offs, lens, total: int) -> np.ndarray:
    """True for every buffer byte that lies inside some range."""
    m = np.zeros(total, bool)
    for o, L in zip(offs, lens):
        m[int(o):int(o) + int(L)] = True
    return m


def pack_messages(lens):
    """Offsets for cas messages at 16-byte aligned starts that are not stage_plan's: message
    k starts 16 (k % 4) bytes after the 64-byte boundary that ends the zero padding of the
    one before -> (offsets, total bytes)."""
    offs, end = [], 0
    for k, L in enumerate(lens):
        start = (end + 63) // 64 * 64 + 16 * (k % 4)
        offs.append(start)
        end = start + int(L)
    return np.array(offs, np.uint64), (end + 63) // 64 * 64 + 64


def message_surroundings(offs, lens, total: int) -> np.ndarray:
    """True for the bytes a cas batch may not depend on: everything but the messages and
    their zero padding up to the next 64-byte boundary."""
    m = np.ones(total, bool)
    for o, L in zip(offs, lens):
        m[int(o):(int(o) + int(L) + 63) // 64 * 64] = False
    return m


# ------------------------------------------------------------------ D: guarded dedup sizes
GROUP_M = (0, 1, 2, 63, 64, 65, 511, 512, 513, 1000)

# ------------------------------------------------------------------ F: partition
PART_NPARTS = (1, 2, 3, 7, 8, 63, 64)
PART_N = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)
PART_BASES = (0, (1 << 40) + 3)
PART_MASKS = ("ones", "zeros", "random", "none")
PART_CASES_PER_NPARTS = len(PART_N) * len(PART_BASES) * len(PART_MASKS)  # 96


def crafted_keys(nparts: int):
    """cas_id keys (Python ints) at the extremes of u64 and one either side of every
    destination boundary floor(k 2^64 / nparts)."""
    keys = [0, 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64]
    for k in range(nparts):
        edge = (k << 64) // nparts
        keys += [(edge - 1) & M64, edge & M64, (edge + 1) & M64]
    assert len(keys) == 6 + 3 * nparts
    return keys


def dest_of_int(key: int, nparts: int) -> int:
    """sd_dedup_partition's destination of one key, in Python integers."""
    return ((key >> 48) * nparts) >> 16


def partition_keys(nparts: int, n: int, seed: int) -> np.ndarray:
    """n keys (u64): the crafted ones first, random ones after; where n is smaller than the
    crafted list, a seeded sample of it."""
    rng = np.random.default_rng(seed)
    crafted = np.array(crafted_keys(nparts), np.uint64)
    if n <= len(crafted):
        return crafted[np.sort(rng.choice(len(crafted), n, replace=False))]
    rest = rng.integers(0, 1 << 64, n - len(crafted), dtype=np.uint64)
    return np.concatenate([crafted, rest])


def hashes_from_keys(keys: np.ndarray, seed: int) -> np.ndarray:
    """n x 32 hash rows whose first 8 bytes are the keys, big-endian; the rest random."""
    h = np.random.default_rng(seed).integers(0, 256, (len(keys), 32), dtype=np.uint8)
    h[:, :8] = keys.astype(">u8").view(np.uint8).reshape(-1, 8)
    return h


def partition_mask(kind: str, n: int, seed: int):
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones(n, np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    assert kind == "random"
    return np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8)


def partition_cases(nparts: int):
    """The PART_CASES_PER_NPARTS cases of one nparts -> [(n, base, mask kind, keys, hash32,
    valid or None)]."""
    out = []
    for n in PART_N:
        keys = partition_keys(nparts, n, 1000 * nparts + n)
        h = hashes_from_keys(keys, n + 1)
        for base in PART_BASES:
            for kind in PART_MASKS:
                out.append((n, base, kind, keys, h, partition_mask(kind, n, 7 * n + nparts)))
    assert len(out) == PART_CASES_PER_NPARTS == 96
    return out
