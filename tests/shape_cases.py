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
# record counts m, not bucket sizes: uniform keys leave every LDS bucket at or under a wave
# (the bucket sizes themselves are D2's)
GROUP_M = (0, 1, 2, 63, 64, 65, 511, 512, 513, 1000)

# ------------------------------------------- D2: the bucket sizes of the LDS-bucket grouping
# The bucket arithmetic of dedup.hip (gb_lg, k_gb_final, k_gb_split) restated, so that every
# case below can assert which branch of k_gb_sort / k_gb_sort_big its buckets take:
#   s <= 64 registers | s <= GB_CAP one wave in LDS | s <= GB_BIG_CAP k_gb_sort_big | overflow
# tests/test_shape_cases.py compares these constants with the ones in dedup.hip.
GB_CAP = 128
GB_BIG_CAP = 4096
GB_BIG_GRID = 128
GB_PER_BUCKET = 48  # gb_lg: nb = 2^lg >= m / 48
GB_LG_MAX = 24
GB_FILLER = 200  # records of bucket_case outside the target bucket, besides the two sentinels

BUCKET_S = (1, 2, 3, 32, 33, 63, 64, 65, 96, 127, 128, 129, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049,
            4095, 4096, 4097)
# layout -> the smallest s at which it differs from the layouts before it
BUCKET_LAYOUTS = {"singles": 1, "one": 2, "late": 3, "pairs": 4, "pairs_shifted": 5, "late5": 7}
BUCKET_CASES_PER_LAYOUT = {"singles": 23, "one": 22, "late": 21, "pairs": 20, "pairs_shifted": 20, "late5": 20}


def gb_lg(m: int) -> int:
    """dedup.hip's gb_lg: the fewest bits lg >= 1 with 48 * 2^lg >= m, at most 24."""
    lg = 1
    while lg < GB_LG_MAX and (GB_PER_BUCKET << lg) < m:
        lg += 1
    return lg


def gb_buckets(keys: np.ndarray):
    """The bucket number of every key (u64) as k_gb_split computes it, (key - kmin) >> shift with
    k_gb_final's shift = max(bit length of (kmax - kmin) - lg, 0) -> (buckets int64, (lg, shift))."""
    keys = np.ascontiguousarray(keys, np.uint64)
    lg = gb_lg(len(keys))
    kmin = int(keys.min())
    bits = (int(keys.max()) - kmin).bit_length()
    shift = bits - lg if bits > lg else 0
    return ((keys - np.uint64(kmin)) >> np.uint64(shift)).astype(np.int64), (lg, shift)


def gb_bucket_sizes(keys: np.ndarray) -> np.ndarray:
    """Records per bucket, all 2^lg of them."""
    bk, (lg, _) = gb_buckets(keys)
    assert 0 <= bk.min() and bk.max() < (1 << lg)
    return np.bincount(bk, minlength=1 << lg)


def bucket_runs(s: int, layout: str):
    """The runs of equal keys, in sorted order, of a bucket of s records."""
    assert s >= BUCKET_LAYOUTS[layout], (s, layout)
    if layout == "singles":
        runs = [1] * s
    elif layout == "one":  # the head at position 0
        runs = [s]
    elif layout == "late":  # the head at position 1: no later chunk has a head of its own
        runs = [1, s - 1]
    elif layout == "pairs":  # a head on every multiple of 64
        runs = [2] * (s // 2) + [1] * (s % 2)
    elif layout == "pairs_shifted":  # a group across every multiple of 64
        runs = [1] + [2] * ((s - 1) // 2) + [1] * ((s - 1) % 2)
    else:
        assert layout == "late5"
        runs = [1] * 5 + [s - 5]
    assert sum(runs) == s and min(runs) >= 1
    starts = np.cumsum([0] + runs[:-1])
    if layout == "pairs" and s > 64:
        assert all(p in starts for p in range(0, s, 64))
    if layout == "pairs_shifted" and s > 65:
        assert not any(p in starts for p in range(64, s - 1, 64))
    return runs


def _keys_in_bucket(b: int, shift: int, runs, rng) -> np.ndarray:
    """sum(runs) keys of bucket b (kmin = 0): len(runs) distinct ones, among them the bucket's
    first and (two or more) last key, the k-th smallest repeated runs[k] times."""
    nd = len(runs)
    low = set([0, (1 << shift) - 1][:nd])
    while len(low) < nd:
        low.update(int(x) for x in rng.integers(0, 1 << shift, nd - len(low), dtype=np.uint64))
    keys = np.array(sorted(low), np.uint64) + np.uint64(b << shift)
    return np.repeat(keys, runs)


def _with_indices(keys: np.ndarray, index_sorted: bool, base: int, rng) -> np.ndarray:
    """Records (key, index) int64 [m, 2] of the keys in a seeded shuffle; the indices base + 3 i +
    5 are distinct, ascending in input order when index_sorted and otherwise a permutation, in
    which the first group's smallest index is not on its first record in input order."""
    m = len(keys)
    keys = keys[rng.permutation(m)]
    i = np.arange(m, dtype=np.int64) if index_sorted else rng.permutation(m).astype(np.int64)
    uniq, cnt = np.unique(keys, return_counts=True)
    if not index_sorted and (cnt > 1).any():
        at = np.nonzero(keys == uniq[np.argmax(cnt > 1)])[0]  # ascending: input order
        lowest = at[np.argmin(i[at])]
        if lowest == at[0]:
            i[at[0]], i[at[1]] = i[at[1]], i[at[0]]
        assert i[at[0]] != i[at].min()
    idx = np.int64(base) + 3 * i + 5
    assert len(np.unique(idx)) == m and (not index_sorted or (np.diff(idx) > 0).all())
    return np.stack([keys.view(np.int64), idx], axis=1)


def bucket_case(s: int, layout: str, index_sorted: bool) -> np.ndarray:
    """Records (key, index) int64 [m, 2], m = s + 202, of which exactly one bucket -- a middle
    one -- holds exactly s, its runs of equal keys those of `layout`.  The sentinel keys 0 and
    2^64 - 1 pin kmin = 0 and shift = 64 - lg; GB_FILLER random keys are dealt over the other
    buckets, which all stay in the register path (<= 64)."""
    seed = 1000 * s + 10 * list(BUCKET_LAYOUTS).index(layout) + int(index_sorted)
    rng = np.random.default_rng(seed)
    m = s + 2 + GB_FILLER
    lg = gb_lg(m)
    nb, shift = 1 << lg, 64 - lg
    target = nb // 2
    others = [b for b in range(nb) if b != target]
    fill_b = np.array([others[j % len(others)] for j in range(GB_FILLER)], np.uint64)
    filler = (fill_b << np.uint64(shift)) | rng.integers(0, 1 << shift, GB_FILLER, dtype=np.uint64)
    runs = bucket_runs(s, layout)
    keys = np.concatenate([np.array([0, M64], np.uint64), filler, _keys_in_bucket(target, shift, runs, rng)])
    recs = _with_indices(keys, index_sorted, PART_BASES[(s + int(index_sorted)) % 2], rng)
    rk = recs[:, 0].view(np.uint64)
    sizes = gb_bucket_sizes(rk)
    bk, (lg2, shift2) = gb_buckets(rk)
    assert (lg2, shift2) == (lg, shift) and int(rk.min()) == 0 and len(recs) == m
    assert 0 < target < nb - 1 and sizes[target] == s and (sizes == s).sum() == 1
    assert np.delete(sizes, target).max() <= 64
    assert np.unique(rk[bk == target], return_counts=True)[1].tolist() == runs  # in key order
    return recs


def bucket_cases(layout: str):
    """Every (s, index_sorted) of one layout -> [(s, index_sorted, records)]; s = 4097, the
    overflow, with index_sorted among them."""
    out = [(s, srt, bucket_case(s, layout, srt)) for s in BUCKET_S if s >= BUCKET_LAYOUTS[layout] for srt in (False, True)]
    assert len(out) == 2 * BUCKET_CASES_PER_LAYOUT[layout]
    assert (GB_BIG_CAP + 1, True) in [(s, srt) for s, srt, _ in out]
    bases = {int(r[:, 1].min()) >= PART_BASES[1] for _, _, r in out}
    assert bases == {False, True}  # both index bases
    return out


assert sum(BUCKET_CASES_PER_LAYOUT.values()) == 126
assert all(sum(1 for s in BUCKET_S if s >= lo) == BUCKET_CASES_PER_LAYOUT[k] for k, lo in BUCKET_LAYOUTS.items())
# one size either side of every branch, and of the 1024-lane chunk and the two-pairs-per-lane step
assert all({c - 1, c, c + 1} <= set(BUCKET_S) for c in (64, GB_CAP, 1024, 2048, GB_BIG_CAP))


def _triples(b: int, shift: int, rng) -> np.ndarray:
    assert (GB_CAP + 1) % 3 == 0
    return _keys_in_bucket(b, shift, [3] * ((GB_CAP + 1) // 3), rng)


def many_big_case(index_sorted: bool = False) -> np.ndarray:
    """GB_BIG_GRID + 2 buckets of GB_CAP + 1 records, in triples of equal keys, and the two
    sentinels: more big buckets than k_gb_sort_big has workgroups, so two of them take a second."""
    nbig = GB_BIG_GRID + 2
    m = nbig * (GB_CAP + 1) + 2
    lg = gb_lg(m)
    shift = 64 - lg
    assert (1 << lg) >= 3 * nbig + 2
    rng = np.random.default_rng(77 + int(index_sorted))
    keys = np.concatenate([np.array([0, M64], np.uint64)] + [_triples(1 + 3 * q, shift, rng) for q in range(nbig)])
    recs = _with_indices(keys, index_sorted, PART_BASES[1], rng)
    sizes = gb_bucket_sizes(recs[:, 0].view(np.uint64))
    assert gb_buckets(keys)[1] == (lg, shift) and len(recs) == m
    assert (sizes > GB_CAP).sum() == nbig == GB_BIG_GRID + 2 and sizes.max() == GB_CAP + 1
    assert sorted(set(sizes.tolist())) == [0, 1, GB_CAP + 1]
    return recs


def all_big_case(index_sorted: bool = False) -> np.ndarray:
    """m = (GB_CAP + 1) 64 records, every one in a bucket of exactly GB_CAP + 1, the first and the
    last bucket (keys 0 and 2^64 - 1) among them: as many big buckets as m records can make, one
    short of the slots of the big[] list."""
    nbig = 64
    m = (GB_CAP + 1) * nbig
    lg = gb_lg(m)
    nb, shift = 1 << lg, 64 - lg
    rng = np.random.default_rng(79 + int(index_sorted))
    at = sorted({0, nb - 1} | {1 + (nb - 2) * q // (nbig - 2) for q in range(nbig - 2)})
    assert len(at) == nbig
    keys = np.concatenate([_triples(b, shift, rng) for b in at])
    recs = _with_indices(keys, index_sorted, PART_BASES[0], rng)
    sizes = gb_bucket_sizes(recs[:, 0].view(np.uint64))
    assert gb_buckets(keys)[1] == (lg, shift) and int(keys.min()) == 0 and int(keys.max()) == M64
    assert sorted(set(sizes.tolist())) == [0, GB_CAP + 1] and sizes[0] and sizes[-1]
    assert (sizes > GB_CAP).sum() == 64 <= m // (GB_CAP + 1) + 1 and m // (GB_CAP + 1) == 64
    return recs


SPAN_M = 1000
SPAN_COUNT = 45  # 11 spans x 4 kmin, and the full span, which only kmin = 0 leaves room for


def span_cases():
    """(key - kmin) >> shift over the spans and offsets at which it can go wrong: m = 1000 keys
    kmin + u, u in [0, span] with both ends present and duplicates from a pool of m / 2, for spans
    of 0..3 (shift 0, a few huge groups), either side of 2^lg (the first shift of 1), of 2^32 and
    of 2^63, and all of u64; kmin 0, 1, a high prefix and the largest that fits.  -> [(span,
    kmin, index_sorted, records)], index_sorted alternating."""
    m = SPAN_M
    lg = gb_lg(m)
    spans = [0, 1, 2, 3, (1 << lg) - 1, 1 << lg, (1 << lg) + 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, M64]
    out = []
    for span in spans:
        kmins = []
        for kmin in (0, 1, (0x1234 << 48) | 5, M64 - span):
            if kmin not in kmins and kmin + span <= M64:
                kmins.append(kmin)
        for kmin in kmins:
            rng = np.random.default_rng(len(out) + 500)
            pool = rng.integers(0, span, m // 2, dtype=np.uint64, endpoint=True)
            u = pool[rng.integers(0, len(pool), m)]
            u[:2] = (0, span)
            keys = np.uint64(kmin) + u
            srt = len(out) % 2 == 1
            recs = _with_indices(keys, srt, PART_BASES[(len(out) // 2) % 2], rng)
            bk, (lg2, shift) = gb_buckets(recs[:, 0].view(np.uint64))
            assert lg2 == lg and int(keys.min()) == kmin and int(keys.max()) == kmin + span
            assert bk.max() < (1 << lg) and shift == max(span.bit_length() - lg, 0)
            if span <= 3:
                assert shift == 0 and np.bincount(bk).max() >= GB_CAP + 1
            out.append((span, kmin, srt, recs))
    assert len(out) == SPAN_COUNT == 11 * 4 + 1
    assert {s for s, _, _, _ in out} == set(spans) and {srt for _, _, srt, _ in out} == {False, True}
    return out


LG_BORDER_M = (96, 97, 192, 193, 384, 385)


def lg_border_cases():
    """Record counts either side of the first three steps of gb_lg, uniform keys with duplicates
    -> [(m, index_sorted, records)]."""
    out = []
    for m in LG_BORDER_M:
        rng = np.random.default_rng(m)
        pool = rng.integers(0, M64, m // 2 + 1, dtype=np.uint64, endpoint=True)
        keys = pool[rng.integers(0, len(pool), m)]
        out.append((m, m % 2 == 1, _with_indices(keys, m % 2 == 1, PART_BASES[(m // 96) % 2], rng)))
    for lo, hi in zip(LG_BORDER_M[::2], LG_BORDER_M[1::2]):
        assert hi == lo + 1 and gb_lg(hi) == gb_lg(lo) + 1
    assert len(out) == 6
    return out

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
