"""Cases for the content-defined chunks (include/sd_cas.h: sd_cdc_*, sd_cpu_cdc_*), shared by
tests/test_cdc.py (the host twins, the wrappers) and tests/test_gpu_cdc.py (the kernels).  Every
builder asserts the premise it exists for, so a wrong edit cannot quietly shrink the sweep.

A case is (name, buf uint8, offs uint64 [n], lens uint64 [n], params (mask_bits, min, max)).  The
buffer carries random bytes, not zeros, in every gap, in every padding and after the last range.

The rule is restated here in numpy from the header's words, not from either implementation: the
gear table from oracle.cas_spec.splitmix64, the rolling value as the sum over the last 64 bytes
(six doubling steps), candidates, the selection walk, the statistics.  The ids come from the
oracle's BLAKE3.  Content is searched for candidates and sliced so that one lands where a case
wants it.

Nothing here touches a device or the library.
"""
from __future__ import annotations

import os
import re

import numpy as np

from oracle import cas_spec as cs

U = np.uint64
P8, P10, PDEF, PBIG = (8, 64, 1024), (10, 256, 4096), (16, 16384, 262144), (20, 65536, 1 << 20)
PARAM_SETS = (P8, P10, PDEF, PBIG)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spacedrive_amd", "csrc")


def scan_tile() -> int:
    """CDC_TILE of cdc.hip: the bytes of one workgroup's tile of the scan"""
    found = re.findall(r"^constexpr\s+uint32_t\s+CDC_TILE\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, "cdc.hip")).read(), re.M)
    assert len(found) == 1
    return int(found[0])


def select_words() -> int:
    """CDC_SELECT_WORDS of cdc.hip: the bitmap words one step of the select's wave looks at"""
    found = re.findall(r"^constexpr\s+uint32_t\s+CDC_SELECT_WORDS\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, "cdc.hip")).read(), re.M)
    assert len(found) == 1
    return int(found[0])


# ---------------------------------------------------------------- the rule
def gear() -> np.ndarray:
    return cs.splitmix64(U(0x5DCDC0DE) ^ np.arange(256, dtype=U))


GEAR = gear()


def rolling(g: np.ndarray) -> np.ndarray:
    """h(i) = the sum over k = 0 .. min(i, 63) of g[i - k] << k, mod 2^64; g = GEAR[bytes]"""
    h = g.astype(U).copy()
    with np.errstate(over="ignore"):
        for step in (1, 2, 4, 8, 16, 32):  # after the step h covers 2 * step bytes
            nxt = h.copy()
            nxt[step:] += h[:-step] << U(step)
            h = nxt
    return h


def mask_of(mask_bits: int) -> np.uint64:
    return U(((1 << mask_bits) - 1) << (64 - mask_bits))


def candidates(data: np.ndarray, mask_bits: int) -> np.ndarray:
    """bool per position of one file"""
    if len(data) == 0:
        return np.zeros(0, bool)
    return (rolling(GEAR[data]) & mask_of(mask_bits)) == 0


def select(cand: np.ndarray, length: int, mn: int, mx: int):
    """-> chunks [(offset, length)], kinds [at a candidate, forced, at the file's end]"""
    ends = np.flatnonzero(cand) + 1
    chunks, kinds, s = [], [0, 0, 0], 0
    while True:
        i = int(np.searchsorted(ends, s + mn))
        hit = i < len(ends) and int(ends[i]) <= s + mx
        e = min(int(ends[i]) if hit else s + mx, length)
        kinds[2 if e == length else 0 if hit else 1] += 1
        chunks.append((s, e - s))
        s = e
        if e == length:
            return chunks, kinds


def compressions(length: int) -> int:
    if length == 0:
        return 1
    blocks = sum((min(1024, length - o) + 63) // 64 for o in range(0, length, 1024))
    return blocks + (length + 1023) // 1024 - 1


def model(buf, offs, lens, params, packed: bool = False) -> dict:
    """-> base uint64 [n + 1], chunks uint64 [m, 2], stats uint64 [8], cand (list of bool arrays).
    packed: the ranges lie at least 63 bytes apart, so one pass over the buffer with the gaps' gear
    values zeroed gives every file's rolling values at once."""
    mask_bits, mn, mx = params
    n = len(lens)
    cands = []
    if packed and n:
        inside = np.zeros(len(buf), bool)
        order = np.argsort(offs)
        ends = (offs + lens)[order].astype(np.int64)
        assert (offs[order][1:].astype(np.int64) - ends[:-1] >= 63).all()
        for o, L in zip(offs, lens):
            inside[int(o):int(o) + int(L)] = True
        g = GEAR[buf]
        g[~inside] = 0
        c = (rolling(g) & mask_of(mask_bits)) == 0
        cands = [c[int(o):int(o) + int(L)] for o, L in zip(offs, lens)]
    else:
        cands = [candidates(buf[int(o):int(o) + int(L)], mask_bits) for o, L in zip(offs, lens)]
    base, chunks, kinds, ncand, comp = [0], [], [0, 0, 0], 0, 0
    for c, L in zip(cands, lens):
        ch, k = select(c, int(L), mn, mx)
        chunks += ch
        kinds = [a + b for a, b in zip(kinds, k)]
        ncand += int(c.sum())
        comp += sum(compressions(ln) for _, ln in ch)
        base.append(len(chunks))
    stats = [n, int(np.asarray(lens, U).sum()) if n else 0, ncand, len(chunks), kinds[0], kinds[1], kinds[2], comp]
    return {"base": np.array(base, U), "chunks": np.array(chunks, U).reshape(-1, 2), "stats": np.array(stats, U),
            "cand": cands}


def oracle_ids(buf, offs, base, chunks) -> np.ndarray:
    """the oracle's BLAKE3 of every chunk's bytes, uint8 [m, 32]"""
    from oracle import native
    m = len(chunks)
    if m == 0:
        return np.zeros((0, 32), np.uint8)
    file_of = np.repeat(np.arange(len(base) - 1), np.diff(base.astype(np.int64)))
    starts = np.asarray(offs, U)[file_of] + chunks[:, 0]
    return native.checksums(np.ascontiguousarray(buf), starts, np.ascontiguousarray(chunks[:, 1]), nthreads=8).reshape(m, 32)


def shared_model(base, chunks, ids, min_chunks: int = 0) -> dict:
    """the header's contract for sd_cdc_shared -> rep, size, files, pairs, stats"""
    n, m = len(base) - 1, len(chunks)
    file_of = np.repeat(np.arange(n), np.diff(np.asarray(base).astype(np.int64))) if n else np.zeros(0, np.int64)
    rows = np.zeros((m, 40), np.uint8)
    rows[:, :8] = chunks[:, 1].astype(">u8").view(np.uint8).reshape(m, 8)
    rows[:, 8:] = ids
    if m:
        _, first, inv, cnt = np.unique(rows.view(np.dtype((np.void, 40))).reshape(-1), return_index=True,
                                       return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        rep, size = first[inv], cnt[inv]
        classes, classes2 = len(first), int((cnt >= 2).sum())
    else:
        rep, size, classes, classes2 = np.zeros(0, np.int64), np.zeros(0, np.int64), 0, 0
    files = [[int(base[f + 1] - base[f]), 0, 0, 0] for f in range(n)]
    pair, own = {}, 0
    for s in range(m):
        f, by = int(file_of[s]), int(chunks[s, 1])
        files[f][1] += size[s] >= 2
        if rep[s] != s:
            files[f][2] += 1
            files[f][3] += by
            g = int(file_of[rep[s]])
            assert g <= f
            if g == f:
                own += 1
                continue
            row = pair.setdefault((f, g), [0, 0])
            row[0] += 1
            row[1] += by
    need = max(1, int(min_chunks))
    pairs = [(f, g, b, y) for (f, g), (b, y) in sorted(pair.items()) if b >= need]
    stats = [n, m, classes, classes2, sum(r[2] for r in files), sum(r[3] for r in files), sum(1 for r in files if r[2]), own]
    return {"rep": np.asarray(rep, U), "size": np.asarray(size, U), "files": np.array(files, U).reshape(-1, 4),
            "pairs": np.array(pairs, U).reshape(-1, 4), "stats": np.array(stats, U)}


def check_identities(got: dict, min_chunks: int = 0) -> None:
    """tree_shared_cases.check_identities for chunks: a file may repeat a chunk of its own"""
    st = [int(x) for x in got["stats"]]
    files, pairs = got["files"], got["pairs"]
    assert st[4] == st[1] - st[2] == (int(files[:, 2].sum()) if len(files) else 0), st
    assert st[5] == (int(files[:, 3].sum()) if len(files) else 0), st
    assert st[3] <= st[2] <= st[1] and st[7] <= st[4] and st[6] <= st[0], st
    if len(files):
        assert int(files[:, 0].sum()) == st[1]
    if min_chunks <= 1:
        assert int(pairs[:, 2].sum()) == st[4] - st[7], st  # the rows leave out what a file repeats of itself
    if len(pairs):
        assert (pairs[:, 1] < pairs[:, 0]).all()
        order = [(int(f), int(g)) for f, g in pairs[:, :2]]
        assert order == sorted(set(order))


# ---------------------------------------------------------------- builders
def synth(cid: int, length: int, offset: int = 0) -> np.ndarray:
    return np.frombuffer(cs.synth_bytes(cid, 0, offset, length), np.uint8)


def pack(files, seed: int, gaps=None):
    """the files at 16-byte aligned starts a random number of 16-byte units apart (gaps: the units
    between the end of file i and the start of file i + 1, rounded up), random bytes around them"""
    rng = np.random.default_rng(seed)
    offs, cur = [], 16 * int(rng.integers(0, 4))
    for i, f in enumerate(files):
        offs.append(cur)
        gap = int(rng.integers(0, 9)) if gaps is None else gaps[i]
        cur = (cur + len(f) + 15) // 16 * 16 + 16 * gap
    total = (cur + 63) // 64 * 64 + 64
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    for f, o in zip(files, offs):
        buf[o:o + len(f)] = f
    return buf, np.array(offs, U), np.array([len(f) for f in files], U)


class Content:
    """synthetic content and its candidates under one mask: slices with a candidate where wanted"""

    def __init__(self, cid: int, length: int, mask_bits: int):
        self.data = synth(cid, length)
        self.pos = np.flatnonzero(candidates(self.data, mask_bits))

    def first_at(self, p: int, length: int, skip: int = 0) -> np.ndarray:
        """a slice of `length` bytes whose first candidate at a position >= 63 lies at position p"""
        assert p >= 63
        gap = np.diff(self.pos)
        ok = np.flatnonzero((gap > p - 63) & (self.pos[1:] >= p) & (self.pos[1:] - p + length <= len(self.data)))
        assert len(ok) > skip, "no such slice in this content"
        c = int(self.pos[1:][ok[skip]])
        out = self.data[c - p:c - p + length]
        rel = self.pos[(self.pos >= c - p + 63) & (self.pos < c - p + length)] - (c - p)  # a position from 63 on sees
        assert int(rel[0]) == p                                                          # the same 64 bytes in the slice
        return out


def all_zero_has_no_candidate() -> bool:
    return (int(GEAR[0]) * -1) % (1 << 64) >> 63 == 1  # the steady rolling value of zeros is -G[0]


def dense_byte(mask_bits: int) -> int:
    """a byte b whose constant file has a candidate at every position from 63 on: (-G[b]) & MASK == 0"""
    hits = [b for b in range(256) if ((-int(GEAR[b])) % (1 << 64)) >> (64 - mask_bits) == 0]
    assert hits, "no dense byte at this mask"
    return hits[0]


_CACHE: dict = {}


def _content(mask_bits: int) -> Content:
    key = ("content", mask_bits)
    if key not in _CACHE:
        _CACHE[key] = Content(11, 2 << 20, mask_bits)
    return _CACHE[key]


def selection_cases():
    mb, mn, mx = P10
    c = _content(mb)
    wide = (mb, mn, 8192)
    lo = mn - 1  # the first bit a step of the select looks at, for s = 0
    out = [
        ("cand_at_min_minus_1", [c.first_at(mn - 2, 3000)], P10),   # end = min - 1: ignored
        ("cand_at_min", [c.first_at(mn - 1, 3000)], P10),           # end = min: taken
        ("cand_at_max", [c.first_at(mx - 1, mx + 900)], P10),       # end = max: taken, a candidate's cut
        ("cand_at_len", [c.first_at(1999, 2000)], P10),             # end = len
        ("none_in_window", [c.first_at(mx + 10, mx + 900)], P10),   # forced
        ("two_forced", [np.concatenate([np.zeros(2 * mx + 100, np.uint8), c.data[:3000]])], P10),
    ]
    for d in (64 * 64 - 1, 64 * 64, 64 * 64 + 1):  # bits after s + min_size - 1 ... and after s + min_size
        out.append((f"select_step_{d}", [c.first_at(lo + d, lo + d + 700), c.first_at(lo + 1 + d, lo + d + 700, 1)], wide))
    edge = ((lo >> 6) + 64) * 64  # the first bit of the wave's second step
    out.append(("select_step_word_edge", [c.first_at(edge - 1, edge + 500), c.first_at(edge, edge + 500, 1)], wide))
    # the first bit of the wave's second round of loads: zeros (no candidate) up to 100 bytes before it
    outer = ((lo >> 6) + select_words()) * 64
    out.append(("select_step_outer_edge", [np.concatenate([np.zeros(outer - 1 - 100, np.uint8), c.first_at(100, 700)]),
                                           np.concatenate([np.zeros(outer - 100, np.uint8), c.first_at(100, 700, 1)])],
                (mb, mn, 2 * outer)))
    return out


def tile_cases():
    T = scan_tile()
    c = _content(8)
    big = c.pos[(c.pos >= 2 * T) & (c.pos + T + 200 < len(c.data))]
    files = [c.data[int(big[0]) - (T - 1):int(big[0]) + 200],        # a candidate at the tile's last position
             c.data[int(big[1]) - T:int(big[1]) + 200],              # at the next tile's first position
             c.data[int(big[2]) - (2 * T - 1):int(big[2]) + 1]]      # at the last position of tile 1 = the file's end
    lens = [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
    return [("tile_edges", files, P8), ("tile_lens", [synth(20 + i, L) for i, L in enumerate(lens)], P8)]


def length_cases():
    out = []
    for name, (mb, mn, mx) in (("p8", P8), ("p10", P10)):
        lens = sorted({0, 1, 63, 64, 65, mn - 1, mn, mn + 1, mx, mx + 1})
        out.append((f"lengths_{name}", [synth(40 + i, L) for i, L in enumerate(lens)], (mb, mn, mx)))
    return out


def bitmap_cases():
    b = dense_byte(4)
    assert all_zero_has_no_candidate()
    return [
        ("all_zero", [np.zeros(3 * 1024 + 17, np.uint8)], P8),
        ("dense", [np.full(64 * 5 + 3, b, np.uint8), np.full(700, b, np.uint8)], (4, 64, 1024)),
        ("mask1_64_64", [synth(60, 1000), synth(61, 4097)], (1, 64, 64)),
        ("mask1_64_128", [synth(62, 1000), synth(63, 4097)], (1, 64, 128)),
        ("mask32", [synth(64, 5000)], (32, 64, 1024)),
    ]


HASH_LENS = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193)


def hash_cases():
    return [
        ("hash_lens", [synth(70 + i, L) for i, L in enumerate(HASH_LENS)], PBIG),  # shorter than min: one chunk each
        ("hash_big", [synth(90, (1 << 20) + 100), synth(91, 255 * 4096), synth(92, (1 << 20) - 1)], (32, 65536, 1 << 20)),
        ("params_p8", [synth(93, 40000), synth(94, 7777)], P8),
        ("params_p10", [synth(95, 150000)], P10),
        ("params_default", [synth(96, 2 << 20), synth(97, 300000)], PDEF),
        ("params_big", [synth(98, 3 << 20)], PBIG),
    ]


def shift_files():
    """A, 5 bytes + A, A with 5 bytes in its middle, A twice (all of it held by A first)"""
    key = "shift"
    if key not in _CACHE:
        A = synth(7, 1 << 20)
        ins = np.arange(1, 6, dtype=np.uint8)
        _CACHE[key] = [A, np.concatenate([ins, A]), np.concatenate([A[:500000], ins, A[500000:]]), np.concatenate([A, A])]
    return _CACHE[key]


def start_cases():
    """a 16-byte file and, 16 bytes after its start, the bytes of a stand-alone file; and that file alone"""
    body = _content(8).data[5000:5000 + 9000]
    head = synth(99, 16)
    return [("starts_pair", [head, body], P8, [0, 0]), ("starts_alone", [body], P8, None)]


def many_cases():
    n_chunks = 1024 * 256 + 1
    rng = np.random.default_rng(77)
    small = [synth(1000 + i, int(L)) for i, L in enumerate(rng.integers(1, 201, 70_000))]
    return [("many_chunks", [synth(100, 64 * n_chunks)], (1, 64, 64), None, False),
            ("many_files", small, (4, 64, 128), [4] * len(small), True)]  # 64 bytes and more between ranges


def all_cases(many: bool = False):
    """[(name, buf, offs, lens, params, want)], want = model(...) with "ids" from the oracle.  The
    two `many` cases come only when asked for: they take a few seconds to build."""
    key = ("cases", many)
    if key in _CACHE:
        return _CACHE[key]
    raw = []
    for i, c in enumerate(length_cases() + selection_cases() + bitmap_cases() + tile_cases() + hash_cases()):
        raw.append(c + (None, False))
    raw += [c + (False,) for c in start_cases()]
    raw.append(("shift", shift_files(), P10, None, False))
    half = shift_files()[0][:1 << 18]  # a file that holds its content twice and holds it first, then the content
    raw.append(("twice", [np.concatenate([half, half]), half], P10, None, False))
    if many:
        raw = many_cases()
    out = []
    for i, (name, files, params, gaps, packed) in enumerate(raw):
        buf, offs, lens = pack(files, 300 + i, gaps)
        want = model(buf, offs, lens, params, packed)
        want["ids"] = oracle_ids(buf, offs, want["base"], want["chunks"])
        out.append((name, buf, offs, lens, params, want))
    if not many:
        check_premises({c[0]: c for c in out})
    _CACHE[key] = out
    return out


def check_premises(by: dict) -> None:
    """what each case exists for, said of the restatement's answer"""
    def first(name, f=0):
        w = by[name][5]
        return [int(x) for x in w["chunks"][int(w["base"][f])]]
    mb, mn, mx = P10
    assert by["cand_at_min_minus_1"][5]["cand"][0][mn - 2] and first("cand_at_min_minus_1")[1] > mn
    assert first("cand_at_min") == [0, mn]
    assert first("cand_at_max") == [0, mx] and by["cand_at_max"][5]["cand"][0][mx - 1]
    assert by["cand_at_max"][5]["stats"][4:7].tolist() == [1, 0, 1]  # a candidate's cut, not a forced one
    w = by["cand_at_len"][5]
    assert w["cand"][0][-1] and int(w["stats"][6]) == 1 and int(w["chunks"][-1].sum()) == 2000
    assert first("none_in_window") == [0, mx] and not by["none_in_window"][5]["cand"][0][mn - 1:mx].any()
    w = by["two_forced"][5]
    assert w["chunks"][:2].tolist() == [[0, mx], [mx, mx]] and int(w["stats"][5]) >= 2
    lo = mn - 1
    for d in (4095, 4096, 4097):
        assert first(f"select_step_{d}") == [0, lo + d + 1] and first(f"select_step_{d}", 1) == [0, lo + d + 2]
    edge = ((lo >> 6) + 64) * 64
    assert first("select_step_word_edge") == [0, edge] and first("select_step_word_edge", 1) == [0, edge + 1]
    outer = ((lo >> 6) + select_words()) * 64
    assert select_words() > 64 and first("select_step_outer_edge") == [0, outer] and first("select_step_outer_edge", 1) == [0, outer + 1]
    w = by["all_zero"][5]
    assert not w["cand"][0][63:].any() and w["chunks"][:3, 1].tolist() == [1024] * 3  # none once 64 zeros are in
    w = by["dense"][5]
    assert w["cand"][0][63:].all() and w["chunks"][:5, 1].tolist() == [64] * 5
    assert set(by["mask1_64_64"][5]["chunks"][:-1, 1].tolist()) <= {64, 1000 % 64, 4097 % 64}
    T = scan_tile()
    c = by["tile_edges"][5]["cand"]
    assert c[0][T - 1] and c[1][T] and c[2][2 * T - 1] and (T - 1) % 64 == 63 and T % 64 == 0
    assert by["tile_lens"][3].tolist() == [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
    assert by["hash_lens"][5]["chunks"][:, 1].tolist() == list(HASH_LENS)
    big = by["hash_big"][5]["chunks"][:, 1].tolist()
    assert big == [1 << 20, 100, 255 * 4096, (1 << 20) - 1]  # 256, 1, 255 and 256 pieces; one chunk of exactly 1 MiB
    residues = set()
    for _, buf, offs, lens, params, w in by.values():
        file_of = np.repeat(np.arange(len(lens)), np.diff(w["base"].astype(np.int64)))
        residues |= set(((offs[file_of] + w["chunks"][:, 0]) % U(16)).tolist())
    assert residues == set(range(16)), residues
    a, b = by["starts_pair"], by["starts_alone"]
    assert int(a[2][1]) - int(a[2][0]) == 16 and int(a[3][0]) == 16
    k = int(a[5]["base"][1])
    assert np.array_equal(a[5]["chunks"][k:], b[5]["chunks"]) and np.array_equal(a[5]["ids"][k:], b[5]["ids"])
