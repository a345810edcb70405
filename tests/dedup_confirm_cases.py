"""Cases for the confirm step (include/sd_cas.h: sd_dedup_confirm, sd_cpu_dedup_confirm), shared
by tests/test_dedup_confirm.py (the host sibling, the numpy mirror, the Python wrappers) and
tests/test_gpu_dedup_confirm.py (the kernels, down both paths).  Every builder asserts the
premise it exists for (a class really crosses the border it is for), so a wrong edit cannot
quietly shrink the sweep.

A case is (name, keys uint64 [m], hashes uint8 [m, 32], valid uint8 [m] or None).

confirm_model is the rule as a dict of lists over Python integers and bytes: no sort of the
files, no numpy in the grouping.  has_tie says whether the prefix path can finish the case.

Nothing here touches a device or the library.
"""
from __future__ import annotations

import numpy as np

from tests.sliced_cases import BLOCKS, SLICE_COUNTS, TILE, slice_len

U = np.uint64
M64 = (1 << 64) - 1
INVALID, SINGLE, CONFIRMED, REFUTED = 0, 1, 2, 3
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513)
PAST_GRID = BLOCKS * TILE + 1  # every workgroup's slice holds more than one tile
MIX = 100_000


def confirm_model(keys, hashes, valid=None) -> dict:
    """group(i) = the valid j with keys[j] == keys[i]; class(i) = those with the same 32 bytes too.
    -> rep, size (uint64 [m]), verdict (uint8 [m]), sets (uint64 [n, 3]: key, rep, size; by key,
    then by the bytes as Python compares bytes objects = memcmp), stats (uint64 [8])."""
    m = len(keys)
    ks = [int(k) for k in keys]
    hs = [bytes(h) for h in np.asarray(hashes, np.uint8).reshape(m, 32)]
    ok = [True] * m if valid is None else [bool(v) for v in valid]
    groups, classes = {}, {}
    for i in range(m):
        if ok[i]:
            groups.setdefault(ks[i], []).append(i)
            classes.setdefault((ks[i], hs[i]), []).append(i)
    rep, size, verdict = [M64] * m, [0] * m, [INVALID] * m
    for (k, h), members in classes.items():
        for i in members:
            rep[i], size[i] = members[0], len(members)  # members were appended in ascending order
            verdict[i] = SINGLE if len(groups[k]) == 1 else CONFIRMED if len(members) >= 2 else REFUTED
    sets = [(k, mem[0], len(mem)) for (k, h), mem in sorted(classes.items()) if len(mem) >= 2]
    per_group = {}
    for (k, h) in classes:
        per_group[k] = per_group.get(k, 0) + 1
    cand = [k for k, g in groups.items() if len(g) >= 2]
    stats = [sum(ok), len(groups), len(cand), len(classes), len(sets), sum(s for _, _, s in sets),
             sum(1 for v in verdict if v == REFUTED), sum(1 for k in cand if per_group[k] >= 2)]
    return {"rep": np.array(rep, U), "size": np.array(size, U), "verdict": np.array(verdict, np.uint8),
            "sets": np.array(sets, U).reshape(-1, 3), "stats": np.array(stats, U)}


def has_tie(keys, hashes, valid=None) -> bool:
    """some valid files share their key and their first 8 checksum bytes and differ after them:
    what sends sd_dedup_confirm down the full-width path"""
    tails = {}
    h = np.asarray(hashes, np.uint8).reshape(len(keys), 32)
    for i in range(len(keys)):
        if valid is None or valid[i]:
            tails.setdefault((int(keys[i]), bytes(h[i, :8])), set()).add(bytes(h[i, 8:]))
    return any(len(t) >= 2 for t in tails.values())


def check_identities(stats) -> None:
    s = [int(x) for x in stats]
    assert s[0] == (s[1] - s[2]) + s[5] + s[6], s
    assert s[3] == (s[1] - s[2]) + s[4] + s[6], s
    assert s[7] <= s[2] <= s[1] <= s[0] and s[4] <= s[3] <= s[0], s


# ---------------------------------------------------------------- builders
def rand_hashes(rng, n: int) -> np.ndarray:
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def rand_keys(rng, n: int) -> np.ndarray:
    return rng.integers(0, 1 << 64, n, dtype=U)


def pooled(m: int, seed: int, with_valid: bool):
    """m files over about m / 3 keys with about two checksums each: singles, confirmed classes
    and refuted files at every size; the first 8 checksum bytes are distinct per pool entry"""
    rng = np.random.default_rng(seed)
    nk = m // 3 + 1
    pool_k, pool_h = rand_keys(rng, nk), rand_hashes(rng, 2 * nk)
    which = rng.integers(0, nk, m)
    keys = pool_k[which]
    hashes = pool_h[2 * which + rng.integers(0, 2, m)].reshape(m, 32)
    valid = (rng.random(m) < 0.9).astype(np.uint8) if with_valid else None
    return keys, hashes, valid


def size_cases():
    out = []
    for m in SIZES:
        out.append((f"size_{m}", *pooled(m, 100 + m, False)))
        out.append((f"size_{m}_valid", *pooled(m, 200 + m, True)))
    return out


def past_grid_case():
    """PAST_GRID files: two tiles per slice; one class longer than two whole slices, starting
    mid-slice; the rest pooled"""
    m = PAST_GRID
    assert slice_len(m) == 2 * TILE
    keys, hashes, valid = pooled(m, 300, True)
    rng = np.random.default_rng(301)
    long_run = 3 * slice_len(m) + 7
    at = rng.choice(m, long_run, replace=False)
    keys[at], hashes[at], valid[at] = U(1) << U(63), rand_hashes(rng, 1)[0], 1
    assert confirm_model(keys[at], hashes[at])["size"].max() == long_run > 2 * slice_len(m)
    return ("past_grid", keys, hashes, valid)


def border_case(m: int):
    """m of SLICE_COUNTS pooled files, with its model and whether it ties as all_cases() gives them:
    the counts at which the slice arithmetic changes (size_* and past_grid pass through five of
    them; BLOCKS * TILE, every workgroup exactly one whole tile, only here)"""
    keys, hashes, valid = pooled(m, 400 + SLICE_COUNTS.index(m), True)
    return (f"border_{m}", keys, hashes, valid, confirm_model(keys, hashes, valid), has_tie(keys, hashes, valid))


def long_class_case():
    """1000 files in slices of one tile: a class of 700 crosses two tile borders and is longer than
    two whole slices wherever the sort puts it; the 300 others are singles around it"""
    m, run = 1000, 700
    assert slice_len(m) == TILE and run > 2 * slice_len(m)
    rng = np.random.default_rng(310)
    keys, hashes = rand_keys(rng, m), rand_hashes(rng, m)
    at = rng.choice(m, run, replace=False)
    keys[at], hashes[at] = keys[at[0]], hashes[at[0]]
    return ("long_class", keys, hashes, None)


def all_invalid_case():
    keys, hashes, _ = pooled(300, 320, False)
    return ("all_invalid", keys, hashes, np.zeros(300, np.uint8))


def alternating_case():
    """one candidate group whose two classes alternate in position order, among singles"""
    rng = np.random.default_rng(330)
    keys, hashes = rand_keys(rng, 90), rand_hashes(rng, 90)
    a, b = rand_hashes(rng, 2)
    keys[10:50] = keys[10]
    hashes[10:50:2], hashes[11:50:2] = a, b
    return ("alternating", keys, hashes, None)


def _tied(tails, key=0x1234_5678_9ABC_DEF0, h0=bytes(range(8))):
    """files of one key whose checksums share their first 8 bytes: tails[i] is 24 bytes"""
    h = np.array([list(h0 + bytes(t)) for t in tails], np.uint8)
    return np.full(len(tails), key, U), h


def tie_cases():
    A, B = bytes([0x11] * 24), bytes([0x22] * 24)
    out = [("tie_aba", *_tied([A, B, A]), None)]
    m = confirm_model(*_tied([A, B, A]))
    assert m["rep"].tolist() == [0, 1, 0] and m["size"].tolist() == [2, 1, 2]
    b8, b31 = bytearray(A), bytearray(A)
    b8[0] ^= 1   # checksum byte 8
    b31[23] ^= 1  # checksum byte 31
    out.append(("tie_byte8", *_tied([A, bytes(b8), A, bytes(b8), A]), None))
    out.append(("tie_byte31", *_tied([A, bytes(b31), bytes(b31), A]), None))
    # the same three among other files, one of the tied invalid
    rng = np.random.default_rng(340)
    keys, hashes, valid = pooled(600, 341, True)
    tk, th = _tied([A, B, A, B, B, A, B])
    at = np.sort(rng.choice(600, 7, replace=False))
    keys[at], hashes[at], valid[at] = tk, th, [1, 1, 1, 0, 1, 1, 1]
    out.append(("tie_among_others", keys, hashes, valid))
    for c in out:
        assert has_tie(*c[1:]), c[0]
    # a tie run that is uniform: equal tails everywhere, so the prefix path finishes it; another key
    # with the same 32 bytes and a second run with another h0 beside it
    uk, uh = _tied([A] * 5 + [B] * 3)
    uh[5:, :8] = 0xEE  # the B run has its own first 8 bytes
    uk2, uh2 = _tied([A] * 2, key=77)
    uniform = ("tie_uniform", np.concatenate([uk, uk2]), np.concatenate([uh, uh2]), None)
    assert not has_tie(*uniform[1:])
    return out + [uniform]


def _pairs(firsts, key=5):
    """two files per checksum; checksum c is firsts[c] followed by zeros"""
    h = np.zeros((2 * len(firsts), 32), np.uint8)
    for c, f in enumerate(firsts):
        h[2 * c:2 * c + 2, :len(f)] = list(f)
    return np.full(len(h), key, U), h


def byte_order_cases():
    """the sets of one key ascend as memcmp orders the checksums: a little-endian or a signed
    compare gets each of these wrong.  Files are listed in descending checksum order."""
    out = []
    for name, firsts in (("order_0001_0100", [b"\x01\x00", b"\x00\x01"]), ("order_7f_80", [b"\x80", b"\x7f"]),
                         ("order_word_low_byte", [b"\x01" + b"\x00" * 7, b"\x00" * 7 + b"\x02"]),
                         # equal first 8 bytes: the order is decided past them (full-width path)
                         ("order_tail_0001_0100", [b"\x09" * 8 + b"\x01\x00", b"\x09" * 8 + b"\x00\x01"]),
                         ("order_tail_7f_80", [b"\x09" * 8 + b"\x00" * 23 + b"\x80", b"\x09" * 8 + b"\x00" * 23 + b"\x7f"])):
        keys, h = _pairs(firsts)
        m = confirm_model(keys, h)
        assert m["sets"][:, 1].tolist() == [2, 0], name  # the later pair comes first
        out.append((name, keys, h, None))
    return out


def extreme_case():
    """keys 0 and 2^64 - 1, checksums all 00 and all ff, each pair twice (equal checksums under
    different keys are different classes), and invalid files with the largest key and checksum
    before, between and after them"""
    keys, hashes, valid = [], [], []
    for rnd in range(2):
        for k in (0, M64):
            for b in (0x00, 0xFF):
                keys += [M64, k]
                hashes += [[0xFF] * 32, [b] * 32]
                valid += [0, 1]
    keys.append(M64), hashes.append([0xFF] * 32), valid.append(0)
    keys, hashes, valid = np.array(keys, U), np.array(hashes, np.uint8), np.array(valid, np.uint8)
    m = confirm_model(keys, hashes, valid)
    assert m["stats"].tolist() == [8, 2, 2, 4, 4, 8, 0, 2] and m["sets"][:, 0].tolist() == [0, 0, M64, M64]
    return ("extremes", keys, hashes, valid)


def invalid_cases():
    rng = np.random.default_rng(350)
    h = rand_hashes(rng, 3)
    # an invalid file with the smallest index of its key: the representative is the next member
    first = ("invalid_first_of_key", np.array([9, 9, 9, 4], U), np.stack([h[0], h[0], h[0], h[1]]),
             np.array([0, 1, 1, 1], np.uint8))
    m = confirm_model(*first[1:])
    assert m["rep"].tolist() == [M64, 1, 1, 3] and m["size"].tolist() == [0, 2, 2, 1]
    # an invalid file whose checksum equals a confirmed class's: not a member, not counted
    same = ("invalid_equals_class", np.array([9, 9, 9, 9], U), np.stack([h[0], h[0], h[0], h[2]]),
            np.array([1, 0, 1, 1], np.uint8))
    m = confirm_model(*same[1:])
    assert m["size"].tolist() == [2, 0, 2, 1] and m["verdict"].tolist() == [CONFIRMED, INVALID, CONFIRMED, REFUTED]
    # the only other file of a key is invalid: a single, not a candidate
    lone = ("invalid_leaves_single", np.array([9, 9], U), np.stack([h[0], h[0]]), np.array([1, 0], np.uint8))
    assert confirm_model(*lone[1:])["verdict"].tolist() == [SINGLE, INVALID]
    return [first, same, lone]


def mix_plant(seed: int = 360, m: int = MIX):
    """about m files with uniformly random keys and checksums; a tenth are exact duplicates of an
    earlier file (key and checksum), a hundredth twins (the key of an earlier file, a checksum of
    their own); 2 % invalid.  -> keys, hashes, valid, n_dup, n_twin"""
    rng = np.random.default_rng(seed)
    keys, hashes = rand_keys(rng, m), rand_hashes(rng, m)
    order = rng.permutation(m)
    n_dup, n_twin = m // 10, m // 100
    originals = order[n_dup + n_twin:]
    src = rng.choice(originals, n_dup + n_twin)
    dup, twin = order[:n_dup], order[n_dup:n_dup + n_twin]
    keys[dup], hashes[dup] = keys[src[:n_dup]], hashes[src[:n_dup]]
    keys[twin] = keys[src[n_dup:]]
    valid = (rng.random(m) < 0.98).astype(np.uint8)
    return keys, hashes, valid, n_dup, n_twin


def mix_case():
    keys, hashes, valid, _, _ = mix_plant()
    return ("random_mix", keys, hashes, valid)


# ---------------------------------------------------------------- planted files (end to end)
MINIMUM_FILE_SIZE = 100 * 1024  # cas.rs:27: larger files are sampled


def planted_files():
    """(len, content id, twin) of 24 sampled files of 110 to 200 KiB and 4 whole-kind files, in a
    seeded order: exact copies, twins (a byte changed outside every sampled window: the same
    cas_id, another checksum) alone and in pairs, and one content at two lengths."""
    s = [112_640, 131_071, 150_001, 163_840, 180_224, 204_800]
    sampled = ([(s[0], 500, 0)] * 3 + [(s[0], 500, 1)] +          # three copies and a lone twin
               [(s[1], 501, 0)] * 2 + [(s[1], 501, 2)] * 2 +      # two copies, two twins of one tag
               [(s[2], 502, 0), (s[2], 502, 3)] +                 # an original and its twin: nothing confirmed
               [(s[3], 503, 0), (s[4], 503, 0)] +                 # one content at two lengths: two cas_ids
               [(s[5] - 1024 * i, 510 + i, 0) for i in range(12)])
    whole = [(50_000, 600, 0)] * 2 + [(1000, 601, 0), (MINIMUM_FILE_SIZE, 602, 0)]
    files = sampled + whole
    assert len(sampled) == 24 and all(110 * 1024 <= L <= 200 * 1024 for L, _, _ in sampled)
    order = np.random.default_rng(370).permutation(len(files))
    return [files[i] for i in order]


def planted_expectation(files):
    """From the plant alone: files are one class iff (len, cid, twin) are equal, one group iff
    (len, cid) are (a whole-kind file's cas_id hashes every byte, the twin's too).
    -> (rep, size, verdict) lists"""
    cls = [(L, c, t) for L, c, t in files]
    grp = [(L, c) if L > MINIMUM_FILE_SIZE else (L, c, t) for L, c, t in files]
    rep = [cls.index(x) for x in cls]
    size = [cls.count(x) for x in cls]
    verdict = [SINGLE if grp.count(g) == 1 else CONFIRMED if n >= 2 else REFUTED for g, n in zip(grp, size)]
    for (L, c, t), r, v in zip(files, rep, verdict):  # a twin is never confirmed with its original
        assert not t or v == REFUTED or files[r][2] == t
    assert verdict.count(REFUTED) == 3 and verdict.count(CONFIRMED) == 9 and verdict.count(SINGLE) == 16
    return rep, size, verdict


def small_cases():
    """every case but the two large ones"""
    return (size_cases() + [long_class_case(), all_invalid_case(), alternating_case()] + tie_cases() +
            byte_order_cases() + [extreme_case()] + invalid_cases())


_ALL = None


def all_cases():
    """the whole list, each with its model and whether it ties, built once per process"""
    global _ALL
    if _ALL is None:
        _ALL = [(name, keys, hashes, valid, confirm_model(keys, hashes, valid), has_tie(keys, hashes, valid))
                for name, keys, hashes, valid in small_cases() + [past_grid_case(), mix_case()]]
    return _ALL
