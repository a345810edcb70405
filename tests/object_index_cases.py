"""Input generators shared by tests/test_object_index.py (the host mirrors and sd_cpu_*),
tests/test_gpu_object_index.py (the kernels and the device entries) and, by construction,
spacedrive_amd/csrc/object_index_selftest.cpp (the same generator and case table in C++):
key sets at the edges of the u64 range, sets that defeat the prefix directory, and the
insert sequences that exercise keep-first, growth and the shard filter.  Every list asserts
the properties it is there for, so a wrong edit cannot quietly shrink a sweep.

Nothing here touches a device or the library.
"""
from __future__ import annotations

import numpy as np

U = np.uint64
M64 = (1 << 64) - 1

INDEX_SIZES = (0, 1, 2, 15, 16, 17, 255, 256, 257, 4097, 100_003)
QUERY_COUNTS = (0, 1, 63, 64, 65, 257, 5000)
EDGE_KEYS = (0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64 - 1, M64)
NPARTS = (1, 2, 3, 8)


def splitmix(seed: int, n: int) -> np.ndarray:
    """n u64 values: splitmix64 of the counters seed + 1 .. seed + n (times the golden gamma)."""
    with np.errstate(over="ignore"):
        z = (U(seed) + (np.arange(1, n + 1, dtype=U) * U(0x9E3779B97F4A7C15)))
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def random_keys(n: int, seed: int) -> np.ndarray:
    """n distinct uniform u64 keys, unsorted (the order splitmix gives them)."""
    k = splitmix(seed, n)
    assert len(np.unique(k)) == n
    return k


def edge_keys() -> np.ndarray:
    k = np.array(EDGE_KEYS, dtype=U)
    assert {0, (1 << 63) - 1, 1 << 63, M64} <= set(int(x) for x in k)
    assert any(int(a) + 1 == int(b) for a, b in zip(k[:-1], k[1:]))  # neighbours k, k + 1
    return k


def shared_prefix_keys(n: int, seed: int = 77) -> np.ndarray:
    """n distinct keys with the same top 32 bits: one directory bucket holds everything."""
    low = np.unique(splitmix(seed, n + n // 8 + 8) & U(0xFFFFFFFF))[:n]
    assert len(low) == n
    k = (U(0xC0FFEE42) << U(32)) | low
    assert len(set((k >> U(32)).tolist())) == 1
    return k[np.argsort(splitmix(seed + 1, n))]  # unsorted


def key_sets(n: int):
    """name -> n keys (unsorted) for an index of n entries: uniform, edges, shared prefix."""
    sets = {"uniform": random_keys(n, 1000 + n)}
    e = edge_keys()
    if n >= len(e):
        rest = random_keys(n - len(e), 2000 + n)
        sets["edges"] = np.concatenate([e, rest[~np.isin(rest, e)]])
    else:
        sets["edges"] = e[:n]
    sets["shared_prefix"] = shared_prefix_keys(n) if n else np.zeros(0, U)
    for k in sets.values():
        assert len(k) == n == len(np.unique(k))
    return sets


def queries(keys: np.ndarray, m: int, seed: int = 5) -> np.ndarray:
    """m query keys against an index of `keys`: present ones, absent ones between two keys
    (key + 1 where that is free), below the minimum and above the maximum, and uniform
    misses, in a shuffled order."""
    if m == 0:
        return np.zeros(0, U)
    s = np.sort(keys)
    parts = []
    if len(s):
        pick = splitmix(seed, m) % U(len(s))
        present = s[pick.astype(np.int64)]
        with np.errstate(over="ignore"):
            between = present + U(1)
        parts = [present[: (m + 1) // 2], between[: m // 4]]
        if int(s[0]) > 0:
            parts.append(np.array([int(s[0]) - 1, 0], dtype=U))
        if int(s[-1]) < M64:
            parts.append(np.array([int(s[-1]) + 1, M64], dtype=U))
    parts.append(splitmix(seed + 9, m))
    q = np.concatenate(parts)[:m]
    assert len(q) == m
    return q[np.argsort(splitmix(seed + 3, m))]


def vals_for(keys: np.ndarray, salt: int) -> np.ndarray:
    """Object ids for keys: any u64 is legal, so 0 and 2^64 - 1 appear among them."""
    with np.errstate(over="ignore"):
        v = splitmix(salt, len(keys)) ^ (keys * U(3))
    if len(v) > 2:
        v[0], v[1] = U(0), U(M64)
    return v


def insert_cases():
    """name -> list of steps (keys u64, object ids u64), each an insert into the index the
    previous steps left (the first into an empty one)."""
    a = random_keys(50, 11)
    mid = (random_keys(40, 12) >> U(2)) | (U(1) << U(62))     # in [2^62, 2^63)
    below = random_keys(30, 13) >> U(3)                        # < 2^61
    above = random_keys(30, 14) | (U(1) << U(63))              # >= 2^63
    dup = np.concatenate([a[:10], a[:10][::-1], a[5:15], a[:3]])
    g1, g2, g3 = random_keys(10, 15), random_keys(30, 16), random_keys(200, 17)
    sp = shared_prefix_keys(300)
    cases = {
        "empty": [(a[:20], vals_for(a[:20], 1))],
        "all_present": [(a, vals_for(a, 2)), (a[::-1].copy(), vals_for(a, 3))],
        "dups_in_input": [(dup, vals_for(dup, 4))],
        "below_min": [(mid, vals_for(mid, 5)), (below, vals_for(below, 6))],
        "above_max": [(mid, vals_for(mid, 7)), (above, vals_for(above, 8))],
        "three_growth": [(g1, vals_for(g1, 9)), (g2, vals_for(g2, 10)),
                         (np.concatenate([g3, g1]), vals_for(np.concatenate([g3, g1]), 11))],
        "edges": [(edge_keys()[::2].copy(), vals_for(edge_keys()[::2], 12)), (edge_keys(), vals_for(edge_keys(), 13))],
        "shared_prefix": [(sp[:100], vals_for(sp[:100], 14)), (sp, vals_for(sp, 15))],
    }
    assert int(mid.min()) > int(below.max()) and int(mid.max()) < int(above.min())
    assert len(np.unique(dup)) < len(dup)
    # three_growth crosses a growth of the buffers (capacity 16 -> 40 -> 240) and changes of
    # the directory bits (n = 10, 40, 240: b = 0, 2, 4)
    assert [len(g1), len(g1) + len(g2), len(g1) + len(g2) + len(g3)] == [10, 40, 240]
    return cases


def dir_bits(n: int) -> int:
    """The directory-size policy (object_index_host.cpp oi_dir_bits): 2^b <= n / 8 < 2^(b+1)."""
    b = 0
    while b < 24 and (16 << b) <= n:
        b += 1
    return b


def scan_cas_ids(n: int, seed: int, dup_frac: float = 0.4, none_frac: float = 0.1):
    """n cas_ids (16 hex digits, or None for an empty file) in file order with duplicates at
    any distance: inside one chunk and across chunks and scans."""
    pool = ["%016x" % int(x) for x in splitmix(seed, max(1, int(n * (1 - dup_frac))))]
    r = splitmix(seed + 1, 2 * n)
    out = []
    for i in range(n):
        if int(r[2 * i]) % 1000 < none_frac * 1000:
            out.append(None)
        elif i % 3 == 0 and out and out[-1] is not None:
            out.append(out[-1])                      # an adjacent duplicate: same chunk (mostly)
        else:
            out.append(pool[int(r[2 * i + 1]) % len(pool)])
    return out
