"""Input generators shared by tests/test_fingerprint.py (the CPU path) and
tests/test_gpu_fingerprint.py (the gather kernel and the device entries): the file lengths
at which the cas message's source map changes shape, and a placement of the files in one
buffer that uses every allowed start alignment.  Every list asserts its own length and the
properties it is there for, so a wrong edit cannot quietly shrink a sweep.

Nothing here touches a device or the library.
"""
from __future__ import annotations

import numpy as np

MiB = 1 << 20
H, S, NS = 8192, 10240, 4  # cas.rs:10-14 header/footer, sample size, sample count
WHOLE_MAX = 102400         # cas.rs:15,27: hashed whole up to and including this length
SAMPLED_MSG_LEN = 57352

WHOLE_LENS = (0, 1, 7, 8, 9, 15, 16, 17, 55, 56, 57, 63, 64, 65, 1015, 1016, 1017, 2040, 2041, 102399, 102400)
SAMPLED_RUN = tuple(range(102401, 102465))
SAMPLED_EXTRA = (131072, MiB - 1, MiB, MiB + 1, 3 * MiB + 5)
N_WHOLE, N_SAMPLED = 21, 69
# cas_id of the content bytes(i % 251) of these lengths
PATTERN_IDS = {0: "71e0a99173564931", 1016: "c0de16cef5f85601", 1017: "62fe3d833d2df619",
               102400: "c66a52267c7e5ee9", 102401: "17f74805066119da"}


def whole_lens():
    assert len(WHOLE_LENS) == N_WHOLE == len(set(WHOLE_LENS)) and max(WHOLE_LENS) == WHOLE_MAX
    return list(WHOLE_LENS)


def segment_shifts(size: int):
    """(source offset - position inside head || samples || tail) mod 16 of the six segments of
    a sampled message: how far the gather shifts each segment's bytes between its aligned
    16-byte loads and its aligned stores (the file itself starts 16-byte aligned)."""
    assert size > WHOLE_MAX
    jump = (size - 2 * H) // NS  # cas.rs:33
    src = [0] + [H + k * jump for k in range(NS)] + [size - H]
    pos = [0] + [H + k * S for k in range(NS)] + [H + NS * S]
    return [(s - p) % 16 for s, p in zip(src, pos)]


def sampled_lens():
    lens = list(SAMPLED_RUN) + list(SAMPLED_EXTRA)
    assert len(lens) == N_SAMPLED and min(lens) == WHOLE_MAX + 1
    sh = np.array([segment_shifts(L) for L in SAMPLED_RUN])
    assert set(sh[:, 0]) == {0} and set(sh[:, 1]) == {0}            # head, sample 0: never shifted
    for col in (2, 4, 5):                                           # samples 1, 3 and the tail: every shift
        assert set(sh[:, col]) == set(range(16)), col
    assert set(sh[:, 3]) == set(range(0, 16, 2))                    # sample 2: 2 * jump is even
    return lens


def cases(cid0: int = 7000):
    """(lens u64, cids u64, twins u32) of the whole and the sampled files, whole first."""
    lens = np.array(whole_lens() + sampled_lens(), np.uint64)
    n = len(lens)
    assert n == N_WHOLE + N_SAMPLED == 90
    return lens, np.arange(cid0, cid0 + n, dtype=np.uint64), (np.arange(n) % 3).astype(np.uint32)


def placement(lens, base: int = 0):
    """Range starts for files of these lengths in one buffer -> (offsets u64, total bytes).
    Starts are 16-byte aligned; file i starts 0, 16 or 32 bytes after the 16-byte boundary
    that follows file i - 1, so the gaps are 0..47 bytes -- some exactly 0: a neighbour's bytes
    follow directly -- and every 16-byte residue mod 128 is used as a start.  The buffer is
    readable to the 64-byte boundary after the last range (`total`)."""
    steps = (0, 1, 2, 0, 2, 1, 0)
    offs, gaps, pos = [], [], base
    for i, L in enumerate(int(x) for x in lens):
        start = (pos + 15) // 16 * 16 + 16 * steps[i % len(steps)]
        if i:
            gaps.append(start - pos)
        offs.append(start)
        pos = start + L
    total = (pos + 63) // 64 * 64 + 64
    if len(offs) >= 40:
        assert {o % 128 for o in offs} == set(range(0, 128, 16))
        assert min(gaps) == 0 and max(gaps) <= 48
    assert all(o % 16 == 0 for o in offs)
    return np.array(offs, np.uint64), total


def host_buffer(lens, cids, twins, offsets, total: int, surround: str):
    """The buffer on the host: synthetic content (oracle generator) in the ranges; outside them
    0xA5 ("a5"), seeded random bytes ("random") or zeros ("zero")."""
    from oracle import native
    if surround == "random":
        buf = np.random.default_rng(4242).integers(0, 256, total, dtype=np.uint8)
    else:
        buf = np.full(total, 0xA5 if surround == "a5" else 0, np.uint8)
    for L, c, t, o in zip(lens, cids, twins, offsets):
        if L:
            buf[int(o):int(o) + int(L)] = np.frombuffer(native.synth_bytes(int(c), int(t), 0, int(L)), np.uint8)
    return buf
