"""Cases for the CDC deltas (include/sd_cas.h, "Deltas": sd_cdc_delta_plan / _pack / _apply and their
host twins), shared by tests/test_cdc_delta.py (the twins, the wrappers) and
tests/test_gpu_cdc_delta.py (the kernels).

The rule is restated here in numpy and plain loops from the header's words, not from either
implementation, on top of cdc_cases' restatement of cut / ids: the representatives (the smallest
slot of each (length, id) class), a slot's kind, the literal offsets, the runs, the statistics; and
the apply as a validation followed by one slice assignment per run.

A plan case is (name, chunk_base, n_base, chunks, ids) -- tables only: the plan reads no data.  A
recipe case is a hand-made recipe for the copy: (name, lit, runs, out_offs, out_lens, out_size).
Nothing here touches a device or the library.
"""
from __future__ import annotations

import numpy as np

from tests import cdc_cases as cc

U = np.uint64
NONE = (1 << 64) - 1
INVALID = "invalid"


# ---------------------------------------------------------------- the rule
def rep_of(chunks, ids) -> np.ndarray:
    """the smallest slot of each (length, id) class, per slot"""
    m = len(chunks)
    if m == 0:
        return np.zeros(0, U)
    rows = np.zeros((m, 40), np.uint8)
    rows[:, :8] = np.ascontiguousarray(chunks[:, 1]).astype(">u8").view(np.uint8).reshape(m, 8)
    rows[:, 8:] = ids
    _, first, inv = np.unique(rows.view(np.dtype((np.void, 40))).reshape(-1), return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(U)


def plan_model(base, n_base: int, chunks, rep) -> dict:
    """-> lit_off uint64 [target slots], runs uint64 [r, 4], files uint64 [targets, 6], stats uint64 [8]"""
    base = [int(x) for x in base]
    n = len(base) - 1
    if n <= 0:
        return {"lit_off": np.zeros(0, U), "runs": np.zeros((0, 4), U), "files": np.zeros((0, 6), U), "stats": np.zeros(8, U)}
    t0, m = base[n_base], base[n]
    length = [int(x) for x in chunks[:, 1]]
    offset = [int(x) for x in chunks[:, 0]]
    rep = [int(x) for x in rep]
    base_file = {}
    for g in range(n_base):
        for s in range(base[g], base[g + 1]):
            base_file[s] = g
    lit_off = [NONE] * (m - t0)
    lit_bytes, runs, files = 0, [], []
    st = [n - n_base, m - t0, 0, 0, 0, 0, 0, 0]
    for f in range(n_base, n):
        row, prev = [base[f + 1] - base[f], 0, 0, 0, 0, 0], None  # prev: (source, the offset its run goes on at)
        for s in range(base[f], base[f + 1]):
            ln, r = length[s], rep[s]
            if ln == 0:  # zero: a literal chunk of no bytes, no run
                st[4] += 1
                prev = None
                continue
            if r < t0:  # copy
                src, off = 1 + base_file[r], offset[r]
                st[2] += 1; st[3] += ln; row[1] += 1; row[2] += ln
            elif r == s:  # literal
                src, off = 0, lit_bytes
                lit_off[s - t0] = off
                lit_bytes += ln
                st[4] += 1; row[3] += ln
            else:  # repeat: r is an earlier target slot, a literal
                assert t0 <= r < s and rep[r] == r and length[r] == ln
                src, off = 0, lit_off[r - t0]
                lit_off[s - t0] = off
                st[6] += 1; row[4] += ln
            if prev == (src, off):
                runs[-1][3] += ln
            else:
                runs.append([f - n_base, src, off, ln])
                row[5] += 1
            prev = (src, off + ln)
        files.append(row)
    st[5], st[7] = lit_bytes, len(runs)
    out = {"lit_off": np.array(lit_off, U), "runs": np.array(runs, U).reshape(-1, 4), "files": np.array(files, U).reshape(-1, 6),
           "stats": np.array(st, U)}
    check_identities(out, sum(length[t0:]))
    return out


def check_identities(got: dict, target_bytes: int) -> None:
    st, files, runs = [int(x) for x in got["stats"]], got["files"], got["runs"]
    assert st[1] == st[2] + st[4] + st[6], st
    repeated = int(files[:, 4].sum()) if len(files) else 0
    assert target_bytes == st[3] + st[5] + repeated, (st, repeated, target_bytes)
    assert st[7] == len(runs) == (int(files[:, 5].sum()) if len(files) else 0)
    if len(files):
        assert int(files[:, 0].sum()) == st[1] and int(files[:, 2].sum()) == st[3] and int(files[:, 3].sum()) == st[5]
    if len(runs):
        assert (np.diff(runs[:, 0].astype(np.int64)) >= 0).all() and int(runs[:, 3].sum()) == target_bytes
        assert int(runs[:, 3].min()) > 0


def pack_model(buf, offs, base, n_base: int, chunks, rep, plan: dict) -> np.ndarray:
    """the literal buffer: every literal slot's bytes at its lit_off"""
    lit = np.zeros(int(plan["stats"][5]), np.uint8)
    t0 = int(base[n_base]) if len(base) > 1 else 0
    for f in range(n_base, len(base) - 1):
        for s in range(int(base[f]), int(base[f + 1])):
            ln = int(chunks[s, 1])
            if ln and int(rep[s]) == s:
                a = int(offs[f]) + int(chunks[s, 0])
                o = int(plan["lit_off"][s - t0])
                lit[o:o + ln] = buf[a:a + ln]
    return lit


def validate(runs, base_lens, lit_bytes: int, out_lens) -> bool:
    """the apply's rule for a recipe, in exact integers"""
    nb, nt = len(base_lens), len(out_lens)
    total = [0] * nt
    t_prev = 0
    for t, src, off, b in ([int(x) for x in row] for row in runs):
        if t >= nt or t < t_prev or src > nb:
            return False
        t_prev = t
        if off + b > (int(base_lens[src - 1]) if src else lit_bytes):
            return False
        total[t] += b
    return total == [int(x) for x in out_lens]


def apply_model(runs, base_buf, base_offs, base_lens, lit, lit_bytes, out, out_offs, out_lens):
    """-> `out` with the targets rebuilt, or INVALID with `out` as it was"""
    if not validate(runs, base_lens, lit_bytes, out_lens):
        return INVALID
    at = [0] * len(out_lens)
    for t, src, off, b in ([int(x) for x in row] for row in runs):
        s = lit[off:off + b] if src == 0 else base_buf[int(base_offs[src - 1]) + off:int(base_offs[src - 1]) + off + b]
        d = int(out_offs[t]) + at[t]
        out[d:d + b] = s
        at[t] += b
    return out


# ---------------------------------------------------------------- hand-made recipes for the copy
COPY_LENS = (1, 15, 16, 17, 31, 33, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1)


def _layout(out_lens, rng, odd: bool):
    """output ranges in order with random gaps; odd: starts at any byte, else 16-byte aligned"""
    offs, cur = [], int(rng.integers(1, 40))
    for L in out_lens:
        cur = cur | 1 if odd else (cur + 15) // 16 * 16
        offs.append(cur)
        cur += int(L) + int(rng.integers(0, 70))
    return np.array(offs, U), (cur + 63) // 64 * 64 + 64


def _lit(nbytes: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def recipe_cases(big: bool = False):
    """[(name, lit, runs, out_offs, out_lens, out_size)]: one or more targets built from runs out of
    the literal buffer alone (n_base == 0)"""
    rng = np.random.default_rng(4242)
    out = []
    # all 256 pairs (source residue, destination residue) mod 16: target t = 16 sr + dr starts 16-byte
    # aligned, a leading run of dr bytes sets the destination residue of the run under test
    lit = _lit(1 << 16, 1)
    runs, lens = [], []
    for sr in range(16):
        for dr in range(16):
            t = 16 * sr + dr
            if dr:
                runs.append([t, 0, 16 * int(rng.integers(0, 100)), dr])
            runs.append([t, 0, 16 * int(rng.integers(0, 1000)) + sr, 100 + t % 7])
            lens.append(dr + 100 + t % 7)
    offs, size = _layout(lens, rng, False)
    out.append(("residues", lit, np.array(runs, U), offs, np.array(lens, U), size))
    # the lengths, each at several residue pairs, the outputs at odd offsets
    runs, lens = [], []
    for L in COPY_LENS:
        for sr, lead in ((0, 0), (5, 0), (0, 7), (3, 11), (13, 2), (15, 15), (8, 4), (4, 8)):
            t = len(lens)
            if lead:
                runs.append([t, 0, int(rng.integers(0, 1000)), lead])
            runs.append([t, 0, 16 * int(rng.integers(0, 1000)) + sr, L])
            lens.append(lead + L)
    offs, size = _layout(lens, rng, True)
    out.append(("lengths", lit, np.array(runs, U), offs, np.array(lens, U), size))
    # segments that meet inside one 16-byte unit: runs of 1..15 bytes back to back
    runs = [[0, 0, int(rng.integers(0, 60000)), 1 + k % 15] for k in range(600)]
    runs += [[1, 0, int(rng.integers(0, 60000)), 15 - k % 15] for k in range(300)]
    lens = [sum(r[3] for r in runs if r[0] == t) for t in (0, 1)]
    offs, size = _layout(lens, rng, True)
    out.append(("meeting", lit, np.array(runs, U), offs, np.array(lens, U), size))
    # a source range that ends on the last byte before its 64-byte readable limit: the buffer is 64 k bytes
    # and not a byte more, the runs end at its end
    lit64 = _lit(4096, 2)
    runs = [[0, 0, 4096 - 37, 37], [0, 0, 4096 - 4001, 4001], [1, 0, 4095, 1], [2, 0, 0, 4096]]
    lens = [37 + 4001, 1, 4096]
    offs, size = _layout(lens, rng, True)
    out.append(("readable_limit", lit64, np.array(runs, U), offs, np.array(lens, U), size))
    # 70 000 runs of 1 to 200 bytes over three targets, and a target without a run between them
    k = 70_000
    rl = rng.integers(1, 201, k)
    ro = rng.integers(0, (1 << 16) - 200, k)
    rt = np.sort(rng.choice([0, 2, 3], k))
    runs = np.stack([rt, np.zeros(k, np.int64), ro, rl], axis=1).astype(U)
    lens = [int(rl[rt == t].sum()) for t in range(4)]
    assert lens[1] == 0
    offs, size = _layout(lens, rng, True)
    out.append(("many_runs", lit, runs, offs, np.array(lens, U), size))
    if big:  # one run of 64 MiB + 1, source and destination at different residues
        n = (64 << 20) + 1
        lit_big = np.resize(_lit((1 << 20) + 13, 3), n + 64)
        out = [("big_run", lit_big, np.array([[0, 0, 3, 5], [0, 0, 9, n]], U), np.array([33], U), np.array([n + 5], U), n + 256)]
    return out


def bad_recipes():
    """(name, runs, how the device buffers must be sized) over base files of 1000 and 2000 bytes, 3000
    literal bytes and targets of 500 and 700 bytes.  Every out-of-range span of a recipe that a faulty
    validator would copy still lies inside SLACK bytes behind each buffer."""
    good = [[0, 1, 0, 300], [0, 0, 100, 200], [1, 2, 1300, 700]]
    def w(j, col, val):
        r = [list(x) for x in good]
        r[j][col] = val
        return r
    return [
        ("source_beyond_n_base", w(0, 1, 3)),
        ("past_base_by_1", w(2, 2, 1301)),
        ("past_literals_by_1", [[0, 1, 0, 300], [0, 0, 2801, 200], [1, 2, 1300, 700]]),
        ("wraps", w(1, 2, (1 << 64) - 100)),
        ("wraps_to_zero", w(1, 2, (1 << 64) - 200)),
        ("one_short", w(1, 3, 199)),
        ("one_long", w(1, 3, 201)),
        ("last_file_short", w(2, 3, 699)),
        ("descending", [[1, 2, 1300, 700], [0, 1, 0, 300], [0, 0, 100, 200]]),
        ("t_beyond_targets", w(2, 0, 2)),
        ("a_file_without_runs", good[:2]),
        ("no_runs_at_all", []),
    ], good


BAD_BASE_LENS, BAD_LIT, BAD_OUT_LENS, SLACK = (1000, 2000), 3000, (500, 700), 4096


# ---------------------------------------------------------------- tables for the plan
def _id(label: int) -> np.ndarray:
    return np.frombuffer(np.random.default_rng(1000 + label).bytes(32), np.uint8)


def table(files):
    """files: per file a list of (length, label) -> chunk_base, chunks, ids.  Equal (length, label) is
    an equal chunk; an empty file is [(0, 0)]"""
    base, chunks, ids = [0], [], []
    for f in files:
        assert len(f) >= 1
        off = 0
        for ln, label in f:
            chunks.append((off, ln))
            ids.append(_id(label if ln else 0))
            off += ln
        base.append(len(chunks))
    return np.array(base, U), np.array(chunks, U).reshape(-1, 2), np.array(ids, np.uint8).reshape(-1, 32)


_CACHE: dict = {}


def insert5_files():
    """1 MiB of synthetic content, and the same with 5 bytes inserted at 1000"""
    A = cc.shift_files()[0]
    return [A, np.concatenate([A[:1000], np.arange(1, 6, dtype=np.uint8), A[1000:]])]


def data_case(name, files, params, n_base, seed):
    """cut and ids from cdc_cases' restatement and the oracle: (name, base, n_base, chunks, ids, buf, offs, lens)"""
    buf, offs, lens = cc.pack(files, seed)
    want = cc.model(buf, offs, lens, params)
    ids = cc.oracle_ids(buf, offs, want["base"], want["chunks"])
    return (name, want["base"], n_base, want["chunks"], ids, buf, offs, lens)


def data_cases():
    """cases with bytes behind them: plan, pack and apply"""
    if "data" in _CACHE:
        return _CACHE["data"]
    mb, mn, mx = cc.P10
    A, A5 = insert5_files()
    zeros = np.zeros(3 * mx + 100, np.uint8)  # no candidate in zeros: three forced chunks of max_size, equal, and a rest
    other = cc.synth(31, 9000)
    new = cc.synth(32, 20000)
    out = [
        data_case("identical", [A[:200000], other, A[:200000]], cc.P10, 2, 900),
        data_case("insert5", [A, A5], cc.P10, 1, 901),
        data_case("constant", [other, zeros], cc.P10, 1, 902),
        data_case("repeat_across_targets", [other, np.concatenate([other[:3000], new]), np.concatenate([new, other])], cc.P10, 1, 903),
        data_case("empty_files", [np.zeros(0, np.uint8), other, np.zeros(0, np.uint8), other[:5000], np.zeros(0, np.uint8)],
                  cc.P10, 2, 904),
        data_case("no_base", [other, np.concatenate([new, other]), new], cc.P10, 0, 905),
        data_case("all_base", [other, new], cc.P10, 2, 906),
    ]
    by = {c[0]: c for c in out}
    # the premises, said of the restatement's answer
    name, base, nb, chunks, ids = by["identical"][:5]
    p = plan_model(base, nb, chunks, rep_of(chunks, ids))
    assert p["runs"].tolist() == [[0, 1, 0, 200000]] and int(p["stats"][5]) == 0
    name, base, nb, chunks, ids = by["insert5"][:5]
    p = plan_model(base, nb, chunks, rep_of(chunks, ids))
    st = [int(x) for x in p["stats"]]
    assert st[1] >= 700 and st[1] - st[2] <= 3 and st[5] <= 3 * mx and st[7] <= 3, st
    name, base, nb, chunks, ids = by["constant"][:5]
    p = plan_model(base, nb, chunks, rep_of(chunks, ids))
    t0 = int(base[1])
    assert chunks[t0:t0 + 3, 1].tolist() == [mx] * 3 and int(p["stats"][6]) == 2
    assert p["runs"][:3, 1:3].tolist() == [[0, 0]] * 3 and p["lit_off"][:3].tolist() == [0, 0, 0]  # literal, repeat, repeat
    name, base, nb, chunks, ids = by["repeat_across_targets"][:5]
    p = plan_model(base, nb, chunks, rep_of(chunks, ids))
    assert int(p["files"][1, 4]) > 0 and int(p["files"][0, 3]) > 0 and int(p["files"][1, 2]) > 0  # repeats what target 0 brought
    name, base, nb, chunks, ids = by["empty_files"][:5]
    p = plan_model(base, nb, chunks, rep_of(chunks, ids))
    assert p["files"][:, 0].tolist() == [1, int(base[4] - base[3]), 1] and p["files"][0, 5] == 0 and int(p["stats"][4]) >= 2
    assert int(p["lit_off"][0]) == NONE and set(p["runs"][:, 0].tolist()) == {1}
    assert int(plan_model(*by["no_base"][1:4], rep_of(*by["no_base"][3:5]))["stats"][2]) == 0
    assert not plan_model(*by["all_base"][1:4], rep_of(*by["all_base"][3:5]))["stats"].any()
    _CACHE["data"] = out
    return out


def table_cases():
    """tables alone: (name, base, n_base, chunks, ids)"""
    X, Y, Z, N = (700, 1), (900, 2), (800, 3), (650, 4)
    out = [
        # the base holds X twice, at offsets 900 and 2500: the copy comes from the smaller slot
        ("base_twice", *_split(table([[Y, X, Y, X], [X, Z, X]]), 1)),
        # consecutive in the base: one run; swapped: two
        ("merge_and_not", *_split(table([[X, Y, Z], [X, Y, Z, Y, X, N, N, Z]]), 1)),
        # equal length, different id: not equal
        ("same_length", *_split(table([[(700, 9)], [X, (700, 9)]]), 1)),
        ("two_bases", *_split(table([[X, Y], [Z], [Z, X, Y, Z], [(0, 0)], [Y, Z]]), 2)),
    ]
    name, base, nb, chunks, ids = out[0]
    p = plan_model(base, nb, chunks, rep_of(chunks, ids))
    assert p["runs"].tolist() == [[0, 1, 900, 700], [0, 0, 0, 800], [0, 1, 900, 700]]
    name, base, nb, chunks, ids = out[1]
    p = plan_model(base, nb, chunks, rep_of(chunks, ids))
    assert p["runs"].tolist() == [[0, 1, 0, 2400], [0, 1, 700, 900], [0, 1, 0, 700], [0, 0, 0, 650], [0, 0, 0, 650],
                                  [0, 1, 1600, 800]]
    return out


def _split(t, n_base):
    base, chunks, ids = t
    return base, n_base, chunks, ids


def many_table():
    """more than 262 144 target chunks (past one trip of a sliced grid's 1024 x 256 lanes): 64-byte
    chunks of 5000 kinds, 3000 of them in the base; three targets"""
    if "many" in _CACHE:
        return _CACHE["many"]
    rng = np.random.default_rng(99)
    kinds = np.frombuffer(rng.bytes(32 * 5000), np.uint8).reshape(5000, 32)
    counts = [3000, 100_000, 1, 170_000]
    labels = np.concatenate([np.arange(3000), rng.integers(0, 5000, sum(counts[1:]))])
    lens = 64 + (labels % 3) * 64
    base = np.concatenate([[0], np.cumsum(counts)]).astype(U)
    offs = np.concatenate([np.cumsum(lens[int(a):int(b)]) - lens[int(a):int(b)] for a, b in zip(base[:-1], base[1:])])
    chunks = np.stack([offs, lens], axis=1).astype(U)
    assert int(base[-1]) - int(base[1]) > 262_144
    _CACHE["many"] = ("many_chunks", base, 1, chunks, np.ascontiguousarray(kinds[labels]))
    return _CACHE["many"]


def split_of(case):
    """a cdc_cases case as a delta case: the first half of the files is the base"""
    name, buf, offs, lens, params, want = case
    return (name, want["base"], len(lens) // 2, want["chunks"], want["ids"], buf, offs, lens)
