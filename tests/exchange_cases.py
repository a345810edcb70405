"""The cases of the dedup exchange over ranks (sd_cas_dedup_mgpu / sd_cas_dedup_mgpu_indexed:
partition by cas_id prefix -> exchange -> group -> Object rule per rank), shared by
tests/test_exchange_cases.py (these lists against themselves, the oracle's identifier replay and
sd_split_range) and tests/test_gpu_exchange.py (the same lists through the in-process
communicator on one GPU).  Every list asserts its own length and the property it exists for, so
a wrong edit cannot quietly shrink the sweep.

A case is a layout -- per rank (index base, file count, mask kind) --, a key distribution -- one
u64 cas_id key per file, made into hash rows by shape_cases.hashes_from_keys, nothing is hashed
--, a rank count R and the identifier's chunk size, CHUNK = 7 throughout, so that many steps
straddle a shard cut.  For each case the module computes, with the host mirrors (group_host,
identifier.object_owners on CPU tensors), what every rank must return, and simulates the order in which the records arrive there, which is what decides whether
the grouping may trust that order (SD_DEDUP_INDEX_SORTED).

Nothing here touches a device or the library.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from spacedrive_amd.dedup import dest_of, group_host, partition_host
from spacedrive_amd.identifier import object_owners
from tests import shape_cases as sc

U = np.uint64
MiB = 1 << 20
CHUNK = 7
N_FILES = 3001
RANKS = (2, 3, 8)
HIGH_BASE = (1 << 40) + 3
UNEVEN_SIZES = (1, 255, 256, 257, 1025)
# the shards of an uneven layout but its last, which takes the rest: every cut lands inside a chunk
UNEVEN_SEQ = (257, 1, 1025, 255, 256, 1, 257)

LAYOUTS = ("even", "uneven", "empty_first", "empty_middle", "empty_last", "only_last", "masked_rank", "no_mask",
           "random_mask", "descending", "rotated", "high_base")
DISTS = ("uniform", "one_dest_first", "one_dest_last", "edges", "step_straddle", "one_group")
UNORDERED = ("descending", "rotated")  # the layouts whose index ranges do not ascend with the rank
EMPTY_RANK = {"empty_first": lambda R: 0, "empty_middle": lambda R: R // 2, "empty_last": lambda R: R - 1}
MASKED_RANK = 0

# one_group: the keys of shape_cases.bucket_case(4097, "late", True) and ONE_GROUP_EXTRA more copies
# of its 4096-fold key.  The extra copies are what keeps the overflow at R > 1: the receiving rank
# sees only its own prefix range, so its key span is narrower than the whole list's, k_gb_final's
# shift drops by at least one bit, and the bucket of 4097 splits into its two keys, 1 + 4096 --
# exactly GB_BIG_CAP, no overflow.  Equal keys share a bucket at any shift.
ONE_GROUP_EXTRA = 64
ONE_GROUP_N = 4097 + 2 + sc.GB_FILLER + ONE_GROUP_EXTRA


# ------------------------------------------------------------------ the selection
# layout -> distribution -> the rank counts it runs at.  Not the full product: every layout meets
# uniform keys at (nearly) every R and each other distribution at one R or more; the unordered
# layouts take the three distributions that must arrive out of index order at every R they can.
# empty_middle at R = 2 is rank 1, which is empty_last there, so empty_last starts at R = 3.
SELECTION = {
    "even":         {"uniform": (2, 3, 8), "one_dest_last": (3,), "edges": (2, 8), "step_straddle": (3,),
                     "one_group": (3,)},
    "uneven":       {"uniform": (2, 3, 8), "one_dest_first": (8,), "one_dest_last": (2, 3, 8), "edges": (3,),
                     "step_straddle": (2, 8)},
    "empty_first":  {"uniform": (3, 8), "one_dest_first": (2,), "step_straddle": (3,)},
    "empty_middle": {"uniform": (2, 3, 8), "one_dest_first": (2, 8), "one_dest_last": (3,), "edges": (8,),
                     "one_group": (8,)},
    "empty_last":   {"uniform": (3, 8), "one_dest_last": (8,), "step_straddle": (3,)},
    "only_last":    {"uniform": (2, 3, 8), "one_dest_first": (2, 8), "one_dest_last": (3,)},
    "masked_rank":  {"uniform": (2, 3, 8), "one_dest_last": (8,), "edges": (8,), "step_straddle": (3,)},
    "no_mask":      {"uniform": (2, 3), "one_dest_first": (8,), "edges": (2,), "step_straddle": (8,)},
    "random_mask":  {"uniform": (2, 3, 8), "one_dest_first": (3,), "edges": (8,), "step_straddle": (8,)},
    "descending":   {"uniform": (2, 3, 8), "one_dest_first": (2, 8), "one_dest_last": (3,),
                     "step_straddle": (2, 3, 8), "one_group": (2, 8)},
    "rotated":      {"uniform": (2, 3, 8), "one_dest_last": (8,), "edges": (3,), "step_straddle": (2, 3, 8),
                     "one_group": (3, 8)},
    "high_base":    {"uniform": (2, 3, 8), "one_dest_first": (3,), "edges": (8,), "step_straddle": (2,),
                     "one_group": (2,)},
}
CASE_COUNT = 85
CASES_PER_R = {2: 23, 3: 29, 8: 33}
# the dists that, on an unordered layout, must deliver some key out of index order
MUST_MISORDER = ("uniform", "step_straddle", "one_group")


@dataclass(frozen=True)
class Spec:
    layout: str
    dist: str
    R: int

    @property
    def name(self) -> str:
        return f"{self.layout}-{self.dist}-R{self.R}"

    @property
    def n_files(self) -> int:
        return ONE_GROUP_N if self.dist == "one_group" else N_FILES


def specs(R: Optional[int] = None) -> List[Spec]:
    """The selected cases in table order, of one rank count or of all."""
    out = [Spec(lay, dist, r) for lay in LAYOUTS for dist in DISTS for r in SELECTION[lay].get(dist, ())]
    assert set(SELECTION) == set(LAYOUTS) and all(set(v) <= set(DISTS) for v in SELECTION.values())
    assert len(out) == CASE_COUNT == sum(CASES_PER_R.values()) and 60 <= CASE_COUNT <= 90
    assert all(sum(1 for s in out if s.R == r) == CASES_PER_R[r] for r in RANKS) and {s.R for s in out} == set(RANKS)
    assert all(SELECTION[lay].get("uniform") for lay in LAYOUTS)  # every layout meets plain keys
    assert all({lay for lay in LAYOUTS if d in SELECTION[lay]} for d in DISTS)
    for lay in UNORDERED:
        assert all(SELECTION[lay].get(d) for d in MUST_MISORDER)
    return out if R is None else [s for s in out if s.R == R]


# ------------------------------------------------------------------ layouts
def _even(pieces: int, n: int, shift: int = 0) -> List[int]:
    """`pieces` shard sizes of about n / pieces; a cut whose index is a multiple of CHUNK moves up
    by one."""
    cuts = [0]
    for k in range(1, pieces):
        c = k * n // pieces
        cuts.append(c + ((c + shift) % CHUNK == 0))
    return np.diff(cuts + [n]).tolist()


def _uneven(pieces: int, n: int) -> List[int]:
    """the first pieces - 1 sizes from UNEVEN_SEQ, the last the rest"""
    head = list(UNEVEN_SEQ[:pieces - 1])
    assert len(head) == pieces - 1 and set(head) <= set(UNEVEN_SIZES) and n - sum(head) > 0
    return head + [n - sum(head)]


def _ranges(sizes, shift: int = 0) -> List[Tuple[int, int]]:
    out, at = [], shift
    for s in sizes:
        out.append((at, int(s)))
        at += int(s)
    return out


def layout(name: str, R: int, n: int) -> List[Tuple[int, int, str]]:
    """Per rank (index base, file count, mask kind of shape_cases.partition_mask)."""
    masks = ["ones"] * R
    if name in ("even", "no_mask"):
        rg = _ranges(_even(R, n))
        if name == "no_mask":
            masks = ["none"] * R
    elif name == "high_base":
        rg = _ranges(_even(R, n, HIGH_BASE), HIGH_BASE)
    elif name in EMPTY_RANK:  # n = 0 where a contiguous shard would start
        at = EMPTY_RANK[name](R)
        rg = _ranges(_uneven(R - 1, n))
        rg.insert(at, (rg[at][0] if at < R - 1 else n, 0))
    elif name == "only_last":
        rg = [(0, 0)] * (R - 1) + [(0, n)]
    else:
        rg = _ranges(_uneven(R, n))
        if name == "masked_rank":
            masks[MASKED_RANK] = "zeros"
        elif name == "random_mask":
            masks = ["random"] * R
        elif name == "descending":  # rank r holds the index range of rank R - 1 - r
            rg = rg[::-1]
        elif name == "rotated":  # rank 0 holds the last range: one adjacent violation
            rg = [rg[-1]] + rg[:-1]
        else:
            assert name == "uneven", name
    shards = [(b, k, m) for (b, k), m in zip(rg, masks)]
    assert len(shards) == R and sum(k for _, k, _ in shards) == n
    # the ranges tile [lo, lo + n) and no cut between two files is a step boundary
    live = sorted((b, k) for b, k, _ in shards if k)
    assert all(b0 + k0 == b1 for (b0, k0), (b1, _) in zip(live, live[1:]))
    assert live[0][0] == (HIGH_BASE if name == "high_base" else 0)
    assert all(b % CHUNK for b, _ in live[1:]), (name, R, n)
    violations = sum(1 for (b0, k0, _), (b1, _, _) in zip(shards, shards[1:]) if b0 + k0 > b1)
    assert violations == {"descending": R - 1, "rotated": 1}.get(name, 0)
    return shards


def shards_ascend(shards) -> bool:
    """dedup.shards_ascend's rule (exchange_plan's `ascending`): every rank's range ends before the
    next rank's starts."""
    return all(b0 + k0 <= b1 for (b0, k0, _), (b1, _, _) in zip(shards, shards[1:]))


# ------------------------------------------------------------------ key distributions
def _seed(*parts) -> int:
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def _uniform(nf: int, rng) -> np.ndarray:
    """random keys, about 30 % drawn again from an earlier file"""
    keys = rng.integers(0, 1 << 64, nf, dtype=U)
    again = rng.random(nf) < 0.3
    src = (rng.random(nf) * np.arange(nf)).astype(np.int64)
    for f in np.flatnonzero(again):
        if f:
            keys[f] = keys[src[f]]
    return keys


def dest_range(d: int, R: int) -> Tuple[int, int]:
    """[lo, hi): the keys sd_dedup_partition sends to rank d of R (the top 16 bits t with
    (t R) >> 16 == d)."""
    lo, hi = -(-d * 65536 // R), -(-(d + 1) * 65536 // R)
    return lo << 48, hi << 48


def _one_dest(nf: int, d: int, R: int, rng) -> np.ndarray:
    lo, hi = dest_range(d, R)
    keys = U(lo) + _uniform(nf, rng) % U(hi - lo)
    assert (dest_of(keys, R) == d).all()
    return keys


class _Files:
    """The files of a layout flattened in rank order: rank, local position, global index and
    validity of each."""

    def __init__(self, shards, valid):
        self.rank = np.concatenate([np.full(k, r, np.int64) for r, (_, k, _) in enumerate(shards)])
        self.index = np.concatenate([np.arange(b, b + k, dtype=np.int64) for b, k, _ in shards])
        self.valid = np.concatenate([np.ones(k, bool) if v is None else v.astype(bool)
                                     for (_, k, _), v in zip(shards, valid)])
        self.at = {int(i): f for f, i in enumerate(self.index)}  # global index -> flat position
        self.nf = len(self.index)
        # the ranks that hold a valid file, and their valid flat positions in order
        self.slots = {r: np.flatnonzero((self.rank == r) & self.valid).tolist() for r in range(len(shards))}
        self.live = [r for r, s in self.slots.items() if s]


def _edges(files: _Files, R: int, rng) -> np.ndarray:
    """crafted_keys(R), each on valid files of two different ranks, the rest uniform"""
    keys = _uniform(files.nf, rng)
    assert len(files.live) >= 2
    nxt = {r: 0 for r in files.live}

    def take(start: int, avoid: int) -> int:
        for j in range(len(files.live)):
            r = files.live[(start + j) % len(files.live)]
            if r != avoid and nxt[r] < len(files.slots[r]):
                nxt[r] += 1
                return r
        raise AssertionError("no rank has room for a crafted key")

    crafted = sc.crafted_keys(R)
    for j, k in enumerate(crafted):
        a = take(j, -1)
        b = take(j + 1, a)
        keys[files.slots[a][nxt[a] - 1]] = keys[files.slots[b][nxt[b] - 1]] = U(k)
    for k in set(crafted):
        holders = np.unique(files.rank[(keys == U(k)) & files.valid])
        assert len(holders) >= 2, (k, holders)
    return keys


def _step_straddle(files: _Files, shards, rng) -> Tuple[np.ndarray, int]:
    """Uniform keys, then at every cut the files either side of it that share an identifier step
    made equal -- (c - 1, c) and, where the step reaches, (c - 2, c + 1) -- and a third copy three
    steps later, which links to the pair's first.  -> (keys, valid pairs across ranks)."""
    keys = _uniform(files.nf, rng)
    live = sorted((b, k) for b, k, _ in shards if k)
    fixed = {}
    pairs = 0
    for (b0, _), (c, k1) in zip(live, live[1:]):
        for i, j in ((c - 1, c), (c - 2, c + 1)):
            if i < b0 or j >= c + k1 or i // CHUNK != j // CHUNK:
                continue
            k = fixed.get(i, fixed.get(j))
            if k is None:
                k = rng.integers(0, 1 << 64, dtype=U)
            for x in (i, j, j + 3 * CHUNK):
                if x in files.at and x not in fixed:
                    fixed[x] = k
                    keys[files.at[x]] = k
            fi, fj = files.at[i], files.at[j]
            assert files.rank[fi] != files.rank[fj] and keys[fi] == keys[fj]
            pairs += int(files.valid[fi] and files.valid[fj])
    return keys, pairs


def one_group_keys() -> np.ndarray:
    """bucket_case(4097, "late", True)'s keys with ONE_GROUP_EXTRA more copies of the 4096-fold one
    at seeded places."""
    base = np.ascontiguousarray(sc.bucket_case(sc.GB_BIG_CAP + 1, "late", True)[:, 0]).view(U)
    uniq, cnt = np.unique(base, return_counts=True)
    assert cnt.max() == sc.GB_BIG_CAP and (cnt == cnt.max()).sum() == 1
    heavy = uniq[np.argmax(cnt)]
    rng = np.random.default_rng(4097)
    keys = np.insert(base, np.sort(rng.integers(0, len(base), ONE_GROUP_EXTRA)), heavy)
    assert len(keys) == ONE_GROUP_N and (keys == heavy).sum() == sc.GB_BIG_CAP + ONE_GROUP_EXTRA
    return keys


def _one_group(files: _Files, R: int) -> np.ndarray:
    """one_group_keys dealt round-robin over the ranks that hold files (a full rank is passed over)"""
    src = one_group_keys()
    assert files.valid.all() and files.nf == len(src)
    keys = np.zeros(files.nf, U)
    room = {r: list(np.flatnonzero(files.rank == r)) for r in range(R)}
    nxt = {r: 0 for r in room}
    order = [r for r in room if room[r]]
    r_at = 0
    for k in src:
        while nxt[order[r_at % len(order)]] >= len(room[order[r_at % len(order)]]):
            r_at += 1
        r = order[r_at % len(order)]
        keys[room[r][nxt[r]]] = k
        nxt[r] += 1
        r_at += 1
    return keys


# ------------------------------------------------------------------ a case and its expectations
@dataclass
class Want:
    """What one rank returns: m records sorted by (key, index), rep, the group count, the owners."""
    m: int
    records: np.ndarray  # int64 [m, 2]
    rep: np.ndarray      # int64 [m]
    n_groups: int
    owner: np.ndarray    # int64 [m]


@dataclass
class Case:
    spec: Spec
    shards: List[Tuple[int, int, str]]
    keys: List[np.ndarray]              # per rank, u64 [n]
    hashes: List[np.ndarray]            # per rank, uint8 [n, 32]
    valid: List[Optional[np.ndarray]]   # per rank, uint8 [n] or None (d_valid == NULL)
    ascending: bool
    want: List[Want]
    recv: List[np.ndarray]              # per rank, the records in simulated arrival order
    all_recs: np.ndarray = field(repr=False, default=None)  # every valid record, rank order

    @property
    def name(self) -> str:
        return self.spec.name

    @property
    def R(self) -> int:
        return self.spec.R

    @property
    def need(self) -> List[int]:
        return [w.m for w in self.want]


def arrival(recs_by_rank, R: int) -> List[np.ndarray]:
    """The receive order of every destination: the concatenation, in source-rank order, of each
    rank's stable partition_host slice for it."""
    parts = [partition_host(np.ascontiguousarray(r[:, 0]).view(U), r[:, 1], R) for r in recs_by_rank]
    out = []
    for d in range(R):
        pieces = []
        for recs, counts in parts:
            off = int(counts[:d].sum())
            pieces.append(recs[off:off + int(counts[d])])
        out.append(np.concatenate(pieces).reshape(-1, 2))
    return out


def _by_key(recv: np.ndarray):
    """the records in a stable sort by key alone: equal keys stay in arrival order"""
    k = np.ascontiguousarray(recv[:, 0]).view(U)
    o = np.argsort(k, kind="stable")
    ks = k[o]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    return recv[o], head


def in_index_order(recv: np.ndarray) -> bool:
    """within every key the indices ascend in arrival order"""
    r, head = _by_key(recv)
    return bool((np.diff(r[:, 1]) > 0)[~head[1:]].all())


def rep_by_arrival(recv: np.ndarray):
    """What a grouping that trusts the arrival order (SD_DEDUP_INDEX_SORTED) computes: one stable
    sort by key, rep = the index of the key's first-arriving record.  -> (records, rep)"""
    r, head = _by_key(recv)
    if len(r) == 0:
        return r, np.zeros(0, np.int64)
    pos = np.maximum.accumulate(np.where(head, np.arange(len(r)), 0))
    return r, r[pos, 1]


def first_not_smallest(recv: np.ndarray) -> int:
    """the keys whose first-arriving record is not their smallest index"""
    r, rep = rep_by_arrival(recv)
    _, head = _by_key(recv)
    least = np.minimum.reduceat(r[:, 1], np.flatnonzero(head)) if len(r) else np.zeros(0, np.int64)
    return int((rep[head] != least).sum())


@functools.lru_cache(maxsize=None)
def case(spec: Spec) -> Case:
    R, n = spec.R, spec.n_files
    shards = layout(spec.layout, R, n)
    seed = _seed(spec.layout, spec.dist, R)
    valid = [None if m == "none" else sc.partition_mask(m, k, seed % 1000 + 7 * r)
             for r, (_, k, m) in enumerate(shards)]
    files = _Files(shards, valid)
    rng = np.random.default_rng(seed)
    if spec.dist == "uniform":
        keys = _uniform(n, rng)
    elif spec.dist in ("one_dest_first", "one_dest_last"):
        keys = _one_dest(n, 0 if spec.dist == "one_dest_first" else R - 1, R, rng)
    elif spec.dist == "edges":
        keys = _edges(files, R, rng)
    elif spec.dist == "step_straddle":
        keys, pairs = _step_straddle(files, shards, rng)
        assert pairs >= 1, spec
    else:
        assert spec.dist == "one_group", spec
        keys = _one_group(files, R)
    assert len(keys) == n == files.nf
    ends = np.cumsum([0] + [k for _, k, _ in shards])
    keys_r = [keys[a:b].copy() for a, b in zip(ends, ends[1:])]
    hashes = [sc.hashes_from_keys(k, seed % 1000 + r) for r, k in enumerate(keys_r)]
    recs_r = []
    for r, (b, k, _) in enumerate(shards):
        ok = files.valid[ends[r]:ends[r + 1]]
        recs_r.append(np.stack([keys_r[r][ok].view(np.int64), np.arange(b, b + k, dtype=np.int64)[ok]], axis=1))
    all_recs = np.concatenate(recs_r)
    dst = dest_of(np.ascontiguousarray(all_recs[:, 0]).view(U), R)
    want = []
    for d in range(R):
        gr, grep, gng = group_host(all_recs[dst == d])
        own = object_owners(torch.from_numpy(np.ascontiguousarray(gr[:, 1])), torch.from_numpy(grep), CHUNK).numpy()
        want.append(Want(len(gr), gr, grep, gng, own))
    c = Case(spec, shards, keys_r, hashes, valid, shards_ascend(shards), want, arrival(recs_r, R), all_recs)
    _self_check(c)
    for a in [*c.keys, *c.hashes, *[v for v in c.valid if v is not None], c.all_recs, *c.recv,
              *[x for w in c.want for x in (w.records, w.rep, w.owner)]]:
        a.flags.writeable = False  # shared between the tests: computed once, left unchanged
    return c


def _self_check(c: Case) -> None:
    """What makes the sweep mean something, per case (the issue's list)."""
    lay, dist, R = c.spec.layout, c.spec.dist, c.R
    assert c.ascending == (lay not in UNORDERED), c.name
    assert sum(c.need) == len(c.all_recs) and [len(x) for x in c.recv] == c.need, c.name
    for d in range(R):  # the simulated arrival is a permutation of what the rank must return
        got = c.recv[d][np.lexsort((c.recv[d][:, 1], c.recv[d][:, 0].view(U)))]
        assert np.array_equal(got, c.want[d].records), (c.name, d)
    ordered = [in_index_order(x) for x in c.recv]
    if c.ascending:
        # arrival order may be trusted: a grouping that does gets the same rep
        assert all(ordered), c.name
        for d in range(R):
            r, rep = rep_by_arrival(c.recv[d])
            assert np.array_equal(r, c.want[d].records) and np.array_equal(rep, c.want[d].rep), (c.name, d)
    elif dist in MUST_MISORDER:
        # ... and may not: some key's first-arriving record is not its smallest index, so a
        # grouping handed SD_DEDUP_INDEX_SORTED regardless returns another rep for it
        assert not all(ordered), c.name
        wrong = [d for d in range(R) if not np.array_equal(rep_by_arrival(c.recv[d])[1], c.want[d].rep)]
        assert wrong and sum(first_not_smallest(x) for x in c.recv) >= 1, c.name
    if dist in ("one_dest_first", "one_dest_last"):
        target = 0 if dist == "one_dest_first" else R - 1
        assert [d for d in range(R) if c.need[d]] == [target] and sorted(c.need)[:R - 1] == [0] * (R - 1), c.name
    if lay in EMPTY_RANK:  # the empty rank sends nothing and still receives
        e = EMPTY_RANK[lay](R)
        assert c.shards[e][1] == 0
        if not (dist.startswith("one_dest") and c.need[e] == 0):
            assert c.need[e] > 0, c.name
    if lay == "only_last":
        assert [k for _, k, _ in c.shards[:-1]] == [0] * (R - 1)
        if not dist.startswith("one_dest"):
            assert all(x > 0 for x in c.need), c.name  # every empty rank receives
    if lay == "masked_rank":
        assert c.shards[MASKED_RANK][1] > 0 and not c.valid[MASKED_RANK].any()
    if lay == "no_mask":
        assert all(v is None for v in c.valid)
    if lay == "random_mask":
        assert all(0 < v.sum() < len(v) for v in c.valid if len(v) > 1)
    if lay == "high_base":
        assert int(c.all_recs[:, 1].min()) == HIGH_BASE and c.all_recs[:, 1].max() >= 1 << 40
    if dist == "one_group":
        heavy = [d for d in range(R) if c.need[d] > sc.GB_BIG_CAP]
        assert len(heavy) == 1, c.name
        rk = np.ascontiguousarray(c.want[heavy[0]].records[:, 0]).view(U)
        assert sc.gb_bucket_sizes(rk).max() > sc.GB_BIG_CAP, c.name  # the overflow fallback really runs
        uniq, cnt = np.unique(rk, return_counts=True)
        big = uniq[np.argmax(cnt)]
        assert cnt.max() == sc.GB_BIG_CAP + ONE_GROUP_EXTRA
        holders = [r for r in range(R) if (c.keys[r] == big).any()]  # the group comes in pieces
        assert len(holders) >= max(2, sum(1 for _, k, _ in c.shards if k > 1)), c.name
    if dist == "uniform":  # duplicates cross shards
        holders, stocked = {}, 0
        for r in range(R):
            ok = np.ones(len(c.keys[r]), bool) if c.valid[r] is None else c.valid[r].astype(bool)
            stocked += int(ok.sum() >= 100)
            for k in np.unique(c.keys[r][ok]).tolist():
                holders[k] = holders.get(k, 0) + 1
        if stocked >= 2:  # (only_last, and masked_rank at R = 2, have one rank with valid files)
            assert max(holders.values()) >= 2, c.name


def all_cases(R: Optional[int] = None) -> List[Case]:
    return [case(s) for s in specs(R)]


# ------------------------------------------------------------------ the subsets the GPU module runs
def gpu_order(R: int) -> List[Spec]:
    """The cases of one R in the order the GPU module runs them on one set of communicators:
    by rank 0's file count, alternately one of the smaller half and one of the larger half, each
    half ascending, so that a rank's send buffer is reused below its size and regrown past it
    several times."""
    by = sorted(specs(R), key=lambda s: (layout(s.layout, R, s.n_files)[0][1], s.name))
    half = (len(by) + 1) // 2
    out = [s for pair in zip(by[:half], by[half:] + [None]) for s in pair if s is not None]
    assert len(out) == CASES_PER_R[R]
    held, grown, reused = 0, 0, 0
    for s in out:
        n0 = max(layout(s.layout, R, s.n_files)[0][1], 1)
        grown += held and n0 > held
        reused += n0 < held
        held = max(held, n0)
    assert grown >= 2 and reused >= 5, (R, grown, reused)
    return out


def variant_specs(R: int) -> List[Spec]:
    """The cases both dedup variants run: the unordered layouts and the one_group distribution."""
    out = [s for s in specs(R) if s.layout in UNORDERED or s.dist == "one_group"]
    assert len(out) == {2: 7, 3: 8, 8: 9}[R]
    assert {s.layout for s in out} >= set(UNORDERED) and any(s.dist == "one_group" for s in out)
    return out


CAPACITY_CASES = (("even", "uniform"), ("uneven", "one_dest_last"))


def capacity_specs(R: int) -> List[Spec]:
    out = [Spec(lay, dist, R) for lay, dist in CAPACITY_CASES]
    assert all(s in specs(R) for s in out) and len(out) == 2
    return out


INDEXED_LAYOUTS = ("empty_middle", "only_last", "descending")


def indexed_specs(R: int) -> List[Spec]:
    """sd_cas_dedup_mgpu_indexed: uniform on the three layouts at every R, one_dest_first at 2 and 8."""
    out = [Spec(lay, "uniform", R) for lay in INDEXED_LAYOUTS]
    if R in (2, 8):
        out += [Spec(lay, "one_dest_first", R) for lay in INDEXED_LAYOUTS]
    assert all(s in specs(R) for s in out) and len(out) == (6 if R in (2, 8) else 3)
    return out


# ------------------------------------------------------------------ split checksums with idle ranks
SPLIT_TOTALS = (0, 1, MiB, MiB + 1, 3 * MiB + 5)
SPLIT_RANKS = (2, 4, 8)
SPLIT_CASES = 15


def split_expect(total: int, R: int):
    """sd_split_range in Python integers -> (nb, q, cv_bytes, [(offset, len, first block, end
    block) per rank]): nb 1 MiB blocks (an empty file has one), q = ceil(nb / R) slots per rank."""
    nb = max((total + MiB - 1) // MiB, 1)
    q = -(-nb // R)
    ranks = []
    for r in range(R):
        b0 = min(nb, r * q)
        b1 = min(nb, b0 + q)
        off = min(total, b0 * MiB)
        ranks.append((off, min(total, b1 * MiB) - off, b0, b1))
    return nb, q, R * q * 32, ranks


def split_cases():
    """(total, R, nb, q, cv_bytes, ranks) for every total and rank count: among them files with
    fewer blocks than ranks (idle ranks) and one-block files (the root is slot 0)."""
    out = [(t, R, *split_expect(t, R)) for R in SPLIT_RANKS for t in SPLIT_TOTALS]
    assert len(out) == SPLIT_CASES == len(SPLIT_TOTALS) * len(SPLIT_RANKS)
    assert sum(1 for _, R, nb, *_ in out if nb < R) == 5 + 4 + 3  # every rank count has idle ranks
    assert sum(1 for _, _, nb, *_ in out if nb == 1) == 9
    assert any(nb >= R for _, R, nb, *_ in out)  # and a file with a block for every rank
    for t, R, nb, q, cvb, ranks in out:
        assert sum(n for _, n, _, _ in ranks) == t and sum(b1 - b0 for _, _, b0, b1 in ranks) == nb
        assert sum(1 for _, _, b0, b1 in ranks if b0 == b1) == R - -(-nb // q)  # the idle ranks
        assert cvb >= nb * 32
    return out
