"""Post-hash duplicate grouping across GPUs.

Reference semantics (core/src/object/file_identifier/mod.rs:136-333): after hashing a
step's files, each file_path is linked to an Object that already owns an equal cas_id,
otherwise a new Object is created; size-0 files (cas_id None, mod.rs:80-88) never
dedup.  The partition of files into equal-cas_id groups is what this module computes,
bit-exactly; which member becomes the Object is a policy of the caller (the reference's
choice depends on 100-row chunking and HashMap order, §8(e)), here the smallest global
file index of the group (the "Object-link candidate").

Multi-GPU: files are sharded by index; each rank buckets its records
``(cas_id as big-endian u64, global index)`` by cas_id prefix (device kernel
``sd_dedup_partition``), the records move to the rank owning their prefix range, and
each rank sorts and groups its bucket (``sd_dedup_group``) and assigns Objects
(``sd_dedup_owners``).  Two transports for the exchange:

* ``dedup_shard_rccl`` -- the product path on GPUs: the whole step behind the C ABI
  (``sd_cas_dedup_mgpu``): an RCCL all-gather of the count matrix, then grouped
  ncclSend/ncclRecv of the records (the all-to-all over xGMI), on libsdcas's own RCCL
  communicator (``make_comm``), so a Rust host drives the same code;
* ``dedup_shard`` -- the same step with the exchange in ``torch.distributed``
  (``all_to_all_single``), which also runs on "gloo" for the CPU tests.

No other collective exists on the data path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist


def shard_plan(sizes, nranks: int) -> np.ndarray:
    """Contiguous index ranges of balanced hashing cost for a library scan over `nranks`
    GPUs (sd_shard_plan): rank r hashes files [bounds[r], bounds[r+1]).  The cost of a file
    is the BLAKE3 compressions of its cas message."""
    import ctypes
    from ._native import check, lib
    s = np.ascontiguousarray(sizes, dtype=np.uint64)
    bounds = np.zeros(nranks + 1, np.uint64)
    check(lib().sd_shard_plan(s.ctypes.data if s.size else None, ctypes.c_size_t(s.size), nranks, bounds.ctypes.data))
    return bounds


def dest_of(keys: np.ndarray, nparts: int) -> np.ndarray:
    """Destination rank of a cas_id key: its top 16 bits scaled to nparts (contiguous ranges)."""
    return (((keys >> np.uint64(48)) * np.uint64(nparts)) >> np.uint64(16)).astype(np.int64)


def keys_from_hashes(h32: np.ndarray) -> np.ndarray:
    """First 8 hash bytes as a big-endian u64 (== the hex cas_id's lexicographic order)."""
    return h32[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)


def exchange(send_records: torch.Tensor, send_counts: torch.Tensor,
             group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
    """All-to-all of records grouped by destination.

    send_records: int64 [m, 2] (key, global index) ordered by destination rank;
    send_counts:  int64 [world] records per destination.  Returns the received records.
    Works for any backend whose tensors live on the device of ``send_records``.
    """
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return send_records
    if dist.get_backend(group) == "gloo" and send_records.is_cuda:
        # CPU transport (tests / single-GPU rehearsal): same exchange, host tensors
        dev = send_records.device
        return exchange(send_records.cpu(), send_counts.cpu(), group).to(dev)
    recv_counts = torch.empty_like(send_counts)
    dist.all_to_all_single(recv_counts, send_counts, group=group)
    rc = recv_counts.cpu().tolist()
    sc = send_counts.cpu().tolist()
    out = torch.empty((int(sum(rc)), 2), dtype=send_records.dtype, device=send_records.device)
    dist.all_to_all_single(out, send_records, output_split_sizes=rc, input_split_sizes=sc, group=group)
    return out


def group_device(ctx, records: torch.Tensor, index_sorted: bool = False) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Sort received records by (cas_id, index) and map each to its group's smallest index."""
    m = records.shape[0]
    rep = torch.empty(max(m, 1), dtype=torch.int64, device=records.device)
    ng = ctx.dedup_group(records, m, rep, index_sorted=index_sorted)
    return records, rep[:m], ng


def keys_from_hashes_device(d_cas_hash32: torch.Tensor, ctx=None) -> torch.Tensor:
    """keys_from_hashes on the device: the cas key (int64 carrying the big-endian u64 of the
    first 8 bytes) of every row of d_cas_hash32 (uint8 [n, 32], e.g. what
    sd_fingerprint_batch_run leaves in d_cas_hash32), in row order.  It is sd_dedup_partition
    over one destination: stable, so the records' key column is the answer."""
    from .device import default_context
    n = int(d_cas_hash32.numel() // 32)
    dev = d_cas_hash32.device
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    assert d_cas_hash32.dtype == torch.uint8 and d_cas_hash32.is_cuda and d_cas_hash32.is_contiguous()
    ctx = default_context(dev.index) if ctx is None else ctx
    counts = torch.empty(1, dtype=torch.int64, device=dev)
    recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
    nv = ctx.dedup_partition(d_cas_hash32, None, n, 0, 1, counts, recs)
    assert nv == n
    return recs[:, 0].contiguous()


def confirm_device(ctx, d_keys: torch.Tensor, d_hash32: torch.Tensor, d_valid: Optional[torch.Tensor] = None,
                   stream=None):
    """sd_dedup_confirm: the candidate groups of m files (d_keys int64 [m] cas keys, d_hash32 uint8
    [m, 32] full checksums, d_valid uint8 [m] or None) split into classes of equal checksums.
    Returns (rep int64 [m], class_size int64 [m], verdict uint8 [m], sets int64 [n_sets, 3] =
    (key, rep, size) ascending by (key, checksum), stats uint64 [8]); include/sd_cas.h has the
    rules.  A class has at least two members, so m // 2 rows always hold the sets."""
    m = int(d_keys.numel())
    dev = d_hash32.device if m else torch.device("cuda", ctx.device)
    assert m == 0 or (d_keys.dtype == torch.int64 and d_keys.is_cuda and d_keys.is_contiguous())
    assert m == 0 or (d_hash32.dtype == torch.uint8 and d_hash32.is_contiguous() and d_hash32.numel() == 32 * m)
    assert d_valid is None or (d_valid.dtype == torch.uint8 and d_valid.is_contiguous() and d_valid.numel() >= m)
    rep = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    size = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    verdict = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
    cap = m // 2
    sets = torch.empty((max(cap, 1), 3), dtype=torch.int64, device=dev)
    n_sets, stats = ctx.dedup_confirm(d_keys, d_hash32, d_valid if m else None, m, rep, size, verdict, sets, cap, stream)
    return rep[:m], size[:m], verdict[:m], sets[:n_sets], stats


def shards_ascend(n_local: int, global_base: int, group: Optional[dist.ProcessGroup] = None,
                   device=None) -> bool:
    """True when every rank's index range [base, base + n) ends before the next rank's
    starts: the records received in rank order are then in ascending index order."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return True
    mine = torch.tensor([global_base, n_local], dtype=torch.int64, device=device)
    rows = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(rows, mine, group=group)
    r = torch.stack(rows).cpu().tolist()
    return all(r[k][0] + r[k][1] <= r[k + 1][0] for k in range(world - 1))


def dedup_shard(ctx, d_hash32: torch.Tensor, d_valid: Optional[torch.Tensor], n_local: int, global_base: int,
                group: Optional[dist.ProcessGroup] = None, index_sorted: Optional[bool] = None, index=None):
    """Full distributed step on one rank: partition -> exchange -> group -> Object owners.

    Returns (records int64 [m, 2] sorted by (key, index), rep int64 [m], n_groups,
    owner int64 [m]) for the cas_id prefix range this rank owns; owner is the file whose
    Object each record links to under the reference's chunk-of-100 rule
    (spacedrive_amd/identifier.py).  ``index_sorted``: whether the shards' index ranges
    ascend with the rank (checked with one small all-gather when None).

    With ``index`` (a device.ObjectIndex sharded as this rank's prefix range) the owners come
    from sd_dedup_owners_indexed -- a file whose cas_id the library already has links to that
    Object (file_identifier/mod.rs:168-225) -- and the tuple gains (existing uint8 [m], new
    heads int64 [n_new, 2] = (key, creating file index) in ascending key order).
    """
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    dev = d_hash32.device
    if index_sorted is None:
        gloo = world > 1 and dist.get_backend(group) == "gloo"
        index_sorted = shards_ascend(n_local, global_base, group, "cpu" if gloo else dev)
    counts = torch.empty(world, dtype=torch.int64, device=dev)
    recs = torch.empty((max(n_local, 1), 2), dtype=torch.int64, device=dev)
    nv = ctx.dedup_partition(d_hash32, d_valid, n_local, global_base, world, counts, recs)
    recv = exchange(recs[:nv], counts, group)
    # the partition is stable: with ascending shards the received records are in index
    # order, and one stable cas_id sort suffices
    records, rep, ng = group_device(ctx, recv, index_sorted=index_sorted)
    # identifier.object_owners is the torch statement of the same rule (tests compare them)
    m = records.shape[0]
    owners = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    if index is None:
        ctx.dedup_owners(records, m, rep, owners)
        return records, rep, ng, owners[:m]
    existing = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
    new = torch.empty((max(m, 1), 2), dtype=torch.int64, device=dev)
    n_new = torch.zeros(1, dtype=torch.int64, device=dev)
    index.owners(records, m, rep, owners, existing, new, n_new)
    return records, rep, ng, owners[:m], existing[:m], new[:int(n_new.item())]


def make_comm(ctx, group: Optional[dist.ProcessGroup] = None):
    """libsdcas's RCCL communicator over the ranks of ``group``: rank 0's ncclUniqueId is
    broadcast through torch.distributed, then every rank joins (sd_comm_create)."""
    from .device import Comm
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    uid = [Comm.unique_id() if rank == 0 else None]
    if world > 1:
        dist.broadcast_object_list(uid, src=0, group=group)
    return Comm(ctx, uid[0], world, rank)


class RcclDedup:
    """sd_cas_dedup_mgpu with reusable output buffers (grown when a rank needs more)."""

    def __init__(self, ctx, comm, device, capacity: int = 0):
        self.ctx, self.comm, self.device = ctx, comm, device
        self.capacity = 0
        self._alloc(capacity)

    def _alloc(self, cap: int) -> None:
        cap = max(int(cap), 1)
        if cap > self.capacity:
            self.records = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
            self.rep = torch.empty(cap, dtype=torch.int64, device=self.device)
            self.owner = torch.empty(cap, dtype=torch.int64, device=self.device)
            self.existing = self.new = None  # allocated by the first call that brings an index
            self.capacity = cap

    def __call__(self, d_hash32, d_valid, n_local: int, global_base: int, chunk_size: int = 100, stream=None,
                 index=None):
        """With ``index`` (this rank's shard of the Object index) the tuple gains (existing
        uint8 [m], new heads int64 [n_new, 2]), as dedup_shard's does."""
        from ._native import SD_ERR_CAPACITY, SdCasError
        for _ in range(2):
            try:
                if index is not None:
                    if self.existing is None:
                        self.existing = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
                        self.new = torch.empty((self.capacity, 2), dtype=torch.int64, device=self.device)
                    m, ng, nn = self.ctx.dedup_mgpu_indexed(self.comm, d_hash32, d_valid, n_local, global_base,
                                                            self.records, self.rep, self.owner, self.capacity, index,
                                                            self.existing, self.new, chunk_size, stream)
                    return self.records[:m], self.rep[:m], ng, self.owner[:m], self.existing[:m], self.new[:nn]
                m, ng = self.ctx.dedup_mgpu(self.comm, d_hash32, d_valid, n_local, global_base, self.records,
                                            self.rep, self.owner, self.capacity, chunk_size, stream)
                return self.records[:m], self.rep[:m], ng, self.owner[:m]
            except SdCasError as e:
                if e.rc != SD_ERR_CAPACITY:
                    raise
                # every rank stopped before the exchange: all retry, each with room for its need
                self._alloc(max(e.needed, self.capacity) * 5 // 4 + 1024)
        raise RuntimeError("sd_cas_dedup_mgpu: capacity still short after regrowing")


def dedup_shard_rccl(ctx, comm, d_hash32: torch.Tensor, d_valid: Optional[torch.Tensor], n_local: int,
                     global_base: int, capacity: Optional[int] = None):
    """dedup_shard through the C ABI's RCCL exchange (sd_cas_dedup_mgpu); same outputs."""
    runner = RcclDedup(ctx, comm, d_hash32.device, capacity if capacity is not None else n_local + 4096)
    return runner(d_hash32, d_valid, n_local, global_base)


# ------------------------------------------------------------------ host reference
def partition_host(keys: np.ndarray, idx: np.ndarray, nparts: int):
    """Host mirror of sd_dedup_partition: stable, grouped by destination, input order within one."""
    d = dest_of(keys, nparts)
    order = np.argsort(d, kind="stable")
    counts = np.bincount(d, minlength=nparts).astype(np.int64)
    recs = np.stack([keys[order].view(np.int64), idx[order].astype(np.int64)], axis=1)
    return recs, counts


def group_host(records: np.ndarray):
    """Host mirror of sd_dedup_group: sort by (key, index); rep = min index of the group."""
    if len(records) == 0:
        return records, np.zeros(0, np.int64), 0
    k = records[:, 0].view(np.uint64)
    i = records[:, 1]
    order = np.lexsort((i, k))
    r = records[order]
    ks = r[:, 0].view(np.uint64)
    head = np.ones(len(r), bool)
    head[1:] = ks[1:] != ks[:-1]
    head_pos = np.maximum.accumulate(np.where(head, np.arange(len(r)), 0))
    return r, r[head_pos, 1], int(head.sum())


def confirm_host(keys, hash32, valid=None):
    """Host mirror of sd_dedup_confirm in numpy: keys uint64 [m], hash32 uint8 [m, 32], valid
    uint8 / bool [m] or None.  Returns (rep uint64 [m], class_size uint64 [m], verdict uint8 [m],
    sets uint64 [n_sets, 3], stats uint64 [8]).  The order is one lexsort by (key, the four
    checksum words as big-endian numbers, position) over the valid files."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    m = len(keys)
    h = np.ascontiguousarray(hash32, dtype=np.uint8).reshape(m, 32)
    ok = np.ones(m, bool) if valid is None else np.asarray(valid).reshape(-1)[:m] != 0
    rep = np.full(m, np.iinfo(np.uint64).max, np.uint64)
    size = np.zeros(m, np.uint64)
    verdict = np.zeros(m, np.uint8)
    stats = np.zeros(8, np.uint64)
    pos = np.flatnonzero(ok).astype(np.uint64)
    v = len(pos)
    if v == 0:
        return rep, size, verdict, np.zeros((0, 3), np.uint64), stats
    w = h[ok].copy().view(">u8").astype(np.uint64)  # [v, 4]
    k = keys[ok]
    order = np.lexsort((pos, w[:, 3], w[:, 2], w[:, 1], w[:, 0], k))
    ks, ws, ps = k[order], w[order], pos[order]
    ghead = np.ones(v, bool)
    ghead[1:] = ks[1:] != ks[:-1]
    chead = ghead.copy()
    chead[1:] |= (ws[1:] != ws[:-1]).any(axis=1)
    cstart, gstart = np.flatnonzero(chead), np.flatnonzero(ghead)
    csize = np.diff(np.append(cstart, v)).astype(np.uint64)
    gsize = np.diff(np.append(gstart, v)).astype(np.uint64)
    cof, gof = np.cumsum(chead) - 1, np.cumsum(ghead) - 1  # class / group of every sorted place
    rep[ps] = ps[cstart][cof]
    size[ps] = csize[cof]
    verdict[ps] = np.where(gsize[gof] == 1, 1, np.where(csize[cof] >= 2, 2, 3)).astype(np.uint8)
    conf = csize >= 2
    sets = np.stack([ks[cstart][conf], ps[cstart][conf], csize[conf]], axis=1).astype(np.uint64)
    classes_in_group = np.add.reduceat(chead.astype(np.int64), gstart)
    stats[:] = [v, len(gstart), int((gsize >= 2).sum()), len(cstart), int(conf.sum()), int(csize[conf].sum()),
                int((verdict == 3).sum()), int(((gsize >= 2) & (classes_in_group >= 2)).sum())]
    return rep, size, verdict, sets.reshape(-1, 3), stats


def index_insert_host(keys: np.ndarray, vals: np.ndarray, new_keys, new_vals, nparts: int = 1, part: int = 0):
    """Host mirror of sd_object_index_insert on an index given as (keys uint64 ascending,
    vals uint64): keep first -- an entry the index has wins, then the earliest pair of a key
    in input (DB) order -- and only keys of shard `part` of `nparts`.  Returns (keys, vals,
    taken)."""
    nk = np.ascontiguousarray(new_keys, dtype=np.uint64).reshape(-1)
    nv = np.ascontiguousarray(new_vals, dtype=np.uint64).reshape(-1)
    order = np.argsort(nk, kind="stable")
    nk, nv = nk[order], nv[order]
    first = np.ones(len(nk), bool)
    first[1:] = nk[1:] != nk[:-1]
    keep = first & (dest_of(nk, nparts) == part) & ~np.isin(nk, keys)
    nk, nv = nk[keep], nv[keep]
    allk = np.concatenate([np.asarray(keys, np.uint64), nk])
    allv = np.concatenate([np.asarray(vals, np.uint64), nv])
    o = np.argsort(allk, kind="stable")
    return allk[o], allv[o], int(keep.sum())


def _index_drop(keys: np.ndarray, vals: np.ndarray, drop: np.ndarray):
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint64)
    return keys[~drop], vals[~drop], np.stack([keys[drop], vals[drop]], axis=1)


def index_remove_host(keys: np.ndarray, vals: np.ndarray, rm_keys, rm_ids=None):
    """Host mirror of sd_object_index_remove on an index given as (keys uint64 ascending, vals
    uint64): entry (k, v) goes iff some pair i has rm_keys[i] == k and (rm_ids is None or
    rm_ids[i] == v).  Returns (keys, vals, removed pairs uint64 [r, 2] ascending by key)."""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint64)
    rk = np.ascontiguousarray(rm_keys, dtype=np.uint64).reshape(-1)
    drop = np.zeros(len(keys), bool)
    if len(keys) and len(rk):
        at = np.minimum(np.searchsorted(keys, rk), len(keys) - 1)
        hit = keys[at] == rk
        if rm_ids is not None:
            hit &= vals[at] == np.ascontiguousarray(rm_ids, dtype=np.uint64).reshape(-1)
        drop[at[hit]] = True
    return _index_drop(keys, vals, drop)


def index_remove_objects_host(keys: np.ndarray, vals: np.ndarray, ids):
    """Host mirror of sd_object_index_remove_objects: every entry whose Object id is among
    `ids` goes.  Returns (keys, vals, removed pairs uint64 [r, 2] ascending by key)."""
    drop = np.isin(np.asarray(vals, np.uint64), np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1))
    return _index_drop(keys, vals, drop)


# ---- the owners mode (SD_OBJECT_INDEX_OWNERS): an index given as (keys uint64 ascending, vals
# uint64 ascending within equal keys, links uint64 >= 1), one entry per (key, Object id) pair
def _pair_codes(*pairs):
    """(keys, ids) lists -> one int64 code array per list: equal pairs get equal codes, and the
    codes ascend with (key, id) (unsigned)."""
    k = np.concatenate([np.asarray(p[0], np.uint64) for p in pairs])
    v = np.concatenate([np.asarray(p[1], np.uint64) for p in pairs])
    order = np.lexsort((v, k))
    ks, vs = k[order], v[order]
    new = np.ones(len(k), bool)
    new[1:] = (ks[1:] != ks[:-1]) | (vs[1:] != vs[:-1])
    code = np.empty(len(k), np.int64)
    code[order] = np.cumsum(new) - 1
    cuts = np.cumsum([len(p[0]) for p in pairs])[:-1]
    return np.split(code, cuts)


def owners_insert_host(keys, vals, links, new_keys, new_vals, nparts: int = 1, part: int = 0):
    """Host mirror of sd_object_index_insert on an owners-mode index: each pair of shard `part`
    adds one link to (k, v), created at 1 if absent; repeated pairs add up; the order of the
    pairs does not matter.  Returns (keys, vals, links, entries created)."""
    keys, vals, links = (np.asarray(a, np.uint64) for a in (keys, vals, links))
    nk = np.ascontiguousarray(new_keys, dtype=np.uint64).reshape(-1)
    nv = np.ascontiguousarray(new_vals, dtype=np.uint64).reshape(-1)
    mine = dest_of(nk, nparts) == part
    nk, nv = nk[mine], nv[mine]
    if len(nk) == 0:
        return keys, vals, links, 0
    ci, cn = _pair_codes((keys, vals), (nk, nv))
    u, first, cnt = np.unique(cn, return_index=True, return_counts=True)
    present = np.isin(u, ci)
    links = links.copy()
    links[np.searchsorted(ci, u[present])] += cnt[present].astype(np.uint64)
    allk = np.concatenate([keys, nk[first[~present]]])
    allv = np.concatenate([vals, nv[first[~present]]])
    alll = np.concatenate([links, cnt[~present].astype(np.uint64)])
    o = np.lexsort((allv, allk))
    return allk[o], allv[o], alll[o], int((~present).sum())


def _owners_drop(keys, vals, links, drop):
    return keys[~drop], vals[~drop], links[~drop], np.stack([keys[drop], vals[drop]], axis=1)


def owners_remove_host(keys, vals, links, rm_keys, rm_ids=None):
    """Host mirror of sd_object_index_remove on an owners-mode index.  With ids each pair takes
    one link from (k, v), pairs naming one entry add up, and an entry asked for at least as
    many links as it has is dropped; without ids every entry of each listed key goes.  Returns
    (keys, vals, links, removed pairs uint64 [r, 2] in ascending (key, id) order)."""
    keys, vals, links = (np.asarray(a, np.uint64) for a in (keys, vals, links))
    rk = np.ascontiguousarray(rm_keys, dtype=np.uint64).reshape(-1)
    if rm_ids is None:
        return _owners_drop(keys, vals, links, np.isin(keys, rk))
    rv = np.ascontiguousarray(rm_ids, dtype=np.uint64).reshape(-1)
    asked = np.zeros(len(keys), np.uint64)
    if len(keys) and len(rk):
        ci, cr = _pair_codes((keys, vals), (rk, rv))
        u, cnt = np.unique(cr, return_counts=True)
        present = np.isin(u, ci)
        asked[np.searchsorted(ci, u[present])] = cnt[present].astype(np.uint64)
    drop = (asked > 0) & (asked >= links)
    return _owners_drop(keys, vals, links - np.where(drop, np.uint64(0), asked), drop)


def owners_remove_objects_host(keys, vals, links, ids):
    """Host mirror of sd_object_index_remove_objects on an owners-mode index: every entry whose
    Object id is listed goes, whatever its links."""
    keys, vals, links = (np.asarray(a, np.uint64) for a in (keys, vals, links))
    return _owners_drop(keys, vals, links, np.isin(vals, np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)))


def owners_apply_host(keys, vals, links, rm_keys, rm_ids, in_keys, in_ids, nparts: int = 1, part: int = 0):
    """Host mirror of sd_object_index_apply on an owners-mode index: for every pair with `held`
    links, named `asked` times in the removal list and `added` times in the insertion list (of
    shard `part`), kept = 0 if held == 0 or 0 < held <= asked else held - asked, and after =
    kept + added.  Returns (keys, vals, links) of the pairs with after > 0, the pairs with held >
    0 and after == 0 as uint64 [r, 2] in ascending (key, id) order, and taken = the number of
    pairs with held == 0 and after > 0."""
    keys, vals, links = (np.asarray(a, np.uint64) for a in (keys, vals, links))
    rk, rv, ik, iv = (np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (rm_keys, rm_ids, in_keys, in_ids))
    mine = dest_of(ik, nparts) == part
    ik, iv = ik[mine], iv[mine]
    ci, cr, cn = _pair_codes((keys, vals), (rk, rv), (ik, iv))
    u = len(keys) + len(rk) + len(ik)  # more than the largest code
    held = np.zeros(u, np.uint64)
    held[ci] = links
    asked = np.bincount(cr, minlength=u).astype(np.uint64)
    added = np.bincount(cn, minlength=u).astype(np.uint64)
    drop = (held == 0) | ((asked != 0) & (asked >= held))
    after = np.where(drop, np.uint64(0), held - np.minimum(asked, held)) + added
    pk, pv = np.zeros(u, np.uint64), np.zeros(u, np.uint64)  # the pair of each code
    for c, k, v in ((ci, keys, vals), (cr, rk, rv), (cn, ik, iv)):
        pk[c], pv[c] = k, v
    stay, gone = after > 0, (held > 0) & (after == 0)
    return (pk[stay], pv[stay], after[stay], np.stack([pk[gone], pv[gone]], axis=1),
            int(((held == 0) & (after > 0)).sum()))


def owners_links_host(keys, vals, links, q_keys, q_ids):
    """Host mirror of sd_object_index_links: the link count per (key, id) pair, 0 if absent."""
    qk = np.ascontiguousarray(q_keys, dtype=np.uint64).reshape(-1)
    qv = np.ascontiguousarray(q_ids, dtype=np.uint64).reshape(-1)
    out = np.zeros(len(qk), np.uint64)
    if len(qk) and len(keys):
        ci, cq = _pair_codes((keys, vals), (qk, qv))
        hit = np.isin(cq, ci)
        out[hit] = np.asarray(links, np.uint64)[np.searchsorted(ci, cq[hit])]
    return out


def owners_object_links_host(vals, links, ids):
    """Host mirror of sd_object_index_object_links on an owners-mode index given by its Object
    ids and link counts: per listed id (any order, repeats allowed) the sum of links[i] over the
    entries with vals[i] == id, in u64, and the number of those entries.  Returns (links,
    entries) uint64 [m]."""
    vals, links = np.asarray(vals, np.uint64), np.asarray(links, np.uint64)
    q = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
    u, inv = np.unique(q, return_inverse=True)
    tl, te = np.zeros(len(u), np.uint64), np.zeros(len(u), np.uint64)
    if len(u) and len(vals):
        at = np.minimum(np.searchsorted(u, vals), len(u) - 1)
        hit = u[at] == vals
        np.add.at(tl, at[hit], links[hit])
        np.add.at(te, at[hit], np.uint64(1))
    return tl[inv.reshape(-1)], te[inv.reshape(-1)]


def owners_orphans_host(vals, ids):
    """Host mirror of sd_object_index_orphans: the distinct listed ids that no entry names,
    ascending (unsigned)."""
    u = np.unique(np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1))
    return u[~np.isin(u, np.asarray(vals, np.uint64))]


def host_u64(a) -> np.ndarray:
    """a uint64 numpy array, or an int64 tensor carrying u64 bit patterns, as uint64 on the host"""
    if isinstance(a, np.ndarray):
        return a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64, copy=False)
    return a.detach().cpu().numpy().view(np.uint64)


def combine_object_links(per_shard):
    """The shards' answers of object_links for one id list -> the library's: per_shard is a list
    of (links, entries) arrays, one per rank; the totals add up."""
    ls = [np.asarray(host_u64(p[0])) for p in per_shard]
    es = [np.asarray(host_u64(p[1])) for p in per_shard]
    return np.sum(ls, axis=0, dtype=np.uint64), np.sum(es, axis=0, dtype=np.uint64)


def combine_orphans(per_shard):
    """The shards' orphan lists for one id list -> the library's: an id is an orphan iff every
    shard lists it.  Ascending (unsigned)."""
    out = None
    for p in per_shard:
        p = np.asarray(host_u64(p))
        out = p if out is None else np.intersect1d(out, p)
    return np.zeros(0, np.uint64) if out is None else np.sort(out)


def owners_groups_host(keys, vals, links):
    """The duplicate groups of an owners-mode index given by its entries in (key, id) order (what
    export_links returns): (group keys ascending, first owner, links(k), owners(k)), uint64 each.
    The group-by a user of export_links runs on the host: np.unique and np.add.reduceat."""
    keys, vals, links = (np.asarray(a, np.uint64).reshape(-1) for a in (keys, vals, links))
    if len(keys) == 0:
        return tuple(np.zeros(0, np.uint64) for _ in range(4))
    gk, head, owners = np.unique(keys, return_index=True, return_counts=True)
    return gk, vals[head], np.add.reduceat(links, head).astype(np.uint64), owners.astype(np.uint64)


def _qualifies(gl, go, min_links, min_owners):
    return (gl >= np.uint64(max(int(min_links), 1))) & (go >= np.uint64(max(int(min_owners), 1)))


def owners_duplicates_host(keys, vals, links, min_links=0, min_owners=0):
    """Host mirror of sd_object_index_duplicates: one row (key, first, links, owners) per key with
    links(k) >= min_links and owners(k) >= min_owners (0 means 1), ascending."""
    gk, gf, gl, go = owners_groups_host(keys, vals, links)
    sel = _qualifies(gl, go, min_links, min_owners)
    return gk[sel], gf[sel], gl[sel], go[sel]


def owners_duplicate_entries_host(keys, vals, links, min_links=0, min_owners=0):
    """Host mirror of sd_object_index_duplicate_entries: the entries (key, id, links) of the
    qualifying keys, in (key, id) order."""
    keys, vals, links = (np.asarray(a, np.uint64).reshape(-1) for a in (keys, vals, links))
    _, _, gl, go = owners_groups_host(keys, vals, links)
    sel = np.repeat(_qualifies(gl, go, min_links, min_owners), go.astype(np.int64))
    return keys[sel], vals[sel], links[sel]


def owners_key_links_host(keys, vals, links, q_keys):
    """Host mirror of sd_object_index_key_links: (links(k), owners(k)) per listed key, 0 and 0 for
    a key without an entry."""
    gk, _, gl, go = owners_groups_host(keys, vals, links)
    q = np.ascontiguousarray(q_keys, dtype=np.uint64).reshape(-1)
    if len(gk) == 0:
        return np.zeros(len(q), np.uint64), np.zeros(len(q), np.uint64)
    at = np.minimum(np.searchsorted(gk, q), len(gk) - 1)
    hit = gk[at] == q
    return np.where(hit, gl[at], np.uint64(0)), np.where(hit, go[at], np.uint64(0))


def owners_duplicate_stats_host(keys, vals, links):
    """Host mirror of sd_object_index_duplicate_stats: uint64 [8] = keys, entries, links, keys
    with links >= 2, their links, keys with owners >= 2, their entries, the largest links(k)."""
    _, _, gl, go = owners_groups_host(keys, vals, links)
    l2, o2 = gl >= np.uint64(2), go >= np.uint64(2)
    return np.array([len(gl), int(go.sum()), int(gl.sum()), int(l2.sum()), int(gl[l2].sum()), int(o2.sum()),
                     int(go[o2].sum()), int(gl.max()) if len(gl) else 0], dtype=np.uint64)


def merge_map(keys, ids):
    """The map for merge_objects from the rows of duplicate_entries(0, 2) (key, Object id; any
    order; the caller may first drop the rows of groups the host did not confirm): Object ids that
    share any key are one component (a host union-find over the distinct ids), and every id but
    the component's smallest (unsigned) maps to that smallest id.  -> (from_ids, to_ids) uint64,
    `from` ascending and distinct; no `to` is a `from`, so the map is chain-free and has no
    contradiction, and a component of one id adds no row."""
    keys = np.ascontiguousarray(host_u64(keys)).reshape(-1)
    ids = np.ascontiguousarray(host_u64(ids)).reshape(-1)
    assert keys.size == ids.size
    u, at = np.unique(ids, return_inverse=True)  # ascending: a smaller slot is a smaller id
    parent = list(range(len(u)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    order = np.argsort(keys, kind="stable")
    sk, sa = keys[order], at.reshape(-1)[order]
    head = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]]) if len(sk) else np.zeros(0, np.int64)
    first = np.repeat(sa[head], np.diff(np.r_[head, len(sk)]))  # the slot of each row's key's first row
    for a, b in zip(sa.tolist(), first.tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)  # the root is the component's smallest slot
    root = np.array([find(a) for a in range(len(u))], dtype=np.int64).reshape(-1)
    moved = root != np.arange(len(u))
    return u[moved], u[root[moved]]


def combine_duplicates(per_shard):
    """The shards' rows of duplicates (or duplicate_entries) -> the library's: per_shard is a list
    of column tuples, one per rank IN RANK ORDER.  sd_dedup_partition's destination is monotone in
    the key, so the shards' groups are disjoint and their rows concatenated are still ascending."""
    cols = list(zip(*[[np.asarray(host_u64(c)) for c in p] for p in per_shard]))
    return tuple(np.concatenate(c) for c in cols)


def combine_duplicate_stats(per_shard):
    """The shards' duplicate_stats -> the library's: the rows add up, [7] takes the maximum."""
    s = np.stack([np.asarray(p, np.uint64) for p in per_shard])
    out = s.sum(axis=0, dtype=np.uint64)
    out[7] = s[:, 7].max()
    return out


def combine_key_links(per_shard):
    """The shards' answers of key_links for one key list -> the library's: a key lives in one
    shard, so the rows add up."""
    return combine_object_links(per_shard)


def owners_indexed_host(records: np.ndarray, rep: np.ndarray, keys: np.ndarray, vals: np.ndarray,
                        chunk_size: int = 100):
    """Host mirror of sd_dedup_owners_indexed on grouped records (int64 [m, 2] sorted by (key,
    index), rep int64 [m]) against an index (keys uint64 ascending, vals uint64):
        owner(i) = index[cas(i)]                       if the index has cas(i)   (existing = 1)
                 = i if chunk(i) == chunk(rep(i)) else rep(i)                    (existing = 0)
    Returns (owner uint64 [m], existing uint8 [m], new heads uint64 [n_new, 2]: (key, file
    index) of each group the index lacks, ascending)."""
    m = len(records)
    if m == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros((0, 2), np.uint64)
    k = np.ascontiguousarray(records[:, 0]).view(np.uint64)
    idx = np.ascontiguousarray(records[:, 1]).view(np.uint64)
    r = np.ascontiguousarray(rep).view(np.uint64)
    keys = np.asarray(keys, np.uint64)
    at = np.searchsorted(keys, k)
    found = np.zeros(m, bool)
    inside = at < len(keys)
    found[inside] = keys[at[inside]] == k[inside]
    c = np.uint64(chunk_size)
    owner = np.where(idx // c == r // c, idx, r)
    owner[found] = np.asarray(vals, np.uint64)[at[found]]
    head = np.ones(m, bool)
    head[1:] = k[1:] != k[:-1]
    head &= ~found
    return owner, found.astype(np.uint8), np.stack([k[head], idx[head]], axis=1)
