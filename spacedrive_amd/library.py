"""One rank's part of a multi-GPU library scan from files on disk: the file identifier
(core/src/object/file_identifier/mod.rs:57-333) over a whole library, one process per GPU.

    bounds = dedup.shard_plan(sizes, R)                  # contiguous, cost-balanced shards
    rank r: sd_cas_hashes_files(its files)               # cas_id messages read as cas.rs does,
                                                         # hashed into device rows
            sd_cas_dedup_mgpu(rows, comm)                # cas_id-prefix all-to-all over RCCL,
                                                         # grouping, chunk-of-100 Object rule
Every rank returns its shard's cas_ids (status per file as generate_cas_id's Result) and
the groups / Object owners of the cas_id prefix range it owns.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import dedup
from .cas import _status_error
from ._native import SD_FILE_OK


def confirm_duplicates(ctx, paths: Sequence[str], cas_ids: Sequence[str], nthreads: int = 16) -> dict:
    """The file route of the confirm step: the members of duplicate groups (`paths` with their
    16-hex `cas_ids`, e.g. the duplicate entries joined with the DB) hashed in full
    (file_checksum, validation/hash.rs:10-24) and split into classes of equal checksums
    (sd_cpu_dedup_confirm: the checksums arrive on the host, so no device is needed for this
    half).  `ctx` None hashes on the CPU path, else through sd_file_checksums on ctx's device.
    A file whose checksum fails is invalid.  Returns {"verdict": uint8 [n] (SD_CONFIRM_*),
    "rep": uint64 [n] (an index into `paths`; UINT64_MAX when invalid), "class_size": uint64
    [n], "checksums": [str | OSError], "sets": [(cas_id, [path indices])] confirmed, ascending by
    (cas_id, checksum), "stats": uint64 [8]}."""
    from . import cas, cpu
    n = len(paths)
    if n != len(cas_ids):
        raise ValueError("paths and cas_ids differ in length")
    sums = cpu.file_checksums(paths, nthreads) if ctx is None else cas.file_checksums(paths, ctx.device)
    valid = np.array([isinstance(s, str) for s in sums], dtype=np.uint8)
    keys = np.array([int(c, 16) for c in cas_ids], dtype=np.uint64)
    h = np.zeros((n, 32), np.uint8)
    for i, s in enumerate(sums):
        if valid[i]:
            h[i] = np.frombuffer(bytes.fromhex(s), np.uint8)
    rep, size, verdict, sets, stats = cpu.confirm(keys, h, valid)
    members = {}
    for i in np.flatnonzero(verdict == 2):
        members.setdefault(int(rep[i]), []).append(int(i))
    return {"verdict": verdict, "rep": rep, "class_size": size, "checksums": sums,
            "sets": [(cas_ids[int(r)], members[int(r)]) for _, r, _ in sets], "stats": stats}


def scan_library(ctx, paths: Sequence[str], sizes, comm=None, group: Optional[dist.ProcessGroup] = None,
                 chunk_size: int = 100, nthreads: int = 16, index=None, object_id_of=None) -> dict:
    """This rank's share of the scan of the whole library (`paths`, `sizes` as the walker's
    metadata reported them; the same lists on every rank).  With `comm` (libsdcas's RCCL
    communicator, dedup.make_comm) the exchange runs inside the library; without it, over
    torch.distributed.  Returns {"shard": (lo, hi), "cas_ids": [str | OSError] for files
    lo..hi-1, "records": int64 [m, 2] (cas_id key, global index) sorted, "rep": [m],
    "owner": [m], "n_groups": int}.  With `index` (a device.ObjectIndex of the Objects the
    library already has, sharded as this rank's prefix range) owners of known cas_ids are those Objects' ids, and the result gains "existing"
    (uint8 [m]) and "new_heads" (int64 [n_new, 2]: key, creating file) to insert once the
    host has given the new Objects their ids.  With an owners-mode index (ObjectIndex(...,
    owners=True)) and `object_id_of` (int64 tensor of creating file indices -> int64 tensor of
    the ids the host gave their Objects) the scan also inserts every record's (key, Object id)
    pair, and the result gains "object_ids" (int64 [m]) and "inserted" (entries created)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    bounds = dedup.shard_plan(sizes, world)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])
    n = hi - lo
    dev = torch.device("cuda", torch.cuda.current_device())
    d_hash = torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev)
    d_valid = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    status = ctx.hashes_files(list(paths[lo:hi]), sizes[lo:hi], d_hash, d_valid, nthreads=nthreads)
    extra = {}
    if index is not None:
        if comm is not None:
            runner = dedup.RcclDedup(ctx, comm, dev, capacity=n * 5 // 4 + 4096)
            recs, rep, ng, owner, existing, new = runner(d_hash, d_valid, n, lo, chunk_size=chunk_size, index=index)
        else:
            recs, rep, ng, owner, existing, new = dedup.dedup_shard(ctx, d_hash, d_valid, n, lo, group, index=index)
        extra = {"existing": existing, "new_heads": new}
        if getattr(index, "owners_mode", False) and object_id_of is not None:
            # owners mode: ONE insert of (key, Object id) for every record, linked and created
            # alike -- a linked record's owner is an Object id already, a created one's is the
            # file whose Object the host has just made.  The host's mapping sees the created
            # records only: a linked owner is an arbitrary u64, not a file index
            created = ~existing.bool()
            object_ids = owner.clone()
            object_ids[created] = object_id_of(owner[created])
            extra["object_ids"] = object_ids
            extra["inserted"] = index.insert(recs[:, 0].contiguous(), object_ids.contiguous())
    elif comm is not None:
        runner = dedup.RcclDedup(ctx, comm, dev, capacity=n * 5 // 4 + 4096)
        recs, rep, ng, owner = runner(d_hash, d_valid, n, lo, chunk_size=chunk_size)
    else:
        recs, rep, ng, owner = dedup.dedup_shard(ctx, d_hash, d_valid, n, lo, group)
    h = d_hash[:n].cpu().numpy()
    ids = [h[i, :8].tobytes().hex() if status[i] == SD_FILE_OK else _status_error(int(status[i]), str(paths[lo + i]))
           for i in range(n)]
    return {"shard": (lo, hi), "cas_ids": ids, "records": recs, "rep": rep, "owner": owner, "n_groups": ng, **extra}
