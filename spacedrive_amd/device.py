"""Device-level interface over libsdcas.so: contexts, prepared batches, device buffers.

Device memory and streams are torch tensors / torch streams (plumbing only); every byte
of hashing runs in the gfx950 kernels of ``csrc/cas_kernels.hip``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from ._native import SD_ERR_CAPACITY, SD_OBJECT_INDEX_OWNERS, Extent, SdCasError, check, lib

EXTENT_DTYPE = np.dtype([("size", "<u8"), ("msg_offset", "<u8"), ("msg_len", "<u4"), ("kind", "<u4")])
assert EXTENT_DTYPE.itemsize == ctypes.sizeof(Extent) == 24


def _ptr(x) -> Optional[int]:
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return int(x)


def _stream(stream) -> Optional[int]:
    """The HIP stream handle a wrapper passes to the C ABI.  A stream other than the
    current one is first ordered after the work queued so far on the current stream (an
    event recorded there, waited on by `stream`): the inputs a caller just produced --
    torch fills, copies, kernels on the current stream -- are complete before the
    library's kernels read them, with no manual wait_stream.  The reverse order (the
    outputs, consumed back on the current stream) stays the caller's, as in torch."""
    cur = torch.cuda.current_stream()
    if stream is None:
        return cur.cuda_stream
    s = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream))
    if s.cuda_stream != cur.cuda_stream:
        s.wait_stream(cur)
    return s.cuda_stream


def stage_plan(sizes) -> tuple:
    """cas.rs:25-58 message layout for files of these sizes -> (extents, staged_bytes)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    ext = np.zeros(len(sizes), dtype=EXTENT_DTYPE)
    total = ctypes.c_uint64(0)
    check(lib().sd_cas_stage_plan(_ptr(sizes), len(sizes), _ptr(ext), ctypes.byref(total)))
    return ext, int(total.value)


class Context:
    """One per device and process; thread-safe (sd_cas_ctx)."""

    def __init__(self, device: Optional[int] = None):
        if device is None:
            device = torch.cuda.current_device()
        self.device = device
        h = ctypes.c_void_p()
        check(lib().sd_cas_ctx_create(device, ctypes.byref(h)))
        self.handle = h

    def close(self) -> None:
        if self.handle:
            lib().sd_cas_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- batches
    def cas_batch(self, extents: np.ndarray) -> "CasBatch":
        return CasBatch(self, extents)

    def checksum_batch(self, offsets, lens) -> "ChecksumBatch":
        return ChecksumBatch(self, offsets, lens)

    def fingerprint_batch(self, offsets, lens) -> "FingerprintBatch":
        return FingerprintBatch(self, offsets, lens)

    def checksum_tree(self, offsets, lens, block_log2: int = 17) -> "ChecksumTree":
        return ChecksumTree(self, offsets, lens, block_log2)

    def checksum_tree_blocks(self, lens, rows, data_offsets, block_log2: int = 17) -> "ChecksumTreeBlocks":
        return ChecksumTreeBlocks(self, lens, rows, data_offsets, block_log2)

    # -------------------------------------------------------------- files -> device hashes
    def hashes_files(self, paths, sizes, d_hash32, d_valid=None, nthreads: int = 16) -> np.ndarray:
        """sd_cas_hashes_files: generate_cas_id's messages of these files hashed into
        d_hash32 (device, n x 32 B; the cas_id is each row's first 8 bytes) and, if given,
        d_valid (device, n B: hashed and not empty).  Returns the int32 status per file."""
        from ._native import path_array
        n = len(paths)
        status = np.zeros(max(n, 1), np.int32)
        keep, arr = path_array(paths)
        sz = np.ascontiguousarray(sizes, dtype=np.uint64)
        assert d_hash32.numel() >= 32 * n and (d_valid is None or d_valid.numel() >= n)
        # the library writes the rows from its own streams: whatever the caller queued on
        # the current stream (e.g. the buffers' zero fills) must be done first
        torch.cuda.current_stream().synchronize()
        check(lib().sd_cas_hashes_files(self.handle, arr, _ptr(sz), n, _ptr(d_hash32),
                                        None if d_valid is None else _ptr(d_valid), _ptr(status), nthreads))
        return status[:n]

    # -------------------------------------------------------------- synthetic data
    def synth_stage_cas(self, d_sizes, d_cids, d_twins, d_extents, n, d_staged, stream=None) -> None:
        check(lib().sd_synth_stage_cas(self.handle, _ptr(d_sizes), _ptr(d_cids), _ptr(d_twins),
                                       _ptr(d_extents), n, _ptr(d_staged), _stream(stream)))

    def synth_fill(self, cid: int, twin: int, length: int, d_out, stream=None, offset: int = 0) -> None:
        """bytes [offset, offset + length) of synthetic content (cid, twin) -> d_out"""
        check(lib().sd_synth_fill_at(self.handle, cid, twin, offset, length, _ptr(d_out), _stream(stream)))

    def valu_peak(self) -> float:
        v = ctypes.c_double(0)
        check(lib().sd_valu_peak(self.handle, ctypes.byref(v)))
        return float(v.value)

    # -------------------------------------------------------------- dedup
    def dedup_partition(self, d_hash32, d_valid, n: int, base: int, nparts: int, d_counts, d_records,
                        stream=None) -> int:
        nv = ctypes.c_uint64(0)
        check(lib().sd_dedup_partition(self.handle, _ptr(d_hash32), _ptr(d_valid), n, base, nparts,
                                       _ptr(d_counts), _ptr(d_records), ctypes.byref(nv), _stream(stream)))
        return int(nv.value)

    def dedup_group(self, d_records, m: int, d_rep, stream=None, index_sorted: bool = False) -> int:
        ng = ctypes.c_uint64(0)
        check(lib().sd_dedup_group(self.handle, _ptr(d_records), m, 1 if index_sorted else 0, _ptr(d_rep),
                                   ctypes.byref(ng), _stream(stream)))
        return int(ng.value)

    def dedup_owners(self, d_records, m: int, d_rep, d_owner, chunk_size: int = 100, stream=None) -> None:
        check(lib().sd_dedup_owners(self.handle, _ptr(d_records), m, _ptr(d_rep), chunk_size, _ptr(d_owner),
                                    _stream(stream)))

    def dedup_confirm(self, d_keys, d_hash32, d_valid, m: int, d_rep=None, d_class_size=None, d_verdict=None,
                      d_sets_out=None, capacity: int = 0, stream=None):
        """sd_dedup_confirm: the candidate groups of m files (cas keys int64 [m], checksums uint8
        [m, 32], d_valid uint8 [m] or None) split into classes of equal checksums.  Writes the
        outputs given (rep, class_size int64 [m]; verdict uint8 [m]; sets int64 [capacity, 3]) and
        returns (n_sets, stats uint64 [8]); a short `capacity` raises SdCasError (SD_ERR_CAPACITY,
        ``.needed`` rows, ``.stats``) with the per-file outputs complete and no set row written."""
        n_sets = ctypes.c_uint64(0)
        stats = np.zeros(8, np.uint64)
        rc = lib().sd_dedup_confirm(self.handle, _ptr(d_keys) if m else None, _ptr(d_hash32) if m else None,
                                    _ptr(d_valid), m, _ptr(d_rep), _ptr(d_class_size), _ptr(d_verdict),
                                    _ptr(d_sets_out), capacity, ctypes.byref(n_sets), _ptr(stats), _stream(stream))
        try:
            check(rc)
        except SdCasError as e:
            e.needed = int(n_sets.value)
            e.stats = stats
            raise
        return int(n_sets.value), stats

    def dedup_confirm_stats(self) -> dict:
        """sd_dedup_confirm_stats: the calls that finished on the prefix path and those that took
        the full-width path, since the context was created."""
        v = np.zeros(2, np.uint64)
        check(lib().sd_dedup_confirm_stats(self.handle, _ptr(v)))
        return {"prefix": int(v[0]), "full": int(v[1])}

    def checksum_tree_shared(self, lens, d_nodes, block_log2: int = 17, min_blocks: int = 0, d_rep=None,
                             d_class_size=None, d_files_out=None, d_pairs_out=None, capacity: int = 0, stream=None):
        """sd_checksum_tree_shared: which blocks of a batch of levels (lens: host uint64 [n]; d_nodes
        uint8 [node_base[n], 32] on the device, the layout ChecksumTree.run leaves) are there more
        than once.  Writes the outputs given (rep, class_size int64 [m]; files int64 [n, 4]; pairs
        int64 [capacity, 4]) and returns (n_pairs, stats uint64 [8]); a short `capacity` raises
        SdCasError (SD_ERR_CAPACITY, ``.needed`` rows, ``.stats``) with every other output complete
        and no pair row written."""
        ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
        n = len(ls)
        n_pairs = ctypes.c_uint64(0)
        stats = np.zeros(8, np.uint64)
        rc = lib().sd_checksum_tree_shared(self.handle, _ptr(ls) if n else None, n, int(block_log2),
                                           _ptr(d_nodes) if n else None, int(min_blocks), _ptr(d_rep),
                                           _ptr(d_class_size), _ptr(d_files_out), _ptr(d_pairs_out), capacity,
                                           ctypes.byref(n_pairs), _ptr(stats), _stream(stream))
        try:
            check(rc)
        except SdCasError as e:
            e.needed = int(n_pairs.value)
            e.stats = stats
            raise
        return int(n_pairs.value), stats

    def dedup_mgpu(self, comm: "Comm", d_hash32, d_valid, n: int, base: int, d_records, d_rep, d_owner,
                   capacity: int, chunk_size: int = 100, stream=None):
        """sd_cas_dedup_mgpu: partition -> RCCL all-to-all -> group -> owners on this rank.
        Returns (m, n_groups); raises SdCasError (SD_ERR_CAPACITY) on every rank when some
        rank's capacity is short -- then ``.needed`` is this rank's requirement."""
        m = ctypes.c_uint64(0)
        ng = ctypes.c_uint64(0)
        rc = lib().sd_cas_dedup_mgpu(self.handle, comm.handle, _ptr(d_hash32), _ptr(d_valid), n, base, chunk_size,
                                     _ptr(d_records), _ptr(d_rep), _ptr(d_owner), capacity, ctypes.byref(m),
                                     ctypes.byref(ng), _stream(stream))
        try:
            check(rc)
        except SdCasError as e:
            e.needed = int(m.value)
            raise
        return int(m.value), int(ng.value)

    def dedup_mgpu_indexed(self, comm: "Comm", d_hash32, d_valid, n: int, base: int, d_records, d_rep, d_owner,
                           capacity: int, index: "ObjectIndex", d_existing, d_new, chunk_size: int = 100, stream=None):
        """sd_cas_dedup_mgpu_indexed: dedup_mgpu with the owners taken through this rank's shard
        of the Object index.  Returns (m, n_groups, n_new); a wrongly sharded index on any rank
        raises SdCasError (SD_ERR_INVALID) on every rank."""
        m = ctypes.c_uint64(0)
        ng = ctypes.c_uint64(0)
        nn = ctypes.c_uint64(0)
        rc = lib().sd_cas_dedup_mgpu_indexed(self.handle, comm.handle, _ptr(d_hash32), _ptr(d_valid), n, base,
                                             chunk_size, _ptr(d_records), _ptr(d_rep), _ptr(d_owner), capacity,
                                             ctypes.byref(m), ctypes.byref(ng), _stream(stream),
                                             None if index is None else index.handle, _ptr(d_existing), _ptr(d_new),
                                             ctypes.byref(nn))
        try:
            check(rc)
        except SdCasError as e:
            e.needed = int(m.value)
            raise
        return int(m.value), int(ng.value), int(nn.value)


class ObjectIndex:
    """The device-resident Object index (sd_object_index): cas_id key -> the Object of the
    library that already owns it (file_identifier/mod.rs:168-225).  Keys are carried in int64
    tensors (the bit pattern of the u64); Object ids likewise.  Insert is keep-first; insert
    and the removals are exclusive; lookups may run concurrently (include/sd_cas.h).

    ``owners=True`` (SD_OBJECT_INDEX_OWNERS) keeps one entry per (cas_id, Object) pair with
    the number of file_paths that link them: insert adds a link per pair, remove with ids
    takes one, an entry leaves at zero, and the first owner of a key is its smallest Object
    id -- the host never asks the DB who else owns a cas_id.  Its view by Object
    (``object_links``, ``orphans``; ``apply(..., orphans=True)``) answers the orphan remover's
    query too: which of these Objects own nothing any more (orphan_remover.rs:57-95).  Its view
    by key (``key_links``, ``duplicates``, ``duplicate_entries``, ``duplicate_stats``) lists the
    cas_ids that several file_paths have or that are split over several Objects, and
    ``merge_objects`` acts on it: "Object B is Object A" in one call (both modes)."""

    def __init__(self, ctx: Context, nparts: int = 1, part: int = 0, owners: bool = False):
        self.ctx, self.nparts, self.part, self.owners_mode = ctx, nparts, part, bool(owners)
        h = ctypes.c_void_p()
        if owners:
            check(lib().sd_object_index_create_ex(ctx.handle, nparts, part, SD_OBJECT_INDEX_OWNERS, ctypes.byref(h)))
        else:
            check(lib().sd_object_index_create(ctx.handle, nparts, part, ctypes.byref(h)))
        self.handle = h

    @property
    def flags(self) -> int:
        f = ctypes.c_int(0)
        check(lib().sd_object_index_flags(self.handle, ctypes.byref(f)))
        return int(f.value)

    def links(self, d_keys: torch.Tensor, d_object_ids: torch.Tensor, stream=None) -> torch.Tensor:
        """-> int64 [m]: the link count of each (key, Object id) pair, 0 if absent (owners mode)."""
        m = int(d_keys.numel())
        assert d_object_ids.numel() == m and d_keys.dtype == d_object_ids.dtype == torch.int64
        out = torch.empty(max(m, 1), dtype=torch.int64, device=torch.device("cuda", self.ctx.device))
        check(lib().sd_object_index_links(self.ctx.handle, self.handle, _ptr(d_keys) if m else None,
                                          _ptr(d_object_ids) if m else None, m, _ptr(out), _stream(stream)))
        return out[:m]

    def export_links(self, stream=None):
        """-> (keys, Object ids, links) int64 [n] in ascending (key, id) order (owners mode)."""
        n = len(self)
        dev = torch.device("cuda", self.ctx.device)
        k, v, c = (torch.empty(max(n, 1), dtype=torch.int64, device=dev) for _ in range(3))
        check(lib().sd_object_index_export_links(self.ctx.handle, self.handle, _ptr(k), _ptr(v), _ptr(c), max(n, 1),
                                                 _stream(stream)))
        return k[:n], v[:n], c[:n]

    def __len__(self) -> int:
        n = ctypes.c_uint64(0)
        check(lib().sd_object_index_count(self.handle, ctypes.byref(n)))
        return int(n.value)

    def insert(self, d_keys: torch.Tensor, d_object_ids: torch.Tensor, stream=None) -> int:
        """(key, Object id) pairs in DB order; returns how many entries were added."""
        m = int(d_keys.numel())
        assert d_object_ids.numel() == m and d_keys.dtype == d_object_ids.dtype == torch.int64
        assert m == 0 or (d_keys.is_cuda and d_object_ids.is_cuda and d_keys.is_contiguous()
                          and d_object_ids.is_contiguous())
        taken = ctypes.c_uint64(0)
        check(lib().sd_object_index_insert(self.ctx.handle, self.handle, _ptr(d_keys) if m else None,
                                           _ptr(d_object_ids) if m else None, m, ctypes.byref(taken), _stream(stream)))
        return int(taken.value)

    def insert_hex(self, cas_ids, object_ids) -> int:
        """The same from the DB's strings: 16-hex-digit cas_ids and their Object ids."""
        m = len(cas_ids)
        buf = b"".join(c.encode("ascii") + b"\0" for c in cas_ids)
        if len(buf) != 17 * m:
            raise ValueError("a cas_id is not 16 characters")
        ids = np.ascontiguousarray(object_ids, dtype=np.uint64)
        assert ids.size == m
        taken = ctypes.c_uint64(0)
        torch.cuda.current_stream().synchronize()
        check(lib().sd_object_index_insert_hex(self.ctx.handle, self.handle, buf if m else None,
                                               _ptr(ids) if m else None, m, ctypes.byref(taken)))
        return int(taken.value)

    # -------------------------------------------------------------- removal
    def _removal(self, call, bound: int, d_removed_out, capacity):
        """Run call(out pointer, capacity, removed) -> rc.  Without a caller's buffer the
        dropped pairs go to one of `bound` rows at most, regrown once to the requirement the
        library reports (SD_ERR_CAPACITY leaves the index unchanged)."""
        removed = ctypes.c_uint64(0)
        own = d_removed_out is None
        cap = max(int(bound), 1) if own else int(d_removed_out.numel() // 2 if capacity is None else capacity)
        for _ in range(2):
            if own:
                d_removed_out = torch.empty((cap, 2), dtype=torch.int64, device=torch.device("cuda", self.ctx.device))
            rc = call(_ptr(d_removed_out), cap, ctypes.byref(removed))
            if rc == SD_ERR_CAPACITY and own:
                cap = int(removed.value)
                continue
            try:
                check(rc)
            except SdCasError as e:
                e.needed = int(removed.value)
                raise
            r = int(removed.value)
            return d_removed_out.view(-1, 2)[:r], r
        raise RuntimeError("sd_object_index_remove: capacity still short after regrowing")

    def remove(self, d_keys: torch.Tensor, d_object_ids: Optional[torch.Tensor] = None, stream=None,
               d_removed_out: Optional[torch.Tensor] = None, capacity: Optional[int] = None, orphans: bool = False):
        """Drop entry (k, v) iff some pair i has d_keys[i] == k and (d_object_ids is None or
        d_object_ids[i] == v).  -> (removed pairs int64 [r, 2] = (key, Object id) in ascending
        key order, r).  With d_removed_out (int64, `capacity` rows of 2) too small the call
        raises SdCasError (SD_ERR_CAPACITY, ``.needed`` rows) and the index is unchanged.
        ``orphans=True`` (owners mode) appends the Objects of the removed pairs that now own
        nothing in this index (_orphans_of)."""
        m = int(d_keys.numel())
        assert d_keys.dtype == torch.int64 and (m == 0 or (d_keys.is_cuda and d_keys.is_contiguous()))
        if d_object_ids is not None:
            assert d_object_ids.numel() == m and d_object_ids.dtype == torch.int64
            assert m == 0 or (d_object_ids.is_cuda and d_object_ids.is_contiguous())
        st = _stream(stream)
        res = self._removal(lambda out, cap, removed: lib().sd_object_index_remove(
            self.ctx.handle, self.handle, _ptr(d_keys) if m else None,
            _ptr(d_object_ids) if m and d_object_ids is not None else None, m, out, cap, removed, st),
            # owners mode without ids: a key drops all its owners, so the bound is the entries
            # (HostObjectIndex.remove sizes its rows the same way)
            len(self) if self.owners_mode and d_object_ids is None else min(m, len(self)), d_removed_out, capacity)
        return res + (self._orphans_of(res[0], stream),) if orphans else res

    def remove_objects(self, d_object_ids: torch.Tensor, stream=None, d_removed_out: Optional[torch.Tensor] = None,
                       capacity: Optional[int] = None, orphans: bool = False):
        """Drop every entry whose Object id is among d_object_ids (orphan_remover.rs:57-95).
        -> (removed pairs int64 [r, 2], r), as remove; ``orphans`` as remove."""
        m = int(d_object_ids.numel())
        assert d_object_ids.dtype == torch.int64 and (m == 0 or (d_object_ids.is_cuda and d_object_ids.is_contiguous()))
        st = _stream(stream)
        res = self._removal(lambda out, cap, removed: lib().sd_object_index_remove_objects(
            self.ctx.handle, self.handle, _ptr(d_object_ids) if m else None, m, out, cap, removed, st),
            min(len(self), max(4 * m, 1024)) if m else 0, d_removed_out, capacity)
        return res + (self._orphans_of(res[0], stream),) if orphans else res

    def remove_hex(self, cas_ids, object_ids=None) -> int:
        """remove from the DB's strings (object_ids None: unconditional); returns the count."""
        m = len(cas_ids)
        buf = b"".join(c.encode("ascii") + b"\0" for c in cas_ids)
        if len(buf) != 17 * m:
            raise ValueError("a cas_id is not 16 characters")
        ids = None if object_ids is None else np.ascontiguousarray(object_ids, dtype=np.uint64)
        assert ids is None or ids.size == m
        removed = ctypes.c_uint64(0)
        torch.cuda.current_stream().synchronize()
        check(lib().sd_object_index_remove_hex(self.ctx.handle, self.handle, buf if m else None,
                                               _ptr(ids) if m and ids is not None else None, m, ctypes.byref(removed)))
        return int(removed.value)

    # -------------------------------------------------------------- apply (owners mode)
    def apply(self, d_rm_keys: torch.Tensor, d_rm_ids: torch.Tensor, d_in_keys: torch.Tensor, d_in_ids: torch.Tensor,
              stream=None, d_removed_out: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
              orphans: bool = False):
        """sd_object_index_apply: the links of the removal list go, then those of the insertion
        list come, in one call and one rewrite of the index (owners mode).  -> (removed, taken):
        the pairs int64 [r, 2] present before and absent after, in ascending (key, id) order, and
        the number of pairs absent before and present after.  d_removed_out / capacity as remove.
        ``orphans=True`` appends the Objects of the removed pairs that now own nothing in this
        index (_orphans_of): the orphan remover's candidates, found without a DB scan."""
        m_rm, m_in = int(d_rm_keys.numel()), int(d_in_keys.numel())
        for t, m in ((d_rm_keys, m_rm), (d_rm_ids, m_rm), (d_in_keys, m_in), (d_in_ids, m_in)):
            assert t.numel() == m and t.dtype == torch.int64 and (m == 0 or (t.is_cuda and t.is_contiguous()))
        st = _stream(stream)
        taken = ctypes.c_uint64(0)
        pairs, _ = self._removal(lambda out, cap, removed: lib().sd_object_index_apply(
            self.ctx.handle, self.handle, _ptr(d_rm_keys) if m_rm else None, _ptr(d_rm_ids) if m_rm else None, m_rm,
            _ptr(d_in_keys) if m_in else None, _ptr(d_in_ids) if m_in else None, m_in, out, cap, removed,
            ctypes.byref(taken), st), min(m_rm, len(self)), d_removed_out, capacity)
        if orphans:
            return pairs, int(taken.value), self._orphans_of(pairs, stream)
        return pairs, int(taken.value)

    # -------------------------------------------------------------- the view by Object (owners mode)
    def object_links(self, d_object_ids: torch.Tensor, stream=None, stride: int = 1, m: Optional[int] = None):
        """sd_object_index_object_links -> (links, entries) int64 [m]: per listed Object id (any
        order, repeats allowed) the sum of its entries' link counts and the number of its
        entries in this index.  ``stride`` (1 or 2, in elements): the id of element j is
        d_object_ids[j * stride], so the id column of (key, id) rows is rows.reshape(-1)[1:]
        with stride 2 and m = the rows."""
        m = (int(d_object_ids.numel()) + stride - 1) // max(stride, 1) if m is None else int(m)
        assert d_object_ids.dtype == torch.int64 and (m == 0 or (d_object_ids.is_cuda and d_object_ids.is_contiguous()))
        assert m == 0 or stride not in (1, 2) or (m - 1) * stride < d_object_ids.numel()
        dev = torch.device("cuda", self.ctx.device)
        links, entries = (torch.empty(max(m, 1), dtype=torch.int64, device=dev) for _ in range(2))
        check(lib().sd_object_index_object_links(self.ctx.handle, self.handle, _ptr(d_object_ids) if m else None, stride,
                                                 m, _ptr(links), _ptr(entries), _stream(stream)))
        return links[:m], entries[:m]

    def orphans(self, d_object_ids: torch.Tensor, stream=None, stride: int = 1, m: Optional[int] = None,
                d_orphans_out: Optional[torch.Tensor] = None, capacity: Optional[int] = None) -> torch.Tensor:
        """sd_object_index_orphans -> int64 [count]: the distinct listed Object ids that have no
        entry in this index, ascending as u64 (orphan_remover.rs:57-95 without the DB scan).
        ``stride`` / ``m`` as object_links.  With d_orphans_out (int64, `capacity` elements)
        too small the call raises SdCasError (SD_ERR_CAPACITY, ``.needed``) and writes nothing."""
        m = (int(d_object_ids.numel()) + stride - 1) // max(stride, 1) if m is None else int(m)
        assert d_object_ids.dtype == torch.int64 and (m == 0 or (d_object_ids.is_cuda and d_object_ids.is_contiguous()))
        assert m == 0 or stride not in (1, 2) or (m - 1) * stride < d_object_ids.numel()
        if d_orphans_out is None:  # the distinct ids are m at most: never short
            d_orphans_out = torch.empty(max(m, 1), dtype=torch.int64, device=torch.device("cuda", self.ctx.device))
            capacity = max(m, 1)
        cap = int(d_orphans_out.numel() if capacity is None else capacity)
        count = ctypes.c_uint64(0)
        try:
            check(lib().sd_object_index_orphans(self.ctx.handle, self.handle, _ptr(d_object_ids) if m else None, stride,
                                                m, _ptr(d_orphans_out), cap, ctypes.byref(count), _stream(stream)))
        except SdCasError as e:
            e.needed = int(count.value)
            raise
        return d_orphans_out[:int(count.value)]

    def _orphans_of(self, pairs: torch.Tensor, stream=None) -> torch.Tensor:
        """The orphans among the Objects of removed (key, id) rows: their id column read at
        stride 2 on the device."""
        r = int(pairs.shape[0])
        return self.orphans(pairs.reshape(-1)[1:] if r else pairs.reshape(-1), stream, stride=2, m=r)

    # -------------------------------------------------------------- the view by key (owners mode)
    def key_links(self, d_keys: torch.Tensor, stream=None):
        """sd_object_index_key_links -> (links, owners) int64 [m]: per listed key (any order,
        repeats allowed) the sum of its entries' link counts and the number of its entries
        (Objects) in this index; 0 and 0 for a key it does not hold."""
        m = int(d_keys.numel())
        assert d_keys.dtype == torch.int64 and (m == 0 or (d_keys.is_cuda and d_keys.is_contiguous()))
        dev = torch.device("cuda", self.ctx.device)
        links, owners = (torch.empty(max(m, 1), dtype=torch.int64, device=dev) for _ in range(2))
        check(lib().sd_object_index_key_links(self.ctx.handle, self.handle, _ptr(d_keys) if m else None, m,
                                              _ptr(links), _ptr(owners), _stream(stream)))
        return links[:m], owners[:m]

    def _group_rows(self, fn, ncols: int, min_links: int, min_owners: int, stream, out, capacity):
        """The capacity convention of the two group calls: without `out` the rows are counted
        first (every output NULL) and then written into tensors of exactly that many rows; with
        `out` (ncols int64 tensors, None for a column not wanted) and `capacity` short, the call
        raises SdCasError (SD_ERR_CAPACITY, ``.needed`` rows) and writes nothing."""
        st = _stream(stream)
        count = ctypes.c_uint64(0)
        if out is None:
            check(fn(self.ctx.handle, self.handle, min_links, min_owners, *([None] * ncols), 0, ctypes.byref(count), st))
            capacity = int(count.value)
            dev = torch.device("cuda", self.ctx.device)
            out = tuple(torch.empty(max(capacity, 1), dtype=torch.int64, device=dev) for _ in range(ncols))
        assert len(out) == ncols and all(t is None or (t.dtype == torch.int64 and t.is_cuda and t.is_contiguous()) for t in out)
        cap = int(min(t.numel() for t in out if t is not None) if capacity is None else capacity)
        try:
            check(fn(self.ctx.handle, self.handle, min_links, min_owners, *(None if t is None else _ptr(t) for t in out),
                     cap, ctypes.byref(count), st))
        except SdCasError as e:
            e.needed = int(count.value)
            raise
        return tuple(None if t is None else t[:int(count.value)] for t in out)

    def duplicates(self, min_links: int = 0, min_owners: int = 0, stream=None, out=None, capacity: Optional[int] = None):
        """sd_object_index_duplicates -> (keys, first, links, owners) int64 [count]: one row per key
        with links(k) >= min_links and owners(k) >= min_owners (0 means 1), ascending as u64.
        min_links=2: content more than one file_path has; min_owners=2: content split over
        several Objects.  `out` / `capacity` as _group_rows."""
        return self._group_rows(lib().sd_object_index_duplicates, 4, min_links, min_owners, stream, out, capacity)

    def duplicate_entries(self, min_links: int = 0, min_owners: int = 0, stream=None, out=None,
                          capacity: Optional[int] = None):
        """sd_object_index_duplicate_entries -> (keys, ids, links) int64 [count]: the entries of the
        qualifying keys in (key, id) order -- export_links filtered to the duplicate groups."""
        return self._group_rows(lib().sd_object_index_duplicate_entries, 3, min_links, min_owners, stream, out, capacity)

    def duplicate_stats(self, stream=None) -> np.ndarray:
        """sd_object_index_duplicate_stats -> uint64 [8]: keys, entries, links, keys with links >= 2,
        their links, keys with owners >= 2, their entries, the largest links(k)."""
        out = np.zeros(8, np.uint64)
        check(lib().sd_object_index_duplicate_stats(self.ctx.handle, self.handle, _ptr(out), _stream(stream)))
        return out

    # -------------------------------------------------------------- merge Objects
    def merge_objects(self, d_from: torch.Tensor, d_to: torch.Tensor, stream=None):
        """sd_object_index_merge_objects: Object d_from[j] IS Object d_to[j] (mod.rs:229-333 gave
        same-step duplicates an Object each).  Every id is relabelled once and simultaneously
        (chains are the caller's to resolve: dedup.merge_map returns a chain-free map); in the
        owners mode the entries of one key that now share an id coalesce and their links add up,
        in one rewrite of the index.  -> (moved, coalesced): the entries whose id changed and the
        drop in the count.  One `from` with two `to` raises SdCasError and changes nothing.
        ``orphans(d_from)`` afterwards lists the Objects that no longer own anything."""
        m = int(d_from.numel())
        for t in (d_from, d_to):
            assert t.numel() == m and t.dtype == torch.int64 and (m == 0 or (t.is_cuda and t.is_contiguous()))
        moved, coalesced = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().sd_object_index_merge_objects(self.ctx.handle, self.handle, _ptr(d_from) if m else None,
                                                  _ptr(d_to) if m else None, m, ctypes.byref(moved),
                                                  ctypes.byref(coalesced), _stream(stream)))
        return int(moved.value), int(coalesced.value)

    def apply_hex(self, rm_cas_ids, rm_object_ids, in_cas_ids, in_object_ids):
        """apply from the DB's strings -> (entries removed, entries taken)."""
        bufs, ids = [], []
        for cas, oid in ((rm_cas_ids, rm_object_ids), (in_cas_ids, in_object_ids)):
            buf = b"".join(c.encode("ascii") + b"\0" for c in cas)
            if len(buf) != 17 * len(cas):
                raise ValueError("a cas_id is not 16 characters")
            a = np.ascontiguousarray(oid, dtype=np.uint64)
            assert a.size == len(cas)
            bufs.append(buf), ids.append(a)
        m_rm, m_in = len(rm_cas_ids), len(in_cas_ids)
        removed, taken = ctypes.c_uint64(0), ctypes.c_uint64(0)
        torch.cuda.current_stream().synchronize()
        check(lib().sd_object_index_apply_hex(self.ctx.handle, self.handle, bufs[0] if m_rm else None,
                                              _ptr(ids[0]) if m_rm else None, m_rm, bufs[1] if m_in else None,
                                              _ptr(ids[1]) if m_in else None, m_in, ctypes.byref(removed),
                                              ctypes.byref(taken)))
        return int(removed.value), int(taken.value)

    def lookup(self, d_keys: torch.Tensor, d_object_ids: torch.Tensor = None, d_found: torch.Tensor = None,
               m: Optional[int] = None, stream=None):
        """-> (object ids int64 [m], found uint8 [m]) for m keys in any order."""
        m = int(d_keys.numel()) if m is None else m
        if d_object_ids is None:
            d_object_ids = torch.empty(max(m, 1), dtype=torch.int64, device=d_keys.device)
        if d_found is None:
            d_found = torch.empty(max(m, 1), dtype=torch.uint8, device=d_keys.device)
        check(lib().sd_object_index_lookup(self.ctx.handle, self.handle, _ptr(d_keys) if m else None, m,
                                           _ptr(d_object_ids), _ptr(d_found), _stream(stream)))
        return d_object_ids[:m], d_found[:m]

    def export(self, stream=None):
        """-> (keys int64 [n] ascending as u64, object ids int64 [n]) on the context's device."""
        n = len(self)
        dev = torch.device("cuda", self.ctx.device)
        k = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        v = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        check(lib().sd_object_index_export(self.ctx.handle, self.handle, _ptr(k), _ptr(v), max(n, 1), _stream(stream)))
        return k[:n], v[:n]

    def owners(self, d_records, m: int, d_rep, d_owner, d_existing, d_new, d_n_new, chunk_size: int = 100,
               stream=None) -> None:
        """sd_dedup_owners_indexed on grouped records; d_n_new is a device int64 [1]."""
        check(lib().sd_dedup_owners_indexed(self.ctx.handle, self.handle, _ptr(d_records), m, _ptr(d_rep), chunk_size,
                                            _ptr(d_owner), _ptr(d_existing), _ptr(d_new), _ptr(d_n_new),
                                            _stream(stream)))

    def close(self) -> None:
        if self.handle:
            lib().sd_object_index_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HostObjectIndex:
    """The host twin (sd_cpu_object_index): the same index over numpy arrays, for a host
    without a gfx950 device.  Keys and Object ids are uint64 arrays."""

    def __init__(self, nparts: int = 1, part: int = 0, owners: bool = False):
        self.nparts, self.part, self.owners_mode = nparts, part, bool(owners)
        h = ctypes.c_void_p()
        if owners:
            check(lib().sd_cpu_object_index_create_ex(nparts, part, SD_OBJECT_INDEX_OWNERS, ctypes.byref(h)))
        else:
            check(lib().sd_cpu_object_index_create(nparts, part, ctypes.byref(h)))
        self.handle = h

    @property
    def flags(self) -> int:
        f = ctypes.c_int(0)
        check(lib().sd_cpu_object_index_flags(self.handle, ctypes.byref(f)))
        return int(f.value)

    def links(self, keys, object_ids) -> np.ndarray:
        """-> uint64 [m]: the link count of each (key, Object id) pair, 0 if absent (owners mode)."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        v = np.ascontiguousarray(object_ids, dtype=np.uint64)
        assert k.size == v.size
        out = np.zeros(max(k.size, 1), np.uint64)
        check(lib().sd_cpu_object_index_links(self.handle, _ptr(k) if k.size else None, _ptr(v) if k.size else None,
                                              k.size, _ptr(out)))
        return out[:k.size]

    def export_links(self):
        """-> (keys, Object ids, links) uint64 [n] in ascending (key, id) order (owners mode)."""
        n = len(self)
        k, v, c = (np.zeros(max(n, 1), np.uint64) for _ in range(3))
        check(lib().sd_cpu_object_index_export_links(self.handle, _ptr(k), _ptr(v), _ptr(c), max(n, 1)))
        return k[:n], v[:n], c[:n]

    def __len__(self) -> int:
        n = ctypes.c_uint64(0)
        check(lib().sd_cpu_object_index_count(self.handle, ctypes.byref(n)))
        return int(n.value)

    def insert(self, keys, object_ids) -> int:
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        v = np.ascontiguousarray(object_ids, dtype=np.uint64)
        assert k.size == v.size
        taken = ctypes.c_uint64(0)
        check(lib().sd_cpu_object_index_insert(self.handle, _ptr(k) if k.size else None, _ptr(v) if k.size else None,
                                               k.size, ctypes.byref(taken)))
        return int(taken.value)

    def _removal(self, call, bound: int, capacity):
        removed = ctypes.c_uint64(0)
        cap = max(int(bound), 1) if capacity is None else int(capacity)
        out = np.zeros((max(cap, 1), 2), np.uint64)
        try:
            check(call(_ptr(out), cap, ctypes.byref(removed)))
        except SdCasError as e:
            e.needed = int(removed.value)
            raise
        r = int(removed.value)
        return out[:r], r

    def remove(self, keys, object_ids=None, capacity: Optional[int] = None, orphans: bool = False):
        """sd_cpu_object_index_remove -> (removed pairs uint64 [r, 2] ascending by key, r);
        `capacity` (rows) below the count raises SdCasError (SD_ERR_CAPACITY, ``.needed``)
        and leaves the index unchanged.  ``orphans=True`` appends the Objects of the removed
        pairs that now own nothing in this index."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        v = None if object_ids is None else np.ascontiguousarray(object_ids, dtype=np.uint64)
        assert v is None or v.size == k.size
        res = self._removal(lambda out, cap, removed: lib().sd_cpu_object_index_remove(
            self.handle, _ptr(k) if k.size else None, _ptr(v) if k.size and v is not None else None, k.size, out, cap,
            removed), len(self) if self.owners_mode and v is None else min(k.size, len(self)), capacity)
        return res + (self._orphans_of(res[0]),) if orphans else res

    def remove_hex(self, cas_ids, object_ids=None) -> int:
        """remove from the DB's strings; returns the count."""
        return self.remove(np.array([int(c, 16) for c in cas_ids], dtype=np.uint64), object_ids)[1]

    def remove_objects(self, object_ids, capacity: Optional[int] = None, orphans: bool = False):
        """sd_cpu_object_index_remove_objects -> (removed pairs uint64 [r, 2], r); ``orphans`` as
        remove."""
        v = np.ascontiguousarray(object_ids, dtype=np.uint64)
        res = self._removal(lambda out, cap, removed: lib().sd_cpu_object_index_remove_objects(
            self.handle, _ptr(v) if v.size else None, v.size, out, cap, removed), len(self), capacity)
        return res + (self._orphans_of(res[0]),) if orphans else res

    def object_links(self, object_ids, stride: int = 1, m: Optional[int] = None):
        """sd_cpu_object_index_object_links -> (links, entries) uint64 [m] per listed Object id;
        ``stride`` / ``m`` as ObjectIndex.object_links."""
        v = np.ascontiguousarray(object_ids, dtype=np.uint64).reshape(-1)
        m = (v.size + stride - 1) // max(stride, 1) if m is None else int(m)
        assert m == 0 or stride not in (1, 2) or (m - 1) * stride < v.size
        links, entries = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
        check(lib().sd_cpu_object_index_object_links(self.handle, _ptr(v) if m else None, stride, m, _ptr(links),
                                                     _ptr(entries)))
        return links[:m], entries[:m]

    def orphans(self, object_ids, stride: int = 1, m: Optional[int] = None, capacity: Optional[int] = None):
        """sd_cpu_object_index_orphans -> uint64 [count]: the distinct listed ids without an entry
        in this index, ascending; `capacity` below the count raises SdCasError (SD_ERR_CAPACITY,
        ``.needed``)."""
        v = np.ascontiguousarray(object_ids, dtype=np.uint64).reshape(-1)
        m = (v.size + stride - 1) // max(stride, 1) if m is None else int(m)
        assert m == 0 or stride not in (1, 2) or (m - 1) * stride < v.size
        cap = max(m, 1) if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), np.uint64)
        count = ctypes.c_uint64(0)
        try:
            check(lib().sd_cpu_object_index_orphans(self.handle, _ptr(v) if m else None, stride, m, _ptr(out), cap,
                                                    ctypes.byref(count)))
        except SdCasError as e:
            e.needed = int(count.value)
            raise
        return out[:int(count.value)]

    def key_links(self, keys):
        """sd_cpu_object_index_key_links -> (links, owners) uint64 [m] per listed key."""
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        links, owners = np.zeros(max(k.size, 1), np.uint64), np.zeros(max(k.size, 1), np.uint64)
        check(lib().sd_cpu_object_index_key_links(self.handle, _ptr(k) if k.size else None, k.size, _ptr(links),
                                                  _ptr(owners)))
        return links[:k.size], owners[:k.size]

    def _group_rows(self, fn, ncols: int, min_links: int, min_owners: int, capacity):
        count = ctypes.c_uint64(0)
        if capacity is None:  # count first, then exactly that many rows
            check(fn(self.handle, min_links, min_owners, *([None] * ncols), 0, ctypes.byref(count)))
            capacity = int(count.value)
        out = tuple(np.zeros(max(int(capacity), 1), np.uint64) for _ in range(ncols))
        try:
            check(fn(self.handle, min_links, min_owners, *(_ptr(a) for a in out), int(capacity), ctypes.byref(count)))
        except SdCasError as e:
            e.needed = int(count.value)
            raise
        return tuple(a[:int(count.value)] for a in out)

    def duplicates(self, min_links: int = 0, min_owners: int = 0, capacity: Optional[int] = None):
        """sd_cpu_object_index_duplicates -> (keys, first, links, owners) uint64 [count], ascending;
        `capacity` (rows) below the count raises SdCasError (SD_ERR_CAPACITY, ``.needed``)."""
        return self._group_rows(lib().sd_cpu_object_index_duplicates, 4, min_links, min_owners, capacity)

    def duplicate_entries(self, min_links: int = 0, min_owners: int = 0, capacity: Optional[int] = None):
        """sd_cpu_object_index_duplicate_entries -> (keys, ids, links) uint64 [count] in (key, id)
        order; `capacity` as duplicates."""
        return self._group_rows(lib().sd_cpu_object_index_duplicate_entries, 3, min_links, min_owners, capacity)

    def duplicate_stats(self) -> np.ndarray:
        """sd_cpu_object_index_duplicate_stats -> uint64 [8], as ObjectIndex.duplicate_stats."""
        out = np.zeros(8, np.uint64)
        check(lib().sd_cpu_object_index_duplicate_stats(self.handle, _ptr(out)))
        return out

    def _orphans_of(self, pairs: np.ndarray) -> np.ndarray:
        r = len(pairs)
        flat = np.ascontiguousarray(pairs).reshape(-1)
        return self.orphans(flat[1:] if r else flat, stride=2, m=r)

    def apply(self, rm_keys, rm_ids, in_keys, in_ids, capacity: Optional[int] = None, orphans: bool = False):
        """sd_cpu_object_index_apply -> (removed pairs uint64 [r, 2] in ascending (key, id) order,
        taken), the net effect of the removal list then the insertion list (owners mode);
        ``orphans=True`` appends the Objects of those pairs that now own nothing in this index."""
        rk, rv, ik, iv = (np.ascontiguousarray(a, dtype=np.uint64) for a in (rm_keys, rm_ids, in_keys, in_ids))
        assert rk.size == rv.size and ik.size == iv.size
        taken = ctypes.c_uint64(0)
        pairs, _ = self._removal(lambda out, cap, removed: lib().sd_cpu_object_index_apply(
            self.handle, _ptr(rk) if rk.size else None, _ptr(rv) if rk.size else None, rk.size,
            _ptr(ik) if ik.size else None, _ptr(iv) if ik.size else None, ik.size, out, cap, removed,
            ctypes.byref(taken)), min(rk.size, len(self)), capacity)
        if orphans:
            return pairs, int(taken.value), self._orphans_of(pairs)
        return pairs, int(taken.value)

    def merge_objects(self, from_ids, to_ids):
        """sd_cpu_object_index_merge_objects -> (moved, coalesced), as ObjectIndex.merge_objects."""
        f, t = (np.ascontiguousarray(a, dtype=np.uint64) for a in (from_ids, to_ids))
        assert f.size == t.size
        moved, coalesced = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().sd_cpu_object_index_merge_objects(self.handle, _ptr(f) if f.size else None,
                                                      _ptr(t) if f.size else None, f.size, ctypes.byref(moved),
                                                      ctypes.byref(coalesced)))
        return int(moved.value), int(coalesced.value)

    def lookup(self, keys):
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        ids = np.zeros(max(k.size, 1), np.uint64)
        found = np.zeros(max(k.size, 1), np.uint8)
        check(lib().sd_cpu_object_index_lookup(self.handle, _ptr(k) if k.size else None, k.size, _ptr(ids),
                                               _ptr(found)))
        return ids[:k.size], found[:k.size]

    def export(self):
        n = len(self)
        k = np.zeros(max(n, 1), np.uint64)
        v = np.zeros(max(n, 1), np.uint64)
        check(lib().sd_cpu_object_index_export(self.handle, _ptr(k), _ptr(v), max(n, 1)))
        return k[:n], v[:n]

    def owners(self, records: np.ndarray, rep: np.ndarray, chunk_size: int = 100):
        """sd_cpu_dedup_owners_indexed on grouped records (int64 [m, 2], rep int64 [m]) ->
        (owner uint64 [m], existing uint8 [m], new heads uint64 [n_new, 2])."""
        m = len(records)
        r = np.ascontiguousarray(records).view(np.uint64).reshape(-1)
        p = np.ascontiguousarray(rep).view(np.uint64)
        owner = np.zeros(max(m, 1), np.uint64)
        existing = np.zeros(max(m, 1), np.uint8)
        new = np.zeros((max(m, 1), 2), np.uint64)
        n_new = ctypes.c_uint64(0)
        check(lib().sd_cpu_dedup_owners_indexed(self.handle, _ptr(r) if m else None, m, _ptr(p) if m else None,
                                                chunk_size, _ptr(owner), _ptr(existing), _ptr(new),
                                                ctypes.byref(n_new)))
        return owner[:m], existing[:m], new[:int(n_new.value)]

    def close(self) -> None:
        if self.handle:
            lib().sd_cpu_object_index_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class CommGroup:
    """sd_comm_group: the in-process rendezvous of ``nranks`` ranks that are threads of one
    process (one Comm per thread, each on its own Context).  Close it after its Comms."""

    def __init__(self, nranks: int):
        h = ctypes.c_void_p()
        check(lib().sd_comm_group_create(nranks, ctypes.byref(h)))
        self.handle, self.nranks = h, nranks

    def close(self) -> None:
        if self.handle:
            lib().sd_comm_group_destroy(self.handle)
            self.handle = None


class Comm:
    """libsdcas's communicator (sd_comm): one per rank, on its context's device -- RCCL, or
    the in-process transport of a CommGroup."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(Comm.ID_BYTES)
        check(lib().sd_comm_id(buf))
        return buf.raw

    def __init__(self, ctx: Context, uid: Optional[bytes], nranks: int, rank: int,
                 group: Optional["CommGroup"] = None):
        """RCCL (``uid`` from ``unique_id()`` on one rank) or, with ``group``, the in-process
        transport (sd_comm_create_local: the ranks are threads of this process)."""
        h = ctypes.c_void_p()
        if group is not None:
            assert group.nranks == nranks
            check(lib().sd_comm_create_local(ctx.handle, group.handle, rank, ctypes.byref(h)))
        else:
            assert uid is not None and len(uid) == Comm.ID_BYTES
            check(lib().sd_comm_create(ctx.handle, uid, nranks, rank, ctypes.byref(h)))
        self.handle, self.nranks, self.rank, self.group = h, nranks, rank, group

    PHASES = ("partition", "allgather_rows", "host_turnaround", "sendrecv", "group_owners")  # SD_DEDUP_PHASES

    def set_timing(self, on: bool) -> None:
        """sd_comm_set_timing: record HIP events at the phases of each sd_cas_dedup_mgpu call."""
        check(lib().sd_comm_set_timing(self.handle, 1 if on else 0))

    def last_phases(self) -> dict:
        """sd_comm_last_phases: the last timed call's phase durations (ms), by name."""
        ms = (ctypes.c_float * len(Comm.PHASES))()
        check(lib().sd_comm_last_phases(self.handle, ms))
        return {k: float(v) for k, v in zip(Comm.PHASES, ms)}

    def close(self) -> None:
        if self.handle:
            lib().sd_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class CasBatch:
    """Prepared cas_id batch (sd_cas_batch): run over device-resident staged messages."""

    def __init__(self, ctx: Context, extents: np.ndarray):
        self.ctx = ctx
        self.extents = np.ascontiguousarray(extents, dtype=EXTENT_DTYPE)
        h = ctypes.c_void_p()
        check(lib().sd_cas_batch_create(ctx.handle, _ptr(self.extents), len(self.extents), ctypes.byref(h)))
        self.handle = h
        st = np.zeros(8, np.uint64)
        check(lib().sd_cas_batch_stats(h, _ptr(st)))
        (self.n, self.n_sampled, self.n_whole, self.whole_chunks, self.compressions,
         self.msg_bytes, self.full_items, self.tail_items) = (int(v) for v in st)

    def run(self, d_staged: torch.Tensor, d_hash32: torch.Tensor, stream=None) -> None:
        assert d_hash32.numel() >= 32 * self.n and d_staged.is_cuda and d_hash32.is_cuda
        check(lib().sd_cas_batch_run(self.ctx.handle, self.handle, _ptr(d_staged), _ptr(d_hash32),
                                     _stream(stream)))

    def run_part(self, parts: int, d_staged: torch.Tensor, d_hash32: torch.Tensor, stream=None) -> None:
        """parts: 1 = sampled-file kernel only, 2 = whole-file kernels only."""
        check(lib().sd_cas_batch_run_part(self.ctx.handle, self.handle, parts, _ptr(d_staged), _ptr(d_hash32),
                                          _stream(stream)))

    def time(self, d_staged, d_hash32, iters: int, stream=None) -> float:
        ms = ctypes.c_float(0)
        check(lib().sd_cas_batch_time(self.ctx.handle, self.handle, _ptr(d_staged), _ptr(d_hash32), iters,
                                      _stream(stream), ctypes.byref(ms)))
        return float(ms.value)

    def close(self) -> None:
        if self.handle:
            lib().sd_cas_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class ChecksumBatch:
    """Prepared full-file checksum batch (sd_checksum_batch) over byte ranges of one buffer."""

    def __init__(self, ctx: Context, offsets, lens):
        self.ctx = ctx
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64)
        h = ctypes.c_void_p()
        check(lib().sd_checksum_batch_create(ctx.handle, _ptr(self.offsets), _ptr(self.lens), len(self.lens),
                                             ctypes.byref(h)))
        self.handle = h
        st = np.zeros(4, np.uint64)
        check(lib().sd_checksum_batch_stats(h, _ptr(st)))
        self.n, self.total_bytes, self.compressions, self.blocks = (int(v) for v in st)

    def run(self, d_data: torch.Tensor, d_hash32: torch.Tensor, stream=None) -> None:
        assert d_hash32.numel() >= 32 * self.n
        check(lib().sd_checksum_batch_run(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_hash32),
                                          _stream(stream)))

    def time(self, d_data, d_hash32, iters: int, stream=None) -> float:
        ms = ctypes.c_float(0)
        check(lib().sd_checksum_batch_time(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_hash32), iters,
                                           _stream(stream), ctypes.byref(ms)))
        return float(ms.value)

    def close(self) -> None:
        if self.handle:
            lib().sd_checksum_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class ChecksumTree:
    """Prepared checksum-tree batch (sd_checksum_tree) over byte ranges of one buffer: every
    file's level at 2^block_log2 bytes (128 KiB .. 1 MiB) beside its checksum.  File i's nodes are
    rows node_base[i] .. node_base[i + 1] of the [total_nodes, 32] level buffer."""

    def __init__(self, ctx: Context, offsets, lens, block_log2: int = 17):
        self.ctx = ctx
        self.block_log2 = int(block_log2)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64)
        h = ctypes.c_void_p()
        check(lib().sd_checksum_tree_create(ctx.handle, _ptr(self.offsets), _ptr(self.lens), len(self.lens),
                                            self.block_log2, ctypes.byref(h)))
        self.handle = h
        st = np.zeros(4, np.uint64)
        check(lib().sd_checksum_tree_stats(h, _ptr(st)))
        self.n, self.total_bytes, self.compressions, self.total_nodes = (int(v) for v in st)
        self.node_base = np.zeros(self.n + 1, np.uint64)
        check(lib().sd_checksum_tree_layout(h, _ptr(self.node_base)))

    def run(self, d_data: torch.Tensor, d_nodes: torch.Tensor, d_hash32: torch.Tensor, stream=None) -> None:
        """one pass over the data: the levels -> d_nodes, the roots -> d_hash32"""
        assert d_nodes.numel() >= 32 * self.total_nodes and d_hash32.numel() >= 32 * self.n
        check(lib().sd_checksum_tree_run(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_nodes), _ptr(d_hash32),
                                         _stream(stream)))

    def roots(self, d_nodes: torch.Tensor, d_hash32: torch.Tensor, stream=None) -> None:
        """the roots from the levels alone -> d_hash32"""
        assert d_nodes.numel() >= 32 * self.total_nodes and d_hash32.numel() >= 32 * self.n
        check(lib().sd_checksum_tree_roots(self.ctx.handle, self.handle, _ptr(d_nodes), _ptr(d_hash32),
                                           _stream(stream)))

    def verify(self, d_data: torch.Tensor, d_expected: torch.Tensor, d_bad: Optional[torch.Tensor] = None,
               d_rows_out: Optional[torch.Tensor] = None, capacity: Optional[int] = None, want_rows: bool = True,
               stream=None):
        """sd_checksum_tree_verify: hashes d_data's blocks and compares them with d_expected (a level
        buffer).  Returns (rows int64 [count, 2] of (file, block) ascending, stats uint64 [4]: files,
        blocks compared, blocks that differ, files with a differing block), and d_bad (uint8
        [total_nodes], written when given) as a third value.  Without d_rows_out the rows go to a
        tensor with room for every block; with it and a short `capacity` the call
        raises SdCasError (SD_ERR_CAPACITY, ``.needed`` rows, ``.stats``) and writes no row.
        want_rows=False only counts (rows comes back empty)."""
        assert d_expected.numel() >= 32 * self.total_nodes and (d_bad is None or d_bad.numel() >= self.total_nodes)
        st = _stream(stream)
        count = ctypes.c_uint64(0)
        stats = np.zeros(4, np.uint64)

        def call(rows, cap):
            rc = lib().sd_checksum_tree_verify(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_expected), _ptr(d_bad),
                                               _ptr(rows), cap, ctypes.byref(count), _ptr(stats), st)
            try:
                check(rc)
            except SdCasError as e:
                e.needed = int(count.value)
                e.stats = stats
                raise

        dev = torch.device("cuda", self.ctx.device)
        if not want_rows:
            call(None, 0)
            rows = torch.empty((0, 2), dtype=torch.int64, device=dev)
        elif d_rows_out is None:  # room for every block: 16 B per >= 128 KiB of data, and one pass
            rows = torch.empty((max(self.total_nodes, 1), 2), dtype=torch.int64, device=dev)
            call(rows, self.total_nodes)
            rows = rows[:int(count.value)]
        else:
            assert d_rows_out.dtype == torch.int64 and d_rows_out.is_cuda and d_rows_out.is_contiguous()
            call(d_rows_out, d_rows_out.numel() // 2 if capacity is None else int(capacity))
            rows = d_rows_out.reshape(-1)[:2 * int(count.value)].reshape(-1, 2)
        return (rows, stats) if d_bad is None else (rows, stats, d_bad)

    def close(self) -> None:
        if self.handle:
            lib().sd_checksum_tree_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class ChecksumTreeBlocks:
    """A list of blocks (sd_checksum_tree_blocks) of files of lengths `lens`: row r = (file, block),
    its bytes at d_data[data_offsets[r]:] wherever they sit (16-byte aligned starts).  Only the
    listed bytes are hashed.  The levels are laid out as ChecksumTree's: file i's nodes are rows
    node_base[i] .. node_base[i + 1]."""

    def __init__(self, ctx: Context, lens, rows, data_offsets, block_log2: int = 17):
        from .cpu import tree_node_base
        self.ctx = ctx
        self.block_log2 = int(block_log2)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
        self.data_offsets = np.ascontiguousarray(data_offsets, dtype=np.uint64).reshape(-1)
        if len(self.rows) != len(self.data_offsets):
            raise ValueError("rows and data_offsets differ in length")
        h = ctypes.c_void_p()
        check(lib().sd_checksum_tree_blocks_create(ctx.handle, _ptr(self.lens), len(self.lens), self.block_log2,
                                                   _ptr(self.rows), _ptr(self.data_offsets), len(self.rows),
                                                   ctypes.byref(h)))
        self.handle = h
        st = np.zeros(4, np.uint64)
        check(lib().sd_checksum_tree_blocks_stats(h, _ptr(st)))
        self.n, self.m, self.bytes_hashed, self.compressions = (int(v) for v in st)
        self.node_base = tree_node_base(self.lens, self.block_log2)
        self.total_nodes = int(self.node_base[self.n])
        self._proof_base = None
        self.q, self.range_base, self.range_proof_base = 0, np.zeros(1, np.uint64), np.zeros(1, np.uint64)

    def run(self, d_data: torch.Tensor, d_nodes_out: torch.Tensor, stream=None) -> None:
        """row r's node -> d_nodes_out[32 r], list order"""
        assert d_nodes_out.numel() >= 32 * self.m
        check(lib().sd_checksum_tree_blocks_run(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_nodes_out),
                                                _stream(stream)))

    def verify(self, d_data: torch.Tensor, d_expected: torch.Tensor, d_bad: Optional[torch.Tensor] = None,
               d_rows_out: Optional[torch.Tensor] = None, capacity: Optional[int] = None, want_rows: bool = True,
               stream=None):
        """sd_checksum_tree_blocks_verify: hashes the listed blocks and compares each with its node of
        d_expected (the whole level buffer).  Returns (rows int64 [count, 2] of (file, block) in list
        order, stats uint64 [4]: files, rows compared, rows that differ, files with a differing row),
        and d_bad (uint8 [m], written when given) as a third value.  Rows, capacity and want_rows as
        ChecksumTree.verify."""
        assert d_expected.numel() >= 32 * self.total_nodes and (d_bad is None or d_bad.numel() >= self.m)
        st = _stream(stream)
        count = ctypes.c_uint64(0)
        stats = np.zeros(4, np.uint64)

        def call(rows, cap):
            rc = lib().sd_checksum_tree_blocks_verify(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_expected),
                                                      _ptr(d_bad), _ptr(rows), cap, ctypes.byref(count), _ptr(stats), st)
            try:
                check(rc)
            except SdCasError as e:
                e.needed = int(count.value)
                e.stats = stats
                raise

        dev = torch.device("cuda", self.ctx.device)
        if not want_rows:
            call(None, 0)
            rows = torch.empty((0, 2), dtype=torch.int64, device=dev)
        elif d_rows_out is None:
            rows = torch.empty((max(self.m, 1), 2), dtype=torch.int64, device=dev)
            call(rows, self.m)
            rows = rows[:int(count.value)]
        else:
            assert d_rows_out.dtype == torch.int64 and d_rows_out.is_cuda and d_rows_out.is_contiguous()
            call(d_rows_out, d_rows_out.numel() // 2 if capacity is None else int(capacity))
            rows = d_rows_out.reshape(-1)[:2 * int(count.value)].reshape(-1, 2)
        return (rows, stats) if d_bad is None else (rows, stats, d_bad)

    def update(self, d_data: torch.Tensor, d_nodes: torch.Tensor, d_hash32: torch.Tensor, stream=None) -> None:
        """the listed blocks' nodes -> their slots of d_nodes (the whole level buffer, patched in
        place), then every file's root from the patched level -> d_hash32"""
        assert d_nodes.numel() >= 32 * self.total_nodes and d_hash32.numel() >= 32 * self.n
        check(lib().sd_checksum_tree_blocks_update(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_nodes),
                                                   _ptr(d_hash32), _stream(stream)))

    @property
    def proof_base(self) -> np.ndarray:
        """uint64 [m + 1]: row r's proof is entries proof_base[r] .. proof_base[r + 1] (32 bytes each)
        of the packed proofs; the counts follow from the lengths, the block size and the rows alone"""
        if self._proof_base is None:
            base = np.zeros(self.m + 1, np.uint64)
            check(lib().sd_checksum_tree_blocks_proof_layout(self.handle, _ptr(base)))
            self._proof_base = base
        return self._proof_base

    def prove(self, d_nodes: torch.Tensor, d_proofs_out: torch.Tensor, stream=None) -> None:
        """every row's proof, in list order, from the whole level buffer d_nodes -> d_proofs_out
        (proof_base[m] x 32 bytes); no file byte is read"""
        assert d_nodes.numel() >= 32 * self.total_nodes and d_proofs_out.numel() >= 32 * int(self.proof_base[self.m])
        check(lib().sd_checksum_tree_blocks_prove(self.ctx.handle, self.handle, _ptr(d_nodes), _ptr(d_proofs_out),
                                                  _stream(stream)))

    def verify_proofs(self, d_data: torch.Tensor, d_proofs: torch.Tensor, d_roots: torch.Tensor,
                      d_nodes_out: Optional[torch.Tensor] = None, d_bad: Optional[torch.Tensor] = None,
                      d_rows_out: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
                      want_rows: bool = True, stream=None):
        """sd_checksum_tree_blocks_verify_proofs: hashes the listed blocks, climbs each row's node
        through its proof (d_proofs, laid out by proof_base) and compares the result with its file's
        checksum in d_roots ([n, 32]).  d_nodes_out ([m, 32], optional) receives the rows' nodes.
        Returns what verify returns: (rows, stats), and d_bad as a third value when given."""
        assert d_roots.numel() >= 32 * self.n and d_proofs.numel() >= 32 * int(self.proof_base[self.m])
        assert (d_bad is None or d_bad.numel() >= self.m) and (d_nodes_out is None or d_nodes_out.numel() >= 32 * self.m)
        st = _stream(stream)
        count = ctypes.c_uint64(0)
        stats = np.zeros(4, np.uint64)

        def call(rows, cap):
            rc = lib().sd_checksum_tree_blocks_verify_proofs(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_proofs),
                                                             _ptr(d_roots), _ptr(d_nodes_out), _ptr(d_bad), _ptr(rows),
                                                             cap, ctypes.byref(count), _ptr(stats), st)
            try:
                check(rc)
            except SdCasError as e:
                e.needed = int(count.value)
                e.stats = stats
                raise

        dev = torch.device("cuda", self.ctx.device)
        if not want_rows:
            call(None, 0)
            rows = torch.empty((0, 2), dtype=torch.int64, device=dev)
        elif d_rows_out is None:
            rows = torch.empty((max(self.m, 1), 2), dtype=torch.int64, device=dev)
            call(rows, self.m)
            rows = rows[:int(count.value)]
        else:
            assert d_rows_out.dtype == torch.int64 and d_rows_out.is_cuda and d_rows_out.is_contiguous()
            call(d_rows_out, d_rows_out.numel() // 2 if capacity is None else int(capacity))
            rows = d_rows_out.reshape(-1)[:2 * int(count.value)].reshape(-1, 2)
        return (rows, stats) if d_bad is None else (rows, stats, d_bad)

    def set_ranges(self, range_base) -> None:
        """sd_checksum_tree_blocks_set_ranges: range i is rows range_base[i] .. range_base[i + 1] of
        the list, consecutive blocks of one file; range_base uint64 [q + 1] ascends strictly from 0
        to m.  A refused call leaves the ranges as they were; calling again replaces them."""
        rb = np.ascontiguousarray(range_base, dtype=np.uint64).reshape(-1)
        q = max(len(rb) - 1, 0)
        check(lib().sd_checksum_tree_blocks_set_ranges(self.handle, _ptr(rb) if len(rb) else None, q))
        self.range_base, self.q = rb, q
        base = np.zeros(q + 1, np.uint64)
        check(lib().sd_checksum_tree_blocks_range_proof_layout(self.handle, _ptr(base)))
        self.range_proof_base = base

    def prove_ranges(self, d_nodes: torch.Tensor, d_proofs_out: torch.Tensor, stream=None) -> None:
        """every range's proof (its left and right flanks, bottom-up), in range order, from the
        whole level buffer d_nodes -> d_proofs_out (range_proof_base[q] x 32 bytes)"""
        assert d_nodes.numel() >= 32 * self.total_nodes
        assert d_proofs_out.numel() >= 32 * int(self.range_proof_base[self.q])
        check(lib().sd_checksum_tree_blocks_prove_ranges(self.ctx.handle, self.handle, _ptr(d_nodes),
                                                         _ptr(d_proofs_out), _stream(stream)))

    def verify_range_proofs(self, d_data: torch.Tensor, d_proofs: torch.Tensor, d_roots: torch.Tensor,
                            d_nodes_out: Optional[torch.Tensor] = None, d_bad: Optional[torch.Tensor] = None,
                            d_ranges_out: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
                            want_rows: bool = True, stream=None):
        """sd_checksum_tree_blocks_verify_range_proofs: hashes the listed blocks, climbs each range
        through its proof (d_proofs, laid out by range_proof_base) and compares the result with its
        file's checksum in d_roots ([n, 32]).  d_nodes_out ([m, 32], optional) receives the rows'
        nodes.  Returns (ranges int64 [count, 3] of (file, first block, blocks) in range order, stats
        uint64 [4]: files, ranges compared, ranges that differ, files with one), and d_bad (uint8
        [q]) as a third value when given.  A failing range does not say which of its blocks is wrong."""
        assert d_roots.numel() >= 32 * self.n and d_proofs.numel() >= 32 * int(self.range_proof_base[self.q])
        assert (d_bad is None or d_bad.numel() >= self.q) and (d_nodes_out is None or d_nodes_out.numel() >= 32 * self.m)
        st = _stream(stream)
        count = ctypes.c_uint64(0)
        stats = np.zeros(4, np.uint64)

        def call(rows, cap):
            rc = lib().sd_checksum_tree_blocks_verify_range_proofs(self.ctx.handle, self.handle, _ptr(d_data),
                                                                   _ptr(d_proofs), _ptr(d_roots), _ptr(d_nodes_out),
                                                                   _ptr(d_bad), _ptr(rows), cap, ctypes.byref(count),
                                                                   _ptr(stats), st)
            try:
                check(rc)
            except SdCasError as e:
                e.needed = int(count.value)
                e.stats = stats
                raise

        dev = torch.device("cuda", self.ctx.device)
        if not want_rows:
            call(None, 0)
            rows = torch.empty((0, 3), dtype=torch.int64, device=dev)
        elif d_ranges_out is None:
            rows = torch.empty((max(self.q, 1), 3), dtype=torch.int64, device=dev)
            call(rows, self.q)
            rows = rows[:int(count.value)]
        else:
            assert d_ranges_out.dtype == torch.int64 and d_ranges_out.is_cuda and d_ranges_out.is_contiguous()
            call(d_ranges_out, d_ranges_out.numel() // 3 if capacity is None else int(capacity))
            rows = d_ranges_out.reshape(-1)[:3 * int(count.value)].reshape(-1, 3)
        return (rows, stats) if d_bad is None else (rows, stats, d_bad)

    def close(self) -> None:
        if self.handle:
            lib().sd_checksum_tree_blocks_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class FingerprintBatch:
    """Prepared fingerprint batch (sd_fingerprint_batch): cas hash and checksum of files that
    are byte ranges of one device buffer, the cas messages gathered on the device."""

    def __init__(self, ctx: Context, offsets, lens):
        self.ctx = ctx
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64)
        if len(self.offsets) != len(self.lens):
            raise ValueError("offsets and lens differ in length")
        h = ctypes.c_void_p()
        check(lib().sd_fingerprint_batch_create(ctx.handle, _ptr(self.offsets), _ptr(self.lens), len(self.lens),
                                                ctypes.byref(h)))
        self.handle = h
        st = np.zeros(8, np.uint64)
        check(lib().sd_fingerprint_batch_stats(h, _ptr(st)))
        (self.n, self.n_sampled, self.n_whole, self.file_bytes, self.staged_bytes, self.cas_compressions,
         self.checksum_compressions, self.gather_read_bytes) = (int(v) for v in st)
        self.extents = np.zeros(self.n, dtype=EXTENT_DTYPE)
        check(lib().sd_fingerprint_batch_extents(h, _ptr(self.extents)))

    def gather(self, d_data: torch.Tensor, d_staged: torch.Tensor, stream=None) -> None:
        """The cas messages alone, into d_staged (>= staged_bytes) at ``extents``."""
        assert d_staged.numel() >= self.staged_bytes and d_data.is_cuda and d_staged.is_cuda
        check(lib().sd_fingerprint_batch_gather(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_staged),
                                                _stream(stream)))

    def run(self, d_data: torch.Tensor, d_cas_hash32: torch.Tensor, d_checksum32: torch.Tensor, stream=None) -> None:
        """gather + cas kernels + checksum kernels; n x 32 B each (the cas_id is a row's first 8)."""
        assert d_cas_hash32.numel() >= 32 * self.n and d_checksum32.numel() >= 32 * self.n and d_data.is_cuda
        check(lib().sd_fingerprint_batch_run(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_cas_hash32),
                                             _ptr(d_checksum32), _stream(stream)))

    def close(self) -> None:
        if self.handle:
            lib().sd_fingerprint_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class SplitChecksum:
    """One file's checksum over the ranks of a communicator (sd_split_checksum): this rank
    hashes its block range to CVs; the gathered CVs reduce to the file's BLAKE3."""

    def __init__(self, ctx: Context, total_len: int, nranks: int = 1, rank: int = 0):
        from .split import split_range
        self.ctx = ctx
        self.total_len, self.nranks, self.rank = int(total_len), nranks, rank
        self.offset, self.len, self.cv_bytes = split_range(total_len, nranks, rank)
        h = ctypes.c_void_p()
        check(lib().sd_split_checksum_create(ctx.handle, self.total_len, nranks, rank, ctypes.byref(h)))
        self.handle = h

    def leaves(self, d_slice: torch.Tensor, d_cvs: torch.Tensor, stream=None) -> None:
        assert d_cvs.numel() >= self.cv_bytes and d_slice.numel() >= self.len
        check(lib().sd_split_checksum_leaves(self.ctx.handle, self.handle, _ptr(d_slice), _ptr(d_cvs),
                                             _stream(stream)))

    def root(self, d_cvs: torch.Tensor, d_hash32: torch.Tensor, stream=None) -> None:
        assert d_cvs.numel() >= self.cv_bytes and d_hash32.numel() >= 32
        check(lib().sd_split_checksum_root(self.ctx.handle, self.handle, _ptr(d_cvs), _ptr(d_hash32),
                                           _stream(stream)))

    def mgpu(self, comm: "Comm", d_slice: torch.Tensor, d_cvs: torch.Tensor, d_hash32: torch.Tensor,
             stream=None) -> None:
        assert d_cvs.numel() >= self.cv_bytes and d_slice.numel() >= self.len and d_hash32.numel() >= 32
        check(lib().sd_split_checksum_mgpu(self.ctx.handle, comm.handle, self.handle, _ptr(d_slice), _ptr(d_cvs),
                                           _ptr(d_hash32), _stream(stream)))

    def close(self) -> None:
        if self.handle:
            lib().sd_split_checksum_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


_default: dict = {}


def default_context(device: Optional[int] = None) -> Context:
    if device is None:
        device = torch.cuda.current_device()
    ctx = _default.get(device)
    if ctx is None:
        ctx = _default[device] = Context(device)
    return ctx
