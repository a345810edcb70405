"""Content-defined chunks (include/sd_cas.h, content-defined chunks): content that is there more
than once at ANY offset -- what tree.shared_blocks, which compares aligned blocks where they lie,
cannot see: a file with its header rewritten, a log and its rotated copy, an edited document.

A file is cut where its content says so (a gear rolling hash over the last 64 bytes; a cut where
its top mask_bits bits are zero, between min_size and max_size bytes after the last one), every
chunk's id is the BLAKE3 of its bytes, and chunks are grouped by (length, id).

``Cdc`` runs the three steps on the device over a torch buffer that holds the files as byte ranges
(csrc/cdc.hip, csrc/tree_shared.hip); ``chunk_files`` and ``compare_files`` read files from disk,
upload them once and use it, or the library's CPU twins (cpu.cdc_cut, cpu.cdc_hash, cpu.cdc_shared)
where there is no device.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import cpu
from ._native import SdCasError, check, lib
from .cpu import CdcParams, cdc_params  # noqa: F401
from .tree import _read


class Cdc:
    """sd_cdc: the content-defined chunks of files that are byte ranges (host offsets / lens, 16-byte
    aligned starts, readable to the next 64-byte boundary after each range) of one device buffer.
    cut() scans and selects, hash() gives the chunk table and the ids, shared() the report.  One
    cut or hash runs at a time."""

    def __init__(self, ctx, offsets, lens, params=None):
        self.ctx = ctx
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
        if len(self.offsets) != len(self.lens):
            raise ValueError("offsets and lens differ in length")
        self.n = len(self.lens)
        self.params = cdc_params(params)
        self.n_chunks: Optional[int] = None
        h = ctypes.c_void_p()
        check(lib().sd_cdc_create(ctx.handle, self.offsets.ctypes.data if self.n else None,
                                  self.lens.ctypes.data if self.n else None, self.n, ctypes.byref(self.params),
                                  ctypes.byref(h)))
        self.handle = h

    def close(self) -> None:
        if self.handle:
            lib().sd_cdc_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def cut(self, d_data, stream=None) -> int:
        """sd_cdc_cut: the number of chunks; syncs the stream."""
        from .device import _ptr, _stream
        m = ctypes.c_uint64(0)
        check(lib().sd_cdc_cut(self.ctx.handle, self.handle, _ptr(d_data), _stream(stream), ctypes.byref(m)))
        self.n_chunks = int(m.value)
        return self.n_chunks

    def layout(self) -> np.ndarray:
        """sd_cdc_layout: chunk_base uint64 [n + 1], the exclusive prefix sum of the chunks per file."""
        base = np.zeros(self.n + 1, np.uint64)
        check(lib().sd_cdc_layout(self.handle, base.ctypes.data))
        return base

    def stats(self) -> np.ndarray:
        """sd_cdc_stats: uint64 [8] = files, bytes, candidates, chunks, chunks ended at a candidate,
        forced, at the file's end, BLAKE3 compressions of the hash."""
        out = np.zeros(8, np.uint64)
        check(lib().sd_cdc_stats(self.handle, out.ctypes.data))
        return out

    def hash(self, d_data, d_chunks=None, d_ids=None, stream=None) -> None:
        """sd_cdc_hash into the outputs given: d_chunks int64 [m, 2] = (offset in the file, length),
        d_ids uint8 [m, 32], both in layout order.  Asynchronous on the stream."""
        from .device import _ptr, _stream
        check(lib().sd_cdc_hash(self.ctx.handle, self.handle, _ptr(d_data), _ptr(d_chunks), _ptr(d_ids), _stream(stream)))

    def shared(self, d_chunks, d_ids, min_chunks: int = 0, d_rep=None, d_class_size=None, d_files_out=None,
               d_pairs_out=None, capacity: int = 0, stream=None):
        """sd_cdc_shared over this batch's layout: (n_pairs, stats uint64 [8]); the outputs given are
        written (rep, class_size int64 [m]; files int64 [n, 4]; pairs int64 [capacity, 4]).  A short
        `capacity` raises SdCasError (SD_ERR_CAPACITY, ``.needed`` rows, ``.stats``)."""
        return shared(self.ctx, self.layout(), d_chunks, d_ids, min_chunks, d_rep, d_class_size, d_files_out, d_pairs_out,
                      capacity, stream)


def shared(ctx, chunk_base, d_chunks, d_ids, min_chunks: int = 0, d_rep=None, d_class_size=None, d_files_out=None,
           d_pairs_out=None, capacity: int = 0, stream=None):
    """sd_cdc_shared: chunk_base host uint64 [n + 1]; d_chunks, d_ids on the device."""
    from .device import _ptr, _stream
    base = np.ascontiguousarray(chunk_base, dtype=np.uint64).reshape(-1)
    n = max(len(base) - 1, 0)
    n_pairs = ctypes.c_uint64(0)
    stats = np.zeros(8, np.uint64)
    rc = lib().sd_cdc_shared(ctx.handle, base.ctypes.data if n else None, n, _ptr(d_chunks) if n else None,
                             _ptr(d_ids) if n else None, int(min_chunks), _ptr(d_rep), _ptr(d_class_size),
                             _ptr(d_files_out), _ptr(d_pairs_out), capacity, ctypes.byref(n_pairs), stats.ctypes.data,
                             _stream(stream))
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(n_pairs.value)
        e.stats = stats
        raise
    return int(n_pairs.value), stats


def _pack(paths):
    """(buffer, offsets, lens): the files read as file_checksum reads them, at 64-byte aligned starts
    of one zeroed buffer with 64 spare bytes after each"""
    datas = [_read(p) for p in paths]
    offs, cur = np.zeros(len(datas), np.uint64), 0
    for i, d in enumerate(datas):
        offs[i] = cur
        cur += (len(d) + 63) // 64 * 64 + 64
    buf = np.zeros(cur + 64, np.uint8)
    for d, o in zip(datas, offs):
        buf[int(o):int(o) + len(d)] = d
    return buf, offs, np.array([len(d) for d in datas], np.uint64)


def _use_device(device) -> bool:
    if device is not None:
        return bool(device)
    import torch
    return torch.cuda.is_available()


def _run(paths, params, min_chunks, want_shared: bool, device, nthreads):
    buf, offs, lens = _pack(paths)
    n = len(lens)
    if not _use_device(device):
        base, chunks, stats = cpu.cdc_cut(buf, offs, lens, params, nthreads=nthreads)
        ids = cpu.cdc_hash(buf, offs, lens, base, chunks, nthreads)
        if not want_shared:
            return base, chunks, ids, stats
        _, _, files, pairs, sstats = cpu.cdc_shared(base, chunks, ids, min_chunks)
        return base, chunks, ids, stats, files, pairs, sstats
    import torch
    from .device import default_context
    ctx = default_context()
    d_data = torch.from_numpy(buf).cuda()
    c = Cdc(ctx, offs, lens, params)
    try:
        m = c.cut(d_data)
        d_chunks = torch.zeros((max(m, 1), 2), dtype=torch.int64, device="cuda")
        d_ids = torch.zeros((max(m, 1), 32), dtype=torch.uint8, device="cuda")
        c.hash(d_data, d_chunks, d_ids)
        base, stats = c.layout(), c.stats()
        out = (base, d_chunks[:m].cpu().numpy().view(np.uint64), d_ids[:m].cpu().numpy(), stats)
        if not want_shared:
            return out
        d_files = torch.zeros((max(n, 1), 4), dtype=torch.int64, device="cuda")
        d_pairs = torch.zeros((max(m, 1), 4), dtype=torch.int64, device="cuda")
        n_pairs, sstats = c.shared(d_chunks, d_ids, min_chunks, d_files_out=d_files, d_pairs_out=d_pairs, capacity=m)
        return out + (d_files[:n].cpu().numpy().view(np.uint64), d_pairs[:n_pairs].cpu().numpy().view(np.uint64), sstats)
    finally:
        c.close()


def chunk_files(paths, params=None, device=None, nthreads: int = cpu.THREADS):
    """The content-defined chunks of the files at `paths`, each read once.  Returns (chunk_base
    uint64 [n + 1], chunks uint64 [m, 2] = (offset in its file, length), ids uint8 [m, 32], stats
    uint64 [8]); file f's chunks are rows chunk_base[f] .. chunk_base[f + 1].  `device`: True / False,
    or None for the device when there is one."""
    return _run(list(paths), params, 0, False, device, nthreads)


def compare_files(paths: list, params=None, min_chunks: int = 0, device=None, nthreads: int = cpu.THREADS):
    """What does file f repeat of earlier files, at any offset?  Returns (files uint64 [n, 4] =
    (chunks, shared, redundant, redundant bytes) per file, pairs uint64 [p, 4] = (f, g, chunks,
    bytes): g < f is the FIRST holder of that many of f's chunks, ascending by (f, g), stats uint64
    [8] of sd_cdc_shared).  A chunk a file repeats of itself is redundant and has no pair row."""
    out = _run(list(paths), params, min_chunks, True, device, nthreads)
    return out[4], out[5], out[6]

