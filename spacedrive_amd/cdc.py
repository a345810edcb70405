"""Content-defined chunks (include/sd_cas.h, content-defined chunks): content that is there more
than once at ANY offset -- what tree.shared_blocks, which compares aligned blocks where they lie,
cannot see: a file with its header rewritten, a log and its rotated copy, an edited document.

A file is cut where its content says so (a gear rolling hash over the last 64 bytes; a cut where
its top mask_bits bits are zero, between min_size and max_size bytes after the last one), every
chunk's id is the BLAKE3 of its bytes, and chunks are grouped by (length, id).

``delta_files`` / ``patch_files`` act on the answer: a file stored or sent as another file's chunks
plus its own few (sd_cdc_delta_plan, _pack, _apply; csrc/cdc_delta.hip), rebuilt and checked against
its checksum.

``Cdc`` runs the three steps on the device over a torch buffer that holds the files as byte ranges
(csrc/cdc.hip, csrc/tree_shared.hip); ``chunk_files`` and ``compare_files`` read files from disk,
upload them once and use it, or the library's CPU twins (cpu.cdc_cut, cpu.cdc_hash, cpu.cdc_shared)
where there is no device.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
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



# ---------------------------------------------------------------- deltas
def delta_plan(ctx, chunk_base, n_base: int, d_chunks, d_rep, d_lit_off=None, d_runs_out=None, capacity: int = 0,
               d_files_out=None, stream=None):
    """sd_cdc_delta_plan: files n_base .. n-1 of the table as runs out of files 0 .. n_base-1 and a
    literal buffer.  Returns (n_runs, stats uint64 [8]); the outputs given are written (lit_off int64
    [target slots]; runs int64 [capacity, 4] = (t, source, src_off, bytes); files int64 [targets, 6]).
    A short `capacity` raises SdCasError (SD_ERR_CAPACITY, ``.needed`` rows, ``.stats``)."""
    from .device import _ptr, _stream
    base = np.ascontiguousarray(chunk_base, dtype=np.uint64).reshape(-1)
    n = max(len(base) - 1, 0)
    n_runs = ctypes.c_uint64(0)
    stats = np.zeros(8, np.uint64)
    rc = lib().sd_cdc_delta_plan(ctx.handle, base.ctypes.data if n else None, n, int(n_base), _ptr(d_chunks) if n else None,
                                 _ptr(d_rep) if n else None, _ptr(d_lit_off), _ptr(d_runs_out), capacity,
                                 ctypes.byref(n_runs), _ptr(d_files_out), stats.ctypes.data, _stream(stream))
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(n_runs.value)
        e.stats = stats
        raise
    return int(n_runs.value), stats


def delta_pack(ctx, chunk_base, n_base: int, offsets, d_chunks, d_lit_off, d_rep, d_data, d_lit_out, stream=None) -> None:
    """sd_cdc_delta_pack: the literal slots' bytes from d_data (the files at host `offsets`) into
    d_lit_out at their lit_off.  Asynchronous on the stream."""
    from .device import _ptr, _stream
    base = np.ascontiguousarray(chunk_base, dtype=np.uint64).reshape(-1)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    n = max(len(base) - 1, 0)
    if len(offs) != n:
        raise ValueError("offsets is not one per file")
    check(lib().sd_cdc_delta_pack(ctx.handle, base.ctypes.data if n else None, n, int(n_base), offs.ctypes.data if n else None,
                                  _ptr(d_chunks) if n else None, _ptr(d_lit_off), _ptr(d_rep) if n else None, _ptr(d_data),
                                  _ptr(d_lit_out), _stream(stream)))


def delta_apply(ctx, d_runs, n_runs: int, base_offsets, base_lens, d_base, d_lit, lit_bytes: int, out_offsets, out_lens,
                d_out, stream=None) -> None:
    """sd_cdc_delta_apply: validates the recipe on the device (a refused one raises SdCasError,
    SD_ERR_INVALID, with no byte of d_out written), then copies the runs into d_out at the host
    `out_offsets`.  The copy is asynchronous on the stream."""
    from .device import _ptr, _stream
    bo = np.ascontiguousarray(base_offsets, dtype=np.uint64).reshape(-1)
    bl = np.ascontiguousarray(base_lens, dtype=np.uint64).reshape(-1)
    oo = np.ascontiguousarray(out_offsets, dtype=np.uint64).reshape(-1)
    ol = np.ascontiguousarray(out_lens, dtype=np.uint64).reshape(-1)
    if len(bo) != len(bl) or len(oo) != len(ol):
        raise ValueError("offsets and lens differ in length")
    check(lib().sd_cdc_delta_apply(ctx.handle, _ptr(d_runs) if n_runs else None, int(n_runs),
                                   bo.ctypes.data if len(bl) else None, bl.ctypes.data if len(bl) else None, len(bl),
                                   _ptr(d_base), _ptr(d_lit) if lit_bytes else None, int(lit_bytes),
                                   oo.ctypes.data if len(ol) else None, ol.ctypes.data if len(ol) else None, len(ol),
                                   _ptr(d_out), _stream(stream)))


@dataclass
class Delta:
    """What delta_files leaves and patch_files takes: the recipe, the literal bytes, and what the
    rebuilt files must be.  No wire or file format is defined for it."""
    runs: np.ndarray         # uint64 [r, 4] = (t, source, src_off, bytes); source 0 = literals, 1 + g = base file g
    literals: np.ndarray     # uint8
    target_lens: np.ndarray  # uint64 [targets]
    checksums: np.ndarray    # uint8 [targets, 32]: file_checksum of each target
    files: np.ndarray        # uint64 [targets, 6]: chunks, copied chunks, copied bytes, new literal bytes, repeated bytes, runs
    stats: np.ndarray        # uint64 [8] of sd_cdc_delta_plan
    params: tuple            # (mask_bits, min_size, max_size)


def _cpu_checksums(buf, offs, lens, nthreads) -> np.ndarray:
    n = len(lens)
    out = np.zeros((max(n, 1), 32), np.uint8)
    if n:
        check(lib().sd_cpu_checksums(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, out.ctypes.data, nthreads))
    return out[:n]


def _device_checksums(ctx, d_data, offs, lens) -> np.ndarray:
    import torch
    n = len(lens)
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    hs = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ctx.checksum_batch(offs, lens).run(d_data, hs)
    return hs.cpu().numpy().reshape(n, 32)


def delta_files(base_paths, target_paths, params=None, device=None, nthreads: int = cpu.THREADS) -> Delta:
    """What does a holder of the files at `base_paths` need to rebuild those at `target_paths`?  Base
    and targets are read once and uploaded once; cut, hash, shared, plan and pack run on the device
    (or on the CPU twins where there is none), and the targets' checksums come from the checksum
    batch over the same upload.  Returns a Delta."""
    base_paths, target_paths = list(base_paths), list(target_paths)
    buf, offs, lens = _pack(base_paths + target_paths)
    nb, n = len(base_paths), len(lens)
    pr = cdc_params(params)
    ptuple = (int(pr.mask_bits), int(pr.min_size), int(pr.max_size))
    if not _use_device(device):
        base, chunks, _ = cpu.cdc_cut(buf, offs, lens, pr, nthreads=nthreads)
        ids = cpu.cdc_hash(buf, offs, lens, base, chunks, nthreads)
        rep = cpu.cdc_shared(base, chunks, ids, want_pairs=False)[0]
        lit_off, runs, files, stats = cpu.cdc_delta_plan(base, nb, chunks, rep)
        lit = cpu.cdc_delta_pack(buf, offs, base, nb, chunks, rep, lit_off, int(stats[5]))
        sums = _cpu_checksums(buf, offs[nb:], lens[nb:], nthreads)
        return Delta(runs.copy(), lit.copy(), lens[nb:].copy(), sums, files.copy(), stats, ptuple)
    import torch
    from .device import default_context
    ctx = default_context()
    d_data = torch.from_numpy(buf).cuda()
    c = Cdc(ctx, offs, lens, pr)
    try:
        m = c.cut(d_data)
        base = c.layout()
        mt = m - (int(base[nb]) if n else 0)
        d_chunks = torch.zeros((max(m, 1), 2), dtype=torch.int64, device="cuda")
        d_ids = torch.zeros((max(m, 1), 32), dtype=torch.uint8, device="cuda")
        c.hash(d_data, d_chunks, d_ids)
        d_rep = torch.zeros(max(m, 1), dtype=torch.int64, device="cuda")
        c.shared(d_chunks, d_ids, d_rep=d_rep)
        d_lit_off = torch.zeros(max(mt, 1), dtype=torch.int64, device="cuda")
        d_runs = torch.zeros((max(mt, 1), 4), dtype=torch.int64, device="cuda")
        d_files = torch.zeros((max(n - nb, 1), 6), dtype=torch.int64, device="cuda")
        n_runs, stats = delta_plan(ctx, base, nb, d_chunks, d_rep, d_lit_off, d_runs, mt, d_files)
        d_lit = torch.zeros(max(int(stats[5]), 1), dtype=torch.uint8, device="cuda")
        delta_pack(ctx, base, nb, offs, d_chunks, d_lit_off, d_rep, d_data, d_lit)
        sums = _device_checksums(ctx, d_data, offs[nb:], lens[nb:])
        return Delta(d_runs[:n_runs].cpu().numpy().view(np.uint64), d_lit[:int(stats[5])].cpu().numpy(), lens[nb:].copy(), sums,
                     d_files[:n - nb].cpu().numpy().view(np.uint64), stats, ptuple)
    finally:
        c.close()


def patch_files(base_paths, delta: Delta, device=None, nthreads: int = cpu.THREADS) -> list:
    """Rebuilds the targets of `delta` from the files at `base_paths` and checks every one against
    delta.checksums.  Returns the rebuilt files as uint8 arrays.  A recipe that is not valid for these
    base files raises SdCasError (nothing is rebuilt); a rebuilt file whose checksum differs raises
    ValueError naming it."""
    buf, offs, lens = _pack(list(base_paths))
    out_lens = np.ascontiguousarray(delta.target_lens, dtype=np.uint64).reshape(-1)
    nt = len(out_lens)
    sums = np.ascontiguousarray(delta.checksums, dtype=np.uint8).reshape(-1, 32)
    if len(sums) != nt:
        raise ValueError("delta.checksums is not one per target")
    out_offs, cur = np.zeros(nt, np.uint64), 0
    for t in range(nt):  # as _pack lays files out: what the checksum batch reads
        out_offs[t] = cur
        cur += (int(out_lens[t]) + 63) // 64 * 64 + 64
    runs = np.ascontiguousarray(delta.runs, dtype=np.uint64).reshape(-1, 4)
    lit = np.ascontiguousarray(delta.literals, dtype=np.uint8).reshape(-1)
    if not _use_device(device):
        out = np.zeros(cur + 64, np.uint8)
        cpu.cdc_delta_apply(runs, buf, offs, lens, lit, out_lens, out, out_offs, nthreads)
        got = _cpu_checksums(out, out_offs, out_lens, nthreads)
    else:
        import torch
        from .device import default_context
        ctx = default_context()
        d_base = torch.from_numpy(buf).cuda()
        lit_pad = np.zeros((len(lit) + 63) // 64 * 64 + 64, np.uint8)
        lit_pad[:len(lit)] = lit
        d_lit = torch.from_numpy(lit_pad).cuda()
        d_runs = torch.from_numpy(runs.view(np.int64).reshape(-1).copy() if len(runs) else np.zeros(4, np.int64)).cuda()
        d_out = torch.zeros(cur + 64, dtype=torch.uint8, device="cuda")
        delta_apply(ctx, d_runs, len(runs), offs, lens, d_base, d_lit, len(lit), out_offs, out_lens, d_out)
        got = _device_checksums(ctx, d_out, out_offs, out_lens)
        out = d_out.cpu().numpy()
    for t in range(nt):
        if not np.array_equal(got[t], sums[t]):
            raise ValueError(f"target {t}: the rebuilt file's checksum {got[t].tobytes().hex()} is not the delta's "
                             f"{sums[t].tobytes().hex()}")
    return [out[int(o):int(o) + int(ln)].copy() for o, ln in zip(out_offs, out_lens)]
