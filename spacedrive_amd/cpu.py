"""The library's CPU path (libsdcas.so ``sd_cpu_*``), with the names and error behaviour of
``spacedrive_amd.cas``: for a node without a gfx950 device, and what the latency policy
uses for few concurrent single-file calls.

Same file-read semantics as the GPU path (cas.rs:23-62, hash.rs:10-24); the hashing is
the library's own host BLAKE3 (csrc/cpu_blake3.cpp: AVX-512 / AVX2 / SSE2 chunk lanes).
It needs no device and no torch device state.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Union

import numpy as np

from ._native import SD_FILE_OK, check, hex_results, lib, path_array
from .cas import _status_error

THREADS = 16  # host threads for batches (the CPU share of one GPU on an MI355X node)


def simd_lanes() -> int:
    """Chunk lanes of the host hasher on this CPU (16 AVX-512, 8 AVX2, 4 SSE2)."""
    return int(lib().sd_cpu_simd_lanes())


def generate_cas_ids(paths: Sequence[Union[str, os.PathLike]], sizes: Sequence[int],
                     nthreads: int = THREADS) -> List[Union[str, OSError]]:
    n = len(paths)
    if n != len(sizes):
        raise ValueError("paths and sizes differ in length")
    if n == 0:
        return []
    sizes_a = np.ascontiguousarray(sizes, dtype=np.uint64)
    status = np.zeros(n, np.int32)
    keep, arr = path_array(paths)
    out = ctypes.create_string_buffer(17 * n)
    check(lib().sd_cpu_cas_ids_files(arr, sizes_a.ctypes.data, n, out, status.ctypes.data, nthreads))
    return hex_results(out, 16, status, paths, _status_error)


def generate_cas_id(path: Union[str, os.PathLike], size: int) -> str:
    """cas.rs:23 on the calling thread."""
    out = ctypes.create_string_buffer(17)
    st = ctypes.c_int32(0)
    check(lib().sd_cpu_cas_id_path(os.fsencode(path), int(size), out, ctypes.byref(st)))
    if st.value != SD_FILE_OK:
        raise _status_error(st.value, os.fsdecode(path))
    return out.raw[:16].decode()


def file_checksums(paths: Sequence[Union[str, os.PathLike]],
                   nthreads: int = THREADS) -> List[Union[str, OSError]]:
    n = len(paths)
    if n == 0:
        return []
    keep, arr = path_array(paths)
    out = ctypes.create_string_buffer(65 * n)
    status = np.zeros(n, np.int32)
    check(lib().sd_cpu_file_checksums(arr, n, out, status.ctypes.data, nthreads))
    return hex_results(out, 64, status, paths, _status_error)


def file_checksum(path: Union[str, os.PathLike]) -> str:
    """hash.rs:10 on the calling thread."""
    out = ctypes.create_string_buffer(65)
    st = ctypes.c_int32(0)
    check(lib().sd_cpu_file_checksum_path(os.fsencode(path), out, ctypes.byref(st)))
    if st.value != SD_FILE_OK:
        raise _status_error(st.value, os.fsdecode(path))
    return out.raw[:64].decode()


def cas_ids_staged(staged: np.ndarray, extents: np.ndarray, status: Optional[np.ndarray] = None,
                   nthreads: int = THREADS) -> List[str]:
    """sd_cpu_cas_ids over host-staged messages (extents as stage_plan builds them)."""
    n = len(extents)
    out = ctypes.create_string_buffer(17 * max(n, 1))
    check(lib().sd_cpu_cas_ids(staged.ctypes.data, staged.nbytes, extents.ctypes.data, n, out,
                               None if status is None else status.ctypes.data, nthreads))
    raw = out.raw  # one copy: each .raw access copies the whole buffer
    return [raw[17 * i:17 * i + 16].decode() for i in range(n)]


def fingerprints(data, offsets, lens, nthreads: int = THREADS):
    """sd_cpu_fingerprints: (cas_ids, checksums) of n byte ranges of a host buffer (starts
    16-byte aligned, size hashed = lens[i]) on host threads; no device."""
    from .cas import _host_ranges, _split_hex
    keep, addr, offs, ls = _host_ranges(data, offsets, lens)
    n = len(ls)
    o17, o65 = ctypes.create_string_buffer(17 * max(n, 1)), ctypes.create_string_buffer(65 * max(n, 1))
    check(lib().sd_cpu_fingerprints(addr, offs.ctypes.data, ls.ctypes.data, n, o17, o65, nthreads))
    return _split_hex(o17, 16, n), _split_hex(o65, 64, n)


def confirm(keys, hash32, valid=None, capacity: Optional[int] = None, want_sets: bool = True):
    """sd_cpu_dedup_confirm: candidate groups (keys uint64 [m]) split into classes of equal
    checksums (hash32 uint8 [m, 32]); valid uint8 [m] or None.  Returns (rep uint64 [m],
    class_size uint64 [m], verdict uint8 [m], sets uint64 [n_sets, 3], stats uint64 [8]).
    `capacity` (default m // 2, always enough) short of the sets raises SdCasError
    (SD_ERR_CAPACITY) with ``.needed``; want_sets=False only counts (sets comes back empty)."""
    from ._native import SdCasError
    k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    m = len(k)
    h = np.ascontiguousarray(hash32, dtype=np.uint8).reshape(-1)
    if h.size != 32 * m:
        raise ValueError("hash32 is not m x 32 bytes")
    v = None if valid is None else np.ascontiguousarray(np.asarray(valid).reshape(-1) != 0, dtype=np.uint8)
    if v is not None and v.size != m:
        raise ValueError("valid is not m bytes")
    rep, size = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
    verdict = np.zeros(max(m, 1), np.uint8)
    cap = m // 2 if capacity is None else int(capacity)
    sets = np.zeros((max(cap, 1), 3), np.uint64)
    n_sets = ctypes.c_uint64(0)
    stats = np.zeros(8, np.uint64)
    rc = lib().sd_cpu_dedup_confirm(k.ctypes.data if m else None, h.ctypes.data if m else None,
                                    None if v is None else v.ctypes.data, m, rep.ctypes.data, size.ctypes.data,
                                    verdict.ctypes.data, sets.ctypes.data if want_sets else None, cap,
                                    ctypes.byref(n_sets), stats.ctypes.data)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(n_sets.value)
        raise
    return rep[:m], size[:m], verdict[:m], sets[:int(n_sets.value) if want_sets else 0], stats


def tree_nodes(length: int, block_log2: int = 17) -> int:
    """sd_checksum_tree_nodes: the blocks (= nodes) of a file of `length` bytes."""
    v = ctypes.c_uint64(0)
    check(lib().sd_checksum_tree_nodes(int(length), int(block_log2), ctypes.byref(v)))
    return int(v.value)


def tree_node_base(lens, block_log2: int = 17) -> np.ndarray:
    """node_base uint64 [n + 1] of a batch: the exclusive prefix sum of the files' node counts."""
    tree_nodes(0, block_log2)  # refuses a block size outside 128 KiB .. 1 MiB
    ls = np.ascontiguousarray(lens, dtype=np.uint64)
    nb = np.maximum((ls + np.uint64((1 << block_log2) - 1)) >> np.uint64(block_log2), np.uint64(1))
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(nb, dtype=np.uint64)])


def checksum_tree(data, offsets, lens, block_log2: int = 17, nthreads: int = THREADS):
    """sd_cpu_checksum_tree: (nodes uint8 [node_base[n], 32], roots uint8 [n, 32], node_base) of n
    byte ranges of a host buffer (starts 16-byte aligned): every file's level at 2^block_log2
    bytes and its file_checksum (hash.rs:10-24)."""
    from .cas import _host_ranges
    keep, addr, offs, ls = _host_ranges(data, offsets, lens)
    n = len(ls)
    base = tree_node_base(ls, block_log2)
    nodes, roots = np.zeros((max(int(base[n]), 1), 32), np.uint8), np.zeros((max(n, 1), 32), np.uint8)
    check(lib().sd_cpu_checksum_tree(addr, offs.ctypes.data, ls.ctypes.data, n, int(block_log2), nodes.ctypes.data,
                                     roots.ctypes.data, nthreads))
    return nodes[:int(base[n])], roots[:n], base


def checksum_tree_roots(nodes, lens, block_log2: int = 17) -> np.ndarray:
    """sd_cpu_checksum_tree_roots: roots uint8 [n, 32] from the levels alone."""
    ls = np.ascontiguousarray(lens, dtype=np.uint64)
    n = len(ls)
    nd = np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1)
    if nd.size != 32 * int(tree_node_base(ls, block_log2)[n]):
        raise ValueError("nodes is not node_base[n] x 32 bytes")
    roots = np.zeros((max(n, 1), 32), np.uint8)
    check(lib().sd_cpu_checksum_tree_roots(nd.ctypes.data if nd.size else None, ls.ctypes.data, n, int(block_log2),
                                           roots.ctypes.data))
    return roots[:n]


def checksum_tree_verify(data, offsets, lens, expected, block_log2: int = 17, capacity: Optional[int] = None,
                         want_rows: bool = True, want_flags: bool = False, nthreads: int = THREADS):
    """sd_cpu_checksum_tree_verify: the blocks of n byte ranges whose node differs from `expected`
    (uint8 [node_base[n], 32]).  Returns (rows uint64 [count, 2] of (file, block) ascending, stats
    uint64 [4]: files, blocks compared, blocks that differ, files with a differing block) and, with
    want_flags, the 0/1 byte per node as a third value.  `capacity` (default: every block) short of
    the rows raises SdCasError (SD_ERR_CAPACITY) with ``.needed`` and writes no row;
    want_rows=False only counts (rows comes back empty)."""
    from ._native import SdCasError
    from .cas import _host_ranges
    keep, addr, offs, ls = _host_ranges(data, offsets, lens)
    n = len(ls)
    total = int(tree_node_base(ls, block_log2)[n])
    exp = np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1)
    if exp.size != 32 * total:
        raise ValueError("expected is not node_base[n] x 32 bytes")
    cap = total if capacity is None else int(capacity)
    rows = np.zeros((max(cap, 1), 2), np.uint64)
    bad = np.zeros(max(total, 1), np.uint8)
    count = ctypes.c_uint64(0)
    stats = np.zeros(4, np.uint64)
    rc = lib().sd_cpu_checksum_tree_verify(addr, offs.ctypes.data, ls.ctypes.data, n, int(block_log2),
                                           exp.ctypes.data if n else None, bad.ctypes.data if want_flags else None,
                                           rows.ctypes.data if want_rows else None, cap, ctypes.byref(count),
                                           stats.ctypes.data, nthreads)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(count.value)
        e.stats = stats
        raise
    out = (rows[:int(count.value) if want_rows else 0], stats)
    return out + (bad[:total],) if want_flags else out


def _block_list(lens, rows, data_offsets, block_log2: int):
    """(lens u64 [n_files], rows u64 [m, 2], data_offsets u64 [m], the rows' byte counts or None when
    a row names no block -- the library refuses such a list before it reads anything)"""
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    rw = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    offs = np.ascontiguousarray(data_offsets, dtype=np.uint64).reshape(-1)
    if len(offs) != len(rw):
        raise ValueError("rows and data_offsets differ in length")
    sizes = None
    if len(rw) and 10 <= int(block_log2) <= 40 and int(rw[:, 0].max()) < len(ls):
        B = 1 << int(block_log2)
        sizes = [max(0, min(B, int(ls[int(f)]) - int(j) * B)) for f, j in rw]
    return ls, rw, offs, sizes


def _block_data(data, offs, sizes):
    from .cas import _host_ranges
    if sizes is None:
        sizes = np.zeros(len(offs), np.uint64)
    keep, addr, _, _ = _host_ranges(data, offs, np.array(sizes, np.uint64))
    return keep, addr


def checksum_tree_blocks(data, lens, rows, data_offsets, block_log2: int = 17, nthreads: int = THREADS) -> np.ndarray:
    """sd_cpu_checksum_tree_blocks: the nodes uint8 [m, 32], in list order, of the listed blocks --
    row r = (file, block) of files of lengths `lens`, its bytes at data[data_offsets[r]:] (starts
    16-byte aligned).  Only the listed bytes are hashed."""
    ls, rw, offs, sizes = _block_list(lens, rows, data_offsets, block_log2)
    keep, addr = _block_data(data, offs, sizes)
    m = len(rw)
    out = np.zeros((max(m, 1), 32), np.uint8)
    check(lib().sd_cpu_checksum_tree_blocks(addr, ls.ctypes.data, len(ls), int(block_log2), rw.ctypes.data,
                                            offs.ctypes.data, m, out.ctypes.data, nthreads))
    return out[:m]


def checksum_tree_blocks_verify(data, lens, rows, data_offsets, expected, block_log2: int = 17,
                                capacity: Optional[int] = None, want_rows: bool = True, want_flags: bool = False,
                                nthreads: int = THREADS):
    """sd_cpu_checksum_tree_blocks_verify: the listed blocks whose node differs from its node of
    `expected` (the batch's whole level, uint8 [node_base[n_files], 32]).  Returns (rows uint64
    [count, 2] of (file, block) in list order, stats uint64 [4]: files, rows compared, rows that
    differ, files with a differing row) and, with want_flags, the 0/1 byte per row as a third
    value.  `capacity` (default: every row) short of the rows raises SdCasError (SD_ERR_CAPACITY)
    with ``.needed`` and writes no row; want_rows=False only counts."""
    from ._native import SdCasError
    ls, rw, offs, sizes = _block_list(lens, rows, data_offsets, block_log2)
    keep, addr = _block_data(data, offs, sizes)
    m = len(rw)
    exp = np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1)
    if sizes is not None and exp.size != 32 * int(tree_node_base(ls, block_log2)[len(ls)]):
        raise ValueError("expected is not node_base[n_files] x 32 bytes")
    cap = m if capacity is None else int(capacity)
    out_rows = np.zeros((max(cap, 1), 2), np.uint64)
    bad = np.zeros(max(m, 1), np.uint8)
    count = ctypes.c_uint64(0)
    stats = np.zeros(4, np.uint64)
    rc = lib().sd_cpu_checksum_tree_blocks_verify(addr, ls.ctypes.data, len(ls), int(block_log2), rw.ctypes.data,
                                                  offs.ctypes.data, m, exp.ctypes.data if exp.size else None,
                                                  bad.ctypes.data if want_flags else None,
                                                  out_rows.ctypes.data if want_rows else None, cap, ctypes.byref(count),
                                                  stats.ctypes.data, nthreads)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(count.value)
        e.stats = stats
        raise
    out = (out_rows[:int(count.value) if want_rows else 0], stats)
    return out + (bad[:m],) if want_flags else out


def checksum_tree_blocks_update(data, lens, rows, data_offsets, nodes, block_log2: int = 17,
                                nthreads: int = THREADS):
    """sd_cpu_checksum_tree_blocks_update: (the patched level uint8 [node_base[n_files], 32], roots
    uint8 [n_files, 32]) -- a copy of `nodes` with the listed blocks' nodes replaced by those of the
    bytes given, every other node as it was, and every file's root from it.  A (file, block) listed
    twice raises SdCasError (SD_ERR_INVALID)."""
    ls, rw, offs, sizes = _block_list(lens, rows, data_offsets, block_log2)
    keep, addr = _block_data(data, offs, sizes)
    nd = np.array(nodes, dtype=np.uint8).reshape(-1, 32)  # a copy: patched in place
    if sizes is not None and len(nd) != int(tree_node_base(ls, block_log2)[len(ls)]):
        raise ValueError("nodes is not node_base[n_files] x 32 bytes")
    roots = np.zeros((max(len(ls), 1), 32), np.uint8)
    check(lib().sd_cpu_checksum_tree_blocks_update(addr, ls.ctypes.data, len(ls), int(block_log2), rw.ctypes.data,
                                                   offs.ctypes.data, len(rw), nd.ctypes.data if nd.size else None,
                                                   roots.ctypes.data, nthreads))
    return nd, roots[:len(ls)]


def tree_proof_entries(length: int, block: int, block_log2: int = 17) -> int:
    """sd_checksum_tree_proof_entries: the 32-byte entries of the proof of `block` of a file of
    `length` bytes -- the levels at which the block's node has a sibling on its way to the root."""
    v = ctypes.c_uint32(0)
    check(lib().sd_checksum_tree_proof_entries(int(length), int(block_log2), int(block), ctypes.byref(v)))
    return int(v.value)


def tree_proof_base(lens, rows, block_log2: int = 17) -> np.ndarray:
    """proof_base uint64 [m + 1] of a list's rows: the exclusive prefix sum of their entry counts."""
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    rw = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    base = np.zeros(len(rw) + 1, np.uint64)
    for r, (f, j) in enumerate(rw):
        if int(f) >= len(ls):
            raise ValueError(f"row {r}: no such file")
        base[r + 1] = base[r] + np.uint64(tree_proof_entries(int(ls[int(f)]), int(j), block_log2))
    return base


def checksum_tree_blocks_prove(nodes, lens, rows, block_log2: int = 17):
    """sd_cpu_checksum_tree_blocks_prove: (proofs uint8 [proof_base[m], 32], proof_base) of the
    listed (file, block) rows from `nodes`, the batch's whole level uint8 [node_base[n_files], 32];
    only the listed files' levels are read.  Row r's proof is proofs[proof_base[r]:proof_base[r + 1]],
    bottom-up."""
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    rw = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    nd = np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1)
    if nd.size != 32 * int(tree_node_base(ls, block_log2)[len(ls)]):
        raise ValueError("nodes is not node_base[n_files] x 32 bytes")
    base = tree_proof_base(ls, rw, block_log2)
    total = int(base[len(rw)])
    out = np.zeros((max(total, 1), 32), np.uint8)
    check(lib().sd_cpu_checksum_tree_blocks_prove(nd.ctypes.data if nd.size else None, ls.ctypes.data, len(ls),
                                                  int(block_log2), rw.ctypes.data, len(rw), out.ctypes.data))
    return out[:total], base


def checksum_tree_blocks_verify_proofs(data, lens, rows, data_offsets, proofs, roots, block_log2: int = 17,
                                       capacity: Optional[int] = None, want_rows: bool = True,
                                       want_flags: bool = False, want_nodes: bool = False, nthreads: int = THREADS):
    """sd_cpu_checksum_tree_blocks_verify_proofs: the listed blocks whose node, climbed through its
    proof (`proofs`, laid out by tree_proof_base), does not reach its file's checksum (`roots` uint8
    [n_files, 32]; only the listed files' are read).  Returns (rows uint64 [count, 2] in list order,
    stats uint64 [4]) as checksum_tree_blocks_verify, then the 0/1 byte per row with want_flags and
    the rows' nodes uint8 [m, 32] with want_nodes.  `capacity` and want_rows as there."""
    from ._native import SdCasError
    ls, rw, offs, sizes = _block_list(lens, rows, data_offsets, block_log2)
    keep, addr = _block_data(data, offs, sizes)
    m = len(rw)
    pf = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1)
    rt = np.ascontiguousarray(roots, dtype=np.uint8).reshape(-1)
    if sizes is not None:
        if rt.size != 32 * len(ls):
            raise ValueError("roots is not n_files x 32 bytes")
        if pf.size != 32 * int(tree_proof_base(ls, rw, block_log2)[m]):
            raise ValueError("proofs is not proof_base[m] x 32 bytes")
    cap = m if capacity is None else int(capacity)
    out_rows = np.zeros((max(cap, 1), 2), np.uint64)
    bad = np.zeros(max(m, 1), np.uint8)
    nodes = np.zeros((max(m, 1), 32), np.uint8)
    count = ctypes.c_uint64(0)
    stats = np.zeros(4, np.uint64)
    rc = lib().sd_cpu_checksum_tree_blocks_verify_proofs(
        addr, ls.ctypes.data, len(ls), int(block_log2), rw.ctypes.data, offs.ctypes.data, m,
        pf.ctypes.data if pf.size else None, rt.ctypes.data if rt.size else None,
        nodes.ctypes.data if want_nodes else None, bad.ctypes.data if want_flags else None,
        out_rows.ctypes.data if want_rows else None, cap, ctypes.byref(count), stats.ctypes.data, nthreads)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(count.value)
        e.stats = stats
        raise
    out = (out_rows[:int(count.value) if want_rows else 0], stats)
    if want_flags:
        out += (bad[:m],)
    if want_nodes:
        out += (nodes[:m],)
    return out


def tree_range_proof_entries(length: int, first: int, count: int, block_log2: int = 17) -> int:
    """sd_checksum_tree_range_proof_entries: the 32-byte entries of the proof of blocks [first,
    first + count) of a file of `length` bytes -- its left and right flanks, at most two per level."""
    v = ctypes.c_uint32(0)
    check(lib().sd_checksum_tree_range_proof_entries(int(length), int(block_log2), int(first), int(count),
                                                     ctypes.byref(v)))
    return int(v.value)


def _range_base(range_base, m: int) -> np.ndarray:
    rb = np.ascontiguousarray(range_base, dtype=np.uint64).reshape(-1)
    if len(rb) == 0:
        if m:
            raise ValueError("range_base holds q + 1 entries")
        rb = np.zeros(1, np.uint64)
    return rb


def tree_range_proof_base(lens, rows, range_base, block_log2: int = 17) -> np.ndarray:
    """proof_base uint64 [q + 1] of a list's ranges (range i = rows range_base[i] .. range_base[i +
    1]): the exclusive prefix sum of their entry counts."""
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    rw = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    rb = _range_base(range_base, len(rw))
    base = np.zeros(len(rb), np.uint64)
    for i in range(len(rb) - 1):
        r0, r1 = int(rb[i]), int(rb[i + 1])
        if not 0 <= r0 < r1 <= len(rw) or int(rw[r0, 0]) >= len(ls):
            raise ValueError(f"range {i}: no such rows")
        base[i + 1] = base[i] + np.uint64(tree_range_proof_entries(int(ls[int(rw[r0, 0])]), int(rw[r0, 1]), r1 - r0,
                                                                   block_log2))
    return base


def checksum_tree_blocks_prove_ranges(nodes, lens, rows, range_base, block_log2: int = 17):
    """sd_cpu_checksum_tree_blocks_prove_ranges: (proofs uint8 [proof_base[q], 32], proof_base) of
    the ranges of the listed rows from `nodes`, the batch's whole level; only the levels of files
    with a range are read.  Range i's proof is proofs[proof_base[i]:proof_base[i + 1]], bottom-up,
    the left flank of a level before its right one."""
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    rw = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    rb = _range_base(range_base, len(rw))
    nd = np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1)
    if nd.size != 32 * int(tree_node_base(ls, block_log2)[len(ls)]):
        raise ValueError("nodes is not node_base[n_files] x 32 bytes")
    from ._native import SdCasError
    total = 0
    try:
        base = tree_range_proof_base(ls, rw, rb, block_log2)
        total = int(base[-1])
    except (SdCasError, ValueError):  # ranges the library refuses below, with its own message
        base = np.zeros(len(rb), np.uint64)
    out = np.zeros((max(total, 1), 32), np.uint8)
    check(lib().sd_cpu_checksum_tree_blocks_prove_ranges(nd.ctypes.data if nd.size else None, ls.ctypes.data, len(ls),
                                                         int(block_log2), rw.ctypes.data, len(rw), rb.ctypes.data,
                                                         len(rb) - 1, out.ctypes.data))
    return out[:total], base


def checksum_tree_blocks_verify_range_proofs(data, lens, rows, data_offsets, range_base, proofs, roots,
                                             block_log2: int = 17, capacity: Optional[int] = None,
                                             want_rows: bool = True, want_flags: bool = False,
                                             want_nodes: bool = False, nthreads: int = THREADS):
    """sd_cpu_checksum_tree_blocks_verify_range_proofs: the ranges of the listed rows whose blocks,
    climbed through the range's proof (`proofs`, laid out by tree_range_proof_base), do not reach the
    file's checksum (`roots` uint8 [n_files, 32]).  Returns (ranges uint64 [count, 3] of (file, first
    block, blocks) in range order, stats uint64 [4]: files, ranges compared, ranges that differ,
    files with one), then the 0/1 byte per range with want_flags and the rows' nodes uint8 [m, 32]
    with want_nodes.  A failing range does not say which of its blocks is wrong."""
    from ._native import SdCasError
    ls, rw, offs, sizes = _block_list(lens, rows, data_offsets, block_log2)
    keep, addr = _block_data(data, offs, sizes)
    m = len(rw)
    rb = _range_base(range_base, m)
    q = len(rb) - 1
    pf = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1)
    rt = np.ascontiguousarray(roots, dtype=np.uint8).reshape(-1)
    if sizes is not None and rt.size != 32 * len(ls):
        raise ValueError("roots is not n_files x 32 bytes")
    try:
        need = 32 * int(tree_range_proof_base(ls, rw, rb, block_log2)[-1])
    except (SdCasError, ValueError):  # ranges the library refuses below, with its own message
        need = pf.size
    if pf.size != need:
        raise ValueError("proofs is not proof_base[q] x 32 bytes")
    cap = q if capacity is None else int(capacity)
    out_rows = np.zeros((max(cap, 1), 3), np.uint64)
    bad = np.zeros(max(q, 1), np.uint8)
    nodes = np.zeros((max(m, 1), 32), np.uint8)
    count = ctypes.c_uint64(0)
    stats = np.zeros(4, np.uint64)
    rc = lib().sd_cpu_checksum_tree_blocks_verify_range_proofs(
        addr, ls.ctypes.data, len(ls), int(block_log2), rw.ctypes.data, offs.ctypes.data, m, rb.ctypes.data, q,
        pf.ctypes.data if pf.size else None, rt.ctypes.data if rt.size else None,
        nodes.ctypes.data if want_nodes else None, bad.ctypes.data if want_flags else None,
        out_rows.ctypes.data if want_rows else None, cap, ctypes.byref(count), stats.ctypes.data, nthreads)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(count.value)
        e.stats = stats
        raise
    out = (out_rows[:int(count.value) if want_rows else 0], stats)
    if want_flags:
        out += (bad[:q],)
    if want_nodes:
        out += (nodes[:m],)
    return out


def checksum_tree_shared(lens, nodes, block_log2: int = 17, min_blocks: int = 0, capacity: Optional[int] = None,
                         want_pairs: bool = True):
    """sd_cpu_checksum_tree_shared: which blocks of a batch of levels (lens uint64 [n], nodes uint8
    [node_base[n], 32] in the level layout) are there more than once.  Returns (rep uint64 [m],
    class_size uint64 [m], files uint64 [n, 4], pairs uint64 [n_pairs, 4], stats uint64 [8]): a
    file's row is (blocks, shared, redundant, redundant bytes), a pair's (f, g, blocks, bytes) with
    g < f the first holder of those blocks.  `capacity` (default m, always enough) short of the
    pairs raises SdCasError (SD_ERR_CAPACITY) with ``.needed``; want_pairs=False only counts."""
    from ._native import SdCasError
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    n = len(ls)
    m = int(tree_node_base(ls, block_log2)[n])
    nd = np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1)
    if nd.size != 32 * m:
        raise ValueError("nodes is not node_base[n] x 32 bytes")
    rep, size = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
    files = np.zeros((max(n, 1), 4), np.uint64)
    cap = m if capacity is None else int(capacity)
    pairs = np.zeros((max(cap, 1), 4), np.uint64)
    n_pairs = ctypes.c_uint64(0)
    stats = np.zeros(8, np.uint64)
    rc = lib().sd_cpu_checksum_tree_shared(ls.ctypes.data if n else None, n, int(block_log2),
                                           nd.ctypes.data if m else None, int(min_blocks), rep.ctypes.data,
                                           size.ctypes.data, files.ctypes.data,
                                           pairs.ctypes.data if want_pairs else None, cap, ctypes.byref(n_pairs),
                                           stats.ctypes.data)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(n_pairs.value)
        e.stats = stats
        raise
    return rep[:m], size[:m], files[:n], pairs[:int(n_pairs.value) if want_pairs else 0], stats


class CdcParams(ctypes.Structure):
    """sd_cdc_params: mask_bits, min_size, max_size, reserved (include/sd_cas.h, content-defined chunks)."""
    _fields_ = [("mask_bits", ctypes.c_uint32), ("min_size", ctypes.c_uint32), ("max_size", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def cdc_params(params=None) -> CdcParams:
    """A CdcParams from None (the default 16 / 16 KiB / 256 KiB), a (mask_bits, min_size, max_size)
    tuple or a CdcParams."""
    from ._native import SD_CDC_DEFAULT
    if isinstance(params, CdcParams):
        return params
    mask_bits, min_size, max_size = SD_CDC_DEFAULT if params is None else params
    return CdcParams(int(mask_bits), int(min_size), int(max_size), 0)


def cdc_gear() -> np.ndarray:
    """sd_cdc_gear: the 256 gear values, uint64."""
    out = np.zeros(256, np.uint64)
    check(lib().sd_cdc_gear(out.ctypes.data))
    return out


def cdc_cut(data, offsets, lens, params=None, capacity: Optional[int] = None, want_chunks: bool = True,
            nthreads: int = THREADS):
    """sd_cpu_cdc_cut: the content-defined chunks of files that are byte ranges of a host buffer
    (16-byte aligned starts).  Returns (chunk_base uint64 [n + 1], chunks uint64 [m, 2] = (offset in
    the file, length) in layout order, stats uint64 [8]).  `capacity` (default: enough) short of the
    chunks raises SdCasError (SD_ERR_CAPACITY) with ``.needed``; want_chunks=False only counts."""
    from ._native import SdCasError
    buf = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    n = len(ls)
    if len(offs) != n:
        raise ValueError("offsets and lens differ in length")
    if n and int((offs + ls).max()) > buf.size:
        raise ValueError("a range ends past the buffer")
    pr = cdc_params(params)
    base = np.zeros(n + 1, np.uint64)
    stats = np.zeros(8, np.uint64)
    count = ctypes.c_uint64(0)

    def call(chunks, cap):
        return lib().sd_cpu_cdc_cut(buf.ctypes.data if buf.size else None, offs.ctypes.data if n else None,
                                    ls.ctypes.data if n else None, n, ctypes.byref(pr), base.ctypes.data,
                                    None if chunks is None else chunks.ctypes.data, cap, ctypes.byref(count),
                                    stats.ctypes.data, nthreads)
    if capacity is None:  # count first, then exactly enough
        check(call(None, 0))
        capacity = int(count.value)
    chunks = np.zeros((max(int(capacity), 1), 2), np.uint64)
    if want_chunks:
        try:
            check(call(chunks, int(capacity)))
        except SdCasError as e:
            e.needed = int(count.value)
            e.stats = stats
            raise
    else:
        check(call(None, 0))
    return base, chunks[:int(count.value) if want_chunks else 0], stats


def cdc_hash(data, offsets, lens, chunk_base, chunks, nthreads: int = THREADS) -> np.ndarray:
    """sd_cpu_cdc_hash: the ids uint8 [m, 32] of the chunks cdc_cut returned -- the BLAKE3 of each
    chunk's bytes, file_checksum of the chunk as a file."""
    buf = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    ls = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    base = np.ascontiguousarray(chunk_base, dtype=np.uint64).reshape(-1)
    ch = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)
    n = len(ls)
    if len(offs) != n or len(base) != n + 1 or len(ch) != (int(base[n]) if n else 0):
        raise ValueError("chunk_base is not [n + 1] or chunks is not chunk_base[n] rows")
    if n and int((offs + ls).max()) > buf.size:
        raise ValueError("a range ends past the buffer")
    ids = np.zeros((max(len(ch), 1), 32), np.uint8)
    check(lib().sd_cpu_cdc_hash(buf.ctypes.data if buf.size else None, offs.ctypes.data if n else None,
                                ls.ctypes.data if n else None, n, base.ctypes.data, ch.ctypes.data if len(ch) else None,
                                ids.ctypes.data, nthreads))
    return ids[:len(ch)]


def cdc_shared(chunk_base, chunks, ids, min_chunks: int = 0, capacity: Optional[int] = None, want_pairs: bool = True):
    """sd_cpu_cdc_shared: which chunks of a batch (cdc_cut's chunk_base and chunks, cdc_hash's ids)
    are there more than once, at any offset.  Returns (rep uint64 [m], class_size uint64 [m], files
    uint64 [n, 4], pairs uint64 [n_pairs, 4], stats uint64 [8]) as checksum_tree_shared does, with
    chunks for blocks; stats[7] counts the redundant chunks a file repeats of itself, which get no
    pair row."""
    from ._native import SdCasError
    base = np.ascontiguousarray(chunk_base, dtype=np.uint64).reshape(-1)
    n = max(len(base) - 1, 0)
    m = int(base[n]) if n else 0
    ch = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)
    hs = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1)
    if len(ch) != m or hs.size != 32 * m:
        raise ValueError("chunks or ids is not chunk_base[n] rows")
    rep, size = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
    files = np.zeros((max(n, 1), 4), np.uint64)
    cap = m if capacity is None else int(capacity)
    pairs = np.zeros((max(cap, 1), 4), np.uint64)
    n_pairs = ctypes.c_uint64(0)
    stats = np.zeros(8, np.uint64)
    rc = lib().sd_cpu_cdc_shared(base.ctypes.data if n else None, n, ch.ctypes.data if m else None,
                                 hs.ctypes.data if m else None, int(min_chunks), rep.ctypes.data, size.ctypes.data,
                                 files.ctypes.data, pairs.ctypes.data if want_pairs else None, cap,
                                 ctypes.byref(n_pairs), stats.ctypes.data)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(n_pairs.value)
        e.stats = stats
        raise
    return rep[:m], size[:m], files[:n], pairs[:int(n_pairs.value) if want_pairs else 0], stats


def _table(chunk_base, chunks, rep):
    base = np.ascontiguousarray(chunk_base, dtype=np.uint64).reshape(-1)
    n = max(len(base) - 1, 0)
    m = int(base[n]) if n else 0
    ch = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)
    rp = np.ascontiguousarray(rep, dtype=np.uint64).reshape(-1)
    if len(ch) != m or len(rp) != m:
        raise ValueError("chunks or rep is not chunk_base[n] rows")
    return base, n, m, ch, rp


def cdc_delta_plan(chunk_base, n_base: int, chunks, rep, capacity: Optional[int] = None, want_runs: bool = True):
    """sd_cpu_cdc_delta_plan: the recipe that rebuilds files n_base .. n-1 of a chunk table (cdc_cut's
    chunk_base and chunks, cdc_shared's rep) from files 0 .. n_base-1 and a literal buffer.  Returns
    (lit_off uint64 [target slots], runs uint64 [r, 4] = (t, source, src_off, bytes), files uint64
    [targets, 6], stats uint64 [8]); source 0 is the literal buffer, 1 + g base file g.  `capacity`
    (default: enough) short of the runs raises SdCasError (SD_ERR_CAPACITY, ``.needed``, ``.stats``)."""
    from ._native import SdCasError
    base, n, m, ch, rp = _table(chunk_base, chunks, rep)
    if not 0 <= int(n_base) <= n:
        raise ValueError("n_base outside 0..n")
    mt = m - (int(base[n_base]) if n else 0)
    nt = n - int(n_base)
    lit_off = np.zeros(max(mt, 1), np.uint64)
    files = np.zeros((max(nt, 1), 6), np.uint64)
    cap = mt if capacity is None else int(capacity)
    runs = np.zeros((max(cap, 1), 4), np.uint64)
    n_runs = ctypes.c_uint64(0)
    stats = np.zeros(8, np.uint64)
    rc = lib().sd_cpu_cdc_delta_plan(base.ctypes.data if n else None, n, int(n_base), ch.ctypes.data if m else None,
                                     rp.ctypes.data if m else None, lit_off.ctypes.data, runs.ctypes.data if want_runs else None,
                                     cap, ctypes.byref(n_runs), files.ctypes.data, stats.ctypes.data)
    try:
        check(rc)
    except SdCasError as e:
        e.needed = int(n_runs.value)
        e.stats = stats
        raise
    return lit_off[:mt], runs[:int(n_runs.value) if want_runs else 0], files[:nt], stats


def cdc_delta_pack(data, offsets, chunk_base, n_base: int, chunks, rep, lit_off, lit_bytes: int) -> np.ndarray:
    """sd_cpu_cdc_delta_pack: the literal buffer uint8 [lit_bytes] (stats[5] of the plan) -- the target
    files' literal chunks, each once, at their lit_off."""
    buf = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    base, n, m, ch, rp = _table(chunk_base, chunks, rep)
    lo = np.ascontiguousarray(lit_off, dtype=np.uint64).reshape(-1)
    if len(offs) != n or not 0 <= int(n_base) <= n or len(lo) != m - (int(base[n_base]) if n else 0):
        raise ValueError("offsets is not [n] or lit_off is not one per target slot")
    lit = np.zeros(max(int(lit_bytes), 1), np.uint8)
    check(lib().sd_cpu_cdc_delta_pack(base.ctypes.data if n else None, n, int(n_base), offs.ctypes.data if n else None,
                                      ch.ctypes.data if m else None, lo.ctypes.data if len(lo) else None,
                                      rp.ctypes.data if m else None, buf.ctypes.data if buf.size else None, lit.ctypes.data))
    return lit[:int(lit_bytes)]


def cdc_delta_apply(runs, base_data, base_offsets, base_lens, literals, out_lens, out=None, out_offsets=None,
                    nthreads: int = THREADS):
    """sd_cpu_cdc_delta_apply: rebuilds the targets from the base files (byte ranges of base_data) and
    the literal buffer.  The recipe is validated first; a refused one raises SdCasError
    (SD_ERR_INVALID) with nothing written.  Returns (out uint8, out_offsets uint64 [targets]): the
    targets packed back to back unless `out` and `out_offsets` are given."""
    rn = np.ascontiguousarray(runs, dtype=np.uint64).reshape(-1, 4)
    bd = np.ascontiguousarray(base_data, dtype=np.uint8).reshape(-1)
    bo = np.ascontiguousarray(base_offsets, dtype=np.uint64).reshape(-1)
    bl = np.ascontiguousarray(base_lens, dtype=np.uint64).reshape(-1)
    lit = np.ascontiguousarray(literals, dtype=np.uint8).reshape(-1)
    ol = np.ascontiguousarray(out_lens, dtype=np.uint64).reshape(-1)
    if len(bo) != len(bl):
        raise ValueError("base_offsets and base_lens differ in length")
    if len(bl) and int((bo + bl).max()) > bd.size:
        raise ValueError("a base range ends past the buffer")
    if out is None:
        oo = np.concatenate([[0], np.cumsum(ol)[:-1]]).astype(np.uint64) if len(ol) else np.zeros(0, np.uint64)
        out = np.zeros(max(int(ol.sum()) if len(ol) else 0, 1), np.uint8)
    else:
        oo = np.ascontiguousarray(out_offsets, dtype=np.uint64).reshape(-1)
        if out.dtype != np.uint8 or not out.flags.c_contiguous or len(oo) != len(ol):
            raise ValueError("out is not a contiguous uint8 array or out_offsets is not one per target")
        if len(ol) and int((oo + ol).max()) > out.size:
            raise ValueError("an output range ends past the buffer")
    check(lib().sd_cpu_cdc_delta_apply(rn.ctypes.data if len(rn) else None, len(rn), bo.ctypes.data if len(bl) else None,
                                       bl.ctypes.data if len(bl) else None, len(bl), bd.ctypes.data if bd.size else None,
                                       lit.ctypes.data if lit.size else None, lit.size, oo.ctypes.data if len(ol) else None,
                                       ol.ctypes.data if len(ol) else None, len(ol), out.ctypes.data, nthreads))
    return out, oo


def blake3(data: bytes) -> bytes:
    """Full 32-byte BLAKE3 of a host buffer (sd_cpu_checksums of one range)."""
    buf = np.frombuffer(bytes(data) + bytes(64), np.uint8)
    offs = np.zeros(1, np.uint64)
    lens = np.array([len(data)], np.uint64)
    out = np.zeros(32, np.uint8)
    check(lib().sd_cpu_checksums(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, 1, out.ctypes.data, 1))
    return out.tobytes()
