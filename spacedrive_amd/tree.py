"""Checksum trees of files (include/sd_cas.h, checksum trees): a file's checksum together with
its level -- one 32-byte BLAKE3 node per 2^block_log2-byte block -- so a later scrub says WHICH
blocks changed (validator_job.rs:138-141), and a sender which to resend (spaceblock's 128 KiB
blocks, p2p/src/spaceblock/block_size.rs:20-23).

Files are read as file_checksum reads them (validation/hash.rs:10-24: 1 MiB reads until a short
one) and hashed by the library's CPU path, the route it prefers for files in the page cache
(DESIGN.md §4.1).  For files already resident on the device: ``Context.checksum_tree``.

verify_blocks_file and update_file take a list of blocks and read only those (os.pread): blocks as
they arrive, the blocks a sender resent, the blocks a write in place touched; blocks_to_rehash
lists the ones an append or a truncation costs.  On the device: ``Context.checksum_tree_blocks``.

prove_blocks and verify_proofs_file are the pair for a receiver that keeps no level, only the
checksum and the length of the library's database: the sender packs each block's siblings on its
way up the tree, the receiver climbs them back to the checksum (include/sd_cas.h, block proofs).
prove_range and verify_range_file do the same for a contiguous run of blocks, a resumed or partial
transfer: only the run's two flanks travel (include/sd_cas.h, range proofs).

shared_blocks compares the levels of several files with each other, and compare_files does so for
files on disk: which blocks a file repeats of an earlier one, block for block where they lie --
what to ask about files the confirm step refuted (include/sd_cas.h, shared blocks).  On the device:
``Context.checksum_tree_shared``.
"""
from __future__ import annotations

import os
from typing import List, Tuple, Union

import numpy as np

from . import cpu

READ_LEN = 1 << 20  # hash.rs:8 BLOCK_LEN


def _read(path: Union[str, os.PathLike]) -> np.ndarray:
    """hash.rs:14-20: read 1 MiB at a time until a read returns fewer bytes"""
    parts = []
    with open(path, "rb", buffering=0) as f:
        while True:
            b = f.read(READ_LEN)
            parts.append(b)
            if len(b) != READ_LEN:
                break
    return np.frombuffer(b"".join(parts), np.uint8)


def file_checksum_tree(path: Union[str, os.PathLike], block_log2: int = 17,
                       nthreads: int = cpu.THREADS) -> Tuple[str, int, np.ndarray]:
    """(hex, length, nodes): file_checksum's 64 hex digits, the bytes hashed, and the file's level
    uint8 [nb, 32].  Store (length, block_log2, nodes) beside the checksum."""
    data = _read(path)
    nodes, roots, _ = cpu.checksum_tree(data, [0], [len(data)], block_log2, nthreads)
    return roots[0].tobytes().hex(), len(data), nodes


def verify_file(path: Union[str, os.PathLike], length: int, nodes, block_log2: int = 17,
                nthreads: int = cpu.THREADS) -> List[int]:
    """The blocks of `path` whose node differs from `nodes` (a level file_checksum_tree returned for
    a file of `length` bytes), ascending; [] when the file still matches.  Raises ValueError when
    the file no longer holds `length` bytes: its blocks then compare only where common_blocks says."""
    data = _read(path)
    if len(data) != length:
        raise ValueError(f"{os.fsdecode(path)}: {len(data)} bytes, the level was taken over {length}")
    rows, _ = cpu.checksum_tree_verify(data, [0], [length], nodes, block_log2, nthreads=nthreads)
    return [int(b) for b in rows[:, 1]]


def _read_blocks(path, length: int, blocks, block_log2: int):
    """(buffer, rows [m, 2], offsets [m]): the listed blocks of a file of `length` bytes, each read
    with one os.pread into a buffer of 64-byte aligned starts -- nothing else of the file is read"""
    B = 1 << block_log2
    nb = cpu.tree_nodes(length, block_log2)
    blocks = [int(j) for j in blocks]
    if any(j < 0 or j >= nb for j in blocks):
        raise ValueError(f"a file of {length} bytes has blocks 0 .. {nb - 1}")
    sizes = [max(0, min(B, length - j * B)) for j in blocks]
    offs = np.zeros(len(blocks), np.uint64)
    cur = 0
    for r, size in enumerate(sizes):
        offs[r] = cur
        cur += (size + 63) // 64 * 64 + 64
    buf = np.zeros(cur + 64, np.uint8)
    fd = os.open(path, os.O_RDONLY)
    try:
        for j, size, o in zip(blocks, sizes, offs):
            got, o = 0, int(o)
            while got < size:
                part = os.pread(fd, size - got, j * B + got)
                if not part:
                    raise ValueError(f"{os.fsdecode(path)}: block {j} ends before byte {j * B + size}")
                buf[o + got:o + got + len(part)] = np.frombuffer(part, np.uint8)
                got += len(part)
    finally:
        os.close(fd)
    rows = np.array([[0, j] for j in blocks], np.uint64).reshape(-1, 2)
    return buf, rows, offs


def verify_blocks_file(path: Union[str, os.PathLike], length: int, nodes, blocks, block_log2: int = 17,
                       nthreads: int = cpu.THREADS) -> List[int]:
    """The listed blocks of `path` (a file of `length` bytes) whose node differs from `nodes` (its
    level), in list order; [] when they all match.  Reads only those blocks: blocks as they arrive,
    or the ones a sender resent after verify_file named them."""
    buf, rows, offs = _read_blocks(path, length, blocks, block_log2)
    bad, _ = cpu.checksum_tree_blocks_verify(buf, [length], rows, offs, nodes, block_log2, nthreads=nthreads)
    return [int(b) for b in bad[:, 1]]


def update_file(path: Union[str, os.PathLike], length: int, nodes, blocks, block_log2: int = 17,
                nthreads: int = cpu.THREADS) -> Tuple[str, np.ndarray]:
    """(hex, nodes) of `path`, now `length` bytes, after a change that touched only `blocks`: the
    level `nodes` taken before the change with those blocks' nodes replaced, and file_checksum's 64
    hex digits from it.  Reads only the listed blocks.  After a write in place `blocks` are the
    blocks written; after an append or a truncation they are blocks_to_rehash(old length, length),
    and the level is cut or grown to the new block count first (every block it gains has to be
    listed)."""
    nb = cpu.tree_nodes(length, block_log2)
    old = np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1, 32)
    listed = {int(j) for j in blocks}
    if any(j not in listed for j in range(len(old), nb)):
        raise ValueError("a block past the old level's end is not listed")
    level = np.zeros((nb, 32), np.uint8)
    level[:min(nb, len(old))] = old[:nb]
    if not listed:  # an empty list is a no-op of the library: the root of the level as it stands
        return cpu.checksum_tree_roots(level, [length], block_log2)[0].tobytes().hex(), level
    buf, rows, offs = _read_blocks(path, length, blocks, block_log2)
    level, roots = cpu.checksum_tree_blocks_update(buf, [length], rows, offs, level, block_log2, nthreads)
    return roots[0].tobytes().hex(), level


def prove_blocks(nodes, length: int, blocks, block_log2: int = 17) -> bytes:
    """The packed proofs of the listed blocks of a file of `length` bytes, from its level `nodes`
    (uint8 [nb, 32]), in list order: what a sender answers a block request with beside the block's
    bytes.  Block j's proof is cpu.tree_proof_entries(length, j, block_log2) entries of 32 bytes."""
    nb = cpu.tree_nodes(length, block_log2)
    blocks = [int(j) for j in blocks]
    if any(j < 0 or j >= nb for j in blocks):
        raise ValueError(f"a file of {length} bytes has blocks 0 .. {nb - 1}")
    rows = np.array([[0, j] for j in blocks], np.uint64).reshape(-1, 2)
    proofs, _ = cpu.checksum_tree_blocks_prove(nodes, [length], rows, block_log2)
    return proofs.tobytes()


def verify_proofs_file(path: Union[str, os.PathLike], length: int, checksum, blocks, proofs, block_log2: int = 17,
                       nthreads: int = cpu.THREADS) -> List[int]:
    """The listed blocks of `path` that their proofs (prove_blocks' bytes, list order) do not carry
    to `checksum` (64 hex digits or 32 bytes) for a file of `length` bytes, in list order; [] when
    every block belongs to that checksum.  The checksum and the length are all the receiver trusts;
    only the listed blocks are read."""
    root = bytes.fromhex(checksum) if isinstance(checksum, str) else bytes(checksum)
    if len(root) != 32:
        raise ValueError("a checksum is 32 bytes")
    buf, rows, offs = _read_blocks(path, length, blocks, block_log2)
    bad, _ = cpu.checksum_tree_blocks_verify_proofs(buf, [length], rows, offs, np.frombuffer(bytes(proofs), np.uint8),
                                                    np.frombuffer(root, np.uint8), block_log2, nthreads=nthreads)
    return [int(b) for b in bad[:, 1]]


def _range_rows(length: int, first: int, count: int, block_log2: int) -> List[int]:
    nb = cpu.tree_nodes(length, block_log2)
    first, count = int(first), int(count)
    if first < 0 or count < 1 or first + count > nb:
        raise ValueError(f"a file of {length} bytes has blocks 0 .. {nb - 1}")
    return list(range(first, first + count))


def prove_range(nodes, length: int, first: int, count: int, block_log2: int = 17) -> bytes:
    """The proof of blocks [first, first + count) of a file of `length` bytes, from its level `nodes`
    (uint8 [nb, 32]): what a sender answers a partial request (spaceblock's Range::Partial) with
    beside the bytes.  Only the run's two flanks travel, cpu.tree_range_proof_entries(length, first,
    count, block_log2) entries of 32 bytes -- at most two per level, however long the run."""
    blocks = _range_rows(length, first, count, block_log2)
    rows = np.array([[0, j] for j in blocks], np.uint64).reshape(-1, 2)
    proofs, _ = cpu.checksum_tree_blocks_prove_ranges(nodes, [length], rows, [0, len(blocks)], block_log2)
    return proofs.tobytes()


def verify_range_file(path: Union[str, os.PathLike], length: int, checksum, first: int, count: int, proof,
                      block_log2: int = 17, nthreads: int = cpu.THREADS) -> bool:
    """Whether blocks [first, first + count) of `path`, climbed through `proof` (prove_range's
    bytes), reach `checksum` (64 hex digits or 32 bytes) for a file of `length` bytes.  The checksum
    and the length are all the receiver trusts; only the range is read.  False says a byte of these
    blocks or an entry of the proof is wrong, not which block: verify_proofs_file names blocks."""
    root = bytes.fromhex(checksum) if isinstance(checksum, str) else bytes(checksum)
    if len(root) != 32:
        raise ValueError("a checksum is 32 bytes")
    blocks = _range_rows(length, first, count, block_log2)
    buf, rows, offs = _read_blocks(path, length, blocks, block_log2)
    bad, _ = cpu.checksum_tree_blocks_verify_range_proofs(buf, [length], rows, offs, [0, len(blocks)],
                                                          np.frombuffer(bytes(proof), np.uint8),
                                                          np.frombuffer(root, np.uint8), block_log2, nthreads=nthreads)
    return len(bad) == 0


def shared_blocks(levels, block_log2: int = 17, min_blocks: int = 0):
    """Which blocks of these files are there more than once (include/sd_cas.h, shared blocks).
    `levels` is a list of (length, nodes) as file_checksum_tree returns them.  Returns (files, pairs,
    stats): files uint64 [n, 4] = (blocks, shared, redundant, redundant bytes) per file; pairs uint64
    [p, 4] = (f, g, blocks, bytes), one row per pair g < f of which g is the FIRST holder of at least
    max(1, min_blocks) blocks of f, ascending by (f, g); stats uint64 [8].  Blocks are compared where
    they lie: aligned blocks only, shifted content is not found.  No file is read."""
    lens = [int(length) for length, _ in levels]
    parts = [np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1, 32) for _, nodes in levels]
    for length, part in zip(lens, parts):
        if len(part) != cpu.tree_nodes(length, block_log2):
            raise ValueError(f"a file of {length} bytes has {cpu.tree_nodes(length, block_log2)} nodes")
    nodes = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    _, _, files, pairs, stats = cpu.checksum_tree_shared(lens, nodes, block_log2, min_blocks)
    return files, pairs, stats


def compare_files(paths, block_log2: int = 17, nthreads: int = cpu.THREADS):
    """shared_blocks of the files at `paths`, each read and hashed once (file_checksum_tree): what to
    ask about files the confirm step refuted -- do they differ in one block or in all of them?
    Returns (checksums, files, pairs, stats), the checksums as 64 hex digits per path."""
    trees = [file_checksum_tree(p, block_log2, nthreads) for p in paths]
    files, pairs, stats = shared_blocks([(length, nodes) for _, length, nodes in trees], block_log2)
    return [hexsum for hexsum, _, _ in trees], files, pairs, stats


def blocks_to_rehash(len_old: int, len_new: int, block_log2: int) -> List[int]:
    """The blocks of a file that went from len_old to len_new bytes whose old nodes cannot be kept
    even if no byte before min(len_old, len_new) changed: the complement of common_blocks among the
    new file's blocks.  Every block when either length is a single block (its node is or was a root
    hash), else the blocks from min(len_old, len_new) // B on."""
    if block_log2 < 10:
        raise ValueError("a block is at least one 1024-byte chunk")
    B = 1 << block_log2
    nb_new = max(1, -(-len_new // B))
    if min(len_old, len_new) <= B:
        return list(range(nb_new))
    return list(range(min(len_old, len_new) // B, nb_new))


def common_blocks(len_a: int, len_b: int, block_log2: int) -> List[int]:
    """The block indices whose nodes of two files' levels are comparable: the block is full in both
    files and neither file is a single block (whose node is its root hash, not a chaining value).
    Equal nodes there mean equal bytes; every other block has to be hashed again.  Pure arithmetic
    in the block size (any block_log2 >= 10, the chunk)."""
    if block_log2 < 10:
        raise ValueError("a block is at least one 1024-byte chunk")
    B = 1 << block_log2
    if min(len_a, len_b) <= B:  # a single block: its node is the file's root hash
        return []
    return list(range(min(len_a, len_b) // B))
