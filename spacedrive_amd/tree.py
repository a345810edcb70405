"""Checksum trees of files (include/sd_cas.h, checksum trees): a file's checksum together with
its level -- one 32-byte BLAKE3 node per 2^block_log2-byte block -- so a later scrub says WHICH
blocks changed (validator_job.rs:138-141), and a sender which to resend (spaceblock's 128 KiB
blocks, p2p/src/spaceblock/block_size.rs:20-23).

Files are read as file_checksum reads them (validation/hash.rs:10-24: 1 MiB reads until a short
one) and hashed by the library's CPU path, the route it prefers for files in the page cache
(DESIGN.md §4.1).  For files already resident on the device: ``Context.checksum_tree``.
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
