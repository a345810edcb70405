"""The slice arithmetic of a sliced pass (spacedrive_amd/csrc/sliced.h), stated once for the
cases of the Object index and of the confirm step: a fixed grid of at most BLOCKS workgroups,
workgroup b owning slice b of the input in whole tiles of TILE positions.
tests/test_dedup_confirm.py pins the two constants to the header.

Nothing here touches a device or the library.
"""
from __future__ import annotations

TILE = 256      # sliced.h TILE: the positions of a workgroup's tile
BLOCKS = 1024   # sliced.h BLOCKS: most workgroups of a sliced pass
# where the arithmetic changes: one position, the last lane of a tile, a whole tile, one position
# into the second workgroup, every workgroup one whole tile, and one more, at which a workgroup's
# slice goes from one tile to two
SLICE_COUNTS = (1, TILE - 1, TILE, TILE + 1, BLOCKS * TILE, BLOCKS * TILE + 1)


def grid(n: int) -> int:
    """the workgroups of a sliced pass over n positions, as sliced_grid computes them"""
    return min(max((n + TILE - 1) // TILE, 1), BLOCKS)


def slice_len(n: int) -> int:
    """the positions of one workgroup's slice in a sliced pass over n, as slice_of computes it:
    whole tiles"""
    g = grid(n)
    return ((n + g - 1) // g + TILE - 1) // TILE * TILE
