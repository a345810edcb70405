"""The slice arithmetic of the Object index's sliced passes (csrc/sliced.h: sliced_flag,
sliced_compact and the primitives under them) at the entry counts where it changes
(tests/sliced_cases.py) -- run on an MI355X: -m gpu.
A sliced pass gives each of at most 1024 workgroups a contiguous run of whole 256-entry tiles:
one entry, the last lane of a tile (255), a whole tile (256), one entry into the second
workgroup (257), every workgroup one whole tile (262 144), and one entry more, at which a
workgroup's slice goes from one tile to two.  At each count one owners-mode index goes through
every family of sliced passes (insert, removal with ids in place and compacting, apply, the
orphans, the duplicate groups), bit-exact against the numpy mirrors of spacedrive_amd/dedup.py
behind tests/test_object_index_duplicates.py's MirrorDuplicates.  The device index writes every
output between guard rows (tests/test_gpu_object_index_duplicates.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import object_index_apply_cases as ac  # noqa: E402
from tests import object_index_owners_cases as wc  # noqa: E402
from tests.sliced_cases import BLOCKS, SLICE_COUNTS, TILE, grid, slice_len  # noqa: E402
from tests.test_gpu_object_index_duplicates import DeviceDuplicates  # noqa: E402
from tests.test_object_index_apply import exports_equal, same  # noqa: E402
from tests.test_object_index_duplicates import MirrorDuplicates  # noqa: E402

U = np.uint64
E = ac.E


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


def test_the_counts_are_where_the_slices_change():
    """a workgroup's slice, as slice_of computes it: whole tiles of ceil(n / workgroups)"""
    assert [slice_len(n) // TILE for n in SLICE_COUNTS] == [1, 1, 1, 1, 1, 2]
    assert all(slice_len(n) % TILE == 0 for n in SLICE_COUNTS)
    assert [grid(n) for n in SLICE_COUNTS] == [1, 1, 1, 2, BLOCKS, BLOCKS]


@pytest.mark.parametrize("n", SLICE_COUNTS)
def test_every_sliced_pass_at_a_slice_border(ctx, n):
    k, v = wc.shaped_pairs(n)
    o = np.lexsort((v, k))
    third = k[o][::3].copy(), v[o][::3].copy()      # every third entry, in the index's order
    back = third[0][::3].copy(), third[1][::3].copy()
    x, m = DeviceDuplicates(ctx), MirrorDuplicates()
    try:
        def both(op, *args):
            got, want = getattr(x, op)(*args), getattr(m, op)(*args)
            assert same(got, want), (n, op)
            assert exports_equal(m, x), (n, op)
            return want
        # 2n pairs, every pair twice: n entries of two links
        assert both("insert", np.concatenate([k, k]), np.concatenate([v, v])) == n == len(x)
        assert (m.export_links()[2] == 2).all()
        # one link goes from every third entry: nothing leaves, the links change in place
        assert both("remove", *third)[1] == 0 and len(x) == n
        # and the other: those entries leave, the survivors close up
        assert both("remove", *third)[1] == len(third[0]) and len(x) == n - len(third[0])
        # one apply puts a third of them back
        assert both("apply", E, E, *back)[1:] == (0, len(back[0])) and len(x) == n - len(third[0]) + len(back[0])
        # the orphans among all ids, repeats included
        gone = both("orphans", v)
        assert np.array_equal(gone, np.setdiff1d(v, m.export_links()[1]))
        # the groups of at least two links
        rows = both("duplicates", 2, 0)
        assert (rows[2] >= 2).all()
    finally:
        x.close()
