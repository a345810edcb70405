"""The range-proof kernels spill nothing (CPU only; needs hipcc): `make resource-usage-tree` compiles
checksum_tree.hip for gfx950 and prints what the compiler allots each kernel.  The range climb, the
range gather and the two sliced passes of the range verify (range_differs, range_rows) use no
scratch, and the climb keeps its LDS to the 256 nodes of a group
(profiles/checksum_ranges/resource_usage.md)."""
import pytest

from tests.test_kernel_resources_proofs import tree_usage  # noqa: F401

KERNELS = ("k_tree_range_climb", "k_tree_range_gather", "range_differs", "range_rows")


@pytest.mark.parametrize("kernel", KERNELS)
def test_range_kernels_no_scratch(tree_usage, kernel):  # noqa: F811
    hits = [(n, u) for n, u in tree_usage.items() if kernel in n]
    assert len(hits) == 1, f"{kernel}: {[n for n, _ in hits]}"
    name, u = hits[0]
    print(name, u)
    assert u["ScratchSize"] == 0, (name, u)
    if kernel == "k_tree_range_climb":
        assert u["LDS Size"] == 256 * 32, (name, u)
