"""The proof kernels spill nothing (CPU only; needs hipcc): `make resource-usage-tree` compiles
checksum_tree.hip for gfx950 and prints what the compiler allots each kernel.  The interior-levels
kernel, the proof gather and the climb -- the flag skeleton instantiated with proof_climb, whose
lanes hold a chaining value, a sibling and a compression's state at once -- use no scratch, and the
interior-levels kernel keeps its LDS to the 256 nodes of a group
(profiles/checksum_proofs/resource_usage.md)."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import CSRC, HIPCC

KERNELS = ("k_tree_levels", "k_tree_proof_gather", "proof_climb")


@pytest.fixture(scope="module")
def tree_usage():
    """{kernel name: {"VGPRs": n, "ScratchSize": n, "Occupancy": n, "LDS Size": n}} from one compile"""
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("hipcc not found")
    r = subprocess.run(["make", "-C", CSRC, "resource-usage-tree", f"HIPCC={HIPCC}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"(VGPRs|ScratchSize|Occupancy|LDS Size)[^:]*: (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_proof_kernels_no_scratch(tree_usage, kernel):
    hits = [(n, u) for n, u in tree_usage.items() if kernel in n]
    assert len(hits) == 1, f"{kernel}: {[n for n, _ in hits]}"
    name, u = hits[0]
    print(name, u)
    assert u["ScratchSize"] == 0, (name, u)
    if kernel == "k_tree_levels":
        assert u["LDS Size"] == 256 * 32, (name, u)
