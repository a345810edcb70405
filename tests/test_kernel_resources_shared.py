"""The shared-blocks kernels spill nothing (CPU only; needs hipcc): `make resource-usage-shared`
compiles tree_shared.hip for gfx950 and prints what the compiler allots each kernel.  The slot map,
the per-slot and per-file sums, the row writer and the five instantiations of the sliced skeletons
(redundant slots, their records, run heads, head positions, long runs) use no scratch
(profiles/tree_shared/resource_usage.md).  Reads the compiler's resource summary only."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import CSRC, HIPCC

KERNELS = ("k_ts_map", "k_ts_slots", "k_ts_files", "k_ts_rows", "ts_redundant", "ts_records", "ts_head_pos",
           "ts_long_run")


@pytest.fixture(scope="module")
def shared_usage():
    """{kernel name: {"VGPRs": n, "ScratchSize": n, "Occupancy": n, "LDS Size": n}} from one compile"""
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("hipcc not found")
    r = subprocess.run(["make", "-C", CSRC, "resource-usage-shared", f"HIPCC={HIPCC}"], capture_output=True, text=True)
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
def test_shared_kernels_no_scratch(shared_usage, kernel):
    hits = [(n, u) for n, u in shared_usage.items() if kernel in n]
    assert len(hits) == 1, f"{kernel}: {[n for n, _ in hits]}"
    name, u = hits[0]
    print(name, u)
    assert u["ScratchSize"] == 0, (name, u)


def test_the_flagged_run_heads_no_scratch(shared_usage):
    """ts_head is a prefix of ts_head_pos: the flag skeleton over ts_head is the one hit that is not
    the compaction"""
    hits = [(n, u) for n, u in shared_usage.items() if "ts_head" in n and "ts_head_pos" not in n]
    assert len(hits) == 1, [n for n, _ in hits]
    assert hits[0][1]["ScratchSize"] == 0, hits[0]
