"""k_ck_blocks keeps what its timing rests on (CPU only; needs hipcc): tests/test_kernel_resources.py's
two checks for both instantiations of the listed-blocks kernel -- no lane spills to scratch, 5 waves
per SIMD as the leaf kernel it shares its lanes with (profiles/checksum_blocks/resource_usage.md) --
and the windowed one keeps its half-rate ops inside the priority windows.  The fixtures are that
file's: one `make resource-usage` and one `make asm` for this module."""
import pytest

from tests.test_kernel_resources import HALF_RATE, listing, usage  # noqa: F401  (fixtures)

BLOCKS = {"_Z11k_ck_blocksILb1E": 5, "_Z11k_ck_blocksILb0E": 5}  # mangled-name prefix -> waves/SIMD floor


@pytest.mark.parametrize("prefix", sorted(BLOCKS))
def test_blocks_kernel_no_scratch_and_waves(usage, prefix):  # noqa: F811
    hits = [(n, u) for n, u in usage.items() if n.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {[n for n, _ in hits]} among {sorted(usage)}"
    name, u = hits[0]
    print(name, u)
    assert u["ScratchSize"] == 0, (name, u)
    assert u["Occupancy"] >= BLOCKS[prefix], (name, u)


def test_blocks_kernel_half_rate_ops_stay_in_their_windows(listing):  # noqa: F811
    hits = [n for n in listing if n.startswith("_Z11k_ck_blocksILb1E")]
    assert len(hits) == 1, hits
    prio, at = 0, [0, 0]
    for ins in listing[hits[0]]:
        op = ins.split()[0]
        if op == "s_setprio":
            prio = int(ins.split()[1])
        elif op.startswith(HALF_RATE):
            at[1 if prio else 0] += 1
    print(hits[0], "half-rate ops at priority 1 / 0:", at[1], "/", at[0])
    assert at[1] >= 336, at  # at least one windowed compression
    assert at[0] <= 32, at   # the bound of tests/test_kernel_resources.py: one escaped compression is 336
