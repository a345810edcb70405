"""The hashing kernels keep the occupancy their timing rests on (CPU only; needs hipcc).

`make -C spacedrive_amd/csrc resource-usage` compiles cas_kernels.hip for gfx950 and prints what
the compiler allots each kernel.  For both instantiations (with and without the priority
windows) of the three kernels where the hashing time goes, no lane may spill to scratch and
the waves per SIMD may not fall under the figures recorded in
profiles/g_rotr16/resource_usage.md: a later edit that costs a register too many would
otherwise lose a wave without any test noticing.

The windowed instantiations of the same kernels also keep their half-rate ops inside the
priority windows: `make asm` lists the kernels, and walking a kernel's listing with the last
`s_setprio` seen, almost no v_add3_u32 / v_alignbit_b32 / SDWA xor may stand at priority 0.
With no inline asm in the windowed G only `sched_barrier` ties an op to its window, and that
binds the scheduler alone: the compiler once sank a whole compression (336 half-rate ops) out
of its windows.  The bound is 32: address and flag arithmetic outside G accounts for 0-16 such
ops per kernel, one escaped compression for 336.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled-name prefix -> waves/SIMD floor (profiles/g_rotr16/resource_usage.md); ILi8ELb1E = <8, true>
FLOORS = {
    "_Z19k_cas_sampled_lanesILi8ELb1E": 6,
    "_Z19k_cas_sampled_lanesILi8ELb0E": 5,
    "_Z13k_whole_itemsILb1E": 8,
    "_Z13k_whole_itemsILb0E": 8,
    "_Z9k_ck_leafILb1E": 5,
    "_Z9k_ck_leafILb0E": 5,
}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel name: {"VGPRs": n, "ScratchSize": n, "Occupancy": n, ...}} from one compile"""
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("hipcc not found")
    objdir = tmp_path_factory.mktemp("resource_usage")
    r = subprocess.run(["make", "-C", CSRC, "resource-usage", f"HIPCC={HIPCC}", f"OBJDIR={objdir}"],
                       capture_output=True, text=True)
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


@pytest.mark.parametrize("prefix", sorted(FLOORS))
def test_no_scratch_and_waves(usage, prefix):
    hits = [(n, u) for n, u in usage.items() if n.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {[n for n, _ in hits]} among {sorted(usage)}"
    name, u = hits[0]
    print(name, u)
    assert u["ScratchSize"] == 0, (name, u)
    assert u["Occupancy"] >= FLOORS[prefix], (name, u)


HALF_RATE = ("v_add3_u32", "v_alignbit_b32", "v_xor_b32_sdwa")
WINDOWED = [p for p in sorted(FLOORS) if p.endswith("Lb1E")]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    """{kernel name: [instruction lines]} of cas_kernels.hip's device code"""
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("hipcc not found")
    objdir = tmp_path_factory.mktemp("asm")
    r = subprocess.run(["make", "-C", CSRC, "asm", f"HIPCC={HIPCC}", f"OBJDIR={objdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out, name = {}, None
    for line in open(os.path.join(objdir, "cas_kernels.s")):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name:
            ins = line.split(";")[0].strip()
            if ins and not ins.startswith("."):
                out[name].append(ins)
    return out


@pytest.mark.parametrize("prefix", WINDOWED)
def test_half_rate_ops_stay_in_their_windows(listing, prefix):
    hits = [n for n in listing if n.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {hits}"
    prio, at = 0, [0, 0]
    for ins in listing[hits[0]]:
        op = ins.split()[0]
        if op == "s_setprio":
            prio = int(ins.split()[1])
        elif op.startswith(HALF_RATE):
            at[1 if prio else 0] += 1
    print(hits[0], "half-rate ops at priority 1 / 0:", at[1], "/", at[0])
    assert at[1] >= 336, at  # at least one windowed compression
    assert at[0] <= 32, at
