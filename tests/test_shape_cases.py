"""The shape sweeps of tests/shape_cases.py without a device: the generators' own counts,
the library's CPU path (the staged and range entry points of spacedrive_amd/cpu.py) and the
Python spec against the C oracle at those shapes, and the host mirror of
sd_dedup_partition at the extremes of its key range.  tests/test_gpu_shapes.py runs the
same lists through the kernels."""
import numpy as np

from oracle import cas_spec as cs
from spacedrive_amd import cpu
from spacedrive_amd._native import check, lib
from spacedrive_amd.dedup import dest_of, partition_host
from spacedrive_amd.device import stage_plan
from tests import shape_cases as sc

NT = 8


def cpu_checksums(data: np.ndarray, offs, lens, nthreads: int = NT) -> np.ndarray:
    """sd_cpu_checksums: the full BLAKE3 of byte ranges of one host buffer."""
    offs = np.ascontiguousarray(offs, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint64)
    out = np.zeros((len(lens), 32), np.uint8)
    check(lib().sd_cpu_checksums(data.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(lens), out.ctypes.data,
                                 nthreads))
    return out


def test_generators_count_their_cases():
    assert len(sc.sweep_a()) == 700 and len(sc.sweep_a_small()) == 62
    b = sc.sweep_b_block()
    assert len(b) == 1024 + 4 * 27
    for C in range(1, 1025):  # one entry per C, four more per all-r class member
        assert sum(1 for c in b if c[0] == C) == (5 if C in sc.SWEEP_B_ALL_R else 1), C
    assert len(sc.sweep_b_stride()) == 162
    assert len(sc.sweep_b_pairs()) == 4 and len(sc.sweep_b_last_blocks()) == 36 and len(sc.sweep_b_reduce()) == 20
    offs, lens, total = sc.packed_ranges()
    assert total == int(offs[-1] + lens[-1]) + 64
    assert sc.range_mask(offs, lens, total).sum() == int(lens.sum())  # no two ranges overlap
    for nparts in sc.PART_NPARTS:
        assert len(sc.partition_cases(nparts)) == 96


def test_sweep_a_cpu_path_vs_oracle(oracle_native):
    """Every whole-file tree shape through sd_cpu_cas_ids (staged messages) and
    sd_cpu_checksums (the same messages as byte ranges), shuffled: the cas_ids and all 32
    hash bytes against the C oracle."""
    cases = sc.sweep_a()
    sizes, cids, twins = sc.cas_files(cases)
    perm = np.random.default_rng(21).permutation(len(cases))
    sizes, cids, twins = sizes[perm], cids[perm], twins[perm]
    ext, total = stage_plan(sizes)
    assert ext["msg_len"].tolist() == [cases[i][2] for i in perm]
    buf = oracle_native.stage_synth(sizes, cids, twins, ext["msg_offset"], total)
    want = oracle_native.checksums(buf, ext["msg_offset"], ext["msg_len"].astype(np.uint64), nthreads=NT)
    ids = oracle_native.cas_ids_synth(sizes, cids, twins, nthreads=NT)
    assert np.array_equal(want[:, :8], ids)
    got_ids = cpu.cas_ids_staged(buf, ext, nthreads=NT)
    bad = [cases[perm[i]] for i in range(len(cases)) if got_ids[i] != ids[i].tobytes().hex()]
    assert not bad, bad[:10]
    got = cpu_checksums(buf, ext["msg_offset"], ext["msg_len"])
    mism = np.nonzero((got != want).any(axis=1))[0]
    assert len(mism) == 0, [cases[perm[i]] for i in mism[:10]]
    assert len(got_ids) == len(got) == sc.SWEEP_A_COUNT


def test_sweep_b_stride_cpu_path_vs_oracle(oracle_native):
    """A stride of the one-block checksum sweep through sd_cpu_checksums, packed at odd
    16-byte starts, against the C oracle's checksums of the same synthetic contents."""
    cases = sc.sweep_b_stride()
    lens = [L for _, _, L in cases]
    cids = np.arange(20000, 20000 + len(cases), dtype=np.uint64)
    twins = (np.arange(len(cases)) % 3).astype(np.uint32)
    offs, total = sc.place(lens, align=16, gap=0)
    buf = np.zeros(total, np.uint8)
    for o, L, c, t in zip(offs, lens, cids, twins):
        buf[o:o + L] = np.frombuffer(oracle_native.synth_bytes(int(c), int(t), 0, L), np.uint8)
    want = oracle_native.checksums_synth(np.array(lens, np.uint64), cids, twins, nthreads=NT)
    got = cpu_checksums(buf, offs, lens)
    mism = np.nonzero((got != want).any(axis=1))[0]
    assert len(mism) == 0, [cases[i] for i in mism[:10]]
    assert len(got) == 162


def test_sweep_a_small_python_spec_pins_oracle(oracle_native):
    """The C <= 9 messages through the Python spec (oracle.cas_spec over oracle.blake3_spec):
    the C oracle the GPU tests compare with is itself right at these lengths."""
    cases = sc.sweep_a_small()
    sizes, cids, twins = sc.cas_files(cases)
    ids = oracle_native.cas_ids_synth(sizes, cids, twins, nthreads=NT)
    n = 0
    for i, (C, r, L) in enumerate(cases):
        assert cs.generate_cas_id(cs.synth_reader(int(cids[i])), int(sizes[i])) == ids[i].tobytes().hex(), (C, r)
        n += 1
    assert n == 62


def test_partition_host_vs_python_loop():
    """partition_host (the GPU tests' expected value) against a plain loop over Python
    integers, on the crafted keys: 0, 2^64 - 1 and one either side of every boundary."""
    n_keys = 0
    for nparts in sc.PART_NPARTS:
        keys = sc.crafted_keys(nparts)
        want = [[] for _ in range(nparts)]
        for i, k in enumerate(keys):
            assert 0 <= sc.dest_of_int(k, nparts) < nparts
            want[sc.dest_of_int(k, nparts)].append((k, i + 5))
        ka = np.array(keys, np.uint64)
        assert dest_of(ka, nparts).tolist() == [sc.dest_of_int(k, nparts) for k in keys]
        recs, counts = partition_host(ka, np.arange(len(keys), dtype=np.int64) + 5, nparts)
        assert counts.tolist() == [len(w) for w in want]
        flat = [kv for w in want for kv in w]
        assert recs[:, 0].view(np.uint64).tolist() == [k for k, _ in flat]
        assert recs[:, 1].tolist() == [i for _, i in flat]
        # the boundaries themselves: key floor(k 2^64 / nparts) opens destination k or closes k - 1
        for k in range(1, nparts):
            edge = (k << 64) // nparts
            assert sc.dest_of_int(edge, nparts) in (k - 1, k) and sc.dest_of_int(edge - 1, nparts) in (k - 1, k)
        n_keys += len(keys)
    assert n_keys == sum(6 + 3 * p for p in sc.PART_NPARTS)
