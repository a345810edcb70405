"""The shape sweeps of tests/shape_cases.py without a device: the generators' own counts,
the library's CPU path (the staged and range entry points of spacedrive_amd/cpu.py) and the
Python spec against the C oracle at those shapes, the host mirror of
sd_dedup_partition at the extremes of its key range, and the bucket-size cases of
sd_dedup_group: their own assertions, group_host against a brute-force grouping, and the
bucket constants against dedup.hip.  tests/test_gpu_shapes.py runs the same lists through
the kernels."""
import os
import re

import numpy as np

from oracle import cas_spec as cs
from spacedrive_amd import cpu
from spacedrive_amd._native import check, lib
from spacedrive_amd.dedup import dest_of, group_host, partition_host
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


def test_bucket_generators_count_their_cases():
    """Every list of section D2 built once: each generator asserts, through the numpy mirror of
    the bucket arithmetic, the bucket sizes it exists for."""
    n = 0
    for layout in sc.BUCKET_LAYOUTS:
        cases = sc.bucket_cases(layout)
        assert all(len(r) == s + 202 for s, _, r in cases)
        n += len(cases)
    assert n == 2 * 126
    assert len(sc.many_big_case()) == 130 * 129 + 2 and len(sc.many_big_case(True)) == 130 * 129 + 2
    assert len(sc.all_big_case()) == 64 * 129 and len(sc.all_big_case(True)) == 64 * 129
    assert len(sc.span_cases()) == 45 and len(sc.lg_border_cases()) == 6
    assert [sc.gb_lg(m) for m in (1, 96, 97, 192, 193, 1000, 48 << 23, (48 << 23) + 1, 1 << 40)] == [1, 1, 2, 2, 3, 5, 23, 24, 24]
    # the mirror on keys a hand can follow: span 2^32 at m = 97 (lg 2) shifts by 33 - 2
    bk, (lg, shift) = sc.gb_buckets(np.array([5] * 95 + [5 + (1 << 32), 5 + (1 << 31)], np.uint64))
    assert (lg, shift) == (2, 31) and bk.tolist() == [0] * 95 + [2, 1]


def brute_group(recs: np.ndarray):
    """sd_dedup_group's rule with no sort network and no scan: a dict from key to its smallest
    index, and Python's sort of (key, index) tuples -- all as unsigned Python integers."""
    pairs = [(int(k), int(i)) for k, i in zip(recs[:, 0].view(np.uint64), recs[:, 1].view(np.uint64))]
    least = {}
    for k, i in pairs:
        least[k] = min(i, least.get(k, i))
    pairs.sort()
    return pairs, [least[k] for k, _ in pairs], len(least)


def test_group_host_vs_brute_force():
    """group_host (the GPU sweeps' expected value) against brute_group at the one-wave LDS size
    and past a 1024-lane chunk, for the layouts with a head off position 0."""
    n = 0
    for s in (65, 1025):
        for layout in ("singles", "late", "pairs_shifted"):
            for srt in (False, True):
                recs = sc.bucket_case(s, layout, srt)
                gr, grep, gng = group_host(recs)
                pairs, reps, ng = brute_group(recs)
                assert gng == ng
                assert list(zip(gr[:, 0].view(np.uint64).tolist(), gr[:, 1].tolist())) == pairs
                assert grep.tolist() == reps
                # the records that are not their group's representative
                assert (grep != gr[:, 1]).sum() == {"singles": 0, "late": s - 2, "pairs_shifted": (s - 1) // 2}[layout]
                n += 1
    assert n == 12


def parse_gb_constants(path: str) -> dict:
    """GB_CAP, GB_BIG_CAP and GB_BIG_GRID from their constexpr lines, and the records per bucket
    and the lg cap from gb_lg's loop, of a dedup.hip."""
    src = open(path).read()
    out = {}
    for name in ("GB_CAP", "GB_BIG_CAP", "GB_BIG_GRID"):
        found = re.findall(r"^constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", src, re.M)
        assert len(found) == 1, name
        out[name] = int(found[0])
    body = re.search(r"static\s+uint32_t\s+gb_lg\(uint64_t m\)\s*\{(.*?)\n\}", src, re.S)
    assert body, "gb_lg"
    loop = re.findall(r"while\s*\(lg\s*<\s*(\d+)\s*&&\s*\(\(uint64_t\)\s*(\d+)\s*<<\s*lg\)\s*<\s*m\)", body.group(1))
    assert len(loop) == 1, "gb_lg's loop"
    out["GB_LG_MAX"], out["GB_PER_BUCKET"] = int(loop[0][0]), int(loop[0][1])
    return out


def test_bucket_constants_match_the_kernels():
    """shape_cases' restatement of the bucket arithmetic uses dedup.hip's constants: a retune of
    the kernels fails here instead of moving a branch out from under the bucket-size sweep."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spacedrive_amd", "csrc", "dedup.hip")
    assert parse_gb_constants(path) == {"GB_CAP": sc.GB_CAP, "GB_BIG_CAP": sc.GB_BIG_CAP, "GB_BIG_GRID": sc.GB_BIG_GRID,
                                        "GB_LG_MAX": sc.GB_LG_MAX, "GB_PER_BUCKET": sc.GB_PER_BUCKET}
    assert (sc.GB_LG_MAX, sc.GB_PER_BUCKET) == (24, 48)


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
