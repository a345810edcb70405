"""bench.py --full end to end on the GPU at reduced sizes: the run exits 0, stdout carries exactly
one JSON line inside the driver's budget with the contract keys first, every leg's oracle
check reports zero mismatches, and the full record lands in the file the line names.  The
driver's own bench runs the default sizes; this guards the emitter and every leg's plumbing
in the driver-run GPU tests.  A plain run (no --full) times the steps
alone: its line keeps the contract keys and carries no leg, and --dump-outputs writes the
last timed step's outputs, checked here against the oracle."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SMALL = ["--steps", "3", "--warmup", "1", "--files-per-gpu", "60000", "--checksum-gib", "1", "--checksum-steps", "2",
         "--split-gib", "1", "--config-files", "20000", "--config-reps", "3", "--warm-ms", "20",
         "--file-backed-files", "20000", "--identifier-files", "10000", "--host-staged-files", "20000",
         "--host-checksum-gib", "1", "--file-checksum-mib", "1024", "--latency-calls", "40", "--cpu-seconds", "0.3"]


def test_bench_small_run_emits_one_compact_line(tmp_path):
    full = str(tmp_path / "full.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", *SMALL, "--full-out", full],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = lines[0]
    assert len(line) <= bench.LINE_TARGET
    d = json.loads(line)
    assert list(d)[:len(bench.STD_KEYS)] == list(bench.STD_KEYS)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert list(d)[len(bench.STD_KEYS):len(bench.STD_KEYS) + 2] == ["roofline", "cpu_baseline"]
    assert 0 < d["roofline"]["frac"] < 1.2 and d["roofline"]["kernel_ms"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] >= 1
    # every leg's oracle check: [files, mismatches] with zero mismatches
    assert d["parity"]["sample"][1] == 0 and d["parity"]["full"] == [60000, 0]
    for k, v in d["legs"].items():
        for pk in ("parity", "parity_full", "mixed_parity"):
            if pk in v:
                assert v[pk][1] == 0 and v[pk][0] > 0, (k, pk, v[pk])
    assert d["legs"]["configs_small"]["parity_full"] == [20000, 0]
    assert d["legs"]["configs_sampled"]["parity_full"] == [20000, 0]
    assert d["dedup"]["parity"] is True and d["dedup"]["records_per_rank"] == [d["dedup"]["records"]]
    assert d["full_record"] == full
    with open(full) as f:
        rec = json.load(f)
    assert abs(rec["value"] / d["value"] - 1) < 1e-3 and "note" in rec["steps_serial"]


def test_plain_run_times_the_steps_alone_and_dumps_their_outputs(tmp_path):
    import numpy as np
    import torch
    from spacedrive_amd import identifier, synth
    from spacedrive_amd.dedup import group_host
    n, steps = 30000, 2
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--files-per-gpu", str(n), "--dump-outputs", str(dump)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert list(d)[:len(bench.STD_KEYS)] == list(bench.STD_KEYS)
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "files/s"
    # value = the shard's files over one timed step
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 / n - 1) < 1e-9
    # nothing beside the timed steps ran
    assert "cpu_baseline" not in d and d["legs"] == {} and "full_record" not in d and d["launch"]["full"] is False
    assert "serial_value" not in d["kernels"] and d["parity"] == {}
    assert d["kernels"]["pipelined_value"] == pytest.approx(d["value"], rel=1e-3)
    a = {p.name[:-4]: np.load(p) for p in dump.iterdir()}
    assert set(a) == {"hashes", "hash_rows", "records", "representative", "owners", "record_rows", "counts"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    # the hashes: every file's row, an even-stride sample of them against the oracle
    assert a["hashes"].shape == (n, 32) and np.array_equal(a["hash_rows"], np.arange(n))
    h = a["hashes"].astype(np.uint8)
    assert np.array_equal(h, a["hashes"])
    sizes, cids, twins = synth.library(0, n, n)
    idx = bench.sample_idx(n, k=512)
    assert np.array_equal(h[idx], bench.oracle_hashes(sizes, cids, twins, idx))
    # the dedup step's records, representatives and owners: the host's grouping of those hashes
    valid = np.nonzero(sizes != 0)[0]
    key = np.ascontiguousarray(h[valid, :8]).view(">u8")[:, 0].astype(np.uint64).view(np.int64)
    want, rep_h, ng = group_host(np.stack([key, valid.astype(np.int64)], axis=1))
    own_h = identifier.object_owners(torch.from_numpy(want[:, 1].copy()), torch.from_numpy(rep_h.copy())).numpy()
    assert a["counts"].tolist() == [len(valid), ng]
    assert np.array_equal(a["record_rows"], np.arange(len(valid)))
    rec = a["records"]
    got_key = (rec[:, 0].astype(np.uint64) << np.uint64(32)) | rec[:, 1].astype(np.uint64)
    order = np.lexsort((rec[:, 2], got_key))
    assert np.array_equal(got_key[order], want[:, 0].view(np.uint64))
    assert np.array_equal(rec[order, 2], want[:, 1])
    assert np.array_equal(a["representative"][order], rep_h) and np.array_equal(a["owners"][order], own_h)
