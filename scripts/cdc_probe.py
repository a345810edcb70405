#!/usr/bin/env python3
"""Measurement record for the content-defined chunks (a tool, not a gate; not part of bench.py):
writes one JSON object, committed as profiles/cdc/probe.json.

Input: synthetic content filled on the device, at the default parameters (16 / 16 KiB / 256 KiB):
`--files` files of `--mib` MiB each (64 x 64 MiB at the default), and one file of `--single-gib` GiB
for the select's serial walk.

One MI355X, one process.  After 2 warm-ups, HIP-event times on the current stream, median of `reps`
with min..max, the arms interleaved on the one data buffer:

* cut        sd_cdc_cut: the scan, the select's two passes, two prefix sums and two host waits;
* hash       sd_cdc_hash with both outputs (the shifted-load BLAKE3 over every chunk);
* yardstick  sd_checksum_batch_run over the same files: the existing aligned-load hash kernels.

The events span calls, not kernels: the scan's and the select's own times come from a kernel trace
of this script (`--reps 1`, a run of its own), kept beside the JSON as kernel_times.txt.  The cuts
and ids of the many-files shape are checked against the CPU twins outside the timed region.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd import cpu  # noqa: E402

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(ms, nbytes=None):
    out = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}
    if nbytes:
        out["GBps_at_median"] = nbytes / out["median_ms"] / 1e6
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(ctx, files: int, length: int, reps: int, verify: bool) -> dict:
    stride = (length + 63) // 64 * 64 + 64
    offs = np.arange(files, dtype=U) * U(stride)
    lens = np.full(files, length, U)
    d_data = torch.empty(files * stride + 64, dtype=torch.uint8, device="cuda")
    for f in range(files):
        ctx.synth_fill(5000 + f, 0, length, d_data[int(offs[f]):])
    torch.cuda.synchronize()
    c = sd.Cdc(ctx, offs, lens, None)
    m = c.cut(d_data)
    d_chunks = torch.empty((m, 2), dtype=torch.int64, device="cuda")
    d_ids = torch.empty((m, 32), dtype=torch.uint8, device="cuda")
    ck = ctx.checksum_batch(offs, lens)
    d_sums = torch.empty(files * 32, dtype=torch.uint8, device="cuda")

    def arm_cut():
        assert c.cut(d_data) == m

    def arm_hash():
        c.hash(d_data, d_chunks, d_ids)

    def arm_yard():
        ck.run(d_data, d_sums)

    ms = {"cut": [], "hash": [], "yardstick": []}
    for r in range(2 + reps):
        t = {"cut": timed(arm_cut), "hash": timed(arm_hash), "yardstick": timed(arm_yard)}
        if r >= 2:
            for k in ms:
                ms[k].append(t[k])
    stats = c.stats()
    nbytes = files * length
    out = {"files": files, "bytes_per_file": length, "bytes": nbytes, "chunks": m, "stats": [int(x) for x in stats],
           "cut": summary(ms["cut"], nbytes), "hash": summary(ms["hash"], nbytes),
           "yardstick_checksum_batch": summary(ms["yardstick"], nbytes)}
    out["hash_over_yardstick"] = out["hash"]["median_ms"] / out["yardstick_checksum_batch"]["median_ms"]
    host = d_data.cpu().numpy()
    base, chunks, c_stats = cpu.cdc_cut(host, offs, lens, None)
    assert np.array_equal(c_stats, stats) and np.array_equal(base, c.layout())
    assert np.array_equal(chunks, d_chunks.cpu().numpy().view(U))
    out["verified"] = "cuts and statistics equal the CPU twin's"
    if verify:
        assert np.array_equal(cpu.cdc_hash(host, offs, lens, base, chunks), d_ids.cpu().numpy())
        sums = np.zeros((files, 32), np.uint8)
        from spacedrive_amd._native import check, lib
        check(lib().sd_cpu_checksums(host.ctypes.data, offs.ctypes.data, lens.ctypes.data, files, sums.ctypes.data, 16))
        assert np.array_equal(sums.reshape(-1), d_sums.cpu().numpy())
        out["verified"] = "cuts, statistics, ids and the yardstick's checksums equal the CPU path's"
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--single-gib", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdc", "probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    runs = [measure(ctx, a.files, a.mib << 20, a.reps, True)]
    if a.single_gib:
        runs.append(measure(ctx, 1, a.single_gib << 30, a.reps, False))
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "params": [16, 16384, 262144], "runs": runs,
           "note": ("one process on a shared box; clocks not pinned: compare the arms with each other, not with "
                    "another run's; cut spans the scan, the select's two passes and two host waits")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
