#!/usr/bin/env python3
"""Measurement record for the CDC deltas (a tool, not a gate; not part of bench.py): writes one JSON
object, committed as profiles/cdc_delta/probe.json.

Input: synthetic content filled on the device at the default parameters (16 / 16 KiB / 256 KiB):
`--files` base files of `--mib` MiB each (64 x 64 MiB at the default) and as many targets, each its
base with 5 bytes inserted at byte 1000; then one base of `--single-gib` GiB and its target.  Cut,
hash and shared run once, untimed.

One MI355X, one process.  After 2 warm-ups, HIP-event times on the current stream, median of `reps`
with min..max, the arms interleaved:

* plan       sd_cdc_delta_plan with every output (its kernels, one scan, one host wait);
* pack       sd_cdc_delta_pack of that plan: the few literal bytes;
* pack_all   sd_cdc_delta_pack of a plan with n_base = 0 over the same table: every distinct chunk
             of base and targets is a literal, so the segment copy moves the base's bytes from chunk
             offsets to literal offsets;
* apply      sd_cdc_delta_apply: the validation, its one host wait, then the segment copy of every
             target byte, almost all of it shifted by 5 bytes against its source;
* yardstick  sd_memcpy, device to device, of as many bytes as the apply moves.

The events span calls, not kernels.  The rebuilt targets are compared with the originals on the
device outside the timed region.
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
from spacedrive_amd import cdc  # noqa: E402
from spacedrive_amd._native import check, lib  # noqa: E402

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSERT_AT, INSERT = 1000, 5


def summary(ms, nbytes=None):
    out = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}
    if nbytes:
        out["bytes_moved"] = int(nbytes)
        out["GBps_at_median"] = nbytes / out["median_ms"] / 1e6
        out["GBps_min_max"] = [nbytes / out["max_ms"] / 1e6, nbytes / out["min_ms"] / 1e6]
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(ctx, files: int, length: int, reps: int) -> dict:
    tlen = length + INSERT
    stride = (tlen + 63) // 64 * 64 + 64
    n = 2 * files
    offs = np.arange(n, dtype=U) * U(stride)
    lens = np.concatenate([np.full(files, length, U), np.full(files, tlen, U)])
    d_data = torch.zeros(n * stride + 64, dtype=torch.uint8, device="cuda")
    ins = torch.arange(1, INSERT + 1, dtype=torch.uint8, device="cuda")
    for f in range(files):
        b, t = int(offs[f]), int(offs[files + f])
        ctx.synth_fill(7000 + f, 0, length, d_data[b:])
        d_data[t:t + INSERT_AT] = d_data[b:b + INSERT_AT]
        d_data[t + INSERT_AT:t + INSERT_AT + INSERT] = ins
        d_data[t + INSERT_AT + INSERT:t + tlen] = d_data[b + INSERT_AT:b + length]
    torch.cuda.synchronize()
    c = sd.Cdc(ctx, offs, lens, None)
    m = c.cut(d_data)
    base = c.layout()
    d_chunks = torch.empty((m, 2), dtype=torch.int64, device="cuda")
    d_ids = torch.empty((m, 32), dtype=torch.uint8, device="cuda")
    c.hash(d_data, d_chunks, d_ids)
    d_rep = torch.empty(m, dtype=torch.int64, device="cuda")
    c.shared(d_chunks, d_ids, d_rep=d_rep)
    mt = m - int(base[files])
    d_lit_off = torch.empty(mt, dtype=torch.int64, device="cuda")
    d_runs = torch.empty((mt, 4), dtype=torch.int64, device="cuda")
    d_files = torch.empty((files, 6), dtype=torch.int64, device="cuda")
    n_runs, stats = cdc.delta_plan(ctx, base, files, d_chunks, d_rep, d_lit_off, d_runs, mt, d_files)
    lit_bytes = int(stats[5])
    d_lit = torch.zeros((lit_bytes + 63) // 64 * 64 + 64, dtype=torch.uint8, device="cuda")
    # the plan with no base: everything distinct is a literal
    d_lit_off0 = torch.empty(m, dtype=torch.int64, device="cuda")
    _, stats0 = cdc.delta_plan(ctx, base, 0, d_chunks, d_rep, d_lit_off0)
    d_lit0 = torch.zeros(int(stats0[5]) + 64, dtype=torch.uint8, device="cuda")
    out_offs, out_lens = offs[:files], lens[files:]
    d_out = torch.zeros(files * stride + 64, dtype=torch.uint8, device="cuda")
    moved = int(out_lens.sum())
    d_yard = torch.empty(moved, dtype=torch.uint8, device="cuda")
    from spacedrive_amd.device import _stream

    def arm_plan():
        cdc.delta_plan(ctx, base, files, d_chunks, d_rep, d_lit_off, d_runs, mt, d_files)

    def arm_pack():
        cdc.delta_pack(ctx, base, files, offs, d_chunks, d_lit_off, d_rep, d_data, d_lit)

    def arm_pack_all():
        cdc.delta_pack(ctx, base, 0, offs, d_chunks, d_lit_off0, d_rep, d_data, d_lit0)

    def arm_apply():
        cdc.delta_apply(ctx, d_runs, n_runs, offs[:files], lens[:files], d_data, d_lit, lit_bytes, out_offs, out_lens, d_out)

    def arm_yard():
        check(lib().sd_memcpy(ctx.handle, d_yard.data_ptr(), d_data.data_ptr(), moved, _stream(None)))

    arms = {"plan": arm_plan, "pack": arm_pack, "pack_all": arm_pack_all, "apply": arm_apply, "yardstick_memcpy": arm_yard}
    ms = {k: [] for k in arms}
    for r in range(2 + reps):
        for k, fn in arms.items():
            t = timed(fn)
            if r >= 2:
                ms[k].append(t)
    for f in range(files):  # the rebuilt targets are the targets
        o, t = int(out_offs[f]), int(offs[files + f])
        assert torch.equal(d_out[o:o + tlen], d_data[t:t + tlen]), f
    nbytes = {"plan": None, "pack": lit_bytes, "pack_all": int(stats0[5]), "apply": moved, "yardstick_memcpy": moved}
    out = {"files": files, "base_bytes_per_file": length, "target_bytes": moved, "chunks": m, "target_chunks": mt,
           "runs": n_runs, "plan_stats": [int(x) for x in stats], "plan_stats_no_base": [int(x) for x in stats0]}
    for k in arms:
        out[k] = summary(ms[k], nbytes[k])
    out["apply_over_yardstick"] = out["apply"]["median_ms"] / out["yardstick_memcpy"]["median_ms"]
    out["pack_all_GBps_over_yardstick_GBps"] = out["pack_all"]["GBps_at_median"] / out["yardstick_memcpy"]["GBps_at_median"]
    out["verified"] = "every rebuilt target equals its original, compared on the device"
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--single-gib", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdc_delta", "probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    runs = [measure(ctx, a.files, a.mib << 20, a.reps)]
    if a.single_gib:
        runs.append(measure(ctx, 1, a.single_gib << 30, a.reps))
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "params": [16, 16384, 262144], "runs": runs,
           "note": ("one process on a shared box; clocks not pinned: compare the arms with each other, not with another "
                    "run's; apply spans the validation and its host wait as well as the copy; bytes moved are bytes "
                    "written (as many are read)")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
