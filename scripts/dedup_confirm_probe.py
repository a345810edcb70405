#!/usr/bin/env python3
"""Measurement record for the confirm step (a tool, not a gate): writes one JSON object,
committed as profiles/dedup_confirm/probe.json.

Input: synth.library(0, n, n) at n = 1 250 000 with its planted duplicates and sample twins.
The keys come from the cas hashes (hashed on the device, sd_dedup_partition's key column); the
checksums are synthetic 32-byte values derived from (content id, twin, size), so no file bytes
are needed: equal for exact duplicates, different for a twin.  Files of size 0 have no cas_id and
are invalid.

After 2 warm-ups, HIP-event times on the current stream (each call ends in its own host sync, so
an event pair spans what a caller waits for), median of 10, in one process on one box:

* sd_dedup_confirm on the prefix path and with "confirm_full_sort" 1;
* sd_dedup_group at the same m (records reset untimed before every call), on its default
  LDS-bucket path and on its radix-sort path ("dedup_variant" 0: one or two 64-bit sorts);
* sd_cpu_dedup_confirm (wall clock, median of 3).

The stats are checked against the plant and the numpy mirror outside the timed region.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd import cpu, dedup, synth  # noqa: E402
from spacedrive_amd.device import stage_plan  # noqa: E402

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def event_ms(fn, reps, warm=2, before=None):
    out = []
    for r in range(warm + reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= warm:
            out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def splitmix(x):
    x = np.asarray(x, U)
    with np.errstate(over="ignore"):
        z = x + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def synthetic_checksums(sizes, cids, twins):
    """32 bytes per file, a function of (content id, twin, size) alone"""
    with np.errstate(over="ignore"):
        seed = splitmix(cids.astype(U)) ^ splitmix(sizes.astype(U) * U(3) + U(1)) ^ splitmix(twins.astype(U) * U(5) + U(2))
        words = np.stack([splitmix(seed + U(w)) for w in range(4)], axis=1)
    return np.ascontiguousarray(words).view(np.uint8).reshape(len(sizes), 32)


def cas_hashes(ctx, sizes, cids, twins):
    n = len(sizes)
    ext, total = stage_plan(sizes)
    d_staged = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
    ctx.synth_stage_cas(dev(sizes.astype(U)), dev(cids.astype(U)), torch.from_numpy(twins.astype(np.int32)).cuda(),
                        d_ext, n, d_staged)
    d_hash = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    b = ctx.cas_batch(ext)
    b.run(d_staged, d_hash)
    torch.cuda.synchronize()
    b.close()
    return d_hash


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1_250_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_confirm", "probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    n = a.files
    sizes, cids, twins = synth.library(0, n, n)
    d_keys = dedup.keys_from_hashes_device(cas_hashes(ctx, sizes, cids, twins), ctx)
    sums = synthetic_checksums(sizes, cids, twins)
    valid = (sizes != 0).astype(np.uint8)
    d_sums, d_valid = torch.from_numpy(sums.reshape(-1)).cuda(), torch.from_numpy(valid).cuda()
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "files": n, "reps": a.reps,
           "dedup_variant": sd.get_tuning("dedup_variant")}

    # ---- the answer, against the plant and the mirror
    rep, size, verdict, sets, stats = dedup.confirm_device(ctx, d_keys, d_sums, d_valid)
    keys = d_keys.cpu().numpy().view(U)
    ok = valid != 0
    plant = np.stack([sizes[ok].astype(U), cids[ok].astype(U), twins[ok].astype(U)], axis=1)
    assert int(stats[0]) == int(ok.sum()) and int(stats[1]) == len(np.unique(keys[ok]))
    assert int(stats[3]) == len(np.unique(plant, axis=0)) and int(stats[4]) == len(sets)
    assert int(stats[0]) == int(stats[1] - stats[2] + stats[5] + stats[6])
    assert int(stats[3]) == int(stats[1] - stats[2] + stats[4] + stats[6])
    h_rep, h_size, h_verdict, h_sets, h_stats = dedup.confirm_host(keys, sums, valid)
    assert np.array_equal(h_stats, stats) and np.array_equal(h_sets, sets.cpu().numpy().view(U))
    assert np.array_equal(h_rep, rep.cpu().numpy().view(U)) and np.array_equal(h_verdict, verdict.cpu().numpy())
    twin_ok = ok & (twins != 0)
    out["stats"] = [int(x) for x in stats]
    out["planted"] = {"valid": int(ok.sum()), "twins": int(twin_ok.sum()),
                      "twins_refuted": int((h_verdict[twin_ok] == 3).sum()),
                      "confirmed_redundant": int(stats[5] - stats[4])}

    # ---- timings
    m = n
    cap = m // 2
    o_rep, o_size = (torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(2))
    o_verdict = torch.empty(m, dtype=torch.uint8, device="cuda")
    o_sets = torch.empty((cap, 3), dtype=torch.int64, device="cuda")

    def confirm():
        ctx.dedup_confirm(d_keys, d_sums, d_valid, m, o_rep, o_size, o_verdict, o_sets, cap)

    counters = {}
    for name, full in (("confirm_prefix", 0), ("confirm_full", 1)):
        sd.set_tuning("confirm_full_sort", full)
        before = ctx.dedup_confirm_stats()
        out[name] = event_ms(confirm, a.reps)
        after = ctx.dedup_confirm_stats()
        counters[name] = {k: after[k] - before[k] for k in after}
    sd.set_tuning("confirm_full_sort", 0)
    out["path_counters"] = counters
    assert counters["confirm_prefix"]["full"] == 0 and counters["confirm_full"]["prefix"] == 0

    orig = torch.stack([d_keys, torch.arange(m, dtype=torch.int64, device="cuda")], dim=1).contiguous()
    recs = orig.clone()
    g_rep = torch.empty(m, dtype=torch.int64, device="cuda")
    out["dedup_group"] = event_ms(lambda: ctx.dedup_group(recs, m, g_rep, index_sorted=True), a.reps,
                                  before=lambda: recs.copy_(orig))
    out["dedup_group_unsorted"] = event_ms(lambda: ctx.dedup_group(recs, m, g_rep), a.reps, before=lambda: recs.copy_(orig))
    # the radix-sort grouping ("dedup_variant" 0): the path whose pass count the prefix path shares
    keep = sd.get_tuning("dedup_variant")
    try:
        sd.set_tuning("dedup_variant", 0)
        out["dedup_group_radix"] = event_ms(lambda: ctx.dedup_group(recs, m, g_rep, index_sorted=True), a.reps,
                                            before=lambda: recs.copy_(orig))
        out["dedup_group_radix_unsorted"] = event_ms(lambda: ctx.dedup_group(recs, m, g_rep), a.reps,
                                                     before=lambda: recs.copy_(orig))
    finally:
        sd.set_tuning("dedup_variant", keep)

    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        cpu.confirm(keys, sums, valid)
        host.append((time.perf_counter() - t0) * 1e3)
    out["cpu_confirm"] = {"median_ms": statistics.median(host), "min_ms": min(host), "max_ms": max(host), "reps": 3}
    out["ratio_prefix_over_group"] = out["confirm_prefix"]["median_ms"] / out["dedup_group"]["median_ms"]
    out["ratio_prefix_over_group_radix_unsorted"] = (out["confirm_prefix"]["median_ms"] /
                                                     out["dedup_group_radix_unsorted"]["median_ms"])
    out["ratio_full_over_prefix"] = out["confirm_full"]["median_ms"] / out["confirm_prefix"]["median_ms"]
    out["note"] = ("one process on a shared box; clocks not pinned: compare the rows with each other, "
                   "not with another run's")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
