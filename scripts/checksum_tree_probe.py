#!/usr/bin/env python3
"""Measurement record for the checksum trees (a tool, not a gate): writes one JSON object,
committed as profiles/checksum_tree/probe.json.

Two device-resident shapes, each at block_log2 17 and 20:

* "large":  a few 1-GiB-class files (odd lengths);
* "many":   a few thousand files of 1-8 MiB (seeded lengths).

Per shape and block size, in one process on one box, HIP-event times on the current stream after
2 warm-ups, median of 10:

* sd_checksum_batch_run and sd_checksum_tree_run on the same buffer and ranges, INTERLEAVED (one
  of each per repetition, so both see the same clock history): what the nodes cost.  The same
  batch through sd_checksum_batch_time (iters = 1) is recorded beside them.
* sd_checksum_tree_roots (the roots from the level alone) and sd_checksum_tree_verify (hash,
  compare, compact; it ends in its own host sync), the latter also as a ratio to _run.

Outside the timed region the roots of _run and _roots are compared with sd_checksum_batch_run's,
a clean verify must return no row and a verify after one flipped byte exactly its block.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


def timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms) -> dict:
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def interleaved(fns: dict, reps: int, warm: int = 2) -> dict:
    """one call of every fn per repetition, in turn"""
    out = {k: [] for k in fns}
    for r in range(warm + reps):
        for k, fn in fns.items():
            ms = timed(fn)
            if r >= warm:
                out[k].append(ms)
    return {k: summary(v) for k, v in out.items()}


def layout(lens):
    offs, cur = [], 0
    for length in lens:
        offs.append(cur)
        cur = (cur + length + 64 + 127) // 128 * 128
    return np.array(offs, np.uint64), cur + 64


def shape_lens(name: str, gib: float, files: int):
    if name == "large":
        n = max(1, int(gib))
        return [MIB * 1024 + 4097 * (i + 1) + 13 for i in range(n)]
    rng = np.random.default_rng(20)
    return [int(x) for x in rng.integers(MIB, 8 * MIB + 1, files)]


def probe_shape(ctx, name, lens, reps):
    offs, total = layout(lens)
    lens_a = np.array(lens, np.uint64)
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    step = 256 * MIB
    for at in range(0, total, step):  # random bytes, a slice at a time
        m = min(step, total - at)
        d[at:at + m] = torch.randint(0, 256, (m,), dtype=torch.uint8, device="cuda", generator=g)
    n = len(lens)
    out = {"files": n, "bytes": int(lens_a.sum())}
    cb = ctx.checksum_batch(offs, lens_a)
    h_plain, h_tree, h_roots = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(3))
    cb.run(d, h_plain)
    for k in (17, 20):
        t = ctx.checksum_tree(offs, lens_a, k)
        nodes = torch.zeros(32 * t.total_nodes, dtype=torch.uint8, device="cuda")
        # ---- the answers
        t.run(d, nodes, h_tree)
        t.roots(nodes, h_roots)
        torch.cuda.synchronize()
        assert torch.equal(h_tree, h_plain) and torch.equal(h_roots, h_plain)
        rows, stats = t.verify(d, nodes)
        assert len(rows) == 0 and list(stats) == [n, t.total_nodes, 0, 0]
        f = n // 2
        at = int(offs[f]) + int(lens[f]) - 1
        d[at] ^= 1
        rows, stats = t.verify(d, nodes)
        d[at] ^= 1
        assert rows.cpu().tolist() == [[f, (int(lens[f]) - 1) >> k]] and list(stats) == [n, t.total_nodes, 1, 1]
        # ---- the timings
        r = {"nodes": t.total_nodes, "node_bytes": 32 * t.total_nodes}
        r.update(interleaved({"checksum_batch_run": lambda: cb.run(d, h_plain), "tree_run": lambda: t.run(d, nodes, h_tree)}, reps))
        r["checksum_batch_time_iters1"] = summary([cb.time(d, h_plain, 1) for _ in range(2 + reps)][2:])
        r.update(interleaved({"tree_roots": lambda: t.roots(nodes, h_roots)}, reps))
        bad = torch.zeros(t.total_nodes, dtype=torch.uint8, device="cuda")
        rows_buf = torch.zeros((max(t.total_nodes, 1), 2), dtype=torch.int64, device="cuda")
        r.update(interleaved({"tree_verify": lambda: t.verify(d, nodes, d_bad=bad, d_rows_out=rows_buf)}, reps))
        r["nodes_cost_percent"] = 100.0 * (r["tree_run"]["median_ms"] / r["checksum_batch_run"]["median_ms"] - 1.0)
        r["verify_over_run"] = r["tree_verify"]["median_ms"] / r["tree_run"]["median_ms"]
        r["tree_run_GBps"] = out["bytes"] / r["tree_run"]["median_ms"] / 1e6
        r["checksum_batch_run_GBps"] = out["bytes"] / r["checksum_batch_run"]["median_ms"] / 1e6
        out[f"block_log2_{k}"] = r
        t.close()
    cb.close()
    del d
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large-gib", type=float, default=4, help="1-GiB-class files of the large shape")
    ap.add_argument("--many-files", type=int, default=2048, help="1-8 MiB files of the many shape")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checksum_tree", "probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "reps": a.reps}
    for name in ("large", "many"):
        out[name] = probe_shape(ctx, name, shape_lens(name, a.large_gib, a.many_files), a.reps)
    out["note"] = ("one process on a shared box; clocks not pinned: compare the rows with each other, "
                   "not with another run's")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
