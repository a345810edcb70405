#!/usr/bin/env python3
"""Measurement record for the shared blocks of a batch of levels (a tool, not a gate): writes one
JSON object, committed as profiles/tree_shared/probe.json.

Input: levels synthesised on the device, `files` files of 128 blocks at 128 KiB (8 388 608 slots =
1 TiB of content at the default, and the same at 1 048 576 slots): random 32-byte nodes; a quarter
of the files are copies of a file of the other three quarters with 1 % of their blocks changed.

One MI355X, one process.  After 2 warm-ups, HIP-event times on the current stream (each call ends
in its own host sync, so an event pair spans what a caller waits for), median of `reps` with
min..max, the arms interleaved on the one level buffer:

* A  sd_dedup_confirm over the same slots with key = block index and every output: the grouping
     core alone;
* B  sd_checksum_tree_shared with every output;
* C  the level copied to the host plus sd_cpu_checksum_tree_shared (wall clock, `host_reps` runs:
     the host sibling sorts on one thread and takes seconds at 8 M slots).

The answer is checked against the plant outside the timed region.
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
from spacedrive_amd import cpu  # noqa: E402

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, K = 128, 17


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def plant(files: int, seed: int):
    """-> d_nodes uint8 [files * NB * 32], src int64 [files] (the file a copy was taken from, -1 for
    an original), changed bool [files, NB]"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    nodes = torch.randint(-(1 << 62), 1 << 62, (files, NB, 4), dtype=torch.int64, device="cuda", generator=g)
    n_copy = files // 4
    perm = torch.randperm(files, device="cuda", generator=g)
    copies, originals = perm[:n_copy], perm[n_copy:]
    src_of = originals[torch.randint(0, len(originals), (n_copy,), device="cuda", generator=g)]
    changed = torch.rand((n_copy, NB), device="cuda", generator=g) < 0.01
    fresh = nodes[copies]
    nodes[copies] = torch.where(changed[:, :, None], fresh, nodes[src_of])
    src = torch.full((files,), -1, dtype=torch.int64, device="cuda")
    src[copies] = src_of
    ch = torch.zeros((files, NB), dtype=torch.bool, device="cuda")
    ch[copies] = changed
    return nodes.view(torch.uint8).reshape(-1), src.cpu().numpy(), ch.cpu().numpy()


def measure(ctx, files: int, reps: int, host_reps: int) -> dict:
    m = files * NB
    lens = np.full(files, NB << K, U)
    d_nodes, src, changed = plant(files, 1000 + files)
    d_keys = torch.arange(NB, dtype=torch.int64, device="cuda").repeat(files)
    o_rep, o_size = (torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(2))
    o_verdict = torch.empty(m, dtype=torch.uint8, device="cuda")
    o_sets = torch.empty((m // 2, 3), dtype=torch.int64, device="cuda")
    o_files = torch.empty((files, 4), dtype=torch.int64, device="cuda")
    o_pairs = torch.empty((m, 4), dtype=torch.int64, device="cuda")

    def arm_a():
        return ctx.dedup_confirm(d_keys, d_nodes, None, m, o_rep, o_size, o_verdict, o_sets, m // 2)

    def arm_b():
        return ctx.checksum_tree_shared(lens, d_nodes, K, 0, o_rep, o_size, o_files, o_pairs, m)

    # ---- the answer, against the plant: a copy's unchanged blocks are redundant exactly when the
    # copy comes after its source, else the source's are
    n_pairs, stats = arm_b()
    is_copy = src >= 0
    kept = (~changed[is_copy]).sum(axis=1)
    assert int(stats[0]) == files and int(stats[1]) == m and int(stats[4]) == int(kept.sum()) == m - int(stats[2])
    assert int(stats[5]) == int(stats[4]) << K
    pairs = o_pairs[:n_pairs].cpu().numpy().view(U)
    assert int(pairs[:, 2].sum()) == int(stats[4]) and n_pairs >= int((kept > 0).sum())  # a copy of a copied file: two holders
    a_sets, a_stats = arm_a()
    assert int(a_stats[3]) == int(stats[2]) and a_sets == int(stats[3])

    ms_a, ms_b = [], []
    for r in range(2 + reps):
        ta, tb = timed(arm_a), timed(arm_b)
        if r >= 2:
            ms_a.append(ta), ms_b.append(tb)
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        nodes = d_nodes.cpu().numpy()
        c_rep, c_size, c_files, c_pairs, c_stats = cpu.checksum_tree_shared(lens, nodes, K)
        host.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(c_stats, stats) and np.array_equal(c_pairs, pairs)
    assert np.array_equal(c_files, o_files.cpu().numpy().view(U)) and np.array_equal(c_rep, o_rep.cpu().numpy().view(U))
    out = {"files": files, "slots": m, "stats": [int(x) for x in stats], "pairs": int(n_pairs),
           "A_dedup_confirm": summary(ms_a), "B_tree_shared": summary(ms_b), "C_d2h_plus_cpu": summary(host)}
    out["B_over_A"] = out["B_tree_shared"]["median_ms"] / out["A_dedup_confirm"]["median_ms"]
    out["C_over_B"] = out["C_d2h_plus_cpu"]["median_ms"] / out["B_tree_shared"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, nargs="+", default=[65536, 8192])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_shared", "probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "block_log2": K, "blocks_per_file": NB,
           "runs": [measure(ctx, f, a.reps, a.host_reps) for f in a.files],
           "note": ("one process on a shared box; clocks not pinned: compare the arms with each other, "
                    "not with another run's")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
