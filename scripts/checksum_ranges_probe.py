#!/usr/bin/env python3
"""Measurement record for the range proofs of the checksum trees (a tool, not a gate): writes one
JSON object, committed as profiles/checksum_ranges/probe.json.

The two device-resident shapes of scripts/checksum_blocks_probe.py ("large": a few 1-GiB-class
files; "many": a few thousand files of 1-8 MiB), each at block_log2 17 and 20, in one process on one
box, HIP-event times on the current stream after 2 warm-ups, median of 10, the arms of a comparison
INTERLEAVED on one buffer and one list.  Rows: about 1 % of the blocks as contiguous runs of 1, 16
and 4 096 blocks (a run length no file of the shape holds is recorded as skipped), and on "large" one
run that is the second half of the first file.

* verify:  A = sd_checksum_tree_blocks_verify_proofs over the rows with per-block proofs (the
               parent's code);
           B = sd_checksum_tree_blocks_verify_range_proofs over the same rows as ranges.
           Target: B's median <= A's median + the spread (max - min) of A's own repetitions.
* prove:   sd_checksum_tree_blocks_prove_ranges against sd_checksum_tree_blocks_prove.  Recorded only.

Outside the timed region both proofs must verify clean against sd_checksum_tree_run's checksums, and
after one flipped byte exactly the range that holds it must come back.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spacedrive_amd as sd  # noqa: E402
from scripts.checksum_blocks_probe import every_block  # noqa: E402
from scripts.checksum_proofs_probe import height  # noqa: E402
from scripts.checksum_tree_probe import interleaved, layout, shape_lens  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
RUNS = (1, 16, 4096)


def pick_runs(nbs, run: int, want_blocks: int, seed: int):
    """[(file, first)] of non-overlapping runs of `run` blocks, run-aligned, until want_blocks are covered"""
    slots = [(f, a) for f, nb in enumerate(nbs) for a in range(0, int(nb) - run + 1, run)]
    if not slots:
        return []
    order = np.random.default_rng(seed).permutation(len(slots))
    return sorted(slots[i] for i in order[:max(1, want_blocks // run)])


def probe_rows(ctx, t, d, level, sums, lens_a, rows, at, ranges, k, reps):
    """one row of the table: `ranges` [(file, first, count)] as one list, both arms on it"""
    n = len(lens_a)
    idx = np.concatenate([int(t.node_base[f]) + np.arange(a, a + c) for f, a, c in ranges])
    rb = np.concatenate([[0], np.cumsum([c for _, _, c in ranges])]).astype(np.uint64)
    bl = ctx.checksum_tree_blocks(lens_a, rows[idx], at[idx], k)
    bl.set_ranges(rb)
    e_blocks, e_ranges = int(bl.proof_base[bl.m]), int(bl.range_proof_base[bl.q])
    p_blocks = torch.zeros(32 * max(e_blocks, 1), dtype=torch.uint8, device="cuda")
    p_ranges = torch.zeros(32 * max(e_ranges, 1), dtype=torch.uint8, device="cuda")
    bl.prove(level, p_blocks)
    bl.prove_ranges(level, p_ranges)
    h_max = max(height(t.node_base[f + 1] - t.node_base[f]) for f, _, _ in ranges)
    r = {"ranges": bl.q, "rows": bl.m, "bytes_hashed": bl.bytes_hashed, "block_proof_bytes": 32 * e_blocks,
         "range_proof_bytes": 32 * e_ranges, "h_max": h_max,
         "verify_proofs_launches": 3, "verify_range_proofs_launches": 3 + max(1, (h_max + 7) // 8)}
    # ---- the answers
    got, stats = bl.verify_proofs(d, p_blocks, sums)
    assert len(got) == 0 and list(stats) == [n, bl.m, 0, 0]
    got, stats = bl.verify_range_proofs(d, p_ranges, sums)
    assert len(got) == 0 and list(stats) == [n, bl.q, 0, 0]
    hit = bl.q // 2
    where = int(at[idx][int(rb[hit + 1]) - 1])
    d[where] ^= 1
    got, stats = bl.verify_range_proofs(d, p_ranges, sums)
    d[where] ^= 1
    assert got.cpu().tolist() == [[int(x) for x in ranges[hit]]] and list(stats) == [n, bl.q, 1, 1]
    # ---- verify: per-block proofs against the range proofs
    bad = torch.zeros(bl.m, dtype=torch.uint8, device="cuda")
    rows_out = torch.zeros((bl.m, 2), dtype=torch.int64, device="cuda")
    rbad = torch.zeros(bl.q, dtype=torch.uint8, device="cuda")
    ranges_out = torch.zeros((bl.q, 3), dtype=torch.int64, device="cuda")
    r["verify"] = interleaved(
        {"verify_proofs": lambda: bl.verify_proofs(d, p_blocks, sums, d_bad=bad, d_rows_out=rows_out),
         "verify_range_proofs": lambda: bl.verify_range_proofs(d, p_ranges, sums, d_bad=rbad, d_ranges_out=ranges_out)}, reps)
    a, b = r["verify"]["verify_proofs"], r["verify"]["verify_range_proofs"]
    r["verify"]["a_spread_ms"] = a["max_ms"] - a["min_ms"]
    r["verify"]["b_minus_a_ms"] = b["median_ms"] - a["median_ms"]
    r["verify"]["within_target"] = bool(b["median_ms"] <= a["median_ms"] + r["verify"]["a_spread_ms"])
    # ---- prove: recorded only
    r["prove"] = interleaved({"blocks_prove": lambda: bl.prove(level, p_blocks),
                              "blocks_prove_ranges": lambda: bl.prove_ranges(level, p_ranges)}, reps)
    r["prove"]["ranges_over_blocks"] = r["prove"]["blocks_prove_ranges"]["median_ms"] / r["prove"]["blocks_prove"]["median_ms"]
    bl.close()
    return r


def probe_shape(ctx, name, lens, reps):
    offs, total = layout(lens)
    lens_a = np.array(lens, np.uint64)
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    step = 256 * MIB
    for at0 in range(0, total, step):  # random bytes, a slice at a time
        m = min(step, total - at0)
        d[at0:at0 + m] = torch.randint(0, 256, (m,), dtype=torch.uint8, device="cuda", generator=g)
    n = len(lens)
    out = {"files": n, "bytes": int(lens_a.sum())}
    sums = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    for k in (17, 20):
        t = ctx.checksum_tree(offs, lens_a, k)
        level = torch.zeros(32 * t.total_nodes, dtype=torch.uint8, device="cuda")
        t.run(d, level, sums)
        rows, at = every_block(lens, offs, k)
        nbs = np.diff(t.node_base)
        res = {"nodes": t.total_nodes}
        for run in RUNS:
            picked = pick_runs(nbs, run, t.total_nodes // 100, 5 + run)
            if not picked:
                res[f"runs_of_{run}"] = {"skipped": "no file of this shape holds such a run"}
                continue
            res[f"runs_of_{run}"] = probe_rows(ctx, t, d, level, sums, lens_a, rows, at, [(f, a, run) for f, a in picked], k, reps)
        if name == "large":
            nb0 = int(nbs[0])
            res["second_half_of_file_0"] = probe_rows(ctx, t, d, level, sums, lens_a, rows, at, [(0, nb0 // 2, nb0 - nb0 // 2)],
                                                      k, reps)
        t.close()
        out[f"block_log2_{k}"] = res
    del d
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large-gib", type=float, default=4, help="1-GiB-class files of the large shape")
    ap.add_argument("--many-files", type=int, default=2048, help="1-8 MiB files of the many shape")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checksum_ranges", "probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "reps": a.reps}
    for name in ("large", "many"):
        out[name] = probe_shape(ctx, name, shape_lens(name, a.large_gib, a.many_files), a.reps)
    out["note"] = ("one process on a shared box; clocks not pinned: compare the arms of a row with each other, "
                   "not with another run's")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
