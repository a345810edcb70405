#!/usr/bin/env python3
"""Measurement record for the block proofs of the checksum trees (a tool, not a gate): writes one
JSON object, committed as profiles/checksum_proofs/probe.json.

The two device-resident shapes of scripts/checksum_blocks_probe.py ("large": a few 1-GiB-class
files; "many": a few thousand files of 1-8 MiB), each at block_log2 17 and 20, 1 % of the blocks
shuffled, in one process on one box, HIP-event times on the current stream after 2 warm-ups, median
of 10, the arms of a comparison INTERLEAVED on one buffer:

* verify:  what a receiver that trusts only the checksums pays for those rows.
           A = sd_checksum_tree_roots over the whole level it was sent + sd_checksum_tree_blocks_verify
               against that level (both the parent's code);
           B = sd_checksum_tree_blocks_verify_proofs over the rows, their proofs and the checksums.
           Target: B's median <= A's median + the spread (max - min) of A's own repetitions.
* prove:   sd_checksum_tree_blocks_prove against sd_checksum_tree_roots on the same level: the ratio
           and the launches (interior-level passes + the gather).  Recorded only.

Outside the timed region the proofs must verify clean against sd_checksum_tree_run's checksums, and
after one flipped byte exactly that row must come back.
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
from scripts.checksum_tree_probe import interleaved, layout, shape_lens  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


def height(nb: int) -> int:
    return (int(nb) - 1).bit_length()


def reduce_passes(nb: int) -> int:
    """sd_checksum_tree_roots' reduce launches for a level of nb nodes: 256 to one per pass"""
    p, n = 0, int(nb)
    while n > 1:
        n, p = -(-n // 256), p + 1
    return p


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
    sums, h_roots = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2))
    for k in (17, 20):
        t = ctx.checksum_tree(offs, lens_a, k)
        level = torch.zeros(32 * t.total_nodes, dtype=torch.uint8, device="cuda")
        t.run(d, level, sums)
        rows, at = every_block(lens, offs, k)
        pick = np.random.default_rng(5).permutation(len(rows))[:max(1, len(rows) // 100)]
        bl = ctx.checksum_tree_blocks(lens_a, rows[pick], at[pick], k)
        entries = int(bl.proof_base[bl.m])
        proofs = torch.zeros(32 * max(entries, 1), dtype=torch.uint8, device="cuda")
        bl.prove(level, proofs)
        listed = sorted({int(f) for f in rows[pick][:, 0]})
        passes = max((max(height(t.node_base[f + 1] - t.node_base[f]) - 1, 0) + 7) // 8 for f in listed)
        r = {"nodes": t.total_nodes, "rows": bl.m, "bytes_hashed": bl.bytes_hashed, "proof_entries": entries,
             "proof_bytes": 32 * entries, "level_bytes": 32 * t.total_nodes, "listed_files": len(listed),
             "prove_launches": passes + 1, "roots_launches": 1 + max(reduce_passes(x) for x in np.diff(t.node_base))}
        # ---- the answers
        got, stats = bl.verify_proofs(d, proofs, sums)
        assert len(got) == 0 and list(stats) == [n, bl.m, 0, 0]
        hit = bl.m // 2
        where = int(at[pick][hit])
        d[where] ^= 1
        got, stats = bl.verify_proofs(d, proofs, sums)
        d[where] ^= 1
        assert got.cpu().tolist() == [[int(x) for x in rows[pick][hit]]] and list(stats) == [n, bl.m, 1, 1]
        # ---- verify: the level route against the proofs
        bad = torch.zeros(bl.m, dtype=torch.uint8, device="cuda")
        rows_out = torch.zeros((bl.m, 2), dtype=torch.int64, device="cuda")

        def level_route():
            t.roots(level, h_roots)
            bl.verify(d, level, d_bad=bad, d_rows_out=rows_out)

        r["verify"] = interleaved({"roots_plus_blocks_verify": level_route,
                                   "verify_proofs": lambda: bl.verify_proofs(d, proofs, sums, d_bad=bad, d_rows_out=rows_out)},
                                  reps)
        a, b = r["verify"]["roots_plus_blocks_verify"], r["verify"]["verify_proofs"]
        r["verify"]["a_spread_ms"] = a["max_ms"] - a["min_ms"]
        r["verify"]["b_minus_a_ms"] = b["median_ms"] - a["median_ms"]
        r["verify"]["within_target"] = bool(b["median_ms"] <= a["median_ms"] + r["verify"]["a_spread_ms"])
        # ---- prove against _roots on the same level
        r["prove"] = interleaved({"tree_roots": lambda: t.roots(level, h_roots), "blocks_prove": lambda: bl.prove(level, proofs)},
                                 reps)
        r["prove"]["prove_over_roots"] = r["prove"]["blocks_prove"]["median_ms"] / r["prove"]["tree_roots"]["median_ms"]
        bl.close()
        t.close()
        out[f"block_log2_{k}"] = r
    del d
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large-gib", type=float, default=4, help="1-GiB-class files of the large shape")
    ap.add_argument("--many-files", type=int, default=2048, help="1-8 MiB files of the many shape")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checksum_proofs", "probe.json"))
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
