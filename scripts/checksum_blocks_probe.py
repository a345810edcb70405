#!/usr/bin/env python3
"""Measurement record for the listed blocks of the checksum trees (a tool, not a gate): writes one
JSON object, committed as profiles/checksum_blocks/probe.json.

The two device-resident shapes of scripts/checksum_tree_probe.py ("large": a few 1-GiB-class files;
"many": a few thousand files of 1-8 MiB), each at block_log2 17 and 20, in one process on one box,
HIP-event times on the current stream after 2 warm-ups, median of 10, the arms of a comparison
INTERLEAVED on one buffer (one call of each per repetition, so both see the same clock history):

* dense:   every block, in file order, at the files' own positions: sd_checksum_tree_blocks_run
           against sd_checksum_tree_run (whose kernels are the parent's) on the same bytes.  The
           list does the same chunk compressions minus the levels above the block and pays a
           32-byte item read per block; the target is a ratio of at most 1.10.
* sparse:  1 % of the blocks, shuffled: sd_checksum_tree_blocks_verify against the full
           sd_checksum_tree_verify (both end in their own host sync).  Recorded only.
* update:  ("large" only) 3 blocks of one file through sd_checksum_tree_blocks_update against
           sd_checksum_tree_run of that file.  Recorded only.

Outside the timed region the dense list's nodes are compared with _tree_run's level, a clean sparse
verify must return no row and one after a flipped byte exactly its row, and the update's roots must
be _tree_run's of the changed bytes.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spacedrive_amd as sd  # noqa: E402
from scripts.checksum_tree_probe import interleaved, layout, shape_lens  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


def every_block(lens, offs, k):
    """(rows [m, 2], data_offsets [m]) of every block in file order at the files' own positions"""
    B = 1 << k
    nb = np.maximum((np.asarray(lens, np.uint64) + np.uint64(B - 1)) >> np.uint64(k), np.uint64(1)).astype(np.int64)
    f = np.repeat(np.arange(len(lens), dtype=np.int64), nb)
    j = np.arange(int(nb.sum()), dtype=np.int64) - np.repeat(np.cumsum(nb) - nb, nb)
    rows = np.stack([f, j], axis=1).astype(np.uint64)
    return rows, (np.asarray(offs, np.uint64)[f] + (j.astype(np.uint64) << np.uint64(k))).astype(np.uint64)


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
    h_tree, h_upd = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2))
    for k in (17, 20):
        t = ctx.checksum_tree(offs, lens_a, k)
        level = torch.zeros(32 * t.total_nodes, dtype=torch.uint8, device="cuda")
        t.run(d, level, h_tree)
        rows, at = every_block(lens, offs, k)
        r = {"nodes": t.total_nodes, "items_per_workgroup": 512 >> (k - 12)}
        # ---- dense
        dense = ctx.checksum_tree_blocks(lens_a, rows, at, k)
        assert dense.m == t.total_nodes and dense.bytes_hashed == out["bytes"]
        listed = torch.zeros(32 * dense.m, dtype=torch.uint8, device="cuda")
        dense.run(d, listed)
        torch.cuda.synchronize()
        assert torch.equal(listed, level)  # file order: the list's nodes are the level
        scratch = torch.zeros_like(level)
        r["dense"] = interleaved({"tree_run": lambda: t.run(d, scratch, h_tree), "blocks_run": lambda: dense.run(d, listed)}, reps)
        r["dense"]["blocks_over_tree_run"] = r["dense"]["blocks_run"]["median_ms"] / r["dense"]["tree_run"]["median_ms"]
        r["dense"]["blocks_run_GBps"] = out["bytes"] / r["dense"]["blocks_run"]["median_ms"] / 1e6
        r["dense"]["tree_run_GBps"] = out["bytes"] / r["dense"]["tree_run"]["median_ms"] / 1e6
        dense.close()
        # ---- sparse: 1 % of the blocks, shuffled
        pick = np.random.default_rng(5).permutation(len(rows))[:max(1, len(rows) // 100)]
        sparse = ctx.checksum_tree_blocks(lens_a, rows[pick], at[pick], k)
        got, stats = sparse.verify(d, level)
        assert len(got) == 0 and list(stats) == [n, sparse.m, 0, 0]
        hit = sparse.m // 2
        where = int(at[pick][hit])
        d[where] ^= 1
        got, stats = sparse.verify(d, level)
        d[where] ^= 1
        assert got.cpu().tolist() == [[int(x) for x in rows[pick][hit]]] and list(stats) == [n, sparse.m, 1, 1]
        bad_s = torch.zeros(sparse.m, dtype=torch.uint8, device="cuda")
        rows_s = torch.zeros((sparse.m, 2), dtype=torch.int64, device="cuda")
        bad_t = torch.zeros(t.total_nodes, dtype=torch.uint8, device="cuda")
        rows_t = torch.zeros((t.total_nodes, 2), dtype=torch.int64, device="cuda")
        r["sparse"] = interleaved({"tree_verify": lambda: t.verify(d, level, d_bad=bad_t, d_rows_out=rows_t),
                                   "blocks_verify": lambda: sparse.verify(d, level, d_bad=bad_s, d_rows_out=rows_s)}, reps)
        r["sparse"]["rows"] = sparse.m
        r["sparse"]["bytes_hashed"] = sparse.bytes_hashed
        r["sparse"]["tree_over_blocks_verify"] = r["sparse"]["tree_verify"]["median_ms"] / r["sparse"]["blocks_verify"]["median_ms"]
        sparse.close()
        t.close()
        # ---- update: 3 blocks of the first file against _tree_run of that file
        if name == "large":
            one = ctx.checksum_tree(offs[:1], lens_a[:1], k)
            nb0 = one.total_nodes
            lv = torch.zeros(32 * nb0, dtype=torch.uint8, device="cuda")
            one.run(d, lv, h_tree[:32])
            js = [1, nb0 // 2, nb0 - 1]
            u_rows = np.array([[0, j] for j in js], np.uint64)
            u_at = np.array([int(offs[0]) + (j << k) for j in js], np.uint64)
            upd = ctx.checksum_tree_blocks(lens_a[:1], u_rows, u_at, k)
            for j in js:
                d[int(offs[0]) + (j << k)] ^= 1
            upd.update(d, lv, h_upd[:32])
            want_lv = torch.zeros_like(lv)
            one.run(d, want_lv, h_tree[:32])
            torch.cuda.synchronize()
            assert torch.equal(lv, want_lv) and torch.equal(h_upd[:32], h_tree[:32])
            r["update"] = interleaved({"tree_run_one_file": lambda: one.run(d, want_lv, h_tree[:32]),
                                       "blocks_update": lambda: upd.update(d, lv, h_upd[:32])}, reps)
            r["update"]["file_bytes"] = int(lens_a[0])
            r["update"]["bytes_hashed"] = upd.bytes_hashed
            r["update"]["tree_run_over_update"] = (r["update"]["tree_run_one_file"]["median_ms"] /
                                                   r["update"]["blocks_update"]["median_ms"])
            for j in js:
                d[int(offs[0]) + (j << k)] ^= 1
            upd.close()
            one.close()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checksum_blocks", "probe.json"))
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
