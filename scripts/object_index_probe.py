#!/usr/bin/env python3
"""Measurement record for the Object index (a tool, not a gate): writes one JSON object,
committed as profiles/object_index/probe.json.

On the records of one 1.25 M-file shard (synth.library at the bench's mixture, hashed on the
device), HIP-event times, 2 warm-ups, median of 10, outputs asserted equal to the numpy mirror
outside the timed region:

* the baseline: sd_dedup_group + sd_dedup_owners (the path without an index), and against it
  sd_dedup_group + sd_dedup_owners_indexed with an index of 0, 1.25 M and 10 M entries at
  0 %, 50 % and 100 % hits, timed in the same run;
* an A/B of the prefix directory against a binary search over the whole key array (tuning
  "index_dir_max_bits" 0) on the 10 M-entry index: the lookup kernel on the shard's keys in
  sorted and in shuffled order, and the owners kernel;
* insert of 1.25 M new pairs into a 10 M-entry index and a bulk build of 10 M, with the
  achieved bytes/s against the algorithmic bytes (both runs read once, the merged run
  written once; 16 B per entry).
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
from spacedrive_amd import dedup, synth  # noqa: E402
from spacedrive_amd.device import ObjectIndex, stage_plan  # noqa: E402

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def event_ms(fn, reps, warm=2, before=None):
    """median and spread of fn()'s time on the current stream, by HIP events; before() runs
    untimed ahead of every call"""
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


def shard_records(ctx, n):
    """the (key, index) records of an n-file shard, unsorted, as sd_dedup_partition leaves them"""
    sizes, cids, twins = synth.library(0, n, n)
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
    del d_staged
    d_valid = torch.from_numpy((sizes != 0).astype(np.uint8)).cuda()
    counts = torch.empty(1, dtype=torch.int64, device="cuda")
    recs = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    nv = ctx.dedup_partition(d_hash, d_valid, n, 0, 1, counts, recs)
    return recs[:nv].clone()


def filler(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, n, dtype=U)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1_250_000)
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_index", "probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "files": a.files, "reps": a.reps,
           "dedup_variant": sd.get_tuning("dedup_variant")}
    orig = shard_records(ctx, a.files)
    m = orig.shape[0]
    recs = orig.clone()
    rep = torch.empty(m, dtype=torch.int64, device="cuda")
    owner = torch.empty(m, dtype=torch.int64, device="cuda")
    existing = torch.empty(m, dtype=torch.uint8, device="cuda")
    new = torch.empty((m, 2), dtype=torch.int64, device="cuda")
    n_new = torch.zeros(1, dtype=torch.int64, device="cuda")
    out["records"] = m

    def reset():
        recs.copy_(orig)

    def baseline():
        ctx.dedup_group(recs, m, rep)
        ctx.dedup_owners(recs, m, rep, owner)

    def group_only():
        ctx.dedup_group(recs, m, rep)

    out["baseline_group_owners"] = event_ms(baseline, a.reps, before=reset)
    out["group_alone"] = event_ms(group_only, a.reps, before=reset)
    base = out["baseline_group_owners"]["median_ms"]
    h_recs, h_rep, ng = dedup.group_host(orig.cpu().numpy())
    uniq = np.unique(h_recs[:, 0].view(U))
    uniq = uniq[np.random.default_rng(1).permutation(len(uniq))]
    out["groups"] = ng
    print("[probe] records %d, groups %d, baseline %.3f ms" % (m, ng, base), file=sys.stderr, flush=True)

    # ---- the indexed owner rule against the baseline
    out["indexed"] = []
    for size in (0, a.files, a.big):
        for hits in (0.0, 0.5, 1.0):
            if size == 0 and hits:
                continue
            known = uniq[:int(hits * len(uniq))][:size]
            keys = np.unique(np.concatenate([known, filler(size - len(known), 2 + size % 97)]))
            vals = keys * U(3) + U(7)
            x = ObjectIndex(ctx)
            assert x.insert(dev(keys), dev(vals)) == len(keys)

            def indexed():
                ctx.dedup_group(recs, m, rep)
                x.owners(recs, m, rep, owner, existing, new, n_new)

            t = event_ms(indexed, a.reps, before=reset)
            w_owner, w_ex, w_new = dedup.owners_indexed_host(h_recs, h_rep, keys, vals)
            torch.cuda.synchronize()
            k = int(n_new.item())
            assert k == len(w_new) and np.array_equal(owner.cpu().numpy().view(U), w_owner)
            assert np.array_equal(existing.cpu().numpy(), w_ex) and np.array_equal(new[:k].cpu().numpy().view(U), w_new)
            out["indexed"].append({"index_entries": len(keys), "hit_share_of_groups": hits,
                                   "hit_share_of_records": float(w_ex.mean()), "new_heads": k, **t,
                                   "ratio_to_baseline": t["median_ms"] / base})
            print("[probe] index %d hits %.1f: %.3f ms (x%.3f)" % (len(keys), hits, t["median_ms"],
                                                                  t["median_ms"] / base), file=sys.stderr, flush=True)
            x.close()

    # ---- A/B: prefix directory vs one binary search over the whole key array, 10 M entries
    big_keys = np.unique(np.concatenate([uniq[:len(uniq) // 2], filler(a.big - len(uniq) // 2, 5)]))
    big_vals = big_keys * U(3) + U(7)
    d_big_k, d_big_v = dev(big_keys), dev(big_vals)
    group_only()
    q_sorted = recs[:, 0].contiguous()
    q_shuffled = q_sorted[torch.randperm(m, device="cuda")].contiguous()
    ids, found = torch.empty(m, dtype=torch.int64, device="cuda"), torch.empty(m, dtype=torch.uint8, device="cuda")
    variants = {}
    keep = sd.get_tuning("index_dir_max_bits")
    try:
        for name, bits in (("directory", keep), ("binary_search", 0)):
            sd.set_tuning("index_dir_max_bits", bits)
            variants[name] = ObjectIndex(ctx)
            assert variants[name].insert(d_big_k, d_big_v) == len(big_keys)
    finally:
        sd.set_tuning("index_dir_max_bits", keep)
    ab = {name: {"lookup_sorted": [], "lookup_shuffled": [], "owners": []} for name in variants}
    want = None
    for _ in range(3):  # the two variants alternate
        for name, x in variants.items():
            ab[name]["lookup_sorted"].append(event_ms(lambda: x.lookup(q_sorted, ids, found), a.reps)["median_ms"])
            ab[name]["lookup_shuffled"].append(event_ms(lambda: x.lookup(q_shuffled, ids, found), a.reps)["median_ms"])
            ab[name]["owners"].append(event_ms(lambda: x.owners(recs, m, rep, owner, existing, new, n_new),
                                               a.reps)["median_ms"])
            torch.cuda.synchronize()
            got = (owner.cpu().numpy().copy(), existing.cpu().numpy().copy(), found.cpu().numpy().copy())
            if want is None:
                want = got
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
    out["directory_ab"] = {"index_entries": len(big_keys), "queries": m,
                           **{name: {k: statistics.median(v) for k, v in r.items()} for name, r in ab.items()}}
    out["directory_ab"]["binary_over_directory"] = {
        k: out["directory_ab"]["binary_search"][k] / out["directory_ab"]["directory"][k]
        for k in ("lookup_sorted", "lookup_shuffled", "owners")}
    print("[probe] A/B", json.dumps(out["directory_ab"]["binary_over_directory"]), file=sys.stderr, flush=True)
    for x in variants.values():
        x.close()

    # ---- insert into a 10 M-entry index, and the bulk build of 10 M
    fresh = filler(a.files, 9)
    fresh = fresh[~np.isin(fresh, big_keys)]
    d_fresh_k, d_fresh_v = dev(fresh), dev(fresh * U(5))
    box = {}

    def make_big():
        if "x" in box:
            box["x"].close()
        box["x"] = ObjectIndex(ctx)
        box["x"].insert(d_big_k, d_big_v)

    def make_empty():
        if "x" in box:
            box["x"].close()
        box["x"] = ObjectIndex(ctx)

    t = event_ms(lambda: box["x"].insert(d_fresh_k, d_fresh_v), a.reps, before=make_big)
    assert len(box["x"]) == len(big_keys) + len(np.unique(fresh))
    alg = 16 * (len(big_keys) + len(fresh)) + 16 * len(box["x"])
    out["insert_into_big"] = {"index_entries": len(big_keys), "new_pairs": len(fresh), **t, "algorithmic_bytes": alg,
                              "algorithmic_GBps": alg / (t["median_ms"] * 1e-3) / 1e9}
    t = event_ms(lambda: box["x"].insert(d_big_k, d_big_v), a.reps, before=make_empty)
    k, v = box["x"].export()
    assert np.array_equal(k.cpu().numpy().view(U), big_keys) and np.array_equal(v.cpu().numpy().view(U), big_vals)
    alg = 32 * len(big_keys)
    out["bulk_build"] = {"entries": len(big_keys), **t, "algorithmic_bytes": alg,
                         "algorithmic_GBps": alg / (t["median_ms"] * 1e-3) / 1e9}
    box["x"].close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
