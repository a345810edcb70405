#!/usr/bin/env python3
"""Measurement record for the view by key of an owners-mode index (a tool, not a gate): writes
one JSON object, committed as profiles/object_index/duplicates_probe.json.

A 10 M-entry owners-mode index in three mixes: one owner per key; 10 % of the keys with two
owners; one key with 1 M owners.  HIP-event times, 2 warm-ups, median of 10, minimum and maximum
recorded; the outputs are asserted equal to the numpy mirrors in the same run.  Per mix:

* sd_object_index_key_links of 100 000 keys, half of them absent (in the third mix the key with
  1 M owners among them, once);
* sd_object_index_duplicates(0, 2) and sd_object_index_duplicate_entries(0, 2) into outputs
  allocated beforehand (the merge candidates and their members);
* sd_object_index_duplicate_stats.

Each is set against two baselines in the same run, neither of which this view touches:
* sd_object_index_export_links on the same index, a pass over the same arrays (HIP events);
* what a user does without the view: export_links, the copy to the host and the numpy group-by
  (np.unique, np.add.reduceat) -- wall-clock time, since most of it is host work; the view's
  calls sync their stream, so their event times are wall-clock times too.

The pass's algorithmic bytes, as achieved GB/s: 16 B per entry (keys and links), plus 8 B per
head (duplicates reads an id per group) or per selected entry (duplicate_entries).
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
from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(U)


def summary(out, reps):
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def event_ms(fn, reps, warm=2):
    out = []
    for r in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= warm:
            out.append(a.elapsed_time(b))
    return summary(out, reps)


def wall_ms(fn, reps, warm=1):
    out = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return summary(out, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_index", "duplicates_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    rng = np.random.default_rng(12)
    log = lambda *s: print("[probe]", *s, file=sys.stderr, flush=True)  # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "reps": a.reps, "mixes": {}}
    pool = np.unique(rng.integers(1, 1 << 64, a.big + a.big // 8, dtype=U))  # distinct keys, ascending
    pool = pool[rng.permutation(len(pool))]

    def mix(name, keys, ids):
        n = len(keys)
        x = ObjectIndex(ctx, owners=True)
        assert x.insert(dev(keys), dev(ids)) == n
        o = np.lexsort((ids, keys))
        ek, ei, el = keys[o], ids[o], np.ones(n, U)
        have = np.unique(ek)
        m = min(a.queries, len(have))
        q = np.concatenate([have[rng.permutation(len(have))[:m // 2]], pool[len(pool) - (m - m // 2):]])
        q[0] = have[np.argmax(np.bincount(np.searchsorted(have, ek)))]  # the key with most owners, once
        q = q[rng.permutation(m)]
        d_q = dev(q)
        res = {}
        c = {"entries": n, "keys": int(len(have)), "queries": m}
        # -- the two baselines
        c["export_links"] = event_ms(lambda: res.update(e=x.export_links()), a.reps)

        def today():
            k, v, l = (host(t) for t in x.export_links())
            res["today"] = dedup.owners_duplicates_host(k, v, l, 0, 2)
        c["export_d2h_numpy_group_by"] = wall_ms(today, max(a.reps // 3, 2))
        # -- the view
        c["key_links"] = event_ms(lambda: res.update(kl=x.key_links(d_q)), a.reps)
        wl, wo = dedup.owners_key_links_host(ek, ei, el, q)
        assert np.array_equal(host(res["kl"][0]), wl) and np.array_equal(host(res["kl"][1]), wo), name
        want = dedup.owners_duplicates_host(ek, ei, el, 0, 2)
        wante = dedup.owners_duplicate_entries_host(ek, ei, el, 0, 2)
        assert all(np.array_equal(g, w) for g, w in zip(res["today"], want)), name
        rows, erows = max(len(want[0]), 1), max(len(wante[0]), 1)
        o4 = tuple(torch.empty(rows, dtype=torch.int64, device="cuda") for _ in range(4))
        o3 = tuple(torch.empty(erows, dtype=torch.int64, device="cuda") for _ in range(3))
        c["duplicates"] = event_ms(lambda: res.update(d=x.duplicates(0, 2, out=o4, capacity=rows)), a.reps)
        c["duplicate_entries"] = event_ms(lambda: res.update(e3=x.duplicate_entries(0, 2, out=o3, capacity=erows)), a.reps)
        c["duplicate_stats"] = event_ms(lambda: res.update(st=x.duplicate_stats()), a.reps)
        assert all(np.array_equal(host(g), w) for g, w in zip(res["d"], want)), name
        assert all(np.array_equal(host(g), w) for g, w in zip(res["e3"], wante)), name
        assert np.array_equal(res["st"], dedup.owners_duplicate_stats_host(ek, ei, el)), name
        c["qualifying_keys"], c["qualifying_entries"] = int(len(want[0])), int(len(wante[0]))
        c["stats"] = [int(t) for t in res["st"]]
        bytes_ = {"duplicates": 16 * n + 8 * len(have), "duplicate_entries": 16 * n + 8 * len(wante[0]),
                  "duplicate_stats": 16 * n, "export_links": 2 * 24 * n}
        c["algorithmic_bytes"] = bytes_
        c["gb_per_s"] = {k: b / (c[k]["median_ms"] * 1e-3) / 1e9 for k, b in bytes_.items()}
        c["key_links_mkeys_per_s"] = m / (c["key_links"]["median_ms"] * 1e-3) / 1e6
        for call in ("key_links", "duplicates", "duplicate_entries", "duplicate_stats"):
            c[call + "_vs_export_links"] = c[call]["median_ms"] / c["export_links"]["median_ms"]
            c[call + "_vs_export_d2h_numpy"] = c[call]["median_ms"] / c["export_d2h_numpy_group_by"]["median_ms"]
        out["mixes"][name] = c
        log("%s: export %.3f ms, today %.1f ms | key_links %.3f, duplicates %.3f, entries %.3f, stats %.3f ms" % (
            name, c["export_links"]["median_ms"], c["export_d2h_numpy_group_by"]["median_ms"], c["key_links"]["median_ms"],
            c["duplicates"]["median_ms"], c["duplicate_entries"]["median_ms"], c["duplicate_stats"]["median_ms"]))
        x.close()

    n = a.big
    mix("one_owner_per_key", pool[:n], rng.permutation(n).astype(U))
    nk = n * 10 // 11  # keys; a tenth of them own twice: nk + nk / 10 = n entries
    keys = np.concatenate([pool[:nk], pool[:n - nk]])
    mix("ten_percent_two_owners", keys, np.arange(n, dtype=U))
    hot = n // 10
    keys = np.concatenate([pool[:n - hot], np.full(hot, pool[n], U)])
    mix("one_key_with_a_tenth_of_the_entries", keys, rng.permutation(n).astype(U))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
