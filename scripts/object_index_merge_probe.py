#!/usr/bin/env python3
"""Measurement record for sd_object_index_merge_objects (a tool, not a gate): writes one JSON
object, committed as profiles/object_index/merge_probe.json.

An owners-mode index of the headline shard's size: 1 249 999 entries over 1 088 888 keys, every
record an Object of its own (mod.rs:229-333 gives same-step duplicates an Object each), so 161 111
Objects are surplus.  duplicate_entries(0, 2) and dedup.merge_map give the map that sends every
surplus Object to its key's first one.  Three routes to the merged index, each on a fresh copy of
the index, interleaved in one process, 1 warm-up round, median of --reps rounds; wall-clock time
around calls that end in a device synchronise, and HIP-event time beside it:

(a) merge_objects(d_from, d_to);
(b) the only route without it: export_links, the copy to the host, the relabel in numpy,
    remove_objects(from), and an insert that names every (key, to) pair once per link;
(c) an sd_object_index_apply that moves the same number of entries (the leaving pairs as its
    removal list, the relabelled pairs as its insertion list): the same-shape yardstick.

The three exports are asserted equal in the same run.
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
SHARD, GROUPS = 1_249_999, 1_088_888


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(U)


def timed(fn):
    """(wall ms, HIP-event ms) of fn, the device idle before and after"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, a.elapsed_time(b)


def summary(rows):
    return {"wall_ms": {"median": statistics.median(r[0] for r in rows), "min": min(r[0] for r in rows),
                        "max": max(r[0] for r in rows)},
            "event_ms": {"median": statistics.median(r[1] for r in rows), "min": min(r[1] for r in rows),
                         "max": max(r[1] for r in rows)}, "reps": len(rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=SHARD)
    ap.add_argument("--keys", type=int, default=GROUPS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="time one route alone (its name in the JSON), for a kernel trace")
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_index", "merge_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    rng = np.random.default_rng(23)
    log = lambda *s: print("[probe]", *s, file=sys.stderr, flush=True)  # noqa: E731
    n, nk = a.entries, a.keys
    pool = np.unique(rng.integers(1, 1 << 64, nk + nk // 8, dtype=U))[:nk]
    assert len(pool) == nk
    keys = np.concatenate([pool, pool[rng.integers(0, nk, n - nk)]])[rng.permutation(n)]
    ids = np.arange(1, n + 1, dtype=U)  # one Object per record
    d_keys, d_ids = dev(keys), dev(ids)

    def fresh():
        x = ObjectIndex(ctx, owners=True)
        assert x.insert(d_keys, d_ids) == n
        return x

    x = fresh()
    dk, di, _ = x.duplicate_entries(0, 2)
    f, t = dedup.merge_map(dk, di)
    x.close()
    d_from, d_to = dev(f), dev(t)
    surplus = len(f)
    assert surplus == n - nk
    # the yardstick's lists: the leaving pairs and what they become (every link count is 1 here)
    at = np.searchsorted(f, ids)
    leaving = f[np.minimum(at, surplus - 1)] == ids
    d_rm_k, d_rm_v = dev(keys[leaving]), dev(ids[leaving])
    d_in_v = dev(t[at[leaving]])
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "entries": n, "keys": nk, "map_rows": surplus,
           "moved": int(leaving.sum())}
    res = {}

    def route_a(x):
        res["a"] = x.merge_objects(d_from, d_to)

    def route_b(x):
        k, v, c = (host(q) for q in x.export_links())
        j = np.searchsorted(f, v)
        go = f[np.minimum(j, surplus - 1)] == v
        rows = np.repeat(np.flatnonzero(go), c[go].astype(np.int64))
        x.remove_objects(d_from)
        x.insert(dev(k[rows]), dev(t[j[rows]]))

    def route_c(x):
        x.apply(d_rm_k, d_rm_v, d_rm_k, d_in_v)

    routes = (("merge_objects", route_a), ("export_relabel_remove_insert", route_b), ("apply_same_moves", route_c))
    routes = tuple(r for r in routes if a.only in (None, r[0]))  # one route alone: for a kernel trace
    rows = {name: [] for name, _ in routes}
    want = None
    for r in range(1 + a.reps):
        for name, fn in routes:
            x = fresh()
            ms = timed(lambda: fn(x))
            if r:
                rows[name].append(ms)
            if r == 0:  # the three routes end at one index
                got = [host(q) for q in x.export_links()]
                assert len(got[0]) == nk
                assert want is None or all(np.array_equal(p, q) for p, q in zip(want, got)), name
                want = got
            x.close()
        log("round %d done" % r)
    assert "a" not in res or res["a"] == (surplus, surplus)
    for name, _ in routes:
        out[name] = summary(rows[name])
        log("%s %.3f ms" % (name, out[name]["wall_ms"]["median"]))
    if len(routes) == 3:
        m = out["merge_objects"]["wall_ms"]["median"]
        out["merge_objects_vs_old_route"] = m / out["export_relabel_remove_insert"]["wall_ms"]["median"]
        out["merge_objects_vs_apply"] = m / out["apply_same_moves"]["wall_ms"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
