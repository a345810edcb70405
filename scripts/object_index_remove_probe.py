#!/usr/bin/env python3
"""Measurement record for the Object index's removals (a tool, not a gate): writes one JSON
object, committed as profiles/object_index/remove_probe.json.

On a 10 M-entry index (uniform keys, one Object per key), HIP-event times, 2 warm-ups, median
of 10, the export and the dropped pairs asserted equal to the numpy mirror in the same run:

* sd_object_index_remove_objects of 512 ids (the orphan remover's batch,
  orphan_remover.rs:62);
* sd_object_index_remove of 1 % of the entries, and of 1.25 M of the 10 M entries.

Each case is timed against what the header prescribed before: a fresh index bulk-built
(sd_object_index_insert into an empty index) from the survivors, which are already resident
and sorted on the device -- the DB dump and the upload a real rebuild needs are left out, which
flatters the rebuild.  Between repetitions the dropped pairs are inserted back, untimed, which
restores the index exactly.
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
from spacedrive_amd import dedup  # noqa: E402
from spacedrive_amd.device import ObjectIndex  # noqa: E402

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(U)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_index", "remove_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    rng = np.random.default_rng(7)
    keys = np.unique(rng.integers(0, 1 << 64, a.big, dtype=U))
    n = len(keys)
    vals = rng.permutation(n).astype(U)  # one Object per key, in no order
    x = ObjectIndex(ctx)
    assert x.insert(dev(keys), dev(vals)) == n
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "index_entries": n, "reps": a.reps, "cases": []}
    pick = rng.permutation(n)
    cases = [("remove_objects_512", "objects", vals[pick[:512]]),
             ("remove_by_key_1_percent", "keys", keys[pick[:n // 100]]),
             ("remove_by_key_1.25M", "keys", keys[pick[:min(1_250_000, n // 8)]])]
    for name, by, arg in cases:
        d_arg = dev(arg)
        buf = torch.empty((len(arg), 2), dtype=torch.int64, device="cuda")
        if by == "objects":
            want_k, want_v, want_pairs = dedup.index_remove_objects_host(keys, vals, arg)
        else:
            want_k, want_v, want_pairs = dedup.index_remove_host(keys, vals, arg)
        state = {}

        def restore():
            if "pairs" in state:
                p = state.pop("pairs")
                assert x.insert(p[:, 0].contiguous(), p[:, 1].contiguous()) == len(p)

        def remove():
            if by == "objects":
                state["pairs"], state["r"] = x.remove_objects(d_arg, d_removed_out=buf, capacity=len(arg))
            else:
                state["pairs"], state["r"] = x.remove(d_arg, d_removed_out=buf, capacity=len(arg))

        t = event_ms(remove, a.reps, before=restore)
        k, v = x.export()
        assert state["r"] == len(want_pairs) == len(arg) and np.array_equal(host(state["pairs"]), want_pairs)
        assert np.array_equal(host(k), want_k) and np.array_equal(host(v), want_v)
        # the rebuild the header prescribed: a fresh index from the survivors, resident and sorted
        box = {}

        def make_empty():
            if "y" in box:
                box["y"].close()
            box["y"] = ObjectIndex(ctx)

        tb = event_ms(lambda: box["y"].insert(k, v), a.reps, before=make_empty)
        yk, yv = box["y"].export()
        assert torch.equal(yk, k) and torch.equal(yv, v)
        box["y"].close()
        alg = 16 * n + 16 * n + len(arg) * (16 if by == "keys" else 8)  # entries read once, written once
        out["cases"].append({"case": name, "removed": int(state["r"]), "inputs": len(arg), **t,
                             "algorithmic_bytes": alg, "algorithmic_GBps": alg / (t["median_ms"] * 1e-3) / 1e9,
                             "rebuild_from_resident_survivors": tb,
                             "ratio_to_rebuild": t["median_ms"] / tb["median_ms"]})
        print("[probe] %s: %.3f ms, rebuild %.3f ms (x%.3f)" % (name, t["median_ms"], tb["median_ms"],
                                                                t["median_ms"] / tb["median_ms"]),
              file=sys.stderr, flush=True)
        restore()
        assert len(x) == n
    x.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
