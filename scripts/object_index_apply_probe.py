#!/usr/bin/env python3
"""Measurement record for sd_object_index_apply (a tool, not a gate): writes one JSON object,
committed as profiles/object_index/apply_probe.json.

One owners-mode index over 10 M uniform keys, one owner per key.  HIP-event times, 2 warm-ups,
median of 10.  Every case is timed twice in the same run: as ONE apply, and as the existing
sd_object_index_remove + sd_object_index_insert on the same lists, from the same starting state
(an untimed reverse call restores it before every repetition).  After each timed series the
index is exported and asserted equal to the numpy mirror (dedup.owners_apply_host).

* change: one content change, (A, O) leaves and (B, O) enters;
* change_in_place: one change where both pairs keep other links (only link counts change);
* burst_10000: 10 000 such changes in one call;
* burst_1_percent: 1 % of the entries leave and as many enter.
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


def event_ms(fn, reps, before, warm=2):
    out = []
    for r in range(warm + reps):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_index", "apply_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    rng = np.random.default_rng(7)
    keys = np.unique(rng.integers(0, 1 << 64, a.big, dtype=U))
    n = len(keys)
    vals = rng.permutation(n).astype(U)
    own = ObjectIndex(ctx, owners=True)
    assert own.insert(dev(keys), dev(vals)) == n
    pick = rng.permutation(n)
    log = lambda *s: print("[probe]", *s, file=sys.stderr, flush=True)  # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "index_entries": n, "reps": a.reps, "cases": {}}

    def fresh(m):
        f = np.unique(rng.integers(0, 1 << 64, m + m // 8 + 8, dtype=U))
        return rng.permutation(f[~np.isin(f, keys)])[:m]

    def case(name, base, rm, ins, leaves, enters):
        """base = (keys, ids, links) the case starts from; rm / ins = the lists (host arrays)"""
        (rk, rv), (ik, iv) = rm, ins
        d_rm, d_in = (dev(rk), dev(rv)), (dev(ik), dev(iv))
        wk, wv, wl, w_pairs, w_taken = dedup.owners_apply_host(*base, rk, rv, ik, iv)
        assert (len(w_pairs), w_taken) == (leaves, enters)

        def restore():  # the reverse: what came goes, what went comes (untimed)
            own.apply(*d_in, *d_rm)

        def check(what):
            assert all(np.array_equal(host(g), w) for g, w in zip(own.export_links(), (wk, wv, wl))), (name, what)
        got = {}
        t_apply = event_ms(lambda: got.update(r=own.apply(*d_rm, *d_in)), a.reps, before=lambda: restore() if got else None)
        assert (len(got["r"][0]), got["r"][1]) == (leaves, enters) and np.array_equal(host(got["r"][0]).reshape(-1, 2), w_pairs)
        check("apply")
        t_two = event_ms(lambda: (own.remove(*d_rm), own.insert(*d_in)), a.reps, before=restore)
        check("remove + insert")
        restore()
        assert all(np.array_equal(host(g), w) for g, w in zip(own.export_links(), base)), (name, "restored")
        out["cases"][name] = {"removal_pairs": len(rk), "insertion_pairs": len(ik), "entries_leaving": leaves,
                              "entries_entering": enters, "apply": t_apply, "remove_then_insert": t_two,
                              "ratio": t_apply["median_ms"] / t_two["median_ms"]}
        log("%s: apply %.3f ms, remove + insert %.3f ms, x%.3f" % (name, t_apply["median_ms"], t_two["median_ms"],
                                                                   out["cases"][name]["ratio"]))

    ones = np.ones(n, U)
    base = (keys, vals, ones)
    for name, m in (("change", 1), ("burst_10000", 10_000), ("burst_1_percent", n // 100)):
        m = max(min(m, n // 4), 1)
        sel = pick[:m]
        case(name, base, (keys[sel], vals[sel]), (fresh(m), vals[sel]), m, m)
    # both pairs keep other links: p1 holds 2 links and gives one up, p2 holds 1 and gains one
    p1, p2 = pick[:1], pick[1:2]
    assert own.insert(dev(keys[p1]), dev(vals[p1])) == 0
    two = ones.copy()
    two[p1] = 2
    case("change_in_place", (keys, vals, two), (keys[p1], vals[p1]), (keys[p2], vals[p2]), 0, 0)
    own.remove(dev(keys[p1]), dev(vals[p1]))
    assert all(np.array_equal(host(g), w) for g, w in zip(own.export_links(), base))
    own.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
