#!/usr/bin/env python3
"""Measurement record for the view by Object of an owners-mode index (a tool, not a gate):
writes one JSON object, committed as profiles/object_index/orphans_probe.json.

A 10 M-entry owners-mode index with one owner per key, and a second one in which one Object owns
10 % of the entries (the hot slot).  HIP-event times, 2 warm-ups, median of 10, minimum and
maximum recorded; the outputs are asserted equal to the numpy mirrors in the same run.  Cases:

* 512 ids (the reference's take per query, orphan_remover.rs:62), half of them absent;
* 100 000 ids, half of them absent;
* 512 ids against the hot-slot index, the hot Object among them;
* 512 ids at stride 2 out of an apply's d_removed_out;
* 512 ids against an index in which two Objects own 40 % of the entries each, alternating along
  the entries, both listed (beyond the four cases above: the lanes change slots at every hit).

Each case times sd_object_index_object_links and sd_object_index_orphans against
* sd_object_index_remove_objects on the same ids on a twin index in the same run (a by-Object
  pass over the same entries that also rewrites them; code this view does not touch), and
* the pass's algorithmic bytes, as achieved GB/s: 8 B per entry + the id list, and for
  object_links 8 B per hit (orphans never reads the links).
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
    ap.add_argument("--variant", default="registers; per-wave combine at a slot change; per-workgroup combine at the end; global atomic add",
                    help="label of the accumulation of k_object_totals that was built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_index", "orphans_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    rng = np.random.default_rng(11)
    keys = np.unique(rng.integers(0, 1 << 64, a.big, dtype=U))
    n = len(keys)
    vals = rng.permutation(n).astype(U)  # one owner per key, every Object one entry
    hot_id = U(n + 5)
    hot_vals = np.where(np.arange(n) % 10 == 0, hot_id, vals)
    ones = np.ones(n, U)
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "index_entries": n, "reps": a.reps,
           "accumulation": a.variant, "cases": {}}
    log = lambda *s: print("[probe]", *s, file=sys.stderr, flush=True)  # noqa: E731
    d_keys = dev(keys)

    def pair_of(v):
        x, twin = ObjectIndex(ctx, owners=True), ObjectIndex(ctx, owners=True)
        d_v = dev(v)
        assert x.insert(d_keys, d_v) == n and twin.insert(d_keys, d_v) == n
        return x, twin

    def case(name, x, twin, v, d_ids, stride, m, ids, twin_v=None):
        """ids: the m listed ids on the host (what d_ids holds at `stride`); v / twin_v: the Object ids
        of the entries of x / of the twin where it differs"""
        t_links = event_ms(lambda: x.object_links(d_ids, stride=stride, m=m), a.reps)
        gl, ge = (host(t).copy() for t in x.object_links(d_ids, stride=stride, m=m))
        res = {}
        t_orph = event_ms(lambda: res.update(o=x.orphans(d_ids, stride=stride, m=m)), a.reps)
        wl, we = dedup.owners_object_links_host(v, ones, ids)
        assert np.array_equal(gl, wl) and np.array_equal(ge, we), name
        assert np.array_equal(host(res["o"]), dedup.owners_orphans_host(v, ids)), name
        # the twin: remove_objects of the same ids into rows sized beforehand, the dropped pairs put
        # back before every run
        hits = int(we[np.unique(ids, return_index=True)[1]].sum())
        d_flat = dev(ids)
        tv = v if twin_v is None else twin_v
        twin_hits = int(dedup.owners_object_links_host(tv, np.ones(len(tv), U), np.unique(ids))[1].sum())
        d_rows = torch.empty((twin_hits + 16, 2), dtype=torch.int64, device="cuda")
        twin_n = len(twin)
        state = {}

        def restore():
            if state:
                p = state["pairs"]
                twin.insert(p[:, 0].contiguous(), p[:, 1].contiguous())

        t_rm = event_ms(lambda: state.update(pairs=twin.remove_objects(d_flat, d_removed_out=d_rows)[0]), a.reps,
                        before=restore)
        assert state["pairs"].shape[0] == twin_hits, name
        restore()
        assert len(twin) == twin_n
        bytes_o = 8 * n + 8 * m * stride  # orphans never reads the links
        bytes_ = bytes_o + 8 * hits
        c = {"ids": m, "stride": stride, "distinct": int(len(np.unique(ids))), "hit_entries": hits,
             "orphans": int(len(res["o"])), "object_links": t_links, "orphans_call": t_orph,
             "remove_objects_twin": t_rm, "remove_objects_twin_dropped": twin_hits, "algorithmic_bytes": bytes_, "orphans_algorithmic_bytes": bytes_o,
             "object_links_gb_per_s": bytes_ / (t_links["median_ms"] * 1e-3) / 1e9,
             "orphans_gb_per_s": bytes_o / (t_orph["median_ms"] * 1e-3) / 1e9,
             "object_links_vs_remove_objects": t_links["median_ms"] / t_rm["median_ms"],
             "orphans_vs_remove_objects": t_orph["median_ms"] / t_rm["median_ms"]}
        out["cases"][name] = c
        log("%s: object_links %.3f ms, orphans %.3f ms, remove_objects %.3f ms (x%.2f, x%.2f), %.0f / %.0f GB/s" % (
            name, t_links["median_ms"], t_orph["median_ms"], t_rm["median_ms"], c["object_links_vs_remove_objects"],
            c["orphans_vs_remove_objects"], c["object_links_gb_per_s"], c["orphans_gb_per_s"]))

    def half_absent(m, v):
        present = v[rng.permutation(n)[:m // 2]]
        absent = np.arange(2 * n + 10, 2 * n + 10 + m - m // 2, dtype=U)
        return np.concatenate([present, absent])[rng.permutation(m)]

    x, twin = pair_of(vals)
    for name, m in (("ids_512_half_absent", 512), ("ids_100000_half_absent", 100_000)):
        ids = half_absent(min(m, n), vals)
        case(name, x, twin, vals, dev(ids), 1, len(ids), ids)
    # 512 pairs leave through apply; their rows stay on the device and are read at stride 2
    pick = rng.permutation(n)[:min(512, n // 2)]
    d_pk, d_pv = dev(keys[pick]), dev(vals[pick])
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    rows, taken = x.apply(d_pk, d_pv, empty, empty)
    assert rows.shape[0] == len(pick) and taken == 0
    left = np.ones(n, bool)
    left[pick] = False
    n_full, n = n, n - len(pick)
    ones_full, ones = ones, ones[:n]
    case("ids_512_stride_2_from_apply", x, twin, vals[left], rows.reshape(-1)[1:], 2, int(rows.shape[0]),
         host(rows).reshape(-1, 2)[:, 1].copy(), twin_v=vals)  # the twin still holds the 512 pairs
    n, ones = n_full, ones_full
    x.close(), twin.close()

    x, twin = pair_of(hot_vals)
    ids = half_absent(min(512, n), hot_vals)
    ids[0] = hot_id
    case("ids_512_hot_slot_10_percent", x, twin, hot_vals, dev(ids), 1, len(ids), ids)
    x.close(), twin.close()

    two = np.where(np.arange(n) % 5 < 2, hot_id, np.where(np.arange(n) % 5 < 4, hot_id + U(1), vals))
    x, twin = pair_of(two)
    ids = half_absent(min(512, n), two)
    ids[0], ids[1] = hot_id, hot_id + U(1)
    case("ids_512_two_objects_40_percent_each", x, twin, two, dev(ids), 1, len(ids), ids)
    x.close(), twin.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
