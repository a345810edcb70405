#!/usr/bin/env python3
"""Measurement record for the Object index's owners mode (a tool, not a gate): writes one JSON
object, committed as profiles/object_index/owners_probe.json.

Two indexes over the same 10 M uniform keys, one owner per key: a first-mode one and an
owners-mode one.  HIP-event times, 2 warm-ups, median of 10; every comparison is against the
first-mode code path in the same run, and the outputs are asserted equal to the numpy mirrors in
the same run.

* reads: sd_object_index_lookup, and sd_dedup_group + sd_dedup_owners_indexed, of the headline
  shard's 1 249 999 records, owners mode as a ratio to first mode (the same kernels);
* per-event calls, the DB query left out on both sides (which favours the old cycle): a
  deletion = one remove (new) against remove + insert (old), once of the pair's last link (the
  entry leaves) and once of one link of two (it stays); a content change = remove + insert (new)
  against remove + lookup + insert (old);
* the scan's insert: 1.25 M pairs at 0 / 50 / 100 % hits into the owners-mode index, against
  the first-mode insert of that scan's new heads only.  The price of the mode, in ms.
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
SHARD = 1_249_999


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


def versus(new, old):
    return {"owners_mode": new, "first_mode": old, "ratio": new["median_ms"] / old["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_index", "owners_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    rng = np.random.default_rng(7)
    keys = np.unique(rng.integers(0, 1 << 64, a.big, dtype=U))
    n = len(keys)
    vals = rng.permutation(n).astype(U)
    first, own = ObjectIndex(ctx), ObjectIndex(ctx, owners=True)
    d_keys, d_vals = dev(keys), dev(vals)
    assert first.insert(d_keys, d_vals) == n and own.insert(d_keys, d_vals) == n
    ones = np.ones(n, U)
    out = {"device": torch.cuda.get_device_name(0), "box": a.box, "index_entries": n, "reps": a.reps,
           "records": SHARD, "bytes_per_entry": {"first_mode": 16, "owners_mode": 24}}
    log = lambda *s: print("[probe]", *s, file=sys.stderr, flush=True)  # noqa: E731

    # ---- reads: the same kernels on both modes
    m = min(SHARD, n)  # (smaller only in a rehearsal with a small --big)
    out["records"] = m
    pick = rng.permutation(n)
    q = np.concatenate([keys[pick[:m // 2]], rng.integers(0, 1 << 64, m - m // 2, dtype=U)])
    q = q[rng.permutation(m)]
    d_q = dev(q)
    ids = torch.empty(m, dtype=torch.int64, device="cuda")
    found = torch.empty(m, dtype=torch.uint8, device="cuda")
    t_new = event_ms(lambda: own.lookup(d_q, ids, found), a.reps)
    got_new = (host(ids).copy(), found.cpu().numpy().copy())
    t_old = event_ms(lambda: first.lookup(d_q, ids, found), a.reps)
    at = np.minimum(np.searchsorted(keys, q), n - 1)
    hit = keys[at] == q
    assert np.array_equal(got_new[1], hit.astype(np.uint8)) and np.array_equal(found.cpu().numpy(), got_new[1])
    assert np.array_equal(got_new[0], np.where(hit, vals[at], U(0))) and np.array_equal(host(ids), got_new[0])
    out["lookup"] = versus(t_new, t_old)
    log("lookup x%.3f" % out["lookup"]["ratio"])

    recs = np.stack([q, np.arange(m, dtype=U)], axis=1).view(np.int64)
    d_src = torch.from_numpy(recs.copy()).cuda()
    d_r = torch.empty_like(d_src)
    d_rep, d_owner = (torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(2))
    d_ex = torch.empty(m, dtype=torch.uint8, device="cuda")
    d_new = torch.empty((m, 2), dtype=torch.int64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")

    def scan(index):
        ctx.dedup_group(d_r.view(-1), m, d_rep)
        index.owners(d_r.view(-1), m, d_rep, d_owner, d_ex, d_new, d_n)

    res = {}
    for name, index in (("owners_mode", own), ("first_mode", first)):
        res[name] = event_ms(lambda: scan(index), a.reps, before=lambda: d_r.copy_(d_src))
        res[name + "_out"] = (host(d_owner).copy(), d_ex.cpu().numpy().copy(), host(d_new[:int(d_n.item())]).copy())
    gr, grep, _ = dedup.group_host(recs)
    want = dedup.owners_indexed_host(gr, grep, keys, vals)
    for name in ("owners_mode_out", "first_mode_out"):
        g = res.pop(name)
        assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and np.array_equal(g[2].reshape(-1, 2), want[2])
    out["group_plus_owners_indexed"] = versus(res["owners_mode"], res["first_mode"])
    log("group + owners x%.3f" % out["group_plus_owners_indexed"]["ratio"])

    # ---- per-event calls on the 10 M index (the DB query is on neither side)
    one = lambda k, v: (dev(np.array([k], U)), dev(np.array([v], U)))  # noqa: E731
    ka, va = one(keys[pick[0]], vals[pick[0]])
    kb, _ = one(keys[pick[1]] ^ U(1), 0)  # cas_id B: not in the index
    assert not np.isin(host(kb), keys).any()
    ab_k, ab_v = torch.cat([ka, kb]), torch.cat([va, va])
    # a deleted file_path (c, O), the last link: new = one remove; old = remove + insert of the
    # DB's remaining owners (here the pair itself, which also restores the index)
    def reset_a():  # (A, O) with exactly one link, B absent
        own.remove(torch.cat([ka, kb]), None)
        own.insert(ka, va)

    t_new = event_ms(lambda: own.remove(ka, va), a.reps, before=reset_a)
    assert len(own) == n - 1
    reset_a()
    t_old = event_ms(lambda: (first.remove(ka, va), first.insert(ka, va)), a.reps)
    out["deletion"] = versus(t_new, t_old)
    # the commoner deletion: the pair keeps another link, so no entry leaves and the link is taken
    # in place; the old cycle's calls are the same two

    def reset_a2():  # (A, O) with two links
        reset_a()
        own.insert(ka, va)

    t_new = event_ms(lambda: own.remove(ka, va), a.reps, before=reset_a2)
    assert len(own) == n and own.links(ka, va).tolist() == [1]
    out["deletion_leaving_links"] = versus(t_new, t_old)
    # a content change A -> B on O: new = remove (A, O) + insert (B, O); old = remove (A, O) +
    # lookup B + insert of the DB's owners of {A, B}
    t_new = event_ms(lambda: (own.remove(ka, va), own.insert(kb, va)), a.reps, before=reset_a)
    assert len(own) == n and own.links(ab_k, ab_v).tolist() == [0, 1]
    reset_a()
    t_old = event_ms(lambda: (first.remove(ka, va), first.lookup(kb), first.insert(ab_k, ab_v)), a.reps,
                     before=lambda: first.remove(kb, None))
    first.remove(kb, None)
    out["content_change"] = versus(t_new, t_old)
    log("deletion x%.3f (leaving links x%.3f), content change x%.3f" % (
        out["deletion"]["ratio"], out["deletion_leaving_links"]["ratio"], out["content_change"]["ratio"]))
    ek, ev, el = (host(t) for t in own.export_links())
    assert np.array_equal(ek, keys) and np.array_equal(ev, vals) and np.array_equal(el, ones)
    fk, fv = (host(t) for t in first.export())
    assert np.array_equal(fk, keys) and np.array_equal(fv, vals)

    # ---- the scan's insert: every record's pair (owners) against the new heads only (first)
    out["scan_insert"] = []
    for pct in (0, 50, 100):
        hits = m * pct // 100
        fresh = rng.integers(0, 1 << 64, m - hits, dtype=U)
        fresh = fresh[~np.isin(fresh, keys)]
        pk = np.concatenate([keys[pick[:hits]], fresh])
        pv = np.concatenate([vals[pick[:hits]], np.arange(n, n + len(fresh), dtype=U)])
        sh = rng.permutation(len(pk))
        pk, pv = pk[sh], pv[sh]
        d_pk, d_pv = dev(pk), dev(pv)
        d_fk, d_fv = dev(fresh), dev(np.arange(n, n + len(fresh), dtype=U))
        state = {}
        t_new = event_ms(lambda: state.update(taken=own.insert(d_pk, d_pv)), a.reps,
                         before=lambda: own.remove(d_pk, d_pv) if state else None)
        wk, wv, wl, w_taken = dedup.owners_insert_host(keys, vals, ones, pk, pv)
        assert state["taken"] == w_taken == len(np.unique(fresh))
        assert all(np.array_equal(host(g), w) for g, w in zip(own.export_links(), (wk, wv, wl)))
        own.remove(d_pk, d_pv)
        case = {"pairs": len(pk), "hit_percent": pct, "new_entries": int(w_taken), "owners_mode": t_new}
        if len(fresh):
            st2 = {}
            t_old = event_ms(lambda: st2.update(taken=first.insert(d_fk, d_fv)), a.reps,
                             before=lambda: first.remove(d_fk, None) if st2 else None)
            assert st2["taken"] == w_taken
            first.remove(d_fk, None)
            case.update(first_mode_new_heads_only=t_old, ratio=t_new["median_ms"] / t_old["median_ms"])
        else:
            case.update(first_mode_new_heads_only=None, ratio=None)  # no new heads: the old cycle inserts nothing
        out["scan_insert"].append(case)
        log("scan insert %d %% hits: %.3f ms (first mode, new heads only: %s)" % (
            pct, t_new["median_ms"], case["first_mode_new_heads_only"] and "%.3f ms" % t_old["median_ms"]))
    assert len(own) == len(first) == n
    first.close(), own.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
