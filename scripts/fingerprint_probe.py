#!/usr/bin/env python3
"""Measurement record for the fingerprint entries (a tool, not a gate): prints one JSON object,
committed as profiles/fingerprint/probe.json.

Device-resident part: HIP-event times of the gather, of the cas kernels it feeds and of the
checksum kernels over the same files, for 100 000 whole-kind files (configs[1]'s size law)
and 20 000 sampled files of 1-8 MiB.

Pinned-host part: the same bytes through sd_fingerprints (one upload) against sd_checksums +
sd_cas_ids over pre-staged messages (two uploads; the baseline's host staging time is left
out, which favours it), "host_cohash_threads" 0 and "checksum_split_adapt" 0 on both sides,
the two routes alternating, their outputs asserted equal.  The sampled batch's host part uses
its first --host-sampled files (pinned host memory for all 20 000 would be ~90 GB).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd import synth  # noqa: E402
from spacedrive_amd._native import check, lib  # noqa: E402
from spacedrive_amd.device import stage_plan  # noqa: E402

MiB = 1 << 20


def place(lens):
    """every range on a 128-B line of one buffer -> (offsets, total)"""
    padded = (lens + np.uint64(127)) // np.uint64(128) * np.uint64(128)
    offs = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.uint64)
    return offs, int(offs[-1] + padded[-1]) + 128


def event_ms(fn, reps, warm=2):
    """median and spread of fn()'s time on the current stream, by HIP events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def device_part(ctx, name, lens, cids, reps):
    offs, total = place(lens)
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    for L, c, o in zip(lens.tolist(), cids.tolist(), offs.tolist()):
        if L:
            ctx.synth_fill(c, 0, L, d[o:])
    torch.cuda.synchronize()
    fp = ctx.fingerprint_batch(offs, lens)
    staged = torch.empty(fp.staged_bytes + 64, dtype=torch.uint8, device="cuda")
    cas = ctx.cas_batch(fp.extents)
    ck = ctx.checksum_batch(offs, lens)
    h1 = torch.empty(32 * fp.n, dtype=torch.uint8, device="cuda")
    h2 = torch.empty(32 * fp.n, dtype=torch.uint8, device="cuda")
    r = {"files": fp.n, "file_bytes": fp.file_bytes, "staged_bytes": fp.staged_bytes,
         "gather_read_bytes": fp.gather_read_bytes,
         "gather": event_ms(lambda: fp.gather(d, staged), reps),
         "cas": event_ms(lambda: cas.run(staged, h1), reps),
         "checksum": event_ms(lambda: ck.run(d, h2), reps),
         "run_all": event_ms(lambda: fp.run(d, h1, h2), reps)}
    g = r["gather"]["median_ms"] * 1e-3
    r["gather_algorithmic_GBps"] = (fp.gather_read_bytes + fp.staged_bytes) / g / 1e9
    r["gather_over_cas"] = r["gather"]["median_ms"] / r["cas"]["median_ms"]
    # the same hashes either way
    fp.run(d, h1, h2)
    c2, k2 = torch.empty_like(h1), torch.empty_like(h2)
    fp.gather(d, staged)
    cas.run(staged, c2)
    ck.run(d, k2)
    torch.cuda.synchronize()
    assert torch.equal(h1, c2) and torch.equal(h2, k2)
    print(f"[{name}] device part done", file=sys.stderr, flush=True)
    return r, d, offs, total, fp, staged


def host_part(ctx, name, d, offs, lens, total, fp, staged, rounds):
    """one upload (sd_fingerprints) vs two (sd_checksums + sd_cas_ids), from pinned memory"""
    n = len(lens)
    data = torch.empty(total, dtype=torch.uint8).pin_memory()
    data.copy_(d[:total])
    fp.gather(d, staged)
    msgs = torch.empty(fp.staged_bytes, dtype=torch.uint8).pin_memory()  # the baseline's pre-staged messages
    msgs.copy_(staged[:fp.staged_bytes])
    torch.cuda.synchronize()
    ext = fp.extents
    o17a, o65a = ctypes.create_string_buffer(17 * n), ctypes.create_string_buffer(65 * n)
    o17b, o65b = ctypes.create_string_buffer(17 * n), ctypes.create_string_buffer(65 * n)

    def one():
        check(lib().sd_fingerprints(ctx.handle, data.data_ptr(), offs.ctypes.data, lens.ctypes.data, n, o17a, o65a))

    def two():
        check(lib().sd_checksums(ctx.handle, data.data_ptr(), offs.ctypes.data, lens.ctypes.data, n, o65b))
        check(lib().sd_cas_ids(ctx.handle, msgs.data_ptr(), fp.staged_bytes, ext.ctypes.data, n, o17b, None))

    t = {"one_upload": [], "two_uploads": []}
    for r in range(rounds + 1):  # round 0 warms both routes (pinned windows, plans) and is not counted
        for key, fn in (("one_upload", one), ("two_uploads", two)) if r % 2 == 0 else \
                (("two_uploads", two), ("one_upload", one)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r:
                t[key].append(dt * 1e3)
    assert o17a.raw == o17b.raw and o65a.raw == o65b.raw
    res = {"files": n, "file_bytes": int(lens.sum()), "message_bytes": int(ext["msg_len"].sum()), "rounds": rounds}
    for k, v in t.items():
        res[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    res["two_over_one"] = res["two_uploads"]["median_ms"] / res["one_upload"]["median_ms"]
    print(f"[{name}] host part done", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--whole", type=int, default=100_000)
    ap.add_argument("--sampled", type=int, default=20_000)
    ap.add_argument("--host-sampled", type=int, default=2_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--box", default=os.uname().nodename, help="label of the machine the numbers are from")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    ctx = sd.default_context(0)
    keep = {k: sd.get_tuning(k) for k in ("host_cohash_threads", "checksum_split_adapt")}
    sd.set_tuning("host_cohash_threads", 0)
    sd.set_tuning("checksum_split_adapt", 0)
    out = {"device": torch.cuda.get_device_name(0), "box": a.box,
           "tuning": {"host_cohash_threads": 0, "checksum_split_adapt": 0,
                      "fingerprint_window_mb": sd.get_tuning("fingerprint_window_mb")}}
    try:
        lens, cids, _ = synth.small_library(0, a.whole)
        r, d, offs, total, fp, staged = device_part(ctx, "whole", lens, cids, a.reps)
        out["whole"] = {"device": r, "pinned_host": host_part(ctx, "whole", d, offs, lens, total, fp, staged, a.rounds)}
        del d, staged
        fp.close()
        torch.cuda.empty_cache()
        u = np.random.default_rng(7).random(a.sampled)
        lens = np.floor(MiB * np.exp(u * np.log(8.0))).astype(np.uint64)  # log-uniform in [1, 8] MiB
        cids = np.arange(500_000, 500_000 + a.sampled, dtype=np.uint64)
        r, d, offs, total, fp, staged = device_part(ctx, "sampled", lens, cids, a.reps)
        out["sampled"] = {"device": r}
        h = min(a.host_sampled, a.sampled)
        fph = ctx.fingerprint_batch(offs[:h], lens[:h])
        sth = torch.empty(fph.staged_bytes + 64, dtype=torch.uint8, device="cuda")
        htotal = int(offs[h - 1] + lens[h - 1]) + 256
        out["sampled"]["pinned_host"] = host_part(ctx, "sampled", d, offs[:h].copy(), lens[:h].copy(), htotal, fph, sth,
                                                  a.rounds)
    finally:
        for k, v in keep.items():
            sd.set_tuning(k, v)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
