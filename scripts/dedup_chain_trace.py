"""The dedup chain beside the hashing, from rocprofv3 --kernel-trace csv files (profiles/dedup_chain/).

    python scripts/dedup_chain_trace.py PIPELINED_kernel_trace.csv [SERIAL_kernel_trace.csv] [--steps 30]

PIPELINED is a trace of `bench.py --steps K`, SERIAL one of `bench.py --steps K --no-overlap`.  A file
`*_memory_copy_trace.csv` beside either is read too when it exists.  Prints markdown:
  * per timed step, the interval between the end of one batch's last hash kernel and the start of the next
    batch's first, and the dedup kernels and copies that run inside it;
  * per link of the chain, its duration beside the hashing and in the serial steps.
"""
from __future__ import annotations

import argparse
import collections
import csv
import os
import statistics

HASH_FIRST, HASH_LAST = "k_cas_sampled_lanes", "k_whole_merge8"
HASH = ("k_cas_sampled_lanes", "k_cas_sampled_merge", "k_whole_items", "k_whole_merge8")
CHAIN_FIRST = "k_part_count"
CHAIN = ("k_part_", "k_gb_", "k_owners", "rccl", "ncclDevKernel", "rocprim", "rocclr")


def short(name: str) -> str:
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    if name.startswith("__amd_rocclr_"):  # the runtime's own copy and fill kernels
        return "rocclr " + name[len("__amd_rocclr_"):]
    if "rocprim" in name:
        for key in ("onesweep_histograms", "onesweep_iteration", "radix_sort", "scan"):
            if key in name:
                return "rocprim " + key
        return "rocprim kernel"
    return name.split("<")[0].split("::")[-1].strip()


def read(path: str):
    ev = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            gx = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
            wx = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 0)
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), gx, wx))
    mc = path.replace("kernel_trace", "memory_copy_trace")
    if mc != path and os.path.exists(mc):
        with open(mc, newline="") as f:
            for r in csv.DictReader(f):
                ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                           "copy " + (r.get("Direction") or "").replace("MEMORY_COPY_", ""), 0, 0))
    ev.sort()
    return ev


def is_chain(name: str) -> bool:
    return name.startswith("copy ") or any(name.startswith(p) or p in name for p in CHAIN)


def batches(ev):
    """(start of the first hash kernel, end of the last) of every batch of the modal launch shape"""
    lanes = [e for e in ev if e[2] == HASH_FIRST]
    if not lanes:
        return []
    grid = collections.Counter(e[3] for e in lanes).most_common(1)[0][0]
    starts = [e[0] for e in lanes if e[3] == grid]
    out = []
    for i, t0 in enumerate(starts):
        t1 = starts[i + 1] if i + 1 < len(starts) else t0 + 50_000_000
        mine = [e for e in ev if t0 <= e[0] < t1 and e[2] in HASH]
        last = [e for e in mine if e[2] == HASH_LAST]
        if last:
            out.append((t0, max(e[1] for e in last)))
    return out


def chains(ev, steps):
    """the last `steps` dedup chains: lists of events from k_part_count to the next chain's start"""
    heads = [e[0] for e in ev if e[2] == CHAIN_FIRST]
    out = []
    for i, t0 in enumerate(heads):
        t1 = heads[i + 1] if i + 1 < len(heads) else t0 + 20_000_000
        out.append([e for e in ev if t0 <= e[0] < t1 and is_chain(e[2]) and not e[2].startswith("copy ")])
    return out[-steps:]


def link_table(chs):
    """name -> (calls per chain, mean us, max us, workgroup size) over the chains"""
    per = collections.OrderedDict()
    for ch in chs:
        for e in ch:
            per.setdefault((e[2], e[4]), []).append((e[1] - e[0]) / 1e3)
    return {k: (len(v) / max(1, len(chs)), statistics.mean(v), max(v)) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pipelined")
    ap.add_argument("serial", nargs="?")
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    ev = read(a.pipelined)
    bs = batches(ev)[-a.steps:]
    print(f"## Between one batch's last hash kernel and the next batch's first ({len(bs) - 1} intervals, pipelined steps)\n")
    print("| interval | gap µs | hash µs of the batch before | dedup kernels and copies inside the gap (µs inside) |")
    print("|---|---|---|---|")
    gaps = []
    for i in range(len(bs) - 1):
        g0, g1 = bs[i][1], bs[i + 1][0]
        gaps.append((g1 - g0) / 1e3)
        inside = []
        for e in ev:
            if e[1] > g0 and e[0] < g1 and is_chain(e[2]):
                inside.append(f"{e[2]} {(min(e[1], g1) - max(e[0], g0)) / 1e3:.0f}")
        print(f"| {i} | {gaps[-1]:.0f} | {(bs[i][1] - bs[i][0]) / 1e3:.0f} | {', '.join(inside) or '-'} |")
    if gaps:
        print(f"\ngap: mean {statistics.mean(gaps):.0f} µs, median {statistics.median(gaps):.0f} µs, max {max(gaps):.0f} µs; "
              f"hash: mean {statistics.mean((b[1] - b[0]) / 1e3 for b in bs):.0f} µs\n")
    chs = chains(ev, a.steps)
    spans = [(max(e[1] for e in ch) - ch[0][0]) / 1e3 for ch in chs if ch]
    print(f"chain span (k_part_count start to the chain's last kernel end), pipelined: mean {statistics.mean(spans):.0f} µs, "
          f"median {statistics.median(spans):.0f} µs, max {max(spans):.0f} µs\n")
    p = link_table(chs)
    s = {}
    if a.serial:
        sch = chains(read(a.serial), a.steps)
        s = link_table(sch)
        sp = [(max(e[1] for e in ch) - ch[0][0]) / 1e3 for ch in sch if ch]
        print(f"chain span, serial steps: mean {statistics.mean(sp):.0f} µs, median {statistics.median(sp):.0f} µs\n")
    print("## Links of the chain: duration beside the hashing and alone\n")
    print("| link | lanes/wg | per chain | beside hashing mean µs | max µs | serial mean µs | ratio |")
    print("|---|---|---|---|---|---|---|")
    for k, (c, m, mx) in p.items():
        sm = s.get(k, (0, 0.0, 0.0))[1]
        print(f"| `{k[0]}` | {k[1]} | {c:.1f} | {m:.1f} | {mx:.1f} | {sm:.1f} | {m / sm if sm else float('nan'):.1f} |")
    tot_p = sum(c * m for c, m, _ in p.values())
    tot_s = sum(c * m for c, m, _ in s.values())
    print(f"\nsum of the links per chain: {tot_p:.0f} µs beside the hashing, {tot_s:.0f} µs alone")


if __name__ == "__main__":
    main()
