#!/usr/bin/env python
"""Rate of the path-pattern census (pn_census.hip) on a random graph of n nodes and `degree` rows per node.

    python tools/census_rate.py [n=1000000] [degree=16] [walk_len=3] [--repeats 20] [--out FILE]

A call enqueues its levels back to back, so a level is timed as a difference of whole calls, each between device events
on one stream after warm-up calls of every shape, median of --repeats:
    level j (writes its table)        = counts(walk_len=j) - counts(walk_len=j-1)
    last level of labels(walk_len=k)  = labels(walk_len=k) - counts(walk_len=k-1)     (argmax epilogue, no table written)
The bytes are the algorithm's, from shapes: level j reads entries * (4 + 1 + 8 * B^(j-1)) and writes 8 * n * B^j (nothing
for the labels-only last level); entries = 2 * rows.  The formula is an upper bound where less is touched: level 1 reads
no table (C_0 is all ones) and the default symbols (node id & 1) need no byte.  Needs a GPU; there is no fallback.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pathnet_amd import PatternCensus  # noqa: E402

PEAK_HBM = 8.0e12       # bytes/s, MI355X


def median_ms(fn, repeats):
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        del out
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    argv = list(sys.argv[1:])
    repeats, out = 20, None
    for flag in ("--repeats", "--out"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--repeats":
                repeats = int(argv[i + 1])
            else:
                out = argv[i + 1]
            del argv[i:i + 2]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    degree = int(argv[1]) if len(argv) > 1 else 16
    k = int(argv[2]) if len(argv) > 2 else 3
    B = 2
    if not torch.cuda.is_available():
        raise SystemExit("census_rate: needs a GPU (a CPU run says nothing about the device)")
    rng = np.random.default_rng(0)
    u, v = rng.integers(0, n, degree * n).astype(np.int32), rng.integers(0, n, degree * n).astype(np.int32)
    cen = PatternCensus(n, u, v)
    entries = cen.entries
    calls = {("counts", j): (lambda j=j: cen.counts(walk_len=j)) for j in range(1, k + 1)}
    calls[("labels", k)] = lambda: cen.labels(walk_len=k)
    for fn in calls.values():                       # warm-up of every shape: code object, allocator blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {key: median_ms(fn, repeats) for key, fn in calls.items()}
    lines = ["census_rate: %s, n=%d rows=%d entries=%d max_list=%d B=%d walk_len=%d, median of %d (min..max), device events"
             % (torch.cuda.get_device_name(0), n, degree * n, entries, cen.max_list, B, k, repeats)]
    for key in calls:
        lines.append("  %s(walk_len=%d)  %.3f ms (%.3f..%.3f)" % (key[0], key[1], *t[key]))
    rec = {"n": n, "rows": degree * n, "walk_len": k, "repeats": repeats, "levels": []}
    for j in list(range(1, k + 1)) + ["labels"]:
        last = j == "labels"
        lvl = k if last else j
        ms = t[("labels", k) if last else ("counts", lvl)][0] - (t[("counts", lvl - 1)][0] if lvl > 1 else 0.0)
        rd, wr = entries * (4 + 1 + 8 * B ** (lvl - 1)), 0 if last else 8 * n * B ** lvl
        rate = (rd + wr) / (ms * 1e-3) if ms > 0 else float("nan")
        lines.append("  level %d%s  %.3f ms  reads %.1f MB writes %.1f MB  %.2f TB/s = %.0f %% of the %.0f TB/s HBM peak"
                     % (lvl, " (labels only)" if last else "", ms, rd / 1e6, wr / 1e6, rate / 1e12, 100 * rate / PEAK_HBM,
                        PEAK_HBM / 1e12))
        rec["levels"].append({"level": lvl, "labels_only": last, "ms": round(ms, 4), "read_bytes": rd, "write_bytes": wr,
                              "bytes_per_s": rate})
    rec["labels_ms"] = round(t[("labels", k)][0], 4)
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rec))
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
