"""What k-means on the GPU costs against the torch composition, at D = 256, cosine, a fixed number of iterations and one
restart, for (N, K) = (1299, 7), (2708, 7), (8192, 7) and (1 000 000, 1024), on random embeddings made here.  The two legs
start from the SAME centroids (K rows of the input), so that both do the same work:
  kmeans  pathnet_amd.kmeans(x, K, iters=I, init=c0)             (pn_kmeans_run: prepare, then assign / update; nothing read back)
  torch   z = normalize(x); I times: label = (z @ c.T).argmax(1), c = normalize(zeros.index_add_(0, label, z))
                                                                  (what a user writes without it: an [N, K] array per iteration
                                                                   and floating-point atomics for the sums)
and alternate in ONE process, every call between two device events; per leg 3 warm-up calls, then the median of --calls (5 at
a million rows).  Peak memory is torch.cuda.max_memory_allocated over one call of the leg, above what is allocated before it.
A torch leg that does not fit is reported as such and the shape is timed without it.  Also reported: the assignments the
kmeans leg ran before it stood still (the later kernels are no-ops then; the torch leg always runs all I), the share of rows
the two legs label alike, and, alone, one run with k-means++ seeding on the device (K passes over the rows).  Prints one line
per shape and one JSON line.  Needs a GPU: there is no fallback.
   python tools/kmeans_ab.py [--iters 10] [--calls 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 256
SHAPES = ((1299, 7), (2708, 7), (8192, 7), (1000000, 1024))


def torch_kmeans(x, c, iters):
    z = torch.nn.functional.normalize(x, dim=1)
    for t in range(iters):
        label = (z @ c.t()).argmax(dim=1)
        if t + 1 < iters:
            c = torch.nn.functional.normalize(torch.zeros_like(c).index_add_(0, label, z), dim=1)
    return label


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_ab: needs a GPU")
    import pathnet_amd
    from pathnet_amd import cluster
    dev = torch.device("cuda:0")
    lines = ["kmeans_ab: D = %d, cosine, %d iterations, 1 restart, the same starting centroids, median of %d calls (5 at 1e6 rows) "
             "after %d warm-ups, legs alternating" % (D, args.iters, args.calls, args.warmup)]
    recs = []
    for N, K in SHAPES:
        calls = args.calls if N < 1000000 else min(args.calls, 5)
        g = torch.Generator().manual_seed(N + K)
        # K loose groups: a direction per group plus unit noise, so that the iterations have something to move
        x = (2.0 * torch.randn(K, D, generator=g)[torch.randint(0, K, (N,), generator=g)] + torch.randn(N, D, generator=g)).to(dev)
        c0 = torch.nn.functional.normalize(x[torch.randperm(N, generator=g)[:K].to(dev)], dim=1).contiguous()
        legs = {"kmeans": lambda: pathnet_amd.kmeans(x, K, iters=args.iters, init=c0), "torch": lambda: torch_kmeans(x, c0, args.iters)}
        vals, peak, times = {}, {}, {}
        for name, fn in list(legs.items()):
            try:
                for _ in range(args.warmup):
                    vals[name] = fn()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - base
                times[name] = []
            except torch.cuda.OutOfMemoryError:
                del legs[name]
                torch.cuda.empty_cache()
        for _ in range(calls):
            for name, fn in legs.items():
                times[name].append(timed(fn)[0])
        plan = cluster.plan(N, D, K)
        rec = dict(N=N, K=K, D=D, iters=args.iters, workgroups=plan["workgroups"], assignments=int(vals["kmeans"].iterations))
        text = []
        for name in ("kmeans", "torch"):
            if name not in legs:
                text.append("%s does not fit" % name)
                continue
            t = np.asarray(times[name])
            rec[name] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()),
                             peak_mib=peak[name] / 2.0 ** 20)
            text.append("%s %9.3f ms (min %.3f max %.3f) peak %8.1f MiB" % (name, rec[name]["median_ms"], rec[name]["min_ms"],
                                                                          rec[name]["max_ms"], rec[name]["peak_mib"]))
        tail = ""
        if len(legs) == 2:
            rec["kmeans_over_torch"] = rec["kmeans"]["median_ms"] / rec["torch"]["median_ms"]
            rec["same_labels"] = float((vals["kmeans"].label == vals["torch"]).double().mean())
            tail = " | kmeans / torch time %.2f, same labels %.4f" % (rec["kmeans_over_torch"], rec["same_labels"])
        seeded = [timed(lambda: pathnet_amd.kmeans(x, K, iters=args.iters))[0] for _ in range(3)]
        rec["seeded_ms"] = float(np.median(seeded))
        recs.append(rec)
        lines.append("N %8d K %4d (%5d workgroups, %2d assignments): %s%s | with k-means++ %.3f ms"
                     % (N, K, plan["workgroups"], rec["assignments"], " | ".join(text), tail, rec["seeded_ms"]))
        del x, c0, vals
        torch.cuda.empty_cache()
    lines.append(json.dumps(recs))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
