"""What the tiled exact k-NN costs against the torch composition, at D = 256, k = 20, cosine, for (Sq, N) = (1299, 2708),
(2708, 2708), (8192, 8192) and (2708, 1 000 000), on random embeddings made here.  The two legs:
  knn     pathnet_amd.knn(q, x, 20)                                        (pn_knn_search: prep, search, merge)
  torch   torch.topk(F.normalize(q) @ F.normalize(x).T, 20)                (what a user writes without it: an [Sq, N] array)
alternate in ONE process, every call between two device events; per leg 3 warm-up calls, then the median of 20.  Peak memory is
torch.cuda.max_memory_allocated over one call of the leg, above what is allocated before it.  A torch leg that does not fit
is reported as such and the shape is timed without it.  Also reported: the splits the library chose, and how many of the
Sq x k neighbours the two legs agree on (they differ where scores tie or differ in the last bits).  Prints one line per shape
and one JSON line.  Needs a GPU: there is no fallback.
--sweep adds the knn leg alone at 8192 x 8192 for D in (256, 16) and k in (1, 20, 64): what the tile and the selection cost.
   python tools/knn_ab.py [--calls 20] [--warmup 3] [--sweep] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, K = 256, 20
SHAPES = ((1299, 2708), (2708, 2708), (8192, 8192), (2708, 1000000))


def torch_knn(q, x, k):
    s = torch.nn.functional.normalize(q, dim=1) @ torch.nn.functional.normalize(x, dim=1).t()
    return torch.topk(s, k, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="also time knn(x, x, k) at 8192 x 8192 over D and k")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_ab: needs a GPU")
    import pathnet_amd
    from pathnet_amd import neighbours
    dev = torch.device("cuda:0")
    lines = ["knn_ab: D = %d, k = %d, cosine, median of %d calls after %d warm-ups, legs alternating" % (D, K, args.calls, args.warmup)]
    recs = []
    for Sq, N in SHAPES:
        g = torch.Generator().manual_seed(Sq + N)
        x = (torch.randn(D, generator=g) + torch.randn(N, D, generator=g)).to(dev)
        q = (torch.randn(D, generator=g) + torch.randn(Sq, D, generator=g)).to(dev)
        legs = {"knn": lambda: pathnet_amd.knn(q, x, K).index, "torch": lambda: torch_knn(q, x, K).indices}
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
        for _ in range(args.calls):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        plan = neighbours.plan(Sq, N, D, K)
        rec = dict(Sq=Sq, N=N, D=D, k=K, splits=plan["splits"], workgroups=plan["workgroups"])
        text = []
        for name in ("knn", "torch"):
            if name not in legs:
                text.append("%s does not fit" % name)
                continue
            t = np.asarray(times[name])
            rec[name] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()),
                             peak_mib=peak[name] / 2.0 ** 20)
            text.append("%s %9.3f ms (min %.3f max %.3f) peak %9.1f MiB" % (name, rec[name]["median_ms"], rec[name]["min_ms"],
                                                                           rec[name]["max_ms"], rec[name]["peak_mib"]))
        tail = ""
        if len(legs) == 2:
            rec["knn_over_torch"] = rec["knn"]["median_ms"] / rec["torch"]["median_ms"]
            rec["same_neighbours"] = float((vals["knn"] == vals["torch"]).double().mean())
            tail = " | knn / torch time %.2f, same neighbours %.4f" % (rec["knn_over_torch"], rec["same_neighbours"])
        recs.append(rec)
        lines.append("Sq %5d N %8d splits %3d (%d workgroups): %s%s" % (Sq, N, plan["splits"], plan["workgroups"],
                                                                        " | ".join(text), tail))
        del x, q, vals
        torch.cuda.empty_cache()
    if args.sweep:
        lines.append("the call at other k and D: median of %d calls after %d warm-ups, knn(x, x, k), cosine" % (args.calls, args.warmup))
        g = torch.Generator().manual_seed(1)
        for d in (256, 16):
            x = (torch.randn(d, generator=g) + torch.randn(8192, d, generator=g)).to(dev)
            for k in (1, 20, 64):
                for _ in range(args.warmup):
                    pathnet_amd.knn(x, x, k)
                t = []
                for _ in range(args.calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    pathnet_amd.knn(x, x, k)
                    e1.record()
                    e1.synchronize()
                    t.append(e0.elapsed_time(e1))
                recs.append(dict(Sq=8192, N=8192, D=d, k=k, knn=dict(median_ms=float(np.median(t)), min_ms=min(t))))
                lines.append("8192 x 8192 D %3d k %2d: %.3f ms (min %.3f)" % (d, k, float(np.median(t)), min(t)))
    lines.append(json.dumps(recs))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
